// Stand-alone self-test of store/csrc/stored_core.hpp: the daemon's
// connection protocol over socket pairs. No Python, no GPU: build with
// -fsanitize=address,undefined and with -fsanitize=thread and run directly
// (tests/test_native_selftests.py does).
//
// CRUD and patch semantics are the Python parity battery's business
// (tests/test_native_store.py). The cases here are the ones a Python client
// reaches only by luck of timing: a frame the socket would not take, a
// response while such a frame waits, the outbox cap, a connection torn down
// under a flushing writer, and the subscribe response's place on the wire.
//
// Every served connection is one reader_loop() thread (plus the writer it
// starts) on one end of a socket pair; the test is the peer on the other end
// and keeps the Conn to look at.

#include <sys/socket.h>
#include <sys/time.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <memory>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "stored_core.hpp"

using stored::Conn;
using stored::Store;
using stored::Value;

#define FAIL(...)                                             \
  do {                                                        \
    std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
    std::fprintf(stderr, __VA_ARGS__);                        \
    std::fprintf(stderr, "\n");                               \
    std::exit(1);                                             \
  } while (0)

#define CHECK(cond)            \
  do {                         \
    if (!(cond)) FAIL(#cond);  \
  } while (0)

// ---- building requests -----------------------------------------------------

static Value S(const std::string& s) { return Value::str(s); }
static Value I(int64_t i) { return Value::integer(i); }

static Value map(std::initializer_list<std::pair<const char*, Value>> kv) {
  Value m = Value::map();
  for (const auto& e : kv) m.setkey(e.first, e.second);
  return m;
}

static Value arr(std::initializer_list<Value> items) {
  Value a = Value::arr();
  for (const auto& v : items) a.a->push_back(v);
  return a;
}

static Value thing(const std::string& name, Value spec) {
  return map({{"kind", S("Thing")},
              {"metadata", map({{"name", S(name)}, {"namespace", S("")}})},
              {"spec", std::move(spec)}});
}

static Value create_req(const std::string& name, Value spec) {
  return map({{"verb", S("create")}, {"quiet", Value::boolean(true)},
              {"obj", thing(name, std::move(spec))}});
}

// set spec.i of Thing `name`
static Value patch_req(const std::string& name, int64_t i) {
  Value op = map({{"op", S("set")}, {"path", arr({S("spec"), S("i")})},
                  {"value", I(i)}});
  return map({{"verb", S("patch")}, {"kind", S("Thing")}, {"name", S(name)},
              {"namespace", S("")}, {"quiet", Value::boolean(true)},
              {"ops", arr({op})}});
}

static Value watch_req(bool replay) {
  return map({{"verb", S("watch")}, {"kind", S("Thing")},
              {"replay", Value::boolean(replay)}});
}

static bool is_ok(const Value& resp) {
  const Value* ok = resp.find("ok");
  return ok && ok->truthy();
}

// an event frame's resourceVersion; -1 for a frame that is no event
static int64_t event_rv(const Value& frame, std::string* type = nullptr,
                        std::string* name = nullptr) {
  const Value* ev = frame.find("event");
  if (!frame.find("watch_id") || !ev || !ev->is_arr() || ev->a->size() != 2)
    return -1;
  const Value* md = (*ev->a)[1].find("metadata");
  CHECK(md);
  if (type) *type = (*ev->a)[0].s;
  if (name) *name = md->str_or("name", "");
  return std::stoll(md->str_or("resourceVersion", ""));
}

// ---- one served connection and its peer ------------------------------------

struct Peer {
  int fd = -1;                 // the test's end
  std::shared_ptr<Conn> conn;  // the daemon's end
  std::thread served;
  int64_t next_id = 0;

  // small_sndbuf: the daemon's socket takes as little as the kernel allows
  explicit Peer(Store& store, bool small_sndbuf = false) {
    int fds[2];
    CHECK(::socketpair(AF_UNIX, SOCK_STREAM, 0, fds) == 0);
    fd = fds[0];
    if (small_sndbuf) {
      int one = 1;  // raised to the kernel's minimum
      CHECK(::setsockopt(fds[1], SOL_SOCKET, SO_SNDBUF, &one, sizeof(one)) == 0);
    }
    // a daemon that stops answering fails the test instead of hanging it
    timeval tv{30, 0};
    CHECK(::setsockopt(fd, SOL_SOCKET, SO_RCVTIMEO, &tv, sizeof(tv)) == 0);
    conn = std::make_shared<Conn>();
    conn->fd = fds[1];
    served = std::thread(stored::reader_loop, std::ref(store), conn);
  }

  Peer(const Peer&) = delete;
  Peer& operator=(const Peer&) = delete;

  ~Peer() { hang_up(); }

  // close our end; the daemon's threads for this connection end
  void hang_up() {
    if (fd >= 0) ::close(fd);
    fd = -1;
    if (served.joinable()) served.join();
  }

  int64_t send(Value req) {
    req.setkey("id", I(++next_id));
    std::string payload;
    stored::pack(req, payload);
    std::string bytes = wire::frame(payload);
    CHECK(Conn::send_all(fd, bytes.data(), bytes.size()));
    return next_id;
  }

  bool recv_exact(char* p, size_t n, bool eof_ok) {
    size_t got = 0;
    while (got < n) {
      ssize_t r = ::recv(fd, p + got, n - got, 0);
      if (r < 0 && errno == EINTR) continue;
      if (r < 0) FAIL("recv: %s", std::strerror(errno));
      if (r == 0) {
        if (!eof_ok || got != 0) FAIL("connection ended inside a frame");
        return false;
      }
      got += static_cast<size_t>(r);
    }
    return true;
  }

  // one frame, decoded; false: the daemon closed the connection (between
  // frames — an end inside a frame fails the test)
  bool read(Value& out) {
    char hdr[wire::kHeaderLen];
    if (!recv_exact(hdr, sizeof(hdr), true)) return false;
    uint32_t len = wire::frame_len(hdr);
    CHECK(len <= wire::kMaxFrame);
    std::string buf(len, '\0');
    recv_exact(&buf[0], len, false);
    out = stored::unpack(buf);  // throws on bytes that are no msgpack
    CHECK(out.is_map());
    return true;
  }

  // request + its response, on a connection that has no watch
  Value call(Value req) {
    int64_t id = send(std::move(req));
    Value resp;
    CHECK(read(resp));
    const Value* rid = resp.find("id");
    CHECK(rid && rid->t == Value::T::Int && rid->i == id);
    return resp;
  }

  // subscribe to Thing; the response must be the very next frame
  int64_t subscribe(bool replay, int64_t* rev = nullptr) {
    int64_t id = send(watch_req(replay));
    Value resp;
    CHECK(read(resp));
    const Value* rid = resp.find("id");
    CHECK(rid && rid->i == id && is_ok(resp));
    const Value* result = resp.find("result");
    CHECK(result && result->find("watch_id") && result->find("rev"));
    if (rev) *rev = result->find("rev")->i;
    return result->find("watch_id")->i;
  }
};

// read `n` events from `w`: consecutive resourceVersions from `first_rv` on
static void expect_consecutive(Peer& w, int64_t first_rv, int n) {
  for (int k = 0; k < n; ++k) {
    Value f;
    CHECK(w.read(f));
    int64_t rv = event_rv(f);
    if (rv != first_rv + k)
      FAIL("event %d of %d: resourceVersion %lld, expected %lld", k, n,
           static_cast<long long>(rv), static_cast<long long>(first_rv + k));
  }
}

// a thread that patches Thing `name` over a connection of its own, `count`
// times, or until told to stop (count < 0; at least `at_least` times)
struct Mutator {
  Peer peer;
  std::atomic<bool> stop{false};
  std::thread th;
  Mutator(Store& store, const std::string& name, int count, int at_least = 0)
      : peer(store) {
    th = std::thread([this, name, count, at_least] {
      for (int i = 0; count >= 0 ? i < count : (i < at_least || !stop.load());
           ++i)
        CHECK(is_ok(peer.call(patch_req(name, i))));
    });
  }
  void join() {
    stop.store(true);
    th.join();
  }
};

// ---- cases -----------------------------------------------------------------

// a. A watcher that does not read: its socket fills, a flush leaves a tail.
// Then a response has to get past that tail without landing inside a frame.
static void test_tail_then_response() {
  constexpr int kBound = 4096;
  static_assert(kBound < static_cast<int>(Conn::kMaxOutbox), "below the cap");
  Store store;
  Peer writer(store);
  CHECK(is_ok(writer.call(create_req(
      "hot", map({{"i", I(0)}, {"pad", S(std::string(1000, 'p'))}})))));
  Peer watcher(store, /*small_sndbuf=*/true);
  int64_t rev = 0;
  watcher.subscribe(false, &rev);
  int sent = 0;
  while (!watcher.conn->tail_pending.load()) {
    if (sent == kBound) FAIL("partial send never reached");
    CHECK(is_ok(writer.call(patch_req("hot", ++sent))));
  }
  int64_t ping_id = watcher.send(map({{"verb", S("ping")}}));
  int events = 0, pongs = 0;
  while (events < sent || pongs < 1) {
    Value f;
    CHECK(watcher.read(f));
    int64_t rv = event_rv(f);
    if (rv >= 0) {
      CHECK(rv == rev + 1 + events);  // in order, none missing
      ++events;
    } else {
      const Value* rid = f.find("id");
      const Value* result = f.find("result");
      CHECK(rid && rid->i == ping_id && is_ok(f));
      CHECK(result && result->is_str() && result->s == "pong");
      ++pongs;
    }
  }
  // nothing follows: our half-close ends the connection, and what the
  // daemon had left to say would come before its end
  CHECK(::shutdown(watcher.fd, SHUT_WR) == 0);
  Value extra;
  CHECK(!watcher.read(extra));
  CHECK(events == sent && pongs == 1);
}

// b. Four connections patch one object, two watchers read: each sees every
// event, in resourceVersion order.
static void test_order_under_contention() {
  constexpr int kMutators = 4, kPatches = 200, kWatchers = 2;
  Store store;
  Peer setup(store);
  CHECK(is_ok(setup.call(create_req("hot", map({{"i", I(0)}})))));
  std::vector<std::unique_ptr<Peer>> watchers;
  std::vector<std::thread> readers;
  for (int w = 0; w < kWatchers; ++w) {
    watchers.emplace_back(new Peer(store));
    int64_t rev = 0;
    watchers.back()->subscribe(false, &rev);
    CHECK(rev == 1);
    Peer* p = watchers.back().get();
    readers.emplace_back(
        [p, rev] { expect_consecutive(*p, rev + 1, kMutators * kPatches); });
  }
  std::vector<std::unique_ptr<Mutator>> mutators;
  for (int m = 0; m < kMutators; ++m)
    mutators.emplace_back(new Mutator(store, "hot", kPatches));
  for (auto& m : mutators) m->join();
  for (auto& r : readers) r.join();
}

// c. A watcher that never reads is cut off at the outbox cap, and the
// connection that made the events is none the worse for it. The cap is
// 65536 events whatever their size; making that many takes about 4 s under
// AddressSanitizer and 17 s under ThreadSanitizer (8 CPUs), so the
// ThreadSanitizer build leaves this case to the other build and to
// tests/test_stored_inline_events.py.
#if defined(__SANITIZE_THREAD__)
#define STORED_SELFTEST_CAP 0
#elif defined(__has_feature)
#if __has_feature(thread_sanitizer)
#define STORED_SELFTEST_CAP 0
#endif
#endif
#ifndef STORED_SELFTEST_CAP
#define STORED_SELFTEST_CAP 1
#endif

#if STORED_SELFTEST_CAP
static void test_cap() {
  constexpr int kBatch = 512;
  constexpr int kMutations = static_cast<int>(Conn::kMaxOutbox) + 8 * kBatch;
  Store store;
  Peer writer(store);
  CHECK(is_ok(writer.call(create_req("hot", map({{"i", I(0)}})))));
  Peer watcher(store, /*small_sndbuf=*/true);
  watcher.subscribe(false);
  for (int sent = 0; sent < kMutations; sent += kBatch) {
    Value reqs = Value::arr();
    for (int k = 0; k < kBatch; ++k) reqs.a->push_back(patch_req("hot", sent + k));
    Value resp = writer.call(map({{"verb", S("batch")},
                                  {"quiet", Value::boolean(true)},
                                  {"requests", std::move(reqs)}}));
    CHECK(is_ok(resp) && resp.find("result")->a->size() == kBatch);
  }
  Value pong = writer.call(map({{"verb", S("ping")}}));
  CHECK(is_ok(pong) && pong.find("result")->s == "pong");
  int received = 0;
  for (Value f; watcher.read(f);) {
    CHECK(event_rv(f) == 2 + received);
    ++received;
  }
  if (received >= kMutations - static_cast<int>(Conn::kMaxOutbox) / 2)
    FAIL("%d of %d events were served: the watcher was not cut off at the cap",
         received, kMutations);
}
#endif

// d. Connections that subscribe with replay and hang up without reading,
// while three threads keep mutating what they subscribed to: their Conns go
// away under threads that may be flushing to them.
static void test_teardown_under_flush() {
  constexpr int kObjects = 20, kChurn = 30;
  Store store;
  Peer setup(store);
  for (int i = 0; i < kObjects; ++i)
    CHECK(is_ok(setup.call(create_req("o" + std::to_string(i), map({{"i", I(0)}})))));
  std::vector<std::unique_ptr<Mutator>> mutators;
  for (int m = 0; m < 3; ++m)
    mutators.emplace_back(new Mutator(store, "o" + std::to_string(m), -1, 100));
  for (int c = 0; c < kChurn; ++c) {
    Peer p(store);
    p.send(watch_req(true));
    if (c % 2) {  // every other one stays until events are on their way
      Value first;
      CHECK(p.read(first) && is_ok(first));
    }
    p.hang_up();  // joins the connection's reader and writer
  }
  for (auto& m : mutators) m->join();
  Value listed = setup.call(map({{"verb", S("list")}, {"kind", S("Thing")}}));
  CHECK(is_ok(listed) && listed.find("result")->a->size() == kObjects);
}

// e. With a writer mutating a matching object all the while, a fresh
// connection's first frame is the subscribe response; the replayed ADDED
// events follow in key order, live events after them and never older.
static void test_subscribe_response_first() {
  constexpr int kObjects = 20, kRounds = 10;
  Store store;
  Peer setup(store);
  std::vector<std::string> names;
  for (int i = 0; i < kObjects; ++i) {
    names.push_back(std::string("o") + (i < 10 ? "0" : "") + std::to_string(i));
    CHECK(is_ok(setup.call(create_req(names.back(), map({{"i", I(0)}})))));
  }
  Mutator churn(store, "o00", -1, 100);
  for (int r = 0; r < kRounds; ++r) {
    Peer p(store);
    int64_t rev = 0;
    int64_t wid = p.subscribe(true, &rev);  // checks: the first frame
    std::string type, name;
    for (int i = 0; i < kObjects; ++i) {
      Value f;
      CHECK(p.read(f));
      CHECK(event_rv(f, &type, &name) >= 0 && f.find("watch_id")->i == wid);
      CHECK(type == "ADDED" && name == names[i]);
    }
    Value f;
    CHECK(p.read(f));
    CHECK(event_rv(f, &type, &name) > rev && type == "MODIFIED");
  }
  churn.join();
}

static void run(const char* name, void (*test)()) {
  auto t0 = std::chrono::steady_clock::now();
  test();
  std::chrono::duration<double> dt = std::chrono::steady_clock::now() - t0;
  std::printf("%-26s %6.2f s\n", name, dt.count());
}

int main() {
  try {
    run("tail then response", test_tail_then_response);
    run("order under contention", test_order_under_contention);
#if STORED_SELFTEST_CAP
    run("cap", test_cap);
#endif
    run("teardown under flush", test_teardown_under_flush);
    run("subscribe response first", test_subscribe_response_first);
  } catch (const std::exception& e) {
    FAIL("exception: %s", e.what());
  }
  std::puts("stored selftest OK");
  return 0;
}
