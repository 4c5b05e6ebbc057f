// Stand-alone self-test of store/csrc/netwire_core.hpp over a socketpair.
// No Python, no GPU: build with -fsanitize=address,undefined and with
// -fsanitize=thread and run directly (tests/test_native_selftests.py does).
//
// The test plays the server on one end of the pair; a Wire owns the other.

#include <sys/ioctl.h>
#include <sys/socket.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <sched.h>
#include <string>
#include <thread>
#include <vector>

#include "netwire_core.hpp"

using netwire::CallStatus;
using netwire::FrameKind;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

// ---- a few msgpack encoders, enough for the protocol's envelope -----------

static std::string mp_str(const std::string& s) {
  std::string o;
  if (s.size() < 32) {
    o.push_back(static_cast<char>(0xa0 | s.size()));
  } else if (s.size() < 256) {
    o.push_back(static_cast<char>(0xd9));
    o.push_back(static_cast<char>(s.size()));
  } else if (s.size() < 65536) {
    o.push_back(static_cast<char>(0xda));
    o.push_back(static_cast<char>(s.size() >> 8));
    o.push_back(static_cast<char>(s.size()));
  } else {
    o.push_back(static_cast<char>(0xdb));
    for (int sh = 24; sh >= 0; sh -= 8)
      o.push_back(static_cast<char>(s.size() >> sh));
  }
  return o + s;
}

static std::string mp_uint(uint64_t v) {
  std::string o;
  if (v < 128) {
    o.push_back(static_cast<char>(v));
  } else if (v < 256) {
    o.push_back(static_cast<char>(0xcc));
    o.push_back(static_cast<char>(v));
  } else if (v < 65536) {
    o.push_back(static_cast<char>(0xcd));
    o.push_back(static_cast<char>(v >> 8));
    o.push_back(static_cast<char>(v));
  } else {
    o.push_back(static_cast<char>(0xce));
    for (int sh = 24; sh >= 0; sh -= 8) o.push_back(static_cast<char>(v >> sh));
  }
  return o;
}

static const std::string kTrue(1, static_cast<char>(0xc3));

// {"id": id, "ok": true, "result": body}; id_last: the daemon's and the
// Python server's key orders differ, so both are exercised
static std::string response(uint64_t id, const std::string& body, bool id_last) {
  std::string idkv = mp_str("id") + mp_uint(id);
  std::string rest = mp_str("ok") + kTrue + mp_str("result") + mp_str(body);
  std::string o(1, static_cast<char>(0x83));
  return o + (id_last ? rest + idkv : idkv + rest);
}

// {"watch_id": wid, "event": ["MODIFIED", {"seq": seq, "id": 7}]} — the
// nested "id" must not make it a response
static std::string event(uint64_t wid, uint64_t seq, bool wid_last) {
  std::string widkv = mp_str("watch_id") + mp_uint(wid);
  std::string obj(1, static_cast<char>(0x82));
  obj += mp_str("seq") + mp_uint(seq) + mp_str("id") + mp_uint(7);
  std::string ev = mp_str("event") + std::string(1, static_cast<char>(0x92)) +
                   mp_str("MODIFIED") + obj;
  std::string o(1, static_cast<char>(0x82));
  return o + (wid_last ? ev + widkv : widkv + ev);
}

static std::string frame(const std::string& payload) {
  std::string o;
  uint32_t n = static_cast<uint32_t>(payload.size());
  for (int sh = 24; sh >= 0; sh -= 8) o.push_back(static_cast<char>(n >> sh));
  return o + payload;
}

// ---- harness ---------------------------------------------------------------

struct Harness {
  int cli = -1, srv = -1;
  std::shared_ptr<netwire::Wire> wire;
  std::mutex mu;
  std::vector<std::string> frames;  // what on_frame saw, in order
  int closed_calls = 0;
  bool frames_after_close = false;
  std::atomic<bool> closed_returned{false};

  Harness() {
    int fds[2];
    CHECK(::socketpair(AF_UNIX, SOCK_STREAM, 0, fds) == 0);
    cli = fds[0];
    srv = fds[1];
    wire = netwire::Wire::create(
        cli,
        [this](const char* p, size_t n) {
          std::lock_guard<std::mutex> g(mu);
          if (closed_returned.load()) frames_after_close = true;
          frames.emplace_back(p, n);
        },
        [this] {
          std::lock_guard<std::mutex> g(mu);
          if (closed_returned.load()) frames_after_close = true;
          ++closed_calls;
        });
  }

  ~Harness() {
    wire->close();
    wire.reset();
    if (srv >= 0) ::close(srv);
    ::close(cli);  // the owner closes the borrowed fd, after close()
  }

  void srv_write(const char* p, size_t n) {
    while (n > 0) {
      ssize_t r = ::send(srv, p, n, MSG_NOSIGNAL);
      CHECK(r > 0);
      p += r;
      n -= static_cast<size_t>(r);
    }
  }
  void srv_write(const std::string& s) { srv_write(s.data(), s.size()); }

  // until the wire's reader has taken every byte written so far: makes a
  // split in the byte stream a split between two recv()s
  void drain() {
    for (;;) {
      int pending = 0;
      CHECK(::ioctl(cli, FIONREAD, &pending) == 0);
      if (pending == 0) return;
      sched_yield();
    }
  }

  // one request frame, as the server reads it: proves the caller's slot is
  // registered (call() registers before it sends)
  std::string srv_read_frame() {
    unsigned char h[4];
    size_t got = 0;
    while (got < 4) {
      ssize_t r = ::recv(srv, h + got, 4 - got, 0);
      CHECK(r > 0);
      got += static_cast<size_t>(r);
    }
    size_t n = (h[0] << 24) | (h[1] << 16) | (h[2] << 8) | h[3];
    std::string body(n, '\0');
    got = 0;
    while (got < n) {
      ssize_t r = ::recv(srv, &body[got], n - got, 0);
      CHECK(r > 0);
      got += static_cast<size_t>(r);
    }
    return body;
  }

  size_t frame_count() {
    std::lock_guard<std::mutex> g(mu);
    return frames.size();
  }
};

struct Caller {
  std::thread th;
  CallStatus st = CallStatus::Ok;
  std::string out;
  Caller(Harness& h, int64_t rid, double timeout_s = 30.0) {
    th = std::thread([this, &h, rid, timeout_s] {
      std::string req = frame(mp_str("req"));
      st = h.wire->call(rid, req.data(), req.size(), timeout_s, out);
    });
  }
  void join() { th.join(); }
};

// ---- cases -----------------------------------------------------------------

static void test_classify() {
  auto kind = [](const std::string& s) {
    return netwire::classify(s.data(), s.size());
  };
  for (bool last : {false, true}) {
    auto c = kind(response(5, "x", last));
    CHECK(c.kind == FrameKind::Response && c.id == 5);
    c = kind(response(300, "x", last));  // uint16 id
    CHECK(c.kind == FrameKind::Response && c.id == 300);
    c = kind(response(70000, std::string(70000, 'r'), last));  // uint32, str32
    CHECK(c.kind == FrameKind::Response && c.id == 70000);
    CHECK(kind(event(3, 9, last)).kind == FrameKind::Event);
  }
  // map16 header
  std::string m16;
  m16.push_back(static_cast<char>(0xde));
  m16.push_back(0);
  m16.push_back(1);
  m16 += mp_str("id") + mp_uint(4);
  CHECK(kind(m16).kind == FrameKind::Response && kind(m16).id == 4);
  // no id, a string id, not a map, empty, truncated at every length
  std::string noid(1, static_cast<char>(0x81));
  noid += mp_str("ok") + kTrue;
  CHECK(kind(noid).kind == FrameKind::Other);
  std::string strid(1, static_cast<char>(0x81));
  strid += mp_str("id") + mp_str("seven");
  CHECK(kind(strid).kind == FrameKind::Other);
  CHECK(kind(mp_str("hello")).kind == FrameKind::Other);
  CHECK(kind("").kind == FrameKind::Other);
  std::string whole = response(9, "abcdefgh", true);
  for (size_t n = 0; n < whole.size(); ++n)
    CHECK(netwire::classify(whole.data(), n).kind == FrameKind::Other);
}

// the byte stream used by the split tests: events and responses interleaved,
// both key orders
static std::string small_stream(std::vector<std::string>& events) {
  std::string s;
  events = {event(1, 0, false), event(1, 1, true), event(2, 2, false)};
  s += frame(events[0]);
  s += frame(response(1, "one", false));
  s += frame(events[1]);
  s += frame(response(2, "two", true));
  s += frame(events[2]);
  return s;
}

static void expect_small_stream(Harness& h, Caller& c1, Caller& c2,
                                const std::vector<std::string>& events) {
  c1.join();
  c2.join();
  CHECK(c1.st == CallStatus::Ok && c2.st == CallStatus::Ok);
  CHECK(c1.out == response(1, "one", false));
  CHECK(c2.out == response(2, "two", true));
  while (h.frame_count() < events.size()) sched_yield();
  std::lock_guard<std::mutex> g(h.mu);
  CHECK(h.frames == events);
}

static void test_split_at_every_boundary() {
  std::vector<std::string> events;
  std::string s = small_stream(events);
  for (size_t k = 0; k <= s.size(); ++k) {
    Harness h;
    Caller c1(h, 1), c2(h, 2);
    h.srv_read_frame();
    h.srv_read_frame();
    h.srv_write(s.data(), k);
    h.drain();
    h.srv_write(s.data() + k, s.size() - k);
    expect_small_stream(h, c1, c2, events);
  }
}

static void test_byte_by_byte() {
  std::vector<std::string> events;
  std::string s = small_stream(events);
  Harness h;
  Caller c1(h, 1), c2(h, 2);
  h.srv_read_frame();
  h.srv_read_frame();
  for (char ch : s) {
    h.srv_write(&ch, 1);
    h.drain();
  }
  expect_small_stream(h, c1, c2, events);
}

static void test_interleaved_order_and_demux() {
  constexpr int kCallers = 8, kEvents = 400;
  Harness h;
  std::vector<std::unique_ptr<Caller>> callers;
  for (int i = 0; i < kCallers; ++i)
    callers.emplace_back(new Caller(h, 100 + i));
  for (int i = 0; i < kCallers; ++i) h.srv_read_frame();
  std::string s;
  std::vector<std::string> events;
  for (int e = 0; e < kEvents; ++e) {
    events.push_back(event(1 + e % 3, e, e % 2 == 1));
    s += frame(events.back());
    if (e % (kEvents / kCallers) == 7) {
      // answered in REVERSE order of registration
      int i = kCallers - 1 - e / (kEvents / kCallers);
      s += frame(response(100 + i, "r" + std::to_string(i), e % 4 < 2));
    }
  }
  h.srv_write(s);
  for (int i = 0; i < kCallers; ++i) {
    callers[i]->join();
    CHECK(callers[i]->st == CallStatus::Ok);
    bool a = callers[i]->out == response(100 + i, "r" + std::to_string(i), false);
    bool b = callers[i]->out == response(100 + i, "r" + std::to_string(i), true);
    CHECK(a || b);
  }
  while (h.frame_count() < events.size()) sched_yield();
  std::lock_guard<std::mutex> g(h.mu);
  CHECK(h.frames == events);
}

static void test_large_frame() {
  Harness h;
  Caller c(h, 1);
  h.srv_read_frame();
  std::string big = response(1, std::string(300000, 'z'), true);
  std::string s = frame(event(1, 0, false)) + frame(big) +
                  frame(event(1, 1, false));
  for (size_t off = 0; off < s.size(); off += 7001) {
    h.srv_write(s.data() + off, std::min<size_t>(7001, s.size() - off));
    h.drain();
  }
  c.join();
  CHECK(c.st == CallStatus::Ok && c.out == big);
  while (h.frame_count() < 2) sched_yield();
}

static void test_peer_close_fails_pending() {
  Harness h;
  Caller c1(h, 1), c2(h, 2), c3(h, 3);
  for (int i = 0; i < 3; ++i) h.srv_read_frame();
  ::close(h.srv);
  h.srv = -1;
  c1.join();
  c2.join();
  c3.join();
  CHECK(c1.st == CallStatus::Lost && c2.st == CallStatus::Lost &&
        c3.st == CallStatus::Lost);
  while (h.wire->alive()) sched_yield();
  {
    std::lock_guard<std::mutex> g(h.mu);
    CHECK(h.closed_calls == 1);
  }
  Caller late(h, 4);  // a call on a dead wire fails at once
  late.join();
  CHECK(late.st == CallStatus::Lost);
}

static void test_oversized_frame_closes() {
  Harness h;
  Caller c(h, 1);
  h.srv_read_frame();
  const unsigned char hdr[4] = {0x04, 0x00, 0x00, 0x01};  // 64 MiB + 1
  h.srv_write(reinterpret_cast<const char*>(hdr), 4);
  c.join();
  CHECK(c.st == CallStatus::Lost);
  char b;
  CHECK(::recv(h.srv, &b, 1, 0) == 0);  // the wire shut the connection
  while (h.wire->alive()) sched_yield();
  std::lock_guard<std::mutex> g(h.mu);
  CHECK(h.closed_calls == 1 && h.frames.empty());
}

static void test_close_with_call_in_flight() {
  Harness h;
  Caller c(h, 1);
  h.srv_read_frame();
  h.wire->close();
  h.closed_returned.store(true);
  c.join();
  CHECK(c.st == CallStatus::Lost);
  CHECK(!h.wire->alive());  // the reader is joined
  h.wire->close();          // idempotent
  // anything the peer still sends goes nowhere
  std::string ev = frame(event(1, 0, false));
  (void)::send(h.srv, ev.data(), ev.size(), MSG_NOSIGNAL);
  std::string req = frame(mp_str("x"));
  CHECK(!h.wire->send(req.data(), req.size()));
  std::lock_guard<std::mutex> g(h.mu);
  CHECK(!h.frames_after_close && h.closed_calls == 0 && h.frames.empty());
}

static void test_close_from_callback() {
  int fds[2];
  CHECK(::socketpair(AF_UNIX, SOCK_STREAM, 0, fds) == 0);
  std::shared_ptr<netwire::Wire> wire;
  std::mutex mu;
  std::atomic<int> frames{0};
  std::atomic<bool> done{false};
  {
    std::lock_guard<std::mutex> g(mu);
    wire = netwire::Wire::create(
        fds[0],
        [&](const char*, size_t) {
          std::shared_ptr<netwire::Wire> w;
          {
            std::lock_guard<std::mutex> g2(mu);
            w = wire;
          }
          ++frames;
          w->close();  // on the reader itself: must not join itself
          done.store(true);
        },
        [] { CHECK(false && "on_closed after close()"); });
  }
  std::string s = frame(event(1, 0, false)) + frame(event(1, 1, false));
  CHECK(::send(fds[1], s.data(), s.size(), MSG_NOSIGNAL) ==
        static_cast<ssize_t>(s.size()));
  while (!done.load()) sched_yield();
  wire->close();  // from outside: waits for the reader to be gone
  CHECK(!wire->alive());
  CHECK(frames.load() == 1);  // the second event fired no callback
  wire.reset();
  ::close(fds[0]);
  ::close(fds[1]);
}

static void test_timeout_then_late_response() {
  Harness h;
  Caller c(h, 1, 0.05);
  h.srv_read_frame();
  c.join();
  CHECK(c.st == CallStatus::Timeout);
  h.srv_write(frame(response(1, "late", false)));  // dropped: nobody waits
  Caller c2(h, 2);
  h.srv_read_frame();
  h.srv_write(frame(response(2, "ok", false)));
  c2.join();
  CHECK(c2.st == CallStatus::Ok && c2.out == response(2, "ok", false));
}

int main() {
  test_classify();
  test_split_at_every_boundary();
  test_byte_by_byte();
  test_interleaved_order_and_demux();
  test_large_frame();
  test_peer_close_fails_pending();
  test_oversized_frame_closes();
  test_close_with_call_in_flight();
  test_close_from_callback();
  test_timeout_then_late_response();
  std::puts("netwire selftest OK");
  return 0;
}
