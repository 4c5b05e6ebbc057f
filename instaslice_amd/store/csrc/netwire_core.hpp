// netwire: the client side of the store wire, off the Python GIL.
//
// One connection of store/netstore.py's protocol (4-byte big-endian length +
// one msgpack map per frame) seen from the client: requests go out under a
// write mutex, one native reader thread cuts frames from the socket and
// sorts them. A RESPONSE ({"id": N, ...}) is handed, as raw payload bytes,
// straight to the thread blocked in call(N) — no interpreter involved; the
// caller decodes it. An EVENT ({"watch_id": N, ...}) and anything the
// classifier cannot place go, in wire order, to the on_frame callback.
//
// Plain C++17 + POSIX sockets, no Python headers: netwire_pybind.cpp wraps
// it, tests/native/netwire_selftest.cpp drives it over a socketpair.
//
// The fd is BORROWED: the owner (the Python socket object) closes it, and
// only after close() returned.

#pragma once

#include <pthread.h>
#include <sys/socket.h>
#include <sys/types.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "wire_frame.hpp"

#if defined(__SANITIZE_THREAD__)  // gcc
#define NETWIRE_TSAN 1
#elif defined(__has_feature)
#if __has_feature(thread_sanitizer)  // clang
#define NETWIRE_TSAN 1
#endif
#endif

namespace netwire {

// ---- msgpack: walk the top-level map's keys, skip everything else ---------

enum class FrameKind { Response, Event, Other };

struct Classified {
  FrameKind kind = FrameKind::Other;
  int64_t id = 0;
};

namespace detail {

struct Cursor {
  const unsigned char* p;
  const unsigned char* end;
  bool need(size_t n) const { return static_cast<size_t>(end - p) >= n; }
  uint64_t be(size_t n) {  // caller checked need(n)
    uint64_t v = 0;
    for (size_t k = 0; k < n; ++k) v = (v << 8) | p[k];
    p += n;
    return v;
  }
};

// Consume one element's head. `children` = elements nested directly under
// it (map: 2 per entry); a scalar's payload bytes are skipped here.
inline bool skip_head(Cursor& c, uint64_t& children) {
  children = 0;
  if (!c.need(1)) return false;
  unsigned char b = *c.p++;
  size_t payload = 0;
  if (b <= 0x7f || b >= 0xe0) return true;            // fixint
  if (b <= 0x8f) { children = 2u * (b & 0x0f); return true; }  // fixmap
  if (b <= 0x9f) { children = b & 0x0f; return true; }         // fixarray
  if (b <= 0xbf) { payload = b & 0x1f; }                       // fixstr
  else switch (b) {
    case 0xc0: case 0xc2: case 0xc3: return true;     // nil, false, true
    case 0xc4: case 0xd9:                             // bin8, str8
      if (!c.need(1)) return false;
      payload = c.be(1); break;
    case 0xc5: case 0xda:                             // bin16, str16
      if (!c.need(2)) return false;
      payload = c.be(2); break;
    case 0xc6: case 0xdb:                             // bin32, str32
      if (!c.need(4)) return false;
      payload = c.be(4); break;
    case 0xc7:                                        // ext8
      if (!c.need(1)) return false;
      payload = c.be(1) + 1; break;
    case 0xc8:                                        // ext16
      if (!c.need(2)) return false;
      payload = c.be(2) + 1; break;
    case 0xc9:                                        // ext32
      if (!c.need(4)) return false;
      payload = c.be(4) + 1; break;
    case 0xca: payload = 4; break;                    // float32
    case 0xcb: payload = 8; break;                    // float64
    case 0xcc: case 0xd0: payload = 1; break;         // uint8, int8
    case 0xcd: case 0xd1: payload = 2; break;
    case 0xce: case 0xd2: payload = 4; break;
    case 0xcf: case 0xd3: payload = 8; break;
    case 0xd4: payload = 2; break;                    // fixext1..16
    case 0xd5: payload = 3; break;
    case 0xd6: payload = 5; break;
    case 0xd7: payload = 9; break;
    case 0xd8: payload = 17; break;
    case 0xdc:                                        // array16
      if (!c.need(2)) return false;
      children = c.be(2); return true;
    case 0xdd:                                        // array32
      if (!c.need(4)) return false;
      children = c.be(4); return true;
    case 0xde:                                        // map16
      if (!c.need(2)) return false;
      children = 2 * c.be(2); return true;
    case 0xdf:                                        // map32
      if (!c.need(4)) return false;
      children = 2 * c.be(4); return true;
    default: return false;                            // 0xc1: never used
  }
  if (!c.need(payload)) return false;
  c.p += payload;
  return true;
}

// skip one whole element, nested ones included (no recursion: a counter of
// elements still owed is all the state a skipper needs)
inline bool skip_value(Cursor& c) {
  uint64_t owed = 1;
  while (owed > 0) {
    uint64_t children;
    if (!skip_head(c, children)) return false;
    owed += children;
    --owed;
  }
  return true;
}

// a str element: pointer + length, cursor moved past it
inline bool read_str(Cursor& c, const unsigned char*& s, size_t& n) {
  if (!c.need(1)) return false;
  unsigned char b = *c.p;
  if (b >= 0xa0 && b <= 0xbf) { c.p += 1; n = b & 0x1f; }
  else if (b == 0xd9) { if (!c.need(2)) return false; c.p += 1; n = c.be(1); }
  else if (b == 0xda) { if (!c.need(3)) return false; c.p += 1; n = c.be(2); }
  else if (b == 0xdb) { if (!c.need(5)) return false; c.p += 1; n = c.be(4); }
  else return false;
  if (!c.need(n)) return false;
  s = c.p;
  c.p += n;
  return true;
}

inline bool read_int(Cursor& c, int64_t& out) {
  if (!c.need(1)) return false;
  unsigned char b = *c.p;
  if (b <= 0x7f) { c.p += 1; out = b; return true; }
  if (b >= 0xe0) { c.p += 1; out = static_cast<int8_t>(b); return true; }
  size_t n;
  bool is_signed;
  switch (b) {
    case 0xcc: n = 1; is_signed = false; break;
    case 0xcd: n = 2; is_signed = false; break;
    case 0xce: n = 4; is_signed = false; break;
    case 0xcf: n = 8; is_signed = false; break;
    case 0xd0: n = 1; is_signed = true; break;
    case 0xd1: n = 2; is_signed = true; break;
    case 0xd2: n = 4; is_signed = true; break;
    case 0xd3: n = 8; is_signed = true; break;
    default: return false;
  }
  if (!c.need(1 + n)) return false;
  c.p += 1;
  uint64_t v = c.be(n);
  if (is_signed) {
    switch (n) {
      case 1: out = static_cast<int8_t>(v); break;
      case 2: out = static_cast<int16_t>(v); break;
      case 4: out = static_cast<int32_t>(v); break;
      default: out = static_cast<int64_t>(v); break;
    }
  } else {
    out = static_cast<int64_t>(v);
  }
  return true;
}

}  // namespace detail

// Event iff a top-level "watch_id" key exists; else Response iff a top-level
// integer "id" exists. Key order is NOT assumed (the Python server and the
// daemon emit different orders), so every top-level key is visited.
inline Classified classify(const char* data, size_t n) {
  using namespace detail;
  Classified out;
  Cursor c{reinterpret_cast<const unsigned char*>(data),
           reinterpret_cast<const unsigned char*>(data) + n};
  if (!c.need(1)) return out;
  unsigned char b = *c.p++;
  uint64_t entries;
  if (b >= 0x80 && b <= 0x8f) entries = b & 0x0f;
  else if (b == 0xde) { if (!c.need(2)) return out; entries = c.be(2); }
  else if (b == 0xdf) { if (!c.need(4)) return out; entries = c.be(4); }
  else return out;
  bool have_id = false;
  for (uint64_t e = 0; e < entries; ++e) {
    const unsigned char* k = nullptr;
    size_t kn = 0;
    const unsigned char* at = c.p;
    if (read_str(c, k, kn)) {
      if (kn == 8 && std::memcmp(k, "watch_id", 8) == 0) {
        out.kind = FrameKind::Event;
        return out;
      }
      if (kn == 2 && std::memcmp(k, "id", 2) == 0) {
        const unsigned char* vat = c.p;
        if (read_int(c, out.id)) {
          have_id = true;
          continue;
        }
        c.p = vat;  // "id" of another type: no response we can route
      }
    } else {
      c.p = at;
      if (!skip_value(c)) return Classified{};  // non-str key
    }
    if (!skip_value(c)) return Classified{};
  }
  if (have_id) out.kind = FrameKind::Response;
  return out;
}

// ---- the wire --------------------------------------------------------------

enum class CallStatus { Ok, Timeout, Lost, SendFailed };

class Wire : public std::enable_shared_from_this<Wire> {
 public:
  using FrameFn = std::function<void(const char*, size_t)>;
  using ClosedFn = std::function<void()>;

  // Always through create(): the reader thread keeps the object alive by a
  // shared_ptr of its own, so dropping the last outside reference from
  // within a callback cannot free the state under the reader.
  static std::shared_ptr<Wire> create(int fd, FrameFn on_frame,
                                      ClosedFn on_closed) {
    std::shared_ptr<Wire> w(new Wire(fd, std::move(on_frame),
                                     std::move(on_closed)));
    w->start();
    return w;
  }

  ~Wire() {
    // only reachable with the reader gone or on the reader itself (it holds
    // a reference while it runs)
    if (reader_.joinable()) {
      if (std::this_thread::get_id() == reader_.get_id() || forked())
        reader_.detach();
      else reader_.join();
    }
  }

  Wire(const Wire&) = delete;
  Wire& operator=(const Wire&) = delete;

  bool send(const char* data, size_t n) {
    std::lock_guard<std::mutex> g(write_mu_);
    if (stop_.load()) return false;
    while (n > 0) {
      ssize_t r = ::send(fd_, data, n, MSG_NOSIGNAL);
      if (r < 0) {
        if (errno == EINTR) continue;
        return false;
      }
      if (r == 0) return false;
      data += r;
      n -= static_cast<size_t>(r);
    }
    return true;
  }

  // Register a slot for `rid`, send the request, block until the reader
  // hands over that id's response payload (moved into `out`).
  CallStatus call(int64_t rid, const char* req, size_t n, double timeout_s,
                  std::string& out) {
    Slot slot;
    {
      std::lock_guard<std::mutex> g(pend_mu_);
      if (dead_) return CallStatus::Lost;
      pending_[rid] = &slot;
    }
    if (!send(req, n)) {
      std::lock_guard<std::mutex> g(pend_mu_);
      pending_.erase(rid);
      return slot.done && slot.status == CallStatus::Lost
                 ? CallStatus::Lost : CallStatus::SendFailed;
    }
    std::unique_lock<std::mutex> g(pend_mu_);
    auto deadline = std::chrono::steady_clock::now() +
                    std::chrono::duration_cast<std::chrono::nanoseconds>(
                        std::chrono::duration<double>(timeout_s));
#if defined(NETWIRE_TSAN)
    // ThreadSanitizer builds only: older runtimes do not model
    // pthread_cond_clockwait (what a steady-clock wait compiles to) and
    // would report the mutex as never released. Wait in short wall-clock
    // slices (pthread_cond_timedwait) against the same monotonic deadline.
    while (!slot.done) {
      auto now = std::chrono::steady_clock::now();
      if (now >= deadline) break;
      auto slice = std::min<std::chrono::steady_clock::duration>(
          deadline - now, std::chrono::milliseconds(50));
      slot.cv.wait_until(g, std::chrono::system_clock::now() + slice);
    }
#else
    slot.cv.wait_until(g, deadline, [&] { return slot.done; });
#endif
    if (!slot.done) {
      pending_.erase(rid);
      return CallStatus::Timeout;
    }
    if (slot.status == CallStatus::Ok) out = std::move(slot.payload);
    return slot.status;
  }

  // Stop the reader, fail pending calls, and (unless called from a callback
  // on the reader itself) wait until the reader is gone. No callback fires
  // after this returns. The fd may be closed by its owner afterwards.
  void close() {
    // In a forked child there is no reader thread to stop, and the socket
    // is the parent's connection: leave both alone.
    if (forked()) return;
    // The fd is touched by the FIRST close() only: once that returned, the
    // owner may have closed the fd and the number may name another socket.
    // A reader that left on its own (EOF, error) needs no unblocking.
    if (!stop_.exchange(true) && !exited_flag_.load()) {
      // unblocks the reader's recv, and a send stuck on a full socket
      ::shutdown(fd_, SHUT_RDWR);
    }
    { std::lock_guard<std::mutex> g(write_mu_); }  // no send past this point
    fail_pending();
    if (std::this_thread::get_id() == reader_id_) return;
    std::unique_lock<std::mutex> g(life_mu_);
    life_cv_.wait(g, [&] { return exited_; });
    if (reader_.joinable()) reader_.join();
  }

  bool alive() const { return !exited_flag_.load(); }

 private:
  bool forked() const { return ::getpid() != pid_; }

  struct Slot {
    std::condition_variable cv;
    bool done = false;
    CallStatus status = CallStatus::Ok;
    std::string payload;
  };

  Wire(int fd, FrameFn on_frame, ClosedFn on_closed)
      : fd_(fd), on_frame_(std::move(on_frame)),
        on_closed_(std::move(on_closed)) {}

  void start() {
    auto self = shared_from_this();
    std::unique_lock<std::mutex> g(life_mu_);
    reader_ = std::thread([self] { self->read_loop(); });
    reader_id_ = reader_.get_id();
  }

  void fail_pending() {
    std::lock_guard<std::mutex> g(pend_mu_);
    dead_ = true;
    for (auto& kv : pending_) {
      kv.second->status = CallStatus::Lost;
      kv.second->done = true;
      kv.second->cv.notify_one();
    }
    pending_.clear();
  }

  void deliver_response(int64_t rid, const char* p, size_t n) {
    std::lock_guard<std::mutex> g(pend_mu_);
    auto it = pending_.find(rid);
    if (it == pending_.end()) return;  // caller gave up (timeout)
    Slot* s = it->second;
    pending_.erase(it);
    s->payload.assign(p, n);
    s->done = true;
    // under the mutex: the slot lives on the waiter's stack and is gone as
    // soon as the waiter can see `done`
    s->cv.notify_one();
  }

  void read_loop() {
    { std::lock_guard<std::mutex> g(life_mu_); }  // reader_id_ is published
#ifdef __linux__
    pthread_setname_np(pthread_self(), "netwire-reader");  // for top -H, /proc
#endif
    std::vector<char> buf(1 << 16);
    size_t rpos = 0, wpos = 0;
    while (!stop_.load()) {
      // cut every complete frame out of [rpos, wpos)
      bool bad = false;
      while (wpos - rpos >= 4) {
        uint32_t len = wire::frame_len(buf.data() + rpos);
        if (len > wire::kMaxFrame) { bad = true; break; }
        if (wpos - rpos - 4 < len) {
          size_t need = static_cast<size_t>(len) + 4;
          if (buf.size() - rpos < need) {
            // make room for the whole frame: compact, then grow
            std::memmove(buf.data(), buf.data() + rpos, wpos - rpos);
            wpos -= rpos;
            rpos = 0;
            if (buf.size() < need) buf.resize(need);
          }
          break;
        }
        const char* payload = buf.data() + rpos + 4;
        Classified c = classify(payload, len);
        if (c.kind == FrameKind::Response) {
          deliver_response(c.id, payload, len);
        } else if (!stop_.load()) {
          on_frame_(payload, len);
        }
        rpos += 4 + static_cast<size_t>(len);
        if (stop_.load()) break;
      }
      if (bad || stop_.load()) break;
      if (rpos == wpos) {
        rpos = wpos = 0;
      } else if (buf.size() - wpos < 4096) {
        std::memmove(buf.data(), buf.data() + rpos, wpos - rpos);
        wpos -= rpos;
        rpos = 0;
        if (buf.size() - wpos < 4096) buf.resize(buf.size() * 2);
      }
      ssize_t r = ::recv(fd_, buf.data() + wpos, buf.size() - wpos, 0);
      if (r < 0 && errno == EINTR) continue;
      if (r <= 0) break;
      wpos += static_cast<size_t>(r);
    }
    // an oversized frame closes the connection, as the daemon does
    if (!stop_.load()) ::shutdown(fd_, SHUT_RDWR);
    fail_pending();
    if (!stop_.load()) on_closed_();
    exited_flag_.store(true);
    {
      std::lock_guard<std::mutex> g(life_mu_);
      exited_ = true;
      // under the mutex: a close() that sees `exited_` may return and let
      // the last reference go
      life_cv_.notify_all();
    }
  }

  const int fd_;
  const pid_t pid_ = ::getpid();
  FrameFn on_frame_;
  ClosedFn on_closed_;

  std::mutex write_mu_;
  std::atomic<bool> stop_{false};

  std::mutex pend_mu_;
  std::unordered_map<int64_t, Slot*> pending_;
  bool dead_ = false;

  std::mutex life_mu_;
  std::condition_variable life_cv_;
  bool exited_ = false;
  std::atomic<bool> exited_flag_{false};
  std::thread reader_;
  std::thread::id reader_id_;
};

}  // namespace netwire
