// instaslice-stored: the daemon's process. Everything about the store and
// its connections is in stored_core.hpp (see there for the design); this
// file parses the command line (`instaslice-stored [port] [snapshot]`),
// listens on loopback, runs the snapshot thread, prints the LISTENING line
// and hands every accepted socket to a reader thread.

#include <arpa/inet.h>
#include <netinet/in.h>
#include <netinet/tcp.h>

#include <csignal>
#include <cstdlib>
#include <functional>

#include "stored_core.hpp"

static std::atomic<bool> g_stop{false};

static void on_signal(int) { g_stop.store(true); }

int main(int argc, char** argv) {
  using namespace stored;
  int port = 0;
  if (argc > 1) port = std::atoi(argv[1]);
  const char* snapshot = (argc > 2) ? argv[2] : nullptr;

  int srv = ::socket(AF_INET, SOCK_STREAM, 0);
  if (srv < 0) { perror("socket"); return 1; }
  int one = 1;
  ::setsockopt(srv, SOL_SOCKET, SO_REUSEADDR, &one, sizeof(one));
  sockaddr_in addr{};
  addr.sin_family = AF_INET;
  addr.sin_addr.s_addr = htonl(INADDR_LOOPBACK);
  addr.sin_port = htons(static_cast<uint16_t>(port));
  if (::bind(srv, reinterpret_cast<sockaddr*>(&addr), sizeof(addr)) != 0) {
    perror("bind");
    return 1;
  }
  socklen_t alen = sizeof(addr);
  ::getsockname(srv, reinterpret_cast<sockaddr*>(&addr), &alen);
  if (::listen(srv, 64) != 0) { perror("listen"); return 1; }
  // parent (store/native.py) parses this line for the chosen port
  Store store;
  if (snapshot) {
    store.set_persist_path(snapshot);
    if (store.load_snapshot())
      std::fprintf(stderr, "resumed from %s\n", snapshot);
    std::signal(SIGTERM, on_signal);
    std::signal(SIGINT, on_signal);
    // write-behind snapshot thread (200 ms debounce) + SIGTERM flush
    std::thread([&store] {
      for (;;) {
        std::this_thread::sleep_for(std::chrono::milliseconds(100));
        if (g_stop.load()) {
          store.flush_snapshot();
          std::_Exit(0);
        }
        if (store.take_dirty()) {
          std::this_thread::sleep_for(std::chrono::milliseconds(100));
          store.take_dirty();
          store.flush_snapshot();
        }
      }
    }).detach();
  }
  std::printf("LISTENING %d\n", ntohs(addr.sin_port));
  std::fflush(stdout);

  for (;;) {
    int fd = ::accept(srv, nullptr, nullptr);
    if (fd < 0) {
      if (errno == EINTR) continue;
      break;
    }
    ::setsockopt(fd, IPPROTO_TCP, TCP_NODELAY, &one, sizeof(one));
    auto conn = std::make_shared<Conn>();
    conn->fd = fd;
    std::thread(reader_loop, std::ref(store), conn).detach();
  }
  return 0;
}
