// The framing of the store wire (store/netstore.py's protocol), stated once
// for the daemon (stored_core.hpp) and the native client (netwire_core.hpp):
// every message is a 4-byte big-endian payload length, then the payload (one
// msgpack map). A length above kMaxFrame closes the connection.

#pragma once

#include <cstdint>
#include <string>

namespace wire {

constexpr uint32_t kMaxFrame = 64u << 20;
constexpr size_t kHeaderLen = 4;

inline std::string frame(const std::string& payload) {
  std::string out;
  out.reserve(payload.size() + kHeaderLen);
  uint32_t n = static_cast<uint32_t>(payload.size());
  for (int sh = 24; sh >= 0; sh -= 8) out.push_back(static_cast<char>(n >> sh));
  out += payload;
  return out;
}

inline uint32_t frame_len(const void* hdr) {  // kHeaderLen bytes
  const unsigned char* h = static_cast<const unsigned char*>(hdr);
  return (uint32_t{h[0]} << 24) | (uint32_t{h[1]} << 16) |
         (uint32_t{h[2]} << 8) | h[3];
}

}  // namespace wire
