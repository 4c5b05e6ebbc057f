// gfx950 memcheck payload: proves that a partition's HBM holds data.
//
// census proves the XCDs, vecadd the ALUs, gemm the matrix cores; this one
// proves the memory a profile promises. It is a moving-inversions test with an
// address-derived pattern:
//
//   one pass (seed = pass index)
//     1. fill   every 16-byte unit with pattern(unit index)
//     2. check  the pattern and write its complement in place
//     3. check  the complement
//
// Three kernels, four traversals of the buffer; kernel boundaries order them.
// Every bit of the buffer is written and read back as 0 and as 1. The pattern
// of unit q is mix64(q ^ key), a bijection of q: two units never expect the
// same data, so a window that is smaller than promised and wraps, overlaps a
// neighbour's or aliases onto itself reads back as a mismatch, as does a
// dropped bit.
//
//   mix64(z): z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
//             z = (z ^ (z >> 27)) * 0x94D049BB133111EB
//             return z ^ (z >> 31)
//   key(seed) = mix64(seed + 0x9E3779B97F4A7C15)     (host side)
//   unit q:  h = mix64(q ^ key); word0 = h; word1 = ~rotl64(h, 31)
//
// One hash (two 64-bit multiplies) per 16 bytes, so the VALU work stays well
// under what a streaming kernel can hide. tests/test_memcheck_payload.py
// re-implements the pattern in numpy: change both together or neither.
//
// Kernel shape: 256-thread blocks, one 16-byte unit per lane per iteration,
// grid-stride loop, 64-bit indices throughout (a 36 GB partition has 2^31
// units and 2^35 bytes). Loads and stores are nontemporal as in
// stream_copy_nt_kernel: the data is used once and is meant to reach HBM.
// The default grid is grid_for(): the project's block sweep at 2 GiB
// (profiles/membw_block_sweep_r01.txt) has its best result at the 65535-block
// cap that grid_for applies.
//
// Mismatches: each lane accumulates privately over its loop; a wave in which
// any lane saw one (__ballot) reduces with __shfl_xor and one lane issues
// atomicAdd / atomicMin / atomicOr on the error record. A clean run issues no
// atomics at all.
//
// CACHE CAVEAT. The chip has a 256 MiB Infinity Cache and 4 MiB of L2 per
// XCD. A buffer no larger than the Infinity Cache can be served back from
// cache: a run of that size proves the kernel, not the HBM. Operational runs
// should be well above 256 MiB. Each traversal streams the whole buffer before
// anything is re-read, and that is what pushes the data out to HBM for large
// buffers.
//
// Included by payload_core.hpp (needs its HIP_CHECK, kBlock, grid_for,
// detail::DeviceBuffer and detail::Event).

#pragma once

#include <chrono>

namespace payload {

typedef unsigned long long mc_u64;  // the type HIP's 64-bit atomics take
typedef mc_u64 mc_unit __attribute__((ext_vector_type(2)));  // 16 bytes, 4 VGPRs

constexpr size_t kMemcheckUnit = 16;
constexpr size_t kMemcheckLlcBytes = size_t{256} << 20;  // Infinity Cache

static_assert(sizeof(mc_u64) == sizeof(uint64_t), "u64 words");
static_assert(sizeof(mc_unit) == kMemcheckUnit, "one dwordx4 access per unit");

// device record of what the check kernels found
struct MemcheckErr {
  mc_u64 bad_words;       // count of wrong 64-bit words
  mc_u64 first_bad_word;  // lowest wrong word index in the buffer, ~0 if none
  mc_u64 bad_bits;        // OR of the XOR differences
};

// ---- pattern -------------------------------------------------------------

__host__ __device__ __forceinline__ mc_u64 memcheck_mix64(mc_u64 z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__host__ __device__ __forceinline__ mc_u64 memcheck_word1(mc_u64 h) {
  return ~((h << 31) | (h >> 33));
}

inline uint64_t memcheck_key(uint64_t seed) {
  return memcheck_mix64(seed + 0x9E3779B97F4A7C15ull);
}

__device__ __forceinline__ mc_unit memcheck_unit(mc_u64 q, mc_u64 key, mc_u64 inv) {
  mc_u64 h = memcheck_mix64(q ^ key);
  mc_unit u;
  u.x = h ^ inv;
  u.y = memcheck_word1(h) ^ inv;
  return u;
}

// ---- kernels -------------------------------------------------------------

// p[i] = pattern(base_unit + i) ^ inv for i < n_units; inv is 0 or all-ones
__global__ __launch_bounds__(kBlock) void memcheck_fill_kernel(
    mc_unit* __restrict__ p, mc_u64 n_units, mc_u64 base_unit, mc_u64 key,
    mc_u64 inv) {
  mc_u64 i = blockIdx.x * static_cast<mc_u64>(blockDim.x) + threadIdx.x;
  mc_u64 stride = static_cast<mc_u64>(gridDim.x) * blockDim.x;
  for (; i < n_units; i += stride)
    __builtin_nontemporal_store(memcheck_unit(base_unit + i, key, inv), &p[i]);
}

// Compare p[i] with pattern ^ inv. kInvert also stores the complement of the
// EXPECTED value (not of what was read) in the same pass, so one bad word is
// counted once and then overwritten.
template <bool kInvert>
__global__ __launch_bounds__(kBlock) void memcheck_check_kernel(
    mc_unit* __restrict__ p, mc_u64 n_units, mc_u64 base_unit, mc_u64 key,
    mc_u64 inv, MemcheckErr* __restrict__ err) {
  mc_u64 i = blockIdx.x * static_cast<mc_u64>(blockDim.x) + threadIdx.x;
  mc_u64 stride = static_cast<mc_u64>(gridDim.x) * blockDim.x;
  mc_u64 bad = 0, first = ~0ull, bits = 0;
  for (; i < n_units; i += stride) {
    mc_unit want = memcheck_unit(base_unit + i, key, inv);
    mc_unit got = __builtin_nontemporal_load(&p[i]);
    mc_u64 d0 = got.x ^ want.x, d1 = got.y ^ want.y;
    if (d0 | d1) {  // rare: keeps the clean path to one OR and a branch
      bad += (d0 != 0) + (d1 != 0);
      mc_u64 w = 2 * i + (d0 ? 0 : 1);
      if (w < first) first = w;
      bits |= d0 | d1;
    }
    if (kInvert) {
      mc_unit flipped;
      flipped.x = ~want.x;
      flipped.y = ~want.y;
      __builtin_nontemporal_store(flipped, &p[i]);
    }
  }
  // all 64 lanes are back together here, whatever their trip counts were
  if (__ballot(bad != 0) != 0) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      bad += __shfl_xor(bad, off);
      mc_u64 f = __shfl_xor(first, off);
      if (f < first) first = f;
      bits |= __shfl_xor(bits, off);
    }
    if ((threadIdx.x & 63) == 0) {
      atomicAdd(&err->bad_words, bad);
      atomicMin(&err->first_bad_word, first);
      atomicOr(&err->bad_bits, bits);
    }
  }
}

// Self-test hook: XOR `mask` into one word of the buffer with a plain store.
// One thread; the host checks that word_index lies inside the buffer.
__global__ void memcheck_flip_kernel(mc_u64* __restrict__ p, mc_u64 word_index,
                                     mc_u64 mask) {
  if (blockIdx.x == 0 && threadIdx.x == 0) p[word_index] ^= mask;
}

// ---- host layer ----------------------------------------------------------

struct MemcheckResult {
  size_t bytes = 0;  // what was tested: the request rounded down to 16
  int passes = 0;
  uint64_t bad_words = 0;
  int64_t first_bad_offset = -1;  // bytes, -1 if none
  uint64_t bad_bits = 0;
  double fill_gb_s = 0;   // step 1: bytes written / event time, over passes
  double check_gb_s = 0;  // step 3 (read-only): bytes read / event time
  double ms = 0;          // wall time between upload and result
};

// Host implementation of the pattern: words first_word .. first_word+n_words-1
// of a buffer whose unit 0 is unit 0 of the pattern. first_word may be odd.
inline void memcheck_pattern(uint64_t* out, uint64_t first_word, size_t n_words,
                             uint64_t seed) {
  const mc_u64 key = memcheck_key(seed);
  for (size_t j = 0; j < n_words; ++j) {
    mc_u64 w = first_word + j;
    mc_u64 h = memcheck_mix64((w >> 1) ^ key);
    out[j] = (w & 1) ? memcheck_word1(h) : h;
  }
}

namespace detail {

inline size_t memcheck_units(size_t bytes, const char* who) {
  size_t n = bytes / kMemcheckUnit;
  if (n == 0)
    throw std::invalid_argument(std::string(who) + ": bytes must be >= 16");
  return n;
}

inline int memcheck_grid(size_t n_units, int blocks) {
  return blocks > 0 ? blocks : grid_for(n_units);
}

}  // namespace detail

// The fill kernel alone on a fresh buffer of `bytes` (rounded down to 16),
// downloaded into out: lets the device pattern be compared with an
// independent reference, so a bug shared by fill and check cannot hide behind
// a clean self-check. base_unit is the pattern index of the buffer's unit 0.
inline void memcheck_fill(uint64_t* out, size_t bytes, uint64_t seed = 0,
                          uint64_t base_unit = 0, bool invert = false,
                          int device = 0, int blocks = 0) {
  size_t n_units = detail::memcheck_units(bytes, "memcheck_fill");
  if (blocks < 0) throw std::invalid_argument("memcheck_fill: blocks must be >= 0");
  HIP_CHECK(hipSetDevice(device));
  detail::DeviceBuffer buf;
  buf.alloc(n_units * kMemcheckUnit);
  hipLaunchKernelGGL(memcheck_fill_kernel,
                     dim3(detail::memcheck_grid(n_units, blocks)), dim3(kBlock),
                     0, 0, buf.as<mc_unit>(), static_cast<mc_u64>(n_units),
                     static_cast<mc_u64>(base_unit),
                     static_cast<mc_u64>(memcheck_key(seed)),
                     invert ? ~0ull : 0ull);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpy(out, buf.p, n_units * kMemcheckUnit, hipMemcpyDeviceToHost));
}

// Moving-inversions sweep of one buffer of `bytes` (rounded down to 16).
// blocks = 0 picks the default grid; an explicit count forces the grid-stride
// loop on a small buffer. flip_offset >= 0 is the self-test: after step 1 of
// pass 0 the word holding that byte is XORed with flip_mask, step 2 must count
// exactly that word and overwrite it, and every later check is clean.
// Argument errors are thrown before the device is touched. A failed hipMalloc
// surfaces as the usual "HIP error: ..." exception: for this probe that is a
// finding (the partition does not have the memory).
inline MemcheckResult run_memcheck(size_t bytes, int passes = 1, int device = 0,
                                   int blocks = 0, int64_t flip_offset = -1,
                                   uint64_t flip_mask = 0) {
  size_t n_units = detail::memcheck_units(bytes, "run_memcheck");
  bytes = n_units * kMemcheckUnit;
  if (passes < 1) throw std::invalid_argument("run_memcheck: passes must be >= 1");
  if (blocks < 0) throw std::invalid_argument("run_memcheck: blocks must be >= 0");
  if (flip_offset >= 0 && static_cast<uint64_t>(flip_offset) >= bytes)
    throw std::invalid_argument("run_memcheck: flip_offset is outside the buffer");

  HIP_CHECK(hipSetDevice(device));
  detail::DeviceBuffer buf, derr;
  buf.alloc(bytes);
  derr.alloc(sizeof(MemcheckErr));
  MemcheckErr herr{0, ~0ull, 0};
  HIP_CHECK(hipMemcpy(derr.p, &herr, sizeof(herr), hipMemcpyHostToDevice));
  auto wall0 = std::chrono::steady_clock::now();

  const dim3 grid(detail::memcheck_grid(n_units, blocks)), block(kBlock);
  mc_unit* p = buf.as<mc_unit>();
  MemcheckErr* e = derr.as<MemcheckErr>();
  const mc_u64 n = n_units;
  detail::Event f0, f1, c0, c1;
  double fill_ms = 0, check_ms = 0;
  for (int pass = 0; pass < passes; ++pass) {
    const mc_u64 key = memcheck_key(static_cast<uint64_t>(pass));
    HIP_CHECK(hipEventRecord(f0.e, 0));
    hipLaunchKernelGGL(memcheck_fill_kernel, grid, block, 0, 0, p, n, 0ull, key, 0ull);
    HIP_CHECK(hipEventRecord(f1.e, 0));
    if (pass == 0 && flip_offset >= 0)
      hipLaunchKernelGGL(memcheck_flip_kernel, dim3(1), dim3(1), 0, 0,
                         buf.as<mc_u64>(), static_cast<mc_u64>(flip_offset) >> 3,
                         static_cast<mc_u64>(flip_mask));
    hipLaunchKernelGGL(memcheck_check_kernel<true>, grid, block, 0, 0, p, n, 0ull,
                       key, 0ull, e);
    HIP_CHECK(hipEventRecord(c0.e, 0));
    hipLaunchKernelGGL(memcheck_check_kernel<false>, grid, block, 0, 0, p, n, 0ull,
                       key, ~0ull, e);
    HIP_CHECK(hipEventRecord(c1.e, 0));
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventSynchronize(c1.e));
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, f0.e, f1.e));
    fill_ms += ms;
    HIP_CHECK(hipEventElapsedTime(&ms, c0.e, c1.e));
    check_ms += ms;
  }
  HIP_CHECK(hipMemcpy(&herr, derr.p, sizeof(herr), hipMemcpyDeviceToHost));
  auto wall1 = std::chrono::steady_clock::now();

  MemcheckResult r;
  r.bytes = bytes;
  r.passes = passes;
  r.bad_words = herr.bad_words;
  r.first_bad_offset =
      herr.bad_words ? static_cast<int64_t>(herr.first_bad_word * 8) : -1;
  r.bad_bits = herr.bad_bits;
  const double moved = static_cast<double>(bytes) * passes;
  r.fill_gb_s = fill_ms > 0 ? moved / (fill_ms * 1e-3) / 1e9 : 0;
  r.check_gb_s = check_ms > 0 ? moved / (check_ms * 1e-3) / 1e9 : 0;
  r.ms = std::chrono::duration<double, std::milli>(wall1 - wall0).count();
  return r;
}

}  // namespace payload
