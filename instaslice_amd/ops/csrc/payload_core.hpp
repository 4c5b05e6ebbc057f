// gfx950 HIP payload kernels: the workloads InstaSlice-AMD runs *inside*
// partitions to validate and benchmark them.
//
// The reference's only GPU workload is a prebuilt cuda-vectoradd container
// (samples/test-pod.yaml:12) used to prove a MIG slice works. Here the
// payloads are first-party CDNA4 kernels with a partition-verification angle:
//
//   vecadd       correctness smoke (the cuda-vectoradd analog); the self-check's
//                operands come from the element index, so a wrong index is a
//                wrong value
//   membw        streaming-copy bandwidth probe: a CPX partition sees ~1/8 of
//                chip HBM bandwidth under NPS1 and its local quadrant's share
//                under NPS4 — measured, this *proves* the partition boundary;
//                the destination is checked against an index-derived pattern,
//                so a rate is only reported for a copy that copied
//   busy         bounded wall-clock spin filling the partition ("sleep pod"),
//                at most 60 s; reports the device-side elapsed time
//   xcd_census   every workgroup reports s_getreg_b32(HW_REG_XCC_ID): in a
//                CPX partition exactly one XCD may appear; in SPX all 8.
//                (XCC_ID read is a validation/performance tool, never a
//                correctness dependency — cdna_hip_programming.md §1.)
//   gemm         bf16 MFMA GEMM, exact-checked and timed: the matrix cores are
//                what a tenant pays for (payload_gemm.hpp, included below)
//   mxgemm       MXFP8 block-scaled MFMA GEMM (OCP e4m3 operands, E8M0 scales
//                per 32 elements), exact-checked and timed: the low-precision
//                matrix path, a different instruction and datapath than bf16
//                (payload_mxgemm.hpp, included below)
//   mx4gemm      MXFP4 block-scaled MFMA GEMM (OCP e2m1 operands, two to a
//                byte, E8M0 scales per 32 elements), exact-checked and timed:
//                the 4-bit matrix path, the same instruction with other format
//                selectors and half the operand registers
//                (payload_mxfp4.hpp, included below)
//   memcheck    moving-inversions memory test with an address-derived
//                pattern at streaming rate: the HBM a profile promises is
//                there, holds data and does not alias (payload_memcheck.hpp,
//                included below)
//   attn         KV-cache decode attention (single-token, grouped-query, head
//                dim 128) with split-KV: K and V streamed from global memory
//                straight through the bf16 MFMA with an fp32 online softmax,
//                exact-checked, bound-checked and timed: the hot kernel of an
//                LLM server in decode (payload_attn.hpp, included below)
//   prefill      causal prefill attention over a whole prompt (grouped-query,
//                head dim 128): K and V tiles staged through swizzled,
//                double-buffered LDS and shared by the workgroup's waves, both
//                products on the bf16 MFMA with the fp32 online softmax in
//                between, exact-checked, bound-checked and timed: the
//                compute-bound half of serving (payload_prefill.hpp, included
//                below)
//
// Kernel style per the CDNA4 playbook: 256-thread blocks (4 waves of 64),
// float4 (dwordx4) streaming accesses for coalescing, grid-strided loops
// sized >> 256 workgroups to fill all 8 XCDs, bounded spins only.

#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

namespace payload {

#define HIP_CHECK(expr)                                                   \
  do {                                                                    \
    hipError_t _e = (expr);                                               \
    if (_e != hipSuccess) {                                               \
      throw std::runtime_error(std::string("HIP error: ") +               \
                               hipGetErrorString(_e) + " at " #expr);     \
    }                                                                     \
  } while (0)

constexpr int kBlock = 256;  // 4 wave64s per workgroup

// ---- kernels -------------------------------------------------------------

__global__ __launch_bounds__(kBlock) void vecadd_kernel(
    const float4* __restrict__ a, const float4* __restrict__ b,
    float4* __restrict__ c, size_t n4) {
  size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x;
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (; i < n4; i += stride) {
    float4 x = a[i], y = b[i];
    c[i] = make_float4(x.x + y.x, x.y + y.y, x.z + y.z, x.w + y.w);
  }
}

// p[e] = float(e & mask) for every float e of the n4 float4s. mask must stay
// below 2^24 so that the value is exact in fp32. run_vecadd fills its operands
// with two disjoint masks: the sum is then exact and names its own index.
__global__ __launch_bounds__(kBlock) void index_fill_kernel(
    float4* __restrict__ p, unsigned int mask, size_t n4) {
  size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x;
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (; i < n4; i += stride) {
    // only the low 24 bits of the element index survive the mask
    unsigned int e = static_cast<unsigned int>(4 * i);
    p[i] = make_float4(static_cast<float>(e & mask),
                       static_cast<float>((e + 1) & mask),
                       static_cast<float>((e + 2) & mask),
                       static_cast<float>((e + 3) & mask));
  }
}

// The 128-bit unit that the bandwidth probe expects at unit index q. The
// multiplier is odd, so h is a bijection of q and (x, y) alone tell any two
// units apart; z and w differ from x and y and from each other, so a dropped
// or swapped component shows as well.
typedef unsigned int copy_unit __attribute__((ext_vector_type(4)));
static_assert(sizeof(copy_unit) == sizeof(float4), "one dwordx4 access per unit");

__device__ __forceinline__ copy_unit copy_pattern(unsigned long long q) {
  unsigned long long h = q * 0x9E3779B97F4A7C15ull + 0x7F4A7C15ull;
  copy_unit u;
  u.x = static_cast<unsigned int>(h);
  u.y = static_cast<unsigned int>(h >> 32);
  u.z = static_cast<unsigned int>(q) ^ 0xA5A5A5A5u;
  u.w = ~u.y;
  return u;
}

__global__ __launch_bounds__(kBlock) void copy_fill_kernel(
    copy_unit* __restrict__ p, size_t n4) {
  size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x;
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (; i < n4; i += stride) p[i] = copy_pattern(i);
}

// Counts the units of p that differ from the pattern RECOMPUTED from the
// index (not from the copy's source: a bad fill shows up too). Each lane
// counts privately; a clean run issues no atomics.
__global__ __launch_bounds__(kBlock) void copy_check_kernel(
    const copy_unit* __restrict__ p, size_t n4,
    unsigned long long* __restrict__ bad_units) {
  size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x;
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  unsigned long long bad = 0;
  for (; i < n4; i += stride) {
    copy_unit got = p[i], want = copy_pattern(i);
    if ((got.x ^ want.x) | (got.y ^ want.y) | (got.z ^ want.z) | (got.w ^ want.w))
      ++bad;
  }
  if (bad) atomicAdd(bad_units, bad);
}

// float4 streaming copy — the measured-bandwidth shape (6.29 TB/s whole-chip,
// MI355X_MICROARCH.md §Chip-level parameters).
__global__ __launch_bounds__(kBlock) void stream_copy_kernel(
    const float4* __restrict__ src, float4* __restrict__ dst, size_t n4) {
  size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x;
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (; i < n4; i += stride) dst[i] = src[i];
}

// Nontemporal variant: streamed data is used exactly once, so bypassing the
// L2/LLC write-allocate path frees cache bandwidth for the reads.
__global__ __launch_bounds__(kBlock) void stream_copy_nt_kernel(
    const float4* __restrict__ src, float4* __restrict__ dst, size_t n4) {
  size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x;
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  // the builtin wants a scalar/vector-of-scalar pointer, not the
  // HIP_vector_type struct: reinterpret as the native 4-float vector
  typedef float vfloat4 __attribute__((ext_vector_type(4)));
  const vfloat4* s = reinterpret_cast<const vfloat4*>(src);
  vfloat4* d = reinterpret_cast<vfloat4*>(dst);
  for (; i < n4; i += stride) {
    vfloat4 v = __builtin_nontemporal_load(&s[i]);
    __builtin_nontemporal_store(v, &d[i]);
  }
}

// Bounded busy-wait on the constant-rate wall clock (s_memrealtime). The
// iteration guard bounds the spin even if the clock misbehaves
// (cdna_hip_programming.md §1: "bound every spin"). Block 0's first lane
// reports what its own spin saw: result[0] = elapsed ticks at exit, result[1]
// = iterations. result must hold two counters.
__global__ __launch_bounds__(kBlock) void busy_kernel(
    unsigned long long ticks, unsigned long long max_iters,
    unsigned int* __restrict__ sink, unsigned long long* __restrict__ result) {
  unsigned long long start = wall_clock64();
  unsigned long long it = 0;
  unsigned int acc = 0;
  while (wall_clock64() - start < ticks && it < max_iters) {
    acc += static_cast<unsigned int>(it++);
  }
  if (threadIdx.x == 0 && acc == 0xFFFFFFFFu) *sink = acc;  // never taken
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    result[0] = wall_clock64() - start;
    result[1] = it;
  }
}

// One lane per workgroup records its XCD id. per_xcd must hold 8 counters.
__global__ __launch_bounds__(kBlock) void xcd_census_kernel(
    unsigned int* __restrict__ per_xcd) {
  if (threadIdx.x == 0) {
    unsigned int xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    atomicAdd(&per_xcd[xcc & 7], 1u);
  }
}

// ---- host wrappers -------------------------------------------------------

struct DeviceInfo {
  int device = 0;
  std::string name;
  std::string gcn_arch;
  int cu_count = 0;
  double total_mem_gb = 0;
  int xcd_count_visible = 0;  // from xcd census
};

constexpr size_t kMaxGrid = 65535;  // grid_for's cap, and the most `blocks` may ask

inline int grid_for(size_t n4) {
  size_t blocks = (n4 + kBlock - 1) / kBlock;
  // >> 256 workgroups to fill 8 XCDs x 32 CUs (cap keeps launch sane)
  if (blocks > kMaxGrid) blocks = kMaxGrid;
  if (blocks < 1) blocks = 1;
  return static_cast<int>(blocks);
}

namespace detail {

// hipFree / hipEventDestroy on every exit path, throws included
struct DeviceBuffer {
  void* p = nullptr;
  DeviceBuffer() = default;
  DeviceBuffer(const DeviceBuffer&) = delete;
  DeviceBuffer& operator=(const DeviceBuffer&) = delete;
  ~DeviceBuffer() {
    if (p) (void)hipFree(p);
  }
  void alloc(size_t bytes) { HIP_CHECK(hipMalloc(&p, bytes)); }
  template <typename T>
  T* as() const { return static_cast<T*>(p); }
};

struct Event {
  hipEvent_t e = nullptr;
  Event() { HIP_CHECK(hipEventCreate(&e)); }
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
  ~Event() {
    if (e) (void)hipEventDestroy(e);
  }
};

// Milliseconds of `iters` calls of launch() between two events, after one
// warm-up call and a device synchronise: the timed loop of the GEMM and
// attention payloads. run_membw_check and run_memcheck keep loops of their
// own, on purpose: the first enqueues its check kernel behind the loop before
// it synchronises, the second times two phases.
template <class Launch>
float time_launches(int iters, Launch&& launch) {
  launch();  // warmup
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipDeviceSynchronize());
  Event t0, t1;
  HIP_CHECK(hipEventRecord(t0.e, 0));
  for (int i = 0; i < iters; ++i) launch();
  HIP_CHECK(hipEventRecord(t1.e, 0));
  HIP_CHECK(hipEventSynchronize(t1.e));
  HIP_CHECK(hipGetLastError());
  float ms = 0;
  HIP_CHECK(hipEventElapsedTime(&ms, t0.e, t1.e));
  return ms;
}

constexpr size_t kGuardBytes = 4096;  // a multiple of 16: the interior stays aligned
constexpr unsigned char kGuardByte = 0xA5;

// A device buffer with kGuardBytes of 0xA5 on each side of the interior that
// the kernel gets: a store that misses the interior by up to 4 KiB lands in
// memory we own and is counted by changed(), fault or no fault.
struct GuardedBuffer {
  DeviceBuffer buf;
  size_t bytes = 0;  // interior
  void alloc(size_t interior_bytes) {
    bytes = interior_bytes;
    buf.alloc(bytes + 2 * kGuardBytes);
    HIP_CHECK(hipMemset(buf.p, kGuardByte, bytes + 2 * kGuardBytes));
  }
  template <typename T>
  T* interior() const {
    return reinterpret_cast<T*>(buf.as<unsigned char>() + kGuardBytes);
  }
  // guard bytes that no longer hold 0xA5
  size_t changed() const {
    std::vector<unsigned char> g(2 * kGuardBytes);
    HIP_CHECK(hipMemcpy(g.data(), buf.p, kGuardBytes, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(g.data() + kGuardBytes,
                        buf.as<unsigned char>() + kGuardBytes + bytes, kGuardBytes,
                        hipMemcpyDeviceToHost));
    size_t n = 0;
    for (unsigned char c : g) n += c != kGuardByte;
    return n;
  }
};

// blocks = 0 is grid_for; an explicit count forces that grid
inline int grid_arg(const char* who, size_t n4, int blocks) {
  if (blocks < 0 || static_cast<size_t>(blocks) > kMaxGrid)
    throw std::invalid_argument(std::string(who) + ": blocks must be in 0 .. 65535");
  return blocks > 0 ? blocks : grid_for(n4);
}

// n floats (or 32-bit words) of host data in a zero-padded device image of
// whole float4s
inline void upload_padded(DeviceBuffer& d, const void* host, size_t n, size_t n4) {
  d.alloc(n4 * sizeof(float4));
  HIP_CHECK(hipMemset(d.p, 0, n4 * sizeof(float4)));
  HIP_CHECK(hipMemcpy(d.p, host, n * sizeof(float), hipMemcpyHostToDevice));
}

}  // namespace detail

// c[i] = a[i] + b[i] over n >= 1 floats of host data on vecadd_kernel: the
// operands are zero-padded to whole float4s, the destination has a guard on
// each side. Returns the number of guard bytes the kernel changed (expect 0).
// Argument errors are thrown before any HIP call.
inline size_t vecadd(const float* a, const float* b, float* c, size_t n,
                     int device = 0, int blocks = 0) {
  if (n < 1) throw std::invalid_argument("vecadd: n must be >= 1");
  size_t n4 = (n + 3) / 4;
  int grid = detail::grid_arg("vecadd", n4, blocks);
  HIP_CHECK(hipSetDevice(device));
  detail::DeviceBuffer da, db;
  detail::GuardedBuffer dc;
  detail::upload_padded(da, a, n, n4);
  detail::upload_padded(db, b, n, n4);
  dc.alloc(n4 * sizeof(float4));
  hipLaunchKernelGGL(vecadd_kernel, dim3(grid), dim3(kBlock), 0, 0, da.as<float4>(),
                     db.as<float4>(), dc.interior<float4>(), n4);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpy(c, dc.interior<float>(), n * sizeof(float),
                      hipMemcpyDeviceToHost));
  return dc.changed();
}

// y[i] = x[i] over n >= 1 32-bit words on stream_copy_kernel or its
// nontemporal variant, padded and guarded as vecadd is. Words, not floats: the
// copy must keep every bit pattern, NaN payloads included.
inline size_t stream_copy(const uint32_t* x, uint32_t* y, size_t n,
                          bool nontemporal = false, int device = 0, int blocks = 0) {
  if (n < 1) throw std::invalid_argument("stream_copy: n must be >= 1");
  size_t n4 = (n + 3) / 4;
  int grid = detail::grid_arg("stream_copy", n4, blocks);
  HIP_CHECK(hipSetDevice(device));
  detail::DeviceBuffer dx;
  detail::GuardedBuffer dy;
  detail::upload_padded(dx, x, n, n4);
  dy.alloc(n4 * sizeof(float4));
  auto kernel = nontemporal ? stream_copy_nt_kernel : stream_copy_kernel;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, 0, dx.as<float4>(),
                     dy.interior<float4>(), n4);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpy(y, dy.interior<uint32_t>(), n * sizeof(uint32_t),
                      hipMemcpyDeviceToHost));
  return dy.changed();
}

// Correctness smoke: c = a + b over n >= 1 floats; returns max |err| (expect
// 0.0). The operands come from the element index e: a[e] = e & 0xFFF and
// b[e] = e & 0xFFF000, both exact in fp32, and their sum e & 0xFFFFFF is exact
// and differs for any two elements less than 2^24 apart, so a kernel that
// reads or writes the wrong element does not pass. Elements a multiple of 2^24
// apart expect the same value: that is the limit of this check. So is this:
// c is not cleared first (the launch count is the one bench.py times), so in
// a warm process a kernel that stores nothing can be vouched for by the c of
// an earlier call of the same size; vecadd() above clears its destination.
inline double run_vecadd(size_t n, int device = 0) {
  if (n < 1) throw std::invalid_argument("run_vecadd: n must be >= 1");
  HIP_CHECK(hipSetDevice(device));
  size_t n4 = (n + 3) / 4;
  detail::DeviceBuffer a, b, c;
  a.alloc(n4 * sizeof(float4));
  b.alloc(n4 * sizeof(float4));
  c.alloc(n4 * sizeof(float4));
  int grid = grid_for(n4);
  hipLaunchKernelGGL(index_fill_kernel, dim3(grid), dim3(kBlock), 0, 0,
                     a.as<float4>(), 0xFFFu, n4);
  hipLaunchKernelGGL(index_fill_kernel, dim3(grid), dim3(kBlock), 0, 0,
                     b.as<float4>(), 0xFFF000u, n4);
  hipLaunchKernelGGL(vecadd_kernel, dim3(grid), dim3(kBlock), 0, 0, a.as<float4>(),
                     b.as<float4>(), c.as<float4>(), n4);
  HIP_CHECK(hipGetLastError());
  std::vector<float> host(4 * n4);
  HIP_CHECK(hipMemcpy(host.data(), c.p, n4 * sizeof(float4), hipMemcpyDeviceToHost));
  // First "is anything wrong at all": int -> float and a compare, which the
  // host compiler vectorises (a tenth of the time of the loop below, and this
  // function is what the benchmark's warm pool times). NaN != x holds.
  const float* h = host.data();
  const size_t total = host.size();
  unsigned int wrong = 0;
  for (size_t e = 0; e < total; ++e)
    wrong |= h[e] != static_cast<float>(
                         static_cast<int>(static_cast<uint32_t>(e) & 0xFFFFFFu));
  if (!wrong) return 0.0;
  double max_err = 0;
  for (size_t e = 0; e < host.size(); ++e) {
    double d = static_cast<double>(host[e]) - static_cast<double>(e & 0xFFFFFFu);
    if (d < 0) d = -d;
    if (!(d <= max_err)) max_err = d != d ? HUGE_VAL : d;  // a NaN is an error too
  }
  return max_err;
}

struct MembwResult {
  double gb_s = 0;  // read+write bytes over event time
  unsigned long long bad_units = 0;  // 16-byte units of dst that are not the pattern
};

// Streaming-copy bandwidth in GB/s (read+write bytes counted), and a check
// that the copy copied: src is filled with copy_pattern(unit index) and, after
// the timed loop, dst is compared with the pattern recomputed from the index.
// blocks=0 picks the default grid; pass an explicit count to sweep the
// workgroups-per-CU space (MI355X: 256 CUs x 8 XCDs; the guide's rule is
// >> 256 workgroups to fill the chip). Argument errors are thrown before any
// HIP call.
inline MembwResult run_membw_check(size_t bytes, int iters, int device = 0,
                                   int blocks = 0, bool nontemporal = false) {
  size_t n4 = bytes / sizeof(float4);
  if (n4 == 0) throw std::invalid_argument("run_membw: bytes must be >= 16");
  if (iters < 1) throw std::invalid_argument("run_membw: iters must be >= 1");
  int grid = detail::grid_arg("run_membw", n4, blocks);
  HIP_CHECK(hipSetDevice(device));
  detail::DeviceBuffer src, dst, bad;
  src.alloc(n4 * sizeof(float4));
  dst.alloc(n4 * sizeof(float4));
  bad.alloc(sizeof(unsigned long long));
  HIP_CHECK(hipMemset(bad.p, 0, sizeof(unsigned long long)));
  // a freed buffer comes back with its old contents: without this, the dst of
  // an earlier clean run would vouch for a copy that wrote nothing. No unit of
  // the pattern is all 0xA5 (w = ~y).
  HIP_CHECK(hipMemset(dst.p, 0xA5, n4 * sizeof(float4)));
  auto kernel = nontemporal ? stream_copy_nt_kernel : stream_copy_kernel;
  hipLaunchKernelGGL(copy_fill_kernel, dim3(grid), dim3(kBlock), 0, 0,
                     src.as<copy_unit>(), n4);
  // warmup
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, 0, src.as<float4>(),
                     dst.as<float4>(), n4);
  HIP_CHECK(hipDeviceSynchronize());
  detail::Event t0, t1;
  HIP_CHECK(hipEventRecord(t0.e, 0));
  for (int i = 0; i < iters; ++i) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, 0, src.as<float4>(),
                       dst.as<float4>(), n4);
  }
  HIP_CHECK(hipEventRecord(t1.e, 0));
  hipLaunchKernelGGL(copy_check_kernel, dim3(grid), dim3(kBlock), 0, 0,
                     dst.as<copy_unit>(), n4, bad.as<unsigned long long>());
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipEventSynchronize(t1.e));
  float ms = 0;
  HIP_CHECK(hipEventElapsedTime(&ms, t0.e, t1.e));
  MembwResult r;
  HIP_CHECK(hipMemcpy(&r.bad_units, bad.p, sizeof(r.bad_units), hipMemcpyDeviceToHost));
  double moved = 2.0 * static_cast<double>(n4) * sizeof(float4) * iters;
  r.gb_s = ms > 0 ? moved / (ms * 1e-3) / 1e9 : 0;
  return r;
}

// The rate alone. A rate from a copy that did not copy is not reported: throws
// if any unit of dst is wrong.
inline double run_membw(size_t bytes, int iters, int device = 0, int blocks = 0,
                        bool nontemporal = false) {
  MembwResult r = run_membw_check(bytes, iters, device, blocks, nontemporal);
  if (r.bad_units != 0)
    throw std::runtime_error("run_membw: " + std::to_string(r.bad_units) +
                             " units of the copy's destination are wrong");
  return r.gb_s;
}

// the longest spin run_busy accepts: ops/verify.py's CHILD_TIMEOUT_S, past
// which no caller is still waiting
constexpr double kBusyMaxMs = 60000.0;

struct BusyResult {
  double elapsed_ms = 0;          // device clock, block 0's first lane
  unsigned long long iters = 0;   // trips of that lane's spin
  bool guard_hit = false;         // the iteration guard ended the spin
};

// Occupy the visible device for ~ms milliseconds (the "sleep pod" payload).
// ms must be finite and in 0 .. 60000: checked before any HIP call, so the
// tick count below is computed from a value known to fit. max_iters bounds
// every lane's spin; 0 is the built-in bound of ~0ull, which no run reaches:
// the loop's iteration rate has not been measured, so a tighter bound that
// never cuts a legitimate 60 s spin short cannot be derived honestly. The
// clock is what ends the spin; ms <= 60000 is what bounds it.
inline BusyResult run_busy(double ms, int device = 0,
                           unsigned long long max_iters = 0) {
  if (!std::isfinite(ms) || ms < 0 || ms > kBusyMaxMs)
    throw std::invalid_argument("run_busy: ms must be finite and in 0 .. 60000");
  HIP_CHECK(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIP_CHECK(hipGetDeviceProperties(&prop, device));
  // wall_clock64 rate: hipDeviceAttributeWallClockRate in kHz = ticks per ms
  int khz = 0;
  HIP_CHECK(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device));
  if (khz <= 0) khz = 100000;  // gfx9 constant clock default 100 MHz
  // at most 6e4 * 2^31 < 2^47; rounded up, so the spin never ends early
  unsigned long long ticks =
      static_cast<unsigned long long>(std::ceil(ms * static_cast<double>(khz)));
  if (max_iters == 0) max_iters = ~0ull;
  detail::DeviceBuffer sink, result;
  sink.alloc(sizeof(unsigned int));
  result.alloc(2 * sizeof(unsigned long long));
  HIP_CHECK(hipMemset(result.p, 0, 2 * sizeof(unsigned long long)));
  int grid = prop.multiProcessorCount;  // one block per CU: full occupancy
  hipLaunchKernelGGL(busy_kernel, dim3(grid > 0 ? grid : 1), dim3(kBlock), 0, 0,
                     ticks, max_iters, sink.as<unsigned int>(),
                     result.as<unsigned long long>());
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipDeviceSynchronize());
  unsigned long long host[2] = {0, 0};
  HIP_CHECK(hipMemcpy(host, result.p, sizeof(host), hipMemcpyDeviceToHost));
  BusyResult r;
  r.elapsed_ms = static_cast<double>(host[0]) / static_cast<double>(khz);
  r.iters = host[1];
  r.guard_hit = host[1] >= max_iters;
  return r;
}

// Which XCDs executed our workgroups? Returns 8 counters that sum to blocks.
inline std::vector<unsigned int> run_xcd_census(int device = 0, int blocks = 4096) {
  if (blocks < 1 || blocks > (1 << 20))
    throw std::invalid_argument("run_xcd_census: blocks must be in 1 .. 1048576");
  HIP_CHECK(hipSetDevice(device));
  detail::DeviceBuffer per_xcd;
  per_xcd.alloc(8 * sizeof(unsigned int));
  HIP_CHECK(hipMemset(per_xcd.p, 0, 8 * sizeof(unsigned int)));
  hipLaunchKernelGGL(xcd_census_kernel, dim3(blocks), dim3(kBlock), 0, 0,
                     per_xcd.as<unsigned int>());
  HIP_CHECK(hipGetLastError());
  std::vector<unsigned int> host(8);
  HIP_CHECK(hipMemcpy(host.data(), per_xcd.p, 8 * sizeof(unsigned int),
                      hipMemcpyDeviceToHost));
  return host;
}

inline DeviceInfo get_device_info(int device = 0) {
  DeviceInfo info;
  info.device = device;
  HIP_CHECK(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIP_CHECK(hipGetDeviceProperties(&prop, device));
  info.name = prop.name;
  info.gcn_arch = prop.gcnArchName;
  info.cu_count = prop.multiProcessorCount;
  info.total_mem_gb = static_cast<double>(prop.totalGlobalMem) / (1024.0 * 1024.0 * 1024.0);
  auto census = run_xcd_census(device, 2048);
  int xcds = 0;
  for (unsigned int c : census)
    if (c) ++xcds;
  info.xcd_count_visible = xcds;
  return info;
}

inline int device_count() {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) return 0;
  return n;
}

}  // namespace payload

// bf16 MFMA GEMM payload: uses HIP_CHECK, kBlock and the detail helpers from
// above, detail::time_launches among them
#include "payload_gemm.hpp"

// MXFP8 block-scaled MFMA GEMM payload: same helpers, plus the gemm pattern
#include "payload_mxgemm.hpp"

// MXFP4 block-scaled MFMA GEMM payload: the MXFP8 one's LDS and scale images,
// pattern and limits
#include "payload_mxfp4.hpp"

// memcheck payload: also uses grid_for
#include "payload_memcheck.hpp"

// decode attention payload: bf16x8, f32x4, to_bf16_rne and the detail helpers.
// It also holds what both attention payloads share on the host: the common
// shape limits (detail::AttnShape), the fp64 reference row, the check result
// and its bound
#include "payload_attn.hpp"

// prefill attention payload: the decode one's head dim, patterns, scale and
// shared host pieces
#include "payload_prefill.hpp"
