// gfx950 INT8 matrix-core (MFMA) GEMM payload, raw int32 and W8A8.
//
// gemm, mxgemm, mx4gemm and dgemm prove the floating-point matrix paths; this
// one proves the integer one, the datapath an inference tenant runs a
// W8A8-quantised model on. C[M,N] = A[M,K] · B[K,N] with int8 operands and
// int32 accumulation on v_mfma_i32_32x32x32_i8: another instruction family, an
// int32 accumulator, and the 32 x 32 tile shape no other GEMM payload uses. An
// integer result is right or wrong, never close.
//
//   block tile   128 x 128, K-step 128 int8, 256 threads (4 wave64s as 2 x 2)
//   wave tile    64 x 64 = 2 x 2 MFMA tiles of 32 x 32, 16 int32 per lane
//                each: 64 accumulator registers
//   staging      the bf16 kernel's: a K-step row of 128 int8 is again 128
//                bytes, so 8 lanes x 16 bytes cover a row, 4 loads per thread
//                per operand; the loads for K-step t+1 are issued before the
//                MFMAs of step t and written to LDS after them
//   fragments    one MFMA takes 16 int8 per lane: lane l supplies row (A) or
//                column (B) l & 31 and the 16 consecutive bytes of k-half
//                l >> 5. A K-step is four sub-steps of 32 k; in sub-step s the
//                lane reads slot 2 s + (l >> 5) of its row, one ds_read_b128.
//                Which k a byte stands for inside one MFMA does not matter to
//                a sum over k, as long as A and B agree, and both index the
//                same slot. Per sub-step and wave: 2 reads for A, 2 for B, 4
//                MFMAs; per K-step 16 ds_read_b128 and 16 MFMAs.
//   LDS image    [128 rows][8 slots of 16 bytes] per operand, the slot index
//                XORed with (row >> 1) & 7: gemm_lds_off's rule, counted in
//                slots (igemm_lds_slot). The rule was derived for the 16 lanes
//                of one ds_read_b128 phase reading 16 consecutive rows at one
//                slot index, and that is still what a phase sees here: a
//                fragment's 32 rows start at a multiple of 32 and lanes 0..15,
//                16..31, 32..47, 48..63 read rows 0..15, 16..31, 0..15, 16..31
//                of it, each group at one slot index. 16 consecutive rows from
//                a multiple of 16 are 8 row pairs with 8 different XOR values,
//                and the two rows of a pair are 128 bytes apart, so the 16
//                reads cover the 16 slots of 2 x 8 of a 256-byte bank row:
//                conflict-free by the 256-byte rule for ds_read_b128. The
//                staging writes are the bf16 kernel's own.
//   C/D map      col = l & 31, row = 8 * (reg >> 2) + 4 * (l >> 5) + (reg & 3)
//                (profiles/igemm_probe.md)
//   epilogues    one template, kDequant false: the int32 accumulators as they
//                stand. kDequant true (W8A8): (float(acc) * sa[row]) * sb[col]
//                in fp32, the conversion round-to-nearest-even, two separate
//                multiplications in that order. A lane loads its two sb values
//                once and an sa value per tile row, straight from global
//                memory.
//
// No int32 partial sum can wrap: K is at most kIgemmMaxK = 131071 in every
// entry point, and 131071 * 128 * 128 < 2^31.
//
// The host stores B transposed (N x K, K-contiguous) and zero-pads M, N to 128
// and K to 128, sa and sb with 1.0: the kernel has no edge branch and no
// address outside its buffers for any shape. Only the M x N region is copied
// back.
//
// Included by payload_core.hpp after payload_gemm.hpp (needs its
// gemm_lds_off, detail::GemmShape, the three drivers, GemmResult and
// PatternErr).

#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <type_traits>

namespace payload {

typedef int i32x4 __attribute__((ext_vector_type(4)));    // one LDS slot: 16 int8
typedef int i32x16 __attribute__((ext_vector_type(16)));  // one MFMA tile's share

constexpr int kIgemmBK = 128;                                // int8 per K-step
constexpr int kIgemmSlots = kIgemmBK / 16;                   // 16-byte slots per row
constexpr int kIgemmLoads = kGemmBM * kIgemmSlots / kBlock;  // per thread per operand
constexpr int kIgemmMaxK = 131071;

static_assert(kIgemmBK * sizeof(int8_t) == kGemmBK * sizeof(uint16_t),
              "a K-step row is 128 bytes, as in the bf16 kernel");
static_assert(kIgemmSlots == 8, "gemm_lds_off's swizzle assumes 8 slots per row");
static_assert(kGemmBM * kIgemmSlots % kBlock == 0, "whole passes only");
static_assert(int64_t{kIgemmMaxK} * 128 * 128 < (int64_t{1} << 31),
              "no int32 partial sum of int8 products can wrap");
static_assert((int64_t{kIgemmMaxK} + 1) * 128 * 128 >= (int64_t{1} << 31),
              "and one more k could");

// ---- kernel --------------------------------------------------------------

// index (in 16-byte slots) of slot `slot` of row `row` in an LDS tile:
// gemm_lds_off counts bf16 elements, 8 to a slot
__device__ __forceinline__ int igemm_lds_slot(int row, int slot) {
  return gemm_lds_off(row, slot) >> 3;
}

// a: Mp x Kp, bt: Np x Kp (B transposed), c: Mp x Np (int32, or float when
// kDequant), sa: Mp, sb: Np (read only when kDequant); Mp, Np, Kp multiples of
// 128. grid = (Np / 128, Mp / 128). Every offset is a size_t: what bounds the
// shape is the grid and the two int arguments.
template <bool kDequant>
__global__ __launch_bounds__(kBlock) void gemm_i8_kernel(
    const int8_t* __restrict__ a, const int8_t* __restrict__ bt,
    std::conditional_t<kDequant, float, int32_t>* __restrict__ c,
    const float* __restrict__ sa, const float* __restrict__ sb, int Np, int Kp) {
  __shared__ __attribute__((aligned(16))) i32x4 lds[(kGemmBM + kGemmBN) * kIgemmSlots];
  i32x4* lds_a = lds;
  i32x4* lds_b = lds + kGemmBM * kIgemmSlots;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;  // wave's 64x64 quadrant
  const int fr = lane & 31, fh = lane >> 5;

  // staging map: 8 consecutive lanes cover one 128-byte row of the K-step
  const int srow = tid >> 3, sslot = tid & 7;
  const size_t brow = static_cast<size_t>(blockIdx.y) * kGemmBM;
  const size_t bcol = static_cast<size_t>(blockIdx.x) * kGemmBN;
  const int8_t* ga = a + (brow + srow) * Kp + sslot * 16;
  const int8_t* gb = bt + (bcol + srow) * Kp + sslot * 16;
  const size_t pass = static_cast<size_t>(kBlock / kIgemmSlots) * Kp;  // 32 rows

  i32x4 ra[kIgemmLoads], rb[kIgemmLoads];
#pragma unroll
  for (int i = 0; i < kIgemmLoads; ++i) {
    ra[i] = *reinterpret_cast<const i32x4*>(ga + i * pass);
    rb[i] = *reinterpret_cast<const i32x4*>(gb + i * pass);
  }

  i32x16 acc[2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int j = 0; j < 16; ++j) acc[m][n][j] = 0;

  for (int k0 = 0; k0 < Kp; k0 += kIgemmBK) {
#pragma unroll
    for (int i = 0; i < kIgemmLoads; ++i) {
      int row = srow + i * (kBlock / kIgemmSlots);
      lds_a[igemm_lds_slot(row, sslot)] = ra[i];
      lds_b[igemm_lds_slot(row, sslot)] = rb[i];
    }
    __syncthreads();

    if (k0 + kIgemmBK < Kp) {  // block-uniform: prefetch the next K-step
#pragma unroll
      for (int i = 0; i < kIgemmLoads; ++i) {
        ra[i] = *reinterpret_cast<const i32x4*>(ga + k0 + kIgemmBK + i * pass);
        rb[i] = *reinterpret_cast<const i32x4*>(gb + k0 + kIgemmBK + i * pass);
      }
    }

#pragma unroll
    for (int s = 0; s < kIgemmSlots / 2; ++s) {
      // lane l: A[row l&31][slot 2s + (l>>5)], B[slot 2s + (l>>5)][col l&31]
      i32x4 fa[2], fb[2];
#pragma unroll
      for (int m = 0; m < 2; ++m)
        fa[m] = lds_a[igemm_lds_slot(wr * 64 + m * 32 + fr, s * 2 + fh)];
#pragma unroll
      for (int n = 0; n < 2; ++n)
        fb[n] = lds_b[igemm_lds_slot(wc * 64 + n * 32 + fr, s * 2 + fh)];
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
          acc[m][n] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[m], fb[n], acc[m][n],
                                                            0, 0, 0);
    }
    __syncthreads();  // all fragment reads done before the next ds_write
  }

  // C/D map: col = lane & 31, row = 8 * (reg >> 2) + 4 * (lane >> 5) + (reg & 3)
  float sbv[2];
  if constexpr (kDequant) {
#pragma unroll
    for (int n = 0; n < 2; ++n) sbv[n] = sb[bcol + wc * 64 + n * 32 + fr];
  }
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      size_t row = brow + wr * 64 + m * 32 + (j >> 2) * 8 + fh * 4 + (j & 3);
      float sav = 0.f;
      if constexpr (kDequant) sav = sa[row];
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        size_t col = bcol + wc * 64 + n * 32 + fr;
        if constexpr (kDequant) {
          float scaled = static_cast<float>(acc[m][n][j]) * sav;
          c[row * Np + col] = scaled * sbv[n];
        } else {
          c[row * Np + col] = acc[m][n][j];
        }
      }
    }
}

// ---- host layer ----------------------------------------------------------

// Symmetric per-row int8 quantisation of one row of k floats, host only:
// scale = absmax / 127 in fp32, code = clamp(nearbyint(x / scale), -127, 127)
// with an fp32 division and round-to-nearest-even, so -128 is never a code.
// Where the quotient absmax / 127 is zero the scale is 1.0 and every code 0:
// the all-zero row, and a row of subnormals so small that the quotient rounds
// to zero. Throws std::invalid_argument on a non-finite element.
inline void quantize_i8_row(const float* x, int k, int8_t* codes, float* scale) {
  float absmax = 0.f;
  for (int i = 0; i < k; ++i) {
    if (!std::isfinite(x[i]))
      throw std::invalid_argument("quantize_i8: x has a non-finite element");
    absmax = std::fmax(absmax, std::fabs(x[i]));
  }
  float s = absmax / 127.0f;
  if (s == 0.f) s = 1.0f;
  for (int i = 0; i < k; ++i) {
    float q = std::nearbyint(x[i] / s);  // the default rounding mode: to even
    codes[i] = static_cast<int8_t>(std::fmin(std::fmax(q, -127.0f), 127.0f));
  }
  *scale = s;
}

namespace detail {

// the padded K of kIgemmMaxK
constexpr size_t kIgemmMaxKp = 131072;
static_assert(kIgemmMaxKp % kIgemmBK == 0 && kIgemmMaxKp >= kIgemmMaxK &&
                  kIgemmMaxKp - kIgemmBK < kIgemmMaxK,
              "kIgemmMaxK rounded up to the K-step");

// k, or std::invalid_argument beyond the depth at which int32 could wrap
inline int igemm_k(int k) {
  if (k > kIgemmMaxK)
    throw std::invalid_argument("igemm: K must be <= 131071 (beyond it an int32 "
                                "sum of int8 products can wrap)");
  return k;
}

// Padded int8 operands on the host plus their device images; with `dequant`,
// the W8A8 scales too (padded with 1.0) and C is float. The limits on Mp
// (grid.y) and Np (an int argument) are GemmShape's.
struct IgemmProblem : GemmShape {
  std::vector<int8_t> a, bt;  // Mp x Kp, Np x Kp, zero-padded
  std::vector<float> sa, sb;  // Mp, Np when dequant, else empty
  bool dequant;
  DeviceBuffer da, dbt, dsa, dsb;

  IgemmProblem(int m, int n, int k, bool dequant_ = false)
      : GemmShape("igemm", m, n, igemm_k(k), kIgemmBK, kIgemmMaxKp), dequant(dequant_) {
    a.assign(Mp * Kp, 0);
    bt.assign(Np * Kp, 0);
    if (dequant) {
      sa.assign(Mp, 1.0f);
      sb.assign(Np, 1.0f);
    }
  }

  // row-major a (M x K) and b (K x N) into the padded images
  void fill(const int8_t* pa, const int8_t* pb) {
    for (int i = 0; i < M; ++i)
      for (int k = 0; k < K; ++k) a[i * Kp + k] = pa[static_cast<size_t>(i) * K + k];
    for (int k = 0; k < K; ++k)
      for (int j = 0; j < N; ++j) bt[j * Kp + k] = pb[static_cast<size_t>(k) * N + j];
  }

  void upload(int device) {
    HIP_CHECK(hipSetDevice(device));
    da.alloc(a.size());
    dbt.alloc(bt.size());
    dc.alloc(Mp * Np * sizeof(int32_t));  // float is as wide
    HIP_CHECK(hipMemcpy(da.p, a.data(), a.size(), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dbt.p, bt.data(), bt.size(), hipMemcpyHostToDevice));
    if (dequant) {
      dsa.alloc(sa.size() * sizeof(float));
      dsb.alloc(sb.size() * sizeof(float));
      HIP_CHECK(hipMemcpy(dsa.p, sa.data(), sa.size() * sizeof(float),
                          hipMemcpyHostToDevice));
      HIP_CHECK(hipMemcpy(dsb.p, sb.data(), sb.size() * sizeof(float),
                          hipMemcpyHostToDevice));
    }
  }

  void launch() const {
    const int np = static_cast<int>(Np), kp = static_cast<int>(Kp);
    if (dequant)
      hipLaunchKernelGGL(gemm_i8_kernel<true>, grid(), dim3(kBlock), 0, 0,
                         da.as<const int8_t>(), dbt.as<const int8_t>(), dc.as<float>(),
                         dsa.as<const float>(), dsb.as<const float>(), np, kp);
    else
      hipLaunchKernelGGL(gemm_i8_kernel<false>, grid(), dim3(kBlock), 0, 0,
                         da.as<const int8_t>(), dbt.as<const int8_t>(),
                         dc.as<int32_t>(), dsa.as<const float>(),
                         dsb.as<const float>(), np, kp);  // both null, never read
  }
};

static_assert(sizeof(float) == sizeof(int32_t), "one C buffer serves both epilogues");

// The exact pattern: the multipliers are odd, so every row and column walks
// through all 256 int8 values, -128 included.
inline int igemm_pat_a(int i, int k) {
  return static_cast<int>((37ll * i + 101ll * k) % 256) - 128;
}
inline int igemm_pat_b(int k, int j) {
  return static_cast<int>((59ll * k + 113ll * j) % 256) - 128;
}

inline void fill_igemm_pattern(IgemmProblem& p) {
  for (int i = 0; i < p.M; ++i)
    for (int k = 0; k < p.K; ++k)
      p.a[i * p.Kp + k] = static_cast<int8_t>(igemm_pat_a(i, k));
  for (int j = 0; j < p.N; ++j)
    for (int k = 0; k < p.K; ++k)
      p.bt[j * p.Kp + k] = static_cast<int8_t>(igemm_pat_b(k, j));
}

// |got - exact|, the exact result an int64 sum
inline double igemm_pattern_err(int32_t got, int i, int j, int K) {
  int64_t s = 0;
  for (int k = 0; k < K; ++k)
    s += static_cast<int64_t>(igemm_pat_a(i, k)) * igemm_pat_b(k, j);
  return std::fabs(static_cast<double>(got) - static_cast<double>(s));
}

}  // namespace detail

// General entry: c[M,N] (int32) = a[M,K] · b[K,N], all row-major. Throws
// std::invalid_argument on K > kIgemmMaxK, before any device work.
inline void gemm_i8(const int8_t* a, const int8_t* b, int32_t* c, int M, int N,
                    int K, int device = 0) {
  detail::IgemmProblem p(M, N, K);
  p.fill(a, b);
  detail::run_once(p, device, c);
}

// W8A8 entry: c[i,j] (float) = (float(sum_k a[i,k] b[k,j]) * sa[i]) * sb[j]:
// the int32 sum converted round-to-nearest-even, then two fp32 products in
// that order. sa: M per-row (per-token) scales, sb: N per-column (per-channel)
// scales. Throws std::invalid_argument on K > kIgemmMaxK or a non-finite scale,
// before any device work.
inline void gemm_w8a8(const int8_t* a, const int8_t* b, const float* sa,
                      const float* sb, float* c, int M, int N, int K, int device = 0) {
  for (int i = 0; i < M; ++i)
    if (!std::isfinite(sa[i]))
      throw std::invalid_argument("gemm_w8a8: sa has a non-finite element");
  for (int j = 0; j < N; ++j)
    if (!std::isfinite(sb[j]))
      throw std::invalid_argument("gemm_w8a8: sb has a non-finite element");
  detail::IgemmProblem p(M, N, K, true);
  std::copy(sa, sa + M, p.sa.begin());
  std::copy(sb, sb + N, p.sb.begin());
  p.fill(a, b);
  detail::run_once(p, device, c);
}

// Self-contained exact check of the raw int32 kernel on the pattern above,
// host reference in int64; returns max |C - ref| over the whole M x N result
// (expect 0.0).
inline double run_igemm_check(int M, int N, int K, int device = 0) {
  detail::IgemmProblem p(M, N, K);
  detail::fill_igemm_pattern(p);
  return detail::run_full_check(p, device, detail::igemm_pattern_err);
}

// Timed run on the same pattern: one warm-up launch, `iters` launches between
// events, then 256 fixed, spread output elements are checked exactly, so a
// fast wrong kernel cannot report a rate. GemmResult::tflops carries 2 M N K
// integer operations per second in units of 10^12.
inline GemmResult run_igemm(int M = 4096, int N = 4096, int K = 4096,
                            int iters = 10, int device = 0) {
  if (iters < 1) throw std::invalid_argument("run_igemm: iters must be >= 1");
  detail::IgemmProblem p(M, N, K);
  detail::fill_igemm_pattern(p);
  return detail::run_timed(p, iters, device, detail::igemm_pattern_err);
}

}  // namespace payload
