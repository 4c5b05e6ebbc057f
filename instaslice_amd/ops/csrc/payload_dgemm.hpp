// gfx950 FP64 matrix-core (MFMA) GEMM payload.
//
// gemm, mxgemm and mx4gemm prove the low-precision matrix paths, which all
// accumulate in fp32; this one proves the double-precision one, the datapath
// an HPC tenant runs DGEMM on. C[M,N] (fp64) = A[M,K] · B[K,N] with fp64
// operands and fp64 accumulation on v_mfma_f64_16x16x4_f64: another
// instruction, operand width and accumulator layout than the bf16 MFMA.
//
//   block tile   128 x 128, K-step 16, 256 threads (4 wave64s as 2 x 2)
//   wave tile    64 x 64 = 4 x 4 MFMA tiles of 16 x 16, 4 doubles per lane
//                each: 128 accumulator registers
//   staging      the bf16 kernel's: a K-step row of 16 doubles is again 128
//                bytes, so 8 lanes x 16 bytes cover a row, 4 loads per thread
//                per operand; the loads for K-step t+1 are issued before the
//                MFMAs of step t and written to LDS after them
//   LDS image    [128 rows][8 slots of 16 bytes] per operand, the slot index
//                XORed with (row >> 1) & 7: gemm_lds_off's rule, counted in
//                slots (dgemm_lds_slot)
//   fragments    one MFMA takes ONE double per lane, A[row l & 15][k l >> 4]
//                and B[k l >> 4][col l & 15]. Reading 8 bytes per MFMA would
//                double the LDS instructions, so a lane reads a whole slot
//                (ds_read_b128, two consecutive k) per fragment and feeds its
//                two doubles to two consecutive MFMAs: the lane in quarter q
//                takes slot 4 g + q of its row (g = 0, 1), k = 8 g + 2 q + h
//                in MFMA h of the pair. Within one MFMA the four quarters then
//                hold k = 8 g + h + {0, 2, 4, 6}, not four consecutive k; a
//                sum over k does not care, as long as A and B use the same
//                (g, h, q) -> k map, which they do: both index the same slot.
//                Per K-step and wave: 16 ds_read_b128, 64 MFMAs.
//   C/D map      col = l & 15, row = 4 * reg + (l >> 4): the four doubles of
//                a lane are four rows 4 apart, not the four consecutive rows
//                of the bf16 MFMA (profiles/dgemm_probe.md)
//
// The host stores B transposed (N x K, K-contiguous) and zero-pads M, N to 128
// and K to 16: the kernel has no edge branch and no address outside its
// buffers for any shape. Only the M x N region is copied back.
//
// Included by payload_core.hpp after payload_gemm.hpp (needs its
// gemm_lds_off, detail::GemmShape, the three drivers, gemm_pat_a / _b and
// GemmResult).

#pragma once

#include <cmath>
#include <cstdint>

namespace payload {

typedef double f64x2 __attribute__((ext_vector_type(2)));  // one LDS slot, 4 VGPRs
typedef double f64x4 __attribute__((ext_vector_type(4)));  // one MFMA tile's share

constexpr int kDgemmBK = 16;                                 // doubles per K-step
constexpr int kDgemmSlots = kDgemmBK / 2;                    // 16-byte slots per row
constexpr int kDgemmLoads = kGemmBM * kDgemmSlots / kBlock;  // per thread per operand

static_assert(kDgemmBK * sizeof(double) == kGemmBK * sizeof(uint16_t),
              "a K-step row is 128 bytes, as in the bf16 kernel");
static_assert(kDgemmSlots == 8, "gemm_lds_off's swizzle assumes 8 slots per row");
static_assert(kGemmBM * kDgemmSlots % kBlock == 0, "whole passes only");

// ---- kernel --------------------------------------------------------------

// index (in 16-byte slots) of slot `slot` of row `row` in an LDS tile:
// gemm_lds_off counts bf16 elements, 8 to a slot
__device__ __forceinline__ int dgemm_lds_slot(int row, int slot) {
  return gemm_lds_off(row, slot) >> 3;
}

// a: Mp x Kp, bt: Np x Kp (B transposed), c: Mp x Np; Mp, Np multiples of 128,
// Kp a multiple of 16. grid = (Np / 128, Mp / 128). Every offset is a size_t:
// what bounds the shape is the grid and the two int arguments.
__global__ __launch_bounds__(kBlock) void gemm_f64_kernel(
    const double* __restrict__ a, const double* __restrict__ bt,
    double* __restrict__ c, int Np, int Kp) {
  __shared__ __attribute__((aligned(16))) f64x2 lds[(kGemmBM + kGemmBN) * kDgemmSlots];
  f64x2* lds_a = lds;
  f64x2* lds_b = lds + kGemmBM * kDgemmSlots;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;  // wave's 64x64 quadrant
  const int fr = lane & 15, fq = lane >> 4;

  // staging map: 8 consecutive lanes cover one 128-byte row of the K-step
  const int srow = tid >> 3, sslot = tid & 7;
  const size_t brow = static_cast<size_t>(blockIdx.y) * kGemmBM;
  const size_t bcol = static_cast<size_t>(blockIdx.x) * kGemmBN;
  const double* ga = a + (brow + srow) * Kp + sslot * 2;
  const double* gb = bt + (bcol + srow) * Kp + sslot * 2;
  const size_t pass = static_cast<size_t>(kBlock / kDgemmSlots) * Kp;  // 32 rows

  f64x2 ra[kDgemmLoads], rb[kDgemmLoads];
#pragma unroll
  for (int i = 0; i < kDgemmLoads; ++i) {
    ra[i] = *reinterpret_cast<const f64x2*>(ga + i * pass);
    rb[i] = *reinterpret_cast<const f64x2*>(gb + i * pass);
  }

  f64x4 acc[4][4];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[m][n] = f64x4{0., 0., 0., 0.};

  for (int k0 = 0; k0 < Kp; k0 += kDgemmBK) {
#pragma unroll
    for (int i = 0; i < kDgemmLoads; ++i) {
      int row = srow + i * (kBlock / kDgemmSlots);
      lds_a[dgemm_lds_slot(row, sslot)] = ra[i];
      lds_b[dgemm_lds_slot(row, sslot)] = rb[i];
    }
    __syncthreads();

    if (k0 + kDgemmBK < Kp) {  // block-uniform: prefetch the next K-step
#pragma unroll
      for (int i = 0; i < kDgemmLoads; ++i) {
        ra[i] = *reinterpret_cast<const f64x2*>(ga + k0 + kDgemmBK + i * pass);
        rb[i] = *reinterpret_cast<const f64x2*>(gb + k0 + kDgemmBK + i * pass);
      }
    }

#pragma unroll
    for (int g = 0; g < kDgemmSlots / 4; ++g) {
      // lane l, MFMA h of the pair: A[row l&15][k = 8g + 2(l>>4) + h],
      // B[k = 8g + 2(l>>4) + h][col l&15]
      f64x2 fa[4], fb[4];
#pragma unroll
      for (int m = 0; m < 4; ++m)
        fa[m] = lds_a[dgemm_lds_slot(wr * 64 + m * 16 + fr, g * 4 + fq)];
#pragma unroll
      for (int n = 0; n < 4; ++n)
        fb[n] = lds_b[dgemm_lds_slot(wc * 64 + n * 16 + fr, g * 4 + fq)];
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
          for (int n = 0; n < 4; ++n)
            acc[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[m][h], fb[n][h],
                                                             acc[m][n], 0, 0, 0);
    }
    __syncthreads();  // all fragment reads done before the next ds_write
  }

  // C/D map: col = lane & 15, row = 4 * reg + (lane >> 4)
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        size_t row = brow + wr * 64 + m * 16 + j * 4 + fq;
        size_t col = bcol + wc * 64 + n * 16 + fr;
        c[row * Np + col] = acc[m][n][j];
      }
}

// ---- host layer ----------------------------------------------------------

// The exact pattern, made to need fp64. In units of 2^-16 an operand is the
// integer pa(i,k) * 2^16 + pa(i+2,k+1), with pa (gemm_pat_a / _b) in [-4, 4]:
// at most kDgemmPatMax in magnitude, 19 bits, exact in fp64. A product is an
// integer of at most kDgemmPatMax^2 (just above 2^36) units of 2^-32, and so is
// every partial sum of K of them in any order: all exact in fp64 as long as
// K * kDgemmPatMax^2 < 2^53. kDgemmMaxExactK is the largest power of two that
// satisfies it. At K = 1024 a result spans 46 bits: a multiply or an
// accumulation in fp32 or anything narrower cannot produce it.
constexpr int64_t kDgemmPatMax = 4 * 65536 + 4;
constexpr int kDgemmMaxExactK = 65536;
static_assert(kDgemmMaxExactK * kDgemmPatMax * kDgemmPatMax < (int64_t{1} << 53),
              "every partial sum of the pattern is exact in fp64");
static_assert(2 * kDgemmMaxExactK * kDgemmPatMax * kDgemmPatMax >= (int64_t{1} << 53),
              "and the next power of two is not");

namespace detail {

// the largest Kp gemm_f64_kernel's int argument allows
constexpr size_t kDgemmMaxKp = 0x7FFFFFF0u;
static_assert(kDgemmMaxKp % kDgemmBK == 0 && kDgemmMaxKp + kDgemmBK > 0x7FFFFFFFu,
              "the largest multiple of the K-step that is an int");

// Padded fp64 operands on the host plus their device images. The limits on
// Mp (grid.y) and Np (an int argument) are GemmShape's.
struct DgemmProblem : GemmShape {
  std::vector<double> a, bt;  // Mp x Kp, Np x Kp, zero-padded
  DeviceBuffer da, dbt;

  DgemmProblem(int m, int n, int k)
      : GemmShape("dgemm", m, n, k, kDgemmBK, kDgemmMaxKp) {
    a.assign(Mp * Kp, 0.0);
    bt.assign(Np * Kp, 0.0);
  }

  void upload(int device) {
    HIP_CHECK(hipSetDevice(device));
    da.alloc(a.size() * sizeof(double));
    dbt.alloc(bt.size() * sizeof(double));
    dc.alloc(Mp * Np * sizeof(double));
    HIP_CHECK(hipMemcpy(da.p, a.data(), a.size() * sizeof(double),
                        hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dbt.p, bt.data(), bt.size() * sizeof(double),
                        hipMemcpyHostToDevice));
  }

  void launch() const {
    hipLaunchKernelGGL(gemm_f64_kernel, grid(), dim3(kBlock), 0, 0,
                       da.as<const double>(), dbt.as<const double>(),
                       dc.as<double>(), static_cast<int>(Np), static_cast<int>(Kp));
  }
};

// the pattern's operands in units of 2^-16
inline int64_t dgemm_pat_a(int i, int k) {
  return gemm_pat_a(i, k) * int64_t{65536} + gemm_pat_a(i + 2, k + 1);
}
inline int64_t dgemm_pat_b(int k, int j) {
  return gemm_pat_b(k, j) * int64_t{65536} + gemm_pat_b(k + 3, j + 1);
}

inline void fill_dgemm_pattern(DgemmProblem& p) {
  for (int i = 0; i < p.M; ++i)
    for (int k = 0; k < p.K; ++k)
      p.a[i * p.Kp + k] = std::ldexp(static_cast<double>(dgemm_pat_a(i, k)), -16);
  for (int j = 0; j < p.N; ++j)
    for (int k = 0; k < p.K; ++k)
      p.bt[j * p.Kp + k] = std::ldexp(static_cast<double>(dgemm_pat_b(k, j)), -16);
}

// |got - exact|, the exact result an int64 sum in units of 2^-32 (below 2^53,
// so its conversion to double is exact too)
inline double dgemm_pattern_err(double got, int i, int j, int K) {
  int64_t s = 0;
  for (int k = 0; k < K; ++k) s += dgemm_pat_a(i, k) * dgemm_pat_b(k, j);
  return std::fabs(got - std::ldexp(static_cast<double>(s), -32));
}

inline void require_exact_dgemm_k(int k, const char* who) {
  if (k > kDgemmMaxExactK)
    throw std::invalid_argument(std::string(who) + ": K must be <= 65536 "
                                "(the 2^-16 pattern is exact in fp64 only up to there)");
}

}  // namespace detail

// General entry: c[M,N] = a[M,K] · b[K,N], all row-major double. Throws
// std::invalid_argument on a non-finite input, before any device work.
inline void gemm_f64(const double* a, const double* b, double* c, int M, int N,
                     int K, int device = 0) {
  detail::DgemmProblem p(M, N, K);
  for (size_t i = 0, n = static_cast<size_t>(M) * K; i < n; ++i)
    if (!std::isfinite(a[i]))
      throw std::invalid_argument("gemm_f64: a has a non-finite element");
  for (size_t i = 0, n = static_cast<size_t>(K) * N; i < n; ++i)
    if (!std::isfinite(b[i]))
      throw std::invalid_argument("gemm_f64: b has a non-finite element");
  for (int i = 0; i < M; ++i)
    for (int k = 0; k < K; ++k) p.a[i * p.Kp + k] = a[static_cast<size_t>(i) * K + k];
  for (int k = 0; k < K; ++k)
    for (int j = 0; j < N; ++j) p.bt[j * p.Kp + k] = b[static_cast<size_t>(k) * N + j];
  detail::run_once(p, device, c);
}

// Self-contained exact check on the 2^-16 pattern above, host reference in
// int64; returns max |C - ref| over the whole M x N result (expect 0.0).
inline double run_dgemm_check(int M, int N, int K, int device = 0) {
  detail::require_exact_dgemm_k(K, "run_dgemm_check");
  detail::DgemmProblem p(M, N, K);
  detail::fill_dgemm_pattern(p);
  return detail::run_full_check(p, device, detail::dgemm_pattern_err);
}

// Timed run on the same pattern: one warm-up launch, `iters` launches between
// events, then 256 fixed, spread output elements are checked exactly, so a
// fast wrong kernel cannot report a rate. FLOPs are counted as 2 M N K.
inline GemmResult run_dgemm(int M = 4096, int N = 4096, int K = 1024,
                            int iters = 10, int device = 0) {
  detail::require_exact_dgemm_k(K, "run_dgemm");
  if (iters < 1) throw std::invalid_argument("run_dgemm: iters must be >= 1");
  detail::DgemmProblem p(M, N, K);
  detail::fill_dgemm_pattern(p);
  return detail::run_timed(p, iters, device, detail::dgemm_pattern_err);
}

}  // namespace payload
