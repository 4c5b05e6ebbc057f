// gfx950 bf16 matrix-core (MFMA) GEMM payload.
//
// vecadd / membw / xcd_census prove a partition is visible and fed; this one
// proves its matrix cores compute. C[M,N] (fp32) = A[M,K] · B[K,N] with bf16
// inputs and fp32 accumulation on v_mfma_f32_16x16x32_bf16.
//
//   block tile   128 x 128, K-step 64, 256 threads (4 wave64s as 2 x 2)
//   wave tile    64 x 64 = 4 x 4 MFMA tiles of 16 x 16 (64 accumulator VGPRs)
//   staging      16-byte global loads -> registers -> ds_write_b128 into one
//                LDS buffer per operand; the loads for K-step t+1 are issued
//                before the MFMAs of step t and written after them
//   LDS image    [128 rows][64 bf16] (128-byte rows), the 16-byte slot index
//                XORed with (row >> 1) & 7 so the 16 rows one ds_read_b128
//                lane group touches fall on 16 distinct slots of the bank row
//                (cdna_hip_programming.md §2 LDS, §5.5 T2). Register staging,
//                so the swizzle sits on the LDS address of both sides.
//
// The host stores B transposed (N x K, K-contiguous) so a lane's 8-element
// fragment is one contiguous 16-byte run for both operands, and zero-pads
// M, N to 128 and K to 64: the kernel has no edge branch and no address
// outside its buffers for any shape. Only the M x N region is copied back.
//
// Included by payload_core.hpp (needs its HIP_CHECK, kBlock, detail::DeviceBuffer
// and detail::time_launches).

#pragma once

#include <cmath>
#include <cstring>

namespace payload {

typedef short bf16x8 __attribute__((ext_vector_type(8)));  // 8 bf16, 4 VGPRs
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kGemmBM = 128;
constexpr int kGemmBN = 128;
constexpr int kGemmBK = 64;
constexpr int kGemmSlots = kGemmBK / 8;                    // 16-byte slots per row
constexpr int kGemmLoads = kGemmBM * kGemmSlots / kBlock;  // per thread per operand
constexpr int kGemmMaxExactK = 1024;  // 16 * K < 2^24: integer pattern exact in fp32

static_assert(kGemmBM == kGemmBN, "one staging index map serves both operands");
static_assert(kGemmSlots == 8, "swizzle below assumes 8 slots per row");
static_assert(kGemmBM * kGemmSlots % kBlock == 0, "whole passes only");

// ---- kernel --------------------------------------------------------------

// element offset (in bf16) of 16-byte slot `slot` of row `row` in an LDS tile
__device__ __forceinline__ int gemm_lds_off(int row, int slot) {
  return row * kGemmBK + ((slot ^ ((row >> 1) & 7)) << 3);
}

// a: Mp x Kp, bt: Np x Kp (B transposed), c: Mp x Np; Mp, Np multiples of 128,
// Kp a multiple of 64. grid = (Np / 128, Mp / 128).
__global__ __launch_bounds__(kBlock) void gemm_bf16_kernel(
    const uint16_t* __restrict__ a, const uint16_t* __restrict__ bt,
    float* __restrict__ c, int Np, int Kp) {
  __shared__ __attribute__((aligned(16))) uint16_t lds[(kGemmBM + kGemmBN) * kGemmBK];
  uint16_t* lds_a = lds;
  uint16_t* lds_b = lds + kGemmBM * kGemmBK;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;  // wave's 64x64 quadrant
  const int fr = lane & 15, fq = lane >> 4;

  // staging map: 8 consecutive lanes cover one 128-byte row of the K-step
  const int srow = tid >> 3, sslot = tid & 7;
  const size_t brow = static_cast<size_t>(blockIdx.y) * kGemmBM;
  const size_t bcol = static_cast<size_t>(blockIdx.x) * kGemmBN;
  const uint16_t* ga = a + (brow + srow) * Kp + sslot * 8;
  const uint16_t* gb = bt + (bcol + srow) * Kp + sslot * 8;
  const size_t pass = static_cast<size_t>(kBlock / kGemmSlots) * Kp;  // 32 rows

  bf16x8 ra[kGemmLoads], rb[kGemmLoads];
#pragma unroll
  for (int i = 0; i < kGemmLoads; ++i) {
    ra[i] = *reinterpret_cast<const bf16x8*>(ga + i * pass);
    rb[i] = *reinterpret_cast<const bf16x8*>(gb + i * pass);
  }

  f32x4 acc[4][4];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int k0 = 0; k0 < Kp; k0 += kGemmBK) {
#pragma unroll
    for (int i = 0; i < kGemmLoads; ++i) {
      int row = srow + i * (kBlock / kGemmSlots);
      *reinterpret_cast<bf16x8*>(lds_a + gemm_lds_off(row, sslot)) = ra[i];
      *reinterpret_cast<bf16x8*>(lds_b + gemm_lds_off(row, sslot)) = rb[i];
    }
    __syncthreads();

    if (k0 + kGemmBK < Kp) {  // block-uniform: prefetch the next K-step
#pragma unroll
      for (int i = 0; i < kGemmLoads; ++i) {
        ra[i] = *reinterpret_cast<const bf16x8*>(ga + k0 + kGemmBK + i * pass);
        rb[i] = *reinterpret_cast<const bf16x8*>(gb + k0 + kGemmBK + i * pass);
      }
    }

#pragma unroll
    for (int kk = 0; kk < kGemmBK / 32; ++kk) {
      // lane l: A[row l&15][k = 8(l>>4) + j], B[k = 8(l>>4) + j][col l&15]
      bf16x8 fa[4], fb[4];
#pragma unroll
      for (int m = 0; m < 4; ++m)
        fa[m] = *reinterpret_cast<const bf16x8*>(
            lds_a + gemm_lds_off(wr * 64 + m * 16 + fr, kk * 4 + fq));
#pragma unroll
      for (int n = 0; n < 4; ++n)
        fb[n] = *reinterpret_cast<const bf16x8*>(
            lds_b + gemm_lds_off(wc * 64 + n * 16 + fr, kk * 4 + fq));
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n)
          acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[m], fb[n],
                                                              acc[m][n], 0, 0, 0);
    }
    __syncthreads();  // all fragment reads done before the next ds_write
  }

  // C/D map: col = lane & 15, row = (lane >> 4) * 4 + reg
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        size_t row = brow + wr * 64 + m * 16 + fq * 4 + j;
        size_t col = bcol + wc * 64 + n * 16 + fr;
        c[row * Np + col] = acc[m][n][j];
      }
}

// ---- host layer ----------------------------------------------------------

// float -> bf16 bits, round-to-nearest-even. NaN stays a quiet NaN, +-inf and
// +-0 are preserved, subnormals are rounded (not flushed), and a finite value
// above the largest bf16 rounds to inf.
inline uint16_t to_bf16_rne(float f) {
  uint32_t u;
  std::memcpy(&u, &f, sizeof(u));
  if ((u & 0x7FFFFFFFu) > 0x7F800000u)
    return static_cast<uint16_t>((u >> 16) | 0x0040u);
  u += 0x7FFFu + ((u >> 16) & 1u);
  return static_cast<uint16_t>(u >> 16);
}

struct GemmResult {
  double tflops = 0;
  double max_err = 0;
};

namespace detail {

// DeviceBuffer and time_launches are payload_core.hpp's

inline size_t round_up(size_t v, size_t m) { return (v + m - 1) / m * m; }

// What the three GEMM payloads' problems share: the shape, the padded shape
// and the padded C. Each problem adds its padded operands, upload() and
// launch().
struct GemmShape {
  int M, N, K;
  size_t Mp, Np, Kp;
  DeviceBuffer dc;

  // who: the name used in messages; bk: the kernel's K-step in elements;
  // max_kp: the largest Kp the kernel's 32-bit offsets allow
  GemmShape(const std::string& who, int m, int n, int k, size_t bk, size_t max_kp)
      : M(m), N(n), K(k) {
    if (m < 1 || n < 1 || k < 1)
      throw std::invalid_argument(who + ": M, N and K must be >= 1");
    Mp = round_up(m, kGemmBM);
    Np = round_up(n, kGemmBN);
    Kp = round_up(k, bk);
    if (Mp / kGemmBM > 65535 || Np > 0x7FFFFF80u || Kp > max_kp)
      throw std::invalid_argument(who + ": shape too large");
  }

  // grid = (Np / 128, Mp / 128) for all three kernels
  dim3 grid() const {
    return dim3(static_cast<unsigned>(Np / kGemmBN), static_cast<unsigned>(Mp / kGemmBM));
  }

  // the un-padded M x N region, row-major, into c
  void download(float* c) const {
    HIP_CHECK(hipMemcpy2D(c, static_cast<size_t>(N) * sizeof(float), dc.p,
                          Np * sizeof(float), static_cast<size_t>(N) * sizeof(float),
                          M, hipMemcpyDeviceToHost));
  }
};

// Padded operands on the host plus their device images.
struct GemmProblem : GemmShape {
  std::vector<uint16_t> a, bt;  // Mp x Kp, Np x Kp, zero-padded
  DeviceBuffer da, dbt;

  GemmProblem(int m, int n, int k) : GemmShape("gemm", m, n, k, kGemmBK, 0x7FFFFFC0u) {
    a.assign(Mp * Kp, 0);
    bt.assign(Np * Kp, 0);
  }

  void upload(int device) {
    HIP_CHECK(hipSetDevice(device));
    da.alloc(a.size() * sizeof(uint16_t));
    dbt.alloc(bt.size() * sizeof(uint16_t));
    dc.alloc(Mp * Np * sizeof(float));
    HIP_CHECK(hipMemcpy(da.p, a.data(), a.size() * sizeof(uint16_t),
                        hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dbt.p, bt.data(), bt.size() * sizeof(uint16_t),
                        hipMemcpyHostToDevice));
  }

  void launch() const {
    hipLaunchKernelGGL(gemm_bf16_kernel, grid(), dim3(kBlock), 0, 0,
                       da.as<const uint16_t>(), dbt.as<const uint16_t>(),
                       dc.as<float>(), static_cast<int>(Np), static_cast<int>(Kp));
  }
};

inline int gemm_pat_a(int i, int k) {
  return static_cast<int>((3ll * i + 5ll * k) % 9) - 4;
}
inline int gemm_pat_b(int k, int j) {
  return static_cast<int>((7ll * k + 11ll * j) % 9) - 4;
}

inline void fill_pattern(GemmProblem& p) {
  for (int i = 0; i < p.M; ++i)
    for (int k = 0; k < p.K; ++k)
      p.a[i * p.Kp + k] = to_bf16_rne(static_cast<float>(gemm_pat_a(i, k)));
  for (int j = 0; j < p.N; ++j)
    for (int k = 0; k < p.K; ++k)
      p.bt[j * p.Kp + k] = to_bf16_rne(static_cast<float>(gemm_pat_b(k, j)));
}

inline int64_t pattern_dot(int i, int j, int K) {
  int64_t s = 0;
  for (int k = 0; k < K; ++k)
    s += static_cast<int64_t>(gemm_pat_a(i, k)) * gemm_pat_b(k, j);
  return s;
}

inline double pattern_err(float got, int i, int j, int K) {
  return std::fabs(static_cast<double>(got) -
                   static_cast<double>(pattern_dot(i, j, K)));
}

// a NaN result is an error, not a skipped comparison
inline void note_err(double& max_err, double e) {
  if (std::isnan(e)) e = INFINITY;
  if (e > max_err) max_err = e;
}

inline void require_exact_k(int k, const char* who) {
  if (k > kGemmMaxExactK)
    throw std::invalid_argument(std::string(who) + ": K must be <= 1024 "
                                "(the integer pattern is exact in fp32 only up to there)");
}

// The three drivers below serve every GEMM payload. P is a problem: a
// GemmShape with upload(device) and launch(). PatternErr is |got - exact| of
// output (i, j) of the problem's own pattern at depth K.
using PatternErr = double (*)(float got, int i, int j, int K);

// upload, one launch, the M x N result into c
template <class P>
void run_once(P& p, int device, float* c) {
  p.upload(device);
  p.launch();
  HIP_CHECK(hipGetLastError());
  p.download(c);
}

// max err over the whole M x N result of a problem filled with its pattern
template <class P>
double run_full_check(P& p, int device, PatternErr err) {
  std::vector<float> host(static_cast<size_t>(p.M) * p.N);
  run_once(p, device, host.data());
  double max_err = 0;
  for (int i = 0; i < p.M; ++i)
    for (int j = 0; j < p.N; ++j)
      note_err(max_err, err(host[static_cast<size_t>(i) * p.N + j], i, j, p.K));
  return max_err;
}

// One warm-up launch, `iters` launches between events, then 256 fixed, spread
// output elements are checked exactly, so a fast wrong kernel cannot report a
// rate. FLOPs are counted as 2 M N K.
template <class P>
GemmResult run_timed(P& p, int iters, int device, PatternErr err) {
  p.upload(device);
  const float ms = time_launches(iters, [&p] { p.launch(); });
  GemmResult r;
  r.tflops = 2.0 * p.M * p.N * p.K * iters / (ms * 1e-3) / 1e12;
  for (int t = 0; t < 256; ++t) {
    int i = static_cast<int>((static_cast<int64_t>(t) * 1031 + 17) % p.M);
    int j = static_cast<int>((static_cast<int64_t>(t) * 2053 + 29) % p.N);
    float got = 0;
    HIP_CHECK(hipMemcpy(&got, p.dc.template as<float>() + static_cast<size_t>(i) * p.Np + j,
                        sizeof(float), hipMemcpyDeviceToHost));
    note_err(r.max_err, err(got, i, j, p.K));
  }
  return r;
}

}  // namespace detail

// General entry: c[M,N] = bf16(a[M,K]) · bf16(b[K,N]), all row-major float.
inline void gemm_bf16(const float* a, const float* b, float* c, int M, int N,
                      int K, int device = 0) {
  detail::GemmProblem p(M, N, K);
  for (int i = 0; i < M; ++i)
    for (int k = 0; k < K; ++k)
      p.a[i * p.Kp + k] = to_bf16_rne(a[static_cast<size_t>(i) * K + k]);
  for (int k = 0; k < K; ++k)
    for (int j = 0; j < N; ++j)
      p.bt[j * p.Kp + k] = to_bf16_rne(b[static_cast<size_t>(k) * N + j]);
  detail::run_once(p, device, c);
}

// Self-contained exact check: integer pattern in [-4, 4], host reference in
// int64, returns max |C - ref| over the whole M x N result (expect 0.0).
inline double run_gemm_check(int M, int N, int K, int device = 0) {
  detail::require_exact_k(K, "run_gemm_check");
  detail::GemmProblem p(M, N, K);
  detail::fill_pattern(p);
  return detail::run_full_check(p, device, detail::pattern_err);
}

// Timed run on the same integer pattern: one warm-up launch, `iters` launches
// between events, then 256 fixed, spread output elements are checked exactly
// against host int64 dot products, so a fast wrong kernel cannot report a rate.
inline GemmResult run_gemm(int M = 4096, int N = 4096, int K = 1024,
                           int iters = 10, int device = 0) {
  detail::require_exact_k(K, "run_gemm");
  if (iters < 1) throw std::invalid_argument("run_gemm: iters must be >= 1");
  detail::GemmProblem p(M, N, K);
  detail::fill_pattern(p);
  return detail::run_timed(p, iters, device, detail::pattern_err);
}

}  // namespace payload

