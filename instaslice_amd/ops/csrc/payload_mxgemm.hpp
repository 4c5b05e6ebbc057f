// gfx950 MXFP8 block-scaled matrix-core GEMM payload.
//
// gemm proves the bf16 MFMA path; this one proves the low-precision path a
// tenant of an MI355X pays for. On gfx950 the fp8 peak is reached only through
// the block-scaled instruction v_mfma_scale_f32_16x16x128_f8f6f4 (twice the
// bf16 rate per clock); the plain _fp8_fp8 forms run at the bf16 rate.
//
//   C[M,N] (fp32) = sum_k A[i,k] * 2^(sa[i,k/32]-127) * B[k,j] * 2^(sb[k/32,j]-127)
//
// A and B are OCP e4m3fn bytes (not the MI300 fnuz encoding), sa and sb E8M0
// bytes, one per 32 consecutive K elements of a row of A or a column of B (the
// OCP MX block).
//
//   block tile   128 x 128, K-step 128, 256 threads (4 wave64s as 2 x 2)
//   wave tile    64 x 64 = 4 x 4 MFMA tiles of 16 x 16 (64 accumulator VGPRs)
//   staging      as gemm_bf16_kernel: 16-byte global loads -> registers ->
//                ds_write_b128 into one LDS buffer per operand; the loads for
//                K-step t+1 are issued before the MFMAs of step t
//   fragment     measured on the hardware with one-hot operands and per-block
//                scales (tests/test_mxgemm_payload.py pins it): lane l holds
//                row/col l & 15; its registers 0-3 hold the 16 consecutive k
//                16 (l >> 4) .. +15 and its registers 4-7 the 16 consecutive k
//                64 + 16 (l >> 4) .. +15, two ds_read_b128. The scale of MX
//                block kb (k = 32 kb .. +31) of row/col r is taken from lane
//                16 kb + r, byte OPSEL of its scale register. So the lane
//                quarter l >> 4 supplies the scale of block l >> 4 although it
//                holds half of two other blocks' elements. (The 32-consecutive-k
//                map that composable-kernel's headers describe gives wrong
//                sums as soon as the scales of a row differ.)
//   LDS image    [128 rows][128 bytes], the 16-byte slot index XORed with
//                (row >> 1) & 7 as in the bf16 kernel. Register half h of lane
//                quarter q reads slot 4 h + q: the read pattern of the bf16
//                kernel's K-substep h, conflict-free for the same reason.
//   scales       one dword per lane, operand and K-step: its four bytes are
//                the scales of the lane's block (l >> 4) for rows l & 15 of
//                the wave's four MFMA tiles, and OPSEL = tile index picks the
//                byte. The host lays the Mp x Kp/32 scale bytes out for that
//                (mx_scale_off): [64-row group][K-step][lane][tile], so a wave
//                reads 256 contiguous bytes per operand and K-step, one K-step
//                ahead like the tiles. Loading a byte per fragment instead
//                (eight byte loads per lane and K-step) halved the rate.
//
// The host stores B transposed (N x K, K-contiguous), zero-pads M, N and K to
// 128 and pads the scale arrays to match with 127 (2^0): the kernel has no edge
// branch and forms no address outside its buffers for any shape.
//
// When both scale operands of the builtin are the compile-time constant 0 the
// compiler emits the unscaled v_mfma_f32_16x16x128_f8f6f4; a scale of 1.0 is
// the byte 127, not 0. Here the scales are always loaded values.
//
// Included by payload_core.hpp after payload_gemm.hpp (needs HIP_CHECK, kBlock,
// f32x4, detail::DeviceBuffer, detail::Event, detail::round_up, gemm_pat_a/b and
// detail::note_err).

#pragma once

#include <algorithm>
#include <cmath>
#include <cstring>

namespace payload {

typedef int i32x4 __attribute__((ext_vector_type(4)));  // 16 fp8, 4 VGPRs
typedef int i32x8 __attribute__((ext_vector_type(8)));  // 32 fp8, 8 VGPRs

constexpr int kMxBM = 128;
constexpr int kMxBN = 128;
constexpr int kMxBK = 128;   // fp8 elements = bytes per row of a K-step
constexpr int kMxBlock = 32;  // elements per scale (the OCP MX block)
constexpr int kMxSlots = kMxBK / 16;                 // 16-byte slots per row
constexpr int kMxLoads = kMxBM * kMxSlots / kBlock;  // per thread per operand
// Exact-check limit. Elements are integers in [-4, 4] and scales 2^-2 .. 2^2,
// so every product is a multiple of 2^-4 of magnitude <= 16 * 2^4 = 2^8. Any
// partial sum over K <= 2048 terms is then an integer of magnitude at most
// 2^12 * 2^11 = 2^23 in units of 2^-4, which fp32 holds exactly: the correct
// result is bit-exact in any accumulation order.
constexpr int kMxMaxExactK = 2048;

static_assert(kMxBM == kMxBN, "one staging index map serves both operands");
static_assert(kMxSlots == 8, "swizzle below assumes 8 slots per row");
static_assert(kMxBM * kMxSlots % kBlock == 0, "whole passes only");
static_assert(kMxBK / kMxBlock == 4, "one scale byte per 16-lane group");

// ---- kernel --------------------------------------------------------------

// byte offset of 16-byte slot `slot` of row `row` in an LDS tile
__device__ __forceinline__ int mx_lds_off(int row, int slot) {
  return row * kMxBK + ((slot ^ ((row >> 1) & 7)) << 4);
}

// byte offset of the scale of (row, MX block kb) in a scale image of Kb blocks
// per row: see "scales" in the header comment
__host__ __device__ inline size_t mx_scale_off(size_t row, size_t kb, size_t Kb) {
  const size_t g = row / 64, m = (row / 16) & 3, fr = row & 15;
  const size_t t = kb / 4, fq = kb & 3;
  return ((g * (Kb / 4) + t) * 64 + fq * 16 + fr) * 4 + m;
}

// cbsz = blgp = 0: e4m3 operands. OA / OB pick the byte of sa / sb that holds
// the scale (the builtin wants them as constants).
template <int OA, int OB>
__device__ __forceinline__ f32x4 mx_mfma(i32x8 a, i32x8 b, f32x4 c, int sa, int sb) {
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 0, 0, OA, sa,
                                                          OB, sb);
}

// a: Mp x Kp, bt: Np x Kp (B transposed), sa, sbt: scale images of Mp x Kp/32
// and Np x Kp/32 bytes (mx_scale_off), c: Mp x Np; Mp, Np and Kp multiples of
// 128. grid = (Np / 128, Mp / 128).
__global__ __launch_bounds__(kBlock) void gemm_mxfp8_kernel(
    const uint8_t* __restrict__ a, const uint8_t* __restrict__ bt,
    const uint8_t* __restrict__ sa, const uint8_t* __restrict__ sbt,
    float* __restrict__ c, int Np, int Kp) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[(kMxBM + kMxBN) * kMxBK];
  uint8_t* lds_a = lds;
  uint8_t* lds_b = lds + kMxBM * kMxBK;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // keep it scalar
  const int wr = wave >> 1, wc = wave & 1;  // wave's 64x64 quadrant
  const int fr = lane & 15, fq = lane >> 4;

  // staging map: 8 consecutive lanes cover one 128-byte row of the K-step
  const int srow = tid >> 3, sslot = tid & 7;
  const size_t brow = static_cast<size_t>(blockIdx.y) * kMxBM;
  const size_t bcol = static_cast<size_t>(blockIdx.x) * kMxBN;
  // block-uniform bases plus 32-bit lane offsets shared by both operands
  // (128 Kp < 2^32: the host limits Kp): fewer address registers
  const uint8_t* ga = a + brow * Kp;
  const uint8_t* gb = bt + bcol * Kp;
  unsigned soff[kMxLoads];
#pragma unroll
  for (int i = 0; i < kMxLoads; ++i)
    soff[i] = static_cast<unsigned>(srow + i * (kBlock / kMxSlots)) *
                  static_cast<unsigned>(Kp) + sslot * 16;

  // the lane's scale dword of K-step t: 64 dwords per wave tile and K-step
  const size_t steps = static_cast<size_t>(Kp / kMxBK);
  const int* gsa = reinterpret_cast<const int*>(sa) +
                   (brow / 64 + wr) * steps * 64 + lane;
  const int* gsb = reinterpret_cast<const int*>(sbt) +
                   (bcol / 64 + wc) * steps * 64 + lane;

  i32x4 ra[kMxLoads], rb[kMxLoads];
  int nsa = gsa[0], nsb = gsb[0];
#pragma unroll
  for (int i = 0; i < kMxLoads; ++i) {
    ra[i] = *reinterpret_cast<const i32x4*>(ga + soff[i]);
    rb[i] = *reinterpret_cast<const i32x4*>(gb + soff[i]);
  }

  f32x4 acc[4][4];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int k0 = 0; k0 < Kp; k0 += kMxBK) {
#pragma unroll
    for (int i = 0; i < kMxLoads; ++i) {
      int row = srow + i * (kBlock / kMxSlots);
      *reinterpret_cast<i32x4*>(lds_a + mx_lds_off(row, sslot)) = ra[i];
      *reinterpret_cast<i32x4*>(lds_b + mx_lds_off(row, sslot)) = rb[i];
    }
    const int sca = nsa, scb = nsb;
    __syncthreads();

    if (k0 + kMxBK < Kp) {  // block-uniform: prefetch the next K-step
#pragma unroll
      for (int i = 0; i < kMxLoads; ++i) {
        ra[i] = *reinterpret_cast<const i32x4*>(ga + k0 + kMxBK + soff[i]);
        rb[i] = *reinterpret_cast<const i32x4*>(gb + k0 + kMxBK + soff[i]);
      }
      const int next = (k0 + kMxBK) / kMxBK * 64;
      nsa = gsa[next];
      nsb = gsb[next];
    }

    // lane l, register half h: A[row l&15][k = 64h + 16(l>>4) + j] and
    // B[k = 64h + 16(l>>4) + j][col l&15], j = 0..15: slots (l>>4) and
    // 4 + (l>>4) of the row
    i32x8 fb[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      int row = wc * 64 + n * 16 + fr;
      i32x4 lo = *reinterpret_cast<const i32x4*>(lds_b + mx_lds_off(row, fq));
      i32x4 hi = *reinterpret_cast<const i32x4*>(lds_b + mx_lds_off(row, 4 + fq));
      fb[n] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    }
    // one row of MFMA tiles at a time: only one A fragment is live
#define MX_MFMA(m, n) acc[m][n] = mx_mfma<m, n>(fa, fb[n], acc[m][n], sca, scb)
#define MX_MFMA_ROW(m)                                                            \
  {                                                                               \
    int row = wr * 64 + m * 16 + fr;                                              \
    i32x4 lo = *reinterpret_cast<const i32x4*>(lds_a + mx_lds_off(row, fq));      \
    i32x4 hi = *reinterpret_cast<const i32x4*>(lds_a + mx_lds_off(row, 4 + fq));  \
    i32x8 fa = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);           \
    MX_MFMA(m, 0); MX_MFMA(m, 1); MX_MFMA(m, 2); MX_MFMA(m, 3);                   \
  }
    MX_MFMA_ROW(0);
    MX_MFMA_ROW(1);
    MX_MFMA_ROW(2);
    MX_MFMA_ROW(3);
#undef MX_MFMA_ROW
#undef MX_MFMA
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

// ---- host layer: formats ---------------------------------------------------

// float -> OCP e4m3fn byte (1 sign, 4 exponent bits of bias 7, 3 mantissa
// bits; largest finite 448 = 0x7E, 0x7F is NaN, no infinities). Round to
// nearest even, subnormals (multiples of 2^-9 below 2^-6) rounded and not
// flushed, +-0 preserved. A finite value that rounds above 448, and +-inf,
// saturate to +-448. NaN gives 0x7F with the sign bit kept.
inline uint8_t to_e4m3_sat(float f) {
  uint32_t u;
  std::memcpy(&u, &f, sizeof(u));
  const uint8_t sign = static_cast<uint8_t>((u >> 24) & 0x80u);
  uint32_t mag = u & 0x7FFFFFFFu;
  if (mag > 0x7F800000u) return sign | 0x7Fu;
  // 448 = 0x43E00000. Anything from there up either is 448, rounds down to it
  // (below the tie 464), ties to its even mantissa (464) or saturates.
  if (mag >= 0x43E00000u) return sign | 0x7Eu;
  if (mag >= 0x3C800000u) {  // 2^-6 and up: normal in e4m3
    mag += 0x7FFFFu + ((mag >> 20) & 1u);
    return sign | static_cast<uint8_t>((mag >> 20) - (120u << 3));
  }
  // below 2^-6: the code is |f| * 2^9 rounded to an integer 0..8 (8 is the
  // smallest normal). |f| = m * 2^(e - 150) with the implicit bit in m.
  const int e = static_cast<int>(mag >> 23);
  const int shift = 141 - e;  // >= 21 here
  if (e == 0 || shift > 24) return sign;  // below half of 2^-9
  const uint32_t m = (mag & 0x7FFFFFu) | 0x800000u;
  uint32_t q = m >> shift;
  const uint32_t rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1);
  if (rem > half || (rem == half && (q & 1u))) ++q;
  return sign | static_cast<uint8_t>(q);
}

inline float from_e4m3(uint8_t code) {
  const int exp = (code >> 3) & 15, man = code & 7;
  float v;
  if (exp == 15 && man == 7)
    v = NAN;
  else if (exp == 0)
    v = std::ldexp(static_cast<float>(man), -9);
  else
    v = std::ldexp(static_cast<float>(8 + man), exp - 10);
  return (code & 0x80) ? -v : v;
}

// OCP MX quantization of one row of K floats: per block of 32 elements (a last
// partial block as if padded with zeros) one E8M0 scale byte
// clamp(floor(log2(amax)) - 8 + 127, 0, 254), 8 being the exponent of the
// largest e4m3 (448 = 1.75 * 2^8), and the elements to_e4m3_sat(x / 2^(scale -
// 127)). An all-zero block gets 127. codes: K bytes, scales: ceil(K / 32).
// A NaN element becomes a NaN code and takes no part in amax.
inline void mx_quantize_row(const float* x, int K, uint8_t* codes, uint8_t* scales) {
  for (int k0 = 0; k0 < K; k0 += kMxBlock) {
    const int n = std::min(kMxBlock, K - k0);
    float amax = 0.f;
    for (int k = 0; k < n; ++k) {
      float v = std::fabs(x[k0 + k]);
      if (v > amax) amax = v;
    }
    int scale = 127;
    if (amax > 0.f) {
      // ilogb is floor(log2) for normals and subnormals; inf clamps to 254
      long e = std::isinf(amax) ? 1000 : std::ilogb(amax);
      scale = static_cast<int>(std::min(254l, std::max(0l, e - 8 + 127)));
    }
    scales[k0 / kMxBlock] = static_cast<uint8_t>(scale);
    // |127 - scale| <= 127 and x * 2^(127 - scale) < 2^9 whenever the clamp at
    // 0 is not hit, so the scaling is exact unless the result is an fp32
    // subnormal, which is far below half of 2^-9 and becomes zero either way
    for (int k = 0; k < n; ++k)
      codes[k0 + k] = to_e4m3_sat(std::ldexp(x[k0 + k], 127 - scale));
  }
}

// ---- host layer: the GEMM --------------------------------------------------

namespace detail {

// Padded operands and scales on the host plus their device images and the
// padded C.
struct MxProblem {
  int M, N, K;
  size_t Mp, Np, Kp, Kb;     // Kb: scale bytes per padded row
  std::vector<uint8_t> a, bt;    // Mp x Kp, Np x Kp, zero-padded
  std::vector<uint8_t> sa, sbt;  // scale images (mx_scale_off), padded with 127
  DeviceBuffer da, dbt, dsa, dsbt, dc;

  MxProblem(int m, int n, int k) : M(m), N(n), K(k) {
    if (m < 1 || n < 1 || k < 1)
      throw std::invalid_argument("mxgemm: M, N and K must be >= 1");
    Mp = round_up(m, kMxBM);
    Np = round_up(n, kMxBN);
    Kp = round_up(k, kMxBK);
    if (Mp / kMxBM > 65535 || Np > 0x7FFFFF80u || Kp > (1u << 24))
      throw std::invalid_argument("mxgemm: shape too large");
    Kb = Kp / kMxBlock;
    a.assign(Mp * Kp, 0);
    bt.assign(Np * Kp, 0);
    sa.assign(Mp * Kb, 127);
    sbt.assign(Np * Kb, 127);
  }

  void upload(int device) {
    HIP_CHECK(hipSetDevice(device));
    da.alloc(a.size());
    dbt.alloc(bt.size());
    dsa.alloc(sa.size());
    dsbt.alloc(sbt.size());
    dc.alloc(Mp * Np * sizeof(float));
    HIP_CHECK(hipMemcpy(da.p, a.data(), a.size(), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dbt.p, bt.data(), bt.size(), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dsa.p, sa.data(), sa.size(), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dsbt.p, sbt.data(), sbt.size(), hipMemcpyHostToDevice));
  }

  void launch() const {
    dim3 grid(static_cast<unsigned>(Np / kMxBN), static_cast<unsigned>(Mp / kMxBM));
    hipLaunchKernelGGL(gemm_mxfp8_kernel, grid, dim3(kBlock), 0, 0,
                       da.as<const uint8_t>(), dbt.as<const uint8_t>(),
                       dsa.as<const uint8_t>(), dsbt.as<const uint8_t>(),
                       dc.as<float>(), static_cast<int>(Np), static_cast<int>(Kp));
  }

  // the un-padded M x N region, row-major, into c
  void download(float* c) const {
    HIP_CHECK(hipMemcpy2D(c, static_cast<size_t>(N) * sizeof(float), dc.p,
                          Np * sizeof(float), static_cast<size_t>(N) * sizeof(float),
                          M, hipMemcpyDeviceToHost));
  }
};

// scale exponents of the exact pattern, in [-2, 2]: asymmetric, and a
// different function of (row, block) than of (block, column)
inline int mx_pat_sa(int i, int kb) {
  return static_cast<int>((3ll * i + kb) % 5) - 2;
}
inline int mx_pat_sb(int kb, int j) {
  return static_cast<int>((2ll * kb + 3ll * j + 1) % 5) - 2;
}

inline void fill_mx_pattern(MxProblem& p) {
  const int blocks = (p.K + kMxBlock - 1) / kMxBlock;
  for (int i = 0; i < p.M; ++i) {
    for (int k = 0; k < p.K; ++k)
      p.a[i * p.Kp + k] = to_e4m3_sat(static_cast<float>(gemm_pat_a(i, k)));
    for (int kb = 0; kb < blocks; ++kb)
      p.sa[mx_scale_off(i, kb, p.Kb)] = static_cast<uint8_t>(127 + mx_pat_sa(i, kb));
  }
  for (int j = 0; j < p.N; ++j) {
    for (int k = 0; k < p.K; ++k)
      p.bt[j * p.Kp + k] = to_e4m3_sat(static_cast<float>(gemm_pat_b(k, j)));
    for (int kb = 0; kb < blocks; ++kb)
      p.sbt[mx_scale_off(j, kb, p.Kb)] = static_cast<uint8_t>(127 + mx_pat_sb(kb, j));
  }
}

// the exact result in units of 2^-4
inline int64_t mx_pattern_dot(int i, int j, int K) {
  int64_t s = 0;
  for (int k = 0; k < K; ++k) {
    int kb = k / kMxBlock;
    int64_t prod = static_cast<int64_t>(gemm_pat_a(i, k)) * gemm_pat_b(k, j);
    s += prod * (int64_t{1} << (mx_pat_sa(i, kb) + mx_pat_sb(kb, j) + 4));
  }
  return s;
}

inline double mx_pattern_err(float got, int i, int j, int K) {
  return std::fabs(static_cast<double>(got) -
                   static_cast<double>(mx_pattern_dot(i, j, K)) / 16.0);
}

inline void require_exact_mx_k(int k, const char* who) {
  if (k > kMxMaxExactK)
    throw std::invalid_argument(std::string(who) + ": K must be <= 2048 "
                                "(the scaled integer pattern is exact in fp32 "
                                "only up to there)");
}

}  // namespace detail

// Raw entry: operands already quantized. a_codes M x K, a_scales M x
// ceil(K/32), b_codes K x N, b_scales ceil(K/32) x N, all row-major bytes;
// c M x N row-major float.
inline void gemm_mxfp8_raw(const uint8_t* a_codes, const uint8_t* a_scales,
                           const uint8_t* b_codes, const uint8_t* b_scales,
                           float* c, int M, int N, int K, int device = 0) {
  detail::MxProblem p(M, N, K);
  const size_t blocks = (static_cast<size_t>(K) + kMxBlock - 1) / kMxBlock;
  for (int i = 0; i < M; ++i) {
    std::memcpy(&p.a[i * p.Kp], a_codes + static_cast<size_t>(i) * K, K);
    for (size_t kb = 0; kb < blocks; ++kb)
      p.sa[mx_scale_off(i, kb, p.Kb)] = a_scales[static_cast<size_t>(i) * blocks + kb];
  }
  for (int k = 0; k < K; ++k)
    for (int j = 0; j < N; ++j)
      p.bt[j * p.Kp + k] = b_codes[static_cast<size_t>(k) * N + j];
  for (size_t kb = 0; kb < blocks; ++kb)
    for (int j = 0; j < N; ++j)
      p.sbt[mx_scale_off(j, kb, p.Kb)] = b_scales[kb * N + j];
  p.upload(device);
  p.launch();
  HIP_CHECK(hipGetLastError());
  p.download(c);
}

// General entry: c[M,N] = mx(a[M,K]) · mx(b[K,N]), all row-major float. Rows
// of a and columns of b are MX-quantized (mx_quantize_row). Throws
// std::invalid_argument on a non-finite input, before any device work.
inline void gemm_mxfp8(const float* a, const float* b, float* c, int M, int N,
                       int K, int device = 0) {
  detail::MxProblem p(M, N, K);
  for (size_t i = 0, n = static_cast<size_t>(M) * K; i < n; ++i)
    if (!std::isfinite(a[i]))
      throw std::invalid_argument("gemm_mxfp8: a has a non-finite element");
  for (size_t i = 0, n = static_cast<size_t>(K) * N; i < n; ++i)
    if (!std::isfinite(b[i]))
      throw std::invalid_argument("gemm_mxfp8: b has a non-finite element");
  const size_t blocks = (static_cast<size_t>(K) + kMxBlock - 1) / kMxBlock;
  std::vector<uint8_t> scales(blocks);
  for (int i = 0; i < M; ++i) {
    mx_quantize_row(a + static_cast<size_t>(i) * K, K, &p.a[i * p.Kp], scales.data());
    for (size_t kb = 0; kb < blocks; ++kb)
      p.sa[mx_scale_off(i, kb, p.Kb)] = scales[kb];
  }
  std::vector<float> col(K);
  for (int j = 0; j < N; ++j) {
    for (int k = 0; k < K; ++k) col[k] = b[static_cast<size_t>(k) * N + j];
    mx_quantize_row(col.data(), K, &p.bt[j * p.Kp], scales.data());
    for (size_t kb = 0; kb < blocks; ++kb)
      p.sbt[mx_scale_off(j, kb, p.Kb)] = scales[kb];
  }
  p.upload(device);
  p.launch();
  HIP_CHECK(hipGetLastError());
  p.download(c);
}

// Self-contained exact check: integer elements in [-4, 4] (gemm_pat_a / _b),
// scale exponents in [-2, 2] (mx_pat_sa / _sb), host reference in int64 in
// units of 2^-4; returns max |C - ref| over the whole M x N result (expect 0.0).
inline double run_mxgemm_check(int M, int N, int K, int device = 0) {
  detail::require_exact_mx_k(K, "run_mxgemm_check");
  detail::MxProblem p(M, N, K);
  detail::fill_mx_pattern(p);
  p.upload(device);
  p.launch();
  HIP_CHECK(hipGetLastError());
  std::vector<float> host(static_cast<size_t>(M) * N);
  p.download(host.data());
  double max_err = 0;
  for (int i = 0; i < M; ++i)
    for (int j = 0; j < N; ++j)
      detail::note_err(max_err, detail::mx_pattern_err(
                                    host[static_cast<size_t>(i) * N + j], i, j, K));
  return max_err;
}

// Timed run on the same pattern: one warm-up launch, `iters` launches between
// events, then the 256 fixed, spread output elements of run_gemm are checked
// exactly. FLOPs are counted as 2 M N K.
inline GemmResult run_mxgemm(int M = 4096, int N = 4096, int K = 2048,
                             int iters = 10, int device = 0) {
  detail::require_exact_mx_k(K, "run_mxgemm");
  if (iters < 1) throw std::invalid_argument("run_mxgemm: iters must be >= 1");
  detail::MxProblem p(M, N, K);
  detail::fill_mx_pattern(p);
  p.upload(device);
  p.launch();  // warmup
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipDeviceSynchronize());
  float ms = 0;
  {
    detail::Event t0, t1;
    HIP_CHECK(hipEventRecord(t0.e, 0));
    for (int i = 0; i < iters; ++i) p.launch();
    HIP_CHECK(hipEventRecord(t1.e, 0));
    HIP_CHECK(hipEventSynchronize(t1.e));
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventElapsedTime(&ms, t0.e, t1.e));
  }
  GemmResult r;
  r.tflops = 2.0 * M * N * K * iters / (ms * 1e-3) / 1e12;
  for (int t = 0; t < 256; ++t) {
    int i = static_cast<int>((static_cast<int64_t>(t) * 1031 + 17) % M);
    int j = static_cast<int>((static_cast<int64_t>(t) * 2053 + 29) % N);
    float got = 0;
    HIP_CHECK(hipMemcpy(&got, p.dc.as<float>() + static_cast<size_t>(i) * p.Np + j,
                        sizeof(float), hipMemcpyDeviceToHost));
    detail::note_err(r.max_err, detail::mx_pattern_err(got, i, j, K));
  }
  return r;
}

}  // namespace payload
