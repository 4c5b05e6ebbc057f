// gfx950 MX block-scaled matrix-core GEMM kernel, and the MXFP8 payload on it.
//
// gemm proves the bf16 MFMA path; the MX payloads prove the low-precision paths
// a tenant of an MI355X pays for. On gfx950 the fp8 and fp4 peaks are reached
// only through the block-scaled instruction v_mfma_scale_f32_16x16x128_f8f6f4
// (e4m3: twice the bf16 rate per clock, e2m1: four times); the plain _fp8_fp8
// forms run at the bf16 rate.
//
//   C[M,N] (fp32) = sum_k A[i,k] * 2^(sa[i,k/32]-127) * B[k,j] * 2^(sb[k/32,j]-127)
//
// sa and sb are E8M0 bytes, one per 32 consecutive K elements of a row of A or
// a column of B (the OCP MX block). For this payload A and B are OCP e4m3fn
// bytes (not the MI300 fnuz encoding); payload_mxfp4.hpp has the e2m1 elements.
//
// One kernel template, gemm_mx_kernel<kSel>, serves both formats. kSel is the
// instruction's format selector (cbsz = blgp): 0 for e4m3, 4 for e2m1. What is
// the same for both:
//
//   block tile   128 x 128, 256 threads (4 wave64s as 2 x 2)
//   wave tile    64 x 64 = 4 x 4 MFMA tiles of 16 x 16 (64 accumulator VGPRs)
//   K-step       128 bytes of every row: 128 e4m3 or 256 e2m1 elements
//   staging      as gemm_bf16_kernel: 16-byte global loads -> registers ->
//                ds_write_b128 into one LDS buffer per operand; the loads for
//                K-step t+1 are issued before the MFMAs of step t
//   LDS image    [128 rows][128 bytes], the 16-byte slot index XORed with
//                (row >> 1) & 7 as in the bf16 kernel (mx_lds_off). A lane of
//                quarter q = l >> 4 reads slot 4 h + q, h = 0 or 1: the read
//                pattern of the bf16 kernel's K-substep h, conflict-free for
//                the same reason.
//   lane map     measured on the hardware with one-hot operands and per-block
//                scales (the K-order and scale-block tests of both formats pin
//                it): lane l holds row/col l & 15, and the scale of MX block
//                kb (k = 32 kb .. +31 of the instruction's 128) of row/col r
//                is taken from lane 16 kb + r, byte OPSEL of its scale
//                register.
//   scales       one dword per lane, operand and MFMA: its four bytes are the
//                scales of the lane's block (l >> 4) for rows l & 15 of the
//                wave's four MFMA tiles, and OPSEL = tile index picks the
//                byte. The host lays the Mp x Kp/32 scale bytes out for that
//                (mx_scale_off): [64-row group][128 k][lane][tile], so a wave
//                reads 256 contiguous bytes per operand and MFMA of a K-step,
//                one K-step ahead like the tiles. Loading a byte per fragment
//                instead (eight byte loads per lane and K-step) halved the
//                e4m3 rate.
//
// What differs (mx_frag, mx_mfma and kSubs below):
//
//   e4m3   one MFMA per K-step. Registers 0-3 of lane l hold the 16 consecutive
//          k 16 (l >> 4) .. +15 and registers 4-7 the 16 consecutive k
//          64 + 16 (l >> 4) .. +15: slots (l >> 4) and 4 + (l >> 4) of the
//          row, two ds_read_b128. So the lane quarter l >> 4 supplies the
//          scale of block l >> 4 although it holds half of two other blocks'
//          elements. (The 32-consecutive-k map that composable-kernel's
//          headers describe gives wrong sums as soon as the scales of a row
//          differ.)
//   e2m1   two MFMAs per K-step, sub-steps s = 0, 1 of 128 elements. Sub-step s
//          reads slot 4 s + (l >> 4), one ds_read_b128, into registers 0-3;
//          registers 4-7 are zeros (payload_mxfp4.hpp has the measured facts).
//
// The host stores B transposed (N x K, K-contiguous), zero-pads M and N to 128
// and K to a K-step and pads the scale arrays to match with 127 (2^0): the
// kernel has no edge branch and forms no address outside its buffers for any
// shape.
//
// When both scale operands of the builtin are the compile-time constant 0 the
// compiler emits the unscaled v_mfma_f32_16x16x128_f8f6f4; a scale of 1.0 is
// the byte 127, not 0. Here the scales are always loaded values.
//
// Included by payload_core.hpp after payload_gemm.hpp (needs HIP_CHECK, kBlock,
// f32x4, detail::DeviceBuffer, gemm_pat_a/b, and the shared GEMM host layer:
// detail::GemmShape, run_once, run_full_check and run_timed).

#pragma once

#include <algorithm>
#include <cmath>
#include <cstring>

namespace payload {

typedef int i32x4 __attribute__((ext_vector_type(4)));  // 16 staged bytes, 4 VGPRs
typedef int i32x8 __attribute__((ext_vector_type(8)));  // an MFMA operand, 8 VGPRs

constexpr int kMxBM = 128;
constexpr int kMxBN = 128;
constexpr int kMxBK = 128;   // bytes per row of a K-step; elements per MFMA
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

// the operand of lane (row, fq) for MFMA s of the K-step staged in `tile`
template <int kSel>
__device__ __forceinline__ i32x8 mx_frag(const uint8_t* tile, int row, int fq, int s) {
  if constexpr (kSel == 0) {
    i32x4 lo = *reinterpret_cast<const i32x4*>(tile + mx_lds_off(row, fq));
    i32x4 hi = *reinterpret_cast<const i32x4*>(tile + mx_lds_off(row, 4 + fq));
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  } else {
    i32x4 v = *reinterpret_cast<const i32x4*>(tile + mx_lds_off(row, 4 * s + fq));
    return i32x8{v[0], v[1], v[2], v[3], 0, 0, 0, 0};  // the compiler drops 4-7
  }
}

// OA / OB pick the byte of sa / sb that holds the scale (the builtin wants them
// as constants).
template <int kSel, int OA, int OB>
__device__ __forceinline__ f32x4 mx_mfma(i32x8 a, i32x8 b, f32x4 c, int sa, int sb) {
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, kSel, kSel, OA,
                                                          sa, OB, sb);
}

// a: Mp rows, bt: Np rows (B transposed) of Kp elements, one (e4m3) or two
// (e2m1) to a byte; sa, sbt: scale images of Mp x Kp/32 and Np x Kp/32 bytes
// (mx_scale_off); c: Mp x Np. Mp and Np are multiples of 128 and a row a
// multiple of 128 bytes. grid = (Np / 128, Mp / 128).
template <int kSel>
__global__ __launch_bounds__(kBlock) void gemm_mx_kernel(
    const uint8_t* __restrict__ a, const uint8_t* __restrict__ bt,
    const uint8_t* __restrict__ sa, const uint8_t* __restrict__ sbt,
    float* __restrict__ c, int Np, int Kp) {
  static_assert(kSel == 0 || kSel == 4, "e4m3 or e2m1");
  constexpr int kSubs = kSel == 4 ? 2 : 1;  // MFMAs per K-step = elements per byte

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
  const int Kbytes = Kp >> (kSubs - 1);  // bytes per row
  // block-uniform bases plus 32-bit lane offsets shared by both operands
  // (128 Kbytes < 2^32: the host limits Kp): fewer address registers
  const uint8_t* ga = a + brow * Kbytes;
  const uint8_t* gb = bt + bcol * Kbytes;
  unsigned soff[kMxLoads];
#pragma unroll
  for (int i = 0; i < kMxLoads; ++i)
    soff[i] = static_cast<unsigned>(srow + i * (kBlock / kMxSlots)) *
                  static_cast<unsigned>(Kbytes) + sslot * 16;

  // the lane's scale dwords: 64 dwords per wave tile and MFMA of a row
  const size_t mfmas = static_cast<size_t>(Kp / kMxBK);
  const int* gsa = reinterpret_cast<const int*>(sa) +
                   (brow / 64 + wr) * mfmas * 64 + lane;
  const int* gsb = reinterpret_cast<const int*>(sbt) +
                   (bcol / 64 + wc) * mfmas * 64 + lane;

  i32x4 ra[kMxLoads], rb[kMxLoads];
  int nsa[kSubs], nsb[kSubs];
#pragma unroll
  for (int s = 0; s < kSubs; ++s) {
    nsa[s] = gsa[64 * s];
    nsb[s] = gsb[64 * s];
  }
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

  // b0: byte offset of the K-step in a row
  for (int b0 = 0; b0 < Kbytes; b0 += kMxBK) {
#pragma unroll
    for (int i = 0; i < kMxLoads; ++i) {
      int row = srow + i * (kBlock / kMxSlots);
      *reinterpret_cast<i32x4*>(lds_a + mx_lds_off(row, sslot)) = ra[i];
      *reinterpret_cast<i32x4*>(lds_b + mx_lds_off(row, sslot)) = rb[i];
    }
    int sca[kSubs], scb[kSubs];
#pragma unroll
    for (int s = 0; s < kSubs; ++s) {
      sca[s] = nsa[s];
      scb[s] = nsb[s];
    }
    __syncthreads();

    if (b0 + kMxBK < Kbytes) {  // block-uniform: prefetch the next K-step
#pragma unroll
      for (int i = 0; i < kMxLoads; ++i) {
        ra[i] = *reinterpret_cast<const i32x4*>(ga + b0 + kMxBK + soff[i]);
        rb[i] = *reinterpret_cast<const i32x4*>(gb + b0 + kMxBK + soff[i]);
      }
      const int next = (b0 + kMxBK) / kMxBK * 64 * kSubs;
#pragma unroll
      for (int s = 0; s < kSubs; ++s) {
        nsa[s] = gsa[next + 64 * s];
        nsb[s] = gsb[next + 64 * s];
      }
    }

#pragma unroll
    for (int s = 0; s < kSubs; ++s) {
      i32x8 fb[4];
#pragma unroll
      for (int n = 0; n < 4; ++n)
        fb[n] = mx_frag<kSel>(lds_b, wc * 64 + n * 16 + fr, fq, s);
      // one row of MFMA tiles at a time: only one A fragment is live
#define MX_MFMA(m, n) \
  acc[m][n] = mx_mfma<kSel, m, n>(fa, fb[n], acc[m][n], sca[s], scb[s])
#define MX_MFMA_ROW(m)                                                   \
  {                                                                      \
    i32x8 fa = mx_frag<kSel>(lds_a, wr * 64 + m * 16 + fr, fq, s);       \
    MX_MFMA(m, 0); MX_MFMA(m, 1); MX_MFMA(m, 2); MX_MFMA(m, 3);          \
  }
      MX_MFMA_ROW(0);
      MX_MFMA_ROW(1);
      MX_MFMA_ROW(2);
      MX_MFMA_ROW(3);
#undef MX_MFMA_ROW
#undef MX_MFMA
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

namespace detail {

// E8M0 scale byte of one MX block of n <= 32 floats for an element format
// whose largest value has exponent emax: clamp(floor(log2(amax)) - emax + 127,
// 0, 254); 127 for an all-zero block. A NaN element takes no part in amax.
inline int mx_block_scale(const float* x, int n, int emax) {
  float amax = 0.f;
  for (int k = 0; k < n; ++k) {
    float v = std::fabs(x[k]);
    if (v > amax) amax = v;
  }
  if (!(amax > 0.f)) return 127;
  // ilogb is floor(log2) for normals and subnormals; inf clamps to 254
  long e = std::isinf(amax) ? 1000 : std::ilogb(amax);
  return static_cast<int>(std::min(254l, std::max(0l, e - emax + 127)));
}

// What tells the MX formats apart on the host. A format F has
//   name          the payload's name in messages
//   kBK           the kernel's K-step, in elements
//   kPerByte      elements per byte of the device image
//   kEmax         the exponent of the format's largest value
//   kernel        the format's instantiation of gemm_mx_kernel
//   encode        float -> element code, one per byte
//   put           the code of element k into its byte of the image
//   pack          a row of K codes, one per byte, into its image bytes
struct Mxfp8 {
  static constexpr const char* name = "mxgemm";
  static constexpr int kBK = kMxBK;
  static constexpr int kPerByte = 1;
  static constexpr int kEmax = 8;  // 448 = 1.75 * 2^8
  static constexpr auto kernel = gemm_mx_kernel<0>;
  static uint8_t encode(float f) { return to_e4m3_sat(f); }
  static void put(uint8_t& byte, size_t, uint8_t code) { byte = code; }
  static void pack(const uint8_t* codes, int K, uint8_t* out) {
    std::memcpy(out, codes, K);
  }
};

// OCP MX quantization of one row of K floats to format F: per block of 32
// elements (a last partial block as if padded with zeros) one E8M0 scale byte
// clamp(floor(log2(amax)) - F::kEmax + 127, 0, 254) and the elements
// F::encode(x * 2^(127 - scale)). An all-zero block gets 127. codes: K bytes,
// one code each, scales: ceil(K / 32).
template <class F>
void mx_quantize_row(const float* x, int K, uint8_t* codes, uint8_t* scales) {
  for (int k0 = 0; k0 < K; k0 += kMxBlock) {
    const int n = std::min(kMxBlock, K - k0);
    const int scale = mx_block_scale(x + k0, n, F::kEmax);
    scales[k0 / kMxBlock] = static_cast<uint8_t>(scale);
    // |127 - scale| <= 127 and x * 2^(127 - scale) < 2^(kEmax + 1) whenever the
    // clamp at 0 is not hit, so the power-of-two scaling is exact unless the
    // result is an fp32 subnormal, which becomes zero either way. e4m3: < 2^9,
    // and a subnormal is far below half of 2^-9. e2m1: < 8, and a subnormal is
    // far below the first tie (0.25).
    for (int k = 0; k < n; ++k)
      codes[k0 + k] = F::encode(std::ldexp(x[k0 + k], 127 - scale));
  }
}

}  // namespace detail

// OCP MX quantization of one row of K floats to e4m3 (detail::mx_quantize_row
// with to_e4m3_sat). codes: K bytes, scales: ceil(K / 32). A NaN element
// becomes a NaN code and takes no part in amax.
inline void mx_quantize_row(const float* x, int K, uint8_t* codes, uint8_t* scales) {
  detail::mx_quantize_row<detail::Mxfp8>(x, K, codes, scales);
}

// ---- host layer: the GEMM --------------------------------------------------

namespace detail {

static_assert(kMxBM == kGemmBM && kMxBN == kGemmBN, "GemmShape pads M and N");

// Padded operands and scales of format F on the host plus their device images.
template <class F>
struct MxProblem : GemmShape {
  static_assert(F::kBK == kMxBK * F::kPerByte, "a K-step row is 128 bytes");
  size_t Kbytes, Kb;            // per padded row: operand bytes, scale bytes
  std::vector<uint8_t> a, bt;    // Mp x Kbytes, Np x Kbytes, zero-padded
  std::vector<uint8_t> sa, sbt;  // scale images (mx_scale_off), padded with 127
  DeviceBuffer da, dbt, dsa, dsbt;

  MxProblem(int m, int n, int k) : GemmShape(F::name, m, n, k, F::kBK, 1u << 24) {
    Kbytes = Kp / F::kPerByte;
    Kb = Kp / kMxBlock;
    a.assign(Mp * Kbytes, 0);
    bt.assign(Np * Kbytes, 0);
    sa.assign(Mp * Kb, 127);
    sbt.assign(Np * Kb, 127);
  }

  uint8_t* row_a(size_t i) { return &a[i * Kbytes]; }
  uint8_t* row_bt(size_t j) { return &bt[j * Kbytes]; }

  // element k of row i of A / of column j of B
  void set_a(size_t i, size_t k, uint8_t code) { F::put(row_a(i)[k / F::kPerByte], k, code); }
  void set_b(size_t k, size_t j, uint8_t code) { F::put(row_bt(j)[k / F::kPerByte], k, code); }

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
    hipLaunchKernelGGL(F::kernel, grid(), dim3(kBlock), 0, 0,
                       da.as<const uint8_t>(), dbt.as<const uint8_t>(),
                       dsa.as<const uint8_t>(), dsbt.as<const uint8_t>(),
                       dc.as<float>(), static_cast<int>(Np), static_cast<int>(Kp));
  }
};

// the `blocks` scales of row `row` of A (or column `row` of B), `stride` bytes
// apart at `scales`, into their places in a scale image of Kb blocks per row
inline void scatter_scales(std::vector<uint8_t>& image, size_t row, size_t Kb,
                           const uint8_t* scales, size_t blocks, size_t stride = 1) {
  for (size_t kb = 0; kb < blocks; ++kb)
    image[mx_scale_off(row, kb, Kb)] = scales[kb * stride];
}

// scale exponents of the exact pattern, in [-2, 2]: asymmetric, and a
// different function of (row, block) than of (block, column)
inline int mx_pat_sa(int i, int kb) {
  return static_cast<int>((3ll * i + kb) % 5) - 2;
}
inline int mx_pat_sb(int kb, int j) {
  return static_cast<int>((2ll * kb + 3ll * j + 1) % 5) - 2;
}

// the gemm integer pattern (gemm_pat_a / _b: every integer in [-4, 4] is an
// e4m3 and an e2m1 value) with the scale pattern above
template <class F>
void fill_mx_pattern(MxProblem<F>& p) {
  const int blocks = (p.K + kMxBlock - 1) / kMxBlock;
  for (int i = 0; i < p.M; ++i) {
    for (int k = 0; k < p.K; ++k)
      p.set_a(i, k, F::encode(static_cast<float>(gemm_pat_a(i, k))));
    for (int kb = 0; kb < blocks; ++kb)
      p.sa[mx_scale_off(i, kb, p.Kb)] = static_cast<uint8_t>(127 + mx_pat_sa(i, kb));
  }
  for (int j = 0; j < p.N; ++j) {
    for (int k = 0; k < p.K; ++k)
      p.set_b(k, j, F::encode(static_cast<float>(gemm_pat_b(k, j))));
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

// the raw entry of format F: codes one per byte, row-major as given
template <class F>
void gemm_mx_raw(const uint8_t* a_codes, const uint8_t* a_scales,
                 const uint8_t* b_codes, const uint8_t* b_scales, float* c, int M,
                 int N, int K, int device) {
  MxProblem<F> p(M, N, K);
  const size_t blocks = (static_cast<size_t>(K) + kMxBlock - 1) / kMxBlock;
  for (int i = 0; i < M; ++i) {
    F::pack(a_codes + static_cast<size_t>(i) * K, K, p.row_a(i));
    scatter_scales(p.sa, i, p.Kb, a_scales + static_cast<size_t>(i) * blocks, blocks);
  }
  for (int k = 0; k < K; ++k)
    for (int j = 0; j < N; ++j) p.set_b(k, j, b_codes[static_cast<size_t>(k) * N + j]);
  for (int j = 0; j < N; ++j)
    scatter_scales(p.sbt, j, p.Kb, b_scales + j, blocks, N);
  run_once(p, device, c);
}

// the general entry of format F; who names the public entry in messages
template <class F>
void gemm_mx(const char* who, const float* a, const float* b, float* c, int M, int N,
             int K, int device) {
  MxProblem<F> p(M, N, K);
  for (size_t i = 0, n = static_cast<size_t>(M) * K; i < n; ++i)
    if (!std::isfinite(a[i]))
      throw std::invalid_argument(std::string(who) + ": a has a non-finite element");
  for (size_t i = 0, n = static_cast<size_t>(K) * N; i < n; ++i)
    if (!std::isfinite(b[i]))
      throw std::invalid_argument(std::string(who) + ": b has a non-finite element");
  const size_t blocks = (static_cast<size_t>(K) + kMxBlock - 1) / kMxBlock;
  std::vector<uint8_t> codes(K), scales(blocks);
  for (int i = 0; i < M; ++i) {
    mx_quantize_row<F>(a + static_cast<size_t>(i) * K, K, codes.data(), scales.data());
    F::pack(codes.data(), K, p.row_a(i));
    scatter_scales(p.sa, i, p.Kb, scales.data(), blocks);
  }
  std::vector<float> col(K);
  for (int j = 0; j < N; ++j) {
    for (int k = 0; k < K; ++k) col[k] = b[static_cast<size_t>(k) * N + j];
    mx_quantize_row<F>(col.data(), K, codes.data(), scales.data());
    F::pack(codes.data(), K, p.row_bt(j));
    scatter_scales(p.sbt, j, p.Kb, scales.data(), blocks);
  }
  run_once(p, device, c);
}

// the exact check and the timed run of format F on the scaled integer pattern
template <class F>
double run_mx_check(const char* who, int M, int N, int K, int device) {
  require_exact_mx_k(K, who);
  MxProblem<F> p(M, N, K);
  fill_mx_pattern(p);
  return run_full_check(p, device, mx_pattern_err);
}

template <class F>
GemmResult run_mx_timed(const char* who, int M, int N, int K, int iters, int device) {
  require_exact_mx_k(K, who);
  if (iters < 1) throw std::invalid_argument(std::string(who) + ": iters must be >= 1");
  MxProblem<F> p(M, N, K);
  fill_mx_pattern(p);
  return run_timed(p, iters, device, mx_pattern_err);
}

}  // namespace detail

// Raw entry: operands already quantized. a_codes M x K, a_scales M x
// ceil(K/32), b_codes K x N, b_scales ceil(K/32) x N, all row-major bytes;
// c M x N row-major float.
inline void gemm_mxfp8_raw(const uint8_t* a_codes, const uint8_t* a_scales,
                           const uint8_t* b_codes, const uint8_t* b_scales,
                           float* c, int M, int N, int K, int device = 0) {
  detail::gemm_mx_raw<detail::Mxfp8>(a_codes, a_scales, b_codes, b_scales, c, M, N, K,
                                     device);
}

// General entry: c[M,N] = mx(a[M,K]) · mx(b[K,N]), all row-major float. Rows
// of a and columns of b are MX-quantized (mx_quantize_row). Throws
// std::invalid_argument on a non-finite input, before any device work.
inline void gemm_mxfp8(const float* a, const float* b, float* c, int M, int N,
                       int K, int device = 0) {
  detail::gemm_mx<detail::Mxfp8>("gemm_mxfp8", a, b, c, M, N, K, device);
}

// Self-contained exact check: integer elements in [-4, 4] (gemm_pat_a / _b),
// scale exponents in [-2, 2] (mx_pat_sa / _sb), host reference in int64 in
// units of 2^-4; returns max |C - ref| over the whole M x N result (expect 0.0).
inline double run_mxgemm_check(int M, int N, int K, int device = 0) {
  return detail::run_mx_check<detail::Mxfp8>("run_mxgemm_check", M, N, K, device);
}

// Timed run on the same pattern: one warm-up launch, `iters` launches between
// events, then the 256 fixed, spread output elements of run_gemm are checked
// exactly. FLOPs are counted as 2 M N K.
inline GemmResult run_mxgemm(int M = 4096, int N = 4096, int K = 2048,
                             int iters = 10, int device = 0) {
  return detail::run_mx_timed<detail::Mxfp8>("run_mxgemm", M, N, K, iters, device);
}

}  // namespace payload

