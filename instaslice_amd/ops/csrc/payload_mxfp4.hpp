// gfx950 MXFP4 block-scaled matrix-core GEMM payload.
//
// gemm proves the bf16 MFMA path and mxgemm the MXFP8 one; this one proves the
// 4-bit path, the datapath an MI355X is bought for: the same instruction,
// v_mfma_scale_f32_16x16x128_f8f6f4, with the format selectors cbsz = blgp = 4
// (e2m1 operands, 4 VGPRs each) runs at four times the bf16 rate per clock and
// twice the e4m3 rate.
//
//   C[M,N] (fp32) = sum_k A[i,k] * 2^(sa[i,k/32]-127) * B[k,j] * 2^(sb[k/32,j]-127)
//
// A and B are OCP e2m1 codes (1 sign bit, 2 exponent bits of bias 1, 1 mantissa
// bit: magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6; no NaN, no infinity, both
// zeros), sa and sb E8M0 bytes, one per 32 consecutive K elements of a row of
// A or a column of B (the OCP MX block).
//
//   device image two elements per byte: element k of a row lives in byte k / 2,
//                even k in bits 3:0 and odd k in bits 7:4
//   block tile   128 x 128, K-step 256 elements, 256 threads (4 wave64s as 2 x 2)
//   wave tile    64 x 64 = 4 x 4 MFMA tiles of 16 x 16 (64 accumulator VGPRs)
//   staging      a K-step row is 128 bytes, so the staging loads, the
//                [128 rows][128 bytes] LDS image and its slot swizzle
//                (mx_lds_off) are the MXFP8 kernel's unchanged
//   sub-steps    each K-step is two sub-steps of 128 elements and 16 MFMAs;
//                sub-step s reads one ds_read_b128 per fragment, slot 4 s +
//                (l >> 4) of the row: the MXFP8 kernel's read of register
//                half s
//   fragment     measured on the hardware with one-hot operands and per-block
//                scales (profiles/mxfp4_probe.md; tests/test_mxfp4_payload.py
//                pins it): lane l holds row/col l & 15; the 32 nibbles of its
//                four registers are one whole MX block, block l >> 4 of the
//                instruction's 128 k (k = 32 (l >> 4) .. +31), and its scale
//                is taken from the lane itself, byte OPSEL of its scale
//                register: lane 16 kb + r supplies block kb of row/col r, as
//                for e4m3, but here the lane also holds that block's
//                elements. Nibble e of A's 16 bytes (e = 2 byte + (bits 7:4))
//                multiplies nibble e of B's, for every e. All 32 share one
//                scale, so the order of k inside a lane, the order of the two
//                nibbles of a byte included, cannot show in any result: even
//                k in bits 3:0 is this project's convention for the image,
//                which the hardware neither confirms nor contradicts. The
//                builtin takes eight registers; elements 4-7 are zeros and
//                the compiler drops them (4-VGPR operands in the ISA).
//   scales       as in the MXFP8 kernel: one dword per lane, operand and
//                128-element sub-step, holding the scales of the lane's block
//                for rows l & 15 of the wave's four MFMA tiles, picked by
//                OPSEL; the image is mx_scale_off's with one "K-step" of that
//                function per sub-step, both dwords prefetched one K-step
//                ahead like the tiles
//
// The host stores B transposed (N x K, K-contiguous), zero-pads M and N to 128
// and K to 256 (code 0 is +0) and pads the scale arrays to match with 127
// (2^0): the kernel has no edge branch and forms no address outside its
// buffers for any shape.
//
// Included by payload_core.hpp after payload_mxgemm.hpp (needs mx_lds_off,
// mx_scale_off, i32x4, i32x8, the kMx* constants, detail::mx_block_scale and
// the MX host layer that detail::Mxfp4 below parameterises: detail::MxProblem,
// gemm_mx, gemm_mx_raw, run_mx_check and run_mx_timed).

#pragma once

#include <algorithm>
#include <cmath>
#include <cstring>

namespace payload {

constexpr int kMx4BK = 256;            // e2m1 elements per K-step
constexpr int kMx4RowBytes = kMx4BK / 2;  // bytes per row of a K-step
constexpr int kMx4Sub = 128;           // elements per MFMA (a sub-step)

static_assert(kMx4RowBytes == kMxBK, "the LDS image is the MXFP8 kernel's");
static_assert(kMx4BK == 2 * kMx4Sub, "two sub-steps per K-step");
static_assert(kMx4Sub / kMxBlock == 4, "one scale byte per 16-lane group");

// ---- kernel --------------------------------------------------------------

// cbsz = blgp = 4: e2m1 operands in elements 0-3 of a and b. OA / OB pick the
// byte of sa / sb that holds the scale (the builtin wants them as constants).
template <int OA, int OB>
__device__ __forceinline__ f32x4 mx4_mfma(i32x4 a, i32x4 b, f32x4 c, int sa, int sb) {
  const i32x8 a8 = {a[0], a[1], a[2], a[3], 0, 0, 0, 0};
  const i32x8 b8 = {b[0], b[1], b[2], b[3], 0, 0, 0, 0};
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a8, b8, c, 4, 4, OA, sa,
                                                          OB, sb);
}

// a: Mp x Kp/2 bytes, bt: Np x Kp/2 bytes (B transposed), sa, sbt: scale
// images of Mp x Kp/32 and Np x Kp/32 bytes (mx_scale_off), c: Mp x Np; Mp and
// Np multiples of 128, Kp (in elements) a multiple of 256.
// grid = (Np / 128, Mp / 128).
__global__ __launch_bounds__(kBlock) void gemm_mxfp4_kernel(
    const uint8_t* __restrict__ a, const uint8_t* __restrict__ bt,
    const uint8_t* __restrict__ sa, const uint8_t* __restrict__ sbt,
    float* __restrict__ c, int Np, int Kp) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[(kMxBM + kMxBN) * kMx4RowBytes];
  uint8_t* lds_a = lds;
  uint8_t* lds_b = lds + kMxBM * kMx4RowBytes;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // keep it scalar
  const int wr = wave >> 1, wc = wave & 1;  // wave's 64x64 quadrant
  const int fr = lane & 15, fq = lane >> 4;

  // staging map: 8 consecutive lanes cover one 128-byte row of the K-step
  const int srow = tid >> 3, sslot = tid & 7;
  const size_t brow = static_cast<size_t>(blockIdx.y) * kMxBM;
  const size_t bcol = static_cast<size_t>(blockIdx.x) * kMxBN;
  const int Kbytes = Kp >> 1;  // bytes per row
  // block-uniform bases plus 32-bit lane offsets shared by both operands
  // (128 Kbytes < 2^32: the host limits Kp)
  const uint8_t* ga = a + brow * Kbytes;
  const uint8_t* gb = bt + bcol * Kbytes;
  unsigned soff[kMxLoads];
#pragma unroll
  for (int i = 0; i < kMxLoads; ++i)
    soff[i] = static_cast<unsigned>(srow + i * (kBlock / kMxSlots)) *
                  static_cast<unsigned>(Kbytes) + sslot * 16;

  // the lane's scale dwords: 64 dwords per wave tile and 128-element sub-step
  const size_t subs = static_cast<size_t>(Kp / kMx4Sub);
  const int* gsa = reinterpret_cast<const int*>(sa) +
                   (brow / 64 + wr) * subs * 64 + lane;
  const int* gsb = reinterpret_cast<const int*>(sbt) +
                   (bcol / 64 + wc) * subs * 64 + lane;

  i32x4 ra[kMxLoads], rb[kMxLoads];
  int nsa[2] = {gsa[0], gsa[64]}, nsb[2] = {gsb[0], gsb[64]};
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
  for (int b0 = 0; b0 < Kbytes; b0 += kMx4RowBytes) {
#pragma unroll
    for (int i = 0; i < kMxLoads; ++i) {
      int row = srow + i * (kBlock / kMxSlots);
      *reinterpret_cast<i32x4*>(lds_a + mx_lds_off(row, sslot)) = ra[i];
      *reinterpret_cast<i32x4*>(lds_b + mx_lds_off(row, sslot)) = rb[i];
    }
    const int sca[2] = {nsa[0], nsa[1]}, scb[2] = {nsb[0], nsb[1]};
    __syncthreads();

    if (b0 + kMx4RowBytes < Kbytes) {  // block-uniform: prefetch the next K-step
#pragma unroll
      for (int i = 0; i < kMxLoads; ++i) {
        ra[i] = *reinterpret_cast<const i32x4*>(ga + b0 + kMx4RowBytes + soff[i]);
        rb[i] = *reinterpret_cast<const i32x4*>(gb + b0 + kMx4RowBytes + soff[i]);
      }
      const int next = (b0 + kMx4RowBytes) / kMx4RowBytes * 128;
      nsa[0] = gsa[next];
      nsa[1] = gsa[next + 64];
      nsb[0] = gsb[next];
      nsb[1] = gsb[next + 64];
    }

    // sub-step s, lane l: A[row l&15][k = 128 s + 32 (l>>4) + j] and
    // B[k = 128 s + 32 (l>>4) + j][col l&15], j = 0..31: slot 4 s + (l>>4)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      i32x4 fb[4];
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        int row = wc * 64 + n * 16 + fr;
        fb[n] = *reinterpret_cast<const i32x4*>(lds_b + mx_lds_off(row, 4 * s + fq));
      }
      // one row of MFMA tiles at a time: only one A fragment is live
#define MX4_MFMA(m, n) \
  acc[m][n] = mx4_mfma<m, n>(fa, fb[n], acc[m][n], sca[s], scb[s])
#define MX4_MFMA_ROW(m)                                                          \
  {                                                                              \
    int row = wr * 64 + m * 16 + fr;                                             \
    i32x4 fa =                                                                   \
        *reinterpret_cast<const i32x4*>(lds_a + mx_lds_off(row, 4 * s + fq));    \
    MX4_MFMA(m, 0); MX4_MFMA(m, 1); MX4_MFMA(m, 2); MX4_MFMA(m, 3);              \
  }
      MX4_MFMA_ROW(0);
      MX4_MFMA_ROW(1);
      MX4_MFMA_ROW(2);
      MX4_MFMA_ROW(3);
#undef MX4_MFMA_ROW
#undef MX4_MFMA
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

// float -> OCP e2m1 code in bits 3:0 (bit 3 the sign). The nearest of 0, 0.5,
// 1, 1.5, 2, 3, 4, 6, a tie going to the code with mantissa bit 0; anything
// beyond 6, and +-inf, saturates to +-6; +-0 is kept. The format has no NaN:
// a NaN input is a precondition violation (callers reject it first) and comes
// back as +-6.
inline uint8_t to_e2m1_sat(float f) {
  const uint8_t sign = std::signbit(f) ? 8u : 0u;
  const float m = std::fabs(f);
  uint8_t code;
  if (m <= 0.25f) code = 0;        // tie 0.25 -> 0
  else if (m < 0.75f) code = 1;    // tie 0.75 -> 1.0
  else if (m <= 1.25f) code = 2;   // tie 1.25 -> 1.0
  else if (m < 1.75f) code = 3;    // tie 1.75 -> 2.0
  else if (m <= 2.5f) code = 4;    // tie 2.5 -> 2.0
  else if (m < 3.5f) code = 5;     // tie 3.5 -> 4.0
  else if (m <= 5.0f) code = 6;    // tie 5.0 -> 4.0
  else code = 7;                   // NaN compares false everywhere above
  return sign | code;
}

inline float from_e2m1(uint8_t code) {
  static const float mag[8] = {0.f, 0.5f, 1.f, 1.5f, 2.f, 3.f, 4.f, 6.f};
  const float v = mag[code & 7];
  return (code & 8) ? -v : v;
}

// OCP MX quantization of one row of K floats to e2m1: per block of 32 elements
// (a last partial block as if padded with zeros) one E8M0 scale byte
// clamp(floor(log2(amax)) - 2 + 127, 0, 254), 2 being the exponent of the
// largest e2m1 (6 = 1.5 * 2^2), and the elements to_e2m1_sat(x * 2^(127 -
// scale)). An all-zero block gets 127. codes: K bytes, one code each
// (unpacked), scales: ceil(K / 32). NaN is a precondition violation.
inline void mx4_quantize_row(const float* x, int K, uint8_t* codes, uint8_t* scales) {
  for (int k0 = 0; k0 < K; k0 += kMxBlock) {
    const int n = std::min(kMxBlock, K - k0);
    const int scale = detail::mx_block_scale(x + k0, n, 2);
    scales[k0 / kMxBlock] = static_cast<uint8_t>(scale);
    // x * 2^(127 - scale) < 8 whenever the clamp at 0 is not hit, and a power
    // of two scaling is exact unless the result is an fp32 subnormal, which is
    // far below the first tie (0.25) and becomes zero either way
    for (int k = 0; k < n; ++k)
      codes[k0 + k] = to_e2m1_sat(std::ldexp(x[k0 + k], 127 - scale));
  }
}

// The device byte image of one row of K codes (0..15, one per byte):
// ceil(K / 2) bytes, even k in bits 3:0 and odd k in bits 7:4, an odd tail
// padded with code 0.
inline void pack_fp4(const uint8_t* codes, int K, uint8_t* out) {
  for (int k = 0; k + 1 < K; k += 2)
    out[k / 2] = static_cast<uint8_t>((codes[k] & 15) | (codes[k + 1] << 4));
  if (K & 1) out[K / 2] = codes[K - 1] & 15;
}

// ---- host layer: the GEMM --------------------------------------------------

namespace detail {

// the e2m1 format of detail::MxProblem (payload_mxgemm.hpp): packed operands,
// K padded to 256; size limits as for e4m3
struct Mxfp4 {
  static constexpr const char* name = "mx4gemm";
  static constexpr int kBK = kMx4BK;
  static constexpr int kPerByte = 2;
  static constexpr auto kernel = gemm_mxfp4_kernel;
  static uint8_t encode(float f) { return to_e2m1_sat(f); }
  static void quantize_row(const float* x, int K, uint8_t* codes, uint8_t* scales) {
    mx4_quantize_row(x, K, codes, scales);
  }
  static void put(uint8_t& byte, size_t k, uint8_t code) {
    byte = (k & 1) ? static_cast<uint8_t>((byte & 0x0F) | (code << 4))
                   : static_cast<uint8_t>((byte & 0xF0) | (code & 15));
  }
  static void pack(const uint8_t* codes, int K, uint8_t* out) { pack_fp4(codes, K, out); }
};

}  // namespace detail

// Raw entry: operands already quantized. a_codes M x K, b_codes K x N, one
// e2m1 code (0..15) per byte; a_scales M x ceil(K/32), b_scales ceil(K/32) x N;
// all row-major bytes; c M x N row-major float. The host packs and transposes.
inline void gemm_mxfp4_raw(const uint8_t* a_codes, const uint8_t* a_scales,
                           const uint8_t* b_codes, const uint8_t* b_scales,
                           float* c, int M, int N, int K, int device = 0) {
  detail::gemm_mx_raw<detail::Mxfp4>(a_codes, a_scales, b_codes, b_scales, c, M, N, K,
                                     device);
}

// General entry: c[M,N] = mx4(a[M,K]) · mx4(b[K,N]), all row-major float. Rows
// of a and columns of b are MX-quantized to e2m1 (mx4_quantize_row). Throws
// std::invalid_argument on a non-finite input, before any device work.
inline void gemm_mxfp4(const float* a, const float* b, float* c, int M, int N,
                       int K, int device = 0) {
  detail::gemm_mx<detail::Mxfp4>("gemm_mxfp4", a, b, c, M, N, K, device);
}

// Self-contained exact check on the MXFP8 payload's pattern: integer elements
// in [-4, 4], scale exponents in [-2, 2], host reference in int64 in units of
// 2^-4; returns max |C - ref| over the whole M x N result (expect 0.0). The
// values and scales are the same numbers as there, so the exactness argument
// at kMxMaxExactK and its limit K <= 2048 carry over unchanged.
inline double run_mx4gemm_check(int M, int N, int K, int device = 0) {
  return detail::run_mx_check<detail::Mxfp4>("run_mx4gemm_check", M, N, K, device);
}

// Timed run on the same pattern, with run_mxgemm's defaults so that the two
// rates compare like for like: one warm-up launch, `iters` launches between
// events, then the same 256 fixed, spread output elements are checked
// exactly. FLOPs are counted as 2 M N K.
inline GemmResult run_mx4gemm(int M = 4096, int N = 4096, int K = 2048,
                              int iters = 10, int device = 0) {
  return detail::run_mx_timed<detail::Mxfp4>("run_mx4gemm", M, N, K, iters, device);
}

}  // namespace payload

