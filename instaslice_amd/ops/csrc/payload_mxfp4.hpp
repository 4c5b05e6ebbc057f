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
// The kernel is gemm_mx_kernel<4> (payload_mxgemm.hpp, which has the tiles,
// the staging, the LDS and scale images and the lane map that both formats
// share). What is e2m1's own:
//
//   device image two elements per byte: element k of a row lives in byte k / 2,
//                even k in bits 3:0 and odd k in bits 7:4. A K-step row of 128
//                bytes is 256 elements, and K is zero-padded to 256 (code 0
//                is +0).
//   fragment     measured on the hardware with one-hot operands and per-block
//                scales (profiles/mxfp4_probe.md; tests/test_mxfp4_payload.py
//                pins it): the 32 nibbles of a lane's four registers are one
//                whole MX block, block l >> 4 of the instruction's 128 k (k =
//                32 (l >> 4) .. +31). Lane 16 kb + r supplies the scale of
//                block kb of row/col r, as for e4m3, but here the lane also
//                holds that block's elements. Nibble e of A's 16 bytes (e = 2
//                byte + (bits 7:4)) multiplies nibble e of B's, for every e.
//                All 32 share one scale, so the order of k inside a lane, the
//                order of the two nibbles of a byte included, cannot show in
//                any result: even k in bits 3:0 is this project's convention
//                for the image, which the hardware neither confirms nor
//                contradicts. The builtin takes eight registers; elements 4-7
//                are zeros and the compiler drops them (4-VGPR operands in
//                the ISA).
//
// Included by payload_core.hpp after payload_mxgemm.hpp (needs gemm_mx_kernel
// and the MX host layer that detail::Mxfp4 below parameterises:
// detail::mx_quantize_row, MxProblem, gemm_mx, gemm_mx_raw, run_mx_check and
// run_mx_timed).

#pragma once

#include <cmath>
#include <cstdint>

namespace payload {

constexpr int kMx4BK = 256;  // e2m1 elements per K-step: 128 bytes of a row

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
  static constexpr int kEmax = 2;  // 6 = 1.5 * 2^2
  static constexpr auto kernel = gemm_mx_kernel<4>;
  static uint8_t encode(float f) { return to_e2m1_sat(f); }
  static void put(uint8_t& byte, size_t k, uint8_t code) {
    byte = (k & 1) ? static_cast<uint8_t>((byte & 0x0F) | (code << 4))
                   : static_cast<uint8_t>((byte & 0xF0) | (code & 15));
  }
  static void pack(const uint8_t* codes, int K, uint8_t* out) { pack_fp4(codes, K, out); }
};

}  // namespace detail

// OCP MX quantization of one row of K floats to e2m1 (detail::mx_quantize_row
// in payload_mxgemm.hpp, with to_e2m1_sat). codes: K bytes, one code each
// (unpacked), scales: ceil(K / 32). NaN is a precondition violation.
inline void mx4_quantize_row(const float* x, int K, uint8_t* codes, uint8_t* scales) {
  detail::mx_quantize_row<detail::Mxfp4>(x, K, codes, scales);
}

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

