// gfx950 paged decode attention over an FP8 (OCP e4m3) KV cache.
//
// attn and paged stream a bf16 cache at close to the rate the memory gives, so
// the one way left to make a decode step faster is to read fewer bytes. A
// serving stack does that by keeping the cache in e4m3 with a scale per kv
// head and widening it on the fly. This payload is that path:
//
//   o[b,h,:] = softmax_t(scale * q[b,h,:] . K'_b[g,t,:]) . V'_b[g,t,:],  t < len[b]
//   K' = k_scale[g] * e4m3(k_code),   V' = v_scale[g] * e4m3(v_code)
//
// q is bf16 and both products run on v_mfma_f32_16x16x32_bf16, as in the bf16
// kernels: fp8 is the storage format, not the matrix format. The block table,
// the ragged lengths, shared pages, the device-side plan (in 64-key chunks),
// the partial format and attn_paged_combine_kernel are those of
// payload_attn_paged.hpp. What the data type changes:
//
//   chunk        64 keys per wave iteration, so that a tensor's chunk image is
//                8 KiB again, a lane load stays 16 bytes and the 64 lanes of
//                one load instruction read one contiguous KiB: 8 loads of K and
//                8 of V per chunk. Page sizes are 64, 128 and 256; the image of
//                (page p, kv head g, chunk c of the page) is at index
//                (p * Hkv + g) * (page / 64) + c.
//   widening     e4m3 -> bf16 is exact (3 mantissa bits, an exponent range
//                inside bf16's; subnormals and +-0 included) and happens in
//                registers, two codes per v_cvt_scalef32_pk_bf16_fp8 with a
//                scale operand of exactly 1.0. The eight low bytes of a lane's
//                16 become one bf16x8 MFMA operand, the eight high bytes the
//                next: no cross-lane movement, no byte shuffle.
//   K image      [load 8][lane 64][16 bytes], load = 2 tile + (d-step >> 1).
//                Lane 16 fq + fr of load (tile t, pair sp) holds key row fr of
//                QK tile t at d = 64 sp + 8 fq + j in bytes j = 0 .. 7 (d-step
//                2 sp) and d = 64 sp + 32 + 8 fq + j in bytes 8 + j (d-step
//                2 sp + 1). Row i of tile t (0 .. 3) is key 32 (t >> 1) +
//                8 (i >> 2) + 4 (t & 1) + (i & 3) of the chunk.
//   key order    so after the four S^T = K Q^T tiles lane quarter fq holds, in
//                order, the keys 8 fq .. 8 fq + 7 (tiles 0, 1) and 32 + 8 fq ..
//                32 + 8 fq + 7 (tiles 2, 3): its sixteen weights, rounded to
//                bf16, are the B fragments of the two 32-key PV k-steps as
//                they stand. P never leaves the registers.
//   V image      [d-tile 8][lane 64][16 bytes]. Lane 16 fq + fr of d-tile dt
//                holds row d = 16 dt + fr of V^T at the keys 8 fq + j in bytes
//                j (k-step 0) and 32 + 8 fq + j in bytes 8 + j (k-step 1).
//   scales       never applied per element: k_scale[g] is folded into the score
//                factor (one multiply per workgroup), v_scale[g] multiplies the
//                wave's 32 output accumulators once before the partial is
//                written.
//   softmax      one running-maximum update and one rescale of o per 64 keys,
//                half the bf16 kernel's VALU work per key, which pays for the
//                conversions. Masking by index, the -inf guards and l summed
//                from the unrounded weights are the bf16 kernel's.
//   prefetch     K is requested one chunk ahead into the 32 VGPRs the QK step
//                has just widened from; the table entry two chunks ahead by a
//                wave-uniform load.
//   stale keys   inside a chunk that is read, keys at and beyond len[b] are
//                masked by index: K there may be any non-NaN code, V must be a
//                non-NaN code (its weight is an exact 0 that goes through the
//                MFMA). Chunks at and beyond ceil(len[b] / 64) are never read,
//                nor are pages that no entry below a length names.
//
// Included by payload_core.hpp after payload_attn_paged.hpp, whose plan, combine
// kernel, problem struct, check case and timed run it uses, and after
// payload_mxgemm.hpp (to_e4m3_sat, from_e4m3).

#pragma once

namespace payload {

constexpr int kAttn8Chunk = 64;                          // keys per wave iteration
constexpr int kAttn8ChunkBytes = kAttn8Chunk * kAttnD;  // per tensor and chunk

// ---- cache layout ------------------------------------------------------------

// byte offset of (key w < 64 of the chunk, d) inside the chunk's K image
__host__ __device__ inline int attn8_k_off(int w, int d) {
  const int t = ((w >> 5) << 1) | ((w >> 2) & 1), fr = (((w & 31) >> 3) << 2) | (w & 3);
  const int s = d >> 5, fq = (d >> 3) & 3, j = d & 7;
  return (((t * 2 + (s >> 1)) * 64) + fq * 16 + fr) * 16 + (s & 1) * 8 + j;
}

// the same for the V image
__host__ __device__ inline int attn8_v_off(int w, int d) {
  const int dt = d >> 4, fr = d & 15, fq = (w & 31) >> 3, j = w & 7;
  return ((dt * 64) + fq * 16 + fr) * 16 + (w >> 5) * 8 + j;
}

// ---- the selection pattern in e4m3 -----------------------------------------
//
// payload_attn.hpp's pattern with every value an e4m3 value under power-of-two
// scales that differ between heads: K' is 0 at the selected keys and -16, -18
// or -20 elsewhere (codes -32 .. -80 under 2^-1 or 2^-2), V' is the integer
// pattern in -4 .. 4 (codes of multiples of 1/4 under 2^1 or 2^2). Unselected
// scores stay at or below -4096, their weights are exact zeros, and the result
// is bit-exact for any split.

__host__ __device__ inline float attn8_k_scale(int g) { return g % 2 ? 0.25f : 0.5f; }
__host__ __device__ inline float attn8_v_scale(int g) { return g % 2 ? 4.f : 2.f; }
__host__ __device__ inline int attn8_pat_k_off(int g, int t, int d) {
  return -16 - 2 * ((t + d + g) % 3);
}

// ---- kernels -------------------------------------------------------------

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 attn8_bf16x2 __attribute__((ext_vector_type(2)));

// eight e4m3 codes (two words) -> one bf16x8 MFMA operand, exactly
__device__ __forceinline__ bf16x8 attn8_widen(unsigned lo, unsigned hi) {
  struct Pairs {
    attn8_bf16x2 p[4];
  } w;
  w.p[0] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, false);
  w.p[1] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, true);
  w.p[2] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, false);
  w.p[3] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, true);
  return __builtin_bit_cast(bf16x8, w);
}

// The e4m3 cache format as the host layer of payload_attn_paged.hpp sees it: 64
// keys per chunk, one byte per element, codes taken as they are.
struct AttnCacheFp8 {
  using Elem = uint8_t;
  using Host = uint8_t;  // the host entry is given codes
  static constexpr int kChunk = kAttn8Chunk;
  static constexpr int kImage = kAttn8ChunkBytes;
  static constexpr int kLane = 16;

  static int k_off(int w, int d) { return attn8_k_off(w, d); }
  static int v_off(int w, int d) { return attn8_v_off(w, d); }
  static Elem encode(uint8_t code) { return code; }
};

// q: [B][Hkv][16][128] bf16, rows G .. 15 zero. kp, vp: the pool's chunk images
// of e4m3 codes. k_scale, v_scale: [Hkv]. table: [B][W]. shift = log2(page /
// 64). items, seq, nitems: the plan in 64-key chunks. Partials and grid as in
// attn_paged_decode_kernel, whose walk and chunk step this kernel repeats at 16
// keys per lane. One kernel templated over both formats computed the same bits
// but was 0.4 % slower on the ragged batch in this format
// (profiles/paged8_probe.md), so this body stays.
__global__ __launch_bounds__(kBlock) void attn_paged_decode_fp8_kernel(
    const uint16_t* __restrict__ q, const uint8_t* __restrict__ kp,
    const uint8_t* __restrict__ vp, const float* __restrict__ k_scale,
    const float* __restrict__ v_scale, const int* __restrict__ table,
    const int* __restrict__ lens, const int4* __restrict__ items,
    const int* __restrict__ nitems, const int2* __restrict__ seq,
    float* __restrict__ pm, float* __restrict__ pl, float* __restrict__ po, int G,
    int W, int shift, int Lmax, float c2) {
  if (static_cast<int>(blockIdx.y) >= *nitems) return;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const int g = blockIdx.x, Hkv = gridDim.x;

  const int4 it = items[blockIdx.y];
  const int b = it.x, ch_end = it.z;
  const int len = min(max(lens[b], 0), Lmax);
  const int* trow = table + static_cast<size_t>(b) * W;
  const int cmask = (1 << shift) - 1;
  const float c2k = c2 * k_scale[g];  // the K scale, once per workgroup

  // byte offset of this lane's first 16 bytes in chunk ch of physical page pg
  auto image = [&](int pg, int ch) {
    const size_t idx =
        ((static_cast<size_t>(pg) * Hkv + g) << shift) + static_cast<size_t>(ch & cmask);
    return idx * kAttn8ChunkBytes + static_cast<size_t>(lane) * 16;
  };

  bf16x8 fqt[kAttnD / 32];
  {
    const uint16_t* qb =
        q + ((static_cast<size_t>(b) * Hkv + g) * 16 + fr) * kAttnD + fq * 8;
#pragma unroll
    for (int s = 0; s < kAttnD / 32; ++s)
      fqt[s] = *reinterpret_cast<const bf16x8*>(qb + s * 32);
  }

  float m = -INFINITY, l = 0.f;
  f32x4 o[kAttnD / 16];
#pragma unroll
  for (int dt = 0; dt < kAttnD / 16; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

  u32x4 rk[8];  // the chunk's K codes: 64 keys in the 32 VGPRs of 32 bf16 keys
  auto load_k = [&](int pg, int ch) {
    const uint8_t* kc = kp + image(pg, ch);
#pragma unroll
    for (int i = 0; i < 8; ++i) rk[i] = *reinterpret_cast<const u32x4*>(kc + i * 1024);
  };

  // pg_v: the page of the chunk in hand; pg_k: the page of the wave's next chunk
  int ch = it.y + wave;
  int pg_v = 0, pg_k = 0;
  if (ch < ch_end) {
    pg_v = trow[ch >> shift];
    load_k(pg_v, ch);
  }
  if (ch + kAttnWaves < ch_end) pg_k = trow[(ch + kAttnWaves) >> shift];

  for (; ch < ch_end; ch += kAttnWaves) {  // wave-uniform
    const int c0 = ch * kAttn8Chunk;
    const uint8_t* vc = vp + image(pg_v, ch);
    u32x4 rv[kAttnD / 16];
#pragma unroll
    for (int dt = 0; dt < kAttnD / 16; ++dt)
      rv[dt] = *reinterpret_cast<const u32x4*>(vc + dt * 1024);

    // tile t, d-step pair sp: bytes 0 .. 7 are d-step 2 sp, bytes 8 .. 15 the next
    f32x4 st[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      st[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int sp = 0; sp < 2; ++sp) {
        const u32x4 r = rk[t * 2 + sp];
        st[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(attn8_widen(r.x, r.y),
                                                        fqt[2 * sp], st[t], 0, 0, 0);
        st[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(attn8_widen(r.z, r.w),
                                                        fqt[2 * sp + 1], st[t], 0, 0, 0);
      }
    }

    const int nx = ch + kAttnWaves;
    if (nx < ch_end) load_k(pg_k, nx);
    pg_v = pg_k;
    if (nx + kAttnWaves < ch_end) pg_k = trow[(nx + kAttnWaves) >> shift];

    // register r of tile t: key c0 + 32 (t >> 1) + 8 fq + 4 (t & 1) + r, so
    // sc[j] is key c0 + 32 (j >> 3) + 8 fq + (j & 7)
    float sc[16];
    float cm = -INFINITY;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int key = c0 + 32 * (j >> 3) + 8 * fq + (j & 7);
      sc[j] = key < len ? st[j >> 2][j & 3] * c2k : -INFINITY;
      cm = fmaxf(cm, sc[j]);
    }
    cm = fmaxf(cm, __shfl_xor(cm, 16));
    cm = fmaxf(cm, __shfl_xor(cm, 32));

    const float mn = fmaxf(m, cm);
    const float ms = mn == -INFINITY ? 0.f : mn;  // never (-inf) - (-inf)
    const float alpha = __builtin_amdgcn_exp2f(m - ms);  // m = -inf: 0
    m = mn;

    bf16x8 fp[2];
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const float p = __builtin_amdgcn_exp2f(sc[j] - ms);
      sum += p;  // l takes the unrounded weight
      fp[j >> 3][j & 7] = attn_p_bf16(p);
    }
    l = l * alpha + sum;

#pragma unroll
    for (int dt = 0; dt < kAttnD / 16; ++dt) {
      const u32x4 r = rv[dt];
      o[dt] *= alpha;
      o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(attn8_widen(r.x, r.y), fp[0],
                                                      o[dt], 0, 0, 0);
      o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(attn8_widen(r.z, r.w), fp[1],
                                                      o[dt], 0, 0, 0);
    }
  }

  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);

  if (fr < G) {
    const float vs = v_scale[g];  // the V scale, once per accumulator
    const int2 sq = seq[b];
    const size_t Hq = static_cast<size_t>(Hkv) * G;
    const size_t part = static_cast<size_t>(sq.x) * Hq +
                        (static_cast<size_t>(g) * G + fr) * sq.y +
                        static_cast<size_t>(it.w) * kAttnWaves + wave;
    if (fq == 0) {
      pm[part] = m;
      pl[part] = l;
    }
#pragma unroll
    for (int dt = 0; dt < kAttnD / 16; ++dt)
      *reinterpret_cast<f32x4*>(po + part * kAttnD + dt * 16 + fq * 4) = o[dt] * vs;
  }
}

// e4m3 code of a value that e4m3 holds exactly: 0, or a normal with three
// mantissa bits
__device__ __forceinline__ unsigned attn8_exact_code(float v) {
  const unsigned u = __float_as_uint(v);
  if ((u & 0x7FFFFFFFu) == 0) return 0;
  return ((u >> 24) & 0x80u) | (((u >> 20) & 0x7FFu) - (120u << 3));
}

// Device-side fill of the e4m3 selection pattern at the lengths lens[b], 16
// bytes of each tensor per thread and step, over the logical 64-key chunks of
// all W pages of every sequence, through the table; keys at and beyond lens[b]
// are zero.
__global__ __launch_bounds__(kBlock) void attn_paged_fill_fp8_kernel(
    uint8_t* __restrict__ k, uint8_t* __restrict__ v, const int* __restrict__ table,
    const int* __restrict__ lens, int Hkv, int W, int shift,
    size_t groups) {  // groups = B Hkv (W << shift) 8192 / 16, per tensor
  size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x;
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  const size_t chunks = static_cast<size_t>(W) << shift;
  for (; i < groups; i += stride) {
    // group i: load (i / 64) % 8 of lane i % 64 of logical chunk image i / 512
    const size_t image = i / 512, bg = image / chunks;
    const int lc = static_cast<int>(image % chunks), c0 = lc * kAttn8Chunk;
    const int b = static_cast<int>(bg / Hkv), g = static_cast<int>(bg % Hkv);
    const int L = lens[b];
    const size_t pg = static_cast<size_t>(table[static_cast<size_t>(b) * W + (lc >> shift)]);
    const size_t dst = ((pg * Hkv + g) << shift) + (lc & ((1 << shift) - 1));
    const int load = static_cast<int>(i / 64) & 7, lane = static_cast<int>(i) & 63;
    const int fr = lane & 15, fq = lane >> 4;
    const float ks = attn8_k_scale(g), vs = attn8_v_scale(g);
    u32x4 kw = {0, 0, 0, 0}, vw = {0, 0, 0, 0};
    {  // K (tile load >> 1, d-step pair load & 1): one key, 16 d
      const int tile = load >> 1, sp = load & 1;
      const int t = c0 + 32 * (tile >> 1) + 8 * (fr >> 2) + 4 * (tile & 1) + (fr & 3);
      const bool off = t < L && !attn_selected(b, g, t, L);
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int d = 64 * sp + 32 * (j >> 3) + 8 * fq + (j & 7);
        const float val = off ? static_cast<float>(attn8_pat_k_off(g, t, d)) / ks : 0.f;
        kw[j >> 2] |= attn8_exact_code(val) << (8 * (j & 3));
      }
    }
    {  // V (d-tile load): one d, 16 keys
      const int d = 16 * load + fr;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int t = c0 + 32 * (j >> 3) + 8 * fq + (j & 7);
        const float val = t < L ? static_cast<float>(attn_pat_v(b, g, t, d)) / vs : 0.f;
        vw[j >> 2] |= attn8_exact_code(val) << (8 * (j & 3));
      }
    }
    const size_t at = (dst * 512 + i % 512) * 16;
    *reinterpret_cast<u32x4*>(k + at) = kw;
    *reinterpret_cast<u32x4*>(v + at) = vw;
  }
}

// ---- host layer ----------------------------------------------------------

struct AttnPaged8Result : AttnPagedResult {
  double us = 0;         // per step (plan + decode + combine)
  double bf16_us = 0;    // the bf16 paged kernel on the same shape and lengths
  double quant_rel = 0;  // fp8 result against fp64 on unquantised dense data
};

// The limits of the fp8 paged payload, or std::invalid_argument; no HIP call.
// Returns Hq / Hkv.
inline int attn_paged_fp8_shape(long long B, long long Hq, long long Hkv, long long page,
                                long long W, long long P, long long workgroups = 0) {
  if (page != 64 && page != 128 && page != 256)
    throw std::invalid_argument("attn_paged_fp8: page must be 64, 128 or 256");
  return attn_paged_shape(B, Hq, Hkv, page, W, P, workgroups);
}

namespace detail {

inline bool attn8_nan_code(uint8_t c) { return (c & 0x7F) == 0x7F; }

// The paged problem over the e4m3 cache: its limits and its scales.
struct AttnPaged8Problem : AttnPagedProblem<AttnCacheFp8> {
  DeviceBuffer dks, dvs;

  AttnPaged8Problem(int b, int hq, int hkv, int pg, int w, int p, int workgroups, int dev)
      : AttnPagedProblem(b, hq, hkv, pg, w, p, workgroups, dev) {
    attn_paged_fp8_shape(b, hq, hkv, pg, w, p, workgroups);
  }

  void alloc() {
    AttnPagedProblem::alloc();
    dks.alloc(static_cast<size_t>(Hkv) * sizeof(float));
    dvs.alloc(static_cast<size_t>(Hkv) * sizeof(float));
  }

  void upload_scales(const float* ks, const float* vs) {
    HIP_CHECK(hipMemcpy(dks.p, ks, static_cast<size_t>(Hkv) * sizeof(float),
                        hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dvs.p, vs, static_cast<size_t>(Hkv) * sizeof(float),
                        hipMemcpyHostToDevice));
  }

  // plan (64-key chunks) + decode + combine
  void launch(float scale) const {
    plan();
    hipLaunchKernelGGL(attn_paged_decode_fp8_kernel, grid(), dim3(kBlock), 0, 0,
                       dq.as<const uint16_t>(), dk.as<const uint8_t>(),
                       dvt.as<const uint8_t>(), dks.as<const float>(),
                       dvs.as<const float>(), dtable.as<const int>(),
                       dlens.as<const int>(), ditems.as<const int4>(),
                       dnitems.as<const int>(), dseq.as<const int2>(), dpm.as<float>(),
                       dpl.as<float>(), dpo.as<float>(), G, W, shift(), L, attn_c2(scale));
    combine();
  }
};

}  // namespace detail

// General entry. q (B, Hq, 128) float; k_codes and v_codes (P, Hkv, page, 128)
// e4m3 bytes in plain key-major order; k_scale and v_scale (Hkv) float; table
// (B, W) and lens (B) int32; o (B, Hq, 128) float; workgroups 0 = auto.
// std::invalid_argument on an unsupported shape, a scale that is not finite and
// positive, a length outside 1 .. W page, a table entry below a length outside
// 0 .. P - 1, a non-finite q or a NaN code (0x7F, 0xFF) in a key of a 64-key
// chunk that will be read; all before any device work.
inline void attn_paged_decode_fp8(const float* q, const uint8_t* k_codes,
                                  const uint8_t* v_codes, const float* k_scale,
                                  const float* v_scale, const int* table, const int* lens,
                                  float* o, int B, int Hq, int Hkv, int page, int W, int P,
                                  float scale, int workgroups = 0, int device = 0) {
  detail::AttnPaged8Problem p(B, Hq, Hkv, page, W, P, workgroups, device);
  detail::attn_paged_check_table(table, lens, B, page, W, P);
  for (int g = 0; g < Hkv; ++g)
    if (!std::isfinite(k_scale[g]) || !std::isfinite(v_scale[g]) || k_scale[g] <= 0 ||
        v_scale[g] <= 0)
      throw std::invalid_argument("attn_paged_fp8: scales must be finite and > 0");
  for (size_t i = 0, n = p.rows() * kAttnD; i < n; ++i)
    if (!std::isfinite(q[i]))
      throw std::invalid_argument("attn_paged_fp8: q has a non-finite element");
  detail::attn_paged_check_read(
      k_codes, v_codes, table, lens, B, Hkv, page, W, kAttn8Chunk, detail::attn8_nan_code,
      "attn_paged_fp8: k or v has a NaN code in a chunk that is read");
  p.alloc();
  p.upload_q_table(q, table, lens);
  p.upload_scales(k_scale, v_scale);
  p.upload_pool(k_codes, v_codes);
  p.launch(scale);
  HIP_CHECK(hipGetLastError());
  p.download(o);
}

namespace detail {

// The paged case of the fp8 checks: the pool is all NaN codes but for what will
// be read, with 448 (0x7E) at the stale keys of a read chunk.
struct Attn8Case : AttnPagedCase {
  std::vector<float> ks, vs;

  Attn8Case(int b, int hq, int hkv, int pg, std::vector<int> lengths, int wg, int dev)
      : AttnPagedCase(b, hq, hkv, pg, std::move(lengths), wg, dev), ks(hkv), vs(hkv) {}

  // kv head of dense element i of (B, Hkv, Lmax, 128)
  int head(size_t i) const {
    return static_cast<int>(i / (static_cast<size_t>(Lmax) * kAttnD) % Hkv);
  }

  // dense codes (B, Hkv, Lmax, 128) -> the pool -> the kernel
  void decode(const float* q, const uint8_t* kc, const uint8_t* vc, float* got) const {
    const std::vector<uint8_t> kpool = pool<uint8_t>(kc, 0x7F, 0x7E, kAttn8Chunk);
    const std::vector<uint8_t> vpool = pool<uint8_t>(vc, 0x7F, 0x7E, kAttn8Chunk);
    attn_paged_decode_fp8(q, kpool.data(), vpool.data(), ks.data(), vs.data(),
                          table.data(), lens.data(), got, B, Hq, Hkv, page, W, P,
                          attn_default_scale(), workgroups, device);
  }

  // The dense hash pattern of run_attn_check (q in [-4, 4], k and v in [-1, 1])
  // quantised with to_e4m3_sat under scales near 1 / 448 that are no powers of
  // two and differ between heads. max_rel: against fp64 on the dequantised
  // values. quant_rel: against fp64 on the unquantised ones.
  void dense(double& max_rel, double& quant_rel) {
    std::vector<float> q(nq()), k(nkv()), v(nkv()), kd(nkv()), vd(nkv()), got(nq());
    std::vector<uint8_t> kc(nkv()), vc(nkv());
    for (int g = 0; g < Hkv; ++g) {
      ks[g] = (1.f + 0.25f * (g % 2)) / 448.f;
      vs[g] = (1.f + 0.5f * (g % 2)) / 448.f;
    }
    for (size_t i = 0; i < nq(); ++i) q[i] = attn_dense(1, i, 256);
    for (size_t i = 0; i < nkv(); ++i) {
      const int g = head(i);
      k[i] = attn_dense(2, i, 64);
      v[i] = attn_dense(3, i, 64);
      kc[i] = to_e4m3_sat(k[i] / ks[g]);
      vc[i] = to_e4m3_sat(v[i] / vs[g]);
      kd[i] = from_e4m3(kc[i]) * ks[g];
      vd[i] = from_e4m3(vc[i]) * vs[g];
    }
    decode(q.data(), kc.data(), vc.data(), got.data());
    max_rel = rel_error(got.data(), q.data(), kd.data(), vd.data());
    quant_rel = rel_error(got.data(), q.data(), k.data(), v.data());
  }
};

}  // namespace detail

// Self-check. ragged: sequence b takes entry b % 8 of {L, 1, 33, 63, 64, 65,
// 2 page + 1, the largest multiple of 64 up to max(64, L / 2)}, each at most L:
// from B = 8 on the batch holds a single key, an empty second k-step, one key
// short of, at and past a chunk, and one key past a page boundary. Otherwise
// every length is L. Pool, table and stale keys as in detail::Attn8Case. (a)
// the e4m3 selection pattern against its closed form: max_err, expect exactly
// 0. (b) dense data (Attn8Case::dense): max_rel <= 2^-8. The widening is exact,
// so the roundings are the bf16 kernel's and its bound holds; the fp32 scale
// folds add relative errors near 2^-24, far inside the bound's factor of two.
inline AttnCheck run_attn_paged_fp8_check(int B, int Hq, int Hkv, int L, int page = 64,
                                          int workgroups = 0, bool ragged = true,
                                          int device = 0) {
  if (L < 1 || L > (1 << 24))
    throw std::invalid_argument("attn_paged_fp8: L must be in 1 .. 2^24");
  attn_paged_fp8_shape(B, Hq, Hkv, page, 1, 1, workgroups);  // page before it divides
  const int rule[8] = {L, 1, 33, 63, 64, 65, 2 * page + 1, std::max(64, L / 2) / 64 * 64};
  std::vector<int> lens(B, L);
  if (ragged)
    for (int b = 0; b < B; ++b) lens[b] = std::min(L, rule[b % 8]);
  detail::Attn8Case c(B, Hq, Hkv, page, lens, workgroups, device);

  std::vector<float> q(c.nq()), want(c.nq()), got(c.nq());
  std::vector<uint8_t> kc(c.nkv()), vc(c.nkv());
  detail::attn_pattern_q(q.data(), B, Hq);
  for (int g = 0; g < Hkv; ++g) {
    c.ks[g] = attn8_k_scale(g);
    c.vs[g] = attn8_v_scale(g);
  }
  for (int b = 0; b < B; ++b) {
    for (int h = 0; h < Hq; ++h)
      detail::attn_pattern_row(want.data() + (static_cast<size_t>(b) * Hq + h) * kAttnD, b,
                               h, c.G, lens[b]);
    for (int g = 0; g < Hkv; ++g)
      for (int t = 0; t < lens[b]; ++t) {
        const size_t off = ((static_cast<size_t>(b) * Hkv + g) * c.Lmax + t) * kAttnD;
        const bool sel = attn_selected(b, g, t, lens[b]);
        for (int d = 0; d < kAttnD; ++d) {
          kc[off + d] = to_e4m3_sat(sel ? 0.f : attn8_pat_k_off(g, t, d) / c.ks[g]);
          vc[off + d] = to_e4m3_sat(attn_pat_v(b, g, t, d) / c.vs[g]);
        }
      }
  }
  AttnCheck r;
  c.decode(q.data(), kc.data(), vc.data(), got.data());
  r.max_err = detail::attn_max_err(got.data(), want.data(), c.nq());
  double quant_rel;
  c.dense(r.max_rel, quant_rel);
  return r;
}

// Timed run on the e4m3 selection pattern, shaped like run_attn_paged: W =
// ceil(L / page) pages per sequence under a fixed scrambled table over a pool
// of B W + 3 pages, filled on the device through the table; one warm-up launch,
// `iters` launches (plan + decode + combine) between events, then 16 spread
// (b, h) rows are checked exactly. KV bytes are sum_b lens[b] Hkv 128 2 per
// launch, half of the bf16 cache's. bf16_us is run_attn_paged on the same
// arguments, in this process, for comparison. quant_rel is Attn8Case::dense's,
// on up to 4 sequences of min(L, 300) keys: a property of the format, reported
// and never judged.
inline AttnPaged8Result run_attn_paged_fp8(int B = 32, int Hq = 64, int Hkv = 8,
                                           int L = 4096, int page = 64, int iters = 10,
                                           bool ragged = false, int workgroups = 0,
                                           int device = 0) {
  using C = AttnCacheFp8;
  const detail::AttnPagedTimed t("run_attn_paged_fp8", attn_paged_fp8_shape, B, Hq, Hkv, L,
                                 page, iters, ragged, workgroups);
  const float scale = detail::attn_default_scale();
  AttnPaged8Result r;
  {
    detail::AttnPaged8Problem p(B, Hq, Hkv, page, t.W, t.P, workgroups, device);
    const float ms = t.time(
        r, p,
        [&] {
          std::vector<float> ks(Hkv), vs(Hkv);
          for (int g = 0; g < Hkv; ++g) {
            ks[g] = attn8_k_scale(g);
            vs[g] = attn8_v_scale(g);
          }
          p.upload_scales(ks.data(), vs.data());
          const size_t groups = static_cast<size_t>(B) * Hkv * t.W * page * kAttnD / C::kLane;
          hipLaunchKernelGGL(attn_paged_fill_fp8_kernel, dim3(grid_for(groups)),
                             dim3(kBlock), 0, 0, p.dk.as<uint8_t>(), p.dvt.as<uint8_t>(),
                             p.dtable.as<const int>(), p.dlens.as<const int>(), Hkv, t.W,
                             p.shift(), groups);
        },
        [&p, scale] { p.launch(scale); });
    r.us = ms * 1e-3 / iters * 1e6;
    t.report(r, ms, p.dout.as<float>(), 2 * sizeof(C::Elem));
  }
  r.bf16_us =
      1e6 / run_attn_paged(B, Hq, Hkv, L, page, iters, ragged, workgroups, device)
                .steps_per_s;
  const int Bd = std::min(B, 4);
  detail::Attn8Case c(Bd, Hq, Hkv, page, std::vector<int>(Bd, std::min(L, 300)),
                      workgroups, device);
  double max_rel;
  c.dense(max_rel, r.quant_rel);
  return r;
}

}  // namespace payload
