// gfx950 KV-cache decode attention payload.
//
// gemm / mxgemm prove the matrix cores and membw / memcheck the memory; this
// one proves the mix an LLM server in decode runs: single-token attention over
// a KV cache, a memory-bound stream of K and V through the matrix cores with an
// online softmax (transcendentals, cross-lane reductions) and a split-KV merge.
//
//   o[b,h,:] = softmax_t(scale * q[b,h,:] . k[b,g,t,:]) . v[b,g,t,:],  t < len[b]
//
// with kv head g = h / (Hq / Hkv) and head dim 128. q, k and v are bf16 (rounded
// on the host, round-to-nearest-even), both products run on
// v_mfma_f32_16x16x32_bf16 with fp32 accumulation, the softmax is fp32, P is
// rounded to bf16 for the PV product and the output is fp32.
//
//   workgroup    one per (sequence, kv head, KV split), 4 wave64s. The split's
//                32-key chunks are dealt round-robin to the waves; every wave
//                keeps its own running (m, l, o) and writes its own partial, so
//                there is no LDS and no barrier in the kernel.
//   MFMA tile    the kv head's G = Hq / Hkv <= 16 query heads are the 16 columns
//                (rows G .. 15 of the padded q image are zero)
//   QK           the swapped product S^T = K Q^T: A = 16 keys x 32 d of K,
//                B = 32 d x 16 heads of Q^T, four d-steps. The result has the
//                head on the lane (l & 15) and four keys in the registers, so a
//                head's chunk maximum is lane-local plus two xor-shuffles (lanes
//                l ^ 16 and l ^ 32).
//   key order    the rows of a QK tile may be any keys. Tile t (0, 1) of a chunk
//                takes key 8 (i >> 2) + 4 t + (i & 3) as its row i, so after both
//                tiles lane quarter q = l >> 4 holds exactly the keys 8 q .. 8 q
//                + 7 of the chunk, in order: its eight weights, rounded to bf16,
//                are the B fragment of the PV MFMA as they stand. P never leaves
//                the registers.
//   PV           O^T = V^T P^T: A = 16 d x 32 keys of V^T, B = 32 keys x 16
//                heads of P^T, eight d-tiles: 32 accumulator VGPRs, again with
//                the head on the lane, so the rescale by exp2(m_old - m_new) is
//                lane-local.
//   cache        the host owns the layout and stores both tensors in fragment
//                order, 8 KiB of K and 8 KiB of V per (sequence, kv head, chunk):
//                K as [tile 2][d-step 4][lane 64][8] and V, transposed, as
//                [d-tile 8][lane 64][8] (attn_k_off / attn_v_off). A lane's
//                fragment is one 16-byte run and the 64 fragments of one MFMA
//                operand are one contiguous KiB, so every load instruction is
//                fully coalesced and goes straight from global memory into
//                VGPRs. Nothing of K or V is staged in LDS: each byte is used
//                once. K is requested one chunk ahead, into the registers the
//                QK MFMAs have just read.
//   softmax      base 2: scale * log2(e) is folded into the scores. Keys t >=
//                len[b] are masked to -inf by index. A running maximum of -inf
//                (nothing seen yet, or a chunk with no valid key) is replaced by
//                0 in the exponent, so (-inf) - (-inf) never occurs. The maximum
//                is updated at every chunk (no deferred-rescale threshold).
//   split-KV     every wave writes an unnormalised (m, l, o[128]) in fp32;
//                attn_combine_kernel merges the 4 * splits partials of a head
//                with weights exp2(m_i - m) and does the only division, a true
//                `/`. A partial with m_i = -inf (an empty split) has weight 0.
//
// The host zero-pads the cache to whole 32-key chunks (Lp) and zeroes the keys
// at and beyond len[b]; the kernel reads chunks below ceil(len[b] / 32) only,
// and forms no address outside its buffers for any shape.
//
// Included by payload_core.hpp after the others (needs HIP_CHECK, kBlock,
// bf16x8, f32x4, to_bf16_rne, detail::DeviceBuffer, detail::time_launches,
// detail::round_up and detail::note_err). The host layer starts with what the
// prefill payload (payload_prefill.hpp) shares with this one.

#pragma once

#include <algorithm>
#include <cmath>
#include <cstring>

namespace payload {

constexpr int kAttnD = 128;              // head dim
constexpr int kAttnChunk = 32;           // keys per wave iteration
constexpr int kAttnWaves = kBlock / 64;  // partials per split
constexpr int kAttnMaxGroup = 16;        // query heads per kv head
constexpr int kAttnMaxSplits = 64;
constexpr double kAttnRelBound = 1.0 / 256;  // dense bound of both attention checks
constexpr int kAttnChunkElems = kAttnChunk * kAttnD;  // per tensor and chunk

static_assert(kAttnD % 32 == 0 && kAttnD % 16 == 0, "whole MFMA steps only");
static_assert(kAttnChunk == 32, "one PV k-step per chunk");

// ---- the selection pattern -------------------------------------------------
//
// All values are small integers, exact in bf16. K is 0 at the n selected keys
// of a (sequence, kv head) and <= -16 elsewhere: selected scores are exactly
// 0, every other score is <= -16 * 2 * 128 = -4096 (times scale: about -362),
// whose weight underflows to exactly 0 in fp32. So o = sum_selected v / n, a
// sum of at most 32 integers in [-4, 4] over a power of two: bit-exact in any
// accumulation order and for any split count.

__host__ __device__ inline int attn_sel_n(int len) {
  int n = 1;
  while (n * 2 <= len && n < 32) n *= 2;
  return n;
}

// key i (< n) of the selection of (b, g)
__host__ __device__ inline int attn_sel_key(int b, int g, int i, int len) {
  const long long n = attn_sel_n(len);
  return static_cast<int>((i * static_cast<long long>(len) / n + b + g) % len);
}

// is key t (< len) selected for (b, g)? floor(i len / n) is strictly
// increasing in i since len >= n, so only the smallest i that reaches u can hit
__host__ __device__ inline bool attn_selected(int b, int g, int t, int len) {
  const long long n = attn_sel_n(len);
  const long long u = ((static_cast<long long>(t) - b - g) % len + len) % len;
  const long long i = (u * n + len - 1) / len;
  return i < n && i * len / n == u;
}

__host__ __device__ inline int attn_pat_q(int b, int h, int d) {
  return 2 + static_cast<int>((3ll * b + 5ll * h + 7ll * d) % 4);
}
__host__ __device__ inline int attn_pat_v(int b, int g, int t, int d) {
  return static_cast<int>((3ll * b + 5ll * g + 7ll * t + 11ll * d) % 9) - 4;
}
// k where key t is not selected (0 where it is)
__host__ __device__ inline int attn_pat_k_off(int g, int t, int d) {
  return -16 - (t + d + g) % 3;
}

// ---- cache layout ------------------------------------------------------------

// element offset of (key w of the chunk, d) inside the chunk's K image: QK tile
// t = (w >> 2) & 1 has the key as its row fr = 4 (w >> 3) + (w & 3); d = 32 s
// + 8 fq + j sits in d-step s, lane 16 fq + fr, element j
__host__ __device__ inline int attn_k_off(int w, int d) {
  const int t = (w >> 2) & 1, fr = ((w >> 3) << 2) | (w & 3);
  const int s = d >> 5, fq = (d >> 3) & 3, j = d & 7;
  return (((t * 4 + s) * 64) + fq * 16 + fr) * 8 + j;
}

// the same for the V image: d = 16 dt + fr is row fr of d-tile dt, key w = 8 fq
// + j element j of lane 16 fq + fr
__host__ __device__ inline int attn_v_off(int w, int d) {
  const int dt = d >> 4, fr = d & 15, fq = w >> 3, j = w & 7;
  return ((dt * 64) + fq * 16 + fr) * 8 + j;
}

// ---- kernels -------------------------------------------------------------

// fp32 -> bf16 bits, round-to-nearest-even, for finite non-negative weights
__device__ __forceinline__ short attn_p_bf16(float f) {
  unsigned u = __float_as_uint(f);
  u += 0x7FFFu + ((u >> 16) & 1u);
  return static_cast<short>(u >> 16);
}

// q: [B][Hkv][16][128] bf16, rows G .. 15 zero. k, vt: [B][Hkv][Lp / 32] chunk
// images of 4096 bf16 (attn_k_off, attn_v_off). lens: [B]. Partials of head row = b Hq + h, part
// = split * 4 + wave, P = 4 * gridDim.x: pm, pl [row * P + part], po [(row * P
// + part) * 128 + d]. c2 = scale * log2(e). grid = (splits, Hkv, B).
__global__ __launch_bounds__(kBlock) void attn_decode_kernel(
    const uint16_t* __restrict__ q, const uint16_t* __restrict__ k,
    const uint16_t* __restrict__ vt, const int* __restrict__ lens,
    float* __restrict__ pm, float* __restrict__ pl, float* __restrict__ po,
    int G, int L, int Lp, float c2) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const int split = blockIdx.x, nsplit = gridDim.x;
  const int g = blockIdx.y, Hkv = gridDim.y, b = blockIdx.z;

  const int len = min(max(lens[b], 0), L);
  const int nch = (len + kAttnChunk - 1) / kAttnChunk;
  const int per = (nch + nsplit - 1) / nsplit;  // chunks per split
  const int ch_begin = split * per;
  const int ch_end = min(nch, ch_begin + per);  // <= ch_begin: an empty split

  const size_t bg = static_cast<size_t>(b) * Hkv + g;

  // B fragments of Q^T: lane l holds q[head l & 15][d = 32 s + 8 (l >> 4) + j]
  bf16x8 fqt[kAttnD / 32];
  {
    const uint16_t* qb = q + (bg * 16 + fr) * kAttnD + fq * 8;
#pragma unroll
    for (int s = 0; s < kAttnD / 32; ++s)
      fqt[s] = *reinterpret_cast<const bf16x8*>(qb + s * 32);
  }

  // A fragments, 512 elements apart. K: row fr of QK tile t is key 8 (fr >> 2)
  // + 4 t + (fr & 3) of the chunk, d = 32 s + 8 fq + j. V^T: row fr of d-tile dt
  // is d = 16 dt + fr, k index 8 fq + j is key 8 fq + j of the chunk.
  const size_t img = bg * (Lp / kAttnChunk) * kAttnChunkElems + lane * 8;
  const uint16_t* kb = k + img;
  const uint16_t* vb = vt + img;

  float m = -INFINITY, l = 0.f;  // l: this lane's 8 keys per chunk only
  f32x4 o[kAttnD / 16];
#pragma unroll
  for (int dt = 0; dt < kAttnD / 16; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

  // K runs one chunk ahead: its registers are free once the QK MFMAs have
  // read them, so the wave's next chunk is requested right there and arrives
  // under the softmax, the PV product and the next V loads. No extra registers.
  bf16x8 fk[2][kAttnD / 32];
  auto load_k = [&](int ch) {
    const uint16_t* kc = kb + static_cast<size_t>(ch) * kAttnChunkElems;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int s = 0; s < kAttnD / 32; ++s)
        fk[t][s] = *reinterpret_cast<const bf16x8*>(kc + (t * 4 + s) * 512);
  };
  if (ch_begin + wave < ch_end) load_k(ch_begin + wave);

  for (int ch = ch_begin + wave; ch < ch_end; ch += kAttnWaves) {  // wave-uniform
    const int c0 = ch * kAttnChunk;
    const uint16_t* vc = vb + static_cast<size_t>(ch) * kAttnChunkElems;
    bf16x8 fv[kAttnD / 16];
#pragma unroll
    for (int dt = 0; dt < kAttnD / 16; ++dt)
      fv[dt] = *reinterpret_cast<const bf16x8*>(vc + dt * 512);

    f32x4 st[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int s = 0; s < kAttnD / 32; ++s)
        st[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fk[t][s], fqt[s], st[t],
                                                        0, 0, 0);

    if (ch + kAttnWaves < ch_end) load_k(ch + kAttnWaves);

    // register r of tile t: row 4 fq + r, that is key c0 + 8 fq + 4 t + r
    float sc[8];
    float cm = -INFINITY;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int key = c0 + 8 * fq + j;
      sc[j] = key < len ? st[j >> 2][j & 3] * c2 : -INFINITY;
      cm = fmaxf(cm, sc[j]);
    }
    cm = fmaxf(cm, __shfl_xor(cm, 16));
    cm = fmaxf(cm, __shfl_xor(cm, 32));

    const float mn = fmaxf(m, cm);
    const float ms = mn == -INFINITY ? 0.f : mn;  // never (-inf) - (-inf)
    const float alpha = __builtin_amdgcn_exp2f(m - ms);  // m = -inf: 0
    m = mn;

    bf16x8 fp;
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float p = __builtin_amdgcn_exp2f(sc[j] - ms);
      sum += p;  // l takes the unrounded weight
      fp[j] = attn_p_bf16(p);
    }
    l = l * alpha + sum;

#pragma unroll
    for (int dt = 0; dt < kAttnD / 16; ++dt) {
      o[dt] *= alpha;
      o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fv[dt], fp, o[dt], 0, 0, 0);
    }
  }

  // the head's l is spread over its four lanes; alpha was common to them
  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);

  if (fr < G) {
    const int Hq = Hkv * G, P = nsplit * kAttnWaves;
    const size_t row = static_cast<size_t>(b) * Hq + static_cast<size_t>(g) * G + fr;
    const size_t part = row * P + split * kAttnWaves + wave;
    if (fq == 0) {
      pm[part] = m;
      pl[part] = l;
    }
    // C/D map: col (head) = lane & 15, row (d) = 16 dt + 4 (lane >> 4) + reg
#pragma unroll
    for (int dt = 0; dt < kAttnD / 16; ++dt)
      *reinterpret_cast<f32x4*>(po + part * kAttnD + dt * 16 + fq * 4) = o[dt];
  }
}

// out[row][d] = sum_i w_i po[row][i][d] / sum_i w_i pl[row][i], w_i = exp2(m_i
// - max m). grid = B Hq, block = 128 (one thread per d).
__global__ __launch_bounds__(kAttnD) void attn_combine_kernel(
    const float* __restrict__ pm, const float* __restrict__ pl,
    const float* __restrict__ po, float* __restrict__ out, int P) {
  const size_t row = blockIdx.x;
  const int d = threadIdx.x;
  const float* m = pm + row * P;
  const float* l = pl + row * P;
  const float* o = po + row * P * kAttnD + d;
  float mx = -INFINITY;
  for (int i = 0; i < P; ++i) mx = fmaxf(mx, m[i]);
  float ls = 0.f, acc = 0.f;
  for (int i = 0; i < P; ++i) {
    const float mi = m[i];
    if (mi == -INFINITY) continue;  // an empty part: weight 0, and mx may be -inf
    const float w = __builtin_amdgcn_exp2f(mi - mx);
    ls += w * l[i];
    acc += w * o[static_cast<size_t>(i) * kAttnD];
  }
  out[row * kAttnD + d] = acc / ls;  // the only division, and a true one
}

// Device-side fill of the selection pattern with full lengths (len = L) into
// the cache layout, one fragment (8 bf16, 16 bytes) of each tensor per thread
// and step; keys L .. Lp - 1 are zero. Small integers are exact in bf16, so
// the top 16 bits of the float are the value.
__device__ __forceinline__ uint16_t attn_int_bf16(int v) {
  return static_cast<uint16_t>(__float_as_uint(static_cast<float>(v)) >> 16);
}

__global__ __launch_bounds__(kBlock) void attn_fill_kv_kernel(
    uint16_t* __restrict__ k, uint16_t* __restrict__ vt, int Hkv, int L, int Lp,
    size_t groups) {  // groups = B Hkv Lp 128 / 8, per tensor
  size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x;
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  const size_t chunks = static_cast<size_t>(Lp / kAttnChunk);
  for (; i < groups; i += stride) {
    // group i is fragment (i / 64) % 8 of lane i % 64 of chunk image i / 512
    const size_t image = i / 512, bg = image / chunks;
    const int c0 = static_cast<int>(image % chunks) * kAttnChunk;
    const int b = static_cast<int>(bg / Hkv), g = static_cast<int>(bg % Hkv);
    const int frag = static_cast<int>(i / 64) & 7, lane = static_cast<int>(i) & 63;
    const int fr = lane & 15, fq = lane >> 4;
    bf16x8 kv, vv;
    {  // K fragment (tile frag >> 2, d-step frag & 3): one key, 8 d
      const int t = c0 + 8 * (fr >> 2) + 4 * (frag >> 2) + (fr & 3);
      const int d0 = 32 * (frag & 3) + 8 * fq;
      const bool sel = t < L && attn_selected(b, g, t, L);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        int val = 0;
        if (t < L && !sel) val = attn_pat_k_off(g, t, d0 + j);
        kv[j] = static_cast<short>(attn_int_bf16(val));
      }
    }
    {  // V fragment (d-tile frag): one d, 8 keys
      const int d = 16 * frag + fr;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int t = c0 + 8 * fq + j;
        vv[j] = static_cast<short>(attn_int_bf16(t < L ? attn_pat_v(b, g, t, d) : 0));
      }
    }
    *reinterpret_cast<bf16x8*>(k + i * 8) = kv;
    *reinterpret_cast<bf16x8*>(vt + i * 8) = vv;
  }
}

// ---- host layer ----------------------------------------------------------

// what run_attn_check and run_prefill_check return
struct AttnCheck {
  double max_err = 0;  // selection pattern: expect exactly 0
  double max_rel = 0;  // dense pattern: max |o - ref| / max |v|, <= kAttnRelBound
};

struct AttnResult {
  double kv_gb_s = 0;      // K and V bytes read per second
  double steps_per_s = 0;  // launches (decode steps of the whole batch)
  double tok_per_s = 0;    // steps_per_s * B
  double max_err = 0;
};

namespace detail {

// What both attention payloads ask of a shape; returns G = Hq / Hkv. `who`
// heads the messages. The arguments are 64-bit here and in the two checks
// built on it, so that a caller can check array extents before it narrows
// them to int.
inline long long attn_group(const char* who, long long b, long long hq, long long hkv,
                            long long len) {
  if (b < 1 || hq < 1 || hkv < 1 || len < 1)
    throw std::invalid_argument(std::string(who) + ": B, Hq, Hkv and L must be >= 1");
  if (hq % hkv != 0)
    throw std::invalid_argument(std::string(who) + ": Hq must be a multiple of Hkv");
  return hq / hkv;
}

// What both problems are: a checked shape, with the group size its check
// returned, on a device.
struct AttnShape {
  int B, Hq, Hkv, L, G, device;
};

inline float attn_default_scale() { return 1.0f / std::sqrt(static_cast<float>(kAttnD)); }

// the kernels' softmax is in base 2: scale * log2(e)
inline float attn_c2(float scale) { return scale * 1.4426950408889634f; }

// row t of the 16 spread rows that a timed run checks, out of `rows`
inline size_t attn_spread_row(int t, size_t rows) {
  return (static_cast<size_t>(t) * 1031 + 17) % rows;
}

// fp64 reference of one output row over its first n keys (all of them in
// decode and without a mask, i + 1 of them for row i under the causal mask),
// from the row's q and the float tensors k and v of its kv head (n x 128 or
// longer); w is scratch of n doubles
inline void attn_ref_row(double* out, const float* qr, const float* kh, const float* vh,
                         int n, double scale, std::vector<double>& w) {
  double mx = -INFINITY;
  for (int t = 0; t < n; ++t) {
    const float* kr = kh + static_cast<size_t>(t) * kAttnD;
    double s = 0;
    for (int d = 0; d < kAttnD; ++d) s += static_cast<double>(qr[d]) * kr[d];
    w[t] = s * scale;
    mx = std::max(mx, w[t]);
  }
  double den = 0;
  for (int t = 0; t < n; ++t) den += (w[t] = std::exp(w[t] - mx));
  for (int d = 0; d < kAttnD; ++d) {
    double num = 0;
    for (int t = 0; t < n; ++t) num += w[t] * vh[static_cast<size_t>(t) * kAttnD + d];
    out[d] = num / den;
  }
}

}  // namespace detail

// The limits of the decode payload, or std::invalid_argument; no HIP call.
// Returns Hq / Hkv.
inline int attn_decode_shape(long long B, long long Hq, long long Hkv, long long L,
                             long long splits = 0) {
  const long long G = detail::attn_group("attn", B, Hq, Hkv, L);
  if (G > kAttnMaxGroup)
    throw std::invalid_argument("attn: Hq / Hkv must be <= 16");
  if (splits < 0 || splits > kAttnMaxSplits)
    throw std::invalid_argument("attn: splits must be in 0 .. 64");
  if (B > 65535 || Hkv > 65535 || L > (1 << 28))
    throw std::invalid_argument("attn: shape too large");
  return static_cast<int>(G);
}

namespace detail {

// Shape, device buffers and launch of one decode problem.
struct AttnProblem : AttnShape {
  int splits;
  size_t Lp;
  DeviceBuffer dq, dk, dvt, dlens, dpm, dpl, dpo, dout;

  AttnProblem(int b, int hq, int hkv, int len, int want_splits, int dev)
      : AttnShape{b, hq, hkv, len, attn_decode_shape(b, hq, hkv, len, want_splits), dev},
        splits(want_splits), Lp(round_up(len, kAttnChunk)) {}

  static void check_lens(const int* lens, int B, int L) {
    if (!lens) return;
    for (int b = 0; b < B; ++b)
      if (lens[b] < 1 || lens[b] > L)
        throw std::invalid_argument("attn: lengths must be in 1 .. L");
  }

  size_t kv_elems() const { return static_cast<size_t>(B) * Hkv * Lp * kAttnD; }
  size_t rows() const { return static_cast<size_t>(B) * Hq; }
  int parts() const { return splits * kAttnWaves; }

  // splits = 0: enough workgroups for half the visible CUs, capped by the chunk
  // count. Measured on 256 CUs (profiles/attn_probe.md): with 256, 64 and 32
  // (sequence, kv head) pairs the best split counts were 1, 2 and 4, that is
  // 256, 128 and 128 workgroups, and covering the CUs twice lost 5 to 26 %. A
  // workgroup keeps 64 KiB of loads in flight, and every further split
  // shortens the waves' loops and adds partials to write and merge.
  void alloc() {
    HIP_CHECK(hipSetDevice(device));
    const int chunks = static_cast<int>(Lp / kAttnChunk);
    if (splits == 0) {
      int cus = 0;
      HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount,
                                      device));
      const long long pairs = static_cast<long long>(B) * Hkv;
      long long s = (std::max(cus, 1) + 2 * pairs - 1) / (2 * pairs);
      splits = static_cast<int>(std::min<long long>(
          std::max<long long>(s, 1), std::min(chunks, kAttnMaxSplits)));
    }
    dq.alloc(static_cast<size_t>(B) * Hkv * 16 * kAttnD * sizeof(uint16_t));
    dk.alloc(kv_elems() * sizeof(uint16_t));
    dvt.alloc(kv_elems() * sizeof(uint16_t));
    dlens.alloc(static_cast<size_t>(B) * sizeof(int));
    dpm.alloc(rows() * parts() * sizeof(float));
    dpl.alloc(rows() * parts() * sizeof(float));
    dpo.alloc(rows() * parts() * kAttnD * sizeof(float));
    dout.alloc(rows() * kAttnD * sizeof(float));
  }

  // q (B, Hq, 128) float -> the padded bf16 image; lens nullable (all L)
  void upload_q_lens(const float* q, const int* lens) {
    std::vector<uint16_t> hq(static_cast<size_t>(B) * Hkv * 16 * kAttnD, 0);
    for (int b = 0; b < B; ++b)
      for (int h = 0; h < Hq; ++h) {
        const size_t dst = ((static_cast<size_t>(b) * Hkv + h / G) * 16 + h % G) * kAttnD;
        const float* src = q + (static_cast<size_t>(b) * Hq + h) * kAttnD;
        for (int d = 0; d < kAttnD; ++d) hq[dst + d] = to_bf16_rne(src[d]);
      }
    std::vector<int> hl(B, L);
    if (lens) std::copy(lens, lens + B, hl.begin());
    HIP_CHECK(hipMemcpy(dq.p, hq.data(), hq.size() * sizeof(uint16_t),
                        hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dlens.p, hl.data(), hl.size() * sizeof(int),
                        hipMemcpyHostToDevice));
  }

  // k, v (B, Hkv, L, 128) float -> the chunk images in bf16; keys at and
  // beyond len[b] stay zero
  void upload_kv(const float* k, const float* v, const int* lens) {
    std::vector<uint16_t> hk(kv_elems(), 0), hvt(kv_elems(), 0);
    for (int b = 0; b < B; ++b) {
      const int len = lens ? lens[b] : L;
      for (int g = 0; g < Hkv; ++g) {
        const size_t bg = static_cast<size_t>(b) * Hkv + g;
        const float* ks = k + bg * L * kAttnD;
        const float* vs = v + bg * L * kAttnD;
        for (int t = 0; t < len; ++t) {
          const size_t image = (bg * (Lp / kAttnChunk) + t / kAttnChunk) * kAttnChunkElems;
          const int w = t % kAttnChunk;
          for (int d = 0; d < kAttnD; ++d) {
            hk[image + attn_k_off(w, d)] =
                to_bf16_rne(ks[static_cast<size_t>(t) * kAttnD + d]);
            hvt[image + attn_v_off(w, d)] =
                to_bf16_rne(vs[static_cast<size_t>(t) * kAttnD + d]);
          }
        }
      }
    }
    HIP_CHECK(hipMemcpy(dk.p, hk.data(), hk.size() * sizeof(uint16_t),
                        hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dvt.p, hvt.data(), hvt.size() * sizeof(uint16_t),
                        hipMemcpyHostToDevice));
  }

  void launch(float scale) const {
    const float c2 = attn_c2(scale);
    dim3 grid(static_cast<unsigned>(splits), static_cast<unsigned>(Hkv),
              static_cast<unsigned>(B));
    hipLaunchKernelGGL(attn_decode_kernel, grid, dim3(kBlock), 0, 0,
                       dq.as<const uint16_t>(), dk.as<const uint16_t>(),
                       dvt.as<const uint16_t>(), dlens.as<const int>(),
                       dpm.as<float>(), dpl.as<float>(), dpo.as<float>(), G, L,
                       static_cast<int>(Lp), c2);
    hipLaunchKernelGGL(attn_combine_kernel, dim3(static_cast<unsigned>(rows())),
                       dim3(kAttnD), 0, 0, dpm.as<const float>(),
                       dpl.as<const float>(), dpo.as<const float>(),
                       dout.as<float>(), parts());
  }

  void download(float* o) const {
    HIP_CHECK(hipMemcpy(o, dout.p, rows() * kAttnD * sizeof(float),
                        hipMemcpyDeviceToHost));
  }
};

// q (B, Hq, 128) of the selection pattern
inline void attn_pattern_q(float* q, int B, int Hq) {
  for (int b = 0; b < B; ++b)
    for (int h = 0; h < Hq; ++h)
      for (int d = 0; d < kAttnD; ++d)
        q[(static_cast<size_t>(b) * Hq + h) * kAttnD + d] =
            static_cast<float>(attn_pat_q(b, h, d));
}

// expected output row (b, h) of the selection pattern: sum of v over the
// selected keys, divided by their (power of two) count
inline void attn_pattern_row(float* out, int b, int h, int G, int len) {
  const int g = h / G, n = attn_sel_n(len);
  for (int d = 0; d < kAttnD; ++d) {
    int s = 0;
    for (int i = 0; i < n; ++i) s += attn_pat_v(b, g, attn_sel_key(b, g, i, len), d);
    out[d] = static_cast<float>(s) / static_cast<float>(n);
  }
}

// the dense pattern: a fixed integer hash, multiples of 2^-6 (exact in bf16)
inline uint32_t attn_hash(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}
// in [-range, range] / 64
inline float attn_dense(uint32_t tensor, size_t idx, int range) {
  const uint32_t h = attn_hash(static_cast<uint32_t>(idx) * 3u + tensor + 0x9e3779b9u);
  return static_cast<float>(static_cast<int>(h % (2u * range + 1u)) - range) / 64.0f;
}

}  // namespace detail

// General entry. q (B, Hq, 128), k and v (B, Hkv, L, 128), o (B, Hq, 128), all
// row-major float; lens (B) or null for full lengths; splits 0 = auto.
// std::invalid_argument on any unsupported shape or length, before any device
// work.
inline void attn_decode(const float* q, const float* k, const float* v,
                        const int* lens, float* o, int B, int Hq, int Hkv, int L,
                        float scale, int splits = 0, int device = 0) {
  detail::AttnProblem p(B, Hq, Hkv, L, splits, device);
  detail::AttnProblem::check_lens(lens, B, L);
  p.alloc();
  p.upload_q_lens(q, lens);
  p.upload_kv(k, v, lens);
  p.launch(scale);
  HIP_CHECK(hipGetLastError());
  p.download(o);
}

// Host only: q (B, Hq, 128), k, v (B, Hkv, L, 128) and the expected output (B,
// Hq, 128) of the selection pattern. Keys at and beyond len[b] get the
// non-selected K value and the pattern's V: they must not matter.
inline void attn_check_pattern(float* q, float* k, float* v, float* expected,
                               int B, int Hq, int Hkv, int L,
                               const int* lens = nullptr) {
  const int G = attn_decode_shape(B, Hq, Hkv, L);
  detail::AttnProblem::check_lens(lens, B, L);
  detail::attn_pattern_q(q, B, Hq);
  for (int b = 0; b < B; ++b) {
    const int len = lens ? lens[b] : L;
    for (int h = 0; h < Hq; ++h)
      detail::attn_pattern_row(expected + (static_cast<size_t>(b) * Hq + h) * kAttnD,
                               b, h, G, len);
    for (int g = 0; g < Hkv; ++g)
      for (int t = 0; t < L; ++t) {
        const size_t off = ((static_cast<size_t>(b) * Hkv + g) * L + t) * kAttnD;
        const bool sel = t < len && attn_selected(b, g, t, len);
        for (int d = 0; d < kAttnD; ++d) {
          k[off + d] = sel ? 0.f : static_cast<float>(attn_pat_k_off(g, t, d));
          v[off + d] = static_cast<float>(attn_pat_v(b, g, t, d));
        }
      }
  }
}

// Self-check at one shape, full lengths. (a) the selection pattern against its
// closed form: max_err, expect exactly 0. (b) a dense hash pattern (q in [-4,
// 4], k and v in [-1, 1], multiples of 2^-6) against an fp64 reference:
// max_rel = max |o - ref| / max |v|, expect <= 2^-8. Each bf16-rounded weight
// is off by at most 2^-9 relative and l is summed from the unrounded weights,
// so |o - ref| <= 2^-9 max |v| plus fp32 terms of order 1e-6; the bound
// doubles that.
inline AttnCheck run_attn_check(int B, int Hq, int Hkv, int L, int splits = 0,
                                int device = 0) {
  const int G = attn_decode_shape(B, Hq, Hkv, L, splits);  // validate first
  const size_t nq = static_cast<size_t>(B) * Hq * kAttnD;
  const size_t nkv = static_cast<size_t>(B) * Hkv * L * kAttnD;
  const float scale = detail::attn_default_scale();
  std::vector<float> q(nq), k(nkv), v(nkv), want(nq), got(nq);
  AttnCheck r;

  attn_check_pattern(q.data(), k.data(), v.data(), want.data(), B, Hq, Hkv, L);
  attn_decode(q.data(), k.data(), v.data(), nullptr, got.data(), B, Hq, Hkv, L,
              scale, splits, device);
  for (size_t i = 0; i < nq; ++i)
    detail::note_err(r.max_err, std::fabs(static_cast<double>(got[i]) -
                                          static_cast<double>(want[i])));

  double vmax = 0;
  for (size_t i = 0; i < nq; ++i) q[i] = detail::attn_dense(1, i, 256);
  for (size_t i = 0; i < nkv; ++i) {
    k[i] = detail::attn_dense(2, i, 64);
    v[i] = detail::attn_dense(3, i, 64);
    vmax = std::max(vmax, std::fabs(static_cast<double>(v[i])));
  }
  attn_decode(q.data(), k.data(), v.data(), nullptr, got.data(), B, Hq, Hkv, L,
              scale, splits, device);
  std::vector<double> w(L), ref(kAttnD);
  double max_abs = 0;
  for (int b = 0; b < B; ++b)
    for (int h = 0; h < Hq; ++h) {
      const size_t bg = static_cast<size_t>(b) * Hkv + h / G;
      const size_t at = (static_cast<size_t>(b) * Hq + h) * kAttnD;
      detail::attn_ref_row(ref.data(), q.data() + at, k.data() + bg * L * kAttnD,
                           v.data() + bg * L * kAttnD, L, static_cast<double>(scale), w);
      for (int d = 0; d < kAttnD; ++d)
        detail::note_err(max_abs, std::fabs(static_cast<double>(got[at + d]) - ref[d]));
    }
  r.max_rel = vmax > 0 ? max_abs / vmax : max_abs;
  return r;
}

// Timed run on the selection pattern at full lengths (so K is zero at the 32
// selected keys of every (sequence, kv head)): the cache is filled on the
// device, one warm-up launch, `iters` launches (decode + combine) between
// events, then 16 spread (b, h) output rows are checked exactly, so a fast
// wrong kernel cannot report a rate. KV bytes are 2 B Hkv L 128 2 per launch:
// 512 MiB at the default shape, above the 256 MiB Infinity Cache.
inline AttnResult run_attn(int B = 32, int Hq = 64, int Hkv = 8, int L = 4096,
                           int iters = 10, int device = 0, int splits = 0) {
  if (iters < 1) throw std::invalid_argument("run_attn: iters must be >= 1");
  detail::AttnProblem p(B, Hq, Hkv, L, splits, device);
  p.alloc();
  std::vector<float> q(p.rows() * kAttnD);
  detail::attn_pattern_q(q.data(), B, Hq);
  p.upload_q_lens(q.data(), nullptr);
  const size_t groups = p.kv_elems() / 8;
  hipLaunchKernelGGL(attn_fill_kv_kernel, dim3(grid_for(groups)), dim3(kBlock), 0, 0,
                     p.dk.as<uint16_t>(), p.dvt.as<uint16_t>(), Hkv, L,
                     static_cast<int>(p.Lp), groups);
  HIP_CHECK(hipGetLastError());
  const float scale = detail::attn_default_scale();
  const float ms = detail::time_launches(iters, [&p, scale] { p.launch(scale); });
  AttnResult r;
  const double sec = ms * 1e-3;
  r.steps_per_s = iters / sec;
  r.tok_per_s = r.steps_per_s * B;
  r.kv_gb_s = 2.0 * B * Hkv * static_cast<double>(L) * kAttnD * 2.0 * iters / sec / 1e9;
  std::vector<float> got(kAttnD), want(kAttnD);
  for (int t = 0; t < 16; ++t) {
    const size_t row = detail::attn_spread_row(t, p.rows());
    HIP_CHECK(hipMemcpy(got.data(), p.dout.as<float>() + row * kAttnD,
                        kAttnD * sizeof(float), hipMemcpyDeviceToHost));
    detail::attn_pattern_row(want.data(), static_cast<int>(row / Hq),
                             static_cast<int>(row % Hq), p.G, L);
    for (int d = 0; d < kAttnD; ++d)
      detail::note_err(r.max_err, std::fabs(static_cast<double>(got[d]) -
                                            static_cast<double>(want[d])));
  }
  return r;
}

}  // namespace payload
