// gfx950 causal prefill attention payload.
//
// attn proves decode, the memory-bound half of serving. This one proves the
// other half: attention over a whole prompt under a causal mask, where every
// K / V byte is reused by hundreds of query rows, so the kernel is bound by
// the matrix cores with v_exp_f32 and cross-lane work between the MFMAs, and
// K / V travel through LDS (staging, swizzle, barriers), a path no other
// payload uses.
//
//   o[b,h,i,:] = softmax_t(scale * q[b,h,i,:] . k[b,g,t,:]) . v[b,g,t,:]
//   g = h / (Hq / Hkv);  t <= i if causal, else t < L
//
// Self-attention (Lq = Lk = L), grouped-query, head dim 128. The numerics are
// those of decode: q, k and v are bf16 (rounded on the host, round-to-nearest-
// even), both products run on the bf16 MFMA with fp32 accumulation, scores and
// softmax are fp32 in base 2 with scale * log2(e) folded in, P is rounded to
// bf16 (RNE) for PV while the normaliser l is summed from the unrounded
// weights, the only division is a true `/` at the end, and the output is fp32.
//
//   workgroup    one per (sequence, query head, block of kPrefillRows = 128
//                query rows), 4 wave64s of 32 rows each. There is no cap on
//                the group size Hq / Hkv: the heads of a kv head are separate
//                workgroups that meet in the L2.
//   grid         one-dimensional, the row block slowest and descending: the
//                heaviest causal blocks (largest i) start first, so the tail
//                of the grid is short work. With B Hq a multiple of 8 the
//                (b, h) index is dealt so that an XCD (block id mod 8) gets
//                consecutive heads, that is whole kv groups, in its L2.
//   Q            each lane keeps its row's B fragments in 32 VGPRs for the
//                whole block.
//   K / V        tiles of kPrefillKeys = 64 keys, double-buffered in LDS (2 x
//                (16 + 16) KiB) and shared by the four waves. The global loads
//                of tile j + 1 are issued before the products of tile j and
//                written to LDS after them; one barrier per tile.
//   QK           the swapped product S^T = K Q^T on v_mfma_f32_32x32x16_bf16: A
//                = 32 keys x 16 d of K from LDS, B = 16 d x 32 rows of Q^T,
//                two key halves x eight d-steps. The result has the query row
//                on the lane (l & 31) and 32 of the tile's 64 keys in its
//                registers; lane l ^ 32 holds the other 32. A row maximum is
//                lane-local plus one exchange.
//   PV           O^T = V^T P^T: the score registers 8 s .. 8 s + 7 of a key
//                half, rounded to bf16, are the B fragment of k-step s as they
//                stand (element j of lane half h is key 16 s + 8 (j >> 2) + 4 h
//                + (j & 3) of the half). P never leaves the registers; the V
//                image stores its keys in exactly that order (prefill_v_pos),
//                so the A fragment is one plain 16-byte LDS read. Four d-tiles
//                of 32: 64 accumulator VGPRs with the row on the lane, so the
//                rescale by exp2(m_old - m_new) is lane-local.
//   images       the host owns the global layout. K and V are stored tile by
//                tile as the LDS images themselves, so staging is a linear,
//                fully coalesced 16-byte copy. K tile: [64 keys][128 d], the
//                16-byte chunk c of key row k at chunk c ^ (k & 15): the 16
//                lanes of a ds_read_b128 group read 16 different key rows at
//                one d and land on 16 different slots. V tile, transposed:
//                [128 d][64 key positions], chunk c of row d at c ^ ((d >> 1) &
//                7): the 16 rows of a group are 128 bytes apart and cover the
//                16 slots of 2 x 8. Both reads are bank-conflict-free by the
//                256-byte rule for ds_read_b128.
//   mask         tiles wholly above a block's diagonal are never loaded; a
//                wave skips the tiles wholly above its own 32 rows; only tiles
//                that cross the wave's diagonal, or hold padded keys, take the
//                per-element path, which sets the score to -inf by key index
//                with a select. The running maximum is updated at every tile
//                (no deferred-rescale threshold); a running maximum of -inf is
//                replaced by 0 in the exponent.
//
// The host zero-pads K and V to whole tiles and Q and the device output to
// whole row blocks, so the kernel forms no address outside its buffers for any
// accepted shape; padded rows are computed and dropped on download.
//
// Resources of attn_prefill_kernel, from the compiler's report for gfx950
// (-Rpass-analysis=kernel-resource-usage): 244 VGPRs, 0 AGPRs, 34 SGPRs, no
// scratch, 65536 bytes of LDS per workgroup, occupancy 2 waves per SIMD: two
// workgroups per CU, 128 of the 160 KiB of LDS. Per tile and wave: 32 MFMAs,
// 32 ds_read_b128, 32 v_exp_f32 (one more for the rescale), 16
// v_cvt_pk_bf16_f32, one ds_bpermute_b32. Measured: profiles/prefill_probe.md.
//
// Included by payload_core.hpp after payload_attn.hpp (needs kAttnD, its
// pattern functions, AttnCheck, kAttnRelBound, detail::AttnShape, attn_group,
// attn_default_scale, attn_c2, attn_spread_row and attn_ref_row, and everything
// that header needs).

#pragma once

#include <algorithm>
#include <cmath>

namespace payload {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kPrefillRows = 128;     // query rows per workgroup
constexpr int kPrefillKeys = 64;      // keys per LDS tile
constexpr int kPrefillWaveRows = 32;  // query rows per wave
constexpr int kPrefillTileElems = kPrefillKeys * kAttnD;  // per tensor and tile
constexpr int kPrefillMaxLen = 1 << 24;

static_assert(kAttnD == 128, "the tile images are laid out for head dim 128");
static_assert(kPrefillRows == (kBlock / 64) * kPrefillWaveRows, "one 32-row strip per wave");
static_assert(kPrefillTileElems * 2 % (kBlock * 16) == 0, "whole 16-byte pieces per thread");

// ---- tile images -------------------------------------------------------------

// element offset of (key w of the tile, d) inside the tile's K image
__host__ __device__ inline int prefill_k_off(int w, int d) {
  return w * kAttnD + ((((d >> 3) ^ (w & 15))) << 3) + (d & 7);
}

// position of key w of the tile inside a V^T row: bits 2 and 3 trade places, so
// that the 8 elements at positions 32 kt + 16 s + 8 h .. + 7 are the keys that
// element j = 0 .. 7 of lane half h holds in score registers 8 s .. 8 s + 7
__host__ __device__ inline int prefill_v_pos(int w) {
  return (w & ~12) | ((w & 4) << 1) | ((w & 8) >> 1);
}

// the same for the V image
__host__ __device__ inline int prefill_v_off(int w, int d) {
  const int pos = prefill_v_pos(w);
  return d * kPrefillKeys + ((((pos >> 3) ^ ((d >> 1) & 7))) << 3) + (pos & 7);
}

// ---- patterns ------------------------------------------------------------------
//
// Selection pattern: small integers, exact in bf16. Key t of (b, g) is selected
// iff t == 0 or (t + b + 2 g) % 5 == 0; K is 0 there and <= -16 elsewhere, q is
// in 2 .. 5, so a selected score is exactly 0 and any other is <= -16 * 2 * 128
// = -4096 (times scale), whose weight is exactly 0 in fp32 whatever the
// running maximum was. o = (sum of v over the visible selected keys) / (their
// count): an exact integer over an exact integer, rounded once by the division,
// bit-exact in any tile order. Key 0 is always selected, so every causal row
// sees one.
//
// Dense pattern: an integer hash of the 64-bit element index, multiples of
// 2^-6: q in [-4, 4], k and v in [-1, 1], all exact in bf16.

__host__ __device__ inline bool prefill_selected(int b, int g, int t) {
  return t == 0 || (static_cast<long long>(t) + b + 2ll * g) % 5 == 0;
}

__host__ __device__ inline int prefill_pat_q(int b, int h, int i, int d) {
  return 2 + static_cast<int>((3ll * b + 5ll * h + 7ll * d + i) % 4);
}

__host__ __device__ inline uint32_t prefill_hash(uint32_t tensor, unsigned long long idx) {
  uint32_t x = static_cast<uint32_t>(idx) ^
               (static_cast<uint32_t>(idx >> 32) * 0x85ebca6bu);
  x = x * 3u + tensor + 0x9e3779b9u;
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

enum PrefillPattern { kPrefillDense = 0, kPrefillSelection = 1 };

// element (b, head, t, d) of tensor 1 (q, `heads` = Hq), 2 (k) or 3 (v, both
// `heads` = Hkv) of a pattern; t is the row for q and the key for k and v
__host__ __device__ inline float prefill_elem(int pat, int tensor, int heads, int L,
                                              int b, int head, int t, int d) {
  if (pat == kPrefillDense) {
    const unsigned long long idx =
        ((static_cast<unsigned long long>(b) * heads + head) * L + t) * kAttnD + d;
    const int range = tensor == 1 ? 256 : 64;
    const uint32_t h = prefill_hash(static_cast<uint32_t>(tensor), idx);
    return static_cast<float>(static_cast<int>(h % (2u * range + 1u)) - range) / 64.0f;
  }
  if (tensor == 1) return static_cast<float>(prefill_pat_q(b, head, t, d));
  if (tensor == 2)
    return prefill_selected(b, head, t)
               ? 0.f : static_cast<float>(attn_pat_k_off(head, t, d));
  return static_cast<float>(attn_pat_v(b, head, t, d));
}

// ---- kernels -------------------------------------------------------------

typedef unsigned prefill_u32x4 __attribute__((ext_vector_type(4)));
typedef float prefill_f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 prefill_bf16x2 __attribute__((ext_vector_type(2)));

// two fp32 -> two bf16 in one word (lo in bits 15:0), round-to-nearest-even:
// the conversion compiles to one v_cvt_pk_bf16_f32, where rounding by hand
// costs five instructions per pair
__device__ __forceinline__ unsigned prefill_pack_bf16(float lo, float hi) {
  const prefill_f32x2 f = {lo, hi};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(f, prefill_bf16x2));
}

// q: [B Hq][Lqp][128] bf16, rows L .. Lqp - 1 zero (Lqp a multiple of 128). k,
// vt: [B Hkv][ntiles] tile images of 8192 bf16 (prefill_k_off, prefill_v_off),
// keys L .. 64 ntiles - 1 zero. o: [B Hq][Lqp][128] fp32. nbh = B Hq, c2 = scale
// * log2(e). grid = nbh * Lqp / 128, block = 256; the second launch bound asks
// for two waves per SIMD, that is at most 256 registers.
__global__ __launch_bounds__(kBlock, 2) void attn_prefill_kernel(
    const uint16_t* __restrict__ q, const uint16_t* __restrict__ k,
    const uint16_t* __restrict__ vt, float* __restrict__ o, int Hq, int G, int L,
    int Lqp, int ntiles, int nbh, int causal, float c2) {
  __shared__ __attribute__((aligned(16))) uint16_t lds[2][2][kPrefillTileElems];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;

  // heaviest row blocks first; an XCD (block id mod 8) takes consecutive heads
  const int bid = static_cast<int>(blockIdx.x);
  int bh = bid % nbh;
  if ((nbh & 7) == 0) bh = (bh & 7) * (nbh >> 3) + (bh >> 3);
  const int rb = Lqp / kPrefillRows - 1 - bid / nbh;
  const int b = bh / Hq, g = (bh % Hq) / G;
  const size_t bg = static_cast<size_t>(b) * (Hq / G) + g;

  const int r0 = rb * kPrefillRows;
  const int q0 = r0 + wave * kPrefillWaveRows;  // the wave's first row
  const int row = q0 + r;                       // this lane's row
  // tiles the block needs: under the mask, those that start at or below its
  // last row
  const int nt = causal ? min(ntiles, (r0 + kPrefillRows - 1) / kPrefillKeys + 1)
                        : ntiles;

  // B fragments of Q^T: lane l holds q[row l & 31][d = 16 s + 8 (l >> 5) + j]
  bf16x8 fq[kAttnD / 16];
  {
    const uint16_t* qb = q + (static_cast<size_t>(bh) * Lqp + row) * kAttnD + h * 8;
#pragma unroll
    for (int s = 0; s < kAttnD / 16; ++s)
      fq[s] = *reinterpret_cast<const bf16x8*>(qb + s * 16);
  }

  // staging: the tile images are copied as they stand, thread t takes the 16-
  // byte pieces t, t + 256, t + 512 and t + 768 of each
  constexpr int kPieces = kPrefillTileElems / 8 / kBlock;  // 4
  const uint16_t* kg = k + bg * ntiles * kPrefillTileElems + tid * 8;
  const uint16_t* vg = vt + bg * ntiles * kPrefillTileElems + tid * 8;
  bf16x8 sk[kPieces], sv[kPieces];
  auto stage_load = [&](int tile) {
    const size_t off = static_cast<size_t>(tile) * kPrefillTileElems;
#pragma unroll
    for (int i = 0; i < kPieces; ++i) {
      sk[i] = *reinterpret_cast<const bf16x8*>(kg + off + i * kBlock * 8);
      sv[i] = *reinterpret_cast<const bf16x8*>(vg + off + i * kBlock * 8);
    }
  };
  auto stage_write = [&](int buf) {
#pragma unroll
    for (int i = 0; i < kPieces; ++i) {
      *reinterpret_cast<bf16x8*>(&lds[buf][0][(i * kBlock + tid) * 8]) = sk[i];
      *reinterpret_cast<bf16x8*>(&lds[buf][1][(i * kBlock + tid) * 8]) = sv[i];
    }
  };

  float m = -INFINITY, l = 0.f;  // l: this lane's 32 keys per tile only
  f32x16 acc[kAttnD / 32];
#pragma unroll
  for (int dt = 0; dt < kAttnD / 32; ++dt)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[dt][i] = 0.f;

  // LDS element offsets of this lane's fragments. K: key row 32 kt + r, chunk 2
  // s + h at (2 s + h) ^ (r & 15). V^T: row 32 dt + r, chunk 4 kt + 2 s + h at
  // (4 kt + 2 s + h) ^ ((r >> 1) & 7), since 32 dt does not reach bits 1 .. 3.
  const int krow = r * kAttnD, kx = r & 15;
  const int vrow = r * kPrefillKeys, vx = (r >> 1) & 7;

  stage_load(0);
  stage_write(0);
  __syncthreads();

  for (int j = 0; j < nt; ++j) {
    const int cur = j & 1;
    const int t0 = j * kPrefillKeys;
    if (j + 1 < nt) stage_load(j + 1);  // in flight under the products below

    if (!causal || t0 <= q0 + kPrefillWaveRows - 1) {  // wave-uniform
      const uint16_t* kl = lds[cur][0];
      const uint16_t* vl = lds[cur][1];

      f32x16 st[2];
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int i = 0; i < 16; ++i) st[kt][i] = 0.f;
#pragma unroll
      for (int s = 0; s < kAttnD / 16; ++s) {
        const int c = ((2 * s + h) ^ kx) << 3;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
          const bf16x8 a =
              *reinterpret_cast<const bf16x8*>(kl + kt * 32 * kAttnD + krow + c);
          st[kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, fq[s], st[kt], 0, 0, 0);
        }
      }

      // register i of half kt: key t0 + 32 kt + 8 (i >> 2) + 4 h + (i & 3).
      // The score is x * xs in base 2. A full tile keeps the raw products (xs
      // = c2) and scales in the exponent's fma: its row maximum is the
      // extreme raw product of c2's sign, times c2. A tile that crosses the
      // wave's diagonal or holds padded keys scales first (xs = 1) and sets
      // the masked scores to -inf by key index.
      float x[32];
      float cm;
      const bool ragged = causal ? t0 + kPrefillKeys - 1 > q0
                                 : t0 + kPrefillKeys - 1 >= L;  // wave-uniform
      if (ragged) {
        const int last = causal ? row : L - 1;  // last visible key of this row
#pragma unroll
        for (int i = 0; i < 32; ++i) {
          const int key = t0 + 32 * (i >> 4) + 8 * ((i & 15) >> 2) + 4 * h + (i & 3);
          x[i] = key <= last ? st[i >> 4][i & 15] * c2 : -INFINITY;
        }
        cm = x[0];
#pragma unroll
        for (int i = 1; i < 32; ++i) cm = fmaxf(cm, x[i]);
      } else {
#pragma unroll
        for (int i = 0; i < 32; ++i) x[i] = st[i >> 4][i & 15];
        cm = x[0];
        if (c2 >= 0.f) {
#pragma unroll
          for (int i = 1; i < 32; ++i) cm = fmaxf(cm, x[i]);
        } else {
#pragma unroll
          for (int i = 1; i < 32; ++i) cm = fminf(cm, x[i]);
        }
        cm *= c2;
      }
      const float xs = ragged ? 1.f : c2;
      cm = fmaxf(cm, __shfl_xor(cm, 32));

      const float mn = fmaxf(m, cm);
      const float ms = mn == -INFINITY ? 0.f : mn;  // never (-inf) - (-inf)
      const float alpha = __builtin_amdgcn_exp2f(m - ms);  // m = -inf: 0
      m = mn;

      bf16x8 fp[4];  // k-step 2 kt + s
      float sum = 0.f;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        prefill_u32x4 packed;
#pragma unroll
        for (int j = 0; j < 8; j += 2) {
          const float p0 = __builtin_amdgcn_exp2f(fmaf(x[8 * ks + j], xs, -ms));
          const float p1 = __builtin_amdgcn_exp2f(fmaf(x[8 * ks + j + 1], xs, -ms));
          sum += p0 + p1;  // l takes the unrounded weights
          packed[j >> 1] = prefill_pack_bf16(p0, p1);
        }
        fp[ks] = __builtin_bit_cast(bf16x8, packed);
      }
      l = l * alpha + sum;

#pragma unroll
      for (int dt = 0; dt < kAttnD / 32; ++dt) {
        acc[dt] *= alpha;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          const int c = ((2 * ks + h) ^ vx) << 3;
          const bf16x8 a = *reinterpret_cast<const bf16x8*>(
              vl + dt * 32 * kPrefillKeys + vrow + c);
          acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, fp[ks], acc[dt], 0, 0, 0);
        }
      }
    }

    if (j + 1 < nt) stage_write(cur ^ 1);  // free since the last barrier
    __syncthreads();
  }

  // the row's l is spread over its two lanes; alpha was common to them
  l += __shfl_xor(l, 32);

  // C/D map: col (row of q) = lane & 31, row (d) = 32 dt + 8 (i >> 2) + 4 h + (i
  // & 3): registers 4 n .. 4 n + 3 are four consecutive d
  float* ob = o + (static_cast<size_t>(bh) * Lqp + row) * kAttnD + 4 * h;
#pragma unroll
  for (int dt = 0; dt < kAttnD / 32; ++dt)
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      f32x4 out;
#pragma unroll
      for (int e = 0; e < 4; ++e) out[e] = acc[dt][4 * n + e] / l;  // a true division
      *reinterpret_cast<f32x4*>(ob + dt * 32 + n * 8) = out;
    }
}

// Device-side fill of a pattern into the q image, one 16-byte piece per thread
// and step. Every pattern value is exact in bf16, so the top 16 bits of the
// float are the value. pieces = B Hq Lqp 128 / 8.
__global__ __launch_bounds__(kBlock) void prefill_fill_q_kernel(
    uint16_t* __restrict__ q, int Hq, int L, int Lqp, int pat, size_t pieces) {
  size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x;
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (; i < pieces; i += stride) {
    const int d0 = static_cast<int>(i & 15) * 8;
    const size_t rowi = i >> 4;
    const int t = static_cast<int>(rowi % Lqp);
    const size_t bh = rowi / Lqp;
    const int b = static_cast<int>(bh / Hq), hd = static_cast<int>(bh % Hq);
    bf16x8 val;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float f = t < L ? prefill_elem(pat, 1, Hq, L, b, hd, t, d0 + j) : 0.f;
      val[j] = static_cast<short>(__float_as_uint(f) >> 16);
    }
    *reinterpret_cast<bf16x8*>(q + i * 8) = val;
  }
}

// The same for the K and V tile images. pieces = B Hkv ntiles 8192 / 8 per tensor.
__global__ __launch_bounds__(kBlock) void prefill_fill_kv_kernel(
    uint16_t* __restrict__ k, uint16_t* __restrict__ vt, int Hkv, int L, int ntiles,
    int pat, size_t pieces) {
  size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x;
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (; i < pieces; i += stride) {
    const size_t image = i >> 10;  // 1024 pieces per tile image
    const int piece = static_cast<int>(i & 1023);
    const int t0 = static_cast<int>(image % ntiles) * kPrefillKeys;
    const size_t bg = image / ntiles;
    const int b = static_cast<int>(bg / Hkv), g = static_cast<int>(bg % Hkv);
    bf16x8 kv, vv;
    {  // K: key row piece >> 4, stored chunk piece & 15 holds chunk ^ (key & 15)
      const int w = piece >> 4, t = t0 + w;
      const int d0 = ((piece & 15) ^ (w & 15)) * 8;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float f = t < L ? prefill_elem(pat, 2, Hkv, L, b, g, t, d0 + j) : 0.f;
        kv[j] = static_cast<short>(__float_as_uint(f) >> 16);
      }
    }
    {  // V^T: row d = piece >> 3, stored chunk piece & 7 holds chunk ^ ((d >> 1) & 7)
      const int d = piece >> 3;
      const int p0 = ((piece & 7) ^ ((d >> 1) & 7)) * 8;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int t = t0 + prefill_v_pos(p0 + j);  // the swap is its own inverse
        const float f = t < L ? prefill_elem(pat, 3, Hkv, L, b, g, t, d) : 0.f;
        vv[j] = static_cast<short>(__float_as_uint(f) >> 16);
      }
    }
    *reinterpret_cast<bf16x8*>(k + i * 8) = kv;
    *reinterpret_cast<bf16x8*>(vt + i * 8) = vv;
  }
}

// ---- host layer ----------------------------------------------------------

struct PrefillResult {
  double tflops = 0;     // unmasked (q, k) pairs only
  double tok_per_s = 0;  // B L per launch
  double max_rel = 0;    // 16 spread rows against fp64
};

// The limits of the prefill payload, or std::invalid_argument; no HIP call.
// There is no cap on Hq / Hkv, which it returns: every axis fits the kernel's
// int arithmetic and the one-dimensional grid.
inline int attn_prefill_shape(long long B, long long Hq, long long Hkv, long long L) {
  const long long G = detail::attn_group("prefill", B, Hq, Hkv, L);
  if (B > 65535 || Hq > 65535 || L > kPrefillMaxLen ||
      B * Hq * ((L + kPrefillRows - 1) / kPrefillRows) > 0x7FFFFFFFll)
    throw std::invalid_argument("prefill: shape too large");
  return static_cast<int>(G);
}

namespace detail {

// Shape, device buffers and launch of one prefill problem.
struct PrefillProblem : AttnShape {
  bool causal;
  size_t Lqp, Lkp;
  DeviceBuffer dq, dk, dvt, dout;

  PrefillProblem(int b, int hq, int hkv, int len, bool is_causal, int dev)
      : AttnShape{b, hq, hkv, len, attn_prefill_shape(b, hq, hkv, len), dev},
        causal(is_causal), Lqp(round_up(len, kPrefillRows)),
        Lkp(round_up(len, kPrefillKeys)) {}

  size_t heads() const { return static_cast<size_t>(B) * Hq; }
  size_t q_elems() const { return heads() * Lqp * kAttnD; }
  size_t kv_elems() const { return static_cast<size_t>(B) * Hkv * Lkp * kAttnD; }
  int ntiles() const { return static_cast<int>(Lkp / kPrefillKeys); }

  void alloc() {
    HIP_CHECK(hipSetDevice(device));
    dq.alloc(q_elems() * sizeof(uint16_t));
    dk.alloc(kv_elems() * sizeof(uint16_t));
    dvt.alloc(kv_elems() * sizeof(uint16_t));
    dout.alloc(q_elems() * sizeof(float));
  }

  // q (B, Hq, L, 128), k and v (B, Hkv, L, 128) float -> the bf16 images
  void upload(const float* q, const float* k, const float* v) {
    std::vector<uint16_t> hq(q_elems(), 0), hk(kv_elems(), 0), hvt(kv_elems(), 0);
    for (size_t bh = 0; bh < heads(); ++bh)
      for (int i = 0; i < L; ++i) {
        const float* src = q + (bh * L + i) * kAttnD;
        uint16_t* dst = hq.data() + (bh * Lqp + i) * kAttnD;
        for (int d = 0; d < kAttnD; ++d) dst[d] = to_bf16_rne(src[d]);
      }
    const size_t nt = Lkp / kPrefillKeys;
    for (size_t bg = 0; bg < static_cast<size_t>(B) * Hkv; ++bg)
      for (int t = 0; t < L; ++t) {
        const size_t image = (bg * nt + t / kPrefillKeys) * kPrefillTileElems;
        const int w = t % kPrefillKeys;
        const float* ks = k + (bg * L + t) * kAttnD;
        const float* vs = v + (bg * L + t) * kAttnD;
        for (int d = 0; d < kAttnD; ++d) {
          hk[image + prefill_k_off(w, d)] = to_bf16_rne(ks[d]);
          hvt[image + prefill_v_off(w, d)] = to_bf16_rne(vs[d]);
        }
      }
    HIP_CHECK(hipMemcpy(dq.p, hq.data(), hq.size() * sizeof(uint16_t),
                        hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dk.p, hk.data(), hk.size() * sizeof(uint16_t),
                        hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dvt.p, hvt.data(), hvt.size() * sizeof(uint16_t),
                        hipMemcpyHostToDevice));
  }

  // the images of a pattern, filled on the device
  void fill(int pat) {
    const size_t qp = q_elems() / 8, kp = kv_elems() / 8;
    hipLaunchKernelGGL(prefill_fill_q_kernel, dim3(grid_for(qp)), dim3(kBlock), 0, 0,
                       dq.as<uint16_t>(), Hq, L, static_cast<int>(Lqp), pat, qp);
    hipLaunchKernelGGL(prefill_fill_kv_kernel, dim3(grid_for(kp)), dim3(kBlock), 0, 0,
                       dk.as<uint16_t>(), dvt.as<uint16_t>(), Hkv, L, ntiles(), pat, kp);
    HIP_CHECK(hipGetLastError());
  }

  void launch(float scale) const {
    const float c2 = attn_c2(scale);
    const unsigned grid = static_cast<unsigned>(heads() * (Lqp / kPrefillRows));
    hipLaunchKernelGGL(attn_prefill_kernel, dim3(grid), dim3(kBlock), 0, 0,
                       dq.as<const uint16_t>(), dk.as<const uint16_t>(),
                       dvt.as<const uint16_t>(), dout.as<float>(), Hq, G, L,
                       static_cast<int>(Lqp), ntiles(), static_cast<int>(heads()),
                       causal ? 1 : 0, c2);
  }

  // rows 0 .. L - 1 of every head
  void download(float* o) const {
    if (Lqp == static_cast<size_t>(L)) {
      HIP_CHECK(hipMemcpy(o, dout.p, q_elems() * sizeof(float), hipMemcpyDeviceToHost));
      return;
    }
    for (size_t bh = 0; bh < heads(); ++bh)
      HIP_CHECK(hipMemcpy(o + bh * L * kAttnD, dout.as<float>() + bh * Lqp * kAttnD,
                          static_cast<size_t>(L) * kAttnD * sizeof(float),
                          hipMemcpyDeviceToHost));
  }
};

}  // namespace detail

// General entry. q (B, Hq, L, 128), k and v (B, Hkv, L, 128), o (B, Hq, L,
// 128), all row-major float. std::invalid_argument on any unsupported shape,
// before any device work.
inline void attn_prefill(const float* q, const float* k, const float* v, float* o,
                         int B, int Hq, int Hkv, int L, bool causal, float scale,
                         int device = 0) {
  detail::PrefillProblem p(B, Hq, Hkv, L, causal, device);
  p.alloc();
  p.upload(q, k, v);
  p.launch(scale);
  HIP_CHECK(hipGetLastError());
  p.download(o);
}

// Host only: q (B, Hq, L, 128), k, v (B, Hkv, L, 128) and the expected output
// (B, Hq, L, 128) of the selection pattern: the sum of v over the selected keys
// a row sees, divided by their count.
inline void prefill_check_pattern(float* q, float* k, float* v, float* expected,
                                  int B, int Hq, int Hkv, int L, bool causal) {
  const int G = attn_prefill_shape(B, Hq, Hkv, L);
  for (int b = 0; b < B; ++b) {
    for (int h = 0; h < Hq; ++h)
      for (int i = 0; i < L; ++i) {
        float* qr = q + ((static_cast<size_t>(b) * Hq + h) * L + i) * kAttnD;
        for (int d = 0; d < kAttnD; ++d)
          qr[d] = prefill_elem(kPrefillSelection, 1, Hq, L, b, h, i, d);
      }
    for (int g = 0; g < Hkv; ++g) {
      const size_t bg = static_cast<size_t>(b) * Hkv + g;
      float* kh = k + bg * L * kAttnD;
      float* vh = v + bg * L * kAttnD;
      for (int t = 0; t < L; ++t)
        for (int d = 0; d < kAttnD; ++d) {
          kh[static_cast<size_t>(t) * kAttnD + d] =
              prefill_elem(kPrefillSelection, 2, Hkv, L, b, g, t, d);
          vh[static_cast<size_t>(t) * kAttnD + d] =
              prefill_elem(kPrefillSelection, 3, Hkv, L, b, g, t, d);
        }
      // sum and count of v over the selected keys row t sees: the keys 0 .. t
      // under the mask (a running sum), all of them without
      int sum[kAttnD] = {0}, count = 0;
      auto take = [&](int t) {
        if (!prefill_selected(b, g, t)) return;
        ++count;
        for (int d = 0; d < kAttnD; ++d)
          sum[d] += static_cast<int>(vh[static_cast<size_t>(t) * kAttnD + d]);
      };
      if (!causal)
        for (int t = 0; t < L; ++t) take(t);
      for (int t = 0; t < L; ++t) {
        if (causal) take(t);
        for (int hh = 0; hh < G; ++hh) {
          float* er = expected +
              ((static_cast<size_t>(b) * Hq + g * G + hh) * L + t) * kAttnD;
          for (int d = 0; d < kAttnD; ++d)
            er[d] = static_cast<float>(sum[d]) / static_cast<float>(count);
        }
      }
    }
  }
}

// Self-check at one shape. (a) the selection pattern against its closed form:
// max_err, expect exactly 0. (b) the dense pattern against an fp64 reference:
// max_rel = max |o - ref| / max |v|, expect <= 2^-8 by decode's derivation
// (run_attn_check): the numerics are the same.
inline AttnCheck run_prefill_check(int B, int Hq, int Hkv, int L, bool causal = true,
                                   int device = 0) {
  const int G = attn_prefill_shape(B, Hq, Hkv, L);  // validate first
  const size_t nq = static_cast<size_t>(B) * Hq * L * kAttnD;
  const size_t nkv = static_cast<size_t>(B) * Hkv * L * kAttnD;
  const float scale = detail::attn_default_scale();
  std::vector<float> q(nq), k(nkv), v(nkv), want(nq), got(nq);
  AttnCheck r;

  prefill_check_pattern(q.data(), k.data(), v.data(), want.data(), B, Hq, Hkv, L, causal);
  attn_prefill(q.data(), k.data(), v.data(), got.data(), B, Hq, Hkv, L, causal, scale,
               device);
  for (size_t i = 0; i < nq; ++i)
    detail::note_err(r.max_err, std::fabs(static_cast<double>(got[i]) -
                                          static_cast<double>(want[i])));

  double vmax = 0;
  for (int b = 0; b < B; ++b) {
    for (int h = 0; h < Hq; ++h)
      for (int i = 0; i < L; ++i)
        for (int d = 0; d < kAttnD; ++d)
          q[((static_cast<size_t>(b) * Hq + h) * L + i) * kAttnD + d] =
              prefill_elem(kPrefillDense, 1, Hq, L, b, h, i, d);
    for (int g = 0; g < Hkv; ++g)
      for (int t = 0; t < L; ++t)
        for (int d = 0; d < kAttnD; ++d) {
          const size_t at = ((static_cast<size_t>(b) * Hkv + g) * L + t) * kAttnD + d;
          k[at] = prefill_elem(kPrefillDense, 2, Hkv, L, b, g, t, d);
          v[at] = prefill_elem(kPrefillDense, 3, Hkv, L, b, g, t, d);
          vmax = std::max(vmax, std::fabs(static_cast<double>(v[at])));
        }
  }
  attn_prefill(q.data(), k.data(), v.data(), got.data(), B, Hq, Hkv, L, causal, scale,
               device);
  std::vector<double> w(L), ref(kAttnD);
  double max_abs = 0;
  for (int b = 0; b < B; ++b)
    for (int h = 0; h < Hq; ++h) {
      const size_t bg = static_cast<size_t>(b) * Hkv + h / G;
      for (int i = 0; i < L; ++i) {
        const size_t at = ((static_cast<size_t>(b) * Hq + h) * L + i) * kAttnD;
        detail::attn_ref_row(ref.data(), q.data() + at, k.data() + bg * L * kAttnD,
                             v.data() + bg * L * kAttnD, causal ? i + 1 : L,
                             static_cast<double>(scale), w);
        for (int d = 0; d < kAttnD; ++d)
          detail::note_err(max_abs, std::fabs(static_cast<double>(got[at + d]) - ref[d]));
      }
    }
  r.max_rel = vmax > 0 ? max_abs / vmax : max_abs;
  return r;
}

// Timed run. q, k and v are filled on the device with the dense hash pattern:
// the probe is bound by the matrix cores, which hold a higher clock on zeros
// and low-entropy data than on random data, so a rate measured on the
// selection pattern would flatter the partition (`pattern` = kPrefillSelection
// measures exactly that gap and is not the default). One warm-up launch,
// `iters` launches between events, then 16 spread (b, h, i) rows are recomputed
// on the host in fp64 from the same pattern, so a fast wrong kernel cannot
// report a rate. FLOPs count the unmasked pairs only: 4 * 128 * B Hq L (L + 1)
// / 2 per launch under the mask, 4 * 128 * B Hq L^2 without.
inline PrefillResult run_prefill(int B = 8, int Hq = 64, int Hkv = 8, int L = 4096,
                                 int iters = 10, bool causal = true, int device = 0,
                                 int pattern = kPrefillDense) {
  if (iters < 1) throw std::invalid_argument("run_prefill: iters must be >= 1");
  if (pattern != kPrefillDense && pattern != kPrefillSelection)
    throw std::invalid_argument("run_prefill: pattern must be 0 (dense) or 1 (selection)");
  detail::PrefillProblem p(B, Hq, Hkv, L, causal, device);
  p.alloc();
  p.fill(pattern);
  const float scale = detail::attn_default_scale();
  const float ms = detail::time_launches(iters, [&p, scale] { p.launch(scale); });
  PrefillResult r;
  const double sec = ms * 1e-3;
  const double pairs = causal ? static_cast<double>(L) * (L + 1.0) / 2.0
                              : static_cast<double>(L) * L;
  r.tflops = 4.0 * kAttnD * B * Hq * pairs * iters / sec / 1e12;
  r.tok_per_s = static_cast<double>(B) * L * iters / sec;

  std::vector<float> got(kAttnD), qr(kAttnD);
  std::vector<float> kh(static_cast<size_t>(L) * kAttnD), vh(kh.size());
  std::vector<double> w(L), ref(kAttnD);
  double max_abs = 0, vmax = 0;
  for (int t = 0; t < 16; ++t) {
    const size_t bh = detail::attn_spread_row(t, p.heads());
    const int b = static_cast<int>(bh / Hq), h = static_cast<int>(bh % Hq), g = h / p.G;
    const int i = static_cast<int>(static_cast<long long>(t) * (L - 1) / 15);
    const int n = causal ? i + 1 : L;
    for (int d = 0; d < kAttnD; ++d) qr[d] = prefill_elem(pattern, 1, Hq, L, b, h, i, d);
    for (int u = 0; u < n; ++u)
      for (int d = 0; d < kAttnD; ++d) {
        const size_t at = static_cast<size_t>(u) * kAttnD + d;
        kh[at] = prefill_elem(pattern, 2, Hkv, L, b, g, u, d);
        vh[at] = prefill_elem(pattern, 3, Hkv, L, b, g, u, d);
        vmax = std::max(vmax, std::fabs(static_cast<double>(vh[at])));
      }
    detail::attn_ref_row(ref.data(), qr.data(), kh.data(), vh.data(), n,
                         static_cast<double>(scale), w);
    HIP_CHECK(hipMemcpy(got.data(), p.dout.as<float>() + (bh * p.Lqp + i) * kAttnD,
                        kAttnD * sizeof(float), hipMemcpyDeviceToHost));
    for (int d = 0; d < kAttnD; ++d)
      detail::note_err(max_abs, std::fabs(static_cast<double>(got[d]) - ref[d]));
  }
  r.max_rel = vmax > 0 ? max_abs / vmax : max_abs;
  return r;
}

}  // namespace payload
