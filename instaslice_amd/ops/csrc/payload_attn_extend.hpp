// gfx950 paged chunked-prefill ("extend") attention payload.
//
// attn, paged and paged8 prove decode: one query token per sequence over a KV
// cache. prefill proves a cold prompt: Lq = Lk on tile images of its own. A
// serving engine spends most of its attention time between the two: a run of n
// new tokens per sequence attends to the keys already in the paged cache and,
// causally, to each other (chunked prefill, a prompt that hits a prefix cache,
// a multi-token verify step). This payload is that step:
//
//   o[b,i,h,:] = softmax_t(scale * q[b,i,h,:] . K_b[g,t,:]) . V_b[g,t,:]
//   g = h / (Hq / Hkv);  t <= lens[b] - qlens[b] + i;  i = 0 .. qlens[b] - 1
//
// lens[b] counts all keys of sequence b in the cache, the new tokens' own keys
// included (the engine wrote them before the step); 1 <= qlens[b] <= lens[b],
// so every row sees key 0. Key t lives in physical page table[b][t / page], at
// key t % page of it: the pool, the table and the stale-key contract are the
// paged payload's (payload_attn_paged.hpp), the cache format is AttnCacheBf16.
// q is packed ragged, (Tq, Hq, 128) with Tq = sum_b qlens[b] and a sequence's
// tokens contiguous; the output has that shape, fp32. The numerics are those of
// the other attention payloads: bf16 operands, both products on
// v_mfma_f32_16x16x32_bf16 with fp32 accumulation, a base-2 fp32 softmax with
// scale * log2(e) folded in, the running maximum updated at every chunk with
// the -inf guards, P rounded to bf16 for PV while l sums the unrounded weights,
// one true division at the end.
//
//   columns      for (sequence b, kv head g) the MFMA columns are the pairs
//                (token i, head j of the group), flattened as c = i G + j, c <
//                qlens[b] G. Any G in 1 .. 16 works and a 16-column tile may
//                straddle tokens. A lane computes its column's position p =
//                lens[b] - qlens[b] + c / G once, before the key loop.
//   workgroup    one per (b, g, block of 128 columns), 4 wave64s, each wave
//                owning two 16-column tiles. All waves walk the same keys, so
//                every K and V fragment read from LDS feeds two MFMAs per wave
//                and eight per workgroup. Columns past the sequence's last
//                load a clamped q row (a select, not a branch) and are not
//                stored; a wave with no real column skips the products.
//   Q            a lane's B fragments, 4 x bf16x8 per tile, loaded once from a
//                bf16 image of q laid out [Hkv][Tq][G][128]: column c of (b, g)
//                is row cu[b] G + c of kv head g.
//   K / V        the pool's 32-key chunk images (attn_k_off / attn_v_off) are
//                MFMA operands as they stand. They are copied to LDS as they
//                stand: 8 KiB of K and 8 KiB of V per chunk, a linear, fully
//                coalesced 16-byte copy, every thread taking two pieces of
//                each. A step is kExtendStepChunks = 2 chunks (64 keys), LDS is
//                double-buffered: 64 KiB, two workgroups per CU. The next
//                step's global loads are issued before the current step's MFMAs
//                and written to LDS after them; one barrier per step. A
//                fragment read is one ds_read_b128 at lane * 16 + fragment *
//                1024 bytes: 64 lanes read one contiguous KiB, conflict-free
//                without a swizzle.
//   table        a chunk's page is resolved by a wave-uniform load of
//                table[b][ch >> shift], one step ahead of the global loads that
//                need it; all offsets are size_t. With page = 32 the two chunks
//                of a step come from different pages.
//   QK / PV      decode's swapped products and key order (S^T = K Q^T, O^T =
//                V^T P^T; payload_attn.hpp): the column is on the lane, P stays
//                in registers, the rescale is lane-local. The chunk step
//                (attn_extend_chunk) is written for two tiles per wave: each
//                fragment is read once and used twice.
//   mask         chunks wholly above the block's last position are never loaded
//                or counted; a wave skips the chunks wholly above its largest
//                position and takes the select-free path on chunks wholly at or
//                below its smallest one (both tests wave-uniform); only chunks
//                that cross a column's position set scores to -inf by key
//                index. Every position is below lens[b], so that mask covers
//                the stale keys of the last chunk too.
//   epilogue     a row's softmax finishes inside its workgroup: l is summed
//                over the lane quarters, each column does a true `/`, and
//                16-byte stores go to o[(cu[b] + i) Hq + g G + j]. No split-KV,
//                no combine kernel.
//   plan         qlens and lens change every step, so the item list is made on
//                the device in every launch: attn_extend_plan_kernel, one
//                workgroup, an LDS prefix scan over ceil(qlens[b] G / 128) and
//                over qlens[b], 256 sequences per stride with a carry. It
//                writes the items {b, first column}, the token offsets cu[b]
//                and the item count. The grid is (Hkv, ceil(Tq G / 128) + B),
//                the bound the host knows; workgroups at or beyond the count
//                leave at once and are the last of the grid.
//                attn_extend_plan() is the same arithmetic on the host and the
//                specification.
//
// The host checks every length, table entry and extent before any device work;
// the kernels trust lens, qlens and the table and form no address outside their
// buffers for any accepted argument.
//
// Resources of attn_extend_kernel, from the compiler's report for gfx950
// (-Rpass-analysis=kernel-resource-usage): 244 VGPRs, 0 AGPRs, 50 SGPRs, no
// scratch and no spills, 65536 bytes of LDS per workgroup, occupancy 2 waves
// per SIMD: two workgroups per CU, 128 of the 160 KiB of LDS. Per chunk and
// wave: 32 MFMAs, 16 ds_read_b128, 16 v_exp_f32 (two more for the rescales), 8
// v_cvt_pk_bf16_f32. The two scheduling barriers in the chunk step are what
// keeps it there: without them the compiler reads all eight K fragments ahead
// of the QK products, needs 254 registers and spills 8 of them, one a staged
// piece that then waits for its global load in front of the MFMAs. Measured on
// a whole MI355X (profiles/extend_probe.md): 660 TFLOP/s at the default shape
// (8 sequences of 4096 keys, 1024 of them new), 691 at N = L against 859 of the
// prefill probe; the 32-key step reaches 637 and 665.
//
// Out of scope: fp8 caches; split-KV (a handful of columns over a very long
// context keeps one workgroup per kv head busy and the rest of the machine
// idle: measured in profiles/extend_probe.md, not optimised); a heaviest-first
// item order (items run in order of (b, column), the light blocks of a sequence
// first).
//
// Included by payload_core.hpp after payload_attn_paged.hpp and
// payload_prefill.hpp: the paged payload's problem struct, check case, table
// and read checks, scrambled table and ragged rule; prefill's patterns and
// bf16 pack; decode's layout, reference row and bound.

#pragma once

#include <algorithm>
#include <cmath>

namespace payload {

constexpr int kExtendCols = 128;      // MFMA columns per workgroup
constexpr int kExtendWaveCols = 32;   // two 16-column tiles per wave
constexpr int kExtendStepChunks = 2;  // 32-key chunks per LDS step
constexpr int kExtendMaxLen = 1 << 24;

static_assert(kExtendCols == (kBlock / 64) * kExtendWaveCols, "two tiles per wave");
static_assert(kAttnChunkElems % (kBlock * 8) == 0, "whole 16-byte pieces per thread");

// ---- the plan --------------------------------------------------------------

struct AttnExtendPlan {
  std::vector<int> items;  // 2 per item: b, first column
  std::vector<int> cu;     // per sequence: its first token in the packed q
};

// column blocks of a sequence of n new tokens
__host__ __device__ inline int attn_extend_blocks(int n, int G) {
  return (n * G + kExtendCols - 1) / kExtendCols;
}

// The specification of attn_extend_plan_kernel. qlens[b] >= 1, G in 1 .. 16,
// sum_b qlens[b] G below 2^31.
inline AttnExtendPlan attn_extend_plan(const int* qlens, int B, int G) {
  if (B < 1 || G < 1 || G > kAttnMaxGroup)
    throw std::invalid_argument("attn_extend_plan: B >= 1 and G in 1 .. 16");
  long long cols = 0;
  for (int b = 0; b < B; ++b) {
    if (qlens[b] < 1) throw std::invalid_argument("attn_extend_plan: qlens must be >= 1");
    cols += static_cast<long long>(qlens[b]) * G;
  }
  if (cols > INT32_MAX) throw std::invalid_argument("attn_extend_plan: too many columns");
  AttnExtendPlan p;
  int tok = 0;
  for (int b = 0; b < B; ++b) {
    p.cu.push_back(tok);
    tok += qlens[b];
    for (int j = 0; j < attn_extend_blocks(qlens[b], G); ++j) {
      p.items.push_back(b);
      p.items.push_back(j * kExtendCols);
    }
  }
  return p;
}

// ---- kernels -------------------------------------------------------------

// One workgroup. qlens: [B]. items: ceil(Tq G / 128) + B entries. cu: [B].
// nitems: one int.
__global__ __launch_bounds__(kBlock) void attn_extend_plan_kernel(
    const int* __restrict__ qlens, int B, int G, int2* __restrict__ items,
    int* __restrict__ cu, int* __restrict__ nitems) {
  __shared__ int scan_n[kBlock], scan_q[kBlock];
  __shared__ int carry_n, carry_q;
  const int tid = threadIdx.x;
  if (tid == 0) carry_n = carry_q = 0;
  __syncthreads();

  for (int b0 = 0; b0 < B; b0 += kBlock) {  // block-uniform
    const int b = b0 + tid;
    const int qn = b < B ? qlens[b] : 0;
    const int n = attn_extend_blocks(qn, G);
    scan_n[tid] = n;
    scan_q[tid] = qn;
    __syncthreads();
    const int live = min(kBlock, B - b0);  // the rest of both scans is zero
    for (int d = 1; d < live; d <<= 1) {   // inclusive scans of the live entries
      const int vn = tid >= d ? scan_n[tid - d] : 0;
      const int vq = tid >= d ? scan_q[tid - d] : 0;
      __syncthreads();
      scan_n[tid] += vn;
      scan_q[tid] += vq;
      __syncthreads();
    }
    const int first = carry_n + scan_n[tid] - n;
    if (b < B) cu[b] = carry_q + scan_q[tid] - qn;
    for (int j = 0; j < n; ++j) items[first + j] = make_int2(b, j * kExtendCols);
    __syncthreads();  // every thread has read the carries
    if (tid == live - 1) {
      carry_n += scan_n[tid];
      carry_q += scan_q[tid];
    }
    __syncthreads();
  }
  if (tid == 0) *nitems = carry_n;
}

// The chunk at key k0 for a wave's two column tiles. kl and vl are this lane's
// first fragment of the chunk's K and V images in LDS; fragment i is 512
// elements further (K: fragment 4 t + s is QK tile t, d-step s; V: fragment dt
// is d-tile dt). Every fragment is read once and feeds both tiles. Register r
// of QK tile t is key k0 + 8 fq + 4 t + r (decode's key order), so a lane's
// weight j is key k0 + 8 fq + j and the eight of them, rounded to bf16, are the
// PV B fragment. kMasked: keys above the column's position pos[c] get -inf;
// without it the chunk is wholly visible to all of the wave's columns.
template <bool kMasked>
__device__ __forceinline__ void attn_extend_chunk(
    const uint16_t* kl, const uint16_t* vl, const bf16x8 (&fqt)[2][kAttnD / 32], int k0,
    int fq, const int (&pos)[2], float c2, float (&m)[2], float (&l)[2],
    f32x4 (&o)[2][kAttnD / 16]) {
  f32x4 st[2][2];  // [column tile][QK tile]
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int t = 0; t < 2; ++t) st[c][t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < 2; ++t) {
#pragma unroll
    for (int s = 0; s < kAttnD / 32; ++s) {
      const bf16x8 a = *reinterpret_cast<const bf16x8*>(kl + (t * 4 + s) * 512);
#pragma unroll
      for (int c = 0; c < 2; ++c)
        st[c][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, fqt[c][s], st[c][t], 0, 0, 0);
    }
    // at most one QK tile's four K fragments are in registers at a time
    __builtin_amdgcn_sched_barrier(0);
  }

  bf16x8 fp[2];
  float alpha[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    float sc[8];
    float cm = -INFINITY;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      sc[j] = st[c][j >> 2][j & 3] * c2;
      if (kMasked) sc[j] = k0 + 8 * fq + j <= pos[c] ? sc[j] : -INFINITY;
      cm = fmaxf(cm, sc[j]);
    }
    cm = fmaxf(cm, __shfl_xor(cm, 16));
    cm = fmaxf(cm, __shfl_xor(cm, 32));

    const float mn = fmaxf(m[c], cm);
    const float ms = mn == -INFINITY ? 0.f : mn;  // never (-inf) - (-inf)
    alpha[c] = __builtin_amdgcn_exp2f(m[c] - ms);  // m = -inf: 0
    m[c] = mn;

    prefill_u32x4 packed;
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < 8; j += 2) {
      const float p0 = __builtin_amdgcn_exp2f(sc[j] - ms);
      const float p1 = __builtin_amdgcn_exp2f(sc[j + 1] - ms);
      sum += p0 + p1;  // l takes the unrounded weights
      packed[j >> 1] = prefill_pack_bf16(p0, p1);
    }
    fp[c] = __builtin_bit_cast(bf16x8, packed);
    l[c] = l[c] * alpha[c] + sum;
  }

  // the V fragments are not read above this line: hoisted over the softmax they
  // would hold 32 registers that the kernel does not have
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int dt = 0; dt < kAttnD / 16; ++dt) {
    const bf16x8 a = *reinterpret_cast<const bf16x8*>(vl + dt * 512);
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      o[c][dt] *= alpha[c];
      o[c][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, fp[c], o[c][dt], 0, 0, 0);
    }
  }
}

// q: [Hkv][Tq][G][128] bf16. kp, vp: the pool's chunk images. table: [B][W].
// lens, qlens, cu: [B]. o: [Tq][Hq][128] fp32. shift = log2(page / 32). grid =
// (Hkv, ceil(Tq G / 128) + B): the kv head is the fast index, so the workgroups
// beyond the item count are the last to be dispatched. The second launch bound
// asks for two waves per SIMD, that is at most 256 registers.
__global__ __launch_bounds__(kBlock, 2) void attn_extend_kernel(
    const uint16_t* __restrict__ q, const uint16_t* __restrict__ kp,
    const uint16_t* __restrict__ vp, const int* __restrict__ table,
    const int* __restrict__ lens, const int* __restrict__ qlens,
    const int2* __restrict__ items, const int* __restrict__ nitems,
    const int* __restrict__ cu, float* __restrict__ o, int G, int W, int shift, int Tq,
    float c2) {
  // [buffer][chunk of the step][K, V]
  __shared__ __attribute__((aligned(16)))
  uint16_t lds[2][kExtendStepChunks][2][kAttnChunkElems];
  if (static_cast<int>(blockIdx.y) >= *nitems) return;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const int g = blockIdx.x, Hkv = gridDim.x;

  const int2 it = items[blockIdx.y];
  const int b = it.x, c0 = it.y;
  const int len = lens[b], qn = qlens[b];
  const int ncol = qn * G, base = len - qn;  // column c is at position base + c / G
  const int tok0 = cu[b];
  const int* trow = table + static_cast<size_t>(b) * W;
  const int cmask = (1 << shift) - 1;

  // the block's chunks: those that start at or below its last position
  const int nch = (base + min(c0 + kExtendCols - 1, ncol - 1) / G) / kAttnChunk + 1;
  const int nsteps = (nch + kExtendStepChunks - 1) / kExtendStepChunks;

  // the wave's columns w0 .. w0 + 31 and the positions of its first and last
  // real one (wave-uniform); a wave with no real column sees no chunk
  const int w0 = c0 + wave * kExtendWaveCols;
  const int pw_min = base + min(w0, ncol - 1) / G;
  const int pw_max = w0 < ncol ? base + min(w0 + kExtendWaveCols - 1, ncol - 1) / G : -1;

  // this lane's two columns, clamped to the sequence's last, their positions
  // and their B fragments of Q^T: q[column][d = 32 s + 8 fq + j]
  int col[2], pos[2];
  bf16x8 fqt[2][kAttnD / 32];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    col[c] = w0 + 16 * c + fr;
    const int cc = min(col[c], ncol - 1);
    pos[c] = base + cc / G;
    const size_t row = (static_cast<size_t>(g) * Tq + tok0) * G + cc;
    const uint16_t* qb = q + row * kAttnD + fq * 8;
#pragma unroll
    for (int s = 0; s < kAttnD / 32; ++s)
      fqt[c][s] = *reinterpret_cast<const bf16x8*>(qb + s * 32);
  }

  // staging: a chunk image is copied as it stands, thread t takes the 16-byte
  // pieces t and t + 256 of K and of V. pg: the pages of the step whose loads
  // come next, resolved a step before them.
  constexpr int kPieces = kAttnChunkElems / 8 / kBlock;  // 2
  bf16x8 sk[kExtendStepChunks][kPieces], sv[kExtendStepChunks][kPieces];
  int pg[kExtendStepChunks];
  auto resolve = [&](int step) {
#pragma unroll
    for (int c = 0; c < kExtendStepChunks; ++c) {
      const int ch = step * kExtendStepChunks + c;
      pg[c] = ch < nch ? trow[ch >> shift] : 0;  // block-uniform
    }
  };
  auto stage_load = [&](int step) {
#pragma unroll
    for (int c = 0; c < kExtendStepChunks; ++c) {
      const int ch = step * kExtendStepChunks + c;
      if (ch >= nch) continue;  // wholly above the block: never loaded
      const size_t image =
          ((static_cast<size_t>(pg[c]) * Hkv + g) << shift) + static_cast<size_t>(ch & cmask);
      const size_t off = image * kAttnChunkElems + static_cast<size_t>(tid) * 8;
#pragma unroll
      for (int i = 0; i < kPieces; ++i) {
        sk[c][i] = *reinterpret_cast<const bf16x8*>(kp + off + i * kBlock * 8);
        sv[c][i] = *reinterpret_cast<const bf16x8*>(vp + off + i * kBlock * 8);
      }
    }
  };
  auto stage_write = [&](int buf, int step) {
#pragma unroll
    for (int c = 0; c < kExtendStepChunks; ++c) {
      if (step * kExtendStepChunks + c >= nch) continue;
#pragma unroll
      for (int i = 0; i < kPieces; ++i) {
        *reinterpret_cast<bf16x8*>(&lds[buf][c][0][(i * kBlock + tid) * 8]) = sk[c][i];
        *reinterpret_cast<bf16x8*>(&lds[buf][c][1][(i * kBlock + tid) * 8]) = sv[c][i];
      }
    }
  };

  float m[2] = {-INFINITY, -INFINITY}, l[2] = {0.f, 0.f};  // l: this lane's keys only
  f32x4 acc[2][kAttnD / 16];
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int dt = 0; dt < kAttnD / 16; ++dt) acc[c][dt] = f32x4{0.f, 0.f, 0.f, 0.f};

  resolve(0);
  stage_load(0);
  if (nsteps > 1) resolve(1);
  stage_write(0, 0);
  __syncthreads();

  for (int j = 0; j < nsteps; ++j) {  // block-uniform
    const int cur = j & 1;
    if (j + 1 < nsteps) {
      stage_load(j + 1);  // in flight under the products below
      if (j + 2 < nsteps) resolve(j + 2);
    }

#pragma unroll
    for (int c = 0; c < kExtendStepChunks; ++c) {
      const int k0 = (j * kExtendStepChunks + c) * kAttnChunk;
      if (k0 > pw_max) continue;  // wholly above the wave (wave-uniform)
      const uint16_t* kl = &lds[cur][c][0][lane * 8];
      const uint16_t* vl = &lds[cur][c][1][lane * 8];
      if (k0 + kAttnChunk - 1 <= pw_min)
        attn_extend_chunk<false>(kl, vl, fqt, k0, fq, pos, c2, m, l, acc);
      else
        attn_extend_chunk<true>(kl, vl, fqt, k0, fq, pos, c2, m, l, acc);
    }

    if (j + 1 < nsteps) stage_write(cur ^ 1, j + 1);  // free since the last barrier
    __syncthreads();
  }

  // C/D map: col (column) = lane & 15, row (d) = 16 dt + 4 fq + reg. The
  // column's l is spread over its four lanes; alpha was common to them.
  const size_t Hq = static_cast<size_t>(Hkv) * G;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    float ls = l[c];
    ls += __shfl_xor(ls, 16);
    ls += __shfl_xor(ls, 32);
    if (col[c] >= ncol) continue;
    const int i = col[c] / G, jh = col[c] % G;
    float* ob = o + ((static_cast<size_t>(tok0) + i) * Hq + static_cast<size_t>(g) * G + jh) *
                        kAttnD + fq * 4;
#pragma unroll
    for (int dt = 0; dt < kAttnD / 16; ++dt) {
      f32x4 out;
#pragma unroll
      for (int e = 0; e < 4; ++e) out[e] = acc[c][dt][e] / ls;  // a true division
      *reinterpret_cast<f32x4*>(ob + dt * 16) = out;
    }
  }
}

// Device-side fill of the timed run: the dense hash pattern of the prefill
// payload (prefill_elem, sequence length L) in the pool through the table, one
// fragment (8 bf16) of each tensor per thread and step over `W << shift`
// logical chunks per (sequence, kv head); keys at and beyond lens[b] are zero.
// groups = B Hkv (W << shift) 4096 / 8, per tensor.
__global__ __launch_bounds__(kBlock) void attn_extend_fill_pool_kernel(
    uint16_t* __restrict__ k, uint16_t* __restrict__ vt, const int* __restrict__ table,
    const int* __restrict__ lens, int Hkv, int W, int shift, int L, size_t groups) {
  size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x;
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  const size_t chunks = static_cast<size_t>(W) << shift;
  for (; i < groups; i += stride) {
    const size_t image = i / 512, bg = image / chunks;
    const int lc = static_cast<int>(image % chunks), c0 = lc * kAttnChunk;
    const int b = static_cast<int>(bg / Hkv), g = static_cast<int>(bg % Hkv);
    const int len = lens[b];
    const size_t pg = static_cast<size_t>(table[static_cast<size_t>(b) * W + (lc >> shift)]);
    const size_t dst = ((pg * Hkv + g) << shift) + (lc & ((1 << shift) - 1));
    const int frag = static_cast<int>(i / 64) & 7, lane = static_cast<int>(i) & 63;
    const int fr = lane & 15, fq = lane >> 4;
    bf16x8 kv, vv;
    {  // K fragment (tile frag >> 2, d-step frag & 3): one key, 8 d
      const int t = c0 + 8 * (fr >> 2) + 4 * (frag >> 2) + (fr & 3);
      const int d0 = 32 * (frag & 3) + 8 * fq;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float f = t < len ? prefill_elem(kPrefillDense, 2, Hkv, L, b, g, t, d0 + j) : 0.f;
        kv[j] = static_cast<short>(__float_as_uint(f) >> 16);
      }
    }
    {  // V fragment (d-tile frag): one d, 8 keys
      const int d = 16 * frag + fr;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int t = c0 + 8 * fq + j;
        const float f = t < len ? prefill_elem(kPrefillDense, 3, Hkv, L, b, g, t, d) : 0.f;
        vv[j] = static_cast<short>(__float_as_uint(f) >> 16);
      }
    }
    const size_t at = (dst * 512 + i % 512) * 8;
    *reinterpret_cast<bf16x8*>(k + at) = kv;
    *reinterpret_cast<bf16x8*>(vt + at) = vv;
  }
}

// The same for the q image [Hkv][Tq][G][128]: token t of the packed q is row
// tok[t].y (its position) of sequence tok[t].x. pieces = Tq Hq 128 / 8.
__global__ __launch_bounds__(kBlock) void attn_extend_fill_q_kernel(
    uint16_t* __restrict__ q, const int2* __restrict__ tok, int Hq, int G, int Tq, int L,
    size_t pieces) {
  size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x;
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (; i < pieces; i += stride) {
    const int d0 = static_cast<int>(i & 15) * 8;
    const size_t row = i >> 4;  // (g Tq + t) G + j
    const int j = static_cast<int>(row % G);
    const int t = static_cast<int>(row / G % Tq), g = static_cast<int>(row / G / Tq);
    const int2 bp = tok[t];
    bf16x8 val;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float f = prefill_elem(kPrefillDense, 1, Hq, L, bp.x, g * G + j, bp.y, d0 + e);
      val[e] = static_cast<short>(__float_as_uint(f) >> 16);
    }
    *reinterpret_cast<bf16x8*>(q + i * 8) = val;
  }
}

// ---- host layer ----------------------------------------------------------

struct AttnExtendResult {
  double tflops = 0;     // unmasked (row, key) pairs only
  double tok_per_s = 0;  // Tq per launch
  double max_rel = 0;    // 16 spread rows against fp64
  int items = 0;         // of the last launch
};

// The limits of the extend payload, or std::invalid_argument; no HIP call: the
// paged payload's, Tq >= 1, and what the column arithmetic (int) and the grid
// (ceil(Tq G / 128) + B rows) need. Returns Hq / Hkv.
inline int attn_extend_shape(long long B, long long Hq, long long Hkv, long long page,
                             long long W, long long P, long long Tq) {
  const int G = attn_paged_shape(B, Hq, Hkv, page, W, P);
  if (Tq < 1) throw std::invalid_argument("attn_extend: Tq must be >= 1");
  if (Tq > INT32_MAX / kAttnMaxGroup ||
      (Tq * G + kExtendCols - 1) / kExtendCols + B > 65535)
    throw std::invalid_argument("attn_extend: shape too large");
  return G;
}

namespace detail {

// qlens in 1 .. lens[b], and their sum is Tq
inline void attn_extend_check_qlens(const int* lens, const int* qlens, int B, int Tq) {
  long long sum = 0;
  for (int b = 0; b < B; ++b) {
    if (qlens[b] < 1 || qlens[b] > lens[b])
      throw std::invalid_argument("attn_extend: qlens must be in 1 .. lens[b]");
    sum += qlens[b];
  }
  if (sum != Tq) throw std::invalid_argument("attn_extend: q must hold sum(qlens) tokens");
}

// The paged bf16 problem (pool, table, lengths and their uploads) with what the
// extend step adds: the packed q image, qlens, the plan's buffers and an output
// per token. Of the base's buffers it allocates only those it uses.
struct AttnExtendProblem : AttnPagedProblem<AttnCacheBf16> {
  int Tq;
  DeviceBuffer dqlens, dcu;

  AttnExtendProblem(int b, int hq, int hkv, int pg, int w, int p, int tq, int dev)
      : AttnPagedProblem(b, hq, hkv, pg, w, p, 0, dev), Tq(tq) {
    attn_extend_shape(b, hq, hkv, pg, w, p, tq);
  }

  size_t q_elems() const { return static_cast<size_t>(Tq) * Hq * kAttnD; }
  int max_items() const { return (Tq * G + kExtendCols - 1) / kExtendCols + B; }

  void alloc() {
    HIP_CHECK(hipSetDevice(device));
    dq.alloc(q_elems() * sizeof(uint16_t));
    dk.alloc(pool_elems() * sizeof(uint16_t));
    dvt.alloc(pool_elems() * sizeof(uint16_t));
    dtable.alloc(static_cast<size_t>(B) * W * sizeof(int));
    dlens.alloc(static_cast<size_t>(B) * sizeof(int));
    dqlens.alloc(static_cast<size_t>(B) * sizeof(int));
    dcu.alloc(static_cast<size_t>(B) * sizeof(int));
    ditems.alloc(static_cast<size_t>(max_items()) * sizeof(int2));
    dnitems.alloc(sizeof(int));
    dout.alloc(q_elems() * sizeof(float));
  }

  void upload_table(const int* table, const int* lens, const int* qlens) {
    HIP_CHECK(hipMemcpy(dtable.p, table, static_cast<size_t>(B) * W * sizeof(int),
                        hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dlens.p, lens, static_cast<size_t>(B) * sizeof(int),
                        hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dqlens.p, qlens, static_cast<size_t>(B) * sizeof(int),
                        hipMemcpyHostToDevice));
  }

  // q (Tq, Hq, 128) float -> the bf16 image [Hkv][Tq][G][128]
  void upload_q(const float* q) {
    std::vector<uint16_t> hq(q_elems());
    for (int t = 0; t < Tq; ++t)
      for (int h = 0; h < Hq; ++h) {
        const size_t dst = ((static_cast<size_t>(h / G) * Tq + t) * G + h % G) * kAttnD;
        const float* src = q + (static_cast<size_t>(t) * Hq + h) * kAttnD;
        for (int d = 0; d < kAttnD; ++d) hq[dst + d] = to_bf16_rne(src[d]);
      }
    HIP_CHECK(hipMemcpy(dq.p, hq.data(), hq.size() * sizeof(uint16_t),
                        hipMemcpyHostToDevice));
  }

  // plan + extend
  void launch(float scale) const {
    hipLaunchKernelGGL(attn_extend_plan_kernel, dim3(1), dim3(kBlock), 0, 0,
                       dqlens.as<const int>(), B, G, ditems.as<int2>(), dcu.as<int>(),
                       dnitems.as<int>());
    hipLaunchKernelGGL(attn_extend_kernel,
                       dim3(static_cast<unsigned>(Hkv), static_cast<unsigned>(max_items())),
                       dim3(kBlock), 0, 0, dq.as<const uint16_t>(), dk.as<const uint16_t>(),
                       dvt.as<const uint16_t>(), dtable.as<const int>(),
                       dlens.as<const int>(), dqlens.as<const int>(),
                       ditems.as<const int2>(), dnitems.as<const int>(),
                       dcu.as<const int>(), dout.as<float>(), G, W, shift(), Tq,
                       attn_c2(scale));
  }

  void download(float* o) const {
    HIP_CHECK(hipMemcpy(o, dout.p, q_elems() * sizeof(float), hipMemcpyDeviceToHost));
  }
};

}  // namespace detail

// General entry. q and o (Tq, Hq, 128), k_pages and v_pages (P, Hkv, page,
// 128), all row-major float; table (B, W), lens and qlens (B) int32; Tq = sum of
// qlens. std::invalid_argument on an unsupported shape, a length outside 1 .. W
// page, a qlens outside 1 .. lens[b] or a sum other than Tq, a table entry
// below a length outside 0 .. P - 1, or a non-finite q or key of a chunk that
// will be read; all before any device work.
inline void attn_paged_extend(const float* q, const float* k_pages, const float* v_pages,
                              const int* table, const int* lens, const int* qlens, float* o,
                              int B, int Hq, int Hkv, int page, int W, int P, int Tq,
                              float scale, int device = 0) {
  detail::AttnExtendProblem p(B, Hq, Hkv, page, W, P, Tq, device);
  detail::attn_paged_check_table(table, lens, B, page, W, P);
  detail::attn_extend_check_qlens(lens, qlens, B, Tq);
  for (size_t i = 0, n = p.q_elems(); i < n; ++i)
    if (!std::isfinite(q[i]))
      throw std::invalid_argument("attn_extend: q has a non-finite element");
  detail::attn_paged_check_read(
      k_pages, v_pages, table, lens, B, Hkv, page, W, kAttnChunk,
      [](float x) { return !std::isfinite(x); },
      "attn_extend: k or v has a non-finite element in a chunk that is read");
  p.alloc();
  p.upload_table(table, lens, qlens);
  p.upload_q(q);
  p.upload_pool(k_pages, v_pages);
  p.launch(scale);
  HIP_CHECK(hipGetLastError());
  p.download(o);
}

// Self-check on a ragged batch derived from L. The lengths are
// run_attn_paged_check's (entry b % 4 of {L, 1, a multiple of 32, a multiple of
// page plus one}); qlens[b] is entry (b + b / 4) % 4 of {1, the whole length,
// min(17, len), len - ((len / 2) | 1)}: decode-shaped, an empty prefix, a run
// that straddles tiles, and an odd prefix, which ends inside a chunk. From B =
// 8 on every length meets two of them. Pool and table are
// detail::AttnPagedCase's: B spare pages, all NaN; -1 above a length; 1e30 at
// the stale keys of a read chunk. (a) prefill's selection pattern
// (prefill_check_pattern, causal): row i of sequence b is row lens[b] -
// qlens[b] + i of that closed form, which depends on the keys at or below it
// only; max_err, expect exactly 0. (b) the dense hash pattern of run_attn_check
// against fp64 (attn_ref_row over the p + 1 visible keys): max_rel <= 2^-8, the
// bound derived there.
inline AttnCheck run_attn_extend_check(int B, int Hq, int Hkv, int L, int page,
                                       int device = 0) {
  if (L < 1 || L > kExtendMaxLen)
    throw std::invalid_argument("attn_extend: L must be in 1 .. 2^24");
  attn_paged_shape(B, Hq, Hkv, page, 1, 1);  // page before it divides
  const int rule[4] = {L, 1, std::max(32, L / 2) / 32 * 32, std::max(1, L / page) * page + 1};
  std::vector<int> lens(B), qlens(B), cu(B);
  int Tq = 0;
  for (int b = 0; b < B; ++b) {
    const int len = lens[b] = rule[b % 4];
    const int qrule[4] = {1, len, std::min(17, len), std::max(1, len - ((len / 2) | 1))};
    cu[b] = Tq;
    Tq += qlens[b] = qrule[(b + b / 4) % 4];
  }
  const detail::AttnPagedCase c(B, Hq, Hkv, page, lens, 0, device);
  attn_extend_shape(B, Hq, Hkv, page, c.W, c.P, Tq);
  const int Lmax = c.Lmax, G = c.G;
  const float scale = detail::attn_default_scale();

  const size_t nq = static_cast<size_t>(Tq) * Hq * kAttnD;
  std::vector<float> q(nq), got(nq), k(c.nkv()), v(c.nkv());
  auto extend = [&] {
    const std::vector<float> kpool = c.pool(k.data(), NAN, 1e30f, kAttnChunk);
    const std::vector<float> vpool = c.pool(v.data(), NAN, 1e30f, kAttnChunk);
    attn_paged_extend(q.data(), kpool.data(), vpool.data(), c.table.data(), lens.data(),
                      qlens.data(), got.data(), B, Hq, Hkv, page, c.W, c.P, Tq, scale,
                      device);
  };
  // packed row (b, i, h) and the dense row (b, h, position) it is
  auto packed = [&](int b, int i, int h) {
    return (static_cast<size_t>(cu[b] + i) * Hq + h) * kAttnD;
  };
  AttnCheck r;
  {
    const size_t nd = static_cast<size_t>(B) * Hq * Lmax * kAttnD;
    std::vector<float> qd(nd), want(nd);
    prefill_check_pattern(qd.data(), k.data(), v.data(), want.data(), B, Hq, Hkv, Lmax, true);
    auto dense_row = [&](int b, int i, int h) {
      return ((static_cast<size_t>(b) * Hq + h) * Lmax + lens[b] - qlens[b] + i) * kAttnD;
    };
    for (int b = 0; b < B; ++b)
      for (int i = 0; i < qlens[b]; ++i)
        for (int h = 0; h < Hq; ++h)
          std::copy_n(qd.data() + dense_row(b, i, h), kAttnD, q.data() + packed(b, i, h));
    extend();
    for (int b = 0; b < B; ++b)
      for (int i = 0; i < qlens[b]; ++i)
        for (int h = 0; h < Hq; ++h)
          detail::note_err(r.max_err,
                           detail::attn_max_err(got.data() + packed(b, i, h),
                                                want.data() + dense_row(b, i, h), kAttnD));
  }

  double vmax = 0, max_abs = 0;
  for (size_t i = 0; i < nq; ++i) q[i] = detail::attn_dense(1, i, 256);
  for (size_t i = 0; i < c.nkv(); ++i) {
    k[i] = detail::attn_dense(2, i, 64);
    v[i] = detail::attn_dense(3, i, 64);
    vmax = std::max(vmax, std::fabs(static_cast<double>(v[i])));
  }
  extend();
  std::vector<double> w(Lmax), ref(kAttnD);
  for (int b = 0; b < B; ++b)
    for (int i = 0; i < qlens[b]; ++i)
      for (int h = 0; h < Hq; ++h) {
        const size_t bg = static_cast<size_t>(b) * Hkv + h / G, at = packed(b, i, h);
        detail::attn_ref_row(ref.data(), q.data() + at, k.data() + bg * Lmax * kAttnD,
                             v.data() + bg * Lmax * kAttnD, lens[b] - qlens[b] + i + 1,
                             static_cast<double>(scale), w);
        for (int d = 0; d < kAttnD; ++d)
          detail::note_err(max_abs, std::fabs(static_cast<double>(got[at + d]) - ref[d]));
      }
  r.max_rel = vmax > 0 ? max_abs / vmax : max_abs;
  return r;
}

// Timed run: sequences of L keys (`ragged`: detail::attn_paged_lens) of which
// the last min(N, lens[b]) are new, W = ceil(L / page) pages per sequence under
// a fixed scrambled table over a pool of B W + 3 pages. The pool and q are
// filled on the device with prefill's dense hash pattern (sequence length L),
// so at N = L this is run_prefill's problem on the same values, and for the
// reason given there: the probe is bound by the matrix cores, which clock
// higher on low-entropy data. One warm-up launch, `iters` launches (plan +
// extend) between events, then 16 spread rows are recomputed on the host in
// fp64. FLOPs count the unmasked pairs only: 4 * 128 * Hq * sum over the rows of
// (p + 1) per launch.
inline AttnExtendResult run_attn_extend(int B = 8, int Hq = 64, int Hkv = 8, int L = 4096,
                                        int N = 1024, int page = 64, int iters = 10,
                                        bool ragged = false, int device = 0) {
  if (iters < 1) throw std::invalid_argument("run_attn_extend: iters must be >= 1");
  if (L < 1 || L > kExtendMaxLen || N < 1)
    throw std::invalid_argument("run_attn_extend: L must be in 1 .. 2^24 and N >= 1");
  attn_paged_shape(B, Hq, Hkv, page, 1, 1);  // page before it divides
  const int W = (L + page - 1) / page;
  const long long Pll = static_cast<long long>(B) * W + 3;
  const std::vector<int> lens = detail::attn_paged_lens(B, L, ragged);
  std::vector<int> qlens(B);
  std::vector<int2> tok;  // per packed token: sequence, position
  double pairs = 0;
  for (int b = 0; b < B; ++b) {
    qlens[b] = std::min(N, lens[b]);
    for (int i = 0; i < qlens[b]; ++i) {
      tok.push_back(make_int2(b, lens[b] - qlens[b] + i));
      pairs += tok.back().y + 1.0;
    }
  }
  attn_extend_shape(B, Hq, Hkv, page, W, Pll, static_cast<long long>(tok.size()));
  const int P = static_cast<int>(Pll), Tq = static_cast<int>(tok.size());

  detail::AttnExtendProblem p(B, Hq, Hkv, page, W, P, Tq, device);
  const std::vector<int> table = detail::attn_paged_scrambled_table(B, W, P);
  p.alloc();
  p.upload_table(table.data(), lens.data(), qlens.data());
  detail::DeviceBuffer dtok;
  dtok.alloc(tok.size() * sizeof(int2));
  HIP_CHECK(hipMemcpy(dtok.p, tok.data(), tok.size() * sizeof(int2), hipMemcpyHostToDevice));
  const size_t groups = static_cast<size_t>(B) * Hkv * W * page * kAttnD / 8;
  const size_t pieces = p.q_elems() / 8;
  hipLaunchKernelGGL(attn_extend_fill_pool_kernel, dim3(grid_for(groups)), dim3(kBlock), 0, 0,
                     p.dk.as<uint16_t>(), p.dvt.as<uint16_t>(), p.dtable.as<const int>(),
                     p.dlens.as<const int>(), Hkv, W, p.shift(), L, groups);
  hipLaunchKernelGGL(attn_extend_fill_q_kernel, dim3(grid_for(pieces)), dim3(kBlock), 0, 0,
                     p.dq.as<uint16_t>(), dtok.as<const int2>(), Hq, p.G, Tq, L, pieces);
  HIP_CHECK(hipGetLastError());

  const float scale = detail::attn_default_scale();
  const float ms = detail::time_launches(iters, [&p, scale] { p.launch(scale); });
  AttnExtendResult r;
  const double sec = ms * 1e-3;
  r.tflops = 4.0 * kAttnD * Hq * pairs * iters / sec / 1e12;
  r.tok_per_s = static_cast<double>(Tq) * iters / sec;
  r.items = p.items();

  std::vector<float> got(kAttnD), qr(kAttnD);
  std::vector<float> kh(static_cast<size_t>(L) * kAttnD), vh(kh.size());
  std::vector<double> w(L), ref(kAttnD);
  double max_abs = 0, vmax = 0;
  for (int t = 0; t < 16; ++t) {
    const size_t row = detail::attn_spread_row(t, static_cast<size_t>(Tq) * Hq);
    const int h = static_cast<int>(row % Hq), g = h / p.G;
    const int b = tok[row / Hq].x, n = tok[row / Hq].y + 1;
    for (int d = 0; d < kAttnD; ++d)
      qr[d] = prefill_elem(kPrefillDense, 1, Hq, L, b, h, n - 1, d);
    for (int u = 0; u < n; ++u)
      for (int d = 0; d < kAttnD; ++d) {
        const size_t at = static_cast<size_t>(u) * kAttnD + d;
        kh[at] = prefill_elem(kPrefillDense, 2, Hkv, L, b, g, u, d);
        vh[at] = prefill_elem(kPrefillDense, 3, Hkv, L, b, g, u, d);
        vmax = std::max(vmax, std::fabs(static_cast<double>(vh[at])));
      }
    detail::attn_ref_row(ref.data(), qr.data(), kh.data(), vh.data(), n,
                         static_cast<double>(scale), w);
    HIP_CHECK(hipMemcpy(got.data(), p.dout.as<float>() + row * kAttnD,
                        kAttnD * sizeof(float), hipMemcpyDeviceToHost));
    for (int d = 0; d < kAttnD; ++d)
      detail::note_err(max_abs, std::fabs(static_cast<double>(got[d]) - ref[d]));
  }
  r.max_rel = vmax > 0 ? max_abs / vmax : max_abs;
  return r;
}

}  // namespace payload
