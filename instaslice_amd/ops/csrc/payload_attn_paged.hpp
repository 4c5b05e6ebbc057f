// gfx950 paged, ragged-batch KV-cache decode attention payload.
//
// attn (payload_attn.hpp) streams a cache that the host lays out as one
// contiguous, equally padded run of chunk images per (sequence, kv head), with
// one split count for the whole batch. An inference server keeps a pool of
// fixed-size pages instead, reaches a sequence's pages through a block table,
// batches lengths that differ by orders of magnitude and lets sequences share
// the pages of a common prefix. This payload is that path:
//
//   o[b,h,:] = softmax_t(scale * q[b,h,:] . K_b[g,t,:]) . V_b[g,t,:],  t < len[b]
//
// where key t of sequence b lives in physical page table[b][t / page], at key
// t % page of it. The arithmetic (QK, key order, base-2 online softmax with the
// -inf guards, P in registers, PV, the merge weights) is the contiguous
// kernel's; what is new is how a chunk is found and how the work is split.
//
//   cache        a pool of P pages of `page` keys, page in {32, 64, 128, 256}.
//                Page p holds, for each kv head g and each 32-key chunk c of
//                the page, one K image and one V image of 4096 bf16 in the
//                fragment order of attn_k_off / attn_v_off, at image index
//                (p * Hkv + g) * (page / 32) + c.
//   table        int32 [B][W]. Only the entries below ceil(len[b] / page) are
//                read; they lie in 0 .. P - 1 (the host checks). The others
//                may hold anything. A page may appear in several sequences.
//   stale keys   keys at and beyond len[b] inside a chunk that is read are
//                masked by index: K there may be any finite value, V must be
//                finite (its weight is an exact 0 that goes through the MFMA).
//                Chunks at and beyond ceil(len[b] / 32) are never read, nor
//                are pages that no entry below a length names.
//   plan         lengths change every decode step, so the split is computed on
//                the device, in every launch. attn_paged_plan_kernel (one
//                workgroup) sums the batch's chunks C, takes a budget per =
//                ceil(C / target) chunks per item and gives sequence b n_b =
//                ceil(chunks_b / per) items of near-equal chunk ranges: an LDS
//                prefix scan over b, 256 sequences per stride with a carry.
//                It writes the item table {b, chunk_begin, chunk_end, item of
//                the sequence} and per sequence {first part, n_b * 4}. Items
//                never span sequences, so there are at most target + B of
//                them; the order is that of (b, chunk), so results do not
//                depend on timing. attn_paged_plan() is the same arithmetic on
//                the host and the specification.
//   decode       grid (Hkv, target + B), 4 wave64s, no LDS, no barrier; a
//                workgroup beyond the item count leaves at once, and those are
//                the last of the grid. The item's chunks are dealt round-robin
//                to the waves. A wave resolves a chunk by a wave-uniform
//                scalar load of its table entry and forms the image address in
//                size_t. K is requested one chunk ahead, so the table entry is
//                fetched two chunks ahead: the indirection's latency sits
//                under the previous chunk's MFMAs and softmax, not in front of
//                the K loads. Every wave writes one unnormalised (m, l,
//                o[128]); a wave with no chunk writes m = -inf.
//   combine      one workgroup per output row merges the row's n_b * 4
//                partials, a count that differs per sequence.
//
// Partials of row (b, h) start at first_part[b] * Hq + h * n_b * 4, part =
// item of the sequence * 4 + wave: a row's partials are contiguous.
//
// The problem struct, the check case and the timed run stand once here for
// every cache format; payload_attn_fp8.hpp adds the e4m3 format (AttnCacheFp8)
// to the bf16 one (AttnCacheBf16). Each format has its own decode kernel.
//
// Included by payload_core.hpp after payload_attn.hpp, whose helpers it uses:
// the chunk step (attn_load_q, attn_load_image, attn_qk, attn_softmax_pv,
// attn_write_partial), the fill kernel, the layout and pattern functions,
// detail::attn_ref_row, the dense hash pattern and kAttnRelBound.

#pragma once

#include <numeric>

namespace payload {

constexpr int kAttnPagedMaxTarget = 4096;  // `workgroups` at most

// ---- the plan --------------------------------------------------------------

struct AttnPagedPlan {
  std::vector<int> items;  // 3 per item: b, chunk_begin, chunk_end
  std::vector<int> seq;    // 2 per sequence: first part, parts (items * 4)
};

// `chunk` keys: 32 for the bf16 cache, 64 for the fp8 one (payload_attn_fp8.hpp)
__host__ __device__ inline int attn_paged_chunks(int len, int chunk = kAttnChunk) {
  return (len + chunk - 1) / chunk;
}

// chunk where item j of n starts in a sequence of c chunks (j = n: c)
__host__ __device__ inline int attn_paged_cut(int c, int n, int j) {
  return static_cast<int>(static_cast<long long>(c) * j / n);
}

// The specification of attn_paged_plan_kernel. lens[b] >= 1, target in 1 ..
// 4096, chunk 32 or 64, sum_b ceil(lens[b] / chunk) below 2^31.
inline AttnPagedPlan attn_paged_plan(const int* lens, int B, int target,
                                     int chunk = kAttnChunk) {
  if (B < 1 || target < 1 || target > kAttnPagedMaxTarget)
    throw std::invalid_argument("attn_paged_plan: B >= 1 and target in 1 .. 4096");
  if (chunk != 32 && chunk != 64)
    throw std::invalid_argument("attn_paged_plan: chunk must be 32 or 64");
  long long C = 0;
  for (int b = 0; b < B; ++b) {
    if (lens[b] < 1) throw std::invalid_argument("attn_paged_plan: lengths must be >= 1");
    C += attn_paged_chunks(lens[b], chunk);
  }
  if (C > INT32_MAX) throw std::invalid_argument("attn_paged_plan: too many chunks");
  const int per = static_cast<int>((C + target - 1) / target);
  AttnPagedPlan p;
  int first = 0;
  for (int b = 0; b < B; ++b) {
    const int c = attn_paged_chunks(lens[b], chunk), n = (c + per - 1) / per;
    p.seq.push_back(first * kAttnWaves);
    p.seq.push_back(n * kAttnWaves);
    for (int j = 0; j < n; ++j) {
      p.items.push_back(b);
      p.items.push_back(attn_paged_cut(c, n, j));
      p.items.push_back(attn_paged_cut(c, n, j + 1));
    }
    first += n;
  }
  return p;
}

// ---- kernels -------------------------------------------------------------

// One workgroup. lens: [B], clamped to 0 .. Lmax. items: target + B entries.
// seq: [B]. nitems: one int. The plan counts chunks of `chunk` keys.
__global__ __launch_bounds__(kBlock) void attn_paged_plan_kernel(
    const int* __restrict__ lens, int B, int Lmax, int target,
    int4* __restrict__ items, int2* __restrict__ seq, int* __restrict__ nitems,
    int chunk = kAttnChunk) {
  __shared__ int scan[kBlock];
  __shared__ int carry;
  const int tid = threadIdx.x;

  int mine = 0;  // chunks of the sequences tid, tid + 256, ...
  for (int b = tid; b < B; b += kBlock)
    mine += attn_paged_chunks(min(max(lens[b], 0), Lmax), chunk);
  scan[tid] = mine;
  if (tid == 0) carry = 0;
  __syncthreads();
  int top = 1;  // entries at and beyond min(B, 256) are zero
  while (top < min(B, kBlock)) top <<= 1;
  for (int d = top / 2; d > 0; d >>= 1) {
    if (tid < d) scan[tid] += scan[tid + d];
    __syncthreads();
  }
  const int C = scan[0];
  const int per = max(1, (C + target - 1) / target);
  __syncthreads();

  for (int b0 = 0; b0 < B; b0 += kBlock) {  // block-uniform
    const int b = b0 + tid;
    const int c = b < B ? attn_paged_chunks(min(max(lens[b], 0), Lmax), chunk) : 0;
    const int n = (c + per - 1) / per;
    scan[tid] = n;
    __syncthreads();
    const int live = min(kBlock, B - b0);  // the rest of scan is zero
    for (int d = 1; d < live; d <<= 1) {  // inclusive scan of the live entries
      const int v = tid >= d ? scan[tid - d] : 0;
      __syncthreads();
      scan[tid] += v;
      __syncthreads();
    }
    const int first = carry + scan[tid] - n;
    if (b < B) seq[b] = make_int2(first * kAttnWaves, n * kAttnWaves);
    for (int j = 0; j < n; ++j)
      items[first + j] =
          make_int4(b, attn_paged_cut(c, n, j), attn_paged_cut(c, n, j + 1), j);
    __syncthreads();  // every thread has read carry
    if (tid == live - 1) carry += scan[tid];
    __syncthreads();
  }
  if (tid == 0) *nitems = carry;
}

// q: [B][Hkv][16][128] bf16, rows G .. 15 zero. kp, vp: the pool's chunk
// images. table: [B][W]. shift = log2(page / 32). Partials as described at the
// top. grid = (Hkv, target + B): the kv head is the fast index, so that the
// workgroups beyond the item count are the last to be dispatched and take no
// CU from a live one. The chunk step is attn_decode_kernel's (payload_attn.hpp).
__global__ __launch_bounds__(kBlock) void attn_paged_decode_kernel(
    const uint16_t* __restrict__ q, const uint16_t* __restrict__ kp,
    const uint16_t* __restrict__ vp, const int* __restrict__ table,
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

  // element offset of this lane's first fragment in chunk ch of physical page pg
  auto image = [&](int pg, int ch) {
    const size_t idx =
        ((static_cast<size_t>(pg) * Hkv + g) << shift) + static_cast<size_t>(ch & cmask);
    return idx * kAttnChunkElems + static_cast<size_t>(lane) * 8;
  };

  bf16x8 fqt[kAttnD / 32];
  attn_load_q(fqt, q, static_cast<size_t>(b) * Hkv + g, fr, fq);

  float m = -INFINITY, l = 0.f;
  f32x4 o[kAttnD / 16];
#pragma unroll
  for (int dt = 0; dt < kAttnD / 16; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

  // pg_v: the page of the chunk in hand (its K is in flight or here); pg_k: the
  // page of the wave's next chunk, fetched a whole chunk before its K loads
  bf16x8 fk[8];
  int ch = it.y + wave;
  int pg_v = 0, pg_k = 0;
  if (ch < ch_end) {
    pg_v = trow[ch >> shift];
    attn_load_image(fk, kp + image(pg_v, ch));
  }
  if (ch + kAttnWaves < ch_end) pg_k = trow[(ch + kAttnWaves) >> shift];

  for (; ch < ch_end; ch += kAttnWaves) {  // wave-uniform
    bf16x8 fv[8];
    attn_load_image(fv, vp + image(pg_v, ch));
    f32x4 st[2];
    attn_qk(fk, fqt, st);

    const int nx = ch + kAttnWaves;
    if (nx < ch_end) attn_load_image(fk, kp + image(pg_k, nx));
    pg_v = pg_k;
    if (nx + kAttnWaves < ch_end) pg_k = trow[(nx + kAttnWaves) >> shift];

    attn_softmax_pv(st, fv, ch * kAttnChunk, fq, len, c2, m, l, o);
  }

  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);

  if (fr < G) {
    const int2 sq = seq[b];
    const size_t Hq = static_cast<size_t>(Hkv) * G;
    const size_t part = static_cast<size_t>(sq.x) * Hq +
                        (static_cast<size_t>(g) * G + fr) * sq.y +
                        static_cast<size_t>(it.w) * kAttnWaves + wave;
    attn_write_partial(pm, pl, po, part, fq, m, l, o);
  }
}

// attn_combine_kernel over a row's own part count. grid = B Hq, block = 128.
__global__ __launch_bounds__(kAttnD) void attn_paged_combine_kernel(
    const float* __restrict__ pm, const float* __restrict__ pl,
    const float* __restrict__ po, const int2* __restrict__ seq,
    float* __restrict__ out, int Hq) {
  const size_t row = blockIdx.x;
  const int d = threadIdx.x;
  const int2 sq = seq[row / Hq];
  const int P = sq.y;
  const size_t base = static_cast<size_t>(sq.x) * Hq + (row % Hq) * P;
  const float* m = pm + base;
  const float* l = pl + base;
  const float* o = po + base * kAttnD + d;
  float mx = -INFINITY;
  for (int i = 0; i < P; ++i) mx = fmaxf(mx, m[i]);
  float ls = 0.f, acc = 0.f;
  for (int i = 0; i < P; ++i) {
    const float mi = m[i];
    if (mi == -INFINITY) continue;  // a wave with no chunk: weight 0
    const float w = __builtin_amdgcn_exp2f(mi - mx);
    ls += w * l[i];
    acc += w * o[static_cast<size_t>(i) * kAttnD];
  }
  out[row * kAttnD + d] = acc / ls;  // the only division, and a true one
}

// ---- host layer ----------------------------------------------------------

struct AttnPagedResult : AttnResult {
  int items = 0;  // of the last launch
};

// The limits of the paged payload, or std::invalid_argument; no HIP call.
// Returns Hq / Hkv.
inline int attn_paged_shape(long long B, long long Hq, long long Hkv, long long page,
                            long long W, long long P, long long workgroups = 0) {
  const long long G = detail::attn_group("attn_paged", B, Hq, Hkv, 1);
  if (G > kAttnMaxGroup)
    throw std::invalid_argument("attn_paged: Hq / Hkv must be <= 16");
  if (page != 32 && page != 64 && page != 128 && page != 256)
    throw std::invalid_argument("attn_paged: page must be 32, 64, 128 or 256");
  if (W < 1 || P < 1)
    throw std::invalid_argument("attn_paged: W and P must be >= 1");
  if (workgroups < 0 || workgroups > kAttnPagedMaxTarget)
    throw std::invalid_argument("attn_paged: workgroups must be in 0 .. 4096");
  if (B > 65535 - kAttnPagedMaxTarget || Hkv > 65535 || P > INT32_MAX || W > (1 << 28) / page ||
      B * W * (page / kAttnChunk) > INT32_MAX)
    throw std::invalid_argument("attn_paged: shape too large");
  return static_cast<int>(G);
}

namespace detail {

// Lengths in 1 .. W page, and every table entry that will be read in 0 .. P - 1
inline void attn_paged_check_table(const int* table, const int* lens, int B, int page,
                                   int W, int P) {
  for (int b = 0; b < B; ++b) {
    if (lens[b] < 1 || lens[b] > static_cast<long long>(W) * page)
      throw std::invalid_argument("attn_paged: lengths must be in 1 .. W * page");
    const int used = (lens[b] + page - 1) / page;
    for (int w = 0; w < used; ++w) {
      const int pg = table[static_cast<size_t>(b) * W + w];
      if (pg < 0 || pg >= P)
        throw std::invalid_argument(
            "attn_paged: a table entry below a length is outside 0 .. P - 1");
    }
  }
}

// a table of B W different pages out of P >= B W, scrambled: entry i names
// page (i a + 1) % P with a coprime to P
inline std::vector<int> attn_paged_scrambled_table(int B, int W, int P) {
  long long a = 7919;
  while (std::gcd(a, static_cast<long long>(P)) != 1) a += 2;
  std::vector<int> table(static_cast<size_t>(B) * W);
  for (size_t i = 0; i < table.size(); ++i)
    table[i] = static_cast<int>((static_cast<long long>(i) * a + 1) % P);
  return table;
}

// Shape and device buffers of one paged problem over a cache of format C
// (AttnCacheBf16, AttnCacheFp8), and of a step's three launches the two that do
// not depend on the format; a format's problem adds launch() with its decode
// kernel between them.
template <class C>
struct AttnPagedProblem : AttnShape {
  int page, W, P, target;
  DeviceBuffer dq, dk, dvt, dtable, dlens, ditems, dseq, dnitems, dpm, dpl, dpo, dout;

  // L is the longest a sequence may be, W page; the shape is checked before
  // that product is formed
  AttnPagedProblem(int b, int hq, int hkv, int pg, int w, int p, int workgroups, int dev)
      : AttnShape{b, hq, hkv, 0, attn_paged_shape(b, hq, hkv, pg, w, p, workgroups), dev},
        page(pg), W(w), P(p), target(workgroups) {
    L = w * pg;
  }

  int shift() const { return __builtin_ctz(page / C::kChunk); }  // chunks of a page
  size_t pool_elems() const {
    return static_cast<size_t>(P) * Hkv * page * kAttnD;
  }
  size_t rows() const { return static_cast<size_t>(B) * Hq; }
  int max_items() const { return target + B; }

  // workgroups = 0: items for half the visible CUs, the count that
  // profiles/attn_probe.md found best for the contiguous kernel
  void alloc() {
    HIP_CHECK(hipSetDevice(device));
    if (target == 0) {
      int cus = 0;
      HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount,
                                      device));
      target = std::max(1, cus / (2 * Hkv));
    }
    const size_t parts = static_cast<size_t>(max_items()) * kAttnWaves * Hq;
    dq.alloc(static_cast<size_t>(B) * Hkv * 16 * kAttnD * sizeof(uint16_t));
    dk.alloc(pool_elems() * sizeof(typename C::Elem));
    dvt.alloc(pool_elems() * sizeof(typename C::Elem));
    dtable.alloc(static_cast<size_t>(B) * W * sizeof(int));
    dlens.alloc(static_cast<size_t>(B) * sizeof(int));
    ditems.alloc(static_cast<size_t>(max_items()) * sizeof(int4));
    dseq.alloc(static_cast<size_t>(B) * sizeof(int2));
    dnitems.alloc(sizeof(int));
    dpm.alloc(parts * sizeof(float));
    dpl.alloc(parts * sizeof(float));
    dpo.alloc(parts * kAttnD * sizeof(float));
    dout.alloc(rows() * kAttnD * sizeof(float));
  }

  // q (B, Hq, 128) float -> the padded bf16 image; the table and the lengths
  void upload_q_table(const float* q, const int* table, const int* lens) {
    std::vector<uint16_t> hq(static_cast<size_t>(B) * Hkv * 16 * kAttnD, 0);
    for (int b = 0; b < B; ++b)
      for (int h = 0; h < Hq; ++h) {
        const size_t dst = ((static_cast<size_t>(b) * Hkv + h / G) * 16 + h % G) * kAttnD;
        const float* src = q + (static_cast<size_t>(b) * Hq + h) * kAttnD;
        for (int d = 0; d < kAttnD; ++d) hq[dst + d] = to_bf16_rne(src[d]);
      }
    HIP_CHECK(hipMemcpy(dq.p, hq.data(), hq.size() * sizeof(uint16_t),
                        hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dtable.p, table, static_cast<size_t>(B) * W * sizeof(int),
                        hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dlens.p, lens, static_cast<size_t>(B) * sizeof(int),
                        hipMemcpyHostToDevice));
  }

  // k, v (P, Hkv, page, 128) in plain key-major order -> the pool's chunk
  // images, every page of it, referenced or not
  void upload_pool(const typename C::Host* k, const typename C::Host* v) {
    std::vector<typename C::Elem> hk(pool_elems()), hvt(pool_elems());
    const size_t heads = static_cast<size_t>(P) * Hkv;
    for (size_t pgh = 0; pgh < heads; ++pgh)
      for (int t = 0; t < page; ++t) {
        const size_t src = (pgh * page + t) * kAttnD;
        const size_t image = ((pgh << shift()) + t / C::kChunk) * C::kImage;
        const int w = t % C::kChunk;
        for (int d = 0; d < kAttnD; ++d) {
          hk[image + C::k_off(w, d)] = C::encode(k[src + d]);
          hvt[image + C::v_off(w, d)] = C::encode(v[src + d]);
        }
      }
    HIP_CHECK(hipMemcpy(dk.p, hk.data(), hk.size() * sizeof(typename C::Elem),
                        hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dvt.p, hvt.data(), hvt.size() * sizeof(typename C::Elem),
                        hipMemcpyHostToDevice));
  }

  // the plan in chunks of C::kChunk keys, the decode kernel's grid, the combine
  void plan() const {
    hipLaunchKernelGGL(attn_paged_plan_kernel, dim3(1), dim3(kBlock), 0, 0,
                       dlens.as<const int>(), B, L, target, ditems.as<int4>(),
                       dseq.as<int2>(), dnitems.as<int>(), C::kChunk);
  }
  dim3 grid() const {
    return dim3(static_cast<unsigned>(Hkv), static_cast<unsigned>(max_items()));
  }
  void combine() const {
    hipLaunchKernelGGL(attn_paged_combine_kernel, dim3(static_cast<unsigned>(rows())),
                       dim3(kAttnD), 0, 0, dpm.as<const float>(), dpl.as<const float>(),
                       dpo.as<const float>(), dseq.as<const int2>(), dout.as<float>(),
                       Hq);
  }
  void download(float* o) const {
    HIP_CHECK(hipMemcpy(o, dout.p, rows() * kAttnD * sizeof(float),
                        hipMemcpyDeviceToHost));
  }

  int items() const {
    int n = 0;
    HIP_CHECK(hipMemcpy(&n, dnitems.p, sizeof(int), hipMemcpyDeviceToHost));
    return n;
  }
};

// the paged problem over the bf16 cache
struct AttnPagedBf16Problem : AttnPagedProblem<AttnCacheBf16> {
  using AttnPagedProblem::AttnPagedProblem;

  // plan + decode + combine
  void launch(float scale) const {
    plan();
    hipLaunchKernelGGL(attn_paged_decode_kernel, grid(), dim3(kBlock), 0, 0,
                       dq.as<const uint16_t>(), dk.as<const uint16_t>(),
                       dvt.as<const uint16_t>(), dtable.as<const int>(),
                       dlens.as<const int>(), ditems.as<const int4>(),
                       dnitems.as<const int>(), dseq.as<const int2>(), dpm.as<float>(),
                       dpl.as<float>(), dpo.as<float>(), G, W, shift(), L, attn_c2(scale));
    combine();
  }
};

// the fixed ragged rule of the timed run: L for every eighth sequence, L / 8
// for the rest
inline std::vector<int> attn_paged_lens(int B, int L, bool ragged) {
  std::vector<int> lens(B, L);
  if (ragged)
    for (int b = 0; b < B; ++b)
      if (b % 8 != 0) lens[b] = std::max(1, L / 8);
  return lens;
}

// dense (B, Hkv, L, 128), L >= lens[b] -> the pool (P, Hkv, page, 128) under
// the table: the keys below lens[b], and `stale` at the further keys of the
// last chunk (of `chunk` keys) that is read. Nothing else of the pool is written.
template <class T>
inline void attn_paged_scatter(const T* dense, T* pool, const int* table,
                               const int* lens, int B, int Hkv, int L, int page, int W,
                               T stale, int chunk = kAttnChunk) {
  for (int b = 0; b < B; ++b) {
    const int read = static_cast<int>(round_up(lens[b], chunk));
    for (int g = 0; g < Hkv; ++g)
      for (int t = 0; t < read; ++t) {
        const size_t pg = static_cast<size_t>(table[static_cast<size_t>(b) * W + t / page]);
        T* dst = pool + ((pg * Hkv + g) * page + t % page) * kAttnD;
        const T* src =
            dense + ((static_cast<size_t>(b) * Hkv + g) * L + std::min(t, L - 1)) * kAttnD;
        for (int d = 0; d < kAttnD; ++d) dst[d] = t < lens[b] ? src[d] : stale;
      }
  }
}

// std::invalid_argument(msg) where bad(k) or bad(v) at an element of a key of a
// chunk (of `chunk` keys) that will be read; the pools are (P, Hkv, page, 128)
template <class T, class Bad>
inline void attn_paged_check_read(const T* k, const T* v, const int* table, const int* lens,
                                  int B, int Hkv, int page, int W, int chunk, Bad bad,
                                  const char* msg) {
  for (int b = 0; b < B; ++b) {
    const int read = static_cast<int>(round_up(lens[b], chunk));
    for (int g = 0; g < Hkv; ++g)
      for (int t = 0; t < read; ++t) {
        const size_t pg = static_cast<size_t>(table[static_cast<size_t>(b) * W + t / page]);
        const size_t at = ((pg * Hkv + g) * page + t % page) * kAttnD;
        for (int d = 0; d < kAttnD; ++d)
          if (bad(k[at + d]) || bad(v[at + d])) throw std::invalid_argument(msg);
      }
  }
}

// One paged problem of the checks of either format: lengths, W pages for the
// longest, a scrambled table with -1 above a length, and a pool with B spare
// pages. The page size has been checked.
struct AttnPagedCase {
  int B, Hq, Hkv, G, page, W, P, Lmax, workgroups, device;
  std::vector<int> lens, table;

  AttnPagedCase(int b, int hq, int hkv, int pg, std::vector<int> lengths, int wg, int dev)
      : B(b), Hq(hq), Hkv(hkv), page(pg), workgroups(wg), device(dev),
        lens(std::move(lengths)) {
    Lmax = *std::max_element(lens.begin(), lens.end());
    W = (Lmax + page - 1) / page;
    const long long Pll = static_cast<long long>(B) * W + B;
    G = attn_paged_shape(B, Hq, Hkv, page, W, Pll, workgroups);
    P = static_cast<int>(Pll);
    table = attn_paged_scrambled_table(B, W, P);
    for (int i = 0; i < B; ++i)
      for (int w = (lens[i] + page - 1) / page; w < W; ++w)
        table[static_cast<size_t>(i) * W + w] = -1;
  }

  size_t nq() const { return static_cast<size_t>(B) * Hq * kAttnD; }
  size_t nkv() const { return static_cast<size_t>(B) * Hkv * Lmax * kAttnD; }

  // dense (B, Hkv, Lmax, 128) -> a pool that is all `poison` but for what will
  // be read (in chunks of `chunk` keys), with `stale` at the stale keys of that
  template <class T>
  std::vector<T> pool(const T* dense, T poison, T stale, int chunk) const {
    std::vector<T> pl(static_cast<size_t>(P) * Hkv * page * kAttnD, poison);
    attn_paged_scatter(dense, pl.data(), table.data(), lens.data(), B, Hkv, Lmax, page, W,
                       stale, chunk);
    return pl;
  }

  // max |got - fp64 attention on (q, k, v)| / max |v|
  double rel_error(const float* got, const float* q, const float* k, const float* v) const {
    std::vector<double> w(Lmax), ref(kAttnD);
    double max_abs = 0, vmax = 0;
    for (size_t i = 0; i < nkv(); ++i)
      vmax = std::max(vmax, std::fabs(static_cast<double>(v[i])));
    for (int b = 0; b < B; ++b)
      for (int h = 0; h < Hq; ++h) {
        const size_t bg = static_cast<size_t>(b) * Hkv + h / G;
        const size_t at = (static_cast<size_t>(b) * Hq + h) * kAttnD;
        attn_ref_row(ref.data(), q + at, k + bg * Lmax * kAttnD, v + bg * Lmax * kAttnD,
                     lens[b], static_cast<double>(attn_default_scale()), w);
        for (int d = 0; d < kAttnD; ++d)
          note_err(max_abs, std::fabs(static_cast<double>(got[at + d]) - ref[d]));
      }
    return vmax > 0 ? max_abs / vmax : max_abs;
  }
};

// What the timed runs of both formats are given and derive: the checked ranges
// (`who` heads the messages, `shape` is the format's limits), W = ceil(L / page)
// pages per sequence, a pool of P = B W + 3, the lengths and the pattern's q.
struct AttnPagedTimed {
  int B, Hq, Hkv, iters, W, P;
  std::vector<int> lens;
  std::vector<float> q;

  template <class Shape>
  AttnPagedTimed(const std::string& who, Shape shape, int b, int hq, int hkv, int L,
                 int page, int it, bool ragged, int workgroups)
      : B(b), Hq(hq), Hkv(hkv), iters(it) {
    if (iters < 1) throw std::invalid_argument(who + ": iters must be >= 1");
    if (L < 1 || L > (1 << 28)) throw std::invalid_argument(who + ": L must be in 1 .. 2^28");
    shape(B, Hq, Hkv, page, 1, 1, workgroups);
    W = (L + page - 1) / page;
    const long long Pll = static_cast<long long>(B) * W + 3;
    shape(B, Hq, Hkv, page, W, Pll, workgroups);
    P = static_cast<int>(Pll);
    lens = attn_paged_lens(B, L, ragged);
    q.resize(static_cast<size_t>(B) * Hq * kAttnD);
    attn_pattern_q(q.data(), B, Hq);
  }

  // the rates of `iters` launches that took ms and read kv_bytes per cache
  // element (K and V), and the 16 spread rows of the output at dout, exactly
  void report(AttnResult& r, float ms, const float* dout, double kv_bytes) const {
    const double sec = ms * 1e-3;
    double keys = 0;
    for (int len : lens) keys += len;
    r.steps_per_s = iters / sec;
    r.tok_per_s = r.steps_per_s * B;
    r.kv_gb_s = keys * Hkv * kAttnD * kv_bytes * iters / sec / 1e9;
    std::vector<float> got(kAttnD), want(kAttnD);
    for (int t = 0; t < 16; ++t) {
      const size_t row = attn_spread_row(t, static_cast<size_t>(B) * Hq);
      HIP_CHECK(hipMemcpy(got.data(), dout + row * kAttnD, kAttnD * sizeof(float),
                          hipMemcpyDeviceToHost));
      const int b = static_cast<int>(row / Hq);
      attn_pattern_row(want.data(), b, static_cast<int>(row % Hq), Hq / Hkv, lens[b]);
      note_err(r.max_err, attn_max_err(got.data(), want.data(), kAttnD));
    }
  }

  // The paged problem p under a fixed scrambled table: `fill` writes the pool
  // (and what else the format needs) on the device, `launch` is timed. Returns
  // the milliseconds that report() takes, with the item count in r.
  template <class Problem, class Fill, class Launch>
  float time(AttnPagedResult& r, Problem& p, Fill fill, Launch launch) const {
    const std::vector<int> table = attn_paged_scrambled_table(B, W, P);
    p.alloc();
    p.upload_q_table(q.data(), table.data(), lens.data());
    fill();
    HIP_CHECK(hipGetLastError());
    const float ms = time_launches(iters, launch);
    r.items = p.items();
    return ms;
  }
};

}  // namespace detail

// General entry. q (B, Hq, 128), k_pages and v_pages (P, Hkv, page, 128), o (B,
// Hq, 128), all row-major float; table (B, W) and lens (B) int32; workgroups 0
// = auto. std::invalid_argument on an unsupported shape, a length outside 1 ..
// W page, a table entry below a length outside 0 .. P - 1, or a non-finite q or
// key of a chunk that will be read; all before any device work.
inline void attn_paged_decode(const float* q, const float* k_pages, const float* v_pages,
                              const int* table, const int* lens, float* o, int B, int Hq,
                              int Hkv, int page, int W, int P, float scale,
                              int workgroups = 0, int device = 0) {
  detail::AttnPagedBf16Problem p(B, Hq, Hkv, page, W, P, workgroups, device);
  detail::attn_paged_check_table(table, lens, B, page, W, P);
  for (size_t i = 0, n = p.rows() * kAttnD; i < n; ++i)
    if (!std::isfinite(q[i]))
      throw std::invalid_argument("attn_paged: q has a non-finite element");
  detail::attn_paged_check_read(
      k_pages, v_pages, table, lens, B, Hkv, page, W, kAttnChunk,
      [](float x) { return !std::isfinite(x); },
      "attn_paged: k or v has a non-finite element in a chunk that is read");
  p.alloc();
  p.upload_q_table(q, table, lens);
  p.upload_pool(k_pages, v_pages);
  p.launch(scale);
  HIP_CHECK(hipGetLastError());
  p.download(o);
}

// Self-check on ragged lengths derived from L, sequence b taking entry b % 4 of
// {L, 1, the largest multiple of 32 up to max(32, L / 2), max(1, L / page) page
// + 1}: from B = 4 on the batch holds a single key, a whole number of chunks
// and one key past a page boundary. Pool and table are detail::AttnPagedCase's:
// B more pages than the table names, all NaN; a scrambled table with -1 above a
// sequence's length; stale keys of a read chunk hold 1e30 in K and V. (a) the
// selection pattern against its closed form: max_err, expect exactly 0. (b) the
// dense hash pattern of run_attn_check against fp64: max_rel <= 2^-8, the bound
// derived there, which does not depend on how the keys are split.
inline AttnCheck run_attn_paged_check(int B, int Hq, int Hkv, int L, int page,
                                      int workgroups = 0, int device = 0) {
  if (L < 1 || L > (1 << 24))
    throw std::invalid_argument("attn_paged: L must be in 1 .. 2^24");
  attn_paged_shape(B, Hq, Hkv, page, 1, 1, workgroups);  // page before it divides
  const int rule[4] = {L, 1, std::max(32, L / 2) / 32 * 32, std::max(1, L / page) * page + 1};
  std::vector<int> lens(B);
  for (int b = 0; b < B; ++b) lens[b] = rule[b % 4];
  const detail::AttnPagedCase c(B, Hq, Hkv, page, lens, workgroups, device);

  std::vector<float> q(c.nq()), k(c.nkv()), v(c.nkv()), want(c.nq()), got(c.nq());
  auto decode = [&] {
    const std::vector<float> kpool = c.pool(k.data(), NAN, 1e30f, kAttnChunk);
    const std::vector<float> vpool = c.pool(v.data(), NAN, 1e30f, kAttnChunk);
    attn_paged_decode(q.data(), kpool.data(), vpool.data(), c.table.data(), lens.data(),
                      got.data(), B, Hq, Hkv, page, c.W, c.P, detail::attn_default_scale(),
                      workgroups, device);
  };
  AttnCheck r;
  attn_check_pattern(q.data(), k.data(), v.data(), want.data(), B, Hq, Hkv, c.Lmax,
                     lens.data());
  decode();
  r.max_err = detail::attn_max_err(got.data(), want.data(), c.nq());

  for (size_t i = 0; i < c.nq(); ++i) q[i] = detail::attn_dense(1, i, 256);
  for (size_t i = 0; i < c.nkv(); ++i) {
    k[i] = detail::attn_dense(2, i, 64);
    v[i] = detail::attn_dense(3, i, 64);
  }
  decode();
  r.max_rel = c.rel_error(got.data(), q.data(), k.data(), v.data());
  return r;
}

// Timed run on the selection pattern: W = ceil(L / page) pages per sequence
// under a fixed scrambled table over a pool of B W + 3 pages, filled on the
// device through the table; one warm-up launch, `iters` launches (plan + decode
// + combine) between events, then 16 spread (b, h) rows are checked exactly.
// KV bytes are sum_b lens[b] Hkv 128 2 2 per launch. `ragged` takes the lengths
// of detail::attn_paged_lens. `contiguous` (L a multiple of `page`) times the
// contiguous kernel of payload_attn.hpp on the same lengths and data instead,
// for comparison: its cache is filled by the same kernel without a table.
inline AttnPagedResult run_attn_paged(int B = 32, int Hq = 64, int Hkv = 8, int L = 4096,
                                      int page = 64, int iters = 10, bool ragged = false,
                                      int workgroups = 0, int device = 0,
                                      bool contiguous = false) {
  using C = AttnCacheBf16;
  const detail::AttnPagedTimed t("run_attn_paged", attn_paged_shape, B, Hq, Hkv, L, page,
                                 iters, ragged, workgroups);
  const float scale = detail::attn_default_scale();
  const size_t groups = static_cast<size_t>(B) * Hkv * t.W * page * kAttnD / C::kLane;
  auto fill = [&](auto& p, const int* table, int shift) {
    hipLaunchKernelGGL(attn_paged_fill_kernel, dim3(grid_for(groups)), dim3(kBlock), 0, 0,
                       p.dk.template as<uint16_t>(), p.dvt.template as<uint16_t>(), table,
                       p.dlens.template as<const int>(), Hkv, t.W, shift, groups);
  };
  AttnPagedResult r;
  if (contiguous) {
    if (L % page != 0)
      throw std::invalid_argument("run_attn_paged: contiguous needs L % page == 0");
    detail::AttnProblem c(B, Hq, Hkv, L, 0, device);
    c.alloc();
    c.upload_q_lens(t.q.data(), t.lens.data());
    fill(c, nullptr, __builtin_ctz(page / kAttnChunk));
    HIP_CHECK(hipGetLastError());
    t.report(r, detail::time_launches(iters, [&c, scale] { c.launch(scale); }),
             c.dout.as<float>(), 2 * sizeof(C::Elem));
    r.items = B * c.splits;
    return r;
  }
  detail::AttnPagedBf16Problem p(B, Hq, Hkv, page, t.W, t.P, workgroups, device);
  const float ms = t.time(
      r, p, [&] { fill(p, p.dtable.as<const int>(), p.shift()); },
      [&p, scale] { p.launch(scale); });
  t.report(r, ms, p.dout.as<float>(), 2 * sizeof(C::Elem));
  return r;
}

}  // namespace payload
