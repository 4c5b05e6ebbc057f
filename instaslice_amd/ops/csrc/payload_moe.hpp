// gfx950 routed mixture-of-experts grouped GEMM payload.
//
// The GEMM payloads prove the dense matrix paths. This one proves the path a
// mixture-of-experts model spends its weights and FLOPs on: rows chosen at run
// time by an index tensor, a ragged M extent per expert that only the device
// knows, tiles scheduled from a table a kernel wrote a moment earlier, and
// results that go back through a permutation and are reduced over the top-k
// experts of a token.
//
//   y[t, :] = sum over j < topk of gates[t, j] * (bf16(x[t, :]) · bf16(w[ids[t, j], :, :]))
//
// x (T, K), w (E, K, N), ids (T, topk) with a token's experts all different,
// gates (T, topk) fp32 or absent (all ones), y (T, N) fp32. S = T * topk slots,
// slot s = t * topk + j. A launch is five kernels on the null stream:
//
//   moe_count_kernel    ids -> counts[e]: an LDS histogram per workgroup, then
//                       one global integer atomic per (workgroup, expert seen)
//   moe_scan_kernel     one workgroup: the exclusive scan of the counts is
//                       seg[0..E], the scatter's cursors start there, and every
//                       expert's run of sorted rows is cut into tiles of BM rows
//                       {expert, first row, row count}; an empty expert gets no
//                       tile. It clears counts for the next launch, so a launch
//                       resets what it needs itself.
//   moe_scatter_kernel  ids -> perm[sorted row] = slot: per pass of 256 slots a
//                       workgroup ranks its slots in an LDS histogram, reserves
//                       a range per expert with one global atomic on the cursor
//                       and writes its slots there. The order inside an
//                       expert's run depends on atomic order; the result does
//                       not, a row's dot product does not involve its
//                       neighbours.
//   moe_gemm_kernel<BM> grid (Np / 128, floor(S / BM) + min(E, S)): the bound
//                       on the tile count for any routing; workgroups at or
//                       beyond the real count leave on a block-uniform test.
//   moe_combine_kernel  y[t] = ys[t*topk] + ... + ys[t*topk + topk - 1], added
//                       in that order in fp32, 16-byte accesses, grid-strided
//
// moe_gemm_kernel<BM>, one template and two geometries:
//
//   BM = 128     prefill-shaped, many rows per expert: the bf16 GEMM kernel's
//                geometry. 128 x 128 block tile, K-step 64, 4 wave64s as 2 x 2,
//                each 64 x 64 = 4 x 4 MFMA tiles of v_mfma_f32_16x16x32_bf16.
//   BM = 32      decode-shaped, a handful of rows per expert, bound by
//                streaming the weights: 32 x 128 block tile, the four waves side
//                by side along N, each 32 x 32 = 2 x 2 MFMA tiles. A tile pads
//                at most 31 rows instead of 127.
//   A side       a gather. Each staging thread resolves its BM / 32 rows once,
//                before the K loop: sorted row -> perm -> slot / topk = token ->
//                a pointer into the bf16 image of x, and streams 16-byte
//                fragments from it. A row past the end of the expert's run
//                points at a zero row appended to x (token T), by a select, not
//                a branch; perm is padded by 128 entries so that reading it
//                needs no branch either.
//   B side       the expert's image in [E][Np][Kp] bf16 (transposed and
//                zero-padded as GemmProblem stores bt), base chosen from the
//                tile table.
//   staging      gemm_bf16_kernel's: registers -> ds_write_b128 into the
//                swizzled image of gemm_lds_off, the next K-step's global loads
//                issued before the current step's MFMAs. No edge branch in K.
//   MFMA         issued with the operands swapped, mfma(B fragment, A
//                fragment): the instruction's two operand maps are alike, so
//                this yields the transposed tile, and lane l holds row l & 15
//                and the four consecutive columns 4 (l >> 4) .. + 3 of it.
//   epilogue     per lane and MFMA tile row: sorted row -> perm -> slot, the
//                slot's gate, gate * acc in fp32 (one rounding), one 16-byte
//                store of four columns into ys[slot]. Rows past the run are not
//                stored; no row is stored by two tiles.
//
// The result is the same bits on every run: each ys row is one tile's work
// whatever its place in the run, and the combine adds in a fixed order.
//
// Limits, checked on the host before anything is launched
// (std::invalid_argument): T, N, K >= 1; 1 <= E <= 256; 1 <= topk <= min(E, 8);
// every id in [0, E) and no expert twice in a token; gates, x and w finite;
// bm 0 (the host's choice: 32 when S / E <= 32, else 128), 32 or 128. Sizes:
// every element offset in the kernels is a size_t, so what bounds the shape is
// what travels as an int or a grid dimension: floor(S / bm) + min(E, S) <=
// 65535 (grid.y; it also keeps S + 128, the padded perm, far below 2^31), Np
// <= 0x7FFFFF80 and Kp <= 0x7FFFFFC0 as in GemmShape.
//
// Included by payload_core.hpp after payload_gemm.hpp (needs bf16x8, f32x4,
// gemm_lds_off, to_bf16_rne, detail::round_up, detail::note_err and
// require_exact_k, and payload_core.hpp's DeviceBuffer and time_launches).

#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>

namespace payload {

constexpr int kMoeMaxExperts = 256;
constexpr int kMoeMaxTopk = 8;
constexpr int kMoePermPad = 128;  // the larger BM: a tile's perm reads stay inside

static_assert(kMoeMaxExperts == kBlock, "one routing thread per expert");

// No packed fp32 arithmetic in these kernels: the gate product and the combine
// are plain v_mul_f32 / v_add_f32, one rounding each.
#if defined(__HIP_DEVICE_COMPILE__)  // the host pass does not know the feature
#define MOE_KERNEL __global__ __launch_bounds__(kBlock) \
    __attribute__((target("no-packed-fp32-ops")))
#else
#define MOE_KERNEL __global__ __launch_bounds__(kBlock)
#endif

// ---- routing kernels -----------------------------------------------------

// counts[e] += slots of ids that name e. counts: 256 ints, zero on entry.
MOE_KERNEL void moe_count_kernel(const int* __restrict__ ids, int S,
                                 int* __restrict__ counts) {
  __shared__ int hist[kMoeMaxExperts];
  hist[threadIdx.x] = 0;
  __syncthreads();
  const size_t stride = static_cast<size_t>(gridDim.x) * kBlock;
  for (size_t s = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
       s < static_cast<size_t>(S); s += stride)
    atomicAdd(&hist[ids[s]], 1);
  __syncthreads();
  const int c = hist[threadIdx.x];
  if (c) atomicAdd(&counts[threadIdx.x], c);
}

// One workgroup, thread e for expert e. seg: E + 1 ints, cursor: 256 ints,
// tiles: floor(S / bm) + min(E, S) entries {expert, first sorted row, rows, 0}.
// Sets counts back to zero.
MOE_KERNEL void moe_scan_kernel(int* __restrict__ counts, int E, int bm,
                                int* __restrict__ seg, int* __restrict__ cursor,
                                int4* __restrict__ tiles, int* __restrict__ ntiles) {
  __shared__ int rows[kMoeMaxExperts], tl[kMoeMaxExperts];
  const int e = threadIdx.x;
  const int c = counts[e];  // zero at and beyond E
  counts[e] = 0;
  const int nt = (c + bm - 1) / bm;
  rows[e] = c;
  tl[e] = nt;
  __syncthreads();
  for (int d = 1; d < kMoeMaxExperts; d <<= 1) {  // inclusive scans
    const int r = e >= d ? rows[e - d] : 0;
    const int t = e >= d ? tl[e - d] : 0;
    __syncthreads();
    rows[e] += r;
    tl[e] += t;
    __syncthreads();
  }
  const int start = rows[e] - c;
  if (e < E) {
    seg[e] = start;
    cursor[e] = start;
  }
  if (e == E - 1) seg[E] = rows[e];
  if (e == kMoeMaxExperts - 1) *ntiles = tl[e];
  const int tbase = tl[e] - nt;
  for (int i = 0; i < nt; ++i)
    tiles[tbase + i] = make_int4(e, start + i * bm, min(bm, c - i * bm), 0);
}

// perm[sorted row] = slot. cursor[e] is seg[e] on entry and seg[e + 1] on exit.
MOE_KERNEL void moe_scatter_kernel(const int* __restrict__ ids, int S,
                                   int* __restrict__ cursor, int* __restrict__ perm) {
  __shared__ int hist[kMoeMaxExperts], base[kMoeMaxExperts];
  const int tid = threadIdx.x;
  const size_t stride = static_cast<size_t>(gridDim.x) * kBlock;
  // block-uniform loop: one pass places 256 consecutive slots
  for (size_t s0 = static_cast<size_t>(blockIdx.x) * kBlock;
       s0 < static_cast<size_t>(S); s0 += stride) {
    hist[tid] = 0;
    __syncthreads();
    const size_t s = s0 + tid;
    const bool live = s < static_cast<size_t>(S);
    int e = 0, rank = 0;
    if (live) {
      e = ids[s];
      rank = atomicAdd(&hist[e], 1);
    }
    __syncthreads();
    const int c = hist[tid];
    if (c) base[tid] = atomicAdd(&cursor[tid], c);
    __syncthreads();
    if (live) perm[base[e] + rank] = static_cast<int>(s);
    __syncthreads();  // base and hist are rewritten by the next pass
  }
}

// ---- the grouped GEMM ----------------------------------------------------

// x: (T + 1) x Kp bf16, row T zero. w: E x Np x Kp bf16. perm: S + 128 ints,
// the last 128 equal to S. gates: S + 1 floats. ys: S x Np floats.
// grid = (Np / 128, floor(S / BM) + min(E, S)).
template <int BM>
MOE_KERNEL void moe_gemm_kernel(
    const uint16_t* __restrict__ x, const uint16_t* __restrict__ w,
    const int* __restrict__ perm, const float* __restrict__ gates,
    const int4* __restrict__ tiles, const int* __restrict__ ntiles,
    float* __restrict__ ys, int T, int topk, int Np, int Kp) {
  static_assert(BM == 32 || BM == 128, "two geometries");
  constexpr int kLoadsA = BM * kGemmSlots / kBlock;  // 4 or 1
  constexpr int kWT = BM == 128 ? 4 : 2;             // MFMA tiles per wave, each way
  static_assert(BM <= kMoePermPad, "perm's padding covers a tile");

  if (static_cast<int>(blockIdx.y) >= *ntiles) return;  // block-uniform
  const int4 tile = tiles[blockIdx.y];
  const int expert = tile.x, row0 = tile.y, rows = tile.z;

  __shared__ __attribute__((aligned(16))) uint16_t lds[(BM + kGemmBN) * kGemmBK];
  uint16_t* lds_a = lds;
  uint16_t* lds_b = lds + BM * kGemmBK;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  // the wave's corner in the block tile: 2 x 2 quadrants, or side by side
  const int wrow = BM == 128 ? (wave >> 1) * 64 : 0;
  const int wcol = BM == 128 ? (wave & 1) * 64 : wave * 32;
  const int fr = lane & 15, fq = lane >> 4;

  // staging map: 8 consecutive lanes cover one 128-byte row of the K-step
  const int srow = tid >> 3, sslot = tid & 7;
  const size_t bcol = static_cast<size_t>(blockIdx.x) * kGemmBN;
  const uint16_t* ga[kLoadsA];
#pragma unroll
  for (int i = 0; i < kLoadsA; ++i) {
    const int r = srow + i * (kBlock / kGemmSlots);
    const int slot = perm[row0 + r];  // padded: in bounds for every r < BM
    const int tok = r < rows ? slot / topk : T;
    ga[i] = x + static_cast<size_t>(tok) * Kp + sslot * 8;
  }
  const uint16_t* gb =
      w + (static_cast<size_t>(expert) * Np + bcol + srow) * Kp + sslot * 8;
  const size_t pass = static_cast<size_t>(kBlock / kGemmSlots) * Kp;  // 32 rows

  bf16x8 ra[kLoadsA], rb[kGemmLoads];
#pragma unroll
  for (int i = 0; i < kLoadsA; ++i) ra[i] = *reinterpret_cast<const bf16x8*>(ga[i]);
#pragma unroll
  for (int i = 0; i < kGemmLoads; ++i)
    rb[i] = *reinterpret_cast<const bf16x8*>(gb + i * pass);

  f32x4 acc[kWT][kWT];
#pragma unroll
  for (int m = 0; m < kWT; ++m)
#pragma unroll
    for (int n = 0; n < kWT; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int k0 = 0; k0 < Kp; k0 += kGemmBK) {
#pragma unroll
    for (int i = 0; i < kLoadsA; ++i)
      *reinterpret_cast<bf16x8*>(
          lds_a + gemm_lds_off(srow + i * (kBlock / kGemmSlots), sslot)) = ra[i];
#pragma unroll
    for (int i = 0; i < kGemmLoads; ++i)
      *reinterpret_cast<bf16x8*>(
          lds_b + gemm_lds_off(srow + i * (kBlock / kGemmSlots), sslot)) = rb[i];
    __syncthreads();

    if (k0 + kGemmBK < Kp) {  // block-uniform: prefetch the next K-step
#pragma unroll
      for (int i = 0; i < kLoadsA; ++i)
        ra[i] = *reinterpret_cast<const bf16x8*>(ga[i] + k0 + kGemmBK);
#pragma unroll
      for (int i = 0; i < kGemmLoads; ++i)
        rb[i] = *reinterpret_cast<const bf16x8*>(gb + k0 + kGemmBK + i * pass);
    }

#pragma unroll
    for (int kk = 0; kk < kGemmBK / 32; ++kk) {
      bf16x8 fa[kWT], fb[kWT];
#pragma unroll
      for (int m = 0; m < kWT; ++m)
        fa[m] = *reinterpret_cast<const bf16x8*>(
            lds_a + gemm_lds_off(wrow + m * 16 + fr, kk * 4 + fq));
#pragma unroll
      for (int n = 0; n < kWT; ++n)
        fb[n] = *reinterpret_cast<const bf16x8*>(
            lds_b + gemm_lds_off(wcol + n * 16 + fr, kk * 4 + fq));
      // operands swapped: the tile comes out transposed (see the epilogue)
#pragma unroll
      for (int m = 0; m < kWT; ++m)
#pragma unroll
        for (int n = 0; n < kWT; ++n)
          acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[n], fa[m],
                                                              acc[m][n], 0, 0, 0);
    }
    __syncthreads();  // all fragment reads done before the next ds_write
  }

  // transposed C/D map: tile row = lane & 15, tile col = (lane >> 4) * 4 + reg
#pragma unroll
  for (int m = 0; m < kWT; ++m) {
    const int r = wrow + m * 16 + fr;
    const int slot = perm[row0 + r];
    const float g = gates[slot];  // slot <= S: in bounds for a padding row too
    if (r < rows) {
      float* out = ys + static_cast<size_t>(slot) * Np + bcol + wcol + fq * 4;
#pragma unroll
      for (int n = 0; n < kWT; ++n) {
        f32x4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = g * acc[m][n][j];
        *reinterpret_cast<f32x4*>(out + n * 16) = v;
      }
    }
  }
}

// y, ys as f32x4; np4 = Np / 4; n4 = T * np4 outputs
MOE_KERNEL void moe_combine_kernel(const f32x4* __restrict__ ys, f32x4* __restrict__ y,
                                   size_t n4, size_t np4, int topk) {
  const size_t stride = static_cast<size_t>(gridDim.x) * kBlock;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x; i < n4;
       i += stride) {
    const size_t t = i / np4, c = i - t * np4;
    const f32x4* p = ys + t * topk * np4 + c;
    f32x4 a = p[0];
    for (int j = 1; j < topk; ++j) {
      const f32x4 b = p[j * np4];
#pragma unroll
      for (int q = 0; q < 4; ++q) a[q] = a[q] + b[q];
    }
    y[i] = a;
  }
}

#undef MOE_KERNEL

// ---- host layer ----------------------------------------------------------

struct MoeResult {
  double tflops = 0;        // 2 S N K per launch
  double tokens_per_s = 0;  // T per launch
  double max_err = 0;
  int bm = 0;               // the variant that ran
};

namespace detail {

// The routing of a problem: the checked ids, the buffers the routing kernels
// write, and their launch. bm is the tile height the tile table is cut for.
struct MoeRouting {
  int T, E, topk, bm;
  size_t S;
  int max_tiles;
  std::vector<int> ids;  // S
  DeviceBuffer dids, dcounts, dcursor, dseg, dperm, dtiles, dntiles;

  MoeRouting(const std::string& who, int t, int e, int tk, int bm_) : T(t), E(e), topk(tk) {
    if (t < 1) throw std::invalid_argument(who + ": T must be >= 1");
    if (e < 1 || e > kMoeMaxExperts)
      throw std::invalid_argument(who + ": experts must be in 1 .. 256");
    if (tk < 1 || tk > std::min(e, kMoeMaxTopk))
      throw std::invalid_argument(who + ": topk must be in 1 .. min(experts, 8)");
    if (bm_ != 0 && bm_ != 32 && bm_ != 128)
      throw std::invalid_argument(who + ": bm must be 0, 32 or 128");
    S = static_cast<size_t>(t) * tk;
    bm = bm_ != 0 ? bm_ : (S / e <= 32 ? 32 : 128);
    const size_t tiles = S / bm + std::min<size_t>(e, S);
    if (tiles > 65535) throw std::invalid_argument(who + ": shape too large");
    max_tiles = static_cast<int>(tiles);
  }

  // ids: T x topk, every id in [0, E), a token's ids all different
  void set_ids(const std::string& who, const int* p) {
    for (size_t s = 0; s < S; ++s) {
      if (p[s] < 0 || p[s] >= E)
        throw std::invalid_argument(who + ": an id is outside [0, experts)");
      for (size_t q = s - s % topk; q < s; ++q)
        if (p[q] == p[s])
          throw std::invalid_argument(who + ": an expert twice in one token");
    }
    ids.assign(p, p + S);
  }

  void upload_routing() {
    dids.alloc(S * sizeof(int));
    dcounts.alloc(kMoeMaxExperts * sizeof(int));
    dcursor.alloc(kMoeMaxExperts * sizeof(int));
    dseg.alloc((E + 1) * sizeof(int));
    dperm.alloc((S + kMoePermPad) * sizeof(int));
    dtiles.alloc(max_tiles * sizeof(int4));
    dntiles.alloc(sizeof(int));
    HIP_CHECK(hipMemcpy(dids.p, ids.data(), S * sizeof(int), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemset(dcounts.p, 0, kMoeMaxExperts * sizeof(int)));
    // perm's padding names slot S, whose token is the zero row T
    const std::vector<int> pad(kMoePermPad, static_cast<int>(S));
    HIP_CHECK(hipMemcpy(dperm.as<int>() + S, pad.data(), pad.size() * sizeof(int),
                        hipMemcpyHostToDevice));
  }

  void launch_routing() const {
    const int s = static_cast<int>(S);
    const dim3 grid(static_cast<unsigned>(std::min<size_t>((S + kBlock - 1) / kBlock, 1024)));
    hipLaunchKernelGGL(moe_count_kernel, grid, dim3(kBlock), 0, 0,
                       dids.as<const int>(), s, dcounts.as<int>());
    hipLaunchKernelGGL(moe_scan_kernel, dim3(1), dim3(kBlock), 0, 0, dcounts.as<int>(),
                       E, bm, dseg.as<int>(), dcursor.as<int>(), dtiles.as<int4>(),
                       dntiles.as<int>());
    hipLaunchKernelGGL(moe_scatter_kernel, grid, dim3(kBlock), 0, 0,
                       dids.as<const int>(), s, dcursor.as<int>(), dperm.as<int>());
  }
};

// Padded images on the host plus their device images, in the style of
// GemmProblem: x (T + 1) x Kp with a zero last row, w E x Np x Kp (each
// expert transposed, K-contiguous), gates S + 1.
struct MoeProblem : MoeRouting {
  int N, K;
  size_t Np, Kp;
  std::vector<uint16_t> x, w;
  std::vector<float> gates;
  DeviceBuffer dx, dw, dgates, dys, dy;

  MoeProblem(const std::string& who, int t, int n, int k, int e, int tk, int bm_)
      : MoeRouting(who, t, e, tk, bm_), N(n), K(k) {
    if (n < 1 || k < 1) throw std::invalid_argument(who + ": N and K must be >= 1");
    Np = round_up(n, kGemmBN);
    Kp = round_up(k, kGemmBK);
    if (Np > 0x7FFFFF80u || Kp > 0x7FFFFFC0u)
      throw std::invalid_argument(who + ": shape too large");
    x.assign((static_cast<size_t>(T) + 1) * Kp, 0);
    w.assign(static_cast<size_t>(E) * Np * Kp, 0);
    gates.assign(S + 1, 1.0f);
    gates[S] = 0.0f;
  }

  uint16_t& x_at(int t, int k) { return x[static_cast<size_t>(t) * Kp + k]; }
  uint16_t& w_at(int e, int k, int c) {
    return w[(static_cast<size_t>(e) * Np + c) * Kp + k];
  }

  void upload(int device) {
    HIP_CHECK(hipSetDevice(device));
    upload_routing();
    dx.alloc(x.size() * sizeof(uint16_t));
    dw.alloc(w.size() * sizeof(uint16_t));
    dgates.alloc(gates.size() * sizeof(float));
    dys.alloc(S * Np * sizeof(float));
    dy.alloc(static_cast<size_t>(T) * Np * sizeof(float));
    HIP_CHECK(hipMemcpy(dx.p, x.data(), x.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dw.p, w.data(), w.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dgates.p, gates.data(), gates.size() * sizeof(float),
                        hipMemcpyHostToDevice));
  }

  // the whole path: route, grouped GEMM, combine
  void launch() const {
    launch_routing();
    const dim3 grid(static_cast<unsigned>(Np / kGemmBN), static_cast<unsigned>(max_tiles));
    auto kernel = bm == 32 ? moe_gemm_kernel<32> : moe_gemm_kernel<128>;
    hipLaunchKernelGGL(kernel, grid, dim3(kBlock), 0, 0, dx.as<const uint16_t>(),
                       dw.as<const uint16_t>(), dperm.as<const int>(),
                       dgates.as<const float>(), dtiles.as<const int4>(),
                       dntiles.as<const int>(), dys.as<float>(), T, topk,
                       static_cast<int>(Np), static_cast<int>(Kp));
    const size_t np4 = Np / 4, n4 = static_cast<size_t>(T) * np4;
    hipLaunchKernelGGL(moe_combine_kernel, dim3(grid_for(n4)), dim3(kBlock), 0, 0,
                       dys.as<const f32x4>(), dy.as<f32x4>(), n4, np4, topk);
  }

  // the un-padded T x N region, row-major
  void download(float* y) const {
    HIP_CHECK(hipMemcpy2D(y, static_cast<size_t>(N) * sizeof(float), dy.p,
                          Np * sizeof(float), static_cast<size_t>(N) * sizeof(float), T,
                          hipMemcpyDeviceToHost));
  }
};

// The self-check pattern. x is gemm_pat_a; w has the expert in the formula.
inline int moe_pat_w(int e, int k, int c) {
  return static_cast<int>((7ll * k + 11ll * c + 5ll * e) % 9) - 4;
}
// gate = moe_pat_gate4 / 4, one of 0.25, 0.5, 1, 2
inline int moe_pat_gate4(int t, int j) { return 1 << ((t + 3 * j) % 4); }
// Routing: where topk < E and E >= 4, expert E / 2 gets no token. Every third
// token goes to the first topk of the others, so those carry more rows.
inline int moe_pat_id(int t, int j, int E, int topk) {
  const bool hole = E >= 4 && topk < E;
  const int active = hole ? E - 1 : E;
  const int first = t % 3 == 0 ? 0 : static_cast<int>(7ll * t % active);
  const int a = (first + j) % active;
  return hole && a >= E / 2 ? a + 1 : a;
}

inline void fill_moe_pattern(MoeProblem& p) {
  uint16_t code[9];
  for (int v = -4; v <= 4; ++v) code[v + 4] = to_bf16_rne(static_cast<float>(v));
  for (int t = 0; t < p.T; ++t)
    for (int k = 0; k < p.K; ++k) p.x_at(t, k) = code[gemm_pat_a(t, k) + 4];
  for (int e = 0; e < p.E; ++e)
    for (int c = 0; c < p.N; ++c)
      for (int k = 0; k < p.K; ++k) p.w_at(e, k, c) = code[moe_pat_w(e, k, c) + 4];
  std::vector<int> ids(p.S);
  for (int t = 0; t < p.T; ++t)
    for (int j = 0; j < p.topk; ++j) {
      ids[static_cast<size_t>(t) * p.topk + j] = moe_pat_id(t, j, p.E, p.topk);
      p.gates[static_cast<size_t>(t) * p.topk + j] = 0.25f * moe_pat_gate4(t, j);
    }
  p.set_ids("moe", ids.data());
}

// |got - exact| of output (t, c) of the pattern: int64, the gates as integers
// over 4
inline double moe_pattern_err(float got, int t, int c, const MoeProblem& p) {
  int64_t s4 = 0;
  for (int j = 0; j < p.topk; ++j) {
    const int e = moe_pat_id(t, j, p.E, p.topk);
    int64_t dot = 0;
    for (int k = 0; k < p.K; ++k)
      dot += static_cast<int64_t>(gemm_pat_a(t, k)) * moe_pat_w(e, k, c);
    s4 += moe_pat_gate4(t, j) * dot;
  }
  return std::fabs(static_cast<double>(got) - static_cast<double>(s4) / 4.0);
}

}  // namespace detail

// General entry: y (T, N) of the operation at the top of this file. x (T, K),
// w (E, K, N), ids (T, topk), gates (T, topk) or null for all ones, all
// row-major. bm: 0 for the host's choice, or 32 or 128. Throws
// std::invalid_argument on any of the limits above, before any device work.
inline void moe_gemm(const float* x, const float* w, const int* ids, const float* gates,
                     float* y, int T, int N, int K, int E, int topk, int bm,
                     int device = 0) {
  detail::MoeProblem p("moe_gemm", T, N, K, E, topk, bm);
  p.set_ids("moe_gemm", ids);
  if (gates)
    for (size_t s = 0; s < p.S; ++s) {
      if (!std::isfinite(gates[s]))
        throw std::invalid_argument("moe_gemm: gates has a non-finite element");
      p.gates[s] = gates[s];
    }
  for (int t = 0; t < T; ++t)
    for (int k = 0; k < K; ++k) {
      const float v = x[static_cast<size_t>(t) * K + k];
      if (!std::isfinite(v))
        throw std::invalid_argument("moe_gemm: x has a non-finite element");
      p.x_at(t, k) = to_bf16_rne(v);
    }
  for (int e = 0; e < E; ++e)
    for (int k = 0; k < K; ++k)
      for (int c = 0; c < N; ++c) {
        const float v = w[(static_cast<size_t>(e) * K + k) * N + c];
        if (!std::isfinite(v))
          throw std::invalid_argument("moe_gemm: w has a non-finite element");
        p.w_at(e, k, c) = to_bf16_rne(v);
      }
  p.upload(device);
  p.launch();
  HIP_CHECK(hipGetLastError());
  p.download(y);
}

// The routing kernels alone: perm[0..S) (the slot at each sorted row) and
// seg[0..E] (the start of each expert's run). The same argument checks.
inline void moe_route(const int* ids, int T, int topk, int E, int* perm, int* seg,
                      int device = 0) {
  detail::MoeRouting r("moe_route", T, E, topk, 0);
  r.set_ids("moe_route", ids);
  HIP_CHECK(hipSetDevice(device));
  r.upload_routing();
  r.launch_routing();
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpy(perm, r.dperm.p, r.S * sizeof(int), hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(seg, r.dseg.p, (E + 1) * sizeof(int), hipMemcpyDeviceToHost));
}

// Self-contained exact check: integer x and w in [-4, 4], gates from {0.25,
// 0.5, 1, 2}, a routing with an empty expert; host reference in int64. Returns
// max |y - ref| over the whole T x N result (expect 0.0). K <= 1024: up to
// there every partial sum times 4 is an integer below 2^24, exact in fp32 in
// any order.
inline double run_moe_check(int T, int N, int K, int E, int topk, int bm = 0,
                            int device = 0) {
  detail::require_exact_k(K, "run_moe_check");
  detail::MoeProblem p("run_moe_check", T, N, K, E, topk, bm);
  detail::fill_moe_pattern(p);
  std::vector<float> host(static_cast<size_t>(T) * N);
  p.upload(device);
  p.launch();
  HIP_CHECK(hipGetLastError());
  p.download(host.data());
  double max_err = 0;
  for (int t = 0; t < T; ++t)
    for (int c = 0; c < N; ++c)
      detail::note_err(max_err,
                       detail::moe_pattern_err(host[static_cast<size_t>(t) * N + c], t, c, p));
  return max_err;
}

// Timed run on the same pattern: one warm-up launch, `iters` launches of the
// whole path (route, GEMM, combine) between events, then 256 fixed, spread
// outputs are checked exactly, so a fast wrong kernel cannot report a rate.
inline MoeResult run_moe(int T = 8192, int N = 4096, int K = 1024, int E = 32,
                         int topk = 4, int iters = 10, int bm = 0, int device = 0) {
  detail::require_exact_k(K, "run_moe");
  if (iters < 1) throw std::invalid_argument("run_moe: iters must be >= 1");
  detail::MoeProblem p("run_moe", T, N, K, E, topk, bm);
  detail::fill_moe_pattern(p);
  p.upload(device);
  const float ms = detail::time_launches(iters, [&p] { p.launch(); });
  MoeResult r;
  r.bm = p.bm;
  r.tflops = 2.0 * p.S * N * K * iters / (ms * 1e-3) / 1e12;
  r.tokens_per_s = static_cast<double>(T) * iters / (ms * 1e-3);
  for (int i = 0; i < 256; ++i) {
    const int t = static_cast<int>((static_cast<int64_t>(i) * 1031 + 17) % T);
    const int c = static_cast<int>((static_cast<int64_t>(i) * 2053 + 29) % N);
    float got = 0;
    HIP_CHECK(hipMemcpy(&got, p.dy.as<float>() + static_cast<size_t>(t) * p.Np + c,
                        sizeof(float), hipMemcpyDeviceToHost));
    detail::note_err(r.max_err, detail::moe_pattern_err(got, t, c, p));
  }
  return r;
}

}  // namespace payload
