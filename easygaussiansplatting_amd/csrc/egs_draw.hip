// The per-tile alpha-blend kernels for gfx950 (CDNA4, wave64): k_draw (reference gsplatcu/kernel.cu:152-271) and
// k_draw_bwd (kernel.cu:809-950), the dispatch order of their tiles (k_tile_order) and the launchers that pick the
// template instance of a raster policy.  One wave64 per 16x16 tile; see egs_raster.h for how this differs from the
// reference by design.  k_draw's blend loop is blend_range of egs_draw_device.h, which k_draw_seg (egs_segments.hip)
// calls too; k_draw_bwd keeps its own staging (it stages the records as they are).
#include "egs_draw_device.h"

namespace egs {

// Longest-list-first dispatch order of the tiles for the two draw kernels.  A tile is one wave whose run
// time is proportional to its list length (0 ... ~2x the mean on the 1 M scene); workgroups are handed to
// the SIMDs in index order, so with tiles in IMAGE order a launch ends with whichever SIMD drew the longest
// lists while the others idle.  Sorted by length (descending) the long tiles start first and the short ones
// fill the gaps (LPT scheduling).  (Tried: the sorted order dealt out in a serpentine over the SIMDs, and sorted
// per XCD with tile row % 8 kept on one XCD, with and without the serpentine -- none faster, DESIGN 3.3, docs/LAB.md.)
// One workgroup: counting sort on the length in LDS -- 8160 tiles take a few microseconds.
constexpr int TO_BINS = 1024;
constexpr int TO_REGS = 16;    // tiles per thread whose (bin, rank) stay in registers between the two passes
constexpr int TO_TAIL = 24;    // ... and parked in the order buffer itself: (TO_REGS + TO_TAIL) * 1024 = 40960 tiles (4K: 32400)
// sort key of tile t: its list length, or -- `work` given -- the work the forward draw kernel measured for it
__device__ __forceinline__ int tile_len(const int32_t* __restrict__ ranges, const int32_t* __restrict__ work, int t) {
  if (work) return work[t];
  const int2 r = reinterpret_cast<const int2*>(ranges)[t];
  return r.y - r.x;
}
__global__ __launch_bounds__(1024) void k_tile_order(const int32_t* __restrict__ ranges,
                                                     const int32_t* __restrict__ work, int T,
                                                     int32_t* __restrict__ order,
                                                     const int32_t* __restrict__ walk = nullptr,
                                                     uint32_t* __restrict__ hint = nullptr) {
  // walk / hint (nullable): hint[1] receives the longest WALK of the camera's previous render (walk[T], next to its work),
  // hint[0] the longest list when the tiles are sorted by length -- page-locked words the host steers by (fused.py: long
  // walks take the segment path)
  // ONE LDS atomic per tile: the returning add that counts a bin also hands the tile its rank inside the bin
  // (arrival order -- any order inside a bin will do); after the scan of the bins its slot is start + rank.
  // LDS atomics retire about one lane per clock whatever the conflicts, so the kernel costs ~T cycles per pass:
  // the first version's two passes took 9 us at 1080p and 45 us at 4K (32400 tiles).
  constexpr int NB = 8 * TO_BINS;
  __shared__ uint32_t bins[NB];
  __shared__ uint32_t wsum[16];
  const int tid = threadIdx.x;
  const int shift = work ? 2 : 0;   // key -> bin: list lengths 1:1; the forward kernel's work measure is ~6x a length
  int lenr[TO_REGS];     // all loads in flight at once: the kernel is a chain of latencies, not of bytes
#pragma unroll
  for (int r = 0; r < TO_REGS; ++r) {
    const int t = tid + r * 1024;
    lenr[r] = t < T ? tile_len(ranges, work, t) : 0;
  }
  for (int i = tid; i < NB; i += 1024) bins[i] = 0u;
  if (hint) {
    int mx = 0;
    if (walk) { for (int t = tid; t < T; t += 1024) mx = max(mx, walk[t]); }
    else if (!work) {
#pragma unroll
      for (int r = 0; r < TO_REGS; ++r) mx = max(mx, lenr[r]);
      for (int t = tid + TO_REGS * 1024; t < T; t += 1024) mx = max(mx, tile_len(ranges, work, t));
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mx = max(mx, __shfl_xor(mx, d, 64));
    if ((tid & 63) == 0) wsum[tid >> 6] = (uint32_t)mx;
  }
  __syncthreads();
  if (hint && tid == 0 && (walk || !work)) {
    uint32_t mx = 0u;
    for (int w = 0; w < 16; ++w) mx = max(mx, wsum[w]);
    hint[walk ? 1 : 0] = mx;
  }
  __syncthreads();
  auto key_of = [&](int len) { return NB - 1 - min(max(len, 0) >> shift, NB - 1); };   // longest first
  // pass 1: (bin, rank) per tile, packed 13 + 19 bits (T < 2^19: checked by the host)
  uint32_t kr[TO_REGS];
#pragma unroll
  for (int r = 0; r < TO_REGS; ++r) {
    const int t = tid + r * 1024;
    kr[r] = 0u;
    if (t < T) {
      const int key = key_of(lenr[r]);
      kr[r] = ((uint32_t)key << 19) | atomicAdd(&bins[key], 1u);
    }
  }
  // (tiles beyond TO_REGS * 1024 keep their (bin, rank) in the order buffer itself until pass 2)
  for (int t = tid + TO_REGS * 1024; t < T; t += 1024) {
    const int key = key_of(tile_len(ranges, work, t));
    order[t] = (int32_t)(((uint32_t)key << 19) | atomicAdd(&bins[key], 1u));
  }
  __syncthreads();
  {  // exclusive scan of the 8192 bins: thread t owns bins [8 t, 8 t + 8)
    uint32_t v[8], s = 0u;
#pragma unroll
    for (int k = 0; k < 8; ++k) { v[k] = bins[8 * tid + k]; s += v[k]; }
    const uint32_t inc = wave_inclusive_scan(s);
    if ((tid & 63) == 63) wsum[tid >> 6] = inc;
    __syncthreads();
    uint32_t pre = 0u;
    for (int w = 0; w < (tid >> 6); ++w) pre += wsum[w];
    uint32_t ex = pre + inc - s;
#pragma unroll
    for (int k = 0; k < 8; ++k) { bins[8 * tid + k] = ex; ex += v[k]; }
  }
  __syncthreads();
  // start of the bin + rank inside it: a permutation of [0, T)
  auto slot_of = [&](uint32_t packed) { return (int)(bins[packed >> 19] + (packed & 0x7FFFFu)); };
  // pass 2 for the tiles parked in the order buffer: read them ALL before any slot is written (a slot may be
  // another tile's parking place)
  uint32_t tail[TO_TAIL];
#pragma unroll
  for (int u = 0; u < TO_TAIL; ++u) {
    const int t = tid + (TO_REGS + u) * 1024;
    tail[u] = t < T ? (uint32_t)order[t] : 0u;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < TO_REGS; ++r) {
    const int t = tid + r * 1024;
    if (t < T) order[slot_of(kr[r])] = t;
  }
#pragma unroll
  for (int u = 0; u < TO_TAIL; ++u) {
    const int t = tid + (TO_REGS + u) * 1024;
    if (t < T) order[slot_of(tail[u])] = t;
  }
}
static_assert(TILE_ORDER_MAX_T == (TO_REGS + TO_TAIL) * 1024, "what k_tile_order handles");

// The per-tile work measure of k_draw (sum of the four blocks' largest contributor index + twice the tile's)
// rebuilt from the `contrib` image, for a backward pass that was not handed the forward pass's record.
__global__ __launch_bounds__(64) void k_tile_work(int W, int H, int gx, const int32_t* __restrict__ contrib,
                                                  int32_t* __restrict__ work, int32_t* __restrict__ walk = nullptr) {
  const int tile = blockIdx.x, lane = threadIdx.x;
  const int tx0 = (tile % gx) * EGS_TILE, ty0 = (tile / gx) * EGS_TILE;
  int w = 0, wmax = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int px = tx0 + (lane & 7) + 8 * (k & 1), py = ty0 + (lane >> 3) + 8 * (k >> 1);
    int mx = (px < W && py < H) ? contrib[(size_t)py * W + px] : 0;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mx = max(mx, __shfl_xor(mx, d, 64));
    w += mx;
    wmax = max(wmax, mx);
  }
  if (lane == 0) { work[tile] = w + 2 * wmax; if (walk) walk[tile] = wmax; }
}
// ... and the tile's walk alone (its largest contributor index), for a splatB that rebuilds segment states
__global__ __launch_bounds__(64) void k_tile_walk(int W, int H, int gx, const int32_t* __restrict__ contrib,
                                                  int32_t* __restrict__ walk) {
  const int tile = blockIdx.x, lane = threadIdx.x;
  const int tx0 = (tile % gx) * EGS_TILE, ty0 = (tile / gx) * EGS_TILE;
  int mx = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int px = tx0 + (lane & 7) + 8 * (k & 1), py = ty0 + (lane >> 3) + 8 * (k >> 1);
    if (px < W && py < H) mx = max(mx, contrib[(size_t)py * W + px]);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) mx = max(mx, __shfl_xor(mx, d, 64));
  if (lane == 0) walk[tile] = mx;
}

// ============================================================================
// draw: per-tile front-to-back blend                   (reference kernel.cu:152-271)
// ============================================================================
// Workgroup b runs on XCD b % 8 (observed dispatch order; speed only): give each
// XCD a contiguous band of tiles so that its private 4-MiB L2 serves 1/8 of the
// Gaussian records instead of all of them.  Bijective for any T.
__device__ __forceinline__ int xcd_tile(int b, const DrawParams& p) {
  if (p.order) {   // (a caller-held buffer: an index outside the image is treated as padding, never dereferenced)
    if (b >= p.ngrid) return -1;
    const int t = p.order[b];
    return (unsigned)t < (unsigned)p.T ? t : -1;
  }
  if (p.map_mode == 0) return b < p.T ? b : -1;
  const int xcd = b & 7, k = b >> 3;
  if (p.map_mode == 1) {   // (never set: make_draw_params picks 0 or 2)
    if (b >= p.T) return -1;
    const int q = p.T >> 3, r = p.T & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
  }
  // mode 2: tile row ty belongs to XCD ty % 8 (balanced when list lengths vary smoothly
  // over the image, still row-coherent inside one L2); the grid is padded to
  // 8 * ceil(gy/8) * gx blocks and the surplus blocks exit.
  const int ty = xcd + 8 * (k / p.gx), tx = k % p.gx;
  return ty < p.gy ? ty * p.gx + tx : -1;
}
// (Tried: dynamic LDS requested only to cap the resident tile-waves per CU, so that the dispatcher hands the remaining
// tiles to whichever SIMD drains first -- no faster for either draw kernel, docs/LAB.md.)
int draw_grid(const DrawParams& p) {
  if (p.order) return p.ngrid;
  return p.map_mode == 2 ? 8 * div_up(p.gy, 8) * p.gx : p.T;
}

// Policy is compiled in (BOX: pixel-box footprint; FLOOR: max(0,m); CLAMP: min(0.99,.));
// the two thresholds stay runtime scalars (SGPR operands of the compares).
//
// One wave64 per 16x16 tile.  The tile is walked as four 8x8 pixel blocks
// (k = 0..3, block (k&1, k>>1)); lane l owns pixel (l&7, l>>3) of each block.  Per
// list entry a block is skipped outright when the entry's certain-miss box (pack
// kernel) or pixel box does not reach it -- a wave-uniform branch.  The forward kernel
// evaluates the exponent as a polynomial about the tile centre (egs_draw_device.h), the backward kernel
// separably from the differences it also needs for the moments: cxx[bx] + cyy[by] +
// cxy[bx]*dy[by].  (Measured on gfx950,
// tools/ubench_valu.hip: v_pk_*_f32 costs exactly 2x a plain fp32 op, v_exp/v_rcp 3x,
// v_max/v_cmp->SGPR 1.6x -- so the kernels minimise instruction count, not pack.)
// A pixel that is finished or outside the image holds tau < tau_stop, so "still
// blending" is the one compare `tau >= stop`; the wave-uniform 4-bit `live` mask of
// blocks with an unfinished pixel is refreshed after every group of eight entries and gates
// the per-block scalar branches and the early exit.
//
// EXTRA (render extras, DrawExtras): the same walk also blends the Gaussian's camera-space z (depth) and the constant 1
// (alpha = 1 - T_final) and adds T_final * bg to the image.
// Non-BOX entries carry z in the free pair of their third piece (11 floats), BOX entries in sZ.  k_draw's occupancy cap
// kept: at eight waves the depth accumulators spill 16 B per lane outside the blend loop, and that is faster than six
// waves without spills (bench scene: 166 against 197 us).  `ex` is read by the EXTRA instances only.
template <bool BOX, bool FLOOR, bool CLAMP, bool SKIP, bool EXTRA>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu((!BOX && SKIP) ? 8 : 6, 8))) void k_draw(DrawParams p, int32_t* __restrict__ ranges,
                                             const int32_t* __restrict__ gsid,
                                             const float4* __restrict__ rec, float* __restrict__ image,
                                             int32_t* __restrict__ contrib, float* __restrict__ final_tau,
                                             DrawExtras ex) {
  // (the layout of a staged entry: blend_range, egs_draw_device.h)
  __shared__ float4 sA[64], sB[64], sC[64];
  __shared__ float sZ[(EXTRA && BOX) ? 64 : 1];   // (never touched by the other instances: no LDS there)
  const int lane = threadIdx.x;
  zero_slice(p, lane);
  const int tile = xcd_tile(blockIdx.x, p);
  if (tile < 0) return;
  const int r0 = ranges[2 * (size_t)tile], r1 = ranges[2 * (size_t)tile + 1];
  const int n = r1 - r0;
  const int tx0 = (tile % p.gx) * EGS_TILE, ty0 = (tile / p.gx) * EGS_TILE;
  TileLane G;
  tile_lane_init(G, tx0, ty0, lane);
  if (n <= 0) {
    if (p.work_out && lane == 0) { p.work_out[tile] = 0; if (p.walk_out) p.walk_out[tile] = 0; walk_raise(p.walk_max, 0); }
    empty_tile<EXTRA>(G, p, tile, r0, r1, lane, ranges, image, contrib, final_tau, &ex);
    return;
  }
  // the blend state (blend_range); lanes outside the image start at tau = -1
  float tau[4], cr[4], cg[4], cb[4];
  float cd[4];   // EXTRA: sum w z
  int cont[4];
  int live = 0;
  const float stop = p.tau_stop;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    cont[k] = 0;
    tau[k] = ((G.pxb[k & 1] < p.W) && (G.pyb[k >> 1] < p.H)) ? 1.f : -1.f;
    cr[k] = 0.f; cg[k] = 0.f; cb[k] = 0.f;
    cd[k] = 0.f;
    if (__any(tau[k] >= stop)) live |= 1 << k;
  }
  blend_range<BOX, FLOOR, CLAMP, SKIP, EXTRA>(tau, cr, cg, cb, cd, cont, live, G, 0, n, r0, tx0, ty0, lane, stop, p.lskip,
                                              p.masked, p.nan_blend, gsid, rec, ex.depths, sA, sB, sC, sZ);
  if (p.work_out) {   // what k_draw_bwd will walk: the largest contributor index of the tile and of its blocks
    int w, wmax;
    block_max(cont, w, wmax);
    if (lane == 0) {
      p.work_out[tile] = w + 2 * wmax;
      if (p.walk_out) p.walk_out[tile] = wmax;
      walk_raise(p.walk_max, wmax);
      if (p.walk_max) walk_raise(p.walk_max + 1, n);      // ... and the longest list of the same render
    }
  }
  const size_t HW = (size_t)p.W * p.H;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int px = G.pxb[k & 1], py = G.pyb[k >> 1];
    if (px < p.W && py < p.H) {
      const size_t pix = (size_t)py * p.W + px;
      if constexpr (EXTRA) {   // what is left of the transmittance sees the background; alpha = 1 - T_final
        image[pix] = fmaf(tau[k], ex.bg[0], cr[k]);
        image[HW + pix] = fmaf(tau[k], ex.bg[1], cg[k]);
        image[2 * HW + pix] = fmaf(tau[k], ex.bg[2], cb[k]);
        if (ex.depth_out) ex.depth_out[pix] = cd[k];
        if (ex.alpha_out) ex.alpha_out[pix] = 1.f - tau[k];
      } else {
        image[pix] = cr[k];
        image[HW + pix] = cg[k];
        image[2 * HW + pix] = cb[k];
      }
      contrib[pix] = cont[k];
      final_tau[pix] = tau[k];
    }
  }
}

// ============================================================================
// draw backward: per-tile back-to-front gradients        (reference kernel.cu:809-950)
// ============================================================================
// ---- transposing wave reduction ------------------------------------------------------------------
// 4 entries x 9 quantities = 36 per-lane partials have to become 36 wave totals.  Every step pairs two
// registers, sends half of each to the partner lanes and adds: one output register per input pair, so the
// register count halves with the lane span (36 -> 18 -> 9 across the 16-lane rows with
// v_permlane32_swap / v_permlane16_swap, then 9 -> 5 -> 3 -> 2 -> 1 inside the rows with DPP mirrors).
// 54 + 27 instructions instead of 36 x 6 DPP adds, and the nine totals of an entry land in nine
// different lanes of its row -- exactly where the one-instruction atomic wants them.  The first step is rows_of4 of
// egs_draw_device.h; the merges inside the rows follow.
// `hi` lanes reduce b, the others reduce a; partner lane through the mirror CTRL (a bijection between
// the two lane classes)
template <int CTRL>
__device__ __forceinline__ float merge2(float a, float b, bool hi) {
  const float own = hi ? b : a, other = hi ? a : b;
  return own + dpp_get<CTRL>(other);
}
// out = a + a[mirror] everywhere, then b + b[mirror] on the banks of `bank_hi`
#define EGS_MERGE_BANK(out, a, b, ctrl, bank_hi)                                                              \
  do {                                                                                                        \
    asm("v_add_f32_dpp %0, %1, %1 " ctrl " row_mask:0xf bank_mask:0xf" : "=v"(out) : "v"(a));                  \
    asm("v_add_f32_dpp %0, %1, %1 " ctrl " row_mask:0xf bank_mask:" bank_hi : "+v"(out) : "v"(b));            \
  } while (0)
// the nine row-wise totals of (q0..q8) in lanes {0, 8, 4, 12, 2, 10, 6, 14, odd} of every row.
// NQ = 10 (render extras): q8 and a tenth q9 share the odd lanes -- both are reduced over the two mirror levels, then
// split by lane bit 1 at the quad level: q8 lands in lanes {1, 5, 9, 13}, q9 in lanes {3, 7, 11, 15}
template <int NQ>
__device__ __forceinline__ float odd_lanes_tail(const float (&q)[NQ], float r, bool h2, bool h1) {
  constexpr int M8 = 0x140, M4 = 0x141, M2 = 0x4E, M1 = 0xB1;
  float s8 = q[8] + dpp_get<M8>(q[8]);
  s8 += dpp_get<M4>(s8);
  if constexpr (NQ == 10) {
    float s9 = q[9] + dpp_get<M8>(q[9]);
    s9 += dpp_get<M4>(s9);
    return merge2<M1>(r, merge2<M2>(s8, s9, h2), h1);
  } else {
    s8 += dpp_get<M2>(s8);
    return merge2<M1>(r, s8, h1);
  }
}
// NQ = 11 (absolute screen-space gradients, ABS): the odd lanes hold the 12-leaf tree without its dz leaf -- q8 keeps lanes
// {1, 5, 9, 13}, and the lanes q9 had are split once more, by lane bit 2: leaf 10 (q[9], sum |t_x|) lands in lanes {3, 11},
// leaf 11 (q[10], sum |t_y|) in lanes {7, 15}.  The bit-2 split is a bank-masked DPP add (banks 1 and 3), no select.
__device__ __forceinline__ float odd_lanes_tail_abs(const float (&q)[11], float r, bool h2, bool h1) {
  constexpr int M8 = 0x140, M4 = 0x141, M2 = 0x4E, M1 = 0xB1;
  float s8 = q[8] + dpp_get<M8>(q[8]);
  s8 += dpp_get<M4>(s8);
  const float sx = q[9] + dpp_get<M8>(q[9]), sy = q[10] + dpp_get<M8>(q[10]);
  float sa;
  EGS_MERGE_BANK(sa, sx, sy, "row_half_mirror", "0xa");
  return merge2<M1>(r, merge2<M2>(s8, sa, h2), h1);
}

// ---- the in-row stage without selects ----------------------------------------------------------------------
// Measured on gfx950 (tools/ubench_calib.hip, cycles per wave instruction per SIMD): add / mul / fma 2.5 (full
// rate); DPP, v_cndmask, v_med3, v_min/max, v_cmp, v_readlane, v_mov_b64 4.3 (half rate); v_permlane{32,16}_swap,
// v_exp, v_rcp 8.4 (quarter rate); ds_swizzle 8.2 and ds_bpermute 24 (the LDS crossbar is shared by the four SIMDs
// of a CU: moving the cross-row exchanges there was measured 10 % SLOWER, so they stay v_permlane swaps).
// merge2 above costs two v_cndmask and a DPP add.  The first two levels split the row by lane bits 3 and 2 --
// exactly what DPP's bank mask addresses (a bank = four consecutive lanes of a row): one DPP add for everybody,
// one bank-masked DPP add for the lanes that reduce the second register; no select.  (Tried: merge2 at every level,
// slower, docs/LAB.md.)  Totals in lanes {0, 8, 4, 12, 2, 10, 6, 14, odd} of every row
template <int NQ>
__device__ __forceinline__ float rows_to_lanes9_bank(const float (&q)[NQ], int c16) {
  const bool h2 = (c16 & 2) != 0, h1 = (c16 & 1) != 0;
  constexpr int M8 = 0x140, M4 = 0x141, M2 = 0x4E, M1 = 0xB1;
  float p01, p23, p45, p67, a, b;
  EGS_MERGE_BANK(p01, q[0], q[1], "row_mirror", "0xc");        // lanes 8..15 (banks 2, 3) reduce the second one
  EGS_MERGE_BANK(p23, q[2], q[3], "row_mirror", "0xc");
  EGS_MERGE_BANK(p45, q[4], q[5], "row_mirror", "0xc");
  EGS_MERGE_BANK(p67, q[6], q[7], "row_mirror", "0xc");
  if constexpr (NQ == 11) {
    EGS_MERGE_BANK(a, p01, p23, "row_half_mirror", "0xa");
    EGS_MERGE_BANK(b, p45, p67, "row_half_mirror", "0xa");
    return odd_lanes_tail_abs(q, merge2<M2>(a, b, h2), h2, h1);
  }
  if constexpr (NQ == 10) {
    EGS_MERGE_BANK(a, p01, p23, "row_half_mirror", "0xa");
    EGS_MERGE_BANK(b, p45, p67, "row_half_mirror", "0xa");
    return odd_lanes_tail(q, merge2<M2>(a, b, h2), h2, h1);
  }
  float s8 = q[8] + dpp_get<M8>(q[8]);
  EGS_MERGE_BANK(a, p01, p23, "row_half_mirror", "0xa");       // lanes 4..7, 12..15 (banks 1, 3)
  EGS_MERGE_BANK(b, p45, p67, "row_half_mirror", "0xa");
  s8 += dpp_get<M4>(s8);
  const float r = merge2<M2>(a, b, h2);
  s8 += dpp_get<M2>(s8);
  return merge2<M1>(r, s8, h1);
}

// Per-tile back-to-front gradient pass.  One wave64 per 16x16 tile walked as four 8x8
// pixel blocks exactly like k_draw (same block cull, same exponent-domain skip test).
// Entries are visited in descending list order in groups of four.  Per entry each lane
// sums over its 4 pixels nine partials:
//   S0 = sum dL/dalpha' g                      -> dalpha          (B.5.1a)
//   S1..S3 = sum dL/dgamma_c alpha' tau        -> dcolor          (B.5b)
//   with w = dL/dalpha' alpha':  M1x = sum w dx, M1y = sum w dy,
//   M2xx = sum w dx dx, M2xy = sum w dx dy, M2yy = sum w dy dy    (B.5.2b / B.5.2c as moments:
//   du = -cinv (M1x, M1y), dcinv = -(M2xx/2, M2xy, M2yy/2), applied once per entry)
// The 9 partials are reduced across the wave 4 entries at a time (transposing reduction below) and nine
// lanes per entry issue the 9 atomics as one instruction: one atomic set per (tile, Gaussian).
// SEG: the launch runs over the forward pass's work items (items1) instead of tiles: DIRECT(tile) is the kernel
// as it always was; SPEC(tile, s) walks entries [s L, (s + 1) L) of a split tile only, and a pixel whose last
// contributor lies BEHIND the segment starts from the state the forward pass's COMPOSE item left for the segment's end
// -- the transmittance there and G, the colour of everything behind it (lq = dL/dgamma . G) -- where the unsplit kernel
// starts every pixel from (final_tau, 0) at its last contributor.
//
// EXTRA (render extras, DrawExtras; never with SEG): the loss also sees depth = sum w z and alpha = sum w, and the image
// T_final * bg.  The scalar recurrence stays one register: lq starts at dL/dgamma . bg (the colour behind the last
// contributor) minus dL/dalpha, and dq gains dL/ddepth z; a tenth partial dz = sum dL/ddepth w goes to gpack[i][9].
// z of the staged entries in sZ, next to sD.  Four waves per SIMD (111-114 VGPRs): under the plain instances' cap of five
// the tenth partial and the per-pixel dL/ddepth spill 44-60 B per lane, and that is slower (bench scene: 531 against
// 494 us).
// fa: the flavour's own argument -- SegArgs fa.sg, or DrawExtras fa.ex for EXTRA (DrawBwdFlavour, egs_raster.h)
//
// ABS (absolute screen-space gradients, AbsGS / gsplat's absgrad; with SEG, never with EXTRA): besides du = sum t the
// walk also sums |t_x| and |t_y| of every hit, t = -w cinv (dx, dy) -- the densification statistic in which the pulls of
// different pixels on a large Gaussian cannot cancel.  cinv is the entry's sD[j] (a broadcast read), the two sums are
// leaves 10 and 11 of the reduction and go out with the other nine, in the same atomic instruction, to the pad slots
// gpack[i][10] and gpack[i][11] (the chain rule never reads them; egs_grad_records_absgrad copies them out).  A
// statistic, not a gradient.  Occupancy: DRAWB_ABS_WAVES.
constexpr int DRAWB_ABS_WAVES = 4;   // waves per SIMD the ABS instances are compiled for (chosen by measurement)
template <bool BOX, bool FLOOR, bool CLAMP, bool SEG, bool EXTRA, bool ABS = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(EXTRA ? 4 : (ABS ? DRAWB_ABS_WAVES : 5), 8))) void k_draw_bwd(DrawParams p, const int32_t* __restrict__ ranges,
                                                 const int32_t* __restrict__ gsid,
                                                 const float4* __restrict__ rec,
                                                 const float* __restrict__ final_tau,
                                                 const int32_t* __restrict__ contrib,
                                                 const float* __restrict__ dLdg,
                                                 float* __restrict__ gpack, DrawBwdFlavour<EXTRA> fa) {
  static_assert(!(SEG && EXTRA), "the EXTRA flavour draws unsplit lists only");
  static_assert(!(ABS && EXTRA), "the ABS flavour is not built for renders with extras");
  __shared__ float4 sA[64], sB[64], sC[64], sD[64];  // sD = {cinv.x, cinv.y, cinv.z, gsid}
  __shared__ float4 szero[3];                        // a line of zeros (see the accumulator reset below)
  __shared__ float sZ[EXTRA ? 64 : 1];               // (never touched by the other instances: no LDS there)
  constexpr int NQ = EXTRA ? 10 : (ABS ? 11 : 9);
  if (threadIdx.x < 3) szero[threadIdx.x] = make_float4(0.f, 0.f, 0.f, 0.f);
  const uint32_t zaddr = (uint32_t)(uintptr_t)szero;   // LDS byte offset of the zero line
  int tile, seg_lo = 0, seg_hi = 0x7fffffff;   // SEG: the entries [seg_lo, seg_hi) of the tile's list are this wave's
  size_t seg_state = 0;
  bool seg_item = false;
  if constexpr (SEG) {
    if ((int)blockIdx.x >= min(fa.sg.hdr[SH_ITEMS1], fa.sg.item_cap)) return;
    const uint32_t item = (uint32_t)fa.sg.items1[blockIdx.x];
    tile = (int)(item & SEG_TILE_MASK);
    if (tile >= p.T) return;
    if ((item >> 30) == (uint32_t)SEG_SPEC) {
      const int L = fa.sg.hdr[SH_L], sidx = (int)((item >> 19) & SEG_SEG_MASK);
      seg_item = true;
      seg_lo = sidx * L; seg_hi = seg_lo + L;
      seg_state = ((size_t)(fa.sg.seg_base[tile] + sidx)) * 256 + threadIdx.x;
    }
  } else {
    tile = xcd_tile(blockIdx.x, p);
    if (tile < 0) return;
  }
  const int r0 = ranges[2 * (size_t)tile], r1 = ranges[2 * (size_t)tile + 1];
  const int n = r1 - r0;
  if (n <= 0) return;
  if (SEG) seg_hi = min(seg_hi, n);
  const int lane = threadIdx.x;
  const int tx0 = (tile % p.gx) * EGS_TILE, ty0 = (tile / p.gx) * EGS_TILE;
  const int pxb[2] = {tx0 + (lane & 7), tx0 + (lane & 7) + 8};
  const int pyb[2] = {ty0 + (lane >> 3), ty0 + (lane >> 3) + 8};
  const float fpx[2] = {(float)pxb[0], (float)pxb[1]};
  const float fpy[2] = {(float)pyb[0], (float)pyb[1]};
  const size_t HW = (size_t)p.W * p.H;
  // lq = dL/dgamma . gamma_cur2last: the only combination of gamma_cur2last (kernel.cu:854,948)
  // the gradient needs, so the 3-vector recurrence q += a'(c - q) is carried as one scalar
  float tau[4], lr[4], lg[4], lb[4], lq[4];
  float ld[4], la[4];   // EXTRA: dL/ddepth, dL/dalpha of the pixel
  int cont[4];
  int bmax[4];  // wave-uniform: largest contrib of block k -> entries >= bmax[k] are inert for it
  int maxcont = 0;
  // (all twenty loads requested first, from clamped addresses: guarded and inside the loop below, every block's
  // five waited for their own round trip before the next block's were issued)
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int px = pxb[k & 1], py = pyb[k >> 1];
    const size_t pix = (size_t)min(py, p.H - 1) * p.W + min(px, p.W - 1);
    tau[k] = final_tau[pix];
    cont[k] = contrib[pix];
    lr[k] = dLdg[pix]; lg[k] = dLdg[HW + pix]; lb[k] = dLdg[2 * HW + pix];
    lq[k] = 0.f;
    ld[k] = 0.f; la[k] = 0.f;
    if constexpr (EXTRA) {
      if (fa.ex.dl_depth) ld[k] = fa.ex.dl_depth[pix];
      if (fa.ex.dl_alpha) la[k] = fa.ex.dl_alpha[pix];
    }
  }
  if constexpr (EXTRA) {
    // lq - dL/dalpha is carried instead of lq: dq = dL/dgamma . c + dL/ddepth z + dL/dalpha - lq with one FMA per hit,
    // and the update lq += a' dq is the same for both
#pragma unroll
    for (int k = 0; k < 4; ++k) lq[k] = lr[k] * fa.ex.bg[0] + lg[k] * fa.ex.bg[1] + lb[k] * fa.ex.bg[2] - la[k];
  }
  float4 segE[4];
  if constexpr (SEG) {   // (requested with the loads above; a DIRECT item or the last segment never uses them)
#pragma unroll
    for (int k = 0; k < 4; ++k) segE[k] = seg_item ? fa.sg.st4[seg_state + 64 * k] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int px = pxb[k & 1], py = pyb[k >> 1];
    if (!(px < p.W && py < p.H)) { tau[k] = 0.f; cont[k] = 0; lr[k] = 0.f; lg[k] = 0.f; lb[k] = 0.f; }
    if constexpr (SEG) {
      if (seg_item) {
        if (cont[k] > seg_hi) {          // contributors behind this segment: start from the state at its end
          tau[k] = segE[k].w;
          lq[k] = lr[k] * segE[k].x + lg[k] * segE[k].y + lb[k] * segE[k].z;
          cont[k] = seg_hi;
        } else if (cont[k] <= seg_lo) {  // the pixel never got this far
          cont[k] = 0;
        }
      }
    }
    int mx = cont[k];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mx = max(mx, __shfl_xor(mx, d, 64));
    bmax[k] = __builtin_amdgcn_readfirstlane(min(mx, n));
    maxcont = max(maxcont, bmax[k]);
  }
  if (maxcont <= 0) return;
  // The loads above must be WAITED FOR here, not at their first use inside the loop: gfx9 counts stores and
  // atomics in the same in-order vmcnt as loads, so a wait the compiler places at the first use (inside the
  // hit body) would, from the second group on, also wait for the previous group's gradient atomics --
  // a round trip to L2 per group of four entries on the critical path of the wave.
#pragma unroll
  for (int k = 0; k < 4; ++k)
    asm volatile("" ::"v"(tau[k]), "v"(lr[k]), "v"(lg[k]), "v"(lb[k]), "v"(cont[k]));
  if constexpr (EXTRA) {
#pragma unroll
    for (int k = 0; k < 4; ++k) asm volatile("" ::"v"(ld[k]), "v"(lq[k]));
  }
  // where the transposing reduction leaves the nine totals inside a row of 16 lanes, and what each of
  // those lanes adds to the packed gradient record {dalpha, dcolor[3], du[2], dcinv[3]}
  const int c16 = lane & 15;
  int qoff = -1, kind = 0;
  float kscale = 1.f;
  if (c16 & 1) {
    if (c16 == 1) { qoff = 8; kscale = -0.5f; }                         // M2yy -> dcinv.z
    else if (EXTRA && c16 == 3) qoff = 9;                               // dz   -> the first pad slot
    else if (ABS && c16 == 3) qoff = 10;                                // sum |t_x| -> the second pad slot
    else if (ABS && c16 == 7) qoff = 11;                                // sum |t_y| -> the third
  }
  else if (c16 == 0) { qoff = 4; kind = 1; }                            // M1x  -> du.x
  else if (c16 == 2) { qoff = 5; kind = 2; }                            // M1y  -> du.y
  else if (c16 == 4) qoff = 0;                                          // dalpha
  else if (c16 == 6) qoff = 1;                                          // dcolor.r
  else if (c16 == 8) qoff = 2;                                          // dcolor.g
  else if (c16 == 10) qoff = 3;                                         // dcolor.b
  else if (c16 == 12) { qoff = 6; kscale = -0.5f; }                     // M2xx -> dcinv.x
  else { qoff = 7; kscale = -1.f; }                                     // M2xy -> dcinv.y  (lane 14)

  const int c_first = (maxcont - 1) >> 6;
  int gnext = (c_first * 64 + lane < n) ? gsid[r0 + c_first * 64 + lane] : 0;   // one chunk ahead, as in k_draw
  const int c_last = SEG ? (seg_lo >> 6) : 0;
  for (int c = c_first; c >= c_last; --c) {
    __syncthreads();
    const int idx = c * 64 + lane;
    int mymask = 0;  // reach mask of the entry THIS lane staged (lane j <-> entry c*64 + j)
    const int gm = gnext;
    const int g = p.masked ? (int)((uint32_t)gm & EGS_GSID_MASK) : gm;
    if (c > c_last) gnext = gsid[r0 + idx - 64];
    if (idx < n) {
      float4 A = rec[3 * (size_t)g], B = rec[3 * (size_t)g + 1];
      const float4 C = rec[3 * (size_t)g + 2];
      constexpr float INVQ = 1.f / EGS_NHL2E;
      // (cinv from the record as it is: an entry with a NaN conic hands NaN to du = -cinv M1, as kernel.cu:926-933 does)
      const float4 Dc = make_float4(A.z * INVQ, A.w * (0.5f * INVQ), B.x * INVQ, __int_as_float(g));
      const bool nanfix = p.nan_blend && nan_entry_fix(A, B);
      mymask = p.masked ? (int)((uint32_t)gm >> EGS_GSID_BITS) : reach_mask<BOX>(A, C, tx0, ty0);
      if (nanfix && !BOX && !p.masked) mymask = 0xF;
      sA[lane] = A;
      sB[lane] = B;
      sC[lane] = C;
      if constexpr (EXTRA) sZ[lane] = fa.ex.depths[g];
      // cinv back out of the pre-scaled conic of the record (q = -0.5 log2(e) (cinv.x, 2 cinv.y, cinv.z)):
      // no second 12-B gather per patch (131 MB of sector traffic at P = 4.1 M)
      sD[lane] = Dc;
    }
    __syncthreads();
    // Which entries of this chunk can contribute at all?  Every lane answers for the entry it staged: its
    // reach mask minus the blocks no pixel of which ever got this far (entry index >= the block's largest
    // contrib, kernel.cu:899); a scalar bit scan then walks the reachable entries in descending list order.
    // Groups of four: each of the four accumulator slots takes entries until one of them HITS (a quarter
    // of the entries that reach a live block hit no pixel: they leave the slot zero and cost neither a
    // re-zeroing nor a share of a wave reduction).
    int rl = mymask;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (idx >= bmax[k]) rl &= ~(1 << k);
    unsigned long long todo = __ballot(rl != 0);
    while (todo != 0ull) {
      int je[4] = {-1, -1, -1, -1};   // chunk-local entry index held by slot e
      float acc[4][NQ];
      bool any = false;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        {
          // The nine zeros come out of LDS: broadcast reads of a zero line cost the VALU nothing (nine v_mov_b32 or
          // five v_mov_b64 are 21 issue cycles per slot in a kernel that is VALU-issue bound; the LDS pipe idles).
          // Inline asm, because the compiler would hoist a plain load and hand out register copies again.  The
          // wait is part of the statement: the compiler does not see these loads in its lgkmcnt bookkeeping and
          // may copy the results anywhere afterwards.  (The wave parks for one LDS latency; its four neighbours
          // on the SIMD issue meanwhile.)
          typedef float f4v __attribute__((ext_vector_type(4)));
          f4v z0, z1;
          float z2;
          asm volatile("ds_read_b128 %0, %3\n ds_read_b128 %1, %3 offset:16\n ds_read_b32 %2, %3 offset:32\n"
                       " s_waitcnt lgkmcnt(0)"
                       : "=v"(z0), "=v"(z1), "=v"(z2) : "v"(zaddr));
          acc[e][0] = z0.x; acc[e][1] = z0.y; acc[e][2] = z0.z; acc[e][3] = z0.w;
          acc[e][4] = z1.x; acc[e][5] = z1.y; acc[e][6] = z1.z; acc[e][7] = z1.w;
          acc[e][8] = z2;
        }
        if constexpr (EXTRA) acc[e][NQ - 1] = 0.f;
        if constexpr (ABS) { acc[e][9] = 0.f; acc[e][10] = 0.f; }
        while (todo != 0ull) {
        const int j = 63 - __clzll((long long)todo);
        todo &= ~(1ull << j);
        bool any_e = false;
        const int i = c * 64 + j;  // forward index of this entry in the tile list
        const int reach = __builtin_amdgcn_readlane(rl, j);  // lane j's register: no LDS round trip
        const float4 A = sA[j], B = sB[j], C = sC[j];
        float zj = 0.f;
        if constexpr (EXTRA) zj = sZ[j];
        float4 Dj = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (ABS) Dj = sD[j];   // cinv of this entry
        bool inx[2] = {true, true}, iny[2] = {true, true};
        if (BOX) {
          const uint32_t bx = __float_as_uint(C.y), by = __float_as_uint(C.z);
          const int x0 = bx & 0xFFFF, x1 = bx >> 16, y0 = by & 0xFFFF, y1 = by >> 16;
#pragma unroll
          for (int b = 0; b < 2; ++b) {
            inx[b] = (pxb[b] >= x0) && (pxb[b] < x1);
            iny[b] = (pyb[b] >= y0) && (pyb[b] < y1);
          }
        }
        // The exponent from scratch per evaluated block (7 full-rate instructions) instead of the separable form
        // cxx[bx] + cyy[by] + cxy[bx] dy[by] (14 per entry up front + 2 per block; tried, slower, docs/LAB.md): most
        // entries reach one or two of the four blocks.
        // (Measured and dropped: skipping the floor / clamp v_med3 for entries with a positive-definite conic and
        // alpha <= 0.989 behind a wave-uniform flag -- the two scalar branches cost more than the two half-rate
        // instructions they save: +1.5 %.)
        float dx[2], dy[2];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int bx = k & 1, by = k >> 1;
          if (!(reach & (1 << k))) continue;  // scalar branch: block culled or past its last contributor
          dx[bx] = A.x - fpx[bx];
          dy[by] = A.y - fpy[by];
          float t = A.z * dx[bx];
          t = fmaf(A.w, dy[by], t);
          float pw = t * dx[bx];
          pw = fmaf(B.x * dy[by], dy[by], pw);
          bool hit = (i < cont[k]) && (pw >= C.w);  // kernel.cu:899,913
          if (BOX) hit = hit && inx[bx] && iny[by];
          if (hit) {
            const float g = __builtin_amdgcn_exp2f(FLOOR ? min_hi(pw, 0.f) : pw);
            float ap = B.y * g;
            if (CLAMP) ap = min_hi(ap, 0.99f);
            const float tk = tau[k] * __builtin_amdgcn_rcpf(1.f - ap);  // undo F.5.2
            tau[k] = tk;
            float dq;   // dL/dgamma . (color - gamma_cur2last)
            if constexpr (EXTRA) dq = fmaf(ld[k], zj, lr[k] * B.z + lg[k] * B.w + lb[k] * C.x) - lq[k];
            else dq = (lr[k] * B.z + lg[k] * B.w + lb[k] * C.x) - lq[k];
            const float dl_dap = tk * dq;  // B.5a
            acc[e][0] += dl_dap * g;  // dalpha'/dalpha = g, also where the clamp binds (kernel.cu:921)
            const float wgt = ap * tk;
            acc[e][1] += lr[k] * wgt; acc[e][2] += lg[k] * wgt; acc[e][3] += lb[k] * wgt;
            if constexpr (EXTRA) acc[e][NQ - 1] += ld[k] * wgt;   // dz
            const float w = dl_dap * ap;
            const float wx = w * dx[bx], wy = w * dy[by];
            acc[e][4] += wx; acc[e][5] += wy;
            acc[e][6] += wx * dx[bx]; acc[e][7] += wx * dy[by]; acc[e][8] += wy * dy[by];
            if constexpr (ABS) {   // |t_x|, |t_y| of this pixel (abs is a source modifier of the add)
              acc[e][9] += fabsf(fmaf(Dj.x, wx, Dj.y * wy));
              acc[e][10] += fabsf(fmaf(Dj.y, wx, Dj.z * wy));
            }
            lq[k] += ap * dq;  // gamma_cur2last <- a' color + (1 - a') gamma_cur2last, dotted with dL/dgamma
            any_e = true;
          }
        }
        if (__any(any_e)) {  // wave-uniform: the entry contributed, the slot is taken
          je[e] = j;
          any = true;
          break;
        }
        }  // next reachable entry into the same (still zero) slot
      }
      if (any) {  // wave-uniform
        // quantity order chosen so that the two first moments meet in one quad (lanes 0 and 2):
        //   lane 0: M1x  2: M1y  4: dalpha  6,8,10: dcolor  12: M2xx  14: M2xy  odd: M2yy
        float rows[NQ];
        // acc index feeding leaf q0..q8 (EXTRA: q9; ABS: q9, q10)
        constexpr int ORDER[11] = {4, 2, 0, 6, 5, 3, 1, 7, 8, 9, 10};
#pragma unroll
        for (int q = 0; q < NQ; ++q)
          rows[q] = rows_of4(acc[0][ORDER[q]], acc[1][ORDER[q]], acc[2][ORDER[q]], acc[3][ORDER[q]]);
        const float v = rows_to_lanes9_bank(rows, c16);
        // row r of the wave holds the totals of slot e = {0,2,1,3}[r]
        const int row = lane >> 4;
        const int e = ((row & 1) << 1) | (row >> 1);
        const int j = (e == 0) ? je[0] : (e == 1) ? je[1] : (e == 2) ? je[2] : je[3];
        // an empty slot (the chunk ran out of entries) holds zeros and no entry: it must not touch memory
        const bool rowact = j >= 0;
        const float4 D = sD[j & 63];
        // B.5.2b / B.5.2c from the moments: du = -cinv (M1x, M1y) needs both first moments -> the partner
        // comes from the other lane of the pair (quad_perm [2,3,0,1]); dcinv = -(M2xx/2, M2xy, M2yy/2).
        // The 9 atomics of an entry are ONE instruction on ONE 48-byte gradient record.
        const float nb = dpp_get<0x4E>(v);
        const float c_own = (kind == 1) ? -D.x : ((kind == 2) ? -D.z : kscale);
        float val = v * c_own;
        if (kind != 0) val = fmaf(nb, -D.y, val);
        if (rowact && qoff >= 0 && val != 0.f)
          unsafeAtomicAdd(gpack + 12 * (size_t)__float_as_int(D.w) + qoff, val);
      }
    }
  }
}

// packed [N][12] gradient records -> the four output tensors of splatB
__global__ __launch_bounds__(256) void k_unpack_grads(int n, const float4* __restrict__ gpack,
                                                      float* __restrict__ dus, float* __restrict__ dcinv,
                                                      float* __restrict__ dalpha, float* __restrict__ dcolor) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float4 a = gpack[3 * (size_t)i], b = gpack[3 * (size_t)i + 1], c = gpack[3 * (size_t)i + 2];
  dalpha[i] = a.x;
  dcolor[3 * (size_t)i] = a.y; dcolor[3 * (size_t)i + 1] = a.z; dcolor[3 * (size_t)i + 2] = a.w;
  dus[2 * (size_t)i] = b.x; dus[2 * (size_t)i + 1] = b.y;
  dcinv[3 * (size_t)i] = b.z; dcinv[3 * (size_t)i + 1] = b.w; dcinv[3 * (size_t)i + 2] = c.x;
}

// slots 10 and 11 of the packed [N][12] gradient records (what the ABS draw instances left there) -> [N][2]
__global__ __launch_bounds__(256) void k_records_absgrad(int n, const float4* __restrict__ gpack,
                                                         float2* __restrict__ dus_abs) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float4 c = gpack[3 * (size_t)i + 2];
  dus_abs[i] = make_float2(c.z, c.w);
}

// ============================================================================
// host side
// ============================================================================
DrawParams make_draw_params(int W, int H, const EgsPolicy* pol, bool backward) {
  DrawParams p;
  p.W = W; p.H = H;
  p.gx = div_up(W, EGS_TILE);
  p.gy = div_up(H, EGS_TILE);
  p.T = p.gx * p.gy;
  // tile -> workgroup map, chosen by measurement (same-box A/B, 1 M Gaussians at 1080p): the forward kernel
  // is 2 % faster with tile rows interleaved over the XCDs (223 vs 227 us), the backward kernel 2.5 % faster
  // with the plain map (580 vs 595 us).
  p.map_mode = backward ? 0 : 2;
  p.order = nullptr;
  p.ngrid = 0;
  p.zero_buf = nullptr;
  p.zero_n4 = 0;
  p.zero_per = 0;
  p.work_out = nullptr;
  p.walk_out = nullptr;
  p.walk_max = nullptr;
  p.masked = 0;
  p.alpha_skip = pol->alpha_skip; p.tau_stop = pol->tau_stop;
  p.lskip = pol->alpha_skip > 0.f ? log2f(pol->alpha_skip) : -INFINITY;
  p.maha_floor = pol->maha_floor; p.alpha_clamp = pol->alpha_clamp;
  p.nan_blend = pol->nan_maha == 0 && pol->maha_floor;
  return p;
}

// Longest-list-first dispatch (k_tile_order) for one of the draw kernels; without a buffer, or for an image of more
// tiles than the kernel handles, the plain tile map stays.
int tile_order_enqueue(DrawParams& p, int32_t* buf, size_t buf_len, const int32_t* ranges, hipStream_t s,
                       const int32_t* work, const int32_t* walk, uint32_t* hint) {
  if (!buf || (size_t)p.T > buf_len || p.T > TILE_ORDER_MAX_T) return 0;
  EGS_LAUNCH("k_tile_order", k_tile_order, dim3(1), dim3(1024), s, ranges, work, p.T, buf, walk, hint);
  EGS_LAUNCH_OK();
  p.order = buf;
  p.ngrid = p.T;
  return 0;
}

int tile_work_from_contrib(const DrawParams& p, const int32_t* contrib, int32_t* work, int32_t* walk, hipStream_t s) {
  if (work) EGS_LAUNCH("k_tile_work", k_tile_work, dim3(p.T), dim3(64), s, p.W, p.H, p.gx, contrib, work, walk);
  else EGS_LAUNCH("k_tile_walk", k_tile_walk, dim3(p.T), dim3(64), s, p.W, p.H, p.gx, contrib, walk);
  EGS_LAUNCH_OK();
  return 0;
}

// policy -> template arguments (compile-time footprint / floor / clamp / skip) and flavour, forward draw
// ex (nullable): the render extras
int launch_draw(const DrawParams& dp, const EgsPolicy* pol, int32_t* ranges, const int32_t* gsid, const float4* rec,
                float* image, int32_t* contrib, float* final_tau, const DrawExtras* ex, hipStream_t s) {
  decltype(&k_draw<false, false, false, false, false>) kern = nullptr;
  with_bools(
      [&](auto box, auto flr, auto clamp, auto skip, auto extra) {
        kern = k_draw<box.value, flr.value, clamp.value, skip.value, extra.value>;
      },
      pol->footprint == 1, pol->maha_floor != 0, pol->alpha_clamp != 0, pol->alpha_skip > 0.f, ex != nullptr);
  EGS_LAUNCH(ex ? "k_draw_extra" : "k_draw", kern, dim3(draw_grid(dp)), dim3(64), s, dp, ranges, gsid, rec, image,
             contrib, final_tau, ex ? *ex : DrawExtras{});
  EGS_LAUNCH_OK();
  return 0;
}

// ... backward draw.  ex (nullable): the render extras
int launch_draw_bwd(const DrawParams& dp, const EgsPolicy* pol, const int32_t* ranges, const int32_t* gsid,
                    const float4* rec, const float* final_tau, const int32_t* contrib, const float* dLdg, float* gpack,
                    const DrawExtras* ex, hipStream_t s, bool absgrad) {
  const bool box = pol->footprint == 1, flr = pol->maha_floor != 0, clamp = pol->alpha_clamp != 0;
  if (ex) {   // the flavour's own kernel argument: two pointer types
    decltype(&k_draw_bwd<false, false, false, false, true>) kern = nullptr;
    with_bools([&](auto b, auto f, auto c) { kern = k_draw_bwd<b.value, f.value, c.value, false, true>; }, box, flr, clamp);
    EGS_LAUNCH("k_draw_bwd_extra", kern, dim3(draw_grid(dp)), dim3(64), s, dp, ranges, gsid, rec, final_tau, contrib,
               dLdg, gpack, DrawBwdFlavour<true>{*ex});
  } else {
    decltype(&k_draw_bwd<false, false, false, false, false>) kern = nullptr;
    with_bools(
        [&](auto b, auto f, auto c, auto a) { kern = k_draw_bwd<b.value, f.value, c.value, false, false, a.value>; },
        box, flr, clamp, absgrad);
    EGS_LAUNCH(absgrad ? "k_draw_bwd_abs" : "k_draw_bwd", kern, dim3(draw_grid(dp)), dim3(64), s, dp, ranges, gsid, rec,
               final_tau, contrib, dLdg, gpack, DrawBwdFlavour<false>{});
  }
  EGS_LAUNCH_OK();
  return 0;
}

int launch_draw_bwd_seg(const DrawParams& dp, const EgsPolicy* pol, const int32_t* ranges, const int32_t* gsid,
                        const float4* rec, const float* final_tau, const int32_t* contrib, const float* dLdg,
                        float* gpack, const SegArgs& sga, int grid, hipStream_t s, bool absgrad) {
  decltype(&k_draw_bwd<false, false, false, true, false>) kern = nullptr;
  with_bools([&](auto flr, auto clamp, auto a) { kern = k_draw_bwd<false, flr.value, clamp.value, true, false, a.value>; },
             pol->maha_floor != 0, pol->alpha_clamp != 0, absgrad);
  EGS_LAUNCH(absgrad ? "k_draw_bwd_seg_abs" : "k_draw_bwd_seg", kern, dim3(grid), dim3(64), s, dp, ranges, gsid, rec,
             final_tau, contrib, dLdg, gpack, DrawBwdFlavour<false>{sga});
  EGS_LAUNCH_OK();
  return 0;
}

int unpack_grads(int n, const float* gpack, float* dus, float* dcinv, float* dalpha, float* dcolor, hipStream_t s) {
  EGS_LAUNCH("k_unpack_grads", k_unpack_grads, dim3(div_up(n, 256)), dim3(256), s, n, (const float4*)gpack, dus, dcinv,
             dalpha, dcolor);
  EGS_LAUNCH_OK();
  return 0;
}

}  // namespace egs

extern "C" int egs_grad_records_absgrad(int n, const float* grad_records, float* dloss_dus_abs, void* stream) {
  using namespace egs;
  EGS_CHECK_ARG(n >= 0);
  if (n == 0) return 0;
  EGS_CHECK_ARG(grad_records && dloss_dus_abs);
  EGS_CHECK_ARG((((uintptr_t)grad_records & 15) | ((uintptr_t)dloss_dus_abs & 7)) == 0);
  EGS_LAUNCH("k_records_absgrad", k_records_absgrad, dim3(div_up(n, 256)), dim3(256), (hipStream_t)stream, n,
             (const float4*)grad_records, (float2*)dloss_dus_abs);
  EGS_LAUNCH_OK();
  return 0;
}

// a caller-held tile_order buffer: [dispatch order of the forward draw | per-tile work it measured | walk (T ints each)]
extern "C" size_t egs_tile_order_len(int width, int height) {
  const int gx = egs::div_up(width, EGS_TILE), gy = egs::div_up(height, EGS_TILE);
  return 3 * (size_t)gx * gy;
}
