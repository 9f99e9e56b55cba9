// The per-tile alpha-blend kernels for gfx950 (CDNA4, wave64): k_draw (reference gsplatcu/kernel.cu:152-271) and
// k_draw_bwd (kernel.cu:809-950), the dispatch order of their tiles (k_tile_order) and the launchers that pick the
// template instance of a raster policy.  One wave64 per 16x16 tile; see egs_raster.h for how this differs from the
// reference by design.
#include "egs_draw_device.h"

#include <stdlib.h>

namespace egs {

// default dispatch order of the tiles for the forward / backward draw kernel (k_tile_order modes)
#ifndef EGS_TILE_ORDER_F_DEFAULT
#define EGS_TILE_ORDER_F_DEFAULT 1
#endif
#ifndef EGS_TILE_ORDER_B_DEFAULT
#define EGS_TILE_ORDER_B_DEFAULT 1
#endif
#ifndef EGS_DRAWB_RED_DEFAULT
#define EGS_DRAWB_RED_DEFAULT 7
#endif

// Longest-list-first dispatch order of the tiles for the two draw kernels.  A tile is one wave whose run
// time is proportional to its list length (0 ... ~2x the mean on the 1 M scene); workgroups are handed to
// the SIMDs in index order, so with tiles in IMAGE order a launch ends with whichever SIMD drew the longest
// lists while the others idle.  Sorted by length (descending) the long tiles start first and the short ones
// fill the gaps (LPT scheduling); when every tile is resident at once (k_draw: 8 waves per SIMD) the
// sorted order is dealt out in a serpentine of `period` slots so that every SIMD receives one tile of each
// length stratum, alternately from its top and its bottom.
//   mode 1: one global order           mode 2: global, serpentine
//   mode 3: per XCD (tile row % 8 stays on XCD b % 8: horizontal neighbours share one L2), sorted
//   mode 4: per XCD, serpentine
// One workgroup: counting sort on (class, length) in LDS -- 8160 tiles take a few microseconds.
constexpr int TO_BINS = 1024;
constexpr int TO_REGS = 16;    // tiles per thread whose (bin, rank) stay in registers between the two passes
// sort key of tile t: its list length, or -- `work` given -- the work the forward draw kernel measured for it
__device__ __forceinline__ int tile_len(const int32_t* __restrict__ ranges, const int32_t* __restrict__ work, int t) {
  if (work) return work[t];
  const int2 r = reinterpret_cast<const int2*>(ranges)[t];
  return r.y - r.x;
}
__global__ __launch_bounds__(1024) void k_tile_order(const int32_t* __restrict__ ranges,
                                                     const int32_t* __restrict__ work, int T, int gx, int mode,
                                                     int period, int32_t* __restrict__ order, int ngrid,
                                                     const int32_t* __restrict__ walk = nullptr,
                                                     uint32_t* __restrict__ hint = nullptr) {
  // walk / hint (nullable): hint[1] receives the longest WALK of the camera's previous render (walk[T], next to its work),
  // hint[0] the longest list when the tiles are sorted by length -- page-locked words the host steers by (fused.py: long
  // walks take the segment path)
  // 8192 bins in all: one class of 8192 (global modes) or eight of 1024 (per-XCD modes).
  // ONE LDS atomic per tile: the returning add that counts a bin also hands the tile its rank inside the bin
  // (arrival order -- any order inside a bin will do); after the scan of the bins its slot is start + rank.
  // LDS atomics retire about one lane per clock whatever the conflicts, so the kernel costs ~T cycles per pass:
  // the first version's two passes took 9 us at 1080p and 45 us at 4K (32400 tiles).
  constexpr int NB = 8 * TO_BINS;
  __shared__ uint32_t bins[NB];
  __shared__ uint32_t wsum[16];
  __shared__ uint32_t cbase[9];
  const int tid = threadIdx.x;
  const bool per_xcd = mode >= 3;
  const int cbins = per_xcd ? TO_BINS : NB;                       // bins per class
  // key -> bin: list lengths 1:1 (1:4 per XCD); the forward kernel's work measure is ~6x a length
  const int shift = (per_xcd ? 2 : 0) + (work ? 2 : 0);
  int lenr[TO_REGS];     // all loads in flight at once: the kernel is a chain of latencies, not of bytes
#pragma unroll
  for (int r = 0; r < TO_REGS; ++r) {
    const int t = tid + r * 1024;
    lenr[r] = t < T ? tile_len(ranges, work, t) : 0;
  }
  for (int i = tid; i < NB; i += 1024) bins[i] = 0u;
  if (per_xcd)   // classes are padded to the largest one: slots without a tile stay -1
    for (int i = tid; i < ngrid; i += 1024) order[i] = -1;
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
  auto key_of = [&](int t, int len) {
    const int q = min(max(len, 0) >> shift, cbins - 1);
    const int cls = per_xcd ? ((t / gx) & 7) : 0;
    return cls * cbins + (cbins - 1 - q);
  };
  // pass 1: (bin, rank) per tile, packed 13 + 19 bits (T < 2^19: checked by the host)
  uint32_t kr[TO_REGS];
#pragma unroll
  for (int r = 0; r < TO_REGS; ++r) {
    const int t = tid + r * 1024;
    kr[r] = 0u;
    if (t < T) {
      const int key = key_of(t, lenr[r]);
      kr[r] = ((uint32_t)key << 19) | atomicAdd(&bins[key], 1u);
    }
  }
  // (tiles beyond TO_REGS * 1024 keep their (bin, rank) in the order buffer itself until pass 2)
  for (int t = tid + TO_REGS * 1024; t < T; t += 1024) {
    const int key = key_of(t, tile_len(ranges, work, t));
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
  if (tid < 8) cbase[tid] = per_xcd ? bins[tid * TO_BINS] : (tid == 0 ? 0u : (uint32_t)T);
  if (tid == 8) cbase[8] = (uint32_t)T;
  __syncthreads();
  const bool serp = (mode == 2 || mode == 4) && period > 0;
  auto slot_of = [&](uint32_t packed) {
    const int key = (int)(packed >> 19);
    const int cls = key / cbins;
    int r = (int)(bins[key] + (packed & 0x7FFFFu) - cbase[cls]);
    if (serp) {
      const int cnt = (int)(cbase[cls + 1] - cbase[cls]);
      const int st = r / period, ps = r - st * period;
      if (st & 1) r = st * period + (min(period, cnt - st * period) - 1 - ps);
    }
    return per_xcd ? 8 * r + cls : r;
  };
  // pass 2 for the tiles parked in the order buffer: read them ALL before any slot is written (a slot may be
  // another tile's parking place)
  constexpr int TO_TAIL = 24;      // up to (TO_REGS + TO_TAIL) * 1024 = 40960 tiles (a 4K image has 32400)
  uint32_t tail[TO_TAIL];
#pragma unroll
  for (int u = 0; u < TO_TAIL; ++u) {
    const int t = tid + (TO_REGS + u) * 1024;
    tail[u] = t < T ? (uint32_t)order[t] : 0u;
  }
  __syncthreads();
  if (per_xcd) {   // the parking places go back to "no tile" before the real slots are written
#pragma unroll
    for (int u = 0; u < TO_TAIL; ++u) {
      const int t = tid + (TO_REGS + u) * 1024;
      if (t < T) order[t] = -1;
    }
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < TO_REGS; ++r) {
    const int t = tid + r * 1024;
    if (t < T) { const int slot = slot_of(kr[r]); if (slot < ngrid) order[slot] = t; }
  }
#pragma unroll
  for (int u = 0; u < TO_TAIL; ++u) {
    const int t = tid + (TO_REGS + u) * 1024;
    if (t < T) { const int slot = slot_of(tail[u]); if (slot < ngrid) order[slot] = t; }
  }
}
static_assert(TILE_ORDER_MAX_T == (TO_REGS + 24) * 1024, "what k_tile_order handles");

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
// capacity of an order buffer: the per-XCD modes pad every class to the largest one
int tile_order_len(int gx, int gy) { return 8 * div_up(gy, 8) * gx; }

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
  if (p.map_mode == 1) {
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
// Dynamic LDS requested only to CAP the number of resident tile-waves per CU (experiment knobs
// EGS_DRAW_LDS_PAD / EGS_DRAWB_LDS_PAD, bytes): fewer resident waves let the dispatcher hand the
// remaining tiles to whichever SIMD drains first (dynamic load balance).
static size_t draw_lds_pad(int which) {
  static const size_t pad[2] = {
      [] { const char* e = getenv("EGS_DRAW_LDS_PAD"); return e ? (size_t)atoi(e) : (size_t)0; }(),
      [] { const char* e = getenv("EGS_DRAWB_LDS_PAD"); return e ? (size_t)atoi(e) : (size_t)0; }()};
  return pad[which];
}
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
// evaluates the exponent as a polynomial about the tile centre (below), the backward kernel
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
// (alpha = 1 - T_final) and adds T_final * bg to the image.  k_draw is the EXTRA = false instance of this body.
template <bool BOX, bool FLOOR, bool CLAMP, bool SKIP>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu((!BOX && SKIP) ? 8 : 6, 8))) void k_draw(DrawParams p, int32_t* __restrict__ ranges,
                                             const int32_t* __restrict__ gsid,
                                             const float4* __restrict__ rec, float* __restrict__ image,
                                             int32_t* __restrict__ contrib, float* __restrict__ final_tau) {
  // staged entry: 12 floats (BOX: three b128 pieces) or 10 (two b128 + one b64: an entry's broadcast reads are
  // 50 of the ~130 SIMD cycles it costs, on an LDS pipe the CU's four SIMDs share; b64 is half a b128)
  // (the third piece keeps the 16-B slot stride: all three reads are immediate offsets from ONE address register)
  __shared__ float4 sA[64], sB[64], sC[64];
  constexpr bool EXTRA = false;
  const DrawExtras ex = {};
  float* const sZ = nullptr;
#include "egs_draw_fwd.inc"
}
// the EXTRA flavour: non-BOX entries carry z in the free pair of their third piece (11 floats), BOX entries in sZ.
// k_draw's occupancy cap kept: at eight waves the depth accumulators spill 16 B per lane outside the blend loop, and that
// is faster than six waves without spills (bench scene: 166 against 197 us)
template <bool BOX, bool FLOOR, bool CLAMP, bool SKIP>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu((!BOX && SKIP) ? 8 : 6, 8))) void k_draw_extra(DrawParams p, int32_t* __restrict__ ranges,
                                             const int32_t* __restrict__ gsid,
                                             const float4* __restrict__ rec, float* __restrict__ image,
                                             int32_t* __restrict__ contrib, float* __restrict__ final_tau,
                                             DrawExtras ex) {
  __shared__ float4 sA[64], sB[64], sC[64];
  __shared__ float sZ[BOX ? 64 : 1];
  constexpr bool EXTRA = true;
#include "egs_draw_fwd.inc"
}

// ============================================================================
// draw backward: per-tile back-to-front gradients        (reference kernel.cu:809-950)
// ============================================================================
// gfx950 cross-half / cross-row swaps (v_permlane32_swap_b32, v_permlane16_swap_b32)
__device__ __forceinline__ void swap32(float& a, float& b) {  // a[32..63] <-> b[0..31]
  auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
  a = __uint_as_float(r[0]);
  b = __uint_as_float(r[1]);
}
__device__ __forceinline__ void swap16(float& a, float& b) {  // odd rows of a <-> even rows of b
  auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
  a = __uint_as_float(r[0]);
  b = __uint_as_float(r[1]);
}
// ---- transposing wave reduction ------------------------------------------------------------------
// 4 entries x 9 quantities = 36 per-lane partials have to become 36 wave totals.  Every step pairs two
// registers, sends half of each to the partner lanes and adds: one output register per input pair, so the
// register count halves with the lane span (36 -> 18 -> 9 across the 16-lane rows with
// v_permlane32_swap / v_permlane16_swap, then 9 -> 5 -> 3 -> 2 -> 1 inside the rows with DPP mirrors).
// 54 + 27 instructions instead of 36 x 6 DPP adds, and the nine totals of an entry land in nine
// different lanes of its row -- exactly where the one-instruction atomic wants them.
__device__ __forceinline__ float rows_of4(float e0, float e1, float e2, float e3) {
  swap32(e0, e1);
  const float s01 = e0 + e1;  // lanes 0-31: e0 halves, lanes 32-63: e1 halves
  swap32(e2, e3);
  const float s23 = e2 + e3;
  float a = s01, b = s23;
  swap16(a, b);               // rows of a: [e0, e2, e1, e3]; rows of b: the other halves
  return a + b;               // row r: 16 partial sums of entry {0,2,1,3}[r]
}
template <int CTRL>
__device__ __forceinline__ float dpp_get(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
// `hi` lanes reduce b, the others reduce a; partner lane through the mirror CTRL (a bijection between
// the two lane classes)
template <int CTRL>
__device__ __forceinline__ float merge2(float a, float b, bool hi) {
  const float own = hi ? b : a, other = hi ? a : b;
  return own + dpp_get<CTRL>(other);
}
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
template <int NQ>
__device__ __forceinline__ float rows_to_lanes9(const float (&q)[NQ], int c16) {
  const bool h8 = (c16 & 8) != 0, h4 = (c16 & 4) != 0, h2 = (c16 & 2) != 0, h1 = (c16 & 1) != 0;
  constexpr int M8 = 0x140, M4 = 0x141, M2 = 0x4E, M1 = 0xB1;  // row_mirror, row_half_mirror, quad [2,3,0,1], [1,0,3,2]
  const float p01 = merge2<M8>(q[0], q[1], h8), p23 = merge2<M8>(q[2], q[3], h8);
  const float p45 = merge2<M8>(q[4], q[5], h8), p67 = merge2<M8>(q[6], q[7], h8);
  if constexpr (NQ == 10) {
    const float a = merge2<M4>(p01, p23, h4), b = merge2<M4>(p45, p67, h4);
    return odd_lanes_tail(q, merge2<M2>(a, b, h2), h2, h1);
  } else {
    float s8 = q[8] + dpp_get<M8>(q[8]);
    const float a = merge2<M4>(p01, p23, h4), b = merge2<M4>(p45, p67, h4);
    s8 += dpp_get<M4>(s8);
    const float r = merge2<M2>(a, b, h2);
    s8 += dpp_get<M2>(s8);
    return merge2<M1>(r, s8, h1);
  }
}

// ---- the in-row stage without selects ----------------------------------------------------------------------
// Measured on gfx950 (tools/ubench_calib.hip, cycles per wave instruction per SIMD): add / mul / fma 2.5 (full
// rate); DPP, v_cndmask, v_med3, v_min/max, v_cmp, v_readlane, v_mov_b64 4.3 (half rate); v_permlane{32,16}_swap,
// v_exp, v_rcp 8.4 (quarter rate); ds_swizzle 8.2 and ds_bpermute 24 (the LDS crossbar is shared by the four SIMDs
// of a CU: moving the cross-row exchanges there was measured 10 % SLOWER, so they stay v_permlane swaps).
// merge2 above costs two v_cndmask and a DPP add.  The first two levels split the row by lane bits 3 and 2 --
// exactly what DPP's bank mask addresses (a bank = four consecutive lanes of a row): one DPP add for everybody,
// one bank-masked DPP add for the lanes that reduce the second register; no select.
// out = a + a[mirror] everywhere, then b + b[mirror] on the banks of `bank_hi`
#define EGS_MERGE_BANK(out, a, b, ctrl, bank_hi)                                                              \
  do {                                                                                                        \
    asm("v_add_f32_dpp %0, %1, %1 " ctrl " row_mask:0xf bank_mask:0xf" : "=v"(out) : "v"(a));                  \
    asm("v_add_f32_dpp %0, %1, %1 " ctrl " row_mask:0xf bank_mask:" bank_hi : "+v"(out) : "v"(b));            \
  } while (0)
// same result layout as rows_to_lanes9: totals in lanes {0, 8, 4, 12, 2, 10, 6, 14, odd} of every row
template <int NQ>
__device__ __forceinline__ float rows_to_lanes9_bank(const float (&q)[NQ], int c16) {
  const bool h2 = (c16 & 2) != 0, h1 = (c16 & 1) != 0;
  constexpr int M8 = 0x140, M4 = 0x141, M2 = 0x4E, M1 = 0xB1;
  float p01, p23, p45, p67, a, b;
  EGS_MERGE_BANK(p01, q[0], q[1], "row_mirror", "0xc");        // lanes 8..15 (banks 2, 3) reduce the second one
  EGS_MERGE_BANK(p23, q[2], q[3], "row_mirror", "0xc");
  EGS_MERGE_BANK(p45, q[4], q[5], "row_mirror", "0xc");
  EGS_MERGE_BANK(p67, q[6], q[7], "row_mirror", "0xc");
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
template <bool BOX, bool FLOOR, bool CLAMP, int RED, bool SEG = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 8))) void k_draw_bwd(DrawParams p, const int32_t* __restrict__ ranges,
                                                 const int32_t* __restrict__ gsid,
                                                 const float4* __restrict__ rec,
                                                 const float* __restrict__ final_tau,
                                                 const int32_t* __restrict__ contrib,
                                                 const float* __restrict__ dLdg,
                                                 float* __restrict__ gpack, SegArgs sg) {
  __shared__ float4 sA[64], sB[64], sC[64], sD[64];  // sD = {cinv.x, cinv.y, cinv.z, gsid}
  __shared__ float4 szero[3];                        // a line of zeros (see the accumulator reset below)
  constexpr bool EXTRA = false;
  const DrawExtras ex = {};
  float* const sZ = nullptr;
#include "egs_draw_bwd.inc"
}
// the EXTRA flavour (unsplit lists only): z of the staged entries in sZ, next to sD.  Four waves per SIMD (111-114
// VGPRs): under k_draw_bwd's cap of five the tenth partial and the per-pixel dL/ddepth spill 44-60 B per lane, and that
// is slower (bench scene: 531 against 494 us)
template <bool BOX, bool FLOOR, bool CLAMP, int RED>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 8))) void k_draw_bwd_extra(DrawParams p, const int32_t* __restrict__ ranges,
                                                 const int32_t* __restrict__ gsid,
                                                 const float4* __restrict__ rec,
                                                 const float* __restrict__ final_tau,
                                                 const int32_t* __restrict__ contrib,
                                                 const float* __restrict__ dLdg,
                                                 float* __restrict__ gpack, DrawExtras ex) {
  __shared__ float4 sA[64], sB[64], sC[64], sD[64];
  __shared__ float4 szero[3];
  __shared__ float sZ[64];
  constexpr bool SEG = false, EXTRA = true;
  const SegArgs sg = {};
#include "egs_draw_bwd.inc"
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
  // with the plain map (580 vs 595 us).  EGS_TILE_MAP=0|1|2 overrides both (tuning knob).
  static const int forced = [] {
    const char* e = getenv("EGS_TILE_MAP");
    return e ? atoi(e) : -1;
  }();
  p.map_mode = forced >= 0 ? forced : (backward ? 0 : 2);
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

// Longest-list-first dispatch (k_tile_order) for one of the draw kernels: which = 0 forward, 1 backward.
// Mode by measurement (same-box A/B at 1 M / 1080p); EGS_TILE_ORDER_F / _B = 0..4 and
// EGS_TILE_SERP override (tuning knobs).
int tile_order_mode(int which) {
  static const int mode[2] = {
      [] { const char* e = getenv("EGS_TILE_ORDER_F"); return e ? atoi(e) : EGS_TILE_ORDER_F_DEFAULT; }(),
      [] { const char* e = getenv("EGS_TILE_ORDER_B"); return e ? atoi(e) : EGS_TILE_ORDER_B_DEFAULT; }()};
  return mode[which];
}
int tile_order_enqueue(DrawParams& p, int which, int32_t* buf, size_t buf_len, const int32_t* ranges, hipStream_t s,
                       const int32_t* work, const int32_t* walk, uint32_t* hint) {
  const int mode = tile_order_mode(which);
  if (mode <= 0 || !buf) return 0;
  const bool per_xcd = mode >= 3;
  const int ngrid = per_xcd ? tile_order_len(p.gx, p.gy) : p.T;
  if ((size_t)ngrid > buf_len || p.T > TILE_ORDER_MAX_T) return 0;   // (larger images keep the plain map)
  static const int serp = [] { const char* e = getenv("EGS_TILE_SERP"); return e ? atoi(e) : 0; }();
  const int period = serp > 0 ? serp : (per_xcd ? 128 : 1024);   // SIMDs per XCD / per chip
  EGS_LAUNCH("k_tile_order", k_tile_order, dim3(1), dim3(1024), s, ranges, work, p.T, p.gx, mode, period, buf, ngrid,
             walk, hint);
  EGS_LAUNCH_OK();
  p.order = buf;
  p.ngrid = ngrid;
  return 0;
}

int tile_work_from_contrib(const DrawParams& p, const int32_t* contrib, int32_t* work, int32_t* walk, hipStream_t s) {
  if (work) EGS_LAUNCH("k_tile_work", k_tile_work, dim3(p.T), dim3(64), s, p.W, p.H, p.gx, contrib, work, walk);
  else EGS_LAUNCH("k_tile_walk", k_tile_walk, dim3(p.T), dim3(64), s, p.W, p.H, p.gx, contrib, walk);
  EGS_LAUNCH_OK();
  return 0;
}

// policy -> template instance (compile-time footprint / floor / clamp)
int launch_draw_extra(const DrawParams& dp, const EgsPolicy* pol, int32_t* ranges, const int32_t* gsid,
                      const float4* rec, float* image, int32_t* contrib, float* final_tau, const DrawExtras& ex,
                      hipStream_t s) {
#define EGS_DRAWX(BOX, FLOOR, CLAMP)                                                                               \
  do {                                                                                                             \
    if (pol->alpha_skip > 0.f)                                                                                     \
      EGS_LAUNCH_LDS("k_draw_extra", (k_draw_extra<BOX, FLOOR, CLAMP, true>), dim3(draw_grid(dp)), dim3(64),       \
                     draw_lds_pad(0), s, dp, ranges, gsid, rec, image, contrib, final_tau, ex);                   \
    else                                                                                                           \
      EGS_LAUNCH_LDS("k_draw_extra", (k_draw_extra<BOX, FLOOR, CLAMP, false>), dim3(draw_grid(dp)), dim3(64),      \
                     draw_lds_pad(0), s, dp, ranges, gsid, rec, image, contrib, final_tau, ex);                   \
  } while (0)
  const int sel = (pol->footprint == 1 ? 4 : 0) | (pol->maha_floor ? 2 : 0) | (pol->alpha_clamp ? 1 : 0);
  switch (sel) {
    case 0: EGS_DRAWX(false, false, false); break;
    case 1: EGS_DRAWX(false, false, true); break;
    case 2: EGS_DRAWX(false, true, false); break;
    case 3: EGS_DRAWX(false, true, true); break;
    case 4: EGS_DRAWX(true, false, false); break;
    case 5: EGS_DRAWX(true, false, true); break;
    case 6: EGS_DRAWX(true, true, false); break;
    default: EGS_DRAWX(true, true, true); break;
  }
#undef EGS_DRAWX
  EGS_LAUNCH_OK();
  return 0;
}

int launch_draw(const DrawParams& dp, const EgsPolicy* pol, int32_t* ranges, const int32_t* gsid, const float4* rec,
                float* image, int32_t* contrib, float* final_tau, hipStream_t s) {
#define EGS_DRAW(BOX, FLOOR, CLAMP)                                                                                \
  do {                                                                                                             \
    if (pol->alpha_skip > 0.f)                                                                                     \
      EGS_LAUNCH_LDS("k_draw", (k_draw<BOX, FLOOR, CLAMP, true>), dim3(draw_grid(dp)), dim3(64), draw_lds_pad(0), s, \
                     dp, ranges, gsid, rec, image, contrib, final_tau);                                            \
    else                                                                                                           \
      EGS_LAUNCH_LDS("k_draw", (k_draw<BOX, FLOOR, CLAMP, false>), dim3(draw_grid(dp)), dim3(64), draw_lds_pad(0), s, \
                     dp, ranges, gsid, rec, image, contrib, final_tau);                                            \
  } while (0)
  const int sel = (pol->footprint == 1 ? 4 : 0) | (pol->maha_floor ? 2 : 0) | (pol->alpha_clamp ? 1 : 0);
  switch (sel) {
    case 0: EGS_DRAW(false, false, false); break;
    case 1: EGS_DRAW(false, false, true); break;
    case 2: EGS_DRAW(false, true, false); break;
    case 3: EGS_DRAW(false, true, true); break;
    case 4: EGS_DRAW(true, false, false); break;
    case 5: EGS_DRAW(true, false, true); break;
    case 6: EGS_DRAW(true, true, false); break;
    default: EGS_DRAW(true, true, true); break;
  }
#undef EGS_DRAW
  EGS_LAUNCH_OK();
  return 0;
}

int launch_draw_bwd(const DrawParams& dp, const EgsPolicy* pol, const int32_t* ranges, const int32_t* gsid,
                    const float4* rec, const float* final_tau, const int32_t* contrib, const float* dLdg, float* gpack,
                    hipStream_t s) {
  // variants of the backward kernel (bit 0: in-row merges of the wave reduction with bank-masked DPP adds instead
  // of selects; bit 1: accumulator zeros loaded from LDS instead of moved; bit 2: exponent per evaluated block);
  // EGS_DRAWB_RED = 0 | 3 | 7 overrides
  static const int red = [] { const char* e = getenv("EGS_DRAWB_RED"); return e ? atoi(e) : EGS_DRAWB_RED_DEFAULT; }();
  const SegArgs nosg = {};
#define EGS_DRAWB(BOX, FLOOR, CLAMP)                                                                               \
  do {                                                                                                             \
    if (red == 0)                                                                                                  \
      EGS_LAUNCH_LDS("k_draw_bwd", (k_draw_bwd<BOX, FLOOR, CLAMP, 0>), dim3(draw_grid(dp)), dim3(64), draw_lds_pad(1), \
                     s, dp, ranges, gsid, rec, final_tau, contrib, dLdg, gpack, nosg);                             \
    else if (red == 3)                                                                                             \
      EGS_LAUNCH_LDS("k_draw_bwd", (k_draw_bwd<BOX, FLOOR, CLAMP, 3>), dim3(draw_grid(dp)), dim3(64), draw_lds_pad(1), \
                     s, dp, ranges, gsid, rec, final_tau, contrib, dLdg, gpack, nosg);                             \
    else                                                                                                           \
      EGS_LAUNCH_LDS("k_draw_bwd", (k_draw_bwd<BOX, FLOOR, CLAMP, 7>), dim3(draw_grid(dp)), dim3(64), draw_lds_pad(1), \
                     s, dp, ranges, gsid, rec, final_tau, contrib, dLdg, gpack, nosg);                             \
  } while (0)
  const int sel = (pol->footprint == 1 ? 4 : 0) | (pol->maha_floor ? 2 : 0) | (pol->alpha_clamp ? 1 : 0);
  switch (sel) {
    case 0: EGS_DRAWB(false, false, false); break;
    case 1: EGS_DRAWB(false, false, true); break;
    case 2: EGS_DRAWB(false, true, false); break;
    case 3: EGS_DRAWB(false, true, true); break;
    case 4: EGS_DRAWB(true, false, false); break;
    case 5: EGS_DRAWB(true, false, true); break;
    case 6: EGS_DRAWB(true, true, false); break;
    default: EGS_DRAWB(true, true, true); break;
  }
#undef EGS_DRAWB
  EGS_LAUNCH_OK();
  return 0;
}

// (the EXTRA flavour exists in the default reduction variant only: EGS_DRAWB_RED is an A/B knob of the plain kernel)
int launch_draw_bwd_extra(const DrawParams& dp, const EgsPolicy* pol, const int32_t* ranges, const int32_t* gsid,
                          const float4* rec, const float* final_tau, const int32_t* contrib, const float* dLdg,
                          float* gpack, const DrawExtras& ex, hipStream_t s) {
#define EGS_DRAWBX(BOX, FLOOR, CLAMP)                                                                              \
  EGS_LAUNCH_LDS("k_draw_bwd_extra", (k_draw_bwd_extra<BOX, FLOOR, CLAMP, EGS_DRAWB_RED_DEFAULT>), dim3(draw_grid(dp)), \
                 dim3(64), draw_lds_pad(1), s, dp, ranges, gsid, rec, final_tau, contrib, dLdg, gpack, ex)
  const int sel = (pol->footprint == 1 ? 4 : 0) | (pol->maha_floor ? 2 : 0) | (pol->alpha_clamp ? 1 : 0);
  switch (sel) {
    case 0: EGS_DRAWBX(false, false, false); break;
    case 1: EGS_DRAWBX(false, false, true); break;
    case 2: EGS_DRAWBX(false, true, false); break;
    case 3: EGS_DRAWBX(false, true, true); break;
    case 4: EGS_DRAWBX(true, false, false); break;
    case 5: EGS_DRAWBX(true, false, true); break;
    case 6: EGS_DRAWBX(true, true, false); break;
    default: EGS_DRAWBX(true, true, true); break;
  }
#undef EGS_DRAWBX
  EGS_LAUNCH_OK();
  return 0;
}

int launch_draw_bwd_seg(const DrawParams& dp, const EgsPolicy* pol, const int32_t* ranges, const int32_t* gsid,
                        const float4* rec, const float* final_tau, const int32_t* contrib, const float* dLdg,
                        float* gpack, const SegArgs& sga, int grid, hipStream_t s) {
#define EGS_DRAWBS(FLOOR, CLAMP)                                                                                   \
  EGS_LAUNCH("k_draw_bwd_seg", (k_draw_bwd<false, FLOOR, CLAMP, 7, true>), dim3(grid), dim3(64), s, dp, ranges, gsid, \
             rec, final_tau, contrib, dLdg, gpack, sga)
  switch ((pol->maha_floor ? 2 : 0) | (pol->alpha_clamp ? 1 : 0)) {
    case 0: EGS_DRAWBS(false, false); break;
    case 1: EGS_DRAWBS(false, true); break;
    case 2: EGS_DRAWBS(true, false); break;
    default: EGS_DRAWBS(true, true); break;
  }
#undef EGS_DRAWBS
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

// a caller-held tile_order buffer: [dispatch order of the forward draw | per-tile work it measured | walk (T ints each)]
extern "C" size_t egs_tile_order_len(int width, int height) {
  const int gx = egs::div_up(width, EGS_TILE), gy = egs::div_up(height, EGS_TILE);
  return (size_t)egs::tile_order_len(gx, gy) + 2 * (size_t)gx * gy;
}
