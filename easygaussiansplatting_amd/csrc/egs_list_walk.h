// The walk over the tile lists of a finished forward pass that k_blend_weights (egs_prune.hip), k_feature_render and
// k_feature_gather (egs_feat.hip) share -- k_draw's walk without colours, bounded by the forward's `contrib` as
// k_draw_bwd's is -- and what their entry points share on the host.  The parameter struct is a template argument: the
// helpers read N, W, H, lskip, nan_blend and masked (the host part also writes gx and T); each library keeps its own
// layout.
//
// 64-entry chunks are staged in LDS by the lane that owns the entry: the conic, the cap, the polynomial about the tile
// centre and (BOX) the pixel box -- no colours.  The exponent is k_draw's, from the same two functions (stage_math and
// pixel_exponent of egs_draw_device.h), so the tau formed here is the forward's tau and the skip decisions agree with it.
// Entry i is live at a pixel iff i < contrib there: tau only falls, so every entry in front of a pixel's last
// contributor met `tau >= tau_stop` in the forward pass, and none behind it hit.
#pragma once
#include <math.h>

#include "egs_draw_device.h"
#include "egs_side_error.h"

namespace egs {

// One wave64 per 16x16 tile, four pixels per lane: k_draw's mapping and monomials (TileLane) and what bounds this walk.
struct Lane : TileLane {
  int cont[4];     // contrib of the lane's four pixels (0 outside the image)
  int bmax[4];     // wave-uniform: largest contrib of block k -> entries >= bmax[k] are inert for it
  int maxcont;     // wave-uniform: the tile is walked to here and no further (0: nothing to walk)
};

template <typename P>
__device__ __forceinline__ void lane_init(Lane& L, const P& p, int tx0, int ty0, int lane, int n,
                                          const int32_t* __restrict__ contrib) {
  tile_lane_init(L, tx0, ty0, lane);
  L.maxcont = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int px = L.pxb[k & 1], py = L.pyb[k >> 1];
    L.cont[k] = (n > 0 && px < p.W && py < p.H) ? contrib[(size_t)py * p.W + px] : 0;
    int mx = L.cont[k];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mx = max(mx, __shfl_xor(mx, d, 64));
    L.bmax[k] = __builtin_amdgcn_readfirstlane(max(min(mx, n), 0));
    L.maxcont = max(L.maxcont, L.bmax[k]);
  }
}

// The staging lane's share of a 64-entry chunk: the conic, the cap, the polynomial about the tile centre and (BOX) the
// pixel box go to LDS; returns the entry's 4-bit reach mask with the blocks it lies behind cleared (0: nobody walks it)
// and the Gaussian index in `g` (valid iff the mask is not 0).
template <bool BOX, bool FLOOR, bool CLAMP, bool SKIP, typename P>
__device__ __forceinline__ int stage_entry(const P& p, const Lane& L, int idx, int gm, int tx0, int ty0,
                                           const float4* __restrict__ rec, float4* sA, float4* sB, float* sC, int lane,
                                           int& g) {
  int mymask = 0;
  g = p.masked ? (int)((uint32_t)gm & EGS_GSID_MASK) : gm;
  if ((unsigned)g < (unsigned)p.N) {
    const float4 A = rec[3 * (size_t)g], B = rec[3 * (size_t)g + 1], C = rec[3 * (size_t)g + 2];
    float4 Q;
    float c0, c1, c2;
    mymask = stage_math<BOX, FLOOR, CLAMP, SKIP>(A, B, C, gm, tx0, ty0, (float)tx0 + 7.5f, (float)ty0 + 7.5f, p.lskip,
                                                 p.masked, p.nan_blend, Q, c0, c1, c2);
    sA[lane] = Q;
    sB[lane] = make_float4(c0, c1, c2, C.y);
    if constexpr (BOX) sC[lane] = C.z;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (idx >= L.bmax[k]) mymask &= ~(1 << k);   // no pixel of block k got this far
  return mymask;
}

// Entry j of the staged chunk (index i of the tile list) at the lane's four pixels: k_draw's exponent (pixel_exponent, one
// min against the cap), live iff i < contrib, a hit iff live and not below the skip threshold.  On a
// hit of pixel K: w = tau alpha', tau -= w, on_hit(integral_constant<K>, w).  -> the lane hit somewhere
template <int K, bool BOX, bool FLOOR, bool CLAMP, typename F>
__device__ __forceinline__ bool blend_pixel(const Lane& L, int reach, int i, const float4& Q, const float4& P, bool inbox,
                                            float lthr, float (&tau)[4], F&& on_hit) {
  bool hit = false;
  if (reach & (1 << K)) {  // scalar branch: block K is in reach and some pixel of it got this far
    float ex = pixel_exponent(L, K, Q, P);
    hit = (i < L.cont[K]) && (ex >= lthr);
    if (BOX) hit = hit && inbox;
    if (hit) {
      if (FLOOR || CLAMP) ex = min_hi(ex, Q.w);
      const float w = tau[K] * __builtin_amdgcn_exp2f(ex);
      tau[K] -= w;
      on_hit(std::integral_constant<int, K>{}, w);
    }
  }
  return hit;
}

template <bool BOX, bool FLOOR, bool CLAMP, typename F>
__device__ __forceinline__ bool blend_entry(const Lane& L, int reach, int i, int j, const float4* sA, const float4* sB,
                                            const float* sC, float lthr, float (&tau)[4], F&& on_hit) {
  const float4 Q = sA[j], P = sB[j];            // wave-uniform address: LDS broadcast
  bool inx[2] = {true, true}, iny[2] = {true, true};
  if (BOX) {
    const uint32_t bx = __float_as_uint(P.w), by = __float_as_uint(sC[j]);
    const int x0 = bx & 0xFFFF, x1 = bx >> 16, y0 = by & 0xFFFF, y1 = by >> 16;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      inx[b] = (L.pxb[b] >= x0) && (L.pxb[b] < x1);
      iny[b] = (L.pyb[b] >= y0) && (L.pyb[b] < y1);
    }
  }
  bool anyhit = blend_pixel<0, BOX, FLOOR, CLAMP>(L, reach, i, Q, P, inx[0] && iny[0], lthr, tau, on_hit);
  anyhit |= blend_pixel<1, BOX, FLOOR, CLAMP>(L, reach, i, Q, P, inx[1] && iny[0], lthr, tau, on_hit);
  anyhit |= blend_pixel<2, BOX, FLOOR, CLAMP>(L, reach, i, Q, P, inx[0] && iny[1], lthr, tau, on_hit);
  anyhit |= blend_pixel<3, BOX, FLOOR, CLAMP>(L, reach, i, Q, P, inx[1] && iny[1], lthr, tau, on_hit);
  return anyhit;
}

// ---- host: what the entry points over these lists share -----------------------------------------------------------------
// Checked for every call, the empty one (n == 0) included.
static int check_view(int n, int width, int height, const EgsPolicy* pol, int flags) {
  SIDE_CHECK_ARG(n >= 0);
  SIDE_CHECK_ARG(width > 0 && height > 0);
  SIDE_CHECK_ARG((flags & ~EGS_DRAW_MASKED_LISTS) == 0);
  SIDE_CHECK_ARG(pol != nullptr);
  return 0;
}

// Checked once there is something to walk (n > 0).
static int check_lists(int n, const float* rec, const int32_t* ranges, const int32_t* gsid, const int32_t* contrib,
                       int flags) {
  SIDE_CHECK_ARG(rec != nullptr && ((uintptr_t)rec & 15) == 0);
  SIDE_CHECK_ARG(ranges != nullptr && ((uintptr_t)ranges & 3) == 0);
  SIDE_CHECK_ARG(gsid != nullptr && ((uintptr_t)gsid & 3) == 0);
  SIDE_CHECK_ARG(contrib != nullptr && ((uintptr_t)contrib & 3) == 0);
  SIDE_CHECK_ARG(!(flags & EGS_DRAW_MASKED_LISTS) || n < (1 << EGS_GSID_BITS));
  return 0;
}

template <typename P>
static void fill_params(P& p, int n, int width, int height, const EgsPolicy* pol, int flags) {
  p.N = n; p.W = width; p.H = height;
  p.gx = div_up(width, EGS_TILE);
  p.T = p.gx * div_up(height, EGS_TILE);
  p.lskip = pol->alpha_skip > 0.f ? log2f(pol->alpha_skip) : -INFINITY;
  p.nan_blend = pol->nan_maha == 0 && pol->maha_floor;
  p.masked = (flags & EGS_DRAW_MASKED_LISTS) != 0;
}

// f(box, floor, clamp, skip) with the policy's four flags as std::true_type / std::false_type: the kernels' <BOX, FLOOR,
// CLAMP, SKIP>
template <typename F>
static void with_policy(const EgsPolicy* pol, F&& f) {
  with_bools(f, pol->footprint == 1, pol->maha_floor != 0, pol->alpha_clamp != 0, pol->alpha_skip > 0.f);
}

}  // namespace egs
