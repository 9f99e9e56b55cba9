// The walk over the tile lists of a finished forward pass that k_blend_weights (egs_prune.hip), k_feature_render and
// k_feature_gather (egs_feat.hip) share -- k_draw's walk without colours, bounded by the forward's `contrib` as
// k_draw_bwd's is -- and what their entry points share on the host.  The parameter struct is a template argument: the
// helpers read N, W, H, lskip, nan_blend and masked (the host part also writes gx and T); each library keeps its own
// layout.
//
// 64-entry chunks are staged in LDS by the lane that owns the entry: the conic, the cap, the polynomial about the tile
// centre and (BOX) the pixel box -- no colours.  The exponent is k_draw's (same polynomial, same fmaf order, log2 alpha
// from the record's threshold, one min against the cap), so the tau formed here is the forward's tau and the skip
// decisions agree with it.  Entry i is live at a pixel iff i < contrib there: tau only falls, so every entry in front of
// a pixel's last contributor met `tau >= tau_stop` in the forward pass, and none behind it hit.
#pragma once
#include <math.h>

#include "egs_draw_device.h"
#include "egs_side_error.h"

namespace egs {

// One wave64 per 16x16 tile, four pixels per lane: pixel k = 2 by + bx of lane l is (tx0 + (l & 7) + 8 bx,
// ty0 + (l >> 3) + 8 by), k_draw's mapping.
struct Lane {
  int pxb[2], pyb[2];
  int cont[4];     // contrib of the lane's four pixels (0 outside the image)
  int bmax[4];     // wave-uniform: largest contrib of block k -> entries >= bmax[k] are inert for it
  int maxcont;     // wave-uniform: the tile is walked to here and no further (0: nothing to walk)
  float X[2], Y[2], XX[2], YY[2], XY[4];
};

template <typename P>
__device__ __forceinline__ void lane_init(Lane& L, const P& p, int tx0, int ty0, int lane, int n,
                                          const int32_t* __restrict__ contrib) {
  L.pxb[0] = tx0 + (lane & 7); L.pxb[1] = L.pxb[0] + 8;
  L.pyb[0] = ty0 + (lane >> 3); L.pyb[1] = L.pyb[0] + 8;
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
  L.X[0] = (float)(lane & 7) - 7.5f; L.X[1] = (float)(lane & 7) + 0.5f;
  L.Y[0] = (float)(lane >> 3) - 7.5f; L.Y[1] = (float)(lane >> 3) + 0.5f;
#pragma unroll
  for (int b = 0; b < 2; ++b) { L.XX[b] = L.X[b] * L.X[b]; L.YY[b] = L.Y[b] * L.Y[b]; }
#pragma unroll
  for (int k = 0; k < 4; ++k) L.XY[k] = L.X[k & 1] * L.Y[k >> 1];
}

// The staging lane's share of a 64-entry chunk: the conic, the cap, the polynomial about the tile centre and (BOX) the
// pixel box go to LDS; returns the entry's 4-bit reach mask with the blocks it lies behind cleared (0: nobody walks it)
// and the Gaussian index in `g` (valid iff the mask is not 0).
template <bool BOX, bool FLOOR, bool CLAMP, bool SKIP, typename P>
__device__ __forceinline__ int stage_entry(const P& p, const Lane& L, int idx, int gm, int tx0, int ty0,
                                           const float4* __restrict__ rec, float4* sA, float4* sB, float* sC, int lane,
                                           int& g) {
  constexpr float L99 = -0.014499569695115089f;  // log2(0.99)
  int mymask = 0;
  g = p.masked ? (int)((uint32_t)gm & EGS_GSID_MASK) : gm;
  if ((unsigned)g < (unsigned)p.N) {
    float4 A = rec[3 * (size_t)g], B = rec[3 * (size_t)g + 1];
    const float4 C = rec[3 * (size_t)g + 2];
    const bool nanfix = p.nan_blend && nan_entry_fix(A, B);
    if (C.w < INFINITY) mymask = p.masked ? (int)((uint32_t)gm >> EGS_GSID_BITS) : reach_mask<BOX>(A, C, tx0, ty0);
    if (nanfix && !BOX && !p.masked && C.w < INFINITY) mymask = 0xF;
    const float la = SKIP ? p.lskip - C.w : __builtin_amdgcn_logf(B.y);
    float cap = 3.0e38f;
    if (FLOOR) cap = CLAMP ? fminf(la, L99) : la;
    else if (CLAMP) cap = L99;
    const float cx0 = (float)tx0 + 7.5f, cy0 = (float)ty0 + 7.5f;
    const float Dx = cx0 - A.x, Dy = cy0 - A.y;
    const float c0 = la + (A.z * Dx * Dx + A.w * Dx * Dy + B.x * Dy * Dy);
    const float c1 = 2.f * A.z * Dx + A.w * Dy, c2 = 2.f * B.x * Dy + A.w * Dx;
    sA[lane] = make_float4(A.z, A.w, B.x, cap);
    sB[lane] = make_float4(c0, c1, c2, C.y);
    if constexpr (BOX) sC[lane] = C.z;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (idx >= L.bmax[k]) mymask &= ~(1 << k);   // no pixel of block k got this far
  return mymask;
}

// Entry j of the staged chunk (index i of the tile list) at the lane's four pixels: k_draw's exponent (same polynomial,
// same fmaf order, one min against the cap), live iff i < contrib, a hit iff live and not below the skip threshold.  On a
// hit of pixel K: w = tau alpha', tau -= w, on_hit(integral_constant<K>, w).  -> the lane hit somewhere
template <int K, bool BOX, bool FLOOR, bool CLAMP, typename F>
__device__ __forceinline__ bool blend_pixel(const Lane& L, int reach, int i, const float4& Q, const float4& P, bool inbox,
                                            float lthr, float (&tau)[4], F&& on_hit) {
  constexpr int bx = K & 1, by = K >> 1;
  bool hit = false;
  if (reach & (1 << K)) {  // scalar branch: block K is in reach and some pixel of it got this far
    float ex = fmaf(P.z, L.Y[by], P.x);
    ex = fmaf(P.y, L.X[bx], ex);
    ex = fmaf(Q.z, L.YY[by], ex);
    ex = fmaf(Q.y, L.XY[K], ex);
    ex = fmaf(Q.x, L.XX[bx], ex);
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
