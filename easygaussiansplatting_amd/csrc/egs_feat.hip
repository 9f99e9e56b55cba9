// Per-Gaussian feature vectors through the tile lists of a finished forward pass, for gfx950 (include/egs_feat.h has the
// contract): k_feature_render blends C channels with the forward's weights w = tau alpha', k_feature_gather is its
// adjoint.  Both walk a tile exactly as k_blend_weights (egs_prune.hip) does -- k_draw's walk, bounded by the forward's
// `contrib` as k_draw_bwd's is -- so no stop decision is derived again and the weights are the forward's.
//
// Built into libegs_feat.so, a library of its own: it shares headers with libegs_hip.so (the reach mask, the NaN rule
// and the one-instruction min of the draw kernels) but no symbol, and keeps its own last-error string.  The reduction
// helpers (swap32, swap16, rows_of4) restate those of egs_prune.hip.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "egs_draw_device.h"
#include "../../include/egs_feat.h"

namespace egs_feat {

static thread_local char g_err[512] = "no error";

static void set_error(int code, const char* what, const char* file, int line) {
  const char* base = strrchr(file, '/');
  snprintf(g_err, sizeof(g_err), "egs_feat error %d: %s (%s:%d)", code, what ? what : "?", base ? base + 1 : file, line);
}

#define FEAT_CHECK_ARG(cond)                                                             \
  do {                                                                                   \
    if (!(cond)) {                                                                       \
      ::egs_feat::set_error(EGS_ERR_BAD_ARG, "bad argument: " #cond, __FILE__, __LINE__); \
      return EGS_ERR_BAD_ARG;                                                            \
    }                                                                                    \
  } while (0)

#define FEAT_HIP(expr)                                                              \
  do {                                                                              \
    hipError_t e__ = (expr);                                                        \
    if (e__ != hipSuccess) {                                                        \
      ::egs_feat::set_error((int)e__, hipGetErrorString(e__), __FILE__, __LINE__);  \
      return (int)e__;                                                              \
    }                                                                               \
  } while (0)

using egs::div_up;
using egs::min_hi;
using egs::nan_entry_fix;
using egs::reach_mask;
using egs::with_bools;

constexpr int CH = 8;   // channels per wave: one (tile, chunk of CH channels) per workgroup

struct FeatParams {
  int N, W, H, gx, T, C;
  float lskip;     // log2(alpha_skip), -inf when there is no skip test
  int nan_blend;   // as DrawParams.nan_blend
  int masked;      // the list values carry the tile's 4-bit block mask in their high bits
  int vec16;       // every feature row chunk is 16-byte aligned (render only)
};

// ---- transposing wave reduction of four entries (rows_of4 of k_draw_bwd / k_blend_weights, sums only) ---------------
// After the two swaps row r of the wave holds 16 partials of entry {0, 2, 1, 3}[r]; four DPP steps inside the row leave
// the total in every lane of it.
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
template <int CTRL>
__device__ __forceinline__ float dpp_get(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
__device__ __forceinline__ float rows_of4(float e0, float e1, float e2, float e3) {
  swap32(e0, e1);
  float a = e0 + e1;      // lanes 0-31: e0 halves, lanes 32-63: e1 halves
  swap32(e2, e3);
  float b = e2 + e3;
  swap16(a, b);           // rows of a: [e0, e2, e1, e3]; rows of b: the other halves
  float v = a + b;
  v += dpp_get<0x140>(v);   // row_mirror
  v += dpp_get<0x141>(v);   // row_half_mirror
  v += dpp_get<0x4E>(v);    // quad_perm [2, 3, 0, 1]
  v += dpp_get<0xB1>(v);    // quad_perm [1, 0, 3, 2]
  return v;
}

// ---- the walk both kernels share --------------------------------------------------------------------------------------
// One wave64 per 16x16 tile, four pixels per lane: pixel k = 2 by + bx of lane l is (tx0 + (l & 7) + 8 bx,
// ty0 + (l >> 3) + 8 by), k_draw's mapping.
struct Lane {
  int pxb[2], pyb[2];
  int cont[4];     // contrib of the lane's four pixels (0 outside the image)
  int bmax[4];     // wave-uniform: largest contrib of block k -> entries >= bmax[k] are inert for it
  int maxcont;     // wave-uniform: the tile is walked to here and no further (0: nothing to walk)
  float X[2], Y[2], XX[2], YY[2], XY[4];
};

__device__ __forceinline__ void lane_init(Lane& L, const FeatParams& p, int tx0, int ty0, int lane, int n,
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

// The staging lane's share of a 64-entry chunk, exactly as k_blend_weights stages it: the conic, the cap, the polynomial
// about the tile centre and (BOX) the pixel box go to LDS; returns the entry's 4-bit reach mask with the blocks it lies
// behind cleared (0: nobody walks it) and the Gaussian index in `g` (valid iff the mask is not 0).
template <bool BOX, bool FLOOR, bool CLAMP, bool SKIP>
__device__ __forceinline__ int stage_entry(const FeatParams& p, const Lane& L, int idx, int gm, int tx0, int ty0,
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

// ---- k_feature_render -------------------------------------------------------------------------------------------------
// Workgroup (tile, chunk): channels c0 = 8 chunk .. c0 + 7 of the tile's 256 pixels.  The staging lane also loads its
// entry's eight feature values into LDS (zeros beyond the last channel); the blend loop reads them back as wave-uniform
// broadcasts and does eight FMAs per hit pixel.  Every pixel of the tile inside the image is WRITTEN, zeros where the
// tile's list is empty: there is no early return.
template <bool BOX, bool FLOOR, bool CLAMP, bool SKIP>
__global__ __launch_bounds__(64) void k_feature_render(FeatParams p, const int32_t* __restrict__ ranges,
                                                       const int32_t* __restrict__ gsid,
                                                       const float4* __restrict__ rec,
                                                       const int32_t* __restrict__ contrib,
                                                       const float* __restrict__ feats, float* __restrict__ fmap) {
  __shared__ float4 sA[64], sB[64];       // (qxx, qxy, qyy, cap), (c0, c1, c2, x pixel box)
  __shared__ float sC[BOX ? 64 : 1];      // y pixel box
  __shared__ float4 sF[2][64];            // the entry's eight feature values
  const int tile = blockIdx.x, lane = threadIdx.x;
  const int c0 = blockIdx.y * CH;
  if (tile >= p.T || c0 >= p.C) return;
  int r0 = ranges[2 * (size_t)tile];
  int n = ranges[2 * (size_t)tile + 1] - r0;
  if (r0 < 0 || n <= 0) n = 0;            // an empty tile: nothing to walk, zeros to write
  const int tx0 = (tile % p.gx) * EGS_TILE, ty0 = (tile / p.gx) * EGS_TILE;
  Lane L;
  lane_init(L, p, tx0, ty0, lane, n, contrib);
  float tau[4] = {1.f, 1.f, 1.f, 1.f};
  float acc[4][CH];
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int c = 0; c < CH; ++c) acc[k][c] = 0.f;
  const float lthr = SKIP ? p.lskip : -INFINITY;
  const bool full16 = p.vec16 && (c0 + CH <= p.C);   // wave-uniform
  for (int base = 0; base < L.maxcont; base += 64) {
    __syncthreads();  // single-wave workgroup: orders the LDS reads of the previous chunk
    const int idx = base + lane;
    int mymask = 0, g = 0;
    if (idx < L.maxcont) {
      mymask = stage_entry<BOX, FLOOR, CLAMP, SKIP>(p, L, idx, gsid[(size_t)r0 + idx], tx0, ty0, rec, sA, sB, sC, lane, g);
      if (mymask != 0) {
        const float* row = feats + (size_t)g * p.C + c0;
        float4 f0, f1;
        if (full16) {
          f0 = reinterpret_cast<const float4*>(row)[0];
          f1 = reinterpret_cast<const float4*>(row)[1];
        } else {
          float f[CH];
#pragma unroll
          for (int c = 0; c < CH; ++c) f[c] = (c0 + c < p.C) ? row[c] : 0.f;
          f0 = make_float4(f[0], f[1], f[2], f[3]);
          f1 = make_float4(f[4], f[5], f[6], f[7]);
        }
        sF[0][lane] = f0;
        sF[1][lane] = f1;
      }
    }
    __syncthreads();
    unsigned long long todo = __ballot(mymask != 0);
    while (todo != 0ull) {
      const int j = __builtin_ctzll(todo);
      todo &= todo - 1ull;
      const int reach = __builtin_amdgcn_readlane(mymask, j);
      const float4 F0 = sF[0][j], F1 = sF[1][j];
      const float F[CH] = {F0.x, F0.y, F0.z, F0.w, F1.x, F1.y, F1.z, F1.w};
      blend_entry<BOX, FLOOR, CLAMP>(L, reach, base + j, j, sA, sB, sC, lthr, tau, [&](auto kc, float w) {
        constexpr int k = decltype(kc)::value;
#pragma unroll
        for (int c = 0; c < CH; ++c) acc[k][c] = fmaf(w, F[c], acc[k][c]);
      });
    }
  }
  const size_t plane = (size_t)p.W * p.H;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    if (c0 + c < p.C) {   // wave-uniform
      float* out = fmap + (size_t)(c0 + c) * plane;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int px = L.pxb[k & 1], py = L.pyb[k >> 1];
        if (px < p.W && py < p.H) out[(size_t)py * p.W + px] = acc[k][c];
      }
    }
  }
}

// ---- k_feature_gather -------------------------------------------------------------------------------------------------
// Workgroup (tile, chunk).  Each lane holds the pixel gradients G[4][8] of its four pixels, loaded ONCE before the loop
// (gfx9 counts loads, stores and atomics in one in-order vmcnt: a wait for a load inside the loop would also wait for
// the previous group's atomics).  Per hit it forms eight partials sum_k w G[k][c].  Entries are taken in groups of four
// slots, a slot taking entries until one of them HITS; each group is reduced by eight rows_of4, which leave entry
// {0, 2, 1, 3}[r] in every lane of row r, and lanes 0..7 of the row issue one float atomic add each into the Gaussian's
// feature row.  An entry that hits nothing costs no reduction and no atomic.
template <bool BOX, bool FLOOR, bool CLAMP, bool SKIP>
__global__ __launch_bounds__(64) void k_feature_gather(FeatParams p, const int32_t* __restrict__ ranges,
                                                       const int32_t* __restrict__ gsid,
                                                       const float4* __restrict__ rec,
                                                       const int32_t* __restrict__ contrib,
                                                       const float* __restrict__ gmap, float* __restrict__ gfeats) {
  __shared__ float4 sA[64], sB[64];
  __shared__ float sC[BOX ? 64 : 1];
  const int tile = blockIdx.x, lane = threadIdx.x;
  const int c0 = blockIdx.y * CH;
  if (tile >= p.T || c0 >= p.C) return;
  const int r0 = ranges[2 * (size_t)tile], r1 = ranges[2 * (size_t)tile + 1];
  const int n = r1 - r0;
  if (r0 < 0 || n <= 0) return;
  const int tx0 = (tile % p.gx) * EGS_TILE, ty0 = (tile / p.gx) * EGS_TILE;
  Lane L;
  lane_init(L, p, tx0, ty0, lane, n, contrib);
  if (L.maxcont <= 0) return;
  const size_t plane = (size_t)p.W * p.H;
  float G[4][CH];
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const bool chan = c0 + c < p.C;   // wave-uniform
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int px = L.pxb[k & 1], py = L.pyb[k >> 1];
      G[k][c] = (chan && px < p.W && py < p.H) ? gmap[(size_t)(c0 + c) * plane + (size_t)py * p.W + px] : 0.f;
    }
  }
  float tau[4] = {1.f, 1.f, 1.f, 1.f};
  const float lthr = SKIP ? p.lskip : -INFINITY;
  // where the reduction leaves the totals: row r of the wave holds entry slot {0, 2, 1, 3}[r]
  const int row = lane >> 4, c16 = lane & 15;
  const int myslot = ((row & 1) << 1) | (row >> 1);
  const bool adder = c16 < CH && c0 + c16 < p.C;
  for (int base = 0; base < L.maxcont; base += 64) {
    __syncthreads();  // single-wave workgroup: orders the LDS reads of the previous chunk
    const int idx = base + lane;
    int mymask = 0, g = 0;
    if (idx < L.maxcont)
      mymask = stage_entry<BOX, FLOOR, CLAMP, SKIP>(p, L, idx, gsid[(size_t)r0 + idx], tx0, ty0, rec, sA, sB, sC, lane, g);
    __syncthreads();
    unsigned long long todo = __ballot(mymask != 0);
    while (todo != 0ull) {
      float part[4][CH];
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int c = 0; c < CH; ++c) part[e][c] = 0.f;
      int ge[4] = {-1, -1, -1, -1};   // Gaussian held by slot e
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        while (todo != 0ull) {
          const int j = __builtin_ctzll(todo);
          todo &= todo - 1ull;
          const int reach = __builtin_amdgcn_readlane(mymask, j);
          const bool anyhit =
              blend_entry<BOX, FLOOR, CLAMP>(L, reach, base + j, j, sA, sB, sC, lthr, tau, [&](auto kc, float w) {
                constexpr int k = decltype(kc)::value;
#pragma unroll
                for (int c = 0; c < CH; ++c) part[e][c] = fmaf(w, G[k][c], part[e][c]);
              });
          if (__ballot(anyhit) != 0ull) {
            ge[e] = __builtin_amdgcn_readlane(g, j);
            break;
          }
        }
      }
      if (ge[0] < 0) break;   // the list ran out before anything hit
      float t[CH];
#pragma unroll
      for (int c = 0; c < CH; ++c) t[c] = rows_of4(part[0][c], part[1][c], part[2][c], part[3][c]);
      const int gs = myslot == 0 ? ge[0] : (myslot == 1 ? ge[1] : (myslot == 2 ? ge[2] : ge[3]));
      float mine = t[0];
#pragma unroll
      for (int c = 1; c < CH; ++c) mine = (c16 == c) ? t[c] : mine;
      if (gs >= 0 && adder) atomicAdd(gfeats + (size_t)gs * p.C + c0 + c16, mine);
    }
  }
}

static int check_common(int n, int width, int height, const float* rec, const EgsPolicy* pol, const int32_t* ranges,
                        const int32_t* gsid, const int32_t* contrib, int flags, int channels, bool lists) {
  FEAT_CHECK_ARG(n >= 0);
  FEAT_CHECK_ARG(width > 0 && height > 0);
  FEAT_CHECK_ARG((flags & ~EGS_DRAW_MASKED_LISTS) == 0);
  FEAT_CHECK_ARG(pol != nullptr);
  FEAT_CHECK_ARG(channels >= 1 && channels <= EGS_FEAT_MAX_CHANNELS);
  if (!lists) return 0;
  FEAT_CHECK_ARG(rec != nullptr && ((uintptr_t)rec & 15) == 0);
  FEAT_CHECK_ARG(ranges != nullptr && ((uintptr_t)ranges & 3) == 0);
  FEAT_CHECK_ARG(gsid != nullptr && ((uintptr_t)gsid & 3) == 0);
  FEAT_CHECK_ARG(contrib != nullptr && ((uintptr_t)contrib & 3) == 0);
  FEAT_CHECK_ARG(!(flags & EGS_DRAW_MASKED_LISTS) || n < (1 << EGS_GSID_BITS));
  return 0;
}

static FeatParams make_params(int n, int width, int height, const EgsPolicy* pol, int flags, int channels) {
  FeatParams p;
  p.N = n; p.W = width; p.H = height; p.C = channels;
  p.gx = div_up(width, EGS_TILE);
  p.T = p.gx * div_up(height, EGS_TILE);
  p.lskip = pol->alpha_skip > 0.f ? log2f(pol->alpha_skip) : -INFINITY;
  p.nan_blend = pol->nan_maha == 0 && pol->maha_floor;
  p.masked = (flags & EGS_DRAW_MASKED_LISTS) != 0;
  p.vec16 = 0;
  return p;
}

}  // namespace egs_feat

using namespace egs_feat;

extern "C" int egs_feat_abi_version(void) { return EGS_FEAT_ABI_VERSION; }
extern "C" const char* egs_feat_last_error_string(void) { return egs_feat::g_err; }

extern "C" int egs_feature_render(int n, int width, int height, const float* rec, const EgsPolicy* pol,
                                  const int32_t* ranges, const int32_t* gsid, const int32_t* contrib, int flags,
                                  int channels, const float* feats, float* fmap, void* stream) {
  if (int rc = check_common(n, width, height, rec, pol, ranges, gsid, contrib, flags, channels, false)) return rc;
  FEAT_CHECK_ARG(fmap != nullptr && ((uintptr_t)fmap & 3) == 0);
  if (n == 0) {
    FEAT_HIP(hipMemsetAsync(fmap, 0, (size_t)channels * width * height * sizeof(float), (hipStream_t)stream));
    return 0;
  }
  if (int rc = check_common(n, width, height, rec, pol, ranges, gsid, contrib, flags, channels, true)) return rc;
  FEAT_CHECK_ARG(feats != nullptr && ((uintptr_t)feats & 3) == 0);
  FeatParams p = make_params(n, width, height, pol, flags, channels);
  p.vec16 = ((uintptr_t)feats & 15) == 0 && (channels & 3) == 0;
  decltype(&k_feature_render<false, false, false, false>) kern = nullptr;
  with_bools(
      [&](auto box, auto flr, auto clamp, auto skip) {
        kern = k_feature_render<box.value, flr.value, clamp.value, skip.value>;
      },
      pol->footprint == 1, pol->maha_floor != 0, pol->alpha_clamp != 0, pol->alpha_skip > 0.f);
  hipLaunchKernelGGL(kern, dim3(p.T, div_up(channels, CH)), dim3(64), 0, (hipStream_t)stream, p, ranges, gsid,
                     (const float4*)rec, contrib, feats, fmap);
  FEAT_HIP(hipGetLastError());
  return 0;
}

extern "C" int egs_feature_gather(int n, int width, int height, const float* rec, const EgsPolicy* pol,
                                  const int32_t* ranges, const int32_t* gsid, const int32_t* contrib, int flags,
                                  int channels, const float* gmap, float* gfeats, void* stream) {
  if (int rc = check_common(n, width, height, rec, pol, ranges, gsid, contrib, flags, channels, n > 0)) return rc;
  if (n == 0) return 0;
  FEAT_CHECK_ARG(gmap != nullptr && ((uintptr_t)gmap & 3) == 0);
  FEAT_CHECK_ARG(gfeats != nullptr && ((uintptr_t)gfeats & 3) == 0);
  FeatParams p = make_params(n, width, height, pol, flags, channels);
  decltype(&k_feature_gather<false, false, false, false>) kern = nullptr;
  with_bools(
      [&](auto box, auto flr, auto clamp, auto skip) {
        kern = k_feature_gather<box.value, flr.value, clamp.value, skip.value>;
      },
      pol->footprint == 1, pol->maha_floor != 0, pol->alpha_clamp != 0, pol->alpha_skip > 0.f);
  hipLaunchKernelGGL(kern, dim3(p.T, div_up(channels, CH)), dim3(64), 0, (hipStream_t)stream, p, ranges, gsid,
                     (const float4*)rec, contrib, gmap, gfeats);
  FEAT_HIP(hipGetLastError());
  return 0;
}
