// Per-Gaussian blend-weight statistics for gfx950 (include/egs_prune.h has the contract): k_blend_weights walks the tile
// lists of a finished forward pass again -- k_draw's walk without colours, bounded by the forward's `contrib` as
// k_draw_bwd's is -- and accumulates sum / max / count of w = tau alpha' per Gaussian.
//
// Built into libegs_prune.so, a library of its own: it shares headers with libegs_hip.so (the reach mask, the NaN rule
// and the one-instruction min of the draw kernels) but no symbol, and keeps its own last-error string.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "egs_draw_device.h"
#include "../../include/egs_prune.h"

namespace egs_prune {

static thread_local char g_err[512] = "no error";

static void set_error(int code, const char* what, const char* file, int line) {
  const char* base = strrchr(file, '/');
  snprintf(g_err, sizeof(g_err), "egs_prune error %d: %s (%s:%d)", code, what ? what : "?", base ? base + 1 : file,
           line);
}

#define PRUNE_CHECK_ARG(cond)                                                             \
  do {                                                                                    \
    if (!(cond)) {                                                                        \
      ::egs_prune::set_error(EGS_ERR_BAD_ARG, "bad argument: " #cond, __FILE__, __LINE__); \
      return EGS_ERR_BAD_ARG;                                                             \
    }                                                                                     \
  } while (0)

#define PRUNE_HIP(expr)                                                              \
  do {                                                                               \
    hipError_t e__ = (expr);                                                         \
    if (e__ != hipSuccess) {                                                         \
      ::egs_prune::set_error((int)e__, hipGetErrorString(e__), __FILE__, __LINE__);  \
      return (int)e__;                                                               \
    }                                                                                \
  } while (0)

using egs::div_up;
using egs::min_hi;
using egs::nan_entry_fix;
using egs::reach_mask;
using egs::with_bools;

struct BlendParams {
  int N, W, H, gx, T;
  float lskip;     // log2(alpha_skip), -inf when there is no skip test
  int nan_blend;   // as DrawParams.nan_blend
  int masked;      // the list values carry the tile's 4-bit block mask in their high bits
};

// ---- transposing wave reduction of four entries (the scheme of k_draw_bwd's rows_of4) -----------------------------
// Four per-lane partials become four row-wise partial sets: after the two swaps row r of the wave holds 16 partials of
// entry {0, 2, 1, 3}[r]; four DPP steps inside the row leave the total in every lane of it.
struct OpAdd { __device__ __forceinline__ float operator()(float a, float b) const { return a + b; } };
struct OpMax { __device__ __forceinline__ float operator()(float a, float b) const { return fmaxf(a, b); } };

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
template <typename Op>
__device__ __forceinline__ float rows_of4(float e0, float e1, float e2, float e3, Op op) {
  swap32(e0, e1);
  float a = op(e0, e1);   // lanes 0-31: e0 halves, lanes 32-63: e1 halves
  swap32(e2, e3);
  float b = op(e2, e3);
  swap16(a, b);           // rows of a: [e0, e2, e1, e3]; rows of b: the other halves
  float v = op(a, b);
  v = op(v, dpp_get<0x140>(v));   // row_mirror
  v = op(v, dpp_get<0x141>(v));   // row_half_mirror
  v = op(v, dpp_get<0x4E>(v));    // quad_perm [2, 3, 0, 1]
  v = op(v, dpp_get<0xB1>(v));    // quad_perm [1, 0, 3, 2]
  return v;
}

// One wave64 per 16x16 tile, four pixels per lane: pixel k = 2 by + bx of lane l is (tx0 + (l & 7) + 8 bx,
// ty0 + (l >> 3) + 8 by), k_draw's mapping.  64-entry chunks are staged in LDS by the lane that owns the entry: the
// conic, the cap, the polynomial about the tile centre and (BOX) the pixel box -- no colours.  The exponent is k_draw's
// (same polynomial, same fmaf order, log2 alpha from the record's threshold, one min against the cap), so the tau formed
// here is the forward's tau and the skip decisions agree with it.  Entry i is live at a pixel iff i < contrib there: tau
// only falls, so every entry in front of a pixel's last contributor met `tau >= tau_stop` in the forward pass, and none
// behind it hit.
template <bool BOX, bool FLOOR, bool CLAMP, bool SKIP>
__global__ __launch_bounds__(64) void k_blend_weights(BlendParams p, const int32_t* __restrict__ ranges,
                                                      const int32_t* __restrict__ gsid,
                                                      const float4* __restrict__ rec,
                                                      const int32_t* __restrict__ contrib, float* __restrict__ stats) {
  __shared__ float4 sA[64], sB[64];       // (qxx, qxy, qyy, cap), (c0, c1, c2, x pixel box)
  __shared__ float sC[BOX ? 64 : 1];      // y pixel box
  const int tile = blockIdx.x, lane = threadIdx.x;
  if (tile >= p.T) return;
  const int r0 = ranges[2 * (size_t)tile], r1 = ranges[2 * (size_t)tile + 1];
  const int n = r1 - r0;
  if (r0 < 0 || n <= 0) return;
  const int tx0 = (tile % p.gx) * EGS_TILE, ty0 = (tile / p.gx) * EGS_TILE;
  const int pxb[2] = {tx0 + (lane & 7), tx0 + (lane & 7) + 8};
  const int pyb[2] = {ty0 + (lane >> 3), ty0 + (lane >> 3) + 8};
  int cont[4], bmax[4];   // bmax: wave-uniform, largest contrib of block k -> entries >= bmax[k] are inert for it
  int maxcont = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int px = pxb[k & 1], py = pyb[k >> 1];
    cont[k] = (px < p.W && py < p.H) ? contrib[(size_t)py * p.W + px] : 0;
    int mx = cont[k];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mx = max(mx, __shfl_xor(mx, d, 64));
    bmax[k] = __builtin_amdgcn_readfirstlane(min(mx, n));
    maxcont = max(maxcont, bmax[k]);
  }
  if (maxcont <= 0) return;
  const float X[2] = {(float)(lane & 7) - 7.5f, (float)(lane & 7) + 0.5f};
  const float Y[2] = {(float)(lane >> 3) - 7.5f, (float)(lane >> 3) + 0.5f};
  const float XX[2] = {X[0] * X[0], X[1] * X[1]}, YY[2] = {Y[0] * Y[0], Y[1] * Y[1]};
  const float XY[4] = {X[0] * Y[0], X[1] * Y[0], X[0] * Y[1], X[1] * Y[1]};
  float tau[4] = {1.f, 1.f, 1.f, 1.f};
  constexpr float L99 = -0.014499569695115089f;  // log2(0.99)
  const float cx0 = (float)tx0 + 7.5f, cy0 = (float)ty0 + 7.5f;
  const float lskip = p.lskip;
  const float lthr = SKIP ? lskip : -INFINITY;
  // where the reduction leaves the totals: row r of the wave holds entry slot {0, 2, 1, 3}[r]; its lanes 0, 1, 2 issue
  // the three atomics into the Gaussian's 16-byte row
  const int row = lane >> 4, c16 = lane & 15;
  const int myslot = ((row & 1) << 1) | (row >> 1);
  for (int base = 0; base < maxcont; base += 64) {
    __syncthreads();  // single-wave workgroup: orders the LDS reads of the previous chunk
    const int idx = base + lane;
    int mymask = 0, g = 0;
    if (idx < maxcont) {
      const int gm = gsid[(size_t)r0 + idx];
      g = p.masked ? (int)((uint32_t)gm & EGS_GSID_MASK) : gm;
      if ((unsigned)g < (unsigned)p.N) {
        float4 A = rec[3 * (size_t)g], B = rec[3 * (size_t)g + 1];
        const float4 C = rec[3 * (size_t)g + 2];
        const bool nanfix = p.nan_blend && nan_entry_fix(A, B);
        if (C.w < INFINITY) mymask = p.masked ? (int)((uint32_t)gm >> EGS_GSID_BITS) : reach_mask<BOX>(A, C, tx0, ty0);
        if (nanfix && !BOX && !p.masked && C.w < INFINITY) mymask = 0xF;
        const float la = SKIP ? lskip - C.w : __builtin_amdgcn_logf(B.y);
        float cap = 3.0e38f;
        if (FLOOR) cap = CLAMP ? fminf(la, L99) : la;
        else if (CLAMP) cap = L99;
        const float Dx = cx0 - A.x, Dy = cy0 - A.y;
        const float c0 = la + (A.z * Dx * Dx + A.w * Dx * Dy + B.x * Dy * Dy);
        const float c1 = 2.f * A.z * Dx + A.w * Dy, c2 = 2.f * B.x * Dy + A.w * Dx;
        sA[lane] = make_float4(A.z, A.w, B.x, cap);
        sB[lane] = make_float4(c0, c1, c2, C.y);
        if constexpr (BOX) sC[lane] = C.z;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (idx >= bmax[k]) mymask &= ~(1 << k);   // no pixel of block k got this far
    }
    __syncthreads();
    // every lane answered for the entry it staged; a scalar bit scan walks the entries that reach a block with a live
    // pixel in list order.  Groups of four: each of the four slots takes entries until one of them HITS, then the four
    // are reduced together.
    unsigned long long todo = __ballot(mymask != 0);
    while (todo != 0ull) {
      float ws[4] = {0.f, 0.f, 0.f, 0.f}, wm[4] = {0.f, 0.f, 0.f, 0.f}, wc[4] = {0.f, 0.f, 0.f, 0.f};
      int ge[4] = {-1, -1, -1, -1};   // Gaussian held by slot e
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        while (todo != 0ull) {
          const int j = __builtin_ctzll(todo);
          todo &= todo - 1ull;
          const int reach = __builtin_amdgcn_readlane(mymask, j);
          const int i = base + j;   // index of this entry in the tile list
          const float4 Q = sA[j], P = sB[j];            // wave-uniform address: LDS broadcast
          bool inx[2] = {true, true}, iny[2] = {true, true};
          if (BOX) {
            const uint32_t bx = __float_as_uint(P.w), by = __float_as_uint(sC[j]);
            const int x0 = bx & 0xFFFF, x1 = bx >> 16, y0 = by & 0xFFFF, y1 = by >> 16;
#pragma unroll
            for (int b = 0; b < 2; ++b) {
              inx[b] = (pxb[b] >= x0) && (pxb[b] < x1);
              iny[b] = (pyb[b] >= y0) && (pyb[b] < y1);
            }
          }
          bool anyhit = false;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const int bx = k & 1, by = k >> 1;
            if (reach & (1 << k)) {  // scalar branch: block k is in reach and some pixel of it got this far
              float ex = fmaf(P.z, Y[by], P.x);
              ex = fmaf(P.y, X[bx], ex);
              ex = fmaf(Q.z, YY[by], ex);
              ex = fmaf(Q.y, XY[k], ex);
              ex = fmaf(Q.x, XX[bx], ex);
              bool hit = (i < cont[k]) && (ex >= lthr);
              if (BOX) hit = hit && inx[bx] && iny[by];
              if (hit) {
                if (FLOOR || CLAMP) ex = min_hi(ex, Q.w);
                const float w = tau[k] * __builtin_amdgcn_exp2f(ex);
                tau[k] -= w;
                ws[e] += w;
                wm[e] = fmaxf(wm[e], w);
                wc[e] += 1.f;
                anyhit = true;
              }
            }
          }
          if (__ballot(anyhit) != 0ull) {
            ge[e] = __builtin_amdgcn_readlane(g, j);
            break;
          }
        }
      }
      if (ge[0] < 0) break;   // the list ran out before anything hit
      const float tsum = rows_of4(ws[0], ws[1], ws[2], ws[3], OpAdd{});
      const float tmax = rows_of4(wm[0], wm[1], wm[2], wm[3], OpMax{});
      const float tcnt = rows_of4(wc[0], wc[1], wc[2], wc[3], OpAdd{});
      const int gs = myslot == 0 ? ge[0] : (myslot == 1 ? ge[1] : (myslot == 2 ? ge[2] : ge[3]));
      if (gs >= 0 && c16 < 3) {
        float* rowp = stats + 4 * (size_t)gs;
        if (c16 == 0) atomicAdd(rowp, tsum);
        else if (c16 == 1) atomicMax(reinterpret_cast<int*>(rowp + 1), __float_as_int(tmax));   // w >= 0: bit order
        else atomicAdd(reinterpret_cast<int*>(rowp + 2), (int)tcnt);
      }
    }
  }
}

}  // namespace egs_prune

using namespace egs_prune;

extern "C" int egs_prune_abi_version(void) { return EGS_PRUNE_ABI_VERSION; }
extern "C" const char* egs_prune_last_error_string(void) { return egs_prune::g_err; }

extern "C" int egs_blend_weights(int n, int width, int height, const float* rec, const EgsPolicy* pol,
                                 const int32_t* ranges, const int32_t* gsid, const int32_t* contrib, int flags,
                                 float* stats, void* stream) {
  PRUNE_CHECK_ARG(n >= 0);
  PRUNE_CHECK_ARG(width > 0 && height > 0);
  PRUNE_CHECK_ARG((flags & ~EGS_DRAW_MASKED_LISTS) == 0);
  PRUNE_CHECK_ARG(pol != nullptr);
  if (n == 0) return 0;
  PRUNE_CHECK_ARG(rec != nullptr && ((uintptr_t)rec & 15) == 0);
  PRUNE_CHECK_ARG(ranges != nullptr);
  PRUNE_CHECK_ARG(gsid != nullptr);
  PRUNE_CHECK_ARG(contrib != nullptr);
  PRUNE_CHECK_ARG(stats != nullptr && ((uintptr_t)stats & 15) == 0);
  PRUNE_CHECK_ARG(!(flags & EGS_DRAW_MASKED_LISTS) || n < (1 << EGS_GSID_BITS));
  BlendParams p;
  p.N = n; p.W = width; p.H = height;
  p.gx = div_up(width, EGS_TILE);
  p.T = p.gx * div_up(height, EGS_TILE);
  p.lskip = pol->alpha_skip > 0.f ? log2f(pol->alpha_skip) : -INFINITY;
  p.nan_blend = pol->nan_maha == 0 && pol->maha_floor;
  p.masked = (flags & EGS_DRAW_MASKED_LISTS) != 0;
  decltype(&k_blend_weights<false, false, false, false>) kern = nullptr;
  with_bools(
      [&](auto box, auto flr, auto clamp, auto skip) {
        kern = k_blend_weights<box.value, flr.value, clamp.value, skip.value>;
      },
      pol->footprint == 1, pol->maha_floor != 0, pol->alpha_clamp != 0, pol->alpha_skip > 0.f);
  hipLaunchKernelGGL(kern, dim3(p.T), dim3(64), 0, (hipStream_t)stream, p, ranges, gsid, (const float4*)rec, contrib,
                     stats);
  PRUNE_HIP(hipGetLastError());
  return 0;
}
