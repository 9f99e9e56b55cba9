// Per-Gaussian feature vectors through the tile lists of a finished forward pass, for gfx950 (include/egs_feat.h has the
// contract): k_feature_render blends C channels with the forward's weights w = tau alpha', k_feature_gather is its
// adjoint.  Both walk a tile exactly as k_blend_weights (egs_prune.hip) does -- k_draw's walk, bounded by the forward's
// `contrib` as k_draw_bwd's is -- so no stop decision is derived again and the weights are the forward's.
//
// Built into libegs_feat.so, a library of its own: it shares headers with libegs_hip.so and libegs_prune.so (the walk
// of egs_list_walk.h, the reduction of egs_draw_device.h) but no symbol, and keeps its own last-error string.
#define EGS_SIDE_LIBRARY "egs_feat"
#include "egs_list_walk.h"
#include "../../include/egs_feat.h"

namespace egs_feat {

using namespace egs;

constexpr int CH = 8;   // channels per wave: one (tile, chunk of CH channels) per workgroup

struct FeatParams {
  int N, W, H, gx, T, C;
  float lskip;     // log2(alpha_skip), -inf when there is no skip test
  int nan_blend;   // as DrawParams.nan_blend
  int masked;      // the list values carry the tile's 4-bit block mask in their high bits
  int vec16;       // every feature row chunk is 16-byte aligned (render only)
};

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
// slots, a slot taking entries until one of them HITS; each group is reduced by eight total_of4, which leave entry
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
      for (int c = 0; c < CH; ++c) t[c] = total_of4(part[0][c], part[1][c], part[2][c], part[3][c]);
      const int gs = myslot == 0 ? ge[0] : (myslot == 1 ? ge[1] : (myslot == 2 ? ge[2] : ge[3]));
      float mine = t[0];
#pragma unroll
      for (int c = 1; c < CH; ++c) mine = (c16 == c) ? t[c] : mine;
      if (gs >= 0 && adder) atomicAdd(gfeats + (size_t)gs * p.C + c0 + c16, mine);
    }
  }
}

}  // namespace egs_feat

using namespace egs_feat;

extern "C" int egs_feat_abi_version(void) { return EGS_FEAT_ABI_VERSION; }
extern "C" const char* egs_feat_last_error_string(void) { return egs_side::g_err; }

extern "C" int egs_feature_render(int n, int width, int height, const float* rec, const EgsPolicy* pol,
                                  const int32_t* ranges, const int32_t* gsid, const int32_t* contrib, int flags,
                                  int channels, const float* feats, float* fmap, void* stream) {
  if (int rc = check_view(n, width, height, pol, flags)) return rc;
  SIDE_CHECK_ARG(channels >= 1 && channels <= EGS_FEAT_MAX_CHANNELS);
  SIDE_CHECK_ARG(fmap != nullptr && ((uintptr_t)fmap & 3) == 0);
  if (n == 0) {
    SIDE_HIP(hipMemsetAsync(fmap, 0, (size_t)channels * width * height * sizeof(float), (hipStream_t)stream));
    return 0;
  }
  if (int rc = check_lists(n, rec, ranges, gsid, contrib, flags)) return rc;
  SIDE_CHECK_ARG(feats != nullptr && ((uintptr_t)feats & 3) == 0);
  FeatParams p;
  fill_params(p, n, width, height, pol, flags);
  p.C = channels;
  p.vec16 = ((uintptr_t)feats & 15) == 0 && (channels & 3) == 0;
  decltype(&k_feature_render<false, false, false, false>) kern = nullptr;
  with_policy(pol, [&](auto box, auto flr, auto clamp, auto skip) {
    kern = k_feature_render<box.value, flr.value, clamp.value, skip.value>;
  });
  hipLaunchKernelGGL(kern, dim3(p.T, div_up(channels, CH)), dim3(64), 0, (hipStream_t)stream, p, ranges, gsid,
                     (const float4*)rec, contrib, feats, fmap);
  SIDE_HIP(hipGetLastError());
  return 0;
}

extern "C" int egs_feature_gather(int n, int width, int height, const float* rec, const EgsPolicy* pol,
                                  const int32_t* ranges, const int32_t* gsid, const int32_t* contrib, int flags,
                                  int channels, const float* gmap, float* gfeats, void* stream) {
  if (int rc = check_view(n, width, height, pol, flags)) return rc;
  SIDE_CHECK_ARG(channels >= 1 && channels <= EGS_FEAT_MAX_CHANNELS);
  if (n == 0) return 0;
  if (int rc = check_lists(n, rec, ranges, gsid, contrib, flags)) return rc;
  SIDE_CHECK_ARG(gmap != nullptr && ((uintptr_t)gmap & 3) == 0);
  SIDE_CHECK_ARG(gfeats != nullptr && ((uintptr_t)gfeats & 3) == 0);
  FeatParams p;
  fill_params(p, n, width, height, pol, flags);
  p.C = channels;
  p.vec16 = 0;
  decltype(&k_feature_gather<false, false, false, false>) kern = nullptr;
  with_policy(pol, [&](auto box, auto flr, auto clamp, auto skip) {
    kern = k_feature_gather<box.value, flr.value, clamp.value, skip.value>;
  });
  hipLaunchKernelGGL(kern, dim3(p.T, div_up(channels, CH)), dim3(64), 0, (hipStream_t)stream, p, ranges, gsid,
                     (const float4*)rec, contrib, gmap, gfeats);
  SIDE_HIP(hipGetLastError());
  return 0;
}
