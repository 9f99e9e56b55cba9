// Per-Gaussian blend-weight statistics for gfx950 (include/egs_prune.h has the contract): k_blend_weights walks the tile
// lists of a finished forward pass again -- k_draw's walk without colours, bounded by the forward's `contrib` as
// k_draw_bwd's is -- and accumulates sum / max / count of w = tau alpha' per Gaussian.
//
// Built into libegs_prune.so, a library of its own: it shares headers with libegs_hip.so and libegs_feat.so (the walk
// of egs_list_walk.h, the reduction of egs_draw_device.h) but no symbol, and keeps its own last-error string.
#define EGS_SIDE_LIBRARY "egs_prune"
#include "egs_list_walk.h"
#include "../../include/egs_prune.h"

namespace egs_prune {

using namespace egs;

struct BlendParams {
  int N, W, H, gx, T;
  float lskip;     // log2(alpha_skip), -inf when there is no skip test
  int nan_blend;   // as DrawParams.nan_blend
  int masked;      // the list values carry the tile's 4-bit block mask in their high bits
};

// The walk of egs_list_walk.h; per hit the entry's slot takes sum / max / count of w.
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
  Lane L;
  lane_init(L, p, tx0, ty0, lane, n, contrib);
  if (L.maxcont <= 0) return;
  float tau[4] = {1.f, 1.f, 1.f, 1.f};
  const float lthr = SKIP ? p.lskip : -INFINITY;
  // where the reduction leaves the totals: row r of the wave holds entry slot {0, 2, 1, 3}[r]; its lanes 0, 1, 2 issue
  // the three atomics into the Gaussian's 16-byte row
  const int row = lane >> 4, c16 = lane & 15;
  const int myslot = ((row & 1) << 1) | (row >> 1);
  for (int base = 0; base < L.maxcont; base += 64) {
    __syncthreads();  // single-wave workgroup: orders the LDS reads of the previous chunk
    const int idx = base + lane;
    int mymask = 0, g = 0;
    if (idx < L.maxcont)
      mymask = stage_entry<BOX, FLOOR, CLAMP, SKIP>(p, L, idx, gsid[(size_t)r0 + idx], tx0, ty0, rec, sA, sB, sC, lane, g);
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
          const bool anyhit =
              blend_entry<BOX, FLOOR, CLAMP>(L, reach, base + j, j, sA, sB, sC, lthr, tau, [&](auto, float w) {
                ws[e] += w;
                wm[e] = fmaxf(wm[e], w);
                wc[e] += 1.f;
              });
          if (__ballot(anyhit) != 0ull) {
            ge[e] = __builtin_amdgcn_readlane(g, j);
            break;
          }
        }
      }
      if (ge[0] < 0) break;   // the list ran out before anything hit
      const float tsum = total_of4(ws[0], ws[1], ws[2], ws[3]);
      const float tmax = total_of4(wm[0], wm[1], wm[2], wm[3], OpMax{});
      const float tcnt = total_of4(wc[0], wc[1], wc[2], wc[3]);
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
extern "C" const char* egs_prune_last_error_string(void) { return egs_side::g_err; }

extern "C" int egs_blend_weights(int n, int width, int height, const float* rec, const EgsPolicy* pol,
                                 const int32_t* ranges, const int32_t* gsid, const int32_t* contrib, int flags,
                                 float* stats, void* stream) {
  if (int rc = check_view(n, width, height, pol, flags)) return rc;
  if (n == 0) return 0;
  if (int rc = check_lists(n, rec, ranges, gsid, contrib, flags)) return rc;
  SIDE_CHECK_ARG(stats != nullptr && ((uintptr_t)stats & 15) == 0);
  BlendParams p;
  fill_params(p, n, width, height, pol, flags);
  decltype(&k_blend_weights<false, false, false, false>) kern = nullptr;
  with_policy(pol, [&](auto box, auto flr, auto clamp, auto skip) {
    kern = k_blend_weights<box.value, flr.value, clamp.value, skip.value>;
  });
  hipLaunchKernelGGL(kern, dim3(p.T), dim3(64), 0, (hipStream_t)stream, p, ranges, gsid, (const float4*)rec, contrib,
                     stats);
  SIDE_HIP(hipGetLastError());
  return 0;
}
