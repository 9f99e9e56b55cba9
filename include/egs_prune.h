/* C ABI of libegs_prune.so: per-Gaussian blend-weight statistics for importance-based pruning on AMD Instinct MI355X
 * (gfx950).
 *
 * The forward draw pass forms the blending weight w = tau alpha' of every (pixel, list entry) pair and keeps only the
 * image.  Compaction methods prune on that weight, gathered over all training views: RadSplat on its maximum,
 * Mini-Splatting on its sum, LightGaussian on hit counts.  egs_blend_weights walks the tile lists of ONE finished
 * forward pass again, without colours, and accumulates the three statistics per Gaussian.
 *
 * A library of its own beside libegs_hip.so (include/egs_hip.h) and libegs_mcmc.so, whose surfaces and ABI numbers it
 * leaves alone.  Same conventions: raw device pointers and a HIP stream (hipStream_t as void*), no device
 * synchronisation, every argument validated BEFORE any HIP call; return 0 on success, otherwise EGS_ERR_BAD_ARG or a
 * hipError_t, and the last-error string of THIS library describes it.
 *
 * The statistic.  Take a tile with list entries k = 0 .. L-1 (Gaussian g_k) and a pixel p of it; c_p = contrib[p] is what
 * the forward pass wrote (the 1-based index of the pixel's last contributor, 0: none).
 *   live   entry k is live at p iff k < c_p (pixel-box footprint: p must also lie inside the Gaussian's pixel box)
 *   hit    live and not alpha'_k(p) < alpha_skip (policies with a skip threshold); an entry whose conic or centre holds
 *          a NaN follows the forward pass's rule (EgsPolicy.nan_maha)
 *   w      w_k(p) = tau_k(p) alpha'_k(p), tau_0 = 1 and, on a hit, tau_{k+1} = tau_k - w_k; alpha' includes the policy's
 *          0.99 clamp and maha >= 0 floor
 * per Gaussian g:  sum[g] += sum_p w,  max[g] = max(max[g], max_p w),  hits[g] += number of hits.
 * The walk is bounded by the forward's contrib: the stop decision (tau < tau_stop) is the forward's and is never derived
 * again, and a tile is walked to its largest c_p and no further.  Over the non-empty tiles of a render,
 * sum_g sum[g] = sum_p (1 - final_tau[p]).
 *
 * Reproducibility: max (an integer atomic max on the bits of a float >= 0) and hits (an integer add) are bitwise
 * reproducible.  sum is a float atomic add per (tile, Gaussian): reproducible only when every Gaussian lies on one tile
 * of one view, otherwise it depends on the order in which the atomics arrive.
 */
#ifndef EGS_PRUNE_H_
#define EGS_PRUNE_H_

#include <stddef.h>
#include <stdint.h>

#include "egs_hip.h" /* EgsPolicy, EGS_DRAW_MASKED_LISTS, EGS_ERR_BAD_ARG */

#ifdef __cplusplus
extern "C" {
#endif

#define EGS_PRUNE_ABI_VERSION 1

int egs_prune_abi_version(void);
const char* egs_prune_last_error_string(void);

/* ACCUMULATES into stats: the caller zeroes it once and may call this for any number of views.
 *   rec      [n][12] packed draw records: egs_pack_records' or the fused forward's (16-B aligned)
 *   ranges   [T][2] tile ranges into gsid, T = ceil(width / 16) ceil(height / 16)
 *   gsid     list values; with EGS_DRAW_MASKED_LISTS they carry the tile's 4-bit block mask in their high bits
 *   contrib  [height][width] of the forward pass
 *   flags    0 or EGS_DRAW_MASKED_LISTS
 *   stats    [n][4]: sum f32 | max f32 | hits i32 | reserved, stays 0   (16-B aligned)
 * A list value outside [0, n) is skipped.  n == 0 returns 0 without a launch. */
int egs_blend_weights(int n, int width, int height, const float* rec, const EgsPolicy* pol, const int32_t* ranges,
                      const int32_t* gsid, const int32_t* contrib, int flags, float* stats, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EGS_PRUNE_H_ */
