/* C ABI of libegs_feat.so: per-Gaussian feature vectors rendered through the tile lists of a finished forward pass, and
 * the adjoint of that render, on AMD Instinct MI355X (gfx950).
 *
 * The draw pass blends three colour channels.  Semantic / language feature fields (LangSplat, Feature-3DGS, Gaussian
 * Grouping), label lifting from 2D masks and attribute maps need an arbitrary per-Gaussian vector f_g in R^C carried
 * through the same weights w = tau alpha'.  egs_feature_render walks the tile lists of ONE finished forward pass again
 * and blends C channels; egs_feature_gather is its adjoint: the pixel gradients of a feature map reduced per Gaussian
 * with the same weights.  Both are linear in the features.  GEOMETRY IS FROZEN: nothing here differentiates with
 * respect to positions, covariances or opacities.
 *
 * A library of its own beside libegs_hip.so (include/egs_hip.h), libegs_mcmc.so and libegs_prune.so, whose surfaces and
 * ABI numbers it leaves alone.  Same conventions: raw device pointers and a HIP stream (hipStream_t as void*), no device
 * synchronisation, every argument validated BEFORE any HIP call; return 0 on success, otherwise EGS_ERR_BAD_ARG or a
 * hipError_t, and the last-error string of THIS library describes it.
 *
 * The weights are those of include/egs_prune.h, word for word.  Take a tile with list entries k = 0 .. L-1 (Gaussian
 * g_k) and a pixel p of it; c_p = contrib[p] is what the forward pass wrote.
 *   live   entry k is live at p iff k < c_p (pixel-box footprint: p must also lie inside the Gaussian's pixel box)
 *   hit    live and not alpha'_k(p) < alpha_skip; an entry whose conic or centre holds a NaN follows the forward's rule
 *   w      w_k(p) = tau_k(p) alpha'_k(p), tau_0 = 1 and, on a hit, tau_{k+1} = tau_k - w_k
 * The walk is bounded by the forward's contrib: no stop decision is derived again.  A list value outside [0, n) is
 * skipped.  No background and no normalisation: a caller who wants the expected feature divides by 1 - final_tau.
 *
 * Reproducibility: egs_feature_render is bitwise reproducible.  egs_feature_gather issues one float atomic add per
 * (tile, Gaussian, channel): reproducible only when every Gaussian lies on one tile of one view.
 */
#ifndef EGS_FEAT_H_
#define EGS_FEAT_H_

#include <stddef.h>
#include <stdint.h>

#include "egs_hip.h" /* EgsPolicy, EGS_DRAW_MASKED_LISTS, EGS_ERR_BAD_ARG */

#ifdef __cplusplus
extern "C" {
#endif

#define EGS_FEAT_ABI_VERSION 1
#define EGS_FEAT_MAX_CHANNELS 4096

int egs_feat_abi_version(void);
const char* egs_feat_last_error_string(void);

/* Arguments of both calls:
 *   rec       [n][12] packed draw records: egs_pack_records' or the fused forward's (16-B aligned)
 *   ranges    [T][2] tile ranges into gsid, T = ceil(width / 16) ceil(height / 16)
 *   gsid      list values; with EGS_DRAW_MASKED_LISTS they carry the tile's 4-bit block mask in their high bits
 *             (then n < 2^28)
 *   contrib   [height][width] of the forward pass
 *   flags     0 or EGS_DRAW_MASKED_LISTS
 *   channels  C in [1, EGS_FEAT_MAX_CHANNELS]
 * Every pointer but rec needs 4-byte alignment only. */

/* fmap[c][y][x] = sum over the tile list of w_k(x, y) feats[g_k][c].  Writes EVERY pixel of all C planes (zeros on
 * empty tiles), so fmap needs no initialisation.
 *   feats  [n][channels]      fmap  [channels][height][width]
 * n == 0 zero-fills fmap (hipMemsetAsync) and returns 0; sizes, flags, pol, channels and fmap are still checked. */
int egs_feature_render(int n, int width, int height, const float* rec, const EgsPolicy* pol, const int32_t* ranges,
                       const int32_t* gsid, const int32_t* contrib, int flags, int channels, const float* feats,
                       float* fmap, void* stream);

/* gfeats[g][c] += sum over pixels and list entries of g of w gmap[c][y][x].  ACCUMULATES: the caller zeroes gfeats once
 * and may call this for any number of views.
 *   gmap  [channels][height][width]      gfeats  [n][channels]
 * n == 0 returns 0 and touches nothing; sizes, flags, pol and channels are still checked. */
int egs_feature_gather(int n, int width, int height, const float* rec, const EgsPolicy* pol, const int32_t* ranges,
                       const int32_t* gsid, const int32_t* contrib, int flags, int channels, const float* gmap,
                       float* gfeats, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EGS_FEAT_H_ */
