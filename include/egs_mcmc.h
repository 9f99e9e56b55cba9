/* C ABI of libegs_mcmc.so: MCMC densification for the Gaussian-splatting trainer on AMD Instinct MI355X (gfx950).
 *
 * "3D Gaussian Splatting as Markov Chain Monte Carlo" (Kheradmand et al., NeurIPS 2024) replaces the clone / split /
 * prune / alpha-reset heuristic by
 *   - a hard cap on the number of Gaussians,
 *   - relocation of dead Gaussians onto live ones (and growth by the same move) with an opacity and scale correction
 *     that leaves the rendered image unchanged,
 *   - a position noise shaped by each Gaussian's covariance, added after every optimizer step,
 *   - two L1 regularisers (opacity, scale) that push unused Gaussians towards death.
 *
 * A library of its own beside libegs_hip.so (include/egs_hip.h), whose surface and ABI number it leaves alone.  Same
 * conventions: raw device pointers and a HIP stream (hipStream_t as void*), float32 row-major tensors, no device
 * synchronisation, every argument validated BEFORE any HIP call; return 0 on success, otherwise EGS_MCMC_ERR_BAD_ARG
 * or a hipError_t, and the last-error string of THIS library describes it.
 *
 * The parameters are the optimizer's raw tensors (gsplat/gsmodel.py:96-129): o = sigmoid(alphas_raw) [N][1],
 * s = exp(scales_raw) [N][3], q = rots_raw / |rots_raw| [N][4] (w x y z), pws [N][3], low_shs [N][3],
 * high_shs [N][high_sh_width].
 *
 * Random streams (counter-based generator of csrc/egs_rng.h == scene.uniform01 / scene.normal; element e of stream s
 * is a pure function of (seed, s, e), so data-parallel replicas agree without a broadcast):
 *   sampling   draw j of sampling round r   u = uniform01(seed, EGS_MCMC_STREAM_SAMPLE + r, j)
 *   noise      component c of row i, step t z = unit_normal(seed, EGS_MCMC_STREAM_NOISE + t, 3 i + c)
 * unit_normal(seed, s, e) reads the uniform streams 2 s + 1000 and 2 s + 1001.  The split offsets of egs_densify_apply
 * are unit_normal(seed, round, .): uniform streams 1000 + 2 round and 1001 + 2 round, below 2^41 for round < 2^40.  The
 * noise reads the uniform streams 2^41 + 1000 + 2 t and 2^41 + 1001 + 2 t, below 2^62 for t < 2^60; sampling reads
 * 2^62 + r.  The three ranges never meet.
 */
#ifndef EGS_MCMC_H_
#define EGS_MCMC_H_

#include <stddef.h>
#include <stdint.h>

#include "egs_hip.h" /* EgsGaussianParams */

#ifdef __cplusplus
extern "C" {
#endif

#define EGS_MCMC_ABI_VERSION 1

#define EGS_MCMC_ERR_BAD_ARG 10001

#define EGS_MCMC_STREAM_SAMPLE (1ull << 62)
#define EGS_MCMC_STREAM_NOISE (1ull << 40)

/* the correction below is evaluated for at most this many copies of one Gaussian (the paper's code: n_max = 51) */
#define EGS_MCMC_N_MAX 51

int egs_mcmc_abi_version(void);
const char* egs_mcmc_last_error_string(void);

/* 1. Sampling weights.  Per row i of n:
 *      o         = sigmoid(alphas_raw[i])
 *      dead[i]   = o <= min_opacity                                  (uint8)
 *      weight[i] = relocation ? (dead[i] ? 0 : o) : o                (float32)
 *    totals (device, int32[2]) = {n_dead, n_live}, n_live = n - n_dead.  Integer atomics: order-independent.  The host
 *    reads the 8 bytes back -- the one synchronisation of a refinement.  n == 0: totals = {0, 0}. */
int egs_mcmc_weights(int n, const float* alphas_raw, float min_opacity, int relocation, float* weight, uint8_t* dead,
                     int32_t* totals, void* stream);

/* 2. Weighted sampling with replacement.
 *      cdf[i] = weight[0] + ... + weight[i] in DOUBLE, in a fixed order: a scan inside workgroups of 1024 rows, a
 *               scan of the workgroup sums by one workgroup, a pass that adds them; no atomics -- the same bits on
 *               every run and every replica
 *      total  = cdf[n - 1]
 *      idx[j] = the first i with cdf[i] > u_j total,  u_j = uniform01(seed, EGS_MCMC_STREAM_SAMPLE + round, j)
 *    by binary search.  u_j < 1, so such an i exists, and cdf[i] > cdf[i - 1] there: a row of weight 0 is never
 *    returned.  (Where the sum is not exact in double, the rounding of a parallel scan could make cdf differ by an
 *    ulp across a row of weight 0; the search then moves on to the next row of positive weight, or back to the last.)
 *    Weights must be >= 0 and finite.  n_positive is the number of rows of positive weight as the host knows it from
 *    the totals it read back (n_live for relocation weights): n_positive <= 0 -- nothing alive, total == 0 -- is
 *    EGS_MCMC_ERR_BAD_ARG, so the call itself never waits for the device.
 *    ws: egs_mcmc_sample_ws_bytes(n) bytes, 256-B aligned.  idx: int32[n_draws], every entry in [0, n). */
size_t egs_mcmc_sample_ws_bytes(int n);
int egs_mcmc_sample(int n, const float* weight, int n_positive, int n_draws, uint64_t seed, uint64_t round,
                    int32_t* idx, void* ws, size_t ws_bytes, void* stream);

/* 3. Relocation / growth: row dst[j] becomes a copy of row src[j], j < n_draws, and every Gaussian that is now
 *    present count times -- count[i] = 1 + the number of draws with src == i -- gets the opacity and scale that leave
 *    the rendered image unchanged.  With N = min(count, EGS_MCMC_N_MAX), o the source's opacity, s its scale vector:
 *      o' = 1 - (1 - o)^(1/N)
 *      D  = sum_{i=1..N} sum_{k=0..i-1} C(i-1,k) (-1)^k / sqrt(k+1) o'^(k+1)
 *      s' = s o / D
 *      o' is then clamped to [min_opacity, 1 - 1e-6];  written: logit(o'), log(s')
 *    all in double from the float32 raw values (binomials by the exact recurrence C(m,k) = C(m,k-1) (m-k+1) / k).
 *    For N = 1, D = o: an undrawn row is not touched at all.
 *    Three launches on the stream, whose order removes the read-after-write hazard on the source rows:
 *      a. counts into the zeroed workspace (integer atomics)
 *      b. per draw: pws, low_shs, high_shs, rots_raw of the source copied to row dst; corrected alphas_raw and
 *         scales_raw from the source's ORIGINAL values; the moments of row dst zeroed
 *      c. per source with count > 1: its own alphas_raw / scales_raw rewritten with the same values, ALL its moments
 *         zeroed (a relocated or thinned Gaussian is not the one its moments describe)
 *    dst rows must be distinct and never a source (dead rows have weight 0; growth rows lie past the old rows).
 *    src / dst entries outside [0, n_rows) are skipped.  exp_avg / exp_avg_sq: both given or both NULL (an optimizer
 *    without state yet).  params and moments hold n_rows rows and are updated in place.
 *    ws: egs_mcmc_relocate_ws_bytes(n_rows) bytes, 256-B aligned. */
size_t egs_mcmc_relocate_ws_bytes(int n_rows);
int egs_mcmc_relocate(int n_rows, int n_draws, int high_sh_width, const int32_t* src, const int32_t* dst,
                      const EgsGaussianParams* params, const EgsGaussianParams* exp_avg,
                      const EgsGaussianParams* exp_avg_sq, float min_opacity, void* ws, size_t ws_bytes, void* stream);

/* 4. Gradient of  lambda_o mean(sigmoid(alphas_raw)) + lambda_s mean(exp(scales_raw)), added in place:
 *      g_alpha[i]    += lambda_o / n     o (1 - o)
 *      g_scale[i][c] += lambda_s / (3 n) s_c
 *    48 bytes of traffic per Gaussian. */
int egs_mcmc_add_reg_grad(int n, const float* alphas_raw, const float* scales_raw, float lambda_o, float lambda_s,
                          float* g_alphas_raw, float* g_scales_raw, void* stream);

/* 5. Position noise after the optimizer step:
 *      z   = unit_noise[i] (nullable, [n][3]) or unit_normal(seed, EGS_MCMC_STREAM_NOISE + step, 3 i + c)
 *      w   = 1 / (1 + exp(-100 ((1 - o) - 0.995)))
 *      pws[i] += R diag(s^2) R^T (z w noise_lr lr_pws)
 *    the covariance itself, not its square root, as in the paper's code.  56 bytes of traffic per Gaussian. */
int egs_mcmc_add_noise(int n, float* pws, const float* alphas_raw, const float* scales_raw, const float* rots_raw,
                       const float* unit_noise, float noise_lr, float lr_pws, uint64_t seed, uint64_t step,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EGS_MCMC_H_ */
