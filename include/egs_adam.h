/* C ABI of libegs_adam.so: visibility-masked ("sparse") Adam for AMD Instinct MI355X (gfx950).
 *
 * A training step renders a few views, and a view sees a fraction of the model.  The Gaussians no view of the step saw
 * receive an exactly zero gradient, yet dense Adam (egs_adam_step, include/egs_hip.h) still reads and writes their 7 x 4
 * bytes per parameter -- and still MOVES them: their old first moment keeps being applied and their second moment keeps
 * decaying.  The masked step of Taming-3DGS (gsplat's SelectiveAdam) updates a Gaussian only in the steps that saw it:
 *
 *   visible[i] == 0   row i of param, exp_avg and exp_avg_sq keeps its bit pattern in every tensor of the call, and row i
 *                     of the gradient is never read (a NaN there changes nothing)
 *   visible[i] != 0   row i gets exactly the element update of egs_adam_step / egs_adam_sh_factored at the same `step`:
 *                     the same float32 result, to the bit
 *
 * Bias correction uses the tensor's own step count (`step`, 1-based, the count AFTER this update), which the caller
 * advances on every call for the tensor as a whole -- as gsplat does -- not a count per Gaussian.
 *
 * A library of its own beside libegs_hip.so, libegs_mcmc.so, libegs_prune.so and libegs_feat.so, whose surfaces and ABI
 * numbers it leaves alone.  Same conventions: raw device pointers and a HIP stream (hipStream_t as void*), no device
 * synchronisation, every argument validated BEFORE any HIP call; return 0 on success, otherwise EGS_ERR_BAD_ARG or a
 * hipError_t, and the last-error string of THIS library describes it.
 */
#ifndef EGS_ADAM_H_
#define EGS_ADAM_H_

#include <stddef.h>
#include <stdint.h>

#include "egs_hip.h" /* EgsAdamGroup, EGS_ERR_BAD_ARG */

#ifdef __cplusplus
extern "C" {
#endif

#define EGS_ADAM_ABI_VERSION 1
#define EGS_SPARSE_ADAM_MAX_GROUPS 8

int egs_adam_abi_version(void);
const char* egs_adam_last_error_string(void);

/* One [n][width] tensor of a masked step, with its gradient and moments (all 16-B aligned, contiguous). */
typedef struct EgsSparseAdamGroup {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  int32_t width; /* floats per Gaussian, > 0 */
  float lr;
  int32_t step; /* >= 1 */
} EgsSparseAdamGroup;

/* All groups (at most EGS_SPARSE_ADAM_MAX_GROUPS) in one launch; every group has exactly n rows, n * width < 2^31.
 *   visible  uint8 [n]; non-zero: the step saw the Gaussian (torch.bool storage is accepted as is)
 * betas / eps are doubles because torch derives 1 - beta and the bias corrections in double.
 * n == 0 or n_groups == 0 returns 0 without a launch (the other arguments are still checked). */
int egs_sparse_adam_step(int n_groups, const EgsSparseAdamGroup* groups, int n, const uint8_t* visible, double beta1,
                         double beta2, double eps, void* stream);

/* The masked form of egs_adam_sh_factored (include/egs_hip.h): same arguments, same sh_dim set {3, 12, 27, 48}, same raw
 * (low [n][3] + high [n][sh_dim - 3]) / whole-tensor (high == NULL: low is [n][sh_dim]) split and same refusals, plus
 * `visible` as above.  A workgroup whose 64 Gaussians are all invisible touches neither pws, rows nor the tensors. */
int egs_sparse_adam_sh_factored(int n, int sh_dim, int views, const float* pws, const float* rows, int64_t row_stride,
                                float scale, const EgsAdamGroup* low, const EgsAdamGroup* high /*nullable*/,
                                const uint8_t* visible, double beta1, double beta2, double eps, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EGS_ADAM_H_ */
