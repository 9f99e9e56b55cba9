/* C ABI of libegs_wloss.so: the fused L1 / SSIM training loss with a weight per pixel, for AMD Instinct MI355X (gfx950).
 *
 * x (image), y (gt): planar float32 [3][H][W].  w (weight): float32 [H][W], w >= 0, one plane for the three channels.
 * S is the SSIM map of libegs_hip.so's egs_gau_loss: window statistics of the UNWEIGHTED images, 11 x 11 Gaussian
 * window (sigma 1.5), zero padding, C1 = 1e-4, C2 = 9e-4.  With sum_w the sum of w over the plane:
 *
 *   l1   = sum_c sum_p w_p |x - y|_cp / (3 sum_w)
 *   ssim = sum_c sum_p w_p S_cp       / (3 sum_w)
 *   loss = (1 - lambda) l1 + lambda (1 - ssim)
 *   dloss_dimage = grad_scale dloss/dx
 *
 * A pixel with w = 0 still receives SSIM gradient from weighted pixels up to 5 pixels away (their windows contain it);
 * image or gt content more than 5 pixels (Chebyshev) from every weighted pixel influences nothing.  sum_w == 0 gives
 * loss_out = {0, 0, 1, 0} and a gradient of zeros.  The values of w are not inspected: a negative or non-finite weight
 * gives a meaningless result, never an out-of-bounds access.  w == 1 everywhere gives the bits of egs_gau_loss.
 *
 * Two launches (forward maps, gradient) or, without a gradient, forward maps and a one-workgroup reduction; sum_w is
 * reduced on the device in a fixed order, so the result is bitwise reproducible and the host reads nothing back.
 *
 * A library of its own beside libegs_hip.so and the other side libraries, whose surfaces and ABI numbers it leaves alone.
 * Raw device pointers (4-B aligned) on the CURRENT device and a HIP stream (hipStream_t as void*); no device
 * synchronisation, no allocation, no environment variable; every argument is validated BEFORE any HIP call.  Return 0 on
 * success, otherwise EGS_ERR_BAD_ARG, EGS_ERR_WORKSPACE or a hipError_t, and the last-error string of THIS library
 * describes it.
 */
#ifndef EGS_WLOSS_H_
#define EGS_WLOSS_H_

#include <stddef.h>
#include <stdint.h>

#include "egs_hip.h" /* EGS_ERR_BAD_ARG, EGS_ERR_WORKSPACE */

#ifdef __cplusplus
extern "C" {
#endif

#define EGS_WLOSS_ABI_VERSION 1
/* the largest plane: H W pixels */
#define EGS_WLOSS_MAX_PIXELS (1 << 28)

int egs_wloss_abi_version(void);
const char* egs_wloss_last_error_string(void);

/* bytes of workspace egs_wloss needs for an H x W image (256 for a non-positive size) */
size_t egs_wloss_ws_bytes(int H, int W);

/* loss_out: 4 device floats {loss, l1, ssim, sum_w}.  dloss_dimage [3][H][W] (nullable: no gradient) is WRITTEN, every
 * entry and may alias neither image.  ws: device memory of at least egs_wloss_ws_bytes(H, W) bytes; scratch. */
int egs_wloss(int H, int W, const float* image, const float* gt, const float* weight, float lambda, float grad_scale,
              void* ws, size_t ws_bytes, float* loss_out, float* dloss_dimage, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EGS_WLOSS_H_ */
