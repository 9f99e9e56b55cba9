/* C ABI of libegs_depthloss.so: the fused depth-prior loss on the render's depth and opacity maps, for AMD Instinct
 * MI355X (gfx950).
 *
 * D (depth = sum w_i z_i), A (alpha = sum w_i), q (prior DISPARITY, inverse depth), w (optional weight >= 0): planar
 * float32 [H][W].  A pixel is VALID when q > 0, q is finite, A > alpha_min and D > 0 (comparisons that are false for NaN).
 * With omega = valid ? (w or 1) : 0, the rendered disparity r = A / D (the reciprocal of the expected depth D / A) and
 * Omega = sum omega:
 *
 *   EGS_DEPTHLOSS_METRIC   s = 1, t = 0
 *   EGS_DEPTHLOSS_AFFINE   (s, t): the omega-weighted least-squares fit of s q + t to r, from Omega, sum omega q,
 *                          sum omega q^2, sum omega r, sum omega q r.  (s, t) are CONSTANTS for the gradient
 *                          (stop-gradient): the gradient is that of the L1 term under the fit of this call.
 *     both:  e = r - (s q + t),  loss = sum omega |e| / Omega,  dloss/dr = omega sign(e) / Omega, sign(0) = 0
 *   EGS_DEPTHLOSS_PEARSON  loss = 1 - rho, rho the omega-weighted correlation of q and r (also needs sum omega r^2);
 *                          exact gradient, with means qm, rm and standard deviations sq, sr:
 *                          dloss/dr = -(omega / Omega) / (sq sr) [(q - qm) - rho (sq / sr) (r - rm)]
 *
 *   dloss_ddepth = -grad_scale dloss/dr A / D^2      dloss_dalpha = grad_scale dloss/dr / D      (0 at invalid pixels)
 *
 * Degenerate cases, decided on the device (stats[5] = 1):
 *   Omega == 0: loss 0, s = 1, t = 0, gradient 0.
 *   AFFINE, the weighted variance of q at most 1e-12 of its mean square, or fewer than two valid pixels:
 *     t = 0, s = sum omega q r / sum omega q^2.
 *   PEARSON, the weighted variance of q or of r at most 1e-12 of its mean square: loss 1, rho 0, gradient 0.
 *
 * alpha_min guards the 1 / D^2 factor at almost-empty pixels; callers pass 0.05, a value nobody has tuned.  The values
 * of w are not inspected: a negative or non-finite weight gives a meaningless result, never an out-of-bounds access.
 * w == NULL and w == 1 everywhere give the same bits.
 *
 * Two launches: the sums, then the gradient, in which every workgroup reduces the per-workgroup partial sums in the same
 * fixed order, in double, and solves the fit itself.  Without a gradient the second launch is one workgroup (AFFINE: the
 * grid again, to sum |e| under the fit, without a store to a gradient plane).  No floating-point atomic: the result is
 * bitwise reproducible from call to call and stream to stream, and the host reads nothing back.
 *
 * A library of its own beside libegs_hip.so and the other side libraries, whose surfaces and ABI numbers it leaves alone.
 * Raw device pointers (4-B aligned; ws 8-B) on the CURRENT device and a HIP stream (hipStream_t as void*); no device
 * synchronisation, no allocation, no environment variable; every argument is validated BEFORE any HIP call.  Return 0 on
 * success, otherwise EGS_ERR_BAD_ARG, EGS_ERR_WORKSPACE or a hipError_t, and the last-error string of THIS library
 * describes it.
 */
#ifndef EGS_DEPTHLOSS_H_
#define EGS_DEPTHLOSS_H_

#include <stddef.h>
#include <stdint.h>

#include "egs_hip.h" /* EGS_ERR_BAD_ARG, EGS_ERR_WORKSPACE */

#ifdef __cplusplus
extern "C" {
#endif

#define EGS_DEPTHLOSS_ABI_VERSION 1
/* the largest plane: H W pixels */
#define EGS_DEPTHLOSS_MAX_PIXELS (1 << 28)

#define EGS_DEPTHLOSS_METRIC 0
#define EGS_DEPTHLOSS_AFFINE 1
#define EGS_DEPTHLOSS_PEARSON 2

int egs_depthloss_abi_version(void);
const char* egs_depthloss_last_error_string(void);

/* bytes of workspace egs_depthloss needs for an H x W plane (256 for a non-positive size) */
size_t egs_depthloss_ws_bytes(int H, int W);

/* stats: 6 device floats {loss, s, t, Omega, rho (0 unless PEARSON), degenerate flag}.  weight is nullable.
 * dloss_ddepth, dloss_dalpha [H][W]: both NULL (no gradient) or both WRITTEN, every entry; they alias no input and not
 * each other.  alpha_min >= 0, grad_scale finite.  ws: device memory of at least egs_depthloss_ws_bytes(H, W) bytes;
 * scratch. */
int egs_depthloss(int H, int W, const float* depth, const float* alpha, const float* prior, const float* weight,
                  int kind, float alpha_min, float grad_scale, void* ws, size_t ws_bytes, float* stats,
                  float* dloss_ddepth, float* dloss_dalpha, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EGS_DEPTHLOSS_H_ */
