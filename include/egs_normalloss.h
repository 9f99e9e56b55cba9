/* C ABI of libegs_normalloss.so: surface-normal supervision and edge-aware normal smoothness on the render's depth and
 * opacity maps, for AMD Instinct MI355X (gfx950).
 *
 * D (depth = sum w_i z_i), A (alpha = sum w_i): planar float32 [H][W]; intrinsics fx, fy, cx, cy; optional prior normals
 * q [3][H][W] in the CAMERA frame (x right, y down, z forward: a surface facing the camera has n_z < 0); optional guide
 * image I [3][H][W]; optional weight w >= 0 [H][W].
 *
 * Depth validity.  A pixel is DEPTH-VALID when A > alpha_min and D > 0 (comparisons that are false for NaN).
 * Back-projection.  z = D / A and p(x, y) = z ((x - cx) / fx, (y - cy) / fy, 1) with INTEGER pixel coordinates (the draw
 *   kernels evaluate a Gaussian at u - (px, py): no half-pixel offset).
 * Normal.  dx = p(x+1, y) - p(x-1, y), dy = p(x, y+1) - p(x, y-1), c = dy x dx, n = c / |c|: a fronto-parallel surface
 *   gives n = (0, 0, -1).
 * Normal validity.  A pixel is NORMAL-VALID when it and its four neighbours lie inside the image, all five are
 *   depth-valid, and |c|^2 > 0 and is finite.  Elsewhere n = 0.  (A plane with H < 3 or W < 3 has no such pixel.)
 * Weight.  omega = normal-valid ? (w or 1) : 0.
 *
 * Prior term.  A prior pixel HAS DATA when its three components are finite and |q|^2 > 0; qh = q / |q| (normalised
 *   here).  omega_p = omega at pixels with data, else 0; Omega_p = sum omega_p;
 *     L_p = sum omega_p (1 - n . qh) / Omega_p
 * Smoothness term.  Over the horizontal and vertical neighbour pairs (a, b), with Omega_s = sum omega_a omega_b:
 *     L_s = sum omega_a omega_b g_ab (1 - n_a . n_b) / Omega_s
 *   g_ab = exp(-edge_gamma mean_c |I_a - I_b|), or 1 without a guide.  1 - n_a . n_b = |n_a - n_b|^2 / 2 (the form the
 *   kernels evaluate): the term is smooth and needs no left-out-pixel rule.
 * Gradients.  dloss_ddepth and dloss_dalpha are those of prior_scale L_p + smooth_scale L_s through z = D / A, exactly
 *   0 at pixels that are not depth-valid.  No gradient goes to q, I or w.
 * Degenerate rules, decided on the device: Omega_p = 0 (with a prior given) or Omega_s = 0 (with the smoothness term
 *   asked for) makes that term 0 with a zero gradient and sets bit 0 or bit 1 of stats[5].
 *
 * alpha_min keeps z = D / A away from almost-empty pixels and edge_gamma sets how fast an image edge switches the
 * smoothness off; callers pass 0.05 and 10, values NOBODY HAS TUNED.  The values of w, q and I are not inspected beyond
 * the rules above: a negative or non-finite weight or guide gives a meaningless result, never an out-of-bounds access.
 * w == NULL and w == 1 everywhere give the same bits, and so do I == NULL and a constant I.
 *
 * At most three launches: the tile pass (z and validity with a one-pixel halo in LDS -> n and 1 / |c| into the workspace,
 * normals_out, the prior sums), the pair pass (the smoothness sums, skipped without that term) and the gradient pass in
 * gather form, in which every workgroup reduces the per-workgroup partial sums in the same fixed order, in double.
 * Without a gradient the last launch is one workgroup.  The per-pixel arithmetic is double.  No floating-point atomic:
 * the result is bitwise reproducible from call to call, stream to stream and with or without gradient planes, and the
 * host reads nothing back.
 *
 * A library of its own beside libegs_hip.so and the other side libraries, whose surfaces and ABI numbers it leaves alone.
 * Raw device pointers (4-B aligned; ws 16-B) on the CURRENT device and a HIP stream (hipStream_t as void*); no device
 * synchronisation, no allocation, no environment variable; every argument is validated BEFORE any HIP call.  Return 0 on
 * success, otherwise EGS_ERR_BAD_ARG, EGS_ERR_WORKSPACE or a hipError_t, and the last-error string of THIS library
 * describes it.
 */
#ifndef EGS_NORMALLOSS_H_
#define EGS_NORMALLOSS_H_

#include <stddef.h>
#include <stdint.h>

#include "egs_hip.h" /* EGS_ERR_BAD_ARG, EGS_ERR_WORKSPACE */

#ifdef __cplusplus
extern "C" {
#endif

#define EGS_NORMALLOSS_ABI_VERSION 1
/* the largest plane: H W pixels (the workspace holds 32 B per pixel) */
#define EGS_NORMALLOSS_MAX_PIXELS (1 << 26)
/* the interior of a tile of the tile and gradient passes: one workgroup of 256 threads, one pixel each */
#define EGS_NORMALLOSS_TILE_W 32
#define EGS_NORMALLOSS_TILE_H 8

int egs_normalloss_abi_version(void);
const char* egs_normalloss_last_error_string(void);

/* bytes of workspace egs_normalloss needs for an H x W plane (256 for a non-positive or too large size) */
size_t egs_normalloss_ws_bytes(int H, int W);

/* stats: 6 device floats {L_p, L_s, Omega_p, Omega_s, number of normal-valid pixels, degenerate flags}.
 * normals == NULL: no prior term (L_p = Omega_p = 0).  smooth == 0: no smoothness term (L_s = Omega_s = 0).
 * guide == NULL: g = 1.  weight == NULL: w = 1.  normals_out: nullable, [3][H][W], every entry written.
 * dloss_ddepth, dloss_dalpha [H][W]: both NULL (no gradient) or both WRITTEN, every entry; the three outputs alias no
 * input and not each other.  fx, fy > 0 and finite, cx, cy finite, alpha_min >= 0, edge_gamma >= 0, both scales finite.
 * ws: device memory of at least egs_normalloss_ws_bytes(H, W) bytes; scratch. */
int egs_normalloss(int H, int W, const float* depth, const float* alpha, float fx, float fy, float cx, float cy,
                   const float* normals, const float* guide, const float* weight, int smooth, float alpha_min,
                   float edge_gamma, float prior_scale, float smooth_scale, void* ws, size_t ws_bytes, float* stats,
                   float* normals_out, float* dloss_ddepth, float* dloss_dalpha, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EGS_NORMALLOSS_H_ */
