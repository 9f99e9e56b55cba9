/* C ABI of libegs_bilagrid.so: bilateral-grid appearance compensation for AMD Instinct MI355X (gfx950).
 *
 * A grid G is float32 [12][L][Gh][Gw], contiguous: channel 4c + j is entry (c, j) of a 3 x 4 affine colour transform A.
 * An image is planar float32 [3][H][W].  Pixel (x, y) with colour rgb reads the lattice at
 *
 *   gx = x (Gw - 1) / max(W - 1, 1)     gy = y (Gh - 1) / max(H - 1, 1)
 *   gz = clamp(0.299 r + 0.587 g + 0.114 b, 0, 1) (L - 1)
 *
 * trilinearly (torch grid_sample, bilinear, border padding, align_corners) and leaves out_c = sum_j A[c][j] rgb_j + A[c][3].
 * The backward pass gives the adjoint of the interpolation for G and, for the image, A^T[:, :3] dout plus the guidance
 * term through the luminance (zero when L == 1 or the luminance lies outside (0, 1)).
 *
 * Every entry point picks one of two kernels from (H, W, Gw, Gh, L) alone: a workgroup owns a block of
 * EGS_BILAGRID_BLOCK_W x EGS_BILAGRID_BLOCK_H pixels; when the box of lattice nodes that the largest block can touch holds
 * at most EGS_BILAGRID_LDS_FLOATS floats the box is staged (forward) or accumulated (backward) in LDS, otherwise the
 * kernel works on global memory.  `out` and `dimage` are written without atomics and are bitwise reproducible; `dgrid`
 * is summed with float atomics and is NOT.
 *
 * A library of its own beside libegs_hip.so and the other side libraries, whose surfaces and ABI numbers it leaves alone.
 * Raw device pointers (4-B aligned) and a HIP stream (hipStream_t as void*) on device `device`; no device
 * synchronisation, no allocation, no environment variable; every argument is validated BEFORE any HIP call.  Return 0 on
 * success, otherwise EGS_ERR_BAD_ARG or a hipError_t, and the last-error string of THIS library describes it.
 */
#ifndef EGS_BILAGRID_H_
#define EGS_BILAGRID_H_

#include <stddef.h>
#include <stdint.h>

#include "egs_hip.h" /* EGS_ERR_BAD_ARG */

#ifdef __cplusplus
extern "C" {
#endif

#define EGS_BILAGRID_ABI_VERSION 1
/* the pixel block of one workgroup */
#define EGS_BILAGRID_BLOCK_W 64
#define EGS_BILAGRID_BLOCK_H 32
/* LDS budget of one box of lattice nodes: 32 KiB (the backward pass holds two, G and dG: 64 KiB) */
#define EGS_BILAGRID_LDS_FLOATS 8192
/* limits: Gw Gh L 12 floats per grid; (W - 1)(Gw - 1) and (H - 1)(Gh - 1), which the kernels form in float32 exactly */
#define EGS_BILAGRID_MAX_GRID_FLOATS (1 << 24)
#define EGS_BILAGRID_MAX_COORD_PRODUCT (1 << 22)

int egs_bilagrid_abi_version(void);
const char* egs_bilagrid_last_error_string(void);

/* out [3][H][W] = the image under the grid.  `out` may not alias `image`. */
int egs_bilagrid_slice(int device, void* stream, int H, int W, int Gw, int Gh, int L, const float* image,
                       const float* grid, float* out);

/* dimage [3][H][W] (nullable) is WRITTEN; dgrid [12][L][Gh][Gw] (nullable) is ACCUMULATED INTO.  Both null: returns 0
 * without a launch (image, grid and dout are still checked). */
int egs_bilagrid_slice_bwd(int device, void* stream, int H, int W, int Gw, int Gh, int L, const float* image,
                           const float* grid, const float* dout, float* dimage, float* dgrid);

/* TV(G) = sum over the axes x, y, z of the mean of the squared forward differences along the axis (an axis of size 1
 * contributes 0).  Writes weight TV to *value_out (one device float) and adds weight dTV/dG to dgrid (nullable), in one
 * launch of one workgroup, without atomics: both are bitwise reproducible. */
int egs_bilagrid_tv(int device, void* stream, int Gw, int Gh, int L, const float* grid, float weight, float* value_out,
                    float* dgrid);

#ifdef __cplusplus
}
#endif
#endif /* EGS_BILAGRID_H_ */
