/* C ABI of libegs_tsdf.so: fusion of depth maps into a truncated signed distance volume (TSDF) and extraction of its zero
 * level set as a triangle mesh, for AMD Instinct MI355X (gfx950).
 *
 * VOLUME.  A lattice of nx x ny x nz samples at p_w = origin + voxel (ix, iy, iz) in the world frame, x fastest: the
 *   linear index of a sample is (iz ny + iy) nx + ix.  Planar float32 planes the caller owns: tsdf [nz][ny][nx] (1 before
 *   the first view), weight [nz][ny][nx] (0 before the first view), optional color [3][nz][ny][nx] (0).
 *
 * INTEGRATING ONE VIEW.  depth [H][W] is the render's sum w z and alpha [H][W] its sum w; alpha == NULL: depth is a
 *   metric z map (a sensor, a prior).  Optional image [3][H][W], optional per-pixel weight [H][W].  Intrinsics fx, fy, cx,
 *   cy; the pose Rcw [9] (row major) and tcw [3] are DEVICE pointers, so a call enqueues with no host readback.  For each
 *   sample of the sub-box [x0, x1) x [y0, y1) x [z0, z1), in float32, every product and sum rounded on its own (no fused
 *   multiply-add), in this order:
 *     1. p_w = origin + voxel * (float)i per axis;  p_c.k = ((R[k][0] p_w.x + R[k][1] p_w.y) + R[k][2] p_w.z) + tcw[k].
 *        Skip unless p_c.z > near.
 *     2. u = (fx p_c.x) / p_c.z + cx, v = (fy p_c.y) / p_c.z + cy; pixel centres sit at integer coordinates (the
 *        convention of egs_normalloss.h).  px = floor(u + 0.5), py = floor(v + 0.5).  Skip unless 0 <= px < W and
 *        0 <= py < H.
 *     3. With alpha: skip unless alpha[py][px] > alpha_min, then z_s = depth / alpha.  Without: z_s = depth.  Skip unless
 *        z_s is finite, z_s > 0 and z_s <= depth_max (depth_max = +inf: no upper limit).
 *     4. sdf = z_s - p_c.z: projective, along the optical axis, as in KinectFusion and Open3D.  Skip if sdf < -trunc.
 *        t = min(1, sdf / trunc).
 *     5. w = weight[py][px] if given, else 1.  Skip if w <= 0 or w is not finite.
 *     6. With W the sample's weight:  tsdf <- (W tsdf + w t) / (W + w);  color_c <- (W color_c + w image_c) / (W + w);
 *        W <- W + w.
 *   A skipped sample is not written.  Views are integrated in call order; a sample is owned by one thread and there is no
 *   atomic, so the result for a given order is bitwise reproducible, and a launch on a sub-box that holds every sample
 *   the view updates equals the full-lattice launch bit for bit.
 *
 * SURFACE.  The zero level set by marching tetrahedra.
 *   Cells.  Cell (cx, cy, cz), 0 <= c < n - 1 per axis, has the linear index (cz (ny - 1) + cy) (nx - 1) + cx and the
 *     corners o + (dx, dy, dz), d in {0, 1}; a volume with a dimension of 1 has no cell.
 *   Tetrahedra.  Each cell is cut into the six Kuhn tetrahedra that share its main diagonal (0,0,0)-(1,1,1): one per
 *     permutation (a, b, c) of the axes, in lexicographic order (xyz, xzy, yxz, yzx, zxy, zyx), with the vertices
 *     {o, o + e_a, o + e_a + e_b, o + e_a + e_b + e_c}.  The triangulation is translation invariant: neighbouring cells
 *     agree on their shared faces, the mesh is watertight by construction.
 *   Valid cells.  A cell emits triangles only if all eight corners have weight >= min_weight (min_weight > 0).
 *   Inside.  A corner is inside iff tsdf < 0; exactly 0 is outside.  A tetrahedron with one or three inside corners gives
 *     one triangle, with two a planar quad as two triangles: a cell gives 0..12.
 *   Vertices.  A vertex lies on a lattice edge between a lower endpoint lo and an upper one hi = lo + d, d in {0,1}^3:
 *     t = f_lo / (f_lo - f_hi), coordinate k = (origin_k + voxel * (float)lo_k) + (d_k ? t * voxel : 0), colour
 *     c_lo + t (c_hi - c_lo), all float32 without fused multiply-add.  Every cell and tetrahedron that shares the edge
 *     computes bit-identical coordinates and colours.
 *   Edge types.  By d = (dx, dy, dz): 0 (1,0,0), 1 (0,1,0), 2 (0,0,1) the axis edges; 3 (1,1,0), 4 (1,0,1), 5 (0,1,1)
 *     the face diagonals; 6 (1,1,1) the body diagonal.
 *   Keys.  key = 7 * (linear sample index of lo) + type, int64: equal keys, equal vertices (the caller welds by key).
 *   Orientation.  The normal (b - a) x (c - a) of a triangle (a, b, c) points from negative to positive tsdf: out of the
 *     surface, towards the cameras.
 *   Order.  By cell index, then tetrahedron, then triangle.
 *
 * alpha_min = 0.5, trunc = 4 voxels and min_weight = 1 are what the Python layer passes by default: values
 * NOBODY HAS TUNED.  The VALUES of the planes and maps are not inspected beyond the rules above: garbage in gives a
 * meaningless result, never an out-of-bounds access.
 *
 * Limits: nx ny nz < 2^31, H W < 2^31, the number of triangles T < 2^31.
 *
 * A library of its own beside libegs_hip.so and the other side libraries, whose surfaces and ABI numbers it leaves alone.
 * Raw device pointers on the CURRENT device (4-B aligned; tsdf, weight and color 16-B, keys and offsets 8-B) and a HIP
 * stream (hipStream_t as void*); no device synchronisation, no allocation, no environment variable; every argument is
 * validated BEFORE any HIP call.  Return 0 on success, otherwise EGS_ERR_BAD_ARG, EGS_TSDF_ERR_CAPACITY or a hipError_t,
 * and the last-error string of THIS library describes it.
 */
#ifndef EGS_TSDF_H_
#define EGS_TSDF_H_

#include <stddef.h>
#include <stdint.h>

#include "egs_hip.h" /* EGS_ERR_BAD_ARG */

#ifdef __cplusplus
extern "C" {
#endif

#define EGS_TSDF_ABI_VERSION 1
/* egs_tsdf_mesh_emit: the output buffers hold fewer triangles than the scan's total */
#define EGS_TSDF_ERR_CAPACITY 10003
/* the most workgroups egs_tsdf_integrate launches (max_blocks == 0); they walk the rows of the sub-box with that stride */
#define EGS_TSDF_MAX_BLOCKS 8192
/* the most triangles of a cell */
#define EGS_TSDF_CELL_TRIANGLES 12

int egs_tsdf_abi_version(void);
const char* egs_tsdf_last_error_string(void);

/* One view into the sub-box [x0,x1) x [y0,y1) x [z0,z1) of the lattice (0 <= x0 <= x1 <= nx, ...; an empty box is a
 * successful call without a launch).  color and image: both NULL or both given.  alpha, pixel_weight: nullable.  voxel,
 * fx, fy, trunc > 0 and finite; origin, cx, cy finite; alpha_min, near >= 0 and finite; depth_max > 0, +inf allowed.
 * max_blocks: 0, or a cap on the grid below EGS_TSDF_MAX_BLOCKS (a caller that wants the stride walk on a small volume).
 * No output plane aliases another plane or an input. */
int egs_tsdf_integrate(int nx, int ny, int nz, float ox, float oy, float oz, float voxel, int x0, int x1, int y0, int y1,
                       int z0, int z1, float* tsdf, float* weight, float* color, int H, int W, const float* depth,
                       const float* alpha, const float* image, const float* pixel_weight, float fx, float fy, float cx,
                       float cy, const float* Rcw, const float* tcw, float trunc, float alpha_min, float near,
                       float depth_max, int max_blocks, void* stream);

/* counts [(nx-1)(ny-1)(nz-1)] int32: the triangles of every cell, 0..12, every entry written.  A volume without a cell
 * is a successful call without a launch. */
int egs_tsdf_mesh_count(int nx, int ny, int nz, const float* tsdf, const float* weight, float min_weight, int32_t* counts,
                        void* stream);

/* offsets [(nx-1)(ny-1)(nz-1)] int64: the EXCLUSIVE scan of the counts, formed by the caller, and `total` its sum.
 * verts [capacity][3][3] float32, keys [capacity][3] int64, colors [capacity][3][3] float32 (with color; both NULL or
 * both given): triangle offsets[cell] + k is the k-th of the cell.  capacity < total: EGS_TSDF_ERR_CAPACITY, nothing
 * written; no thread writes at or beyond `total` whatever the offsets hold.  total == 0: a successful call without a
 * launch (verts and keys may then be NULL). */
int egs_tsdf_mesh_emit(int nx, int ny, int nz, float ox, float oy, float oz, float voxel, const float* tsdf,
                       const float* weight, const float* color, float min_weight, const int64_t* offsets, int64_t total,
                       int64_t capacity, float* verts, int64_t* keys, float* colors, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EGS_TSDF_H_ */
