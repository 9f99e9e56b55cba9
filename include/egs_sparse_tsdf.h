/* C ABI of libegs_sparsetsdf.so: a BLOCK-ALLOCATED truncated signed distance volume -- the fusion and the marching
 * tetrahedra of include/egs_tsdf.h (which states what a sample and a cell compute; this library calls the same functions
 * of csrc/egs_tsdf_device.h) on a volume that stores only the 8 x 8 x 8-sample blocks near an observed surface, for AMD
 * Instinct MI355X (gfx950).  DESIGN 3.22.
 *
 * STORAGE.  The virtual lattice of nx x ny x nz samples at origin + voxel (ix, iy, iz) is cut into blocks of
 *   EGS_SPARSETSDF_BLOCK = 8 samples a side: nb_k = ceil(n_k / 8) blocks per axis, block (bx, by, bz) has the linear block
 *   index (bz nb_y + by) nb_x + bx and holds the samples 8 b_k .. 8 b_k + 7 (those at or past n_k, in a ragged last block,
 *   exist in the pool and are never updated nor meshed).  All of it is memory the caller owns:
 *     directory    [nb_z][nb_y][nb_x] int32 : -1 for an unallocated block, its pool slot otherwise.  At most
 *                  EGS_SPARSETSDF_MAX_DIRECTORY = 2^27 entries.
 *     block_coords [capacity] int32         : the linear block index of every slot in use (slots 0 .. n_blocks - 1).
 *     tsdf, weight [capacity][512] float32  : 1 and 0 before the first view; within a block x runs fastest, then y, then z:
 *                  sample (lx, ly, lz) of slot s is entry 512 s + 64 lz + 8 ly + lx.
 *     color        [3][capacity][512] float32, optional: 0.
 *   capacity <= EGS_SPARSETSDF_MAX_SLOTS = 2^22, so an index into a plane fits 32 bits, as in the dense kernel.
 *
 * ONE VIEW is four calls, in this order; the caller forms one exclusive scan between the second and the third and reads
 * its total, the number of new blocks, back -- the only readback of a view:
 *   1. egs_sparsetsdf_touch.  A thread per pixel.  The pixel PASSES if it clears steps 3 and 5 of egs_tsdf.h: alpha >
 *      alpha_min (with alpha), z_s finite, > 0 and <= depth_max, pixel weight > 0 and finite.  A passing pixel (px, py)
 *      marches its own ray p_c = z ((px - cx) / fx, (py - cy) / fy, 1) over z in [max(near, z_s - trunc), z_s + trunc]:
 *      the points z_0 + k voxel, k = 0, 1, ..., and the far end itself -- THE MARCH STEP IS ONE VOXEL OF p_c.z.  Each
 *      point goes to the world frame, p_w = R^T (p_c - t), and to the sample nearest to it, i_k = floor((p_w - origin)_k /
 *      voxel + 0.5), of block b_k = floor(i_k / 8).  A point with -1 <= b_k <= nb_k on every axis sets flags[b'] = 1 at
 *      b'_k = min(max(b_k, 0), nb_k - 1): a point in the one-block rim around the grid flags the grid block it touches;
 *      every other point outside the block grid is ignored.  flags [nb_z][nb_y][nb_x] int32 is zeroed by the caller; the
 *      call only ever stores the value 1.
 *      COVERAGE.  Let rho = 0.5 z sqrt(1 / fx^2 + 1 / fy^2) be the half diagonal of a pixel's footprint at depth z, and
 *      |d| = |((px - cx) / fx, (py - cy) / fy, 1)| the length of the ray per unit of z.  If, for every passing pixel and
 *      every z <= z_s + trunc at which the lattice can have a sample (z <= the largest p_c.z of its eight corners),
 *          (rho + 0.5 voxel |d|) / voxel + 0.5  <=  7.5,
 *      then every sample the view updates with t < 1 lies within one block, in Chebyshev distance, of a flagged block
 *      (DESIGN 3.22 has the derivation; the half sample left of the eight is what float32 may lose).  At a pixel footprint
 *      of a voxel or two -- a volume sized for its images -- the left side is below 3.
 *   2. egs_sparsetsdf_mark.  fresh[b] = 1 if block b is unallocated and it or one of its 26 neighbours is flagged (the
 *      dilation by one block the coverage rule needs), else 0; every entry is written.
 *   3. egs_sparsetsdf_assign.  offsets = the exclusive scan of fresh.  Block b with fresh[b] takes slot n_blocks +
 *      offsets[b]: directory[b] and block_coords[slot] are written, new slots in ascending linear block index after all
 *      earlier ones.  A slot at or past `capacity` is never written (the caller grows the pool first).  The pool entries of
 *      a new slot must hold 1 / 0 / 0: the caller initialises them.
 *   4. egs_sparsetsdf_integrate.  Every sample of the slots 0 .. n_blocks - 1 with ix < nx, iy < ny, iz < nz goes through
 *      steps 1-6 of egs_tsdf.h with its lattice coordinates, in the same float32 operations: a sample holds the bits the
 *      dense kernel gives it from the same previous bits.  A thread owns a 16-byte quad of a block's row, decides its four
 *      samples before any pool traffic, touches no pool memory when none is updated, and never writes a skipped sample.
 *      The (slot, quad) items are walked with the stride of the grid, which max_blocks caps as in egs_tsdf_integrate.
 *   SEMANTICS.  A block is updated only from the view that allocates it onwards: free-space observations (t = 1) that
 *   earlier views made of its samples are not recorded.
 *
 * SURFACE.  egs_sparsetsdf_mesh_count / _emit: a workgroup per slot, a thread per cell whose corner 0 is a sample of the
 *   block (512 cells; the far corners are read from up to seven neighbouring blocks through the directory, the 9^3 halo of
 *   tsdf and weight staged in LDS).  A cell is meshed when all eight corners lie inside the lattice, in allocated blocks,
 *   with weight >= min_weight; its triangles are those of egs_tsdf.h: the same coordinates, colours and KEYS -- 7 x (linear
 *   sample index in the virtual lattice) + edge type -- as the dense volume with the same planes.  Order: by slot, then the
 *   local cell 64 lz + 8 ly + lx, then the cell's own order.  counts and offsets have 512 n_blocks entries.
 *
 * No atomics, no hash table: every output is owned by one thread, or is the same-value store of a flag.  Raw device
 * pointers on the CURRENT device (4-B aligned; tsdf, weight and color 16-B, keys and offsets 8-B) and a HIP stream
 * (hipStream_t as void*); no device synchronisation, no allocation, no environment variable; every argument is validated
 * BEFORE any HIP call.  The VALUES in directory and block_coords are checked where an address is formed from them: garbage
 * gives a meaningless result, never an out-of-bounds access.  Return 0 on success, otherwise EGS_ERR_BAD_ARG,
 * EGS_SPARSETSDF_ERR_CAPACITY or a hipError_t, and the last-error string of THIS library describes it.  A library of its
 * own: libegs_tsdf.so and the others keep their surfaces and ABI numbers.
 */
#ifndef EGS_SPARSE_TSDF_H_
#define EGS_SPARSE_TSDF_H_

#include <stddef.h>
#include <stdint.h>

#include "egs_hip.h" /* EGS_ERR_BAD_ARG */

#ifdef __cplusplus
extern "C" {
#endif

#define EGS_SPARSETSDF_ABI_VERSION 1
/* egs_sparsetsdf_mesh_emit: the output buffers hold fewer triangles than the scan's total */
#define EGS_SPARSETSDF_ERR_CAPACITY 10003
/* samples of a block along an axis, and in a block */
#define EGS_SPARSETSDF_BLOCK 8
#define EGS_SPARSETSDF_BLOCK_SAMPLES 512
/* the most directory entries nb_x nb_y nb_z, and the most pool slots */
#define EGS_SPARSETSDF_MAX_DIRECTORY 134217728
#define EGS_SPARSETSDF_MAX_SLOTS 4194304
/* the most workgroups egs_sparsetsdf_integrate launches (max_blocks == 0) */
#define EGS_SPARSETSDF_MAX_BLOCKS 8192
/* the longest march of a pixel, in steps: 2 trunc <= EGS_SPARSETSDF_MAX_MARCH * voxel */
#define EGS_SPARSETSDF_MAX_MARCH 4096

int egs_sparsetsdf_abi_version(void);
const char* egs_sparsetsdf_last_error_string(void);

/* Step 1.  nx, ny, nz > 0 with at most EGS_SPARSETSDF_MAX_DIRECTORY blocks; voxel, fx, fy, trunc > 0 and finite; origin,
 * cx, cy finite; alpha_min, near >= 0 and finite; depth_max > 0, +inf allowed; alpha and pixel_weight nullable; H W < 2^31.
 * 2 trunc <= EGS_SPARSETSDF_MAX_MARCH voxel.  flags aliases no input. */
int egs_sparsetsdf_touch(int nx, int ny, int nz, float ox, float oy, float oz, float voxel, int H, int W,
                         const float* depth, const float* alpha, const float* pixel_weight, float fx, float fy, float cx,
                         float cy, const float* Rcw, const float* tcw, float trunc, float alpha_min, float near,
                         float depth_max, int32_t* flags, void* stream);

/* Step 2.  flags, directory, fresh: [nb_z][nb_y][nb_x] int32, fresh aliasing neither. */
int egs_sparsetsdf_mark(int nx, int ny, int nz, const int32_t* flags, const int32_t* directory, int32_t* fresh,
                        void* stream);

/* Step 3.  offsets [nb_z nb_y nb_x] int64: the exclusive scan of fresh.  0 <= n_blocks <= capacity <=
 * EGS_SPARSETSDF_MAX_SLOTS. */
int egs_sparsetsdf_assign(int nx, int ny, int nz, const int32_t* fresh, const int64_t* offsets, int n_blocks, int capacity,
                          int32_t* directory, int32_t* block_coords, void* stream);

/* Step 4.  color and image: both NULL or both given.  n_blocks == 0: a successful call without a launch.  max_blocks: 0,
 * or a cap on the grid below EGS_SPARSETSDF_MAX_BLOCKS.  No output plane aliases another plane or an input. */
int egs_sparsetsdf_integrate(int nx, int ny, int nz, float ox, float oy, float oz, float voxel, int n_blocks, int capacity,
                             const int32_t* block_coords, float* tsdf, float* weight, float* color, int H, int W,
                             const float* depth, const float* alpha, const float* image, const float* pixel_weight,
                             float fx, float fy, float cx, float cy, const float* Rcw, const float* tcw, float trunc,
                             float alpha_min, float near, float depth_max, int max_blocks, void* stream);

/* counts [512 n_blocks] int32: the triangles of every cell, 0..12, every entry written.  n_blocks == 0: a successful call
 * without a launch. */
int egs_sparsetsdf_mesh_count(int nx, int ny, int nz, int n_blocks, int capacity, const int32_t* directory,
                              const int32_t* block_coords, const float* tsdf, const float* weight, float min_weight,
                              int32_t* counts, void* stream);

/* offsets [512 n_blocks] int64: the EXCLUSIVE scan of the counts, `total` its sum.  verts [out_capacity][3][3] float32,
 * keys [out_capacity][3] int64, colors [out_capacity][3][3] float32 (with color; both NULL or both given).  out_capacity <
 * total: EGS_SPARSETSDF_ERR_CAPACITY, nothing written; no thread writes at or beyond `total` whatever the offsets hold.
 * total == 0: a successful call without a launch. */
int egs_sparsetsdf_mesh_emit(int nx, int ny, int nz, float ox, float oy, float oz, float voxel, int n_blocks, int capacity,
                             const int32_t* directory, const int32_t* block_coords, const float* tsdf, const float* weight,
                             const float* color, float min_weight, const int64_t* offsets, int64_t total,
                             int64_t out_capacity, float* verts, int64_t* keys, float* colors, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EGS_SPARSE_TSDF_H_ */
