/* C ABI of libegs_simplify.so: vertex-clustering simplification of an indexed triangle mesh on the device, with
 * quadric-optimal cluster representatives (Lindstrom's out-of-core scheme; what Open3D calls simplify_vertex_clustering with
 * Quadric contraction), for AMD Instinct MI355X (gfx950).  Every cell of a uniform grid that holds a vertex becomes ONE
 * vertex, placed where it minimises the summed squared distance to the planes of the faces that touched the cell; faces
 * that collapse and duplicate faces are dropped.
 *
 * MESH.  The inputs of egs_meshops.h: vertices [V][3] float32, faces [F][3] int64, optional colors [V][3] float32, V, F <
 *   2^31.  A face with an index outside [0, V) is SKIPPED everywhere: it contributes to no quadric and is never kept.  No
 *   input VALUE is trusted to stay inside a buffer (keys, cluster ids, CSR rows, sort orders): what would index outside is
 *   skipped or clamped; garbage in gives a meaningless mesh, never an out-of-bounds access.
 *
 * CELLS.  origin: three doubles, cell: a double > 0.  For a vertex p, i_k = floor(((double)p_k - origin_k) / cell), with
 *   IEEE subtraction, division and floor in double; i_k is clamped to [0, 2^21 - 1] and NaN goes to 0;
 *   key = i_x | i_y << 21 | i_z << 42 as int64.  The caller guarantees finite vertices, origin <= the bounding box minimum and
 *   an extent below 2^21 cells (the Python layer raises ValueError otherwise): the clamp is there for memory safety only.
 *   The CENTRE of a cell is c_k = origin_k + ((double)i_k + 0.5) * cell, the indices taken back out of the key.
 *
 * CLUSTERS.  The distinct keys in ASCENDING key order (the caller's unique with its inverse): cluster[v] [V] int64 is the rank
 *   of v's key, Vc their number.  The members of a cluster are its vertices in ASCENDING vertex index, in CSR form the caller
 *   builds from a stable sort of cluster[]: members [V] int64, member_start [Vc + 1] int64.
 *
 * PER-VERTEX QUADRIC.  With c the centre of v's cell, walk v's row of the vertex-to-face incidence of egs_meshops.h (rows
 *   [3F], row_start [V + 1], entries e = 3 f + k) in row order.  For the face (a, b, c2) of an entry, all in double, every
 *   operation rounded on its own (no fused multiply-add), u = b - a, w = c2 - a:
 *     n = (uy wz - uz wy, uz wx - ux wz, ux wy - uy wx),  L = sqrt((nx nx + ny ny) + nz nz);
 *     L zero or not finite: the entry contributes nothing;  otherwise with inv = 1 / L, m = inv * n (componentwise),
 *     r = a - c,  d = (nx rx + ny ry) + nz rz:
 *     A_v += (mx nx, mx ny, mx nz, my ny, my nz, mz nz)   (a00 a01 a02 a11 a12 a22),   g_v += (d mx, d my, d mz).
 *   This is Garland and Heckbert's plane quadric weighted by twice the face's area, with the cell centre as the reference
 *   point.  A face counts once per (face, corner) entry: a face with two corners in one cluster counts twice there.  The nine
 *   sums start at +0.
 *
 * PER-CLUSTER SOLVE.  Over the members in ascending order, each sum starting at +0, in double:
 *     A = sum A_v,  g = sum g_v,  s = sum ((double)p_v - c),  col = sum (double)colour_v.
 *   y_m = s / count.  tr = (a00 + a11) + a22,  rho = 1e-3 * tr.  If tr > 0 and finite, solve (A + rho I) y = g + rho y_m by the
 *   Cholesky factorisation below -- the matrix is positive definite with condition <= 1001 by construction --, otherwise
 *   y = y_m.  With B = A + rho I (only the diagonal changes) and b = g + rho * y_m:
 *     l00 = sqrt(b00)  l10 = b01 / l00  l20 = b02 / l00  l11 = sqrt(b11 - l10 l10)  l21 = (b12 - l20 l10) / l11
 *     l22 = sqrt((b22 - l20 l20) - l21 l21)
 *     z0 = b0 / l00  z1 = (b1 - l10 z0) / l11  z2 = ((b2 - l20 z0) - l21 z1) / l22
 *     y2 = z2 / l22  y1 = (z1 - l21 y2) / l11  y0 = ((z0 - l10 y1) - l20 y2) / l00.
 *   y is clamped componentwise to [-cell / 2, cell / 2] (y < -h ? -h : y > h ? h : y), x = c + y, each component rounded ONCE
 *   to float32.  With placement MEAN, x = c + y_m and no quadric is formed.  The colour is col / count, rounded once.
 *   placed[cluster] int32 says what happened: 0 the mean by request, 1 solved, 2 solved and clamped, 3 no non-degenerate face
 *   (tr not > 0): the mean.  A cluster without a member (garbage CSR) gets the centre, colour 0 and its placement code.
 *   The regulariser makes the position a continuous function of the input: it pulls towards the cell mean along the
 *   directions the planes leave free, which Lindstrom's truncated SVD does discontinuously.  1e-3 is his truncation ratio
 *   reused as a weight: a value NOBODY HAS TUNED here.
 *
 * FACES.  Every corner of a face goes through cluster[].  The face is INVALID when it is skipped, when a cluster id lies
 *   outside [0, Vc) or when two corners coincide; otherwise it is rotated so that its smallest index comes first (the
 *   orientation is kept) into (a, b, c) and gets the sortable key (a * Vc + b, c), two int64.  An invalid face is written as
 *   (-1, -1, -1) with the key (-1, -1).  The caller sorts the faces by (key_hi, key_lo), stably, so that equal keys stand in
 *   ascending face index; order [F] int64 is that permutation.  Of the valid faces with equal rotated triples the one with
 *   the SMALLEST face index is kept (fkeep = 1).  Two faces on the same three clusters with opposite orientation have
 *   different rotated triples: both stay.  ckeep[cluster] = 1 iff a kept face names it.  Kept faces keep their relative
 *   order and are written in rotated form, kept clusters keep ascending key order and indices are rewritten: that is
 *   egs_meshops_compact on (positions, colours, rotated faces, ckeep, fkeep) behind the caller's scans.
 *
 * TOPOLOGY.  Vertex clustering does not keep a closed manifold closed: the result of a sphere has a few opposite face pairs
 *   and an Euler characteristic other than 2.  A property of the method (Open3D's too), not repaired here.
 *
 * GRID.  Every entry point takes max_blocks: 0 for the default grid (at most EGS_SIMPLIFY_MAX_BLOCKS workgroups of 256
 *   threads, which walk their items with the stride of the grid), otherwise a cap on the number of workgroups.  No float
 *   atomic anywhere: every output is a pure function of the input, the same bits on every grid and stream.
 *
 * A library of its own beside libegs_meshops.so and the others, whose surfaces and ABI numbers it leaves alone.  Raw device
 * pointers on the CURRENT device (float32 and int32 4-B, int64 and double 8-B aligned) and a HIP stream (hipStream_t as
 * void*); no device synchronisation, no allocation, no readback, no environment variable; every argument is validated BEFORE
 * any HIP call, and a refused call writes nothing.  Empty inputs are accepted everywhere and launch nothing.  No output
 * aliases another buffer of the call.  Return 0 on success, otherwise EGS_SIMPLIFY_ERR_BAD_ARG or a hipError_t, and the
 * last-error string of THIS library describes it.
 */
#ifndef EGS_SIMPLIFY_H_
#define EGS_SIMPLIFY_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EGS_SIMPLIFY_ABI_VERSION 1
#define EGS_SIMPLIFY_ERR_BAD_ARG 10001
/* the most workgroups a kernel is launched with (max_blocks == 0) */
#define EGS_SIMPLIFY_MAX_BLOCKS 8192
/* bits per axis of a cell key */
#define EGS_SIMPLIFY_KEY_BITS 21
#define EGS_SIMPLIFY_PLACE_QUADRIC 0
#define EGS_SIMPLIFY_PLACE_MEAN 1

int egs_simplify_abi_version(void);
const char* egs_simplify_last_error_string(void);

/* keys [V] int64, every entry written.  origin finite, cell finite and > 0. */
int egs_simplify_keys(int V, const float* vertices, double ox, double oy, double oz, double cell, int64_t* keys,
                      int max_blocks, void* stream);

/* quadrics [V][9] double (a00 a01 a02 a11 a12 a22 g0 g1 g2), every entry written: the vertex-parallel pass of the two-pass
 * form.  F == 0: faces, row_start and rows may be NULL, every quadric is 0. */
int egs_simplify_vertex_quadrics(int V, int F, const float* vertices, const int64_t* faces, const int64_t* row_start,
                                 const int64_t* rows, const int64_t* keys, double ox, double oy, double oz, double cell,
                                 double* quadrics, int max_blocks, void* stream);

/* out_vertices [Vc][3], out_colors [Vc][3] (iff colors) float32, placed [Vc] int32, every entry written.  keys [V] as
 * egs_simplify_keys wrote them.  placement QUADRIC reads the per-vertex quadrics when `quadrics` is given (two-pass form);
 * with quadrics == NULL it forms each member's quadric itself, in the same order and to the same bits (fused form), and then
 * needs faces, row_start and rows unless F == 0.  placement MEAN reads none of the four. */
int egs_simplify_clusters(int V, int F, int Vc, const float* vertices, const float* colors, const int64_t* keys,
                          const int64_t* member_start, const int64_t* members, const double* quadrics,
                          const int64_t* faces, const int64_t* row_start, const int64_t* rows, double ox, double oy,
                          double oz, double cell, int placement, float* out_vertices, float* out_colors, int32_t* placed,
                          int max_blocks, void* stream);

/* rotated [F][3], key_hi [F], key_lo [F] int64, valid [F] int32, every entry written.  Vc >= 0. */
int egs_simplify_remap_faces(int V, int F, int Vc, const int64_t* faces, const int64_t* cluster, int64_t* rotated,
                             int32_t* valid, int64_t* key_hi, int64_t* key_lo, int max_blocks, void* stream);

/* fkeep [F], ckeep [Vc] int32, every entry written.  order [F]: the faces sorted by (key_hi, key_lo), equal keys in
 * ascending face index; rotated, valid, key_hi, key_lo as egs_simplify_remap_faces wrote them. */
int egs_simplify_keep_flags(int F, int Vc, const int64_t* order, const int64_t* rotated, const int32_t* valid,
                            const int64_t* key_hi, const int64_t* key_lo, int32_t* fkeep, int32_t* ckeep, int max_blocks,
                            void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EGS_SIMPLIFY_H_ */
