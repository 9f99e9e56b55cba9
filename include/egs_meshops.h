/* C ABI of libegs_meshops.so: cleaning of an indexed triangle mesh on the device -- connected components, removal of small
 * components with compaction, vertex normals and Taubin smoothing -- for AMD Instinct MI355X (gfx950).
 *
 * MESH.  vertices [V][3] float32, faces [F][3] int64 (what mesh.TSDFVolume.extract returns: there is no conversion pass),
 *   optional colors [V][3] and normals [V][3] float32.  V, F < 2^31.  Labels, counts, ranks and flags are int32.
 *   A face with an index outside [0, V) is SKIPPED by every kernel of this library: it joins nothing, is counted nowhere,
 *   is never kept and contributes to no normal and no smoothing step.  The VALUES of the other inputs (flags, scans, rows)
 *   are not trusted either: an entry that would lead outside a buffer is skipped; garbage in gives a meaningless result,
 *   never an out-of-bounds access.
 *
 * COMPONENTS.  Two vertices are connected when a face holds both: VERTEX connectivity (Open3D's
 *   cluster_connected_triangles joins triangles over shared EDGES; the two differ only at non-manifold pinch points, where
 *   this library joins and Open3D separates).
 *     label[v]      : the smallest vertex index of v's component;
 *     comp_faces[r] : for a representative r (label[r] == r) the number of faces of its component, 0 at every other index;
 *     comp_verts[r] : likewise the number of vertices.
 *   A face belongs to the component of its first vertex.  A vertex no face names is a component of one vertex and 0 faces.
 *   The labels come from a lock-free union-find (parent[v] <= v throughout, so the root of a component is its minimum
 *   index whatever order the hardware ran the threads in) and the counts are integer sums: all three outputs are pure
 *   functions of the input, bit for bit, from run to run and from grid to grid.
 *
 * KEEPING.  A component is kept when it has at least max(min_faces, 1) faces and -- with keep_largest > 0 -- rank[r] <
 *   keep_largest, rank[r] being the position of representative r in the order "more faces first, ties to the smaller
 *   label" (the caller's stable descending sort of comp_faces).  vkeep[v] = 1 iff v's component is kept, else 0; fkeep[f]
 *   = 1 iff the face is not skipped and its first vertex is kept, else 0.  Components without a face are always dropped:
 *   that removes unreferenced vertices.
 *
 * COMPACTION.  vscan [V] and fscan [F] int64 are the INCLUSIVE scans of vkeep and fkeep, formed by the caller, Vk and Fk
 *   their last entries.  A kept vertex v moves to row vscan[v] - 1, a kept face f to row fscan[f] - 1 with every index i
 *   rewritten to vscan[i] - 1: kept vertices and faces keep their relative order; coordinates, colours and normals travel
 *   with their vertices bit for bit; degenerate faces are left as they are.
 *
 * INCIDENCE.  Normals and smoothing read a vertex-to-face incidence in CSR form the caller builds: rows [3F] int64 holds
 *   the entries e = 3 f + k (corner k of face f) grouped by the vertex faces[f][k], in ASCENDING e within a vertex (a
 *   stable sort of the flattened faces gives it); row_start [V + 1] int64 the start of each vertex's group.  Both
 *   kernels are gathers with one thread per vertex that sum in the order of the row: no float atomic, bitwise
 *   reproducible.  A hub of high valence is walked by one thread.
 *
 * NORMALS.  S(v) = sum over v's row of (b - a) x (c - a) of the incident face (a, b, c): area weighted, and the outward
 *   orientation of the TSDF extraction.  Differences, products and the sum in double, every operation rounded on its own
 *   (no fused multiply-add); n = S / |S| with |S| = sqrt((Sx Sx + Sy Sy) + Sz Sz), each component rounded ONCE to
 *   float32.  (0, 0, 0) when |S| is 0 or not finite, or when the vertex has no face.
 *
 * TAUBIN SMOOTHING.  An iteration is a lambda step and a mu step of p' = p + s (m - p), s = lam then s = mu.  m is the
 *   FACE UMBRELLA: with (q, r) the other two vertices of an entry's face (corners k + 1 and k + 2 mod 3), A = sum over
 *   the row of (q + r) and deg the row's number of entries, m = A / (2 deg).  On a closed manifold this is the uniform
 *   umbrella; at a boundary, interior neighbours weigh double.  All in double in row order, no fused multiply-add, ONE
 *   rounding to float32 per step and component.  A vertex of degree 0 keeps its bits.  The steps ping-pong between `out`
 *   and `tmp`; the input is not modified; the result is in `out`.  lam = 0.5 and mu = -0.53 (Taubin's pair, Open3D's
 *   defaults) and 10 iterations are what the Python layer passes by default: values NOBODY HAS TUNED here.
 *
 * GRID.  Every entry point takes max_blocks: 0 for the default grid (at most EGS_MESHOPS_MAX_BLOCKS workgroups of 256
 *   threads, which walk their items with the stride of the grid), otherwise a cap on the number of workgroups.
 *
 * A library of its own beside libegs_hip.so and the other side libraries, whose surfaces and ABI numbers it leaves alone.
 * Raw device pointers on the CURRENT device (float32 and int32 4-B, int64 8-B aligned) and a HIP stream (hipStream_t as
 * void*); no device synchronisation, no allocation, no readback, no environment variable; every argument is validated
 * BEFORE any HIP call, and a refused call writes nothing.  V == 0 or F == 0 is accepted everywhere; what then has nothing
 * to do launches nothing.  No output aliases another buffer of the call.  Return 0 on success, otherwise
 * EGS_MESHOPS_ERR_BAD_ARG or a hipError_t, and the last-error string of THIS library describes it.
 */
#ifndef EGS_MESHOPS_H_
#define EGS_MESHOPS_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EGS_MESHOPS_ABI_VERSION 1
#define EGS_MESHOPS_ERR_BAD_ARG 10001
/* the most workgroups a kernel is launched with (max_blocks == 0) */
#define EGS_MESHOPS_MAX_BLOCKS 8192

int egs_meshops_abi_version(void);
const char* egs_meshops_last_error_string(void);

/* label, comp_faces, comp_verts [V] int32, every entry written.  V == 0: no launch.  F == 0: every vertex its own
 * component.  faces may be NULL iff F == 0. */
int egs_meshops_components(int V, int F, const int64_t* faces, int32_t* label, int32_t* comp_faces, int32_t* comp_verts,
                           int max_blocks, void* stream);

/* vkeep [V], fkeep [F] int32, every entry written.  keep_largest >= 0: 0 means no such rule, and rank is then not read
 * (it may be NULL); otherwise rank [V] int32 is needed.  min_faces >= 0 (0 and 1 mean the same: a component needs a
 * face). */
int egs_meshops_keep_flags(int V, int F, const int64_t* faces, const int32_t* label, const int32_t* comp_faces,
                           const int32_t* rank, int min_faces, int keep_largest, int32_t* vkeep, int32_t* fkeep,
                           int max_blocks, void* stream);

/* out_vertices [Vk][3], out_colors [Vk][3] (iff colors), out_normals [Vk][3] (iff normals), out_faces [Fk][3] int64.
 * 0 <= Vk <= V, 0 <= Fk <= F.  Outputs of size 0 may be NULL. */
int egs_meshops_compact(int V, int F, const float* vertices, const float* colors, const float* normals,
                        const int64_t* faces, const int32_t* vkeep, const int32_t* fkeep, const int64_t* vscan,
                        const int64_t* fscan, int Vk, int Fk, float* out_vertices, float* out_colors, float* out_normals,
                        int64_t* out_faces, int max_blocks, void* stream);

/* normals [V][3] float32, every entry written.  F == 0: faces and rows may be NULL, every normal is 0. */
int egs_meshops_vertex_normals(int V, int F, const float* vertices, const int64_t* faces, const int64_t* row_start,
                               const int64_t* rows, float* normals, int max_blocks, void* stream);

/* out, tmp [V][3] float32.  iterations >= 0 (0: out is a copy of vertices); lam, mu finite.  tmp may be NULL iff
 * iterations == 0. */
int egs_meshops_taubin(int V, int F, const float* vertices, const int64_t* faces, const int64_t* row_start,
                       const int64_t* rows, int iterations, double lam, double mu, float* out, float* tmp,
                       int max_blocks, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EGS_MESHOPS_H_ */
