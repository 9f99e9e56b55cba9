/* C ABI of libegs_kmeans.so: Lloyd's k-means on the device -- the nearest-centroid assignment and the weighted centroid
 * update -- for AMD Instinct MI355X (gfx950).  It builds the codebook of the higher-order SH coefficients of a compressed
 * scene file (easygaussiansplatting_amd/compress.py).
 *
 * DATA.  Rows x [N][D] float32, contiguous; centroids c [K][D] float32, contiguous.  1 <= D <= EGS_KMEANS_MAX_D,
 *   1 <= K <= EGS_KMEANS_MAX_K, 0 <= N < 2^31.
 *
 * ASSIGN.  The label of a row is the index of the centroid nearest to it.  The score of row x against centroid k is
 *     s_k = ||c_k||^2 - 2 x . c_k            (the squared distance less ||x||^2, which does not depend on k),
 *   in float32 in this order: n_k = fma chain over d = 0 .. D-1 of c_kd * c_kd starting at +0 (the pre-kernel, which writes
 *   cnorm [K]); then acc = n_k and, for d = 0 .. D-1 ascending, acc = fma(x_d, -2 c_kd, acc) (the product by -2 is exact).
 *   The kernel forms this sum on the f32 matrix cores (v_mfma_f32_32x32x2_f32, which AMD documents as accumulating its
 *   products in ascending k with one rounding each, i.e. as that chain; NO TEST HERE PINS the score's bits -- scores are not
 *   an output, and the tests hold the labels to exactness on lattice inputs and to the derived gap bound otherwise, which
 *   any float32 order of this formula meets).  D is padded with zeros to 16, 32, 48 or 64, and fma(0, 0, acc) leaves acc
 *   as it is.
 *   The label is the LOWEST k whose score is the minimum: comparison is strict < in ascending k, starting from +infinity
 *   with label 0.  A NaN score never wins; if no score is below +infinity the label is 0.
 *   A row with a component that is not finite (NaN, +-Inf) gets LABEL 0, whatever its scores.  A label is always in [0, K).
 *   dist (nullable) [N] float32: the squared distance of the row to the centroid of its label, formed directly:
 *   acc = +0; for d ascending: t = x_d - c_d, acc = fma(t, t, acc).  (For a row that is not finite this is NaN or +Inf.)
 *
 * UPDATE.  The members of cluster k are the rows order[offsets[k] .. offsets[k+1]) -- order [N] int64 is the caller's STABLE
 *   sort of the labels (members in ascending row index), offsets [K+1] int64 the exclusive scan of the counts.  They are cut
 *   into chunks of EGS_KMEANS_CHUNK members.  A chunk's partial sums are, per column d, the double sum, starting at +0, in
 *   member order, of (double)w_i * (double)x_id (the product is exact), and the double sum of (double)w_i likewise.  The
 *   cluster's sums are the chunk sums added in chunk order, starting at +0.  New centroid kd = (float)(S_kd / W_k), one
 *   rounding to float32.  weights [N] float32 >= 0, nullable: NULL means 1 for every row (the same bits as weights of 1.0).
 *   wsum [K] double = W_k, count [K] int32 = the number of members; both always written.  A centroid without a member, or
 *   with W_k not > 0, KEEPS ITS BITS: centroids is read and written in place.
 *   No input VALUE is trusted to stay inside a buffer: an entry of order outside [0, N) is skipped, offsets are clamped to
 *   [0, N]; garbage in gives meaningless centroids, never an out-of-bounds access.
 *   Workspace: egs_kmeans_update_ws_bytes(N, D, K) bytes, 8-byte aligned, contents undefined before and after.
 *
 * GRID.  Every entry point takes max_blocks: 0 for the default grid (at most EGS_KMEANS_MAX_BLOCKS workgroups of 256
 *   threads, which walk their items with the stride of the grid), otherwise a cap on the number of workgroups.  No float
 *   atomic anywhere: every output is a pure function of the input, the same bits on every grid and stream.
 *
 * A library of its own beside libegs_hip.so and the other side libraries, whose surfaces and ABI numbers it leaves alone.
 * Raw device pointers on the CURRENT device (float32 and int32 4-B, int64 and double 8-B aligned) and a HIP stream
 * (hipStream_t as void*); no device synchronisation, no allocation, no readback, no environment variable; every argument is
 * validated BEFORE any HIP call, and a refused call writes nothing.  N == 0 is accepted everywhere, launches nothing and writes
 * nothing.  No output aliases another buffer of the call.  Return 0 on success, otherwise EGS_KMEANS_ERR_BAD_ARG or a hipError_t, and the last-error string of
 * THIS library describes it.
 */
#ifndef EGS_KMEANS_H_
#define EGS_KMEANS_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EGS_KMEANS_ABI_VERSION 1
#define EGS_KMEANS_ERR_BAD_ARG 10001
/* the most workgroups a kernel is launched with (max_blocks == 0) */
#define EGS_KMEANS_MAX_BLOCKS 8192
#define EGS_KMEANS_MAX_D 64
#define EGS_KMEANS_MAX_K 65536
/* assign: rows per workgroup, and centroids per LDS tile */
#define EGS_KMEANS_ROWS 256
#define EGS_KMEANS_TILE 64
/* update: members per chunk */
#define EGS_KMEANS_CHUNK 256

int egs_kmeans_abi_version(void);
const char* egs_kmeans_last_error_string(void);

/* labels [N] int32 and cnorm [K] float32 (the squared norms of the centroids, workspace and output), every entry written;
 * dist [N] float32 or NULL.  N == 0: success, nothing is launched and nothing written. */
int egs_kmeans_assign(int N, int D, int K, const float* x, const float* centroids, float* cnorm, int32_t* labels,
                      float* dist, int max_blocks, void* stream);

/* bytes of workspace egs_kmeans_update needs; 0 for arguments it would refuse */
size_t egs_kmeans_update_ws_bytes(int N, int D, int K);

/* centroids [K][D] in place, wsum [K] double and count [K] int32 every entry written.  N == 0: success, nothing is
 * launched and nothing written (every cluster is empty and keeps its bits; wsum and count are NOT written). */
int egs_kmeans_update(int N, int D, int K, const float* x, const float* weights, const int64_t* order,
                      const int64_t* offsets, float* centroids, double* wsum, int32_t* count, void* ws, size_t ws_bytes,
                      int max_blocks, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EGS_KMEANS_H_ */
