// libegs_kmeans.so (include/egs_kmeans.h, which states every rule): Lloyd's k-means for the SH codebook of a compressed
// scene file.
//
//   k_norms          : a thread per centroid: n_k = ||c_k||^2, an fma chain in ascending d
//   k_assign<DP>     : a workgroup of 4 waves per KM_ROWS = 256 rows, walked with the stride of the grid.  A wave keeps 2 x 32
//                      rows in registers as the B operands of v_mfma_f32_32x32x2_f32 (lane l: row l & 31, column 2 s + (l >> 5)
//                      of k-step s); the centroids go by in LDS tiles of KM_TILE = 64, staged as A operands already multiplied
//                      by -2 (exact) and double-buffered: the next tile's global loads are in flight while this one is
//                      multiplied.  The accumulator of a 32 x 32 block starts at the centroids' norms, so after DP / 2 MFMAs a
//                      lane holds 16 finished scores of ONE row, in ascending centroid index: the argmin is 16 compares per
//                      lane and 32 x 32 x DP multiply-adds, off the matrix pipe.  The two lane halves (which hold different
//                      centroids of the same row) are merged once, at the end, by (score, index).
//                      The f32 MFMA is documented as the fmaf chain in ascending d (not pinned by a test: the scores are
//                      no output) and runs at the VALU's rate; what it buys is operand
//                      traffic: one ds_read_b32 feeds 2 MFMAs = 128 cycles of the pipe, where the VALU form needs a wave-
//                      uniform centroid value per fma.
//   k_update_partial : a wave per chunk slot (KM_CHUNK members of one cluster), lane = column: double sums in member order
//   k_update_final   : a thread per (cluster, column): chunk sums added in chunk order, one division, one rounding
//
// No atomic, no cross-workgroup hand-off: every output is a pure function of the input.
#define EGS_SIDE_LIBRARY "egs_kmeans"
#include "egs_side_error.h"

#include <float.h>
#include <math.h>

#include <initializer_list>

#include "../../include/egs_kmeans.h"

static_assert(EGS_KMEANS_ERR_BAD_ARG == EGS_ERR_BAD_ARG, "one bad-argument code across the libraries");

#pragma clang fp contract(off)

namespace egs {

constexpr int KM_THREADS = 256;
constexpr int KM_WAVES = KM_THREADS / 64;
constexpr int KM_GROUPS = 2;                           // 32-row groups per wave
constexpr int KM_ROWS = EGS_KMEANS_ROWS;
constexpr int KM_TILE = EGS_KMEANS_TILE;
constexpr int KM_TBLOCKS = KM_TILE / 32;               // 32-centroid blocks per tile
constexpr int KM_CHUNK = EGS_KMEANS_CHUNK;
static_assert(KM_ROWS == KM_WAVES * KM_GROUPS * 32, "rows per workgroup");
static_assert(KM_TILE % 32 == 0 && KM_TILE <= KM_THREADS, "centroid tile");

typedef float f32x16 __attribute__((ext_vector_type(16)));

__global__ __launch_bounds__(KM_THREADS) void k_norms(int D, int K, const float* __restrict__ c, float* __restrict__ cnorm) {
  for (int64_t k = (int64_t)blockIdx.x * KM_THREADS + threadIdx.x; k < K; k += (int64_t)gridDim.x * KM_THREADS) {
    float acc = 0.f;
    for (int d = 0; d < D; ++d) {
      const float v = c[k * D + d];
      acc = fmaf(v, v, acc);
    }
    cnorm[k] = acc;
  }
}

template <int DP>
__global__ __launch_bounds__(KM_THREADS, 2) void k_assign(int N, int D, int K, const float* __restrict__ x,
                                                      const float* __restrict__ c, const float* __restrict__ cnorm,
                                                      int32_t* __restrict__ labels, float* __restrict__ dist) {
  constexpr int S = DP / 2;                            // k-steps (MFMAs) per 32 x 32 block
  constexpr int TILE_F = KM_TILE * DP;                 // floats of a staged tile: [block][k-step][lane]
  constexpr int PER_T = TILE_F / KM_THREADS;           // staged floats per thread
  static_assert(TILE_F % KM_THREADS == 0, "whole staging passes");
  __shared__ float sA[2][TILE_F];
  __shared__ __attribute__((aligned(16))) float sN[2][KM_TILE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int ntiles = (K + KM_TILE - 1) / KM_TILE;
  const int64_t nblk = ((int64_t)N + KM_ROWS - 1) / KM_ROWS;

  float stage[PER_T];
  float stage_n = 0.f;
  // tile t from global memory into registers: element (p = tid / 64 + 4 j, lane) of the image, p = block * S + k-step
  auto load_tile = [&](int t) {
    const int t0 = t * KM_TILE;
#pragma unroll
    for (int j = 0; j < PER_T; ++j) {
      const int p = wave + KM_WAVES * j;
      const int k = t0 + 32 * (p / S) + r, d = 2 * (p % S) + h;
      stage[j] = (k < K && d < D) ? -2.f * c[(int64_t)k * D + d] : 0.f;
    }
    if (tid < KM_TILE) stage_n = t0 + tid < K ? cnorm[t0 + tid] : INFINITY;
  };
  auto store_tile = [&](int buf) {
#pragma unroll
    for (int j = 0; j < PER_T; ++j) sA[buf][(wave + KM_WAVES * j) * 64 + lane] = stage[j];
    if (tid < KM_TILE) sN[buf][tid] = stage_n;
  };

  for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int64_t row0 = blk * KM_ROWS + wave * (KM_GROUPS * 32);
    float xb[KM_GROUPS][S];
    bool bad[KM_GROUPS];
    float best[KM_GROUPS];
    int bk[KM_GROUPS];
#pragma unroll
    for (int g = 0; g < KM_GROUPS; ++g) {
      const int64_t row = row0 + g * 32 + r;
      bad[g] = false;
      best[g] = INFINITY;
      bk[g] = 0;
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const int d = 2 * s + h;
        const float v = (row < N && d < D) ? x[row * D + d] : 0.f;
        bad[g] = bad[g] || !(fabsf(v) <= FLT_MAX);
        xb[g][s] = v;
      }
    }
    load_tile(0);
    store_tile(0);
    __syncthreads();
    for (int t = 0; t < ntiles; ++t) {
      const int buf = t & 1;
      if (t + 1 < ntiles) load_tile(t + 1);
#pragma unroll
      for (int b = 0; b < KM_TBLOCKS; ++b) {
        f32x16 acc[KM_GROUPS];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float4 n4 = *reinterpret_cast<const float4*>(&sN[buf][32 * b + 8 * q + 4 * h]);
#pragma unroll
          for (int g = 0; g < KM_GROUPS; ++g) {
            acc[g][4 * q] = n4.x; acc[g][4 * q + 1] = n4.y; acc[g][4 * q + 2] = n4.z; acc[g][4 * q + 3] = n4.w;
          }
        }
#pragma unroll
        for (int s = 0; s < S; ++s) {
          const float a = sA[buf][(b * S + s) * 64 + lane];
#pragma unroll
          for (int g = 0; g < KM_GROUPS; ++g) acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, xb[g][s], acc[g], 0, 0, 0);
        }
        const int k0 = t * KM_TILE + 32 * b + 4 * h;
#pragma unroll
        for (int g = 0; g < KM_GROUPS; ++g) {
#pragma unroll
          for (int v = 0; v < 16; ++v) {
            const float sc = acc[g][v];
            if (sc < best[g]) { best[g] = sc; bk[g] = k0 + 8 * (v >> 2) + (v & 3); }
          }
        }
      }
      if (t + 1 < ntiles) store_tile(buf ^ 1);
      __syncthreads();
    }
#pragma unroll
    for (int g = 0; g < KM_GROUPS; ++g) {
      const float ob = __shfl_xor(best[g], 32);
      const int ok = __shfl_xor(bk[g], 32);
      const int obad = __shfl_xor((int)bad[g], 32);
      int lab = (ob < best[g] || (ob == best[g] && ok < bk[g])) ? ok : bk[g];
      if (bad[g] || obad != 0) lab = 0;
      const int64_t row = row0 + g * 32 + r;
      if (h == 0 && row < N) {
        labels[row] = lab;
        if (dist != nullptr) {
          float acc = 0.f;
          for (int d = 0; d < D; ++d) {
            const float tt = x[row * D + d] - c[(int64_t)lab * D + d];
            acc = fmaf(tt, tt, acc);
          }
          dist[row] = acc;
        }
      }
    }
  }
}

__device__ __forceinline__ int64_t clamp_off(const int64_t* __restrict__ offsets, int k, int N) {
  const int64_t o = offsets[k];
  return o < 0 ? 0 : (o > N ? N : o);
}
// the first chunk slot of cluster k: strictly increasing in k, and cluster k's chunks end before slot_base(k + 1)
__device__ __forceinline__ int64_t slot_base(const int64_t* __restrict__ offsets, int k, int N) {
  return clamp_off(offsets, k, N) / KM_CHUNK + k;
}

__global__ __launch_bounds__(KM_THREADS) void k_update_partial(int N, int D, int K, const float* __restrict__ x,
                                                              const float* __restrict__ weights,
                                                              const int64_t* __restrict__ order,
                                                              const int64_t* __restrict__ offsets,
                                                              double* __restrict__ partial) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t nslots = (int64_t)N / KM_CHUNK + K;
  for (int64_t slot = (int64_t)blockIdx.x * KM_WAVES + wave; slot < nslots; slot += (int64_t)gridDim.x * KM_WAVES) {
    int lo = 0, hi = K - 1;                            // the last cluster whose first slot is <= slot
    while (lo < hi) {
      const int mid = (int)(((int64_t)lo + hi + 1) >> 1);
      if (slot_base(offsets, mid, N) <= slot) lo = mid; else hi = mid - 1;
    }
    const int64_t m0 = clamp_off(offsets, lo, N), m1 = clamp_off(offsets, lo + 1, N);
    const int64_t j = slot - slot_base(offsets, lo, N);
    if (j < 0) continue;
    const int64_t b = m0 + j * KM_CHUNK;
    if (b >= m1) continue;
    const int64_t e = b + KM_CHUNK < m1 ? b + KM_CHUNK : m1;
    double s = 0.0, w = 0.0;
    for (int64_t i = b; i < e; ++i) {
      const int64_t row = order[i];
      if (row < 0 || row >= N) continue;
      const double wi = weights != nullptr ? (double)weights[row] : 1.0;
      w += wi;
      if (lane < D) s += wi * (double)x[row * D + lane];
    }
    if (lane < D) partial[slot * (D + 1) + lane] = s;
    if (lane == 0) partial[slot * (D + 1) + D] = w;
  }
}

__global__ __launch_bounds__(KM_THREADS) void k_update_final(int N, int D, int K, const int64_t* __restrict__ offsets,
                                                            const double* __restrict__ partial,
                                                            float* __restrict__ centroids, double* __restrict__ wsum,
                                                            int32_t* __restrict__ count) {
  const int64_t nslots = (int64_t)N / KM_CHUNK + K, items = (int64_t)K * D;
  for (int64_t e = (int64_t)blockIdx.x * KM_THREADS + threadIdx.x; e < items; e += (int64_t)gridDim.x * KM_THREADS) {
    const int k = (int)(e / D), d = (int)(e % D);
    const int64_t m0 = clamp_off(offsets, k, N), m1 = clamp_off(offsets, k + 1, N);
    const int64_t cnt = m1 > m0 ? m1 - m0 : 0;
    const int64_t nch = (cnt + KM_CHUNK - 1) / KM_CHUNK, base = slot_base(offsets, k, N);
    double s = 0.0, w = 0.0;
    for (int64_t j = 0; j < nch; ++j) {
      const int64_t slot = base + j;
      if (slot >= nslots) break;
      s += partial[slot * (D + 1) + d];
      w += partial[slot * (D + 1) + D];
    }
    if (d == 0) {
      wsum[k] = w;
      count[k] = (int32_t)cnt;
    }
    if (cnt > 0 && w > 0.0) centroids[e] = (float)(s / w);
  }
}

}  // namespace egs

using namespace egs;

static bool aligned_to(const void* a, uintptr_t k) { return ((uintptr_t)a & (k - 1)) == 0; }
static bool blocks_ok(int max_blocks) { return max_blocks >= 0 && max_blocks <= EGS_KMEANS_MAX_BLOCKS; }
static bool shape_ok(int N, int D, int K) {
  return N >= 0 && D >= 1 && D <= EGS_KMEANS_MAX_D && K >= 1 && K <= EGS_KMEANS_MAX_K;
}
static int grid_for(int64_t want, int max_blocks) {
  const int64_t cap = max_blocks > 0 ? max_blocks : EGS_KMEANS_MAX_BLOCKS;
  return (int)(want < 1 ? 1 : (want < cap ? want : cap));
}
// no two of the non-null pointers are equal
static bool distinct(std::initializer_list<const void*> ps) {
  for (auto a = ps.begin(); a != ps.end(); ++a)
    for (auto b = a + 1; b != ps.end(); ++b)
      if (*a != nullptr && *a == *b) return false;
  return true;
}

extern "C" int egs_kmeans_abi_version(void) { return EGS_KMEANS_ABI_VERSION; }
extern "C" const char* egs_kmeans_last_error_string(void) { return egs_side::g_err; }

extern "C" int egs_kmeans_assign(int N, int D, int K, const float* x, const float* centroids, float* cnorm, int32_t* labels,
                                 float* dist, int max_blocks, void* stream) {
  SIDE_CHECK_ARG(shape_ok(N, D, K));
  SIDE_CHECK_ARG(blocks_ok(max_blocks));
  SIDE_CHECK_ARG(aligned_to(x, 4) && aligned_to(centroids, 4) && aligned_to(cnorm, 4) && aligned_to(labels, 4) &&
                 aligned_to(dist, 4));
  SIDE_CHECK_ARG(centroids != nullptr && cnorm != nullptr);
  SIDE_CHECK_ARG(N == 0 || (x != nullptr && labels != nullptr));
  SIDE_CHECK_ARG(distinct({x, centroids, cnorm, labels, dist}));
  if (N == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_norms, dim3(grid_for(((int64_t)K + KM_THREADS - 1) / KM_THREADS, max_blocks)), dim3(KM_THREADS), 0, s,
                     D, K, centroids, cnorm);
  const dim3 grid(grid_for(((int64_t)N + KM_ROWS - 1) / KM_ROWS, max_blocks));
  if (D <= 16)
    hipLaunchKernelGGL(k_assign<16>, grid, dim3(KM_THREADS), 0, s, N, D, K, x, centroids, cnorm, labels, dist);
  else if (D <= 32)
    hipLaunchKernelGGL(k_assign<32>, grid, dim3(KM_THREADS), 0, s, N, D, K, x, centroids, cnorm, labels, dist);
  else if (D <= 48)
    hipLaunchKernelGGL(k_assign<48>, grid, dim3(KM_THREADS), 0, s, N, D, K, x, centroids, cnorm, labels, dist);
  else
    hipLaunchKernelGGL(k_assign<64>, grid, dim3(KM_THREADS), 0, s, N, D, K, x, centroids, cnorm, labels, dist);
  SIDE_HIP(hipGetLastError());
  return 0;
}

extern "C" size_t egs_kmeans_update_ws_bytes(int N, int D, int K) {
  if (!shape_ok(N, D, K)) return 0;
  return (size_t)((int64_t)N / KM_CHUNK + K) * (size_t)(D + 1) * sizeof(double);
}

extern "C" int egs_kmeans_update(int N, int D, int K, const float* x, const float* weights, const int64_t* order,
                                 const int64_t* offsets, float* centroids, double* wsum, int32_t* count, void* ws,
                                 size_t ws_bytes, int max_blocks, void* stream) {
  SIDE_CHECK_ARG(shape_ok(N, D, K));
  SIDE_CHECK_ARG(blocks_ok(max_blocks));
  SIDE_CHECK_ARG(aligned_to(x, 4) && aligned_to(weights, 4) && aligned_to(order, 8) && aligned_to(offsets, 8) &&
                 aligned_to(centroids, 4) && aligned_to(wsum, 8) && aligned_to(count, 4) && aligned_to(ws, 8));
  SIDE_CHECK_ARG(offsets != nullptr && centroids != nullptr && wsum != nullptr && count != nullptr);
  SIDE_CHECK_ARG(N == 0 || (x != nullptr && order != nullptr));
  SIDE_CHECK_ARG(N == 0 || (ws != nullptr && ws_bytes >= egs_kmeans_update_ws_bytes(N, D, K)));
  SIDE_CHECK_ARG(distinct({x, weights, order, offsets, centroids, wsum, count, ws}));
  if (N == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const int64_t nslots = (int64_t)N / KM_CHUNK + K;
  hipLaunchKernelGGL(k_update_partial, dim3(grid_for((nslots + KM_WAVES - 1) / KM_WAVES, max_blocks)), dim3(KM_THREADS), 0, s,
                     N, D, K, x, weights, order, offsets, (double*)ws);
  hipLaunchKernelGGL(k_update_final, dim3(grid_for(((int64_t)K * D + KM_THREADS - 1) / KM_THREADS, max_blocks)),
                     dim3(KM_THREADS), 0, s, N, D, K, offsets, (const double*)ws, centroids, wsum, count);
  SIDE_HIP(hipGetLastError());
  return 0;
}
