// Row traffic of the lane-per-Gaussian kernels (egs_preprocess.hip): a workgroup's 256 rows of K floats between
// registers and global memory, through LDS.
//
// Why through LDS.  A lane that loads or stores its own K-float row issues K dword (or K/4 dwordx4) instructions
// whose 64 lanes are 4K bytes apart: every instruction touches 64 different cache lines and moves 4 or 16 bytes of
// each -- the AoS pattern that kept the seven-op kernels at 3.0-3.7 TB/s.  The workgroup's 256 rows are ONE contiguous,
// 16-B aligned span of the tensor (256 * K * 4 bytes), so the span moves as coalesced dwordx4, full lines, and every
// lane meets its row in LDS: rows_in (high_shs of the RAW fused kernels, whose 36- and 180-B rows cannot be
// dwordx4-loaded per lane at all) and rows_out (values and Jacobians of the seven ops, K = 3 ... 24, 832 B per Gaussian
// with calc_J; dL/dsh of k_chain_rule; draw records, dcolor/dpw, dL/dsh and dL/dhigh_shs of the fused kernels).
// Measured with the rows leaving as full lines: k_cov3d 70 -> 38-46 us, k_cov2d 46 -> 29 us at 1 M Gaussians; the RAW
// 45-float rows 100 us forward / 101 us backward as one dwordx4 span against 187 / 240 us staged dword by dword
// (docs/LAB.md).
//
// Why these strides.  Lane t owns lds[t * STRIDE .. t * STRIDE + K).  An odd STRIDE makes the lanes' dword accesses
// conflict-free, an odd number of 16-B units their b128 accesses (RowStage below).  For an odd K the row needs no
// padding: the span lies in LDS exactly as in memory and moves as float4 on both sides.
//
// Why every row is written.  rows_out writes all rows of the workgroup below n, culled Gaussians as the zeros their
// lanes hold: the callers allocate with torch.empty, not torch.zeros (the reference's zero-filled outputs,
// gausplat.cu:170-178 etc., cost 528 B per Gaussian and step of pure fill here).
#pragma once
#include "egs_common.h"

namespace egs {

enum class RowKind {
  DIRECT,   // K <= 2 (out only): one dword / dwordx2 store per lane, no LDS
  QUAD,     // K % 4 == 0: float4 pieces on both sides, row stride an odd number of 16-B units
  CONTIG,   // odd K: the span unpadded, STRIDE == K
  PADDED,   // K % 4 == 2 (out only; K = 6, 18): stride K + 1, the span's float4 pieces are gathered dword by dword
};

template <int K>
struct RowStage {
  static constexpr RowKind KIND = K <= 2 ? RowKind::DIRECT : K % 4 == 0 ? RowKind::QUAD
                                  : K % 2 == 1 ? RowKind::CONTIG : RowKind::PADDED;
  static constexpr int Q = K / 4;                                                     // float4 per row (QUAD)
  static constexpr int STRIDE = KIND == RowKind::QUAD ? 4 * ((Q + 1) | 1) : (K | 1);   // floats
  static_assert(KIND == RowKind::QUAD ? (STRIDE / 4) % 2 == 1 : STRIDE % 2 == 1, "conflict-free LDS rows: odd stride");
  static constexpr int LDS_FLOATS = 256 * STRIDE;
  static constexpr int OUT_LDS_FLOATS = KIND == RowKind::DIRECT ? 1 : LDS_FLOATS;     // a kernel that only calls rows_out
  // the float4 pieces of a span of `rows` rows: pieces(rows) whole ones (a tail of <= 3 floats unless QUAD), has_piece(f)
  // for f below that (QUAD: in terms of the row, which the piece's LDS address needs anyway)
  static __device__ __forceinline__ int pieces(int rows) { return KIND == RowKind::QUAD ? rows * Q : (rows * K) >> 2; }
  static __device__ __forceinline__ bool has_piece(int f, int rows) {
    return KIND == RowKind::QUAD ? f / Q < rows : f < pieces(rows);
  }
  // piece f, out of the rows deposited in LDS
  static __device__ __forceinline__ float4 piece(const float* lds, int f) {
    if constexpr (KIND == RowKind::QUAD) {
      const int r = f / Q, c = f - r * Q;
      return *reinterpret_cast<const float4*>(lds + r * STRIDE + 4 * c);
    } else if constexpr (KIND == RowKind::CONTIG) {
      return reinterpret_cast<const float4*>(lds)[f];
    } else {
      int r = (4 * f) / K, c = 4 * f - r * K;
      float v[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        v[t] = lds[r * STRIDE + c];
        if (++c == K) { c = 0; ++r; }
      }
      return make_float4(v[0], v[1], v[2], v[3]);
    }
  }
};
constexpr int cmax(int a, int b) { return a > b ? a : b; }

// row[0..K) of lane t = src row base + t.  All 256 threads of the workgroup call this (a barrier inside); `row` of
// lanes past n is undefined.  The caller's next rows_out on the same `lds` brings its own leading barrier.
template <int K>
__device__ __forceinline__ void rows_in(const float* __restrict__ src, int n, int base, float* lds, float* row) {
  using RS = RowStage<K>;
  static_assert(RS::KIND == RowKind::QUAD || RS::KIND == RowKind::CONTIG, "no caller stages such rows in");
  const int rows = min(256, n - base);
  const int tid = threadIdx.x;
  const float4* __restrict__ s4 = reinterpret_cast<const float4*>(src + (size_t)K * base);
  if constexpr (RS::KIND == RowKind::QUAD) {
#pragma unroll
    for (int j = 0; j < RS::Q; ++j) {
      const int f = tid + 256 * j;
      const int r = f / RS::Q, c = f - r * RS::Q;
      if (r < rows) *reinterpret_cast<float4*>(lds + r * RS::STRIDE + 4 * c) = s4[f];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < RS::Q; ++j) {
      const float4 v = *reinterpret_cast<const float4*>(lds + tid * RS::STRIDE + 4 * j);
      row[4 * j] = v.x; row[4 * j + 1] = v.y; row[4 * j + 2] = v.z; row[4 * j + 3] = v.w;
    }
  } else {
    const int total = rows * K, nq = total >> 2;
    for (int f = tid; f < nq; f += 256) reinterpret_cast<float4*>(lds)[f] = s4[f];
    for (int f = 4 * nq + tid; f < total; f += 256) lds[f] = src[(size_t)K * base + f];   // <= 3 tail floats
    __syncthreads();
#pragma unroll
    for (int j = 0; j < K; ++j) row[j] = lds[tid * K + j];
  }
}

// dst row base + t = row[0..K) of lane t (accum: += -- a read-modify-write of the same coalesced span; without it the
// values leave with their bits, no arithmetic touches them: -0.0 stays -0.0).  All 256 threads of the workgroup call
// this (barriers inside); `row` of lanes past n is ignored.
template <int K>
__device__ __forceinline__ void rows_out(const float* row, float* __restrict__ dst, int n, int base, float* lds,
                                         bool accum = false) {
  using RS = RowStage<K>;
  const int rows = min(256, n - base);
  const int tid = threadIdx.x;
  if constexpr (RS::KIND == RowKind::DIRECT) {
    if (tid < rows) {
      if constexpr (K == 2) reinterpret_cast<float2*>(dst)[base + tid] = make_float2(row[0], row[1]);
      else dst[base + tid] = row[0];
    }
  } else {
    __syncthreads();   // the previous user of `lds` is done with it
    if constexpr (RS::KIND == RowKind::QUAD) {
#pragma unroll
      for (int j = 0; j < RS::Q; ++j)
        *reinterpret_cast<float4*>(lds + tid * RS::STRIDE + 4 * j) =
            make_float4(row[4 * j], row[4 * j + 1], row[4 * j + 2], row[4 * j + 3]);
    } else {
#pragma unroll
      for (int j = 0; j < K; ++j) lds[tid * RS::STRIDE + j] = row[j];
    }
    __syncthreads();
    const int total = rows * K, nq = RS::pieces(rows);
    float4* __restrict__ d4 = reinterpret_cast<float4*>(dst + (size_t)K * base);
    constexpr int NI = (K + 3) / 4;            // pieces per thread: 256 K / 4 float4 over 256 threads
    // accum: the old values of all the thread's pieces are requested first (clamped addresses, no branches) -- read
    // at its use inside the loop below, each piece waited for its own load AND for the previous piece's store
    float4 o[NI];
    if (accum && (RS::KIND == RowKind::QUAD || nq > 0)) {   // (no whole piece: a lone row of three floats)
#pragma unroll
      for (int j = 0; j < NI; ++j) o[j] = d4[min(tid + 256 * j, nq - 1)];
    }
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const int f = tid + 256 * j;
      if (RS::has_piece(f, rows)) {
        float4 v = RS::piece(lds, f);
        if (accum) { v.x += o[j].x; v.y += o[j].y; v.z += o[j].z; v.w += o[j].w; }
        d4[f] = v;
      }
    }
    if constexpr (RS::KIND != RowKind::QUAD) {   // <= 3 floats, when the last workgroup's rows * K is no multiple of four
      const int f = 4 * nq + tid;
      if (f < total) {
        const int r = f / K, c = f - r * K;
        float v = lds[r * RS::STRIDE + c];
        if (accum) v += dst[(size_t)K * base + f];
        dst[(size_t)K * base + f] = v;
      }
    }
  }
}

// A lane's own row, for the rows that are not staged: the widest vector load the row's alignment allows (a dword load
// per float costs one L1 lookup per lane and float: 24 instructions x 64 lookups for a dcov3d/drot row, 6 x 64 as
// dwordx4).  The SH rows of the non-RAW kernels come this way: staging them through LDS measured 10 % slower in
// k_preprocess_fwd.
// (tried: streaming (non-temporal) loads of the SH rows -- k_preprocess_fwd 99 -> 172 us, k_sh2color 86 -> 132 us: the
// twelve loads of a lane re-touch its lines and live on the cache hits; docs/LAB.md)
template <int K>
__device__ __forceinline__ void load_row(const float* __restrict__ row, float* out) {
  if constexpr (K % 4 == 0) {
#pragma unroll
    for (int j = 0; j < K / 4; ++j) {
      const float4 v = reinterpret_cast<const float4*>(row)[j];
      out[4 * j] = v.x; out[4 * j + 1] = v.y; out[4 * j + 2] = v.z; out[4 * j + 3] = v.w;
    }
  } else if constexpr (K % 2 == 0) {
#pragma unroll
    for (int j = 0; j < K / 2; ++j) {
      const float2 v = reinterpret_cast<const float2*>(row)[j];
      out[2 * j] = v.x; out[2 * j + 1] = v.y;
    }
  } else {
#pragma unroll
    for (int j = 0; j < K; ++j) out[j] = row[j];
  }
}

}  // namespace egs
