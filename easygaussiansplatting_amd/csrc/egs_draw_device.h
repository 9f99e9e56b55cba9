// Device code shared by egs_draw.hip (k_draw, k_draw_bwd), egs_segments.hip (k_draw_seg) and egs_list_walk.h
// (k_blend_weights, k_feature_render, k_feature_gather): the forward blend of a tile list -- the lane's tile geometry,
// the staging math of a list entry, the exponent at a pixel, the chunk loop of k_draw and k_draw_seg and their small
// epilogues -- and the wave reductions of the backward pass.
#pragma once
#include "egs_raster.h"

namespace egs {

// 4-bit reach mask of one list entry over the four 8x8 blocks of a tile (bit k = block
// (k&1, k>>1)).  Computed ONCE per entry by the lane that stages it (64 entries in
// parallel) instead of by all 64 lanes of the blend loop.
template <bool BOX>
__device__ __forceinline__ int reach_mask(const float4& A, const float4& C, int tx0, int ty0) {
  bool okx[2], oky[2];
  if (BOX) {  // overlap of the pixel box (gausplat.py:212-215) with the block
    const uint32_t bx = __float_as_uint(C.y), by = __float_as_uint(C.z);
    const int x0 = bx & 0xFFFF, x1 = bx >> 16, y0 = by & 0xFFFF, y1 = by >> 16;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      okx[b] = (x0 < tx0 + 8 * b + 8) && (x1 > tx0 + 8 * b);
      oky[b] = (y0 < ty0 + 8 * b + 8) && (y1 > ty0 + 8 * b);
    }
  } else {    // certain-miss box (ex, ey) of the pack kernel vs the block (half size 3.5 px)
    const float rx = C.y + 3.5f, ry = C.z + 3.5f;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      okx[b] = fabsf(A.x - ((float)tx0 + 3.5f + 8.f * b)) <= rx;
      oky[b] = fabsf(A.y - ((float)ty0 + 3.5f + 8.f * b)) <= ry;
    }
  }
  return (int)(okx[0] && oky[0]) | ((int)(okx[1] && oky[0]) << 1) | ((int)(okx[0] && oky[1]) << 2) |
         ((int)(okx[1] && oky[1]) << 3);
}

// CUDA's max(0.0f, NaN) == 0 (kernel.cu:243-246, 909-913): a Mahalanobis term that is NaN counts as 0 and the Gaussian
// blends at min(0.99, alpha).  A NaN in the conic or the centre of an entry makes EVERY pixel's term NaN, so the lane that
// stages the entry decides it once: conic := 0, centre := 0 -- the exponent is then log2(alpha) everywhere (forward) and
// the power 0 (backward).  Per entry, 64 entries in parallel, nothing in the blend loops.  (A NaN that arises at single
// pixels from inf * 0 is not covered: EgsPolicy.nan_maha.)
__device__ __forceinline__ bool nan_entry_fix(float4& A, float4& B) {
  if (A.x != A.x || A.y != A.y || A.z != A.z || A.w != A.w || B.x != B.x) {
    A = make_float4(0.f, 0.f, 0.f, 0.f);
    B.x = 0.f;
    return true;
  }
  return false;
}

// The longest walk of a render -> the host's hint word, without a launch of its own.  The host reads that word WITHOUT
// waiting, while the GPU may be in the middle of a render, so it must only ever hold the maximum of a COMPLETED render.
// Two things were tried first in round 6 and measured: a running maximum mirrored into the host word by whichever wave
// raises it (the host saw 300 of an 8 000-entry walk, took the unsplit kernels, and the path flip-flopped), and tickets
// -- every wave counts its arrival, the last one publishes (k_draw 152 -> 452 us: 8 160 returning device-scope atomics
// on one cache line serialise at ~40 ns each, sharded or not).  What is left costs nothing: the waves gather the
// maximum in a PERSISTENT device word the host keeps per (problem size, stream) -- the conditional load keeps all but a
// few dozen waves off the atomic -- and the range kernel of the NEXT render on that stream publishes it (stream order:
// the render it belongs to is complete) and resets it to -1 = "nothing gathered yet".
// (Round 5: a k_seg_report launch behind the compose launch, 6 us; nothing on the unsplit path, where the word was
// refreshed every 4th render of a camera by k_tile_order -- after reset_alpha a trainer kept walking 8 000-entry lists
// with one wave per tile for an epoch.)
__device__ __forceinline__ void walk_raise(int32_t* __restrict__ word, int wmax) {
  if (word && wmax > *word) atomicMax(word, wmax);
}

// min(x, hi) as ONE v_med3_f32 (fminf() costs a canonicalising v_max + v_min in IEEE mode; the
// low bound is finite so the compiler cannot fold the median back into a min)
__device__ __forceinline__ float min_hi(float x, float hi) {
  return __builtin_amdgcn_fmed3f(x, hi, -3.0e38f);
}

// ---- the forward blend of a tile list, once ---------------------------------------------------------------------------
// k_draw and k_draw_seg walk their lists with blend_range below; the list-walk kernels (egs_list_walk.h) bound the same
// walk by the forward's `contrib` instead of tau and so keep a loop of their own, built from the same stage_math and
// pixel_exponent: every kernel that forms alpha' of a (tile, entry, pixel) forms it with the same operations in the same
// order.
//
// One wave64 per 16x16 tile, four pixels per lane: pixel k = 2 by + bx of lane l is (tx0 + (l & 7) + 8 bx,
// ty0 + (l >> 3) + 8 by).  The exponent of alpha' = exp2(e) is evaluated as a polynomial in the pixel's offset (X, Y)
// from the TILE CENTRE:  e = c0 + c1 X + c2 Y + qxx XX + qxy XY + qyy YY  with the entry's  c0 = log2(alpha) + E(D),
// (c1, c2) = grad E(D), D = tile centre - u, computed once per (tile, entry) by the lane that stages the
// entry (64 entries in parallel), and the monomials per-lane CONSTANTS (|X|, |Y| <= 7.5).  Five FMAs
// per 8x8 block and no per-entry set-up (the separable form cxx[bx] + cyy[by] + cxy[bx] dy[by] cost 14
// VALU instructions per entry before the first block); same accuracy as differences from u itself
// (emulated in fp32 on the 1 M scene: mean |error| 6e-7, max 4e-5 in the log2 domain, either way).
struct TileLane {
  int pxb[2], pyb[2];
  float X[2], Y[2], XX[2], YY[2], XY[4];
};
__device__ __forceinline__ void tile_lane_init(TileLane& G, int tx0, int ty0, int lane) {
  G.pxb[0] = tx0 + (lane & 7); G.pxb[1] = G.pxb[0] + 8;
  G.pyb[0] = ty0 + (lane >> 3); G.pyb[1] = G.pyb[0] + 8;
  G.X[0] = (float)(lane & 7) - 7.5f; G.X[1] = (float)(lane & 7) + 0.5f;
  G.Y[0] = (float)(lane >> 3) - 7.5f; G.Y[1] = (float)(lane >> 3) + 0.5f;
#pragma unroll
  for (int b = 0; b < 2; ++b) { G.XX[b] = G.X[b] * G.X[b]; G.YY[b] = G.Y[b] * G.Y[b]; }
#pragma unroll
  for (int k = 0; k < 4; ++k) G.XY[k] = G.X[k & 1] * G.Y[k >> 1];
}

// What the lane that stages a list entry computes from its record (A, B, C) and its list value gm: returns the entry's
// 4-bit reach mask, Q = (qxx, qxy, qyy, cap) and the polynomial (c0, c1, c2) about the centre (cx0, cy0) = (tx0 + 7.5,
// ty0 + 7.5) of the tile.  The centre is handed in: a chunk loop forms it once, in front of the loop (formed in here,
// k_draw's EXTRA instances at eight waves spilled two more registers).  The caller packs the results into its own LDS
// pieces, with the colours, z or the pixel box it needs.
template <bool BOX, bool FLOOR, bool CLAMP, bool SKIP>
__device__ __forceinline__ int stage_math(float4 A, float4 B, const float4& C, int gm, int tx0, int ty0, float cx0,
                                          float cy0, float lskip, int masked, int nan_blend, float4& Q, float& c0,
                                          float& c1, float& c2) {
  constexpr float L99 = -0.014499569695115089f;  // log2(0.99): min(0.99, a) == exp2(min(log2 a, L99))
  int mymask = 0;
  const bool nanfix = nan_blend && nan_entry_fix(A, B);
  // the record's thr = log2(skip / alpha), +inf for an entry that never blends (alpha < skip, or
  // alpha < 0 when there is no skip test): such an entry reaches nothing
  if (C.w < INFINITY) mymask = masked ? (int)((uint32_t)gm >> EGS_GSID_BITS) : reach_mask<BOX>(A, C, tx0, ty0);
  // (a NaN entry blends everywhere, its certain-miss box says nothing -- unmasked lists: the public splatB's rebuild,
  // EGS_CULL_LISTS=0)
  if (nanfix && !BOX && !masked && C.w < INFINITY) mymask = 0xF;
  // alpha' = exp2(e), e = log2(alpha) + log2 exp(-maha/2) (F.5.1, common.cuh:85-88, pre-scaled conic):
  // no multiply by alpha; the floor (maha >= 0) and the 0.99 clamp are ONE min against `cap`
  const float la = SKIP ? lskip - C.w : __builtin_amdgcn_logf(B.y);
  float cap = 3.0e38f;
  if (FLOOR) cap = CLAMP ? fminf(la, L99) : la;
  else if (CLAMP) cap = L99;
  const float Dx = cx0 - A.x, Dy = cy0 - A.y;
  c0 = la + (A.z * Dx * Dx + A.w * Dx * Dy + B.x * Dy * Dy);
  c1 = 2.f * A.z * Dx + A.w * Dy;
  c2 = 2.f * B.x * Dy + A.w * Dx;
  Q = make_float4(A.z, A.w, B.x, cap);
  return mymask;
}

// The exponent of a staged entry (Q, P = (c0, c1, c2, .)) at pixel k of the lane: five FMAs, in this order.
__device__ __forceinline__ float pixel_exponent(const TileLane& G, int k, const float4& Q, const float4& P) {
  const int bx = k & 1, by = k >> 1;
  float e = fmaf(P.z, G.Y[by], P.x);
  e = fmaf(P.y, G.X[bx], e);
  e = fmaf(Q.z, G.YY[by], e);
  e = fmaf(Q.y, G.XY[k], e);
  e = fmaf(Q.x, G.XX[bx], e);
  return e;
}

// Front-to-back blend of entries [e0, e1) of the tile list that starts at gsid[r0] into the caller's blend state, in
// 64-entry chunks staged in the caller's LDS arrays.  The state of the lane's four pixels: tau, the colour sums cr, cg, cb,
// cd = sum w z (EXTRA) and cont, the 1-based list index of the last contributor; `live` is wave-uniform, bit k set while
// block k still has an unfinished pixel.  A pixel is finished when its tau fell below tau_stop (kernel.cu:256-260):
// `tau >= stop` IS the "still blending" test, so no separate done flag is kept; a pixel that does not take part (outside
// the image, finished in front of a segment) starts at tau = -1.  The tile is walked as four 8x8 pixel blocks; per list
// entry a block is skipped outright when the entry does not reach it or no pixel of it is unfinished -- wave-uniform
// branches.  EXTRA also blends the Gaussian's camera-space z (`depths`; non-BOX entries carry it in the free pair of
// their third piece, BOX entries in sZ).
// The state is seven references, not one struct, and that is measured: with the arrays in one struct every k_draw
// instance at eight waves spilled (28 to 130 registers against 0 to 3).
template <bool BOX, bool FLOOR, bool CLAMP, bool SKIP, bool EXTRA>
__device__ __forceinline__ void blend_range(float (&tau)[4], float (&cr)[4], float (&cg)[4], float (&cb)[4],
                                            float (&cd)[4], int (&cont)[4], int& live, const TileLane& G, int e0, int e1,
                                            int r0, int tx0, int ty0, int lane, float stop, float lskip, int masked,
                                            int nan_blend, const int32_t* __restrict__ gsid,
                                            const float4* __restrict__ rec, const float* __restrict__ depths,
                                            float4* sA, float4* sB, float4* sC, float* sZ) {
  // alpha' >= alpha_skip (kernel.cu:246) in the exponent domain: e >= log2(skip), a kernel constant (SKIP =
  // the policy has a skip threshold, compiled in); without one only a NaN exponent fails the compare
  const float lthr = SKIP ? lskip : -INFINITY;
  const float cx0 = (float)tx0 + 7.5f, cy0 = (float)ty0 + 7.5f;   // the tile centre
  // the list value of the NEXT chunk is fetched one chunk ahead: the staging of a chunk then pays one global
  // latency (the record gather), not two dependent ones
  int gnext = (e0 + lane < e1) ? gsid[r0 + e0 + lane] : 0;
  for (int base = e0; base < e1 && live != 0; base += 64) {
    __syncthreads();  // single-wave workgroup: orders the LDS reads of the previous chunk
    int mymask = 0;   // reach mask of the entry THIS lane staged (lane j <-> entry base + j)
    const int gm = gnext;
    const int g = masked ? (int)((uint32_t)gm & EGS_GSID_MASK) : gm;
    if (base + 64 + lane < e1) gnext = gsid[r0 + base + 64 + lane];
    if (base + lane < e1) {
      const float4 A = rec[3 * (size_t)g], B = rec[3 * (size_t)g + 1], C = rec[3 * (size_t)g + 2];
      float z = 0.f;
      if constexpr (EXTRA) z = depths[g];
      float4 Q;
      float c0, c1, c2;
      mymask = stage_math<BOX, FLOOR, CLAMP, SKIP>(A, B, C, gm, tx0, ty0, cx0, cy0, lskip, masked, nan_blend, Q, c0, c1,
                                                   c2);
      // staged entry: 12 floats (BOX: three b128 pieces) or 10 (two b128 + one b64: an entry's broadcast reads are
      // 50 of the ~130 SIMD cycles it costs, on an LDS pipe the CU's four SIMDs share; b64 is half a b128)
      // (the third piece keeps the 16-B slot stride: all three reads are immediate offsets from ONE address register)
      sA[lane] = Q;
      if constexpr (BOX) {
        sB[lane] = make_float4(c0, c1, c2, C.y);      // polynomial about the tile centre; x pixel box
        sC[lane] = make_float4(B.z, B.w, C.x, C.z);   // colour; y pixel box
        if constexpr (EXTRA) sZ[lane] = z;            // (no free float in the BOX slots: a piece of its own)
      } else {
        sB[lane] = make_float4(c0, c1, c2, B.z);      // polynomial about the tile centre; red
        if constexpr (EXTRA) sC[lane] = make_float4(B.w, C.x, z, 0.f);   // green, blue, z
        else *reinterpret_cast<float2*>(&sC[lane]) = make_float2(B.w, C.x);   // green, blue
      }
    }
    __syncthreads();
    // The reach masks of eight consecutive entries packed into one dword (4 bits each), gathered into the
    // group's first lane through the LDS permute path (ds_bpermute: no VALU issue slot): the blend loop
    // reads ONE SGPR per group of eight entries, skips the whole group when none of them reaches a live
    // block, and is fully unrolled over the group -- LDS addresses are an immediate offset from one base,
    // no per-entry v_readlane / v_mov / loop counter.  (Entries past the end of the range staged mask 0.)
    int pk = mymask;
    pk |= __shfl_down(pk, 1, 64) << 4;
    pk |= __shfl_down(pk, 2, 64) << 8;
    pk |= __shfl_down(pk, 4, 64) << 16;
    const int m = __builtin_amdgcn_readfirstlane(min(64, e1 - base));
    for (int j0 = 0; j0 < m && live != 0; j0 += 8) {  // eight entries, then the live-mask refresh
      const uint32_t act = (uint32_t)__builtin_amdgcn_readlane(pk, j0) & ((uint32_t)live * 0x11111111u);
      if (act != 0u) {
      const int vidx0 = base + j0 + 1;
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        const int reach = (int)((act >> (4 * t)) & 0xFu);
        if (reach != 0) {  // scalar branch: some live block is within reach of this entry
          const int j = j0 + t;
          const float4 Q = sA[j], P = sB[j];            // wave-uniform address: LDS broadcast
          float4 K;
          float zj = 0.f;
          if constexpr (BOX) { K = sC[j]; if constexpr (EXTRA) zj = sZ[j]; }
          else if constexpr (EXTRA) { const float4 gbz = sC[j]; K = make_float4(P.w, gbz.x, gbz.y, 0.f); zj = gbz.z; }
          else { const float2 gb = *reinterpret_cast<const float2*>(&sC[j]); K = make_float4(P.w, gb.x, gb.y, 0.f); }
          bool inx[2] = {true, true}, iny[2] = {true, true};
          if (BOX) {
            const uint32_t bx = __float_as_uint(P.w), by = __float_as_uint(K.w);
            const int x0 = bx & 0xFFFF, x1 = bx >> 16, y0 = by & 0xFFFF, y1 = by >> 16;
#pragma unroll
            for (int b = 0; b < 2; ++b) {
              inx[b] = (G.pxb[b] >= x0) && (G.pxb[b] < x1);
              iny[b] = (G.pyb[b] >= y0) && (G.pyb[b] < y1);
            }
          }
          const int idx = vidx0 + t;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            if (reach & (1 << k)) {  // scalar branch: the whole 8x8 block is live and in reach
              float e = pixel_exponent(G, k, Q, P);
              // unfinished and alpha' >= alpha_skip; the cap cannot change the outcome of the skip test
              // (cap >= log2(skip) for every entry that blends at all), so it is applied to the hits only
              bool hit = (tau[k] >= stop) && (e >= lthr);
              if (BOX) hit = hit && inx[k & 1] && iny[k >> 1];
              if (hit) {
                if (FLOOR || CLAMP) e = min_hi(e, Q.w);
                const float w = tau[k] * __builtin_amdgcn_exp2f(e);  // F.5: tau alpha'
                cr[k] += w * K.x; cg[k] += w * K.y; cb[k] += w * K.z;
                if constexpr (EXTRA) cd[k] += w * zj;
                tau[k] -= w;  // F.5.2: tau (1 - alpha')
                cont[k] = idx;
              }
            }
          }
        }
      }
      // Finished pixels fail `tau >= stop` on their own, so the live-block mask only saves work: it is
      // refreshed after a group that blended something instead of tracking "some pixel just finished" per
      // block; when it empties, every pixel of the tile is finished and both loops end (scalar exit).
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if ((live & (1 << k)) && !__any(tau[k] >= stop)) live &= ~(1 << k);
      }
    }
  }
}

// ---- what k_draw and k_draw_seg share around the loop ---------------------------------------------------------------
// every workgroup of the grid (padding ones included) clears its slice of p.zero_buf
__device__ __forceinline__ void zero_slice(const DrawParams& p, int lane) {
  if (p.zero_buf) {
    const uint32_t z0 = blockIdx.x * p.zero_per, z1 = min(p.zero_n4, z0 + p.zero_per);
    float4* __restrict__ zb = p.zero_buf;
    for (uint32_t i = z0 + lane; i < z1; i += 64) zb[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

// empty tile: image = 0, contrib = 0 and final_tau = 0 (NOT 1), exactly what the reference's early return leaves in
// its zero-filled outputs (kernel.cu:182); ex (EXTRA only): the background, no depth, no opacity
template <bool EXTRA>
__device__ __forceinline__ void empty_tile(const TileLane& G, const DrawParams& p, int tile, int r0, int r1, int lane,
                                           int32_t* __restrict__ ranges, float* __restrict__ image,
                                           int32_t* __restrict__ contrib, float* __restrict__ final_tau,
                                           const DrawExtras* ex) {
  // a tile without patches still holds the (INT_MAX, 0) the binning initialised it with: (0, 0), as the reference
  if (lane == 0 && (r0 != 0 || r1 != 0)) { ranges[2 * (size_t)tile] = 0; ranges[2 * (size_t)tile + 1] = 0; }
  const size_t HW = (size_t)p.W * p.H;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int px = G.pxb[k & 1], py = G.pyb[k >> 1];
    if (px < p.W && py < p.H) {
      const size_t pix = (size_t)py * p.W + px;
      if constexpr (EXTRA) {   // T = 1 here (final_tau keeps its quirk)
        image[pix] = ex->bg[0]; image[HW + pix] = ex->bg[1]; image[2 * HW + pix] = ex->bg[2];
        if (ex->depth_out) ex->depth_out[pix] = 0.f;
        if (ex->alpha_out) ex->alpha_out[pix] = 0.f;
      } else {
        image[pix] = 0.f; image[HW + pix] = 0.f; image[2 * HW + pix] = 0.f;
      }
      contrib[pix] = 0; final_tau[pix] = 0.f;
    }
  }
}

// how far a tile was walked, from its pixels' last contributors: w = the sum over the four blocks of the block's largest
// contributor index, wmax = the tile's (the work measure is w + 2 wmax, the walk wmax)
__device__ __forceinline__ void block_max(const int (&cont)[4], int& w, int& wmax) {
  w = 0; wmax = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    int mx = cont[k];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mx = max(mx, __shfl_xor(mx, d, 64));
    w += mx;
    wmax = max(wmax, mx);
  }
}

// gfx950 cross-half / cross-row swaps (v_permlane32_swap_b32, v_permlane16_swap_b32)
__device__ __forceinline__ void swap32(float& a, float& b) {  // a[32..63] <-> b[0..31]
  auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
  a = __uint_as_float(r[0]);
  b = __uint_as_float(r[1]);
}
__device__ __forceinline__ void swap16(float& a, float& b) {  // odd rows of a <-> even rows of b
  auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
  a = __uint_as_float(r[0]);
  b = __uint_as_float(r[1]);
}
template <int CTRL>
__device__ __forceinline__ float dpp_get(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}

// ---- transposing wave reduction of four entries -------------------------------------------------------------------
// Two steps, both generic over the operation (add unless told otherwise).  rows_of4: four per-lane partials become one
// register of row-wise partials -- after the two swaps row r of the wave holds 16 partials of entry {0, 2, 1, 3}[r]
// (k_draw_bwd stops here and merges nine such registers inside the rows).  row_total: four DPP steps inside the row
// leave the total in every lane of it.  total_of4 is the two together.
struct OpAdd { __device__ __forceinline__ float operator()(float a, float b) const { return a + b; } };
struct OpMax { __device__ __forceinline__ float operator()(float a, float b) const { return fmaxf(a, b); } };

template <typename Op = OpAdd>
__device__ __forceinline__ float rows_of4(float e0, float e1, float e2, float e3, Op op = Op{}) {
  swap32(e0, e1);
  float a = op(e0, e1);   // lanes 0-31: e0 halves, lanes 32-63: e1 halves
  swap32(e2, e3);
  float b = op(e2, e3);
  swap16(a, b);           // rows of a: [e0, e2, e1, e3]; rows of b: the other halves
  return op(a, b);
}
template <typename Op = OpAdd>
__device__ __forceinline__ float row_total(float v, Op op = Op{}) {
  v = op(v, dpp_get<0x140>(v));   // row_mirror
  v = op(v, dpp_get<0x141>(v));   // row_half_mirror
  v = op(v, dpp_get<0x4E>(v));    // quad_perm [2, 3, 0, 1]
  v = op(v, dpp_get<0xB1>(v));    // quad_perm [1, 0, 3, 2]
  return v;
}
template <typename Op = OpAdd>
__device__ __forceinline__ float total_of4(float e0, float e1, float e2, float e3, Op op = Op{}) {
  return row_total(rows_of4(e0, e1, e2, e3, op), op);
}

}  // namespace egs
