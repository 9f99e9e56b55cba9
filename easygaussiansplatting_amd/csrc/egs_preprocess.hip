// Per-Gaussian stages of the splatting pipeline for gfx950 (wave64):
//   * the five ops of the reference surface -- project / cov3d / cov2d / sh2color /
//     inv_cov2d (+ optional Jacobians stored to HBM, as gsplatcu does) -- and the chain
//     rule kernel that consumes those Jacobians;
//   * the fused training path: k_preprocess_fwd (all five stages in
//     one pass, 236 B read + 44 B written per Gaussian, no Jacobians materialised) and
//     k_preprocess_bwd (re-derives the Jacobians in registers and applies the chain rule:
//     236 + 48 B read, 244 B written, instead of 436 B of Jacobians written then re-read).
//
// The math lives in egs_gaussian_math.h (one source of truth for both paths), the row traffic
// in egs_rows.h: rows_in / rows_out move a workgroup's 256 rows through LDS as one coalesced
// span, load_row is a lane's own vector loads.
// All kernels: one Gaussian per lane, 256-thread workgroups (4 waves), >= 3900
// workgroups at N = 1 M so all 256 CUs are covered many times over.  They are
// HBM-bound streaming kernels; algorithmic bytes per Gaussian are listed in DESIGN.md.
#include "egs_gaussian_math.h"
#include "egs_rows.h"

namespace egs {

// ---- project                                          (reference kernel.cu:553-617)
// (60 B per Gaussian: too little to pay for a trip through LDS -- measured 20 us direct, 23 us staged; every row is
// still written, culled Gaussians as zeros)
__global__ __launch_bounds__(256) void k_project(int n, const float* __restrict__ pws,
                                                 const float* __restrict__ Rcw,
                                                 const float* __restrict__ tcw, float fx, float fy,
                                                 float cx, float cy, int near_cull,
                                                 float* __restrict__ us, float* __restrict__ pcs,
                                                 float* __restrict__ depths,
                                                 float* __restrict__ du_dpcs) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const Proj P = project_f(ld3(pws + 3 * (size_t)i), Rcw, tcw, fx, fy, cx, cy);
  const bool cull = near_cull && P.pc.z < EGS_MIN_DEPTH;
  float2* J2 = du_dpcs ? reinterpret_cast<float2*>(du_dpcs + 6 * (size_t)i) : nullptr;   // 24-B rows: 8-B aligned
  if (cull) {   // everything but the marker reads 0, like the reference's zero-filled outputs
    reinterpret_cast<float2*>(us)[i] = make_float2(0.f, 0.f);
    st3(pcs + 3 * (size_t)i, {0.f, 0.f, 0.f});
    depths[i] = EGS_BAD_MARKER;
    if (J2) { J2[0] = make_float2(0.f, 0.f); J2[1] = make_float2(0.f, 0.f); J2[2] = make_float2(0.f, 0.f); }
    return;
  }
  reinterpret_cast<float2*>(us)[i] = make_float2(P.u0, P.u1);
  st3(pcs + 3 * (size_t)i, P.pc);
  depths[i] = P.pc.z;
  if (J2) {
    float j00, j02, j11, j12;
    project_jac(P, fx, fy, j00, j02, j11, j12);
    J2[0] = make_float2(j00, 0.f); J2[1] = make_float2(j02, 0.f); J2[2] = make_float2(j11, j12);
  }
}

// ---- cov3d                                            (reference kernel.cu:326-423)
__global__ __launch_bounds__(256) void k_cov3d(int n, const float* __restrict__ rots,
                                               const float* __restrict__ scales,
                                               const float* __restrict__ depths, int near_cull,
                                               float* __restrict__ cov3ds,
                                               float* __restrict__ dcov3d_drots,
                                               float* __restrict__ dcov3d_dscales) {
  __shared__ float stage[RowStage<24>::OUT_LDS_FLOATS];
  const int base = blockIdx.x * 256, i = base + threadIdx.x;
  const bool jac = dcov3d_drots && dcov3d_dscales;
  float c6[6], dq[24], ds[18];
#pragma unroll
  for (int k = 0; k < 6; ++k) c6[k] = 0.f;
#pragma unroll
  for (int k = 0; k < 24; ++k) dq[k] = 0.f;
#pragma unroll
  for (int k = 0; k < 18; ++k) ds[k] = 0.f;
  if (i < n && !(near_cull && depths[i] < EGS_MIN_DEPTH)) {
    const float4 q = *reinterpret_cast<const float4*>(rots + 4 * (size_t)i);  // 16-B aligned rows
    const f3 s = ld3(scales + 3 * (size_t)i);
    const Cov3 c = cov3d_f(q, s);
#pragma unroll
    for (int k = 0; k < 6; ++k) c6[k] = c.c[k];
    if (jac) cov3d_jac(c, q, s, dq, ds);
  }
  rows_out<6>(c6, cov3ds, n, base, stage);
  if (jac) {
    rows_out<24>(dq, dcov3d_drots, n, base, stage);
    rows_out<18>(ds, dcov3d_dscales, n, base, stage);
  }
}

// ---- cov2d                                            (reference kernel.cu:425-551)
__global__ __launch_bounds__(256) void k_cov2d(int n, const float* __restrict__ cov3ds,
                                               const float* __restrict__ pcs,
                                               const float* __restrict__ Rcw,
                                               const float* __restrict__ depths, float fx, float fy,
                                               float limx, float limy, int clamp_fov, int near_cull,
                                               float* __restrict__ cov2ds,
                                               float* __restrict__ dcov2d_dcov3ds,
                                               float* __restrict__ dcov2d_dpcs) {
  __shared__ float stage[RowStage<18>::OUT_LDS_FLOATS];
  const int base = blockIdx.x * 256, i = base + threadIdx.x;
  const bool jac = dcov2d_dcov3ds && dcov2d_dpcs;
  float c3[3] = {0.f, 0.f, 0.f}, J3[18], Jp[9];
#pragma unroll
  for (int k = 0; k < 18; ++k) J3[k] = 0.f;
#pragma unroll
  for (int k = 0; k < 9; ++k) Jp[k] = 0.f;
  if (i < n && !(near_cull && depths[i] < EGS_MIN_DEPTH)) {
    const f3 pc = ld3(pcs + 3 * (size_t)i);
    float cv[6];
    const float2* cr = reinterpret_cast<const float2*>(cov3ds + 6 * (size_t)i);   // 24-B rows: 8-B aligned
#pragma unroll
    for (int k = 0; k < 3; ++k) { const float2 v = cr[k]; cv[2 * k] = v.x; cv[2 * k + 1] = v.y; }
    const Cov2 c = cov2d_f(cv, pc, Rcw, fx, fy, limx, limy, clamp_fov);
    c3[0] = c.c[0]; c3[1] = c.c[1]; c3[2] = c.c[2];
    if (jac) cov2d_jac(c, pc.z, Rcw, fx, fy, J3, Jp);
  }
  rows_out<3>(c3, cov2ds, n, base, stage);
  if (jac) {
    rows_out<18>(J3, dcov2d_dcov3ds, n, base, stage);
    rows_out<9>(Jp, dcov2d_dpcs, n, base, stage);
  }
}

// ---- sh2color                                         (reference kernel.cu:619-807)
// Colour and dcolor/dpw come out of ONE pass over the SH row here (sh_color_and_jac_dpw).  (Tried: the same one pass
// in k_preprocess_fwd<.., JW> -- 82 -> 60 VGPRs, 5 -> 8 waves per SIMD, and SLOWER, 99 -> 110 us: more resident waves
// mean more SH rows competing for the 32-KB L1 between the twelve row loads of a lane; docs/LAB.md)
constexpr int SH2COLOR_WAVES = 1;   // minimum waves per SIMD of k_sh2color (106 VGPRs = 4 as compiled freely)
template <int NC>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(SH2COLOR_WAVES, 8))) void k_sh2color(int n, const float* __restrict__ shs,
                                                  const float* __restrict__ pws,
                                                  const float* __restrict__ twc,
                                                  float* __restrict__ colors,
                                                  float* __restrict__ dcolor_dshs,
                                                  float* __restrict__ dcolor_dpws) {
  __shared__ float stage[cmax(RowStage<NC>::OUT_LDS_FLOATS, RowStage<9>::OUT_LDS_FLOATS)];
  const int base = blockIdx.x * 256, i = base + threadIdx.x;
  constexpr int K = 3 * NC;
  const bool jac = dcolor_dshs && dcolor_dpws;
  float col[3] = {0.f, 0.f, 0.f}, jp[9];
#pragma unroll
  for (int j = 0; j < 9; ++j) jp[j] = 0.f;
  // Round 4: the basis row leaves FIRST (it depends on the direction alone), then ONE pass over the coefficients sums
  // colour and dcolor/ddir, re-evaluating each basis value where it is used: neither the 16 basis values nor the
  // consumed part of the SH row stay in registers (110 -> see DESIGN 3.1).
  float sh[K];
  ShDir<NC> d;
#pragma unroll
  for (int c = 0; c < NC; ++c) d.B[c] = 0.f;
  d.d0 = 0.f; d.d1 = 0.f; d.d2 = 0.f; d.ninv = 0.f; d.x = 0.f; d.y = 0.f; d.z = 0.f;
  if (i < n) {   // colour has no depth test in the reference (kernel.cu:619-725)
    load_row<K>(shs + (size_t)K * i, sh);
    d = sh_basis_f<NC>(ld3(pws + 3 * (size_t)i), twc);
  }
  if (jac) {
    rows_out<NC>(d.B, dcolor_dshs, n, base, stage);
    // (the direction is laundered: the compiler must not keep the 16 stored values alive for the pass below)
    asm volatile("" : "+v"(d.x), "+v"(d.y), "+v"(d.z));
    if (i < n) sh_color_and_jac_dpw<NC, true, true>(d, sh, col, jp);
  } else if (i < n) {
    sh_color_and_jac_dpw<NC, true, false>(d, sh, col, jp);
  }
  rows_out<3>(col, colors, n, base, stage);
  if (jac) rows_out<9>(jp, dcolor_dpws, n, base, stage);
}

// ---- inverse_cov2d                                    (reference kernel.cu:274-324)
__global__ __launch_bounds__(256) void k_inv_cov2d(int n, const float* __restrict__ cov2ds,
                                                   float* __restrict__ depths, float det_eps,
                                                   int near_cull, int nan_cull, int radius_mode,
                                                   float* __restrict__ cinv2ds,
                                                   int32_t* __restrict__ areas,
                                                   float* __restrict__ dcinv2d_dcov2ds) {
  __shared__ float stage[RowStage<9>::OUT_LDS_FLOATS];
  const int base = blockIdx.x * 256, i = base + threadIdx.x;
  float ci[3] = {0.f, 0.f, 0.f}, ar[2] = {0.f, 0.f}, J[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) J[k] = 0.f;
  if (i < n && !(near_cull && depths[i] < EGS_MIN_DEPTH)) {
    const float c2[3] = {cov2ds[3 * (size_t)i], cov2ds[3 * (size_t)i + 1], cov2ds[3 * (size_t)i + 2]};
    float cc[3];
    const float det_inv = inv_cov2d_f(c2, det_eps, cc);
    if (nan_cull && isnan(det_inv)) {
      depths[i] = EGS_BAD_MARKER;  // in-place contract GSFunction relies on (gsmodel.py:50)
    } else {
      ci[0] = cc[0]; ci[1] = cc[1]; ci[2] = cc[2];
      int rx, ry;
      radius_f(c2, radius_mode, rx, ry);
      ar[0] = __int_as_float(rx); ar[1] = __int_as_float(ry);   // (bit patterns of the int32 radii)
      if (dcinv2d_dcov2ds) inv_cov2d_jac(c2, det_inv, J);
    }
  }
  rows_out<3>(ci, cinv2ds, n, base, stage);
  rows_out<2>(ar, reinterpret_cast<float*>(areas), n, base, stage);
  if (dcinv2d_dcov2ds) rows_out<9>(J, dcinv2d_dcov2ds, n, base, stage);
}

// ----------------------------------------------------------------------------
// fused chain rule: reference gsplat/gsmodel.py:71-85 == backward_cpu.py:476-482
// (nine batched [N,1,a]@[N,a,b] matmuls there; one pass over the Jacobians here)
// ----------------------------------------------------------------------------
template <int NC>
__global__ __launch_bounds__(256) void k_chain_rule(
    int n, const float* __restrict__ dL_du, const float* __restrict__ dL_dcinv,
    const float* __restrict__ dL_dcolor, const float* __restrict__ Rcw,
    const float* __restrict__ J_cinv_cov2, const float* __restrict__ J_cov2_cov3,
    const float* __restrict__ J_cov3_rot, const float* __restrict__ J_cov3_scale,
    const float* __restrict__ J_color_sh, const float* __restrict__ J_u_pc,
    const float* __restrict__ J_cov2_pc, const float* __restrict__ J_color_pw,
    float* __restrict__ dL_dpw, float* __restrict__ dL_dsh, float* __restrict__ dL_dscale,
    float* __restrict__ dL_drot) {
  constexpr int K = 3 * NC;
  __shared__ float stage[cmax(RowStage<K>::OUT_LDS_FLOATS, RowStage<3>::OUT_LDS_FLOATS)];
  const int base = blockIdx.x * 256, i = base + threadIdx.x;
  float grot[4] = {0.f, 0.f, 0.f, 0.f}, gsc[3] = {0.f, 0.f, 0.f}, gpw[3] = {0.f, 0.f, 0.f}, gsh[K];
#pragma unroll
  for (int k = 0; k < K; ++k) gsh[k] = 0.f;
  if (i < n) {
    const f3 gci = ld3(dL_dcinv + 3 * (size_t)i);
    float A[9];
    load_row<9>(J_cinv_cov2 + 9 * (size_t)i, A);
    // dL/dcov2d = dL/dcinv2d @ J (row vector times 3x3)
    const f3 gc2 = {gci.x * A[0] + gci.y * A[3] + gci.z * A[6], gci.x * A[1] + gci.y * A[4] + gci.z * A[7],
                    gci.x * A[2] + gci.y * A[5] + gci.z * A[8]};
    float Bm[18];
    load_row<18>(J_cov2_cov3 + 18 * (size_t)i, Bm);
    float gc3[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) gc3[k] = gc2.x * Bm[k] + gc2.y * Bm[6 + k] + gc2.z * Bm[12 + k];
    float Cq[24];
    load_row<24>(J_cov3_rot + 24 * (size_t)i, Cq);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float s = 0.f;
#pragma unroll
      for (int r = 0; r < 6; ++r) s += gc3[r] * Cq[4 * r + k];
      grot[k] = s;
    }
    float Cs[18];
    load_row<18>(J_cov3_scale + 18 * (size_t)i, Cs);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      float s = 0.f;
#pragma unroll
      for (int r = 0; r < 6; ++r) s += gc3[r] * Cs[3 * r + k];
      gsc[k] = s;
    }
    const f3 gcol = ld3(dL_dcolor + 3 * (size_t)i);
    float Bs[NC];
    load_row<NC>(J_color_sh + (size_t)NC * i, Bs);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      gsh[3 * c] = gcol.x * Bs[c]; gsh[3 * c + 1] = gcol.y * Bs[c]; gsh[3 * c + 2] = gcol.z * Bs[c];
    }
    // dL/dpc = dL/du @ du_dpc + dL/dcov2d @ dcov2d_dpc ; dL/dpw = dL/dpc @ Rcw + dL/dcolor @ dcolor_dpw
    const float2 gu = reinterpret_cast<const float2*>(dL_du)[i];
    const float gu0 = gu.x, gu1 = gu.y;
    float U[6], Pc[9], W[9];
    load_row<6>(J_u_pc + 6 * (size_t)i, U);
    load_row<9>(J_cov2_pc + 9 * (size_t)i, Pc);
    load_row<9>(J_color_pw + 9 * (size_t)i, W);
    const f3 gpc = {gu0 * U[0] + gu1 * U[3] + gc2.x * Pc[0] + gc2.y * Pc[3] + gc2.z * Pc[6],
                    gu0 * U[1] + gu1 * U[4] + gc2.x * Pc[1] + gc2.y * Pc[4] + gc2.z * Pc[7],
                    gu0 * U[2] + gu1 * U[5] + gc2.x * Pc[2] + gc2.y * Pc[5] + gc2.z * Pc[8]};
#pragma unroll
    for (int k = 0; k < 3; ++k)
      gpw[k] = gpc.x * Rcw[k] + gpc.y * Rcw[3 + k] + gpc.z * Rcw[6 + k] + gcol.x * W[k] + gcol.y * W[3 + k] +
               gcol.z * W[6 + k];
    *reinterpret_cast<float4*>(dL_drot + 4 * (size_t)i) = make_float4(grot[0], grot[1], grot[2], grot[3]);
  }
  rows_out<3>(gsc, dL_dscale, n, base, stage);
  rows_out<3>(gpw, dL_dpw, n, base, stage);
  rows_out<K>(gsh, dL_dsh, n, base, stage);   // the 4K-byte dL/dsh rows leave as full lines
}

// ============================================================================
// fused training path
// ============================================================================
struct PreParams {
  float fx, fy, cx, cy, limx, limy, det_eps, alpha_skip;
  int clamp_fov, near_cull, nan_cull, radius_mode, footprint, W, H;
};

// ---- activations of the raw training parameters (reference gsplat/utils.py:121-150) -------------
// The RAW variants of the fused kernels read the optimizer's own tensors -- alphas_raw, scales_raw,
// rots_raw, low_shs [N,3] and high_shs [N,K-3] -- and return gradients with respect to THEM, so the
// torch ops around GSFunction (sigmoid, exp, normalize, cat and their autograd twins: ~0.4 ms per
// step at 1 M Gaussians, 12 launches, 0.9 GB of HBM traffic) disappear.
__device__ __forceinline__ float act_alpha(float a) { return 1.f / (1.f + expf(-a)); }   // get_alphas
__device__ __forceinline__ f3 act_scale(const f3& s) { return {expf(s.x), expf(s.y), expf(s.z)}; }  // get_scales
__device__ __forceinline__ float4 act_rot(const float4& r, float& norm) {                // get_rots
  norm = fmaxf(sqrtf(r.x * r.x + r.y * r.y + r.z * r.z + r.w * r.w), 1e-12f);            // F.normalize eps
  return make_float4(r.x / norm, r.y / norm, r.z / norm, r.w / norm);
}

// The SH gradient rows of a workgroup on their way out (k_preprocess_bwd, k_sh_grad_views): dL_dsh [N][K], or for RAW the
// low part dL_dsh [N][3] from its lane and the high part dL_dsh_high [N][K-3] as a span; accum: added to what is there.
// All 256 threads call this (`stage` holds RowStage<K or K-3>::LDS_FLOATS floats).
template <int NC, bool RAW>
__device__ __forceinline__ void sh_grad_rows_out(const float* gsh, float* dL_dsh, float* dL_dsh_high, int n, int base,
                                                 float* stage, bool accum) {
  constexpr int K = 3 * NC, KH = K - 3;
  if constexpr (RAW) {
    const int i = base + threadIdx.x;
    if (i < n) {
#pragma unroll
      for (int k = 0; k < 3; ++k) dL_dsh[3 * (size_t)i + k] = gsh[k] + (accum ? dL_dsh[3 * (size_t)i + k] : 0.f);
    }
    if constexpr (KH > 0) rows_out<KH>(gsh + 3, dL_dsh_high, n, base, stage, accum);
  } else {
    rows_out<K>(gsh, dL_dsh, n, base, stage, accum);
  }
}

// forward.md steps 1-5 for one Gaussian in one pass (== gsmodel.py:21-35 minus splat):
// writes exactly what splat / splatB / the backward pass consume.
// RAW: rots/scales/alphas are the un-activated tensors, shs = low_shs [N,3], shs_high = high_shs [N,K-3]
// JW: also write dcolor/dpw (dcolor_dpws) for the backward pass -- a training render
// Order inside a wave: the four small loads, the whole SH row, then everything that needs no SH coefficient (basis,
// projection, cull, covariances, radius, binning and footprint records, the stores that are final) under the row's
// flight, then colour and dcolor/dpw.  The first wait of the geometry is a counted one (vmcnt(14) .. (12) at SH degree
// 3: the twelve row loads stay outstanding).  The row's 3 NC destination registers are live over the geometry: 101
// VGPRs / 4 waves per SIMD with JW at degree 3, 95 / 5 without -- so no instance is pinned to 8 waves any more (at 64
// VGPRs the degree-2 and degree-3 rows spill).  Measured 101 -> 90 us at 1 M Gaussians, the forward-only render
// 0.353 -> 0.344 ms; docs/LAB.md, DESIGN 3.1, profiles/pre_wave_order_ab.txt.
// (Loads alone do not do it: rotation / scale / opacity requested with the position and all twelve SH loads hoisted,
// but the SH block still FIRST, measured equal to the six dependent round trips before it, 0.860-0.868 ms per step
// either way -- what matters is which arithmetic runs while the row is in flight.)
constexpr int PRE_FWD_WAVES = 1;   // minimum waves per SIMD of every instance (register cap 512 / waves)
// AA (anti-aliased rendering): every Gaussian is binned and drawn with opacity alpha comp
template <int NC, bool RAW, bool JW, bool AA>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(PRE_FWD_WAVES, 8))) void k_preprocess_fwd(int n, PreParams pp, const float* __restrict__ pws,
                                                        const float* __restrict__ rots,
                                                        const float* __restrict__ scales,
                                                        const float* __restrict__ shs,
                                                        const float* __restrict__ shs_high,
                                                        const float* __restrict__ alphas,
                                                        const float* __restrict__ Rcw,
                                                        const float* __restrict__ tcw,
                                                        const float* __restrict__ twc,
                                                        float* __restrict__ us, float* __restrict__ depths,
                                                        float* __restrict__ cinv2ds,
                                                        float* __restrict__ colors,
                                                        int32_t* __restrict__ areas,
                                                        float4* __restrict__ rec, BinParams bp, BinCountOut bo,
                                                        uint8_t* __restrict__ visible,
                                                        float* __restrict__ dcolor_dpws) {
  // dcolor_dpws (nullable, [N][9]): dcolor/dpw of every Gaussian, for the backward pass -- the ONLY thing that pass
  // needs the SH coefficients for (eq (7): dL/dpw += dL/dcolor . dcolor/dpw; dL/dsh needs the basis alone).  36 B
  // written here save the 4K-byte SH row re-read there (192 B at SH degree 3).
  constexpr int K = 3 * NC;
  constexpr int KH = K - 3;   // width of high_shs
  constexpr int STAGE_FLOATS = (RAW && KH > 0 && RowStage<KH>::LDS_FLOATS > RowStage<12>::LDS_FLOATS)
                                   ? RowStage<KH>::LDS_FLOATS : RowStage<12>::LDS_FLOATS;
  __shared__ float stage[STAGE_FLOATS];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (bo.cr)     // the superblock sums of the depth sort that follows must start from zero
    for (uint32_t z = (uint32_t)i; z < bo.sort_sup_words; z += gridDim.x * 256u) bo.sort_sup[z] = 0u;
  uint32_t dkey = 0u;
  float sh[K];
  if constexpr (RAW) {   // 180-B high_shs rows cannot be dwordx4-loaded per lane: the workgroup's span through LDS
    if constexpr (KH > 0) rows_in<KH>(shs_high, n, blockIdx.x * 256, stage, sh + 3);
  }
  float4 r[3] = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};
  float jw[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  uint4 crec = make_uint4(0u, 0u, 0u, 0u);
  if (i < n) {
    // Every input of the row is requested here, the four small ones first and the SH row behind them: the memory
    // counter is in order, so the geometry below waits for the small loads only and runs while the row is in flight.
    // (The near-cull decides what is used, not what is loaded: the addresses are valid for every i < n.)
    const f3 pw = ld3(pws + 3 * (size_t)i);
    float4 q = *reinterpret_cast<const float4*>(rots + 4 * (size_t)i);
    f3 sc = ld3(scales + 3 * (size_t)i);
    const float alpha_in = (rec || bo.br) ? alphas[i] : 0.f;
    if constexpr (RAW) {
      sh[0] = shs[3 * (size_t)i]; sh[1] = shs[3 * (size_t)i + 1]; sh[2] = shs[3 * (size_t)i + 2];
    } else {  // direct dwordx4 row loads: staging them through LDS measured 10 % slower here
      load_row<K>(shs + (size_t)K * i, sh);
    }
    __builtin_amdgcn_sched_barrier(0);   // (no load sinks below this line, no arithmetic rises above it)
    // ---- everything that needs no SH coefficient
    const ShDir<NC> d = sh_basis_f<NC>(pw, twc);
    const Proj P = project_f(pw, Rcw, tcw, pp.fx, pp.fy, pp.cx, pp.cy);
    float u0 = 0.f, u1 = 0.f, depth = EGS_BAD_MARKER, ci[3] = {0.f, 0.f, 0.f};
    int rx = 0, ry = 0;
    float aa_comp = 0.f;   // (AA: the opacity compensation; 0 for near-culled Gaussians)
    if (!(pp.near_cull && P.pc.z < EGS_MIN_DEPTH)) {
      u0 = P.u0; u1 = P.u1; depth = P.pc.z;
      if constexpr (RAW) { float nrm; q = act_rot(q, nrm); sc = act_scale(sc); }
      const Cov3 c3 = cov3d_f(q, sc);
      const Cov2 c2 = cov2d_f(c3.c, P.pc, Rcw, pp.fx, pp.fy, pp.limx, pp.limy, pp.clamp_fov);
      const float det_inv = inv_cov2d_f(c2.c, pp.det_eps, ci);
      if constexpr (AA) aa_comp = aa_comp_f(c2.c);
      if (pp.nan_cull && isnan(det_inv)) {
        depth = EGS_BAD_MARKER; ci[0] = 0.f; ci[1] = 0.f; ci[2] = 0.f;
      } else {
        radius_f(c2.c, pp.radius_mode, rx, ry);
      }
    }
    float alpha_act = (rec || bo.br) ? (RAW ? act_alpha(alpha_in) : alpha_in) : 0.f;
    // AA: the Gaussian is binned and drawn with the compensated opacity alpha comp (the records carry it)
    if constexpr (AA) alpha_act *= aa_comp;
    if (bo.br) {  // getRects + depth key of the binning stage, straight from registers (no k_bin_count pass)
      uint4 rect;
      bool cull;
      const uint32_t cnt = bin_count_one(bp, u0, u1, (float)rx, (float)ry, depth, rect, dkey, cull);
      if (cull) { depth = EGS_BAD_MARKER; rx = 0; ry = 0; }  // in-place contract of splat (kernel.cu:114-119)
      bo.ids[i] = (uint32_t)i;
      // the footprint record of the binning stage and the number of tiles the Gaussian is emitted for: its rect
      // (the reference's lists) or, bp.cull_lists, the tiles its footprint alpha' >= alpha_skip can reach
      const BinRec brec = make_binrec(u0, u1, ci[0], ci[1], ci[2], alpha_act, pp.alpha_skip, bp.cull_lists != 0,
                                      rect, cnt);
      if (cnt) {
        const uint32_t w = brec.wh & 0xFFFFu, h = brec.wh >> 16;
        if (w <= 4u && h <= 4u) {          // the blocks the footprint reaches, as a bitmap: emission is bit arithmetic
          const unsigned long long bits = foot_bitmap(brec);
          crec = make_uint4(brec.xy, brec.wh, (uint32_t)bits, (uint32_t)(bits >> 32));
        } else {                           // a bigger rect
          const bool walk = brec.m < __int_as_float(0x7f800000);
          if (walk && w <= 8u && h <= 8u) {   // its TILES as a bitmap; k_bin_emit evaluates the slabs of one tile
            const unsigned long long bits = foot_tilemap(brec);
            crec = make_uint4(brec.xy, brec.wh | EGS_CR_TILEMAP, (uint32_t)bits, (uint32_t)(bits >> 32));
          } else {                            // counted here, walked row by row by k_bin_emit
            crec = make_uint4(brec.xy, brec.wh | EGS_CR_BIG, walk ? foot_count(brec) : cnt, walk ? 1u : 0u);
          }
          if (walk) {
            float4* o = reinterpret_cast<float4*>(bo.br + i);
            o[0] = make_float4(brec.ux, brec.uy, brec.A, brec.Bh);
            o[1] = make_float4(brec.C, brec.m, __uint_as_float(brec.xy), __uint_as_float(brec.wh));
          }
        }
      }
      bo.dkeys[i] = dkey;
    }
    // us / cinv2ds / colors / areas are only needed by callers that go on with the seven-op surface; the
    // fused path draws from the packed records alone and passes NULL (40 B/Gaussian less to write)
    if (us) { us[2 * (size_t)i] = u0; us[2 * (size_t)i + 1] = u1; }
    depths[i] = depth;
    if (visible) visible[i] = depth > 0.2f;  // the mask GSFunction returns (gsmodel.py:50)
    if (cinv2ds) st3(cinv2ds + 3 * (size_t)i, {ci[0], ci[1], ci[2]});
    if (areas) { areas[2 * (size_t)i] = rx; areas[2 * (size_t)i + 1] = ry; }
    // the packed 2D record of the draw kernels, straight from registers (no k_pack_records pass): its geometry fields
    if (rec)
      make_record(u0, u1, ci[0], ci[1], ci[2], alpha_act, 0.f, 0.f, 0.f, rx, ry,
                  pp.W, pp.H, pp.footprint, pp.alpha_skip, r);
    // ---- the SH row is waited for here.  Colour has no depth test in the reference (kernel.cu:619-725)
    float col[3];
    sh_color_f<NC>(d, sh, col);
    if (colors) st3(colors + 3 * (size_t)i, {col[0], col[1], col[2]});
    if constexpr (JW) sh_jac_dpw<NC>(d, sh, jw);
    if (rec) { r[1].z = col[0]; r[1].w = col[1]; r[2].x = col[2]; }
  }
  if (bo.br) {
    __syncthreads();   // (RAW: every wave is done with the rows staged in)
    block_max_key(dkey, bo.maxkey, reinterpret_cast<uint32_t*>(stage));
    if (i < n) bo.cr[i] = crec;     // (16 B per lane, consecutive lanes: full lines)
  }
  // 48-B records leave as full lines (lane-strided 16-B pieces cost 3x the write requests)
  if (rec) rows_out<12>(reinterpret_cast<const float*>(r), reinterpret_cast<float*>(rec), n, blockIdx.x * 256, stage);
  if constexpr (JW) rows_out<9>(jw, dcolor_dpws, n, blockIdx.x * 256, stage);
}

// backward.md eq (3)(4)(5)(7) == gsmodel.py:71-85 with every Jacobian re-derived in
// registers from the parameters.  gpack = the packed per-Gaussian gradient records
// written by k_draw_bwd: {dalpha, dcolor[3], du[2], dcinv[3], pad[3]}.
// RAW: parameters as in k_preprocess_fwd<.., true>; gradients come out with respect to the raw tensors
// (dL_dsh = low_shs [N,3], dL_dsh_high = high_shs [N,K-3]); alphas = alphas_raw (only read when RAW)
// EXTRA (render extras): gpack[i][9] holds dL/dz of the Gaussian's camera-space depth
// POSE (camera pose gradient): every other output as without it, plus one partial row {dL/dRcw [9],
// dL/dtcw [3], dL/dtwc [3], 0} per workgroup in pose_ws (read by the POSE instances only), summed by k_pose_reduce
// AA (anti-aliased rendering): the records were drawn with opacity alpha comp; reads alphas[i] also
// without RAW (4 B per Gaussian)
// POSE_ONLY (with POSE; EGS_BWD_POSE_ONLY): the partial row in pose_ws is the ONLY output -- the same 15 per-lane
// terms and the same reduction as the POSE instance, but no old gradients, no cov3d_vjp, no J3 product, no gsh rows, and
// the seven dL_d* pointers (NULL or not) are never dereferenced; `mode` is ignored.  With JW the SH rows are never
// touched; without it they are still read (W needs them)
template <int NC, bool RAW, bool JW, bool EXTRA, bool POSE, bool AA, bool POSE_ONLY>
__global__ __launch_bounds__(256) void k_preprocess_bwd(
    int n, PreParams pp, const float* __restrict__ pws, const float* __restrict__ rots,
    const float* __restrict__ scales, const float* __restrict__ shs, const float* __restrict__ shs_high,
    const float* __restrict__ alphas, const float* __restrict__ Rcw,
    const float* __restrict__ tcw, const float* __restrict__ twc, const float* __restrict__ depths,
    const float4* __restrict__ gpack, float* __restrict__ dL_dpw, float* __restrict__ dL_dsh,
    float* __restrict__ dL_dsh_high, float* __restrict__ dL_dalpha, float* __restrict__ dL_dscale, float* __restrict__ dL_drot,
    float* __restrict__ dL_du, const float* __restrict__ dcolor_dpws, int mode, float* __restrict__ pose_ws) {
  // AA (anti-aliased rendering): the forward drew opacity alpha comp, so ga.x = dL/d(alpha comp):
  // dL/dalpha = ga.x comp and dL/dcov2d gains ga.x alpha dcomp/dcov2d before it feeds J3, Jp and the pose W term
  // dcolor_dpws (nullable): [N][9] left by k_preprocess_fwd; with it this kernel never reads the SH coefficients
  // mode bit 1 (EGS_BWD_FACTORED_SH): the SH gradient stays in its factored form -- eq (5) is an outer product
  // dL/dcolour (x) basis, so dL_dsh receives the THREE floats dL/dcolour per Gaussian ([N][3], always written, never
  // accumulated) and the rows are formed once per step, for all views, by k_sh_grad_views; dL_dsh_high is not touched
  static_assert(POSE || !POSE_ONLY, "POSE_ONLY is a flavour of the POSE instances");
  const int accum = POSE_ONLY ? 0 : (mode & 1);
  const bool factored = !POSE_ONLY && (mode & 2) != 0;
  // accum: the five (six) parameter-gradient outputs already hold the gradients of EARLIER views of the step and this
  // view's are ADDED to them (dL_du is per view and always written): a rank that renders V views per step then needs
  // no separate accumulation kernels (torch's `.grad += new`: 976 B per Gaussian and view against 488 here)
  constexpr int K = 3 * NC;
  constexpr int KH = K - 3;
  constexpr int KS = RAW ? (KH > 0 ? KH : 1) : K;   // width of the rows that go through LDS
  __shared__ float stage[RowStage<KS>::LDS_FLOATS];
  const int i = blockIdx.x * 256 + threadIdx.x;
  float sh[JW ? 1 : K], gsh[POSE_ONLY ? 1 : K];
  if constexpr (!JW) {
    if constexpr (RAW) {
      if constexpr (KH > 0) rows_in<KH>(shs_high, n, blockIdx.x * 256, stage, sh + 3);
      if (i < n) { sh[0] = shs[3 * (size_t)i]; sh[1] = shs[3 * (size_t)i + 1]; sh[2] = shs[3 * (size_t)i + 2]; }
    } else if (i < n) {   // (direct row loads: rows_in measured 10 % slower, reads do not pay for partial lines)
      load_row<K>(shs + (size_t)K * i, sh);
    }
  }
  // (Tried: the gsh rows formed and staged out right after the loads, the Jacobians and cov3d_vjp behind them, so that
  // the rows' 192 B per Gaussian drain under the arithmetic -- 63 -> 66 us: the stage's barriers then stand between
  // the loads and ALL of the arithmetic, and stores issued last never held a wave anyway; docs/LAB.md.)
  if constexpr (!POSE_ONLY) {
#pragma unroll
    for (int k = 0; k < K; ++k) gsh[k] = 0.f;
  }
  f3 gcol_out = {0.f, 0.f, 0.f};
  // POSE: this lane's share of the camera gradient, {dL/dRcw [3][3], dL/dtcw [3], dL/dtwc [3]}
  float pg[POSE ? 15 : 1];
  if constexpr (POSE) {
#pragma unroll
    for (int k = 0; k < 15; ++k) pg[k] = 0.f;
  }
  if (i < n) {
    // Every input of the row is requested here, before anything is used: with the parameter loads behind the depth
    // test, the Jacobian row at its use and the old gradients (accum) at theirs, a row went through four dependent
    // round trips to memory (the ISA had a full wait after each group).
    const float4 ga = gpack[3 * (size_t)i], gb = gpack[3 * (size_t)i + 1], gc = gpack[3 * (size_t)i + 2];
    const float depth_i = depths[i];
    const f3 pw = ld3(pws + 3 * (size_t)i);
    float4 q = *reinterpret_cast<const float4*>(rots + 4 * (size_t)i);
    f3 s = ld3(scales + 3 * (size_t)i);
    float W[9];
    if constexpr (JW) load_row<9>(dcolor_dpws + 9 * (size_t)i, W);
    float al_raw = 0.f;   // (AA without RAW: the activated alpha)
    if constexpr ((RAW && !POSE_ONLY) || AA) al_raw = alphas[i];
    float4 o_rot = make_float4(0.f, 0.f, 0.f, 0.f);
    f3 o_scale = {0.f, 0.f, 0.f}, o_pw = {0.f, 0.f, 0.f};
    float o_alpha = 0.f;
    if (!POSE_ONLY && accum) {
      o_rot = *reinterpret_cast<const float4*>(dL_drot + 4 * (size_t)i);
      o_scale = ld3(dL_dscale + 3 * (size_t)i);
      o_pw = ld3(dL_dpw + 3 * (size_t)i);
      o_alpha = dL_dalpha[i];
    }
    const f3 gcol = {ga.y, ga.z, ga.w};
    const float gu0 = gb.x, gu1 = gb.y;
    const f3 gci = {gb.z, gb.w, gc.x};
    if constexpr (AA || POSE_ONLY) {
      // (AA: stored below, once comp is known; culled: comp = 0)
    } else if constexpr (RAW) {
      const float al = act_alpha(al_raw);
      dL_dalpha[i] = ga.x * al * (1.f - al) + o_alpha;   // sigmoid'
    } else {
      dL_dalpha[i] = ga.x + o_alpha;
    }
    if constexpr (!POSE_ONLY) { dL_du[2 * (size_t)i] = gu0; dL_du[2 * (size_t)i + 1] = gu1; }
    if (pp.near_cull && depth_i < EGS_MIN_DEPTH) {  // culled: never drawn, all gradients are zero
      // (without AA the store above has already put ga.x there: records handed in by a phase-2 caller need not be zero)
      if constexpr (!POSE_ONLY) dL_dalpha[i] = o_alpha;
      if (!POSE_ONLY && !accum) {   // (POSE_ONLY: pg stays zero, nothing else to write)
        st3(dL_dpw + 3 * (size_t)i, {0.f, 0.f, 0.f});
        st3(dL_dscale + 3 * (size_t)i, {0.f, 0.f, 0.f});
        st4(dL_drot + 4 * (size_t)i, {0.f, 0.f, 0.f, 0.f});
      }
    } else {
      float qnorm = 1.f;
      if constexpr (RAW) { q = act_rot(q, qnorm); s = act_scale(s); }
      const Proj P = project_f(pw, Rcw, tcw, pp.fx, pp.fy, pp.cx, pp.cy);
      const Cov3 c3 = cov3d_f(q, s);
      const Cov2 c2 = cov2d_f(c3.c, P.pc, Rcw, pp.fx, pp.fy, pp.limx, pp.limy, pp.clamp_fov);
      float ci[3];
      const float det_inv = inv_cov2d_f(c2.c, pp.det_eps, ci);
      float Ji[9];
      inv_cov2d_jac(c2.c, det_inv, Ji);
      // dL/dcov2d = dL/dcinv2d @ J  (row vector times 3x3)
      float g2[3] = {gci.x * Ji[0] + gci.y * Ji[3] + gci.z * Ji[6],
                     gci.x * Ji[1] + gci.y * Ji[4] + gci.z * Ji[7],
                     gci.x * Ji[2] + gci.y * Ji[5] + gci.z * Ji[8]};
      if constexpr (AA) {
        const float al = RAW ? act_alpha(al_raw) : al_raw;
        const float comp = aa_comp_vjp(c2.c, ga.x * al, g2);   // g2 += ga.x alpha dcomp/dcov2d
        if constexpr (!POSE_ONLY) {
          const float gal = ga.x * comp;
          dL_dalpha[i] = (RAW ? gal * al * (1.f - al) : gal) + o_alpha;
        }
      }
      float J3[18], Jp[9];
      cov2d_jac(c2, P.pc.z, Rcw, pp.fx, pp.fy, J3, Jp);
      if constexpr (!POSE_ONLY) {   // (POSE_ONLY: only Jp of the line above is used, J3 is dead code)
        float g3[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) g3[k] = g2[0] * J3[k] + g2[1] * J3[6 + k] + g2[2] * J3[12 + k];
        q4 gq; f3 gs;
        cov3d_vjp(c3, q, s, g3, gq, gs);
        if constexpr (RAW) {   // through normalize: (g - q (q.g)) / |r|; through exp: g * scale
          const float qg = q.x * gq.w + q.y * gq.x + q.z * gq.y + q.w * gq.z;
          gq = {(gq.w - q.x * qg) / qnorm, (gq.x - q.y * qg) / qnorm, (gq.y - q.z * qg) / qnorm,
                (gq.z - q.w * qg) / qnorm};
          gs = {gs.x * s.x, gs.y * s.y, gs.z * s.z};
        }
        if (accum) {
          gq = {gq.w + o_rot.x, gq.x + o_rot.y, gq.y + o_rot.z, gq.z + o_rot.w};
          gs = {gs.x + o_scale.x, gs.y + o_scale.y, gs.z + o_scale.z};
        }
        st4(dL_drot + 4 * (size_t)i, gq);      // eq (3)
        st3(dL_dscale + 3 * (size_t)i, gs);    // eq (4)
      }
      float j00, j02, j11, j12;
      project_jac(P, pp.fx, pp.fy, j00, j02, j11, j12);
      f3 gpc = {gu0 * j00 + g2[0] * Jp[0] + g2[1] * Jp[3] + g2[2] * Jp[6],
                gu1 * j11 + g2[0] * Jp[1] + g2[1] * Jp[4] + g2[2] * Jp[7],
                gu0 * j02 + gu1 * j12 + g2[0] * Jp[2] + g2[1] * Jp[5] + g2[2] * Jp[8]};
      // render extras: depth blends z = (Rcw pw + tcw).z, so its gradient dz (gpack[i][9]) joins dL/dpc.z
      if constexpr (EXTRA) gpc.z += gc.y;
      const ShDir<NC> d = sh_basis_f<NC>(pw, twc);
      // eq (5): dL/dsh[c, rgb] = dL/dcolor[rgb] * basis[c]
      gcol_out = gcol;
      if constexpr (!POSE_ONLY) {
        if (!factored) {
#pragma unroll
          for (int c = 0; c < NC; ++c) {
            gsh[3 * c] = gcol.x * d.B[c]; gsh[3 * c + 1] = gcol.y * d.B[c]; gsh[3 * c + 2] = gcol.z * d.B[c];
          }
        }
      }
      if constexpr (!JW) sh_jac_dpw<NC>(d, sh, W);   // (POSE_ONLY with JW: the basis d is never used)
      if constexpr (!POSE_ONLY) {
        float* opw = dL_dpw + 3 * (size_t)i;  // eq (7)
        const float opw_old[3] = {o_pw.x, o_pw.y, o_pw.z};
#pragma unroll
        for (int k = 0; k < 3; ++k)
          opw[k] = gpc.x * Rcw[k] + gpc.y * Rcw[3 + k] + gpc.z * Rcw[6 + k] + gcol.x * W[k] + gcol.y * W[3 + k] +
                   gcol.z * W[6 + k] + opw_old[k];
      }
      if constexpr (POSE) {
        // p_c = Rcw pw + tcw: dL/dtcw += gpc, dL/dRcw += gpc pw^T (projection, J(p_c) of cov2d, depth)
        const float gp[3] = {gpc.x, gpc.y, gpc.z}, pwv[3] = {pw.x, pw.y, pw.z};
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          pg[9 + r] = gp[r];
#pragma unroll
          for (int k = 0; k < 3; ++k) pg[3 * r + k] = gp[r] * pwv[k];
        }
        // the W = Rcw factor of cov2d = (J W) Sigma (J W)^T with J held (clamped x/z, y/z as cov2d_f):
        // dL/dM0 = 2 g2[0] v0 + g2[1] v1, dL/dM1 = g2[1] v0 + 2 g2[2] v1;  dL/dRcw += J0^T dL/dM0 + J1^T dL/dM1
        const f3 gM0 = (2.f * g2[0]) * c2.v0 + g2[1] * c2.v1;
        const f3 gM1 = g2[1] * c2.v0 + (2.f * g2[2]) * c2.v1;
        const float z = P.pc.z, z2 = z * z;
        const float a00 = pp.fx / z, a02 = -(pp.fx * c2.x) / z2, a11 = pp.fy / z, a12 = -(pp.fy * c2.y) / z2;
        pg[0] += a00 * gM0.x; pg[1] += a00 * gM0.y; pg[2] += a00 * gM0.z;
        pg[3] += a11 * gM1.x; pg[4] += a11 * gM1.y; pg[5] += a11 * gM1.z;
        pg[6] += a02 * gM0.x + a12 * gM1.x; pg[7] += a02 * gM0.y + a12 * gM1.y; pg[8] += a02 * gM0.z + a12 * gM1.z;
        // the SH colour sees pw - twc: dL/dtwc = -gcol^T dcolor/dpw
#pragma unroll
        for (int k = 0; k < 3; ++k) pg[12 + k] = -(gcol.x * W[k] + gcol.y * W[3 + k] + gcol.z * W[6 + k]);
      }
    }
  }
  if constexpr (POSE) {
    // one partial row of 16 floats per workgroup: a fixed butterfly across the wave64, the 4 waves in order through
    // LDS.  No atomics -- k_pose_reduce sums the rows in a fixed order, so the result is bitwise reproducible.
    __shared__ float pose_part[4][16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 15; ++k) {
      float v = pg[k];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
      if (lane == 0) pose_part[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < 16)
      pose_ws[16 * (size_t)blockIdx.x + threadIdx.x] =
          threadIdx.x < 15 ? ((pose_part[0][threadIdx.x] + pose_part[1][threadIdx.x]) + pose_part[2][threadIdx.x]) +
                                 pose_part[3][threadIdx.x]
                           : 0.f;
  }
  if constexpr (POSE_ONLY) return;   // the partial row above is the instance's only output
  if (factored) {   // (a kernel argument: the whole workgroup leaves here)
    if (i < n) st3(dL_dsh + 3 * (size_t)i, gcol_out);
    // the view's camera centre behind the [N][3] block: the row format of egs_sh_grad_views (dL_dsh_high = its address)
    if (dL_dsh_high && blockIdx.x == 0 && threadIdx.x < 3) dL_dsh_high[threadIdx.x] = twc[threadIdx.x];
    return;
  }
  sh_grad_rows_out<NC, RAW>(gsh, dL_dsh, dL_dsh_high, n, blockIdx.x * 256, stage, accum != 0);
}

// The camera pose gradient from the partial rows of k_preprocess_bwd<.., POSE>: ONE workgroup of 1024 threads, thread t sums
// column t % 16 of rows t / 16, t / 16 + 64, ... in double (eight loads in flight, added in row order), the 64 partial
// sums of a column are added in index order, then the camera centre twc = -Rcw^T tcw is folded back:
// dL/dRcw[r][k] -= tcw[r] dL/dtwc[k],  dL/dtcw -= Rcw dL/dtwc.  Every sum has a fixed order: identical partial rows
// give identical bits.
__global__ __launch_bounds__(1024) void k_pose_reduce(int rows, const float* __restrict__ pose_ws,
                                                      const float* __restrict__ Rcw, const float* __restrict__ tcw,
                                                      float* __restrict__ dL_dRcw, float* __restrict__ dL_dtcw) {
  __shared__ double part[64][17];
  __shared__ double g[16];
  const int t = threadIdx.x, col = t & 15;
  double acc = 0.0;
  int r = t >> 4;
  for (; r + 7 * 64 < rows; r += 8 * 64) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = pose_ws[16 * (size_t)(r + 64 * j) + col];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc += (double)v[j];
  }
  for (; r < rows; r += 64) acc += (double)pose_ws[16 * (size_t)r + col];
  part[t >> 4][col] = acc;
  __syncthreads();
  if (t < 16) {
    double v = 0.0;
    for (int j = 0; j < 64; ++j) v += part[j][t];
    g[t] = v;
  }
  __syncthreads();
  if (t == 0) {
    const double* gt = g + 12;   // dL/dtwc
    for (int i = 0; i < 3; ++i) {
      for (int k = 0; k < 3; ++k) dL_dRcw[3 * i + k] = (float)(g[3 * i + k] - (double)tcw[i] * gt[k]);
      dL_dtcw[i] = (float)(g[9 + i] - ((double)Rcw[3 * i] * gt[0] + (double)Rcw[3 * i + 1] * gt[1] +
                                       (double)Rcw[3 * i + 2] * gt[2]));
    }
  }
}

// The SH gradient of a step from its FACTORED form (dist_views.FactoredShGrad).  For one view dL/dsh[c][rgb] is the
// outer product dL/dcolour[rgb] * basis_c(pw - camera centre) -- eq (5), gsmodel.py:84-85 -- so the views of a step
// (this rank's and, all-gathered, every other rank's) travel as 3 floats per Gaussian and view instead of 48 per
// Gaussian and rank, and this kernel forms  scale * sum_v dcolour_v (x) basis(pw - twc_v)  once.
// rows: [views][stride] floats, row v = {dL/dcolour [N][3], twc[3], padding}.  Outputs as k_preprocess_bwd's.
template <int NC, bool RAW>
__global__ __launch_bounds__(256) void k_sh_grad_views(int n, int views, const float* __restrict__ pws,
                                                       const float* __restrict__ rows, int64_t stride, float scale,
                                                       float* __restrict__ dL_dsh, float* __restrict__ dL_dsh_high,
                                                       int accum) {
  constexpr int K = 3 * NC;
  constexpr int KH = K - 3;
  constexpr int KS = RAW ? (KH > 0 ? KH : 1) : K;
  __shared__ float stage[RowStage<KS>::LDS_FLOATS];
  const int i = blockIdx.x * 256 + threadIdx.x;
  float gsh[K];
#pragma unroll
  for (int k = 0; k < K; ++k) gsh[k] = 0.f;
  if (i < n) sh_grad_row<NC>(ld3(pws + 3 * (size_t)i), rows, stride, views, n, i, scale, gsh);
  sh_grad_rows_out<NC, RAW>(gsh, dL_dsh, dL_dsh_high, n, blockIdx.x * 256, stage, accum != 0);
}

}  // namespace egs

// ============================================================================
// C ABI
// ============================================================================
using namespace egs;

static void fov_limits(const EgsPolicy* pol, float fx, float fy, float width, float height, float* limx,
                       float* limy) {
  *limx = 0.f; *limy = 0.f;
  if (pol->fov_mode == 0) {  // gausplat.cu:225-226
    *limx = 1.3f * (width / (2 * fx));
    *limy = 1.3f * (height / (2 * fy));
  } else if (pol->fov_mode == 1) {  // gausplat.py:136-140 (an angle, misnamed tan there)
    *limx = (float)(1.3 * (2 * atan((double)width / (2 * (double)fx))));
    *limy = (float)(1.3 * (2 * atan((double)height / (2 * (double)fy))));
  }
}

extern "C" int egs_project(int n, const float* pws, const float* Rcw, const float* tcw, float fx, float fy,
                           float cx, float cy, const EgsPolicy* pol, float* us, float* pcs, float* depths,
                           float* du_dpcs, void* stream) {
  EGS_CHECK_ARG(n >= 0 && pol);
  if (n == 0) return 0;
  EGS_CHECK_ARG(pws && Rcw && tcw && us && pcs && depths);
  EGS_CHECK_ARG((((uintptr_t)us | (uintptr_t)du_dpcs) & 7) == 0);
  EGS_LAUNCH("k_project", k_project, dim3(div_up(n, 256)), dim3(256), (hipStream_t)stream, n, pws, Rcw, tcw, fx,
                     fy, cx, cy, pol->near_cull, us, pcs, depths, du_dpcs);
  EGS_LAUNCH_OK();
  return 0;
}

extern "C" int egs_cov3d(int n, const float* rots, const float* scales, const float* depths,
                         const EgsPolicy* pol, float* cov3ds, float* dcov3d_drots, float* dcov3d_dscales,
                         void* stream) {
  EGS_CHECK_ARG(n >= 0 && pol);
  if (n == 0) return 0;
  EGS_CHECK_ARG(rots && scales && depths && cov3ds);
  EGS_CHECK_ARG((dcov3d_drots == nullptr) == (dcov3d_dscales == nullptr));
  EGS_CHECK_ARG(((uintptr_t)rots & 15) == 0);
  EGS_CHECK_ARG((((uintptr_t)cov3ds | (uintptr_t)dcov3d_drots | (uintptr_t)dcov3d_dscales) & 15) == 0);
  EGS_LAUNCH("k_cov3d", k_cov3d, dim3(div_up(n, 256)), dim3(256), (hipStream_t)stream, n, rots, scales, depths,
                     pol->near_cull, cov3ds, dcov3d_drots, dcov3d_dscales);
  EGS_LAUNCH_OK();
  return 0;
}

extern "C" int egs_cov2d(int n, const float* cov3ds, const float* pcs, const float* Rcw, const float* depths,
                         float fx, float fy, float width, float height, const EgsPolicy* pol, float* cov2ds,
                         float* dcov2d_dcov3ds, float* dcov2d_dpcs, void* stream) {
  EGS_CHECK_ARG(n >= 0 && pol);
  if (n == 0) return 0;
  EGS_CHECK_ARG(cov3ds && pcs && Rcw && depths && cov2ds);
  EGS_CHECK_ARG((dcov2d_dcov3ds == nullptr) == (dcov2d_dpcs == nullptr));
  EGS_CHECK_ARG((((uintptr_t)cov3ds & 7) | (((uintptr_t)cov2ds | (uintptr_t)dcov2d_dcov3ds | (uintptr_t)dcov2d_dpcs) & 15)) == 0);
  float limx, limy;
  fov_limits(pol, fx, fy, width, height, &limx, &limy);
  EGS_LAUNCH("k_cov2d", k_cov2d, dim3(div_up(n, 256)), dim3(256), (hipStream_t)stream, n, cov3ds, pcs, Rcw,
                     depths, fx, fy, limx, limy, pol->fov_mode != 2, pol->near_cull, cov2ds, dcov2d_dcov3ds,
                     dcov2d_dpcs);
  EGS_LAUNCH_OK();
  return 0;
}

extern "C" int egs_sh2color(int n, int sh_dim, const float* shs, const float* pws, const float* twc,
                            float* colors, float* dcolor_dshs, float* dcolor_dpws, void* stream) {
  EGS_CHECK_ARG(n >= 0);
  EGS_CHECK_ARG(sh_dim == 3 || sh_dim == 12 || sh_dim == 27 || sh_dim == 48);
  if (n == 0) return 0;
  EGS_CHECK_ARG(shs && pws && twc && colors);
  EGS_CHECK_ARG((dcolor_dshs == nullptr) == (dcolor_dpws == nullptr));
  EGS_CHECK_ARG(sh_dim % 4 != 0 || ((uintptr_t)shs & 15) == 0);
  EGS_CHECK_ARG((((uintptr_t)colors | (uintptr_t)dcolor_dshs | (uintptr_t)dcolor_dpws) & 15) == 0);
  dim3 g(div_up(n, 256)), b(256);
  hipStream_t s = (hipStream_t)stream;
  decltype(&k_sh2color<1>) kern = nullptr;
  with_sh_dim(sh_dim, [&](auto nc) { kern = k_sh2color<nc.value>; });
  EGS_LAUNCH("k_sh2color", kern, g, b, s, n, shs, pws, twc, colors, dcolor_dshs, dcolor_dpws);
  EGS_LAUNCH_OK();
  return 0;
}

extern "C" int egs_inv_cov2d(int n, const float* cov2ds, float* depths, const EgsPolicy* pol, float* cinv2ds,
                             int32_t* areas, float* dcinv2d_dcov2ds, void* stream) {
  EGS_CHECK_ARG(n >= 0 && pol);
  if (n == 0) return 0;
  EGS_CHECK_ARG(cov2ds && depths && cinv2ds && areas);
  EGS_CHECK_ARG((((uintptr_t)cinv2ds | (uintptr_t)areas | (uintptr_t)dcinv2d_dcov2ds) & 15) == 0);
  EGS_LAUNCH("k_inv_cov2d", k_inv_cov2d, dim3(div_up(n, 256)), dim3(256), (hipStream_t)stream, n, cov2ds, depths,
                     pol->det_eps, pol->near_cull, pol->nan_cull, pol->radius_mode, cinv2ds, areas,
                     dcinv2d_dcov2ds);
  EGS_LAUNCH_OK();
  return 0;
}

extern "C" int egs_chain_rule(int n, int sh_dim, const float* dloss_dus, const float* dloss_dcinv2ds,
                              const float* dloss_dcolors, const float* Rcw, const float* dcinv2d_dcov2ds,
                              const float* dcov2d_dcov3ds, const float* dcov3d_drots,
                              const float* dcov3d_dscales, const float* dcolor_dshs, const float* du_dpcs,
                              const float* dcov2d_dpcs, const float* dcolor_dpws, float* dloss_dpws,
                              float* dloss_dshs, float* dloss_dscales, float* dloss_drots, void* stream) {
  EGS_CHECK_ARG(n >= 0);
  EGS_CHECK_ARG(sh_dim == 3 || sh_dim == 12 || sh_dim == 27 || sh_dim == 48);
  if (n == 0) return 0;
  EGS_CHECK_ARG(dloss_dus && dloss_dcinv2ds && dloss_dcolors && Rcw && dcinv2d_dcov2ds && dcov2d_dcov3ds &&
                dcov3d_drots && dcov3d_dscales && dcolor_dshs && du_dpcs && dcov2d_dpcs && dcolor_dpws &&
                dloss_dpws && dloss_dshs && dloss_dscales && dloss_drots);
  EGS_CHECK_ARG((((uintptr_t)dloss_dpws | (uintptr_t)dloss_dshs | (uintptr_t)dloss_dscales | (uintptr_t)dloss_drots |
                  (uintptr_t)dcov3d_drots | (sh_dim % 12 == 0 ? (uintptr_t)dcolor_dshs : 0)) & 15) == 0);
  EGS_CHECK_ARG((((uintptr_t)dloss_dus | (uintptr_t)dcov2d_dcov3ds | (uintptr_t)dcov3d_dscales | (uintptr_t)du_dpcs) & 7) == 0);
  dim3 g(div_up(n, 256)), b(256);
  hipStream_t s = (hipStream_t)stream;
  decltype(&k_chain_rule<1>) kern = nullptr;
  with_sh_dim(sh_dim, [&](auto nc) { kern = k_chain_rule<nc.value>; });
  EGS_LAUNCH("k_chain_rule", kern, g, b, s, n, dloss_dus, dloss_dcinv2ds, dloss_dcolors, Rcw, dcinv2d_dcov2ds,
             dcov2d_dcov3ds, dcov3d_drots, dcov3d_dscales, dcolor_dshs, du_dpcs, dcov2d_dpcs, dcolor_dpws, dloss_dpws,
             dloss_dshs, dloss_dscales, dloss_drots);
  EGS_LAUNCH_OK();
  return 0;
}

static PreParams make_pre_params(const EgsPolicy* pol, float fx, float fy, float cx, float cy, int width,
                                 int height) {
  PreParams pp;
  pp.fx = fx; pp.fy = fy; pp.cx = cx; pp.cy = cy;
  fov_limits(pol, fx, fy, (float)width, (float)height, &pp.limx, &pp.limy);
  pp.det_eps = pol->det_eps; pp.alpha_skip = pol->alpha_skip;
  pp.footprint = pol->footprint; pp.W = width; pp.H = height;
  pp.clamp_fov = pol->fov_mode != 2; pp.near_cull = pol->near_cull; pp.nan_cull = pol->nan_cull;
  pp.radius_mode = pol->radius_mode;
  return pp;
}

extern "C" int egs_fused_forward(int n, int sh_dim, const float* pws, const float* rots, const float* scales,
                                 const float* shs, const float* shs_high, const float* alphas, const float* Rcw,
                                 const float* tcw, const float* twc, float fx, float fy, float cx, float cy, int width,
                                 int height, const EgsPolicy* pol, float* us, float* depths, float* cinv2ds,
                                 float* colors, int32_t* areas, void* rec, uint8_t* visible, float* dcolor_dpws,
                                 int flags, int key_bits_hint, void* ws_bin, size_t ws_bin_bytes,
                                 uint32_t* total_patches, uint32_t* host_totals, void* stream) {
  EGS_CHECK_ARG((flags & ~(EGS_FUSED_CULLED_LISTS | EGS_FUSED_ANTIALIASED | EGS_FUSED_RAW)) == 0);
  const bool cull_lists = (flags & EGS_FUSED_CULLED_LISTS) != 0;
  const bool aa = (flags & EGS_FUSED_ANTIALIASED) != 0;
  const bool raw = (flags & EGS_FUSED_RAW) != 0;
  EGS_CHECK_ARG(!aa || rec);   // the compensated opacity only exists inside the records
  EGS_CHECK_ARG(!raw || n == 0 || (rec && alphas));   // so does the activated alpha
  EGS_CHECK_ARG(raw || !shs_high);
  EGS_CHECK_ARG(n >= 0 && pol && width > 0 && height > 0 && total_patches);
  EGS_CHECK_ARG(!cull_lists || (rec && n < (1 << EGS_GSID_BITS)));   // culled lists are drawn from the records only
  EGS_CHECK_ARG(((uintptr_t)dcolor_dpws & 15) == 0);
  EGS_CHECK_ARG(width < 32768 && height < 32768);
  EGS_CHECK_ARG(sh_dim == 3 || sh_dim == 12 || sh_dim == 27 || sh_dim == 48);
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) {
    EGS_HIP(hipMemsetAsync(total_patches, 0, 8, s));
    if (host_totals) EGS_HIP(hipMemcpyAsync(host_totals, total_patches, 8, hipMemcpyDeviceToHost, s));
    return 0;
  }
  EGS_CHECK_ARG(pws && rots && scales && shs && Rcw && tcw && twc && depths);
  EGS_CHECK_ARG(rec || (us && cinv2ds && colors && areas));   // something must carry the 2D Gaussians on
  EGS_CHECK_ARG(!rec || alphas);
  EGS_CHECK_ARG(ws_bin);
  EGS_CHECK_ARG(((uintptr_t)rots & 15) == 0);
  if (raw) EGS_CHECK_ARG(sh_dim == 3 || (shs_high && ((uintptr_t)shs_high & 15) == 0));
  else EGS_CHECK_ARG(sh_dim % 4 != 0 || ((uintptr_t)shs & 15) == 0);
  BinCountOut bo;
  if (!bin_count_outputs(ws_bin, ws_bin_bytes, n, &bo)) {
    set_error(EGS_ERR_WORKSPACE, "bin workspace too small", __FILE__, __LINE__);
    return EGS_ERR_WORKSPACE;
  }
  const BinParams bp = make_bin_params(width, height, pol, cull_lists);
  const PreParams pp = make_pre_params(pol, fx, fy, cx, cy, width, height);
  dim3 g(div_up(n, 256)), b(256);
  // (tried: dynamic LDS to cap the resident workgroups per CU of this kernel at 4, 3, 2 -- no faster, docs/LAB.md)
  decltype(&k_preprocess_fwd<1, false, false, false>) kern = nullptr;   // flags -> template arguments
  with_sh_dim(sh_dim, [&](auto nc) {
    with_bools([&](auto raw_c, auto jw, auto aa_c) { kern = k_preprocess_fwd<nc.value, raw_c.value, jw.value, aa_c.value>; },
               raw, dcolor_dpws != nullptr, aa);
  });
  EGS_LAUNCH(aa ? "k_preprocess_fwd_aa" : "k_preprocess_fwd", kern, g, b, s, n, pp, pws, rots, scales, shs, shs_high,
             alphas, Rcw, tcw, twc, us, depths, cinv2ds, colors, areas, (float4*)rec, bp, bo, visible, dcolor_dpws);
  EGS_LAUNCH_OK();
  // the kernel above already did getRects + depth keys (k_bin_count of egs_splat_bin)
  return splat_bin_after_count(n, key_bits_hint, ws_bin, ws_bin_bytes, total_patches, stream, host_totals);
}

extern "C" size_t egs_fused_backward_ws_bytes(int n) { return egs_splat_bwd_ws_bytes(n); }

// one partial row of 16 floats per 256-Gaussian workgroup of k_preprocess_bwd<.., POSE>
extern "C" size_t egs_pose_ws_bytes(int n) { return align_up((size_t)div_up(n > 0 ? n : 1, 256) * 16 * sizeof(float), 256); }

extern "C" int egs_fused_backward(int n, int sh_dim, int64_t patches, int width, int height, const float* pws,
                                  const float* rots, const float* scales, const float* shs, const float* shs_high,
                                  const float* alphas, const float* Rcw, const float* tcw, const float* twc, float fx,
                                  float fy, float cx, float cy, const EgsPolicy* pol, const float* us,
                                  const float* cinv2ds, const float* colors, const int32_t* areas, const void* rec,
                                  const float* depths, const int32_t* contrib, const float* final_tau,
                                  const int32_t* patch_range_per_tile, const int32_t* gsid_per_patch,
                                  const float* dloss_dgammas, void* ws, size_t ws_bytes, float* dloss_dpws,
                                  float* dloss_dshs, float* dloss_dshs_high, float* dloss_dalphas,
                                  float* dloss_dscales, float* dloss_drots, float* dloss_dus,
                                  const int32_t* tile_order, float* grad_records, const float* dcolor_dpws, int phase,
                                  int row_begin, int row_count, void* seg_ws, size_t seg_ws_bytes, void* stream,
                                  const EgsExtras* extras, const EgsPoseGrad* pose) {
  // extras (nullable): the render had depth / opacity / background (egs_splat_draw_rec_seg with extras); the draw pass
  // takes their upstream gradients and leaves dL/dz in gpack[i][9], the chain rule adds it to dL/dpw
  // (k_preprocess_bwd<.., EXTRA>)
  // phase 0: everything; 1: only the draw pass (-> packed gradient records in ws); 2: only the per-Gaussian
  // chain rule, for rows [row_begin, row_begin + row_count) -- a data-parallel caller launches the rows in a
  // few chunks and starts exchanging a chunk's gradients while the next one is computed (dist_views)
  EGS_CHECK_ARG(n >= 0 && pol && width > 0 && height > 0 && patches >= 0);
  const bool keep_order = (phase & EGS_BWD_KEEP_FORWARD_ORDER) != 0;
  const bool masked = (phase & EGS_FUSED_CULLED_LISTS) != 0;
  // kernel `mode`: bit 0 accumulate, bit 1 factored SH gradient (dloss_dshs = dL/dcolour [N][3])
  const int accum = ((phase & EGS_BWD_ACCUMULATE) ? 1 : 0) | ((phase & EGS_BWD_FACTORED_SH) ? 2 : 0);
  const bool factored = (phase & EGS_BWD_FACTORED_SH) != 0;
  // the render was anti-aliased: the chain rule takes the AA instances
  const bool aa = (phase & EGS_FUSED_ANTIALIASED) != 0;
  const bool raw = (phase & EGS_FUSED_RAW) != 0;
  // the draw pass also sums |dL/du| per pixel into the records' slots 10 and 11 (the ABS instances of k_draw_bwd)
  const bool absgrad = (phase & EGS_BWD_ABSGRAD) != 0;
  // only the camera gradient is wanted: the chain rule takes the POSE_ONLY instances, the seven per-Gaussian outputs
  // may be NULL and are never written
  const bool pose_only = (phase & EGS_BWD_POSE_ONLY) != 0;
  phase &= ~(EGS_BWD_KEEP_FORWARD_ORDER | EGS_BWD_ACCUMULATE | EGS_BWD_FACTORED_SH | EGS_FUSED_CULLED_LISTS |
             EGS_FUSED_ANTIALIASED | EGS_FUSED_RAW | EGS_BWD_ABSGRAD | EGS_BWD_POSE_ONLY);
  EGS_CHECK_ARG(phase >= 0 && phase <= 2);
  EGS_CHECK_ARG(!pose_only || (pose && phase == 0 && !accum && !absgrad));
  // (the caller reads the records afterwards: they must be its own; no ABS + EXTRA instance of the draw kernel)
  EGS_CHECK_ARG(!absgrad || ((grad_records || n == 0) && !extras));
  EGS_CHECK_ARG(raw || (!shs_high && !dloss_dshs_high));
  // pose (nullable): the camera gradient needs every row in one launch (k_pose_reduce sums all partial rows)
  if (pose) {
    EGS_CHECK_ARG(phase == 0 && pose->dloss_dRcw && pose->dloss_dtcw);
    if (pose->ws_bytes < egs_pose_ws_bytes(n) || !pose->ws) {
      set_error(EGS_ERR_WORKSPACE, "fused_backward pose workspace too small", __FILE__, __LINE__);
      return EGS_ERR_WORKSPACE;
    }
    if (n == 0) {   // nothing drawn: the pose gradient is zero
      EGS_HIP(hipMemsetAsync(pose->dloss_dRcw, 0, 9 * sizeof(float), (hipStream_t)stream));
      EGS_HIP(hipMemsetAsync(pose->dloss_dtcw, 0, 3 * sizeof(float), (hipStream_t)stream));
    }
  }
  if (phase != 2) { row_begin = 0; row_count = n; }
  EGS_CHECK_ARG(row_begin >= 0 && row_count >= 0 && row_begin + (int64_t)row_count <= n && row_begin % 256 == 0);
  EGS_CHECK_ARG(sh_dim == 3 || sh_dim == 12 || sh_dim == 27 || sh_dim == 48);
  if (n == 0) return 0;
  EGS_CHECK_ARG(pws && rots && scales && shs && alphas && Rcw && tcw && twc && depths && ws &&
                (pose_only || (dloss_dpws && dloss_dshs && dloss_dalphas && dloss_dscales && dloss_drots && dloss_dus)));
  if (raw) EGS_CHECK_ARG(rec && (sh_dim == 3 || (shs_high && (dloss_dshs_high || factored || pose_only))));
  if (ws_bytes < egs_splat_bwd_ws_bytes(n)) {
    set_error(EGS_ERR_WORKSPACE, "fused_backward workspace too small", __FILE__, __LINE__);
    return EGS_ERR_WORKSPACE;
  }
  // where splat_bwd_packed puts the records
  float* gpack = grad_records ? grad_records : (float*)((char*)ws + align_up((size_t)n * 48, 256));
  if (phase != 2) {
    // (the forward's own segment workspace, never a rebuild; no hint words: the forward draw reports the walks)
    int rc = splat_bwd_packed(
        n, patches, width, height, pol,
        {.rec = rec, .us = us, .cinv2ds = cinv2ds, .alphas = alphas, .colors = colors, .areas = areas},
        {.contrib = contrib, .final_tau = final_tau, .ranges = patch_range_per_tile, .gsid = gsid_per_patch},
        dloss_dgammas, ws,
        {.tile_order = tile_order, .grad_records = grad_records, .keep_forward_order = keep_order, .masked_lists = masked,
         .seg_ws = seg_ws, .seg_ws_bytes = seg_ws_bytes, .extras = extras, .absgrad = absgrad},
        &gpack, stream);
    if (rc) return rc;
    if (phase == 1) return 0;
  }
  if (row_count == 0) return 0;
  const PreParams pp = make_pre_params(pol, fx, fy, cx, cy, width, height);
  const int kh = sh_dim - 3;
  const size_t r0 = (size_t)row_begin;
  dim3 g(div_up(row_count, 256)), b(256);
  hipStream_t s = (hipStream_t)stream;
  float* pose_ws = pose ? (float*)pose->ws : nullptr;
  // the profiler label names the flavour: POSE_ONLY over AA over POSE over EXTRA
  const char* label = pose_only ? "k_preprocess_bwd_pose_only"
                      : aa      ? "k_preprocess_bwd_aa"
                      : pose    ? "k_preprocess_bwd_pose"
                      : extras  ? "k_preprocess_bwd_extra"
                                : "k_preprocess_bwd";
  // the widths of the SH rows in (shs) and out (dloss_dshs): the low part alone for RAW / the factored gradient
  const int sh_in = raw ? 3 : sh_dim, sh_out = (factored || raw) ? 3 : sh_dim;
  // row_begin is a multiple of the workgroup's 256 rows: every offset pointer keeps its 16-B alignment
  decltype(&k_preprocess_bwd<1, false, false, false, false, false, false>) kern = nullptr;   // flags -> template arguments
  with_sh_dim(sh_dim, [&](auto nc) {
    if (pose_only)   // (instantiated with POSE alone)
      with_bools(
          [&](auto raw_c, auto jw, auto extra, auto aa_c) {
            kern = k_preprocess_bwd<nc.value, raw_c.value, jw.value, extra.value, true, aa_c.value, true>;
          },
          raw, dcolor_dpws != nullptr, extras != nullptr, aa);
    else
      with_bools(
          [&](auto raw_c, auto jw, auto extra, auto pose_c, auto aa_c) {
            kern = k_preprocess_bwd<nc.value, raw_c.value, jw.value, extra.value, pose_c.value, aa_c.value, false>;
          },
          raw, dcolor_dpws != nullptr, extras != nullptr, pose != nullptr, aa);
  });
  EGS_LAUNCH(label, kern, g, b, s, row_count, pp, pws + 3 * r0, rots + 4 * r0, scales + 3 * r0, shs + sh_in * r0,
             (raw && shs_high) ? shs_high + kh * r0 : shs_high, alphas + r0, Rcw, tcw, twc, depths + r0,
             (const float4*)gpack + 3 * r0, dloss_dpws + 3 * r0, dloss_dshs + sh_out * r0,
             factored ? (row_begin == 0 ? dloss_dshs + 3 * (size_t)n : nullptr)
                      : ((raw && dloss_dshs_high) ? dloss_dshs_high + kh * r0 : dloss_dshs_high),
             dloss_dalphas + r0, dloss_dscales + 3 * r0, dloss_drots + 4 * r0, dloss_dus + 2 * r0,
             dcolor_dpws ? dcolor_dpws + 9 * r0 : dcolor_dpws, accum, pose_ws);
  EGS_LAUNCH_OK();
  if (pose) {
    EGS_LAUNCH("k_pose_reduce", k_pose_reduce, dim3(1), dim3(1024), s, (int)g.x, pose_ws, Rcw, tcw, pose->dloss_dRcw,
               pose->dloss_dtcw);
    EGS_LAUNCH_OK();
  }
  return 0;
}

extern "C" int egs_sh_grad_views(int n, int sh_dim, int views, const float* pws, const float* rows,
                                 int64_t row_stride, float scale, float* dloss_dshs, float* dloss_dhigh_shs,
                                 int accumulate, void* stream) {
  EGS_CHECK_ARG(n >= 0 && views >= 0);
  EGS_CHECK_ARG(sh_dim == 3 || sh_dim == 12 || sh_dim == 27 || sh_dim == 48);
  if (n == 0) return 0;
  EGS_CHECK_ARG(pws && dloss_dshs && (views == 0 || rows) && row_stride >= 3 * (int64_t)n + 3);
  const bool raw = dloss_dhigh_shs != nullptr;
  EGS_CHECK_ARG((((uintptr_t)dloss_dshs | (uintptr_t)dloss_dhigh_shs) & 15) == 0);
  dim3 g(div_up(n, 256)), b(256);
  hipStream_t s = (hipStream_t)stream;
  decltype(&k_sh_grad_views<1, false>) kern = nullptr;
  with_sh_dim(sh_dim, [&](auto nc) {
    // degree 0: the row IS the low part ([N][3] either way) -- no RAW instance
    with_bools([&](auto raw_c) { kern = k_sh_grad_views<nc.value, raw_c.value && nc.value != 1>; }, raw);
  });
  EGS_LAUNCH("k_sh_grad_views", kern, g, b, s, n, views, pws, rows, row_stride, scale, dloss_dshs, dloss_dhigh_shs,
             accumulate ? 1 : 0);
  EGS_LAUNCH_OK();
  return 0;
}
