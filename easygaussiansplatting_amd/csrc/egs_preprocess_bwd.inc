// Body of the chain-rule kernels k_preprocess_bwd (EXTRA = false), k_preprocess_bwd_extra (EXTRA = true),
// k_preprocess_bwd_pose (POSE = true) and k_preprocess_bwd_aa (AA = true, either EXTRA, either POSE),
// egs_preprocess.hip.  Included inside the kernel, as egs_draw_fwd.inc: the parameters, NC, RAW, JW, EXTRA, POSE and AA
// come from there.
  // AA (anti-aliased rendering, DESIGN §3.9): the forward drew opacity alpha comp, so ga.x = dL/d(alpha comp):
  // dL/dalpha = ga.x comp and dL/dcov2d gains ga.x alpha dcomp/dcov2d before it feeds J3, Jp and the pose W term
  // dcolor_dpws (nullable): [N][9] left by k_preprocess_fwd; with it this kernel never reads the SH coefficients
  // mode bit 1 (EGS_BWD_FACTORED_SH): the SH gradient stays in its factored form -- eq (5) is an outer product
  // dL/dcolour (x) basis, so dL_dsh receives the THREE floats dL/dcolour per Gaussian ([N][3], always written, never
  // accumulated) and the rows are formed once per step, for all views, by k_sh_grad_views; dL_dsh_high is not touched
  const int accum = mode & 1;
  const bool factored = (mode & 2) != 0;
  // accum: the five (six) parameter-gradient outputs already hold the gradients of EARLIER views of the step and this
  // view's are ADDED to them (dL_du is per view and always written): a rank that renders V views per step then needs
  // no separate accumulation kernels (torch's `.grad += new`: 976 B per Gaussian and view against 488 here)
  constexpr int K = 3 * NC;
  constexpr int KH = K - 3;
  constexpr int KS = RAW ? (KH > 0 ? KH : 1) : K;   // width of the rows that go through LDS
  __shared__ float stage[RowStage<KS>::LDS_FLOATS];
  const int i = blockIdx.x * 256 + threadIdx.x;
  float sh[JW ? 1 : K], gsh[K];
  if constexpr (!JW) {
    if constexpr (RAW) {
      if constexpr (KH > 0) {
        if constexpr (KH % 2 == 1) stage_span_in<KH>(shs_high, n, blockIdx.x * 256, stage, sh + 3);
        else stage_rows_in<KH>(shs_high, n, blockIdx.x * 256, stage, sh + 3);
      }
      if (i < n) { sh[0] = shs[3 * (size_t)i]; sh[1] = shs[3 * (size_t)i + 1]; sh[2] = shs[3 * (size_t)i + 2]; }
    } else {
      if (pp.stage_in) stage_rows_in<K>(shs, n, blockIdx.x * 256, stage, sh);
      else if (i < n) load_sh_row<K>(shs + (size_t)K * i, sh);
    }
  }
#pragma unroll
  for (int k = 0; k < K; ++k) gsh[k] = 0.f;
  f3 gcol_out = {0.f, 0.f, 0.f};
  // POSE: this lane's share of the camera gradient, {dL/dRcw [3][3], dL/dtcw [3], dL/dtwc [3]} (DESIGN §3.8)
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
    if constexpr (RAW || AA) al_raw = alphas[i];
    float4 o_rot = make_float4(0.f, 0.f, 0.f, 0.f);
    f3 o_scale = {0.f, 0.f, 0.f}, o_pw = {0.f, 0.f, 0.f};
    float o_alpha = 0.f;
    if (accum) {
      o_rot = *reinterpret_cast<const float4*>(dL_drot + 4 * (size_t)i);
      o_scale = ld3(dL_dscale + 3 * (size_t)i);
      o_pw = ld3(dL_dpw + 3 * (size_t)i);
      o_alpha = dL_dalpha[i];
    }
    const f3 gcol = {ga.y, ga.z, ga.w};
    const float gu0 = gb.x, gu1 = gb.y;
    const f3 gci = {gb.z, gb.w, gc.x};
    if constexpr (AA) {
      // (stored below, once comp is known; culled: comp = 0)
    } else if constexpr (RAW) {
      const float al = act_alpha(al_raw);
      dL_dalpha[i] = ga.x * al * (1.f - al) + o_alpha;   // sigmoid'
    } else {
      dL_dalpha[i] = ga.x + o_alpha;
    }
    dL_du[2 * (size_t)i] = gu0; dL_du[2 * (size_t)i + 1] = gu1;
    if (pp.near_cull && depth_i < EGS_MIN_DEPTH) {  // culled: never drawn, all gradients are zero
      if constexpr (AA) dL_dalpha[i] = o_alpha;
      if (!accum) {
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
        const float gal = ga.x * comp;
        dL_dalpha[i] = (RAW ? gal * al * (1.f - al) : gal) + o_alpha;
      }
      float J3[18], Jp[9];
      cov2d_jac(c2, P.pc.z, Rcw, pp.fx, pp.fy, J3, Jp);
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
      if (!factored) {
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          gsh[3 * c] = gcol.x * d.B[c]; gsh[3 * c + 1] = gcol.y * d.B[c]; gsh[3 * c + 2] = gcol.z * d.B[c];
        }
      }
      if constexpr (!JW) sh_jac_dpw<NC>(d, sh, W);
      float* opw = dL_dpw + 3 * (size_t)i;  // eq (7)
      const float opw_old[3] = {o_pw.x, o_pw.y, o_pw.z};
#pragma unroll
      for (int k = 0; k < 3; ++k)
        opw[k] = gpc.x * Rcw[k] + gpc.y * Rcw[3 + k] + gpc.z * Rcw[6 + k] + gcol.x * W[k] + gcol.y * W[3 + k] +
                 gcol.z * W[6 + k] + opw_old[k];
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
  if (factored) {   // (a kernel argument: the whole workgroup leaves here)
    if (i < n) st3(dL_dsh + 3 * (size_t)i, gcol_out);
    // the view's camera centre behind the [N][3] block: the row format of egs_sh_grad_views (dL_dsh_high = its address)
    if (dL_dsh_high && blockIdx.x == 0 && threadIdx.x < 3) dL_dsh_high[threadIdx.x] = twc[threadIdx.x];
    return;
  }
  if constexpr (RAW) {
    if (i < n) {
#pragma unroll
      for (int k = 0; k < 3; ++k) dL_dsh[3 * (size_t)i + k] = gsh[k] + (accum ? dL_dsh[3 * (size_t)i + k] : 0.f);
    }
    if constexpr (KH > 0) {
      if constexpr (KH % 2 == 1) stage_span_out<KH>(gsh + 3, dL_dsh_high, n, blockIdx.x * 256, stage, accum != 0);
      else stage_rows_out<KH>(gsh + 3, dL_dsh_high, n, blockIdx.x * 256, stage, accum != 0);
    }
  } else {
    stage_rows_out<K>(gsh, dL_dsh, n, blockIdx.x * 256, stage, accum != 0);
  }
