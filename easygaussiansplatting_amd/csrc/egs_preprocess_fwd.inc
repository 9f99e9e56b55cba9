// Body of the fused forward kernels k_preprocess_fwd (AA = false) and k_preprocess_fwd_aa (AA = true),
// egs_preprocess.hip.  Included inside the kernel, as egs_preprocess_bwd.inc: the parameters, NC, RAW, JW and AA come
// from there.
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
    if constexpr (KH > 0) {
      if constexpr (KH % 2 == 1) stage_span_in<KH>(shs_high, n, blockIdx.x * 256, stage, sh + 3);
      else stage_rows_in<KH>(shs_high, n, blockIdx.x * 256, stage, sh + 3);
    }
  }
  float4 r[3] = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};
  float jw[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  uint4 crec = make_uint4(0u, 0u, 0u, 0u);
  if (i < n) {
    const f3 pw = ld3(pws + 3 * (size_t)i);
#if EGS_PRE_EARLY_LOADS
    // (requested with the position, not after the colour: one dependent round trip less per row)
    float4 q_in = *reinterpret_cast<const float4*>(rots + 4 * (size_t)i);
    f3 sc_in = ld3(scales + 3 * (size_t)i);
    const float alpha_in = (rec || bo.br) ? alphas[i] : 0.f;
#endif
    float col[3];
    {  // colour has no depth test in the reference (kernel.cu:619-725)
      if constexpr (RAW) {
        sh[0] = shs[3 * (size_t)i]; sh[1] = shs[3 * (size_t)i + 1]; sh[2] = shs[3 * (size_t)i + 2];
      } else {  // direct dwordx4 row loads: staging them through LDS measured 10 % slower here
        load_sh_row<K>(shs + (size_t)K * i, sh);
      }
      const ShDir<NC> d = sh_basis_f<NC>(pw, twc);
#if EGS_SH_FUSED_JAC_PRE
      if constexpr (JW) sh_color_and_jac_dpw<NC>(d, sh, col, jw);
      else sh_color_f<NC>(d, sh, col);
      if (colors) st3(colors + 3 * (size_t)i, {col[0], col[1], col[2]});
#else
      sh_color_f<NC>(d, sh, col);
      if (colors) st3(colors + 3 * (size_t)i, {col[0], col[1], col[2]});
      if constexpr (JW) sh_jac_dpw<NC>(d, sh, jw);
#endif
    }
    const Proj P = project_f(pw, Rcw, tcw, pp.fx, pp.fy, pp.cx, pp.cy);
    float u0 = 0.f, u1 = 0.f, depth = EGS_BAD_MARKER, ci[3] = {0.f, 0.f, 0.f};
    int rx = 0, ry = 0;
    float aa_comp = 0.f;   // (AA: the opacity compensation; 0 for near-culled Gaussians)
    if (!(pp.near_cull && P.pc.z < EGS_MIN_DEPTH)) {
      u0 = P.u0; u1 = P.u1; depth = P.pc.z;
#if EGS_PRE_EARLY_LOADS
      float4 q = q_in;
      f3 sc = sc_in;
#else
      float4 q = *reinterpret_cast<const float4*>(rots + 4 * (size_t)i);
      f3 sc = ld3(scales + 3 * (size_t)i);
#endif
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
#if EGS_PRE_EARLY_LOADS
    float alpha_act = (rec || bo.br) ? (RAW ? act_alpha(alpha_in) : alpha_in) : 0.f;
#else
    float alpha_act = (rec || bo.br) ? (RAW ? act_alpha(alphas[i]) : alphas[i]) : 0.f;
#endif
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
    // the packed 2D record of the draw kernels, straight from registers (no k_pack_records pass)
    if (rec)
      make_record(u0, u1, ci[0], ci[1], ci[2], alpha_act, col[0], col[1], col[2], rx, ry,
                  pp.W, pp.H, pp.footprint, pp.alpha_skip, r);
  }
  if (bo.br) {
    __syncthreads();   // (RAW: every wave is done with the rows staged in)
    block_max_key(dkey, bo.maxkey, reinterpret_cast<uint32_t*>(stage));
    if (i < n) bo.cr[i] = crec;     // (16 B per lane, consecutive lanes: full lines)
  }
  // 48-B records leave as full lines (lane-strided 16-B pieces cost 3x the write requests)
  if (rec) stage_rows_out<12>(reinterpret_cast<const float*>(r), reinterpret_cast<float*>(rec), n, blockIdx.x * 256, stage);
  if constexpr (JW) rows_out<9>(jw, dcolor_dpws, n, blockIdx.x * 256, stage);
