// Body of the forward draw kernels k_draw (EXTRA = false) and k_draw_extra (EXTRA = true), egs_draw.hip.  Included
// inside the kernel so that both are the kernel's own code: the parameters (p, ranges, gsid, rec, image, contrib,
// final_tau), the LDS pieces sA, sB, sC, sZ, `ex` (DrawExtras) and the template flags BOX, FLOOR, CLAMP, SKIP, EXTRA come
// from there.  (A shared inline function instead changed the register allocation of the plain instances.)
  const int lane = threadIdx.x;
  if (p.zero_buf) {   // every workgroup of the grid (padding ones included) clears its slice
    const uint32_t z0 = blockIdx.x * p.zero_per, z1 = min(p.zero_n4, z0 + p.zero_per);
    float4* __restrict__ zb = p.zero_buf;
    for (uint32_t i = z0 + lane; i < z1; i += 64) zb[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  const int tile = xcd_tile(blockIdx.x, p);
  if (tile < 0) return;
  const int r0 = ranges[2 * (size_t)tile], r1 = ranges[2 * (size_t)tile + 1];
  const int n = r1 - r0;
  const int tx0 = (tile % p.gx) * EGS_TILE, ty0 = (tile / p.gx) * EGS_TILE;
  // pixel k = 2*by + bx of this lane: (tx0 + (lane&7) + 8 bx, ty0 + (lane>>3) + 8 by)
  const int pxb[2] = {tx0 + (lane & 7), tx0 + (lane & 7) + 8};
  const int pyb[2] = {ty0 + (lane >> 3), ty0 + (lane >> 3) + 8};
  if (n <= 0) {  // empty tile: image = 0, contrib = 0 and final_tau = 0 (NOT 1), exactly what the
                 // reference's early return leaves in its zero-filled outputs (kernel.cu:182)
    if (p.work_out && lane == 0) { p.work_out[tile] = 0; if (p.walk_out) p.walk_out[tile] = 0; walk_raise(p.walk_max, 0); }
    // a tile without patches still holds the (INT_MAX, 0) the binning initialised it with: (0, 0), as the reference
    if (lane == 0 && (r0 != 0 || r1 != 0)) { ranges[2 * (size_t)tile] = 0; ranges[2 * (size_t)tile + 1] = 0; }
    const size_t HW0 = (size_t)p.W * p.H;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int px = pxb[k & 1], py = pyb[k >> 1];
      if (px < p.W && py < p.H) {
        const size_t pix = (size_t)py * p.W + px;
        if constexpr (EXTRA) {   // T = 1 here: the background, no depth, no opacity (final_tau keeps its quirk)
          image[pix] = ex.bg[0]; image[HW0 + pix] = ex.bg[1]; image[2 * HW0 + pix] = ex.bg[2];
          if (ex.depth_out) ex.depth_out[pix] = 0.f;
          if (ex.alpha_out) ex.alpha_out[pix] = 0.f;
        } else {
          image[pix] = 0.f; image[HW0 + pix] = 0.f; image[2 * HW0 + pix] = 0.f;
        }
        contrib[pix] = 0; final_tau[pix] = 0.f;
      }
    }
    return;
  }
  // The exponent of alpha' = exp2(e) is evaluated as a polynomial in the pixel's offset (X, Y) from the TILE
  // CENTRE:  e = c0 + c1 X + c2 Y + qxx XX + qxy XY + qyy YY  with the entry's  c0 = log2(alpha) + E(D),
  // (c1, c2) = grad E(D), D = tile centre - u, computed once per (tile, entry) by the lane that stages the
  // entry (64 entries in parallel), and the six monomials per-lane CONSTANTS (|X|, |Y| <= 7.5).  Five FMAs
  // per 8x8 block and no per-entry set-up (the separable form cxx[bx] + cyy[by] + cxy[bx] dy[by] cost 14
  // VALU instructions per entry before the first block); same accuracy as differences from u itself
  // (emulated in fp32 on the 1 M scene: mean |error| 6e-7, max 4e-5 in the log2 domain, either way).
  const float X[2] = {(float)(lane & 7) - 7.5f, (float)(lane & 7) + 0.5f};
  const float Y[2] = {(float)(lane >> 3) - 7.5f, (float)(lane >> 3) + 0.5f};
  const float XX[2] = {X[0] * X[0], X[1] * X[1]}, YY[2] = {Y[0] * Y[0], Y[1] * Y[1]};
  const float XY[4] = {X[0] * Y[0], X[1] * Y[0], X[0] * Y[1], X[1] * Y[1]};
  // A pixel is finished when its tau fell below tau_stop (kernel.cu:256-260): `tau >= stop` IS the
  // "still blending" test, so no separate done flag is kept.  Lanes outside the image start at -1.
  float tau[4], cr[4], cg[4], cb[4];
  float cd[4];   // EXTRA: sum w z
  int cont[4];
  int live = 0;  // wave-uniform: bit k set while block k still has an unfinished pixel
  const float stop = p.tau_stop, lskip = p.lskip;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    cont[k] = 0;
    tau[k] = ((pxb[k & 1] < p.W) && (pyb[k >> 1] < p.H)) ? 1.f : -1.f;
    cr[k] = 0.f; cg[k] = 0.f; cb[k] = 0.f;
    cd[k] = 0.f;
    if (__any(tau[k] >= stop)) live |= 1 << k;
  }
  constexpr float L99 = -0.014499569695115089f;  // log2(0.99): min(0.99, a) == exp2(min(log2 a, L99))
  const float cx0 = (float)tx0 + 7.5f, cy0 = (float)ty0 + 7.5f;
  // alpha' >= alpha_skip (kernel.cu:246) in the exponent domain: e >= log2(skip), a kernel constant (SKIP =
  // the policy has a skip threshold, compiled in); without one only a NaN exponent fails the compare
  const float lthr = SKIP ? lskip : -INFINITY;
  // the list value of the NEXT chunk is fetched one chunk ahead: the staging of a chunk then pays one global
  // latency (the record gather), not two dependent ones
  int gnext = (lane < n) ? gsid[r0 + lane] : 0;
  for (int base = 0; base < n && live != 0; base += 64) {
    __syncthreads();  // single-wave workgroup: orders the LDS reads of the previous chunk
    int mymask = 0;   // reach mask of the entry THIS lane staged (lane j <-> entry base + j)
    const int gm = gnext;
    const int g = p.masked ? (int)((uint32_t)gm & EGS_GSID_MASK) : gm;
    if (base + 64 + lane < n) gnext = gsid[r0 + base + 64 + lane];
    if (base + lane < n) {
      float4 A = rec[3 * (size_t)g], B = rec[3 * (size_t)g + 1];
      const float4 C = rec[3 * (size_t)g + 2];
      float z = 0.f;
      if constexpr (EXTRA) z = ex.depths[g];
      const bool nanfix = p.nan_blend && nan_entry_fix(A, B);
      // the record's thr = log2(skip / alpha), +inf for an entry that never blends (alpha < skip, or
      // alpha < 0 when there is no skip test): such an entry reaches nothing
      if (C.w < INFINITY) mymask = p.masked ? (int)((uint32_t)gm >> EGS_GSID_BITS) : reach_mask<BOX>(A, C, tx0, ty0);
      if (nanfix && !BOX && !p.masked && C.w < INFINITY) mymask = 0xF;
      // alpha' = exp2(e), e = log2(alpha) + log2 exp(-maha/2) (F.5.1, common.cuh:85-88, pre-scaled conic):
      // no multiply by alpha; the floor (maha >= 0) and the 0.99 clamp are ONE min against `cap`
      const float la = SKIP ? lskip - C.w : __builtin_amdgcn_logf(B.y);
      float cap = 3.0e38f;
      if (FLOOR) cap = CLAMP ? fminf(la, L99) : la;
      else if (CLAMP) cap = L99;
      const float Dx = cx0 - A.x, Dy = cy0 - A.y;
      const float c0 = la + (A.z * Dx * Dx + A.w * Dx * Dy + B.x * Dy * Dy);
      const float c1 = 2.f * A.z * Dx + A.w * Dy, c2 = 2.f * B.x * Dy + A.w * Dx;
      sA[lane] = make_float4(A.z, A.w, B.x, cap);   // qxx, qxy, qyy, cap
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
    // no per-entry v_readlane / v_mov / loop counter.  (Entries past the end of the list staged mask 0.)
    int pk = mymask;
    pk |= __shfl_down(pk, 1, 64) << 4;
    pk |= __shfl_down(pk, 2, 64) << 8;
    pk |= __shfl_down(pk, 4, 64) << 16;
    const int m = __builtin_amdgcn_readfirstlane(min(64, n - base));
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
            inx[b] = (pxb[b] >= x0) && (pxb[b] < x1);
            iny[b] = (pyb[b] >= y0) && (pyb[b] < y1);
          }
        }
        const int idx = vidx0 + t;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int bx = k & 1, by = k >> 1;
          if (reach & (1 << k)) {  // scalar branch: the whole 8x8 block is live and in reach
            float e = fmaf(P.z, Y[by], P.x);
            e = fmaf(P.y, X[bx], e);
            e = fmaf(Q.z, YY[by], e);
            e = fmaf(Q.y, XY[k], e);
            e = fmaf(Q.x, XX[bx], e);
            // unfinished and alpha' >= alpha_skip; the cap cannot change the outcome of the skip test
            // (cap >= log2(skip) for every entry that blends at all), so it is applied to the hits only
            bool hit = (tau[k] >= stop) && (e >= lthr);
            if (BOX) hit = hit && inx[bx] && iny[by];
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
  if (p.work_out) {   // what k_draw_bwd will walk: the largest contributor index of the tile and of its blocks
    int w = 0, wmax = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      int mx = cont[k];
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) mx = max(mx, __shfl_xor(mx, d, 64));
      w += mx;
      wmax = max(wmax, mx);
    }
    if (lane == 0) {
      p.work_out[tile] = w + 2 * wmax;
      if (p.walk_out) p.walk_out[tile] = wmax;
      walk_raise(p.walk_max, wmax);
      if (p.walk_max) walk_raise(p.walk_max + 1, n);      // ... and the longest list of the same render
    }
  }
  const size_t HW = (size_t)p.W * p.H;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int px = pxb[k & 1], py = pyb[k >> 1];
    if (px < p.W && py < p.H) {
      const size_t pix = (size_t)py * p.W + px;
      if constexpr (EXTRA) {   // what is left of the transmittance sees the background; alpha = 1 - T_final
        image[pix] = fmaf(tau[k], ex.bg[0], cr[k]);
        image[HW + pix] = fmaf(tau[k], ex.bg[1], cg[k]);
        image[2 * HW + pix] = fmaf(tau[k], ex.bg[2], cb[k]);
        if (ex.depth_out) ex.depth_out[pix] = cd[k];
        if (ex.alpha_out) ex.alpha_out[pix] = 1.f - tau[k];
      } else {
        image[pix] = cr[k];
        image[HW + pix] = cg[k];
        image[2 * HW + pix] = cb[k];
      }
      contrib[pix] = cont[k];
      final_tau[pix] = tau[k];
    }
  }
