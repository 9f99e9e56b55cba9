// Body of the backward draw kernels k_draw_bwd (EXTRA = false) and k_draw_bwd_extra (EXTRA = true), egs_draw.hip.
// Included inside the kernel, as egs_draw_fwd.inc: the parameters (p, ranges, gsid, rec, final_tau, contrib, dLdg, gpack,
// sg), the LDS pieces sA, sB, sC, sD, szero, sZ, `ex` (DrawExtras) and the flags BOX, FLOOR, CLAMP, RED, SEG, EXTRA come
// from there.
  constexpr bool ZLDS = (RED & 2) != 0, LAZY = (RED & 4) != 0;
  constexpr int NQ = EXTRA ? 10 : 9;
  if (ZLDS && threadIdx.x < 3) szero[threadIdx.x] = make_float4(0.f, 0.f, 0.f, 0.f);
  const uint32_t zaddr = (uint32_t)(uintptr_t)szero;   // LDS byte offset of the zero line
  int tile, seg_lo = 0, seg_hi = 0x7fffffff;   // SEG: the entries [seg_lo, seg_hi) of the tile's list are this wave's
  size_t seg_state = 0;
  bool seg_item = false;
  if constexpr (SEG) {
    if ((int)blockIdx.x >= min(sg.hdr[SH_ITEMS1], sg.item_cap)) return;
    const uint32_t item = (uint32_t)sg.items1[blockIdx.x];
    tile = (int)(item & SEG_TILE_MASK);
    if (tile >= p.T) return;
    if ((item >> 30) == (uint32_t)SEG_SPEC) {
      const int L = sg.hdr[SH_L], sidx = (int)((item >> 19) & SEG_SEG_MASK);
      seg_item = true;
      seg_lo = sidx * L; seg_hi = seg_lo + L;
      seg_state = ((size_t)(sg.seg_base[tile] + sidx)) * 256 + threadIdx.x;
    }
  } else {
    tile = xcd_tile(blockIdx.x, p);
    if (tile < 0) return;
  }
  const int r0 = ranges[2 * (size_t)tile], r1 = ranges[2 * (size_t)tile + 1];
  const int n = r1 - r0;
  if (n <= 0) return;
  if (SEG) seg_hi = min(seg_hi, n);
  const int lane = threadIdx.x;
  const int tx0 = (tile % p.gx) * EGS_TILE, ty0 = (tile / p.gx) * EGS_TILE;
  const int pxb[2] = {tx0 + (lane & 7), tx0 + (lane & 7) + 8};
  const int pyb[2] = {ty0 + (lane >> 3), ty0 + (lane >> 3) + 8};
  const float fpx[2] = {(float)pxb[0], (float)pxb[1]};
  const float fpy[2] = {(float)pyb[0], (float)pyb[1]};
  const size_t HW = (size_t)p.W * p.H;
  // lq = dL/dgamma . gamma_cur2last: the only combination of gamma_cur2last (kernel.cu:854,948)
  // the gradient needs, so the 3-vector recurrence q += a'(c - q) is carried as one scalar
  float tau[4], lr[4], lg[4], lb[4], lq[4];
  float ld[4], la[4];   // EXTRA: dL/ddepth, dL/dalpha of the pixel
  int cont[4];
  int bmax[4];  // wave-uniform: largest contrib of block k -> entries >= bmax[k] are inert for it
  int maxcont = 0;
  // (all twenty loads requested first, from clamped addresses: guarded and inside the loop below, every block's
  // five waited for their own round trip before the next block's were issued)
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int px = pxb[k & 1], py = pyb[k >> 1];
    const size_t pix = (size_t)min(py, p.H - 1) * p.W + min(px, p.W - 1);
    tau[k] = final_tau[pix];
    cont[k] = contrib[pix];
    lr[k] = dLdg[pix]; lg[k] = dLdg[HW + pix]; lb[k] = dLdg[2 * HW + pix];
    lq[k] = 0.f;
    ld[k] = 0.f; la[k] = 0.f;
    if constexpr (EXTRA) {
      if (ex.dl_depth) ld[k] = ex.dl_depth[pix];
      if (ex.dl_alpha) la[k] = ex.dl_alpha[pix];
    }
  }
  if constexpr (EXTRA) {
    // lq - dL/dalpha is carried instead of lq: dq = dL/dgamma . c + dL/ddepth z + dL/dalpha - lq with one FMA per hit,
    // and the update lq += a' dq is the same for both
#pragma unroll
    for (int k = 0; k < 4; ++k) lq[k] = lr[k] * ex.bg[0] + lg[k] * ex.bg[1] + lb[k] * ex.bg[2] - la[k];
  }
  float4 segE[4];
  if constexpr (SEG) {   // (requested with the loads above; a DIRECT item or the last segment never uses them)
#pragma unroll
    for (int k = 0; k < 4; ++k) segE[k] = seg_item ? sg.st4[seg_state + 64 * k] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int px = pxb[k & 1], py = pyb[k >> 1];
    if (!(px < p.W && py < p.H)) { tau[k] = 0.f; cont[k] = 0; lr[k] = 0.f; lg[k] = 0.f; lb[k] = 0.f; }
    if constexpr (SEG) {
      if (seg_item) {
        if (cont[k] > seg_hi) {          // contributors behind this segment: start from the state at its end
          tau[k] = segE[k].w;
          lq[k] = lr[k] * segE[k].x + lg[k] * segE[k].y + lb[k] * segE[k].z;
          cont[k] = seg_hi;
        } else if (cont[k] <= seg_lo) {  // the pixel never got this far
          cont[k] = 0;
        }
      }
    }
    int mx = cont[k];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mx = max(mx, __shfl_xor(mx, d, 64));
    bmax[k] = __builtin_amdgcn_readfirstlane(min(mx, n));
    maxcont = max(maxcont, bmax[k]);
  }
  if (maxcont <= 0) return;
  // The loads above must be WAITED FOR here, not at their first use inside the loop: gfx9 counts stores and
  // atomics in the same in-order vmcnt as loads, so a wait the compiler places at the first use (inside the
  // hit body) would, from the second group on, also wait for the previous group's gradient atomics --
  // a round trip to L2 per group of four entries on the critical path of the wave.
#pragma unroll
  for (int k = 0; k < 4; ++k)
    asm volatile("" ::"v"(tau[k]), "v"(lr[k]), "v"(lg[k]), "v"(lb[k]), "v"(cont[k]));
  if constexpr (EXTRA) {
#pragma unroll
    for (int k = 0; k < 4; ++k) asm volatile("" ::"v"(ld[k]), "v"(lq[k]));
  }
  // where the transposing reduction leaves the nine totals inside a row of 16 lanes, and what each of
  // those lanes adds to the packed gradient record {dalpha, dcolor[3], du[2], dcinv[3]}
  const int c16 = lane & 15;
  int qoff = -1, kind = 0;
  float kscale = 1.f;
  if (c16 & 1) {
    if (c16 == 1) { qoff = 8; kscale = -0.5f; }                         // M2yy -> dcinv.z
    else if (EXTRA && c16 == 3) qoff = 9;                               // dz   -> the first pad slot
  }
  else if (c16 == 0) { qoff = 4; kind = 1; }                            // M1x  -> du.x
  else if (c16 == 2) { qoff = 5; kind = 2; }                            // M1y  -> du.y
  else if (c16 == 4) qoff = 0;                                          // dalpha
  else if (c16 == 6) qoff = 1;                                          // dcolor.r
  else if (c16 == 8) qoff = 2;                                          // dcolor.g
  else if (c16 == 10) qoff = 3;                                         // dcolor.b
  else if (c16 == 12) { qoff = 6; kscale = -0.5f; }                     // M2xx -> dcinv.x
  else { qoff = 7; kscale = -1.f; }                                     // M2xy -> dcinv.y  (lane 14)

  const int c_first = (maxcont - 1) >> 6;
  int gnext = (c_first * 64 + lane < n) ? gsid[r0 + c_first * 64 + lane] : 0;   // one chunk ahead, as in k_draw
  const int c_last = SEG ? (seg_lo >> 6) : 0;
  for (int c = c_first; c >= c_last; --c) {
    __syncthreads();
    const int idx = c * 64 + lane;
    int mymask = 0;  // reach mask of the entry THIS lane staged (lane j <-> entry c*64 + j)
    const int gm = gnext;
    const int g = p.masked ? (int)((uint32_t)gm & EGS_GSID_MASK) : gm;
    if (c > c_last) gnext = gsid[r0 + idx - 64];
    if (idx < n) {
      float4 A = rec[3 * (size_t)g], B = rec[3 * (size_t)g + 1];
      const float4 C = rec[3 * (size_t)g + 2];
      constexpr float INVQ = 1.f / EGS_NHL2E;
      // (cinv from the record as it is: an entry with a NaN conic hands NaN to du = -cinv M1, as kernel.cu:926-933 does)
      const float4 Dc = make_float4(A.z * INVQ, A.w * (0.5f * INVQ), B.x * INVQ, __int_as_float(g));
      const bool nanfix = p.nan_blend && nan_entry_fix(A, B);
      mymask = p.masked ? (int)((uint32_t)gm >> EGS_GSID_BITS) : reach_mask<BOX>(A, C, tx0, ty0);
      if (nanfix && !BOX && !p.masked) mymask = 0xF;
      sA[lane] = A;
      sB[lane] = B;
      sC[lane] = C;
      if constexpr (EXTRA) sZ[lane] = ex.depths[g];
      // cinv back out of the pre-scaled conic of the record (q = -0.5 log2(e) (cinv.x, 2 cinv.y, cinv.z)):
      // no second 12-B gather per patch (131 MB of sector traffic at P = 4.1 M)
      sD[lane] = Dc;
    }
    __syncthreads();
    // Which entries of this chunk can contribute at all?  Every lane answers for the entry it staged: its
    // reach mask minus the blocks no pixel of which ever got this far (entry index >= the block's largest
    // contrib, kernel.cu:899); a scalar bit scan then walks the reachable entries in descending list order.
    // Groups of four: each of the four accumulator slots takes entries until one of them HITS (a quarter
    // of the entries that reach a live block hit no pixel: they leave the slot zero and cost neither a
    // re-zeroing nor a share of a wave reduction).
    int rl = mymask;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (idx >= bmax[k]) rl &= ~(1 << k);
    unsigned long long todo = __ballot(rl != 0);
    while (todo != 0ull) {
      int je[4] = {-1, -1, -1, -1};   // chunk-local entry index held by slot e
      float acc[4][NQ];
      bool any = false;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (ZLDS) {
          // The nine zeros come out of LDS: broadcast reads of a zero line cost the VALU nothing (nine v_mov_b32 or
          // five v_mov_b64 are 21 issue cycles per slot in a kernel that is VALU-issue bound; the LDS pipe idles).
          // Inline asm, because the compiler would hoist a plain load and hand out register copies again.  The
          // wait is part of the statement: the compiler does not see these loads in its lgkmcnt bookkeeping and
          // may copy the results anywhere afterwards.  (The wave parks for one LDS latency; its four neighbours
          // on the SIMD issue meanwhile.)
          typedef float f4v __attribute__((ext_vector_type(4)));
          f4v z0, z1;
          float z2;
          asm volatile("ds_read_b128 %0, %3\n ds_read_b128 %1, %3 offset:16\n ds_read_b32 %2, %3 offset:32\n"
                       " s_waitcnt lgkmcnt(0)"
                       : "=v"(z0), "=v"(z1), "=v"(z2) : "v"(zaddr));
          acc[e][0] = z0.x; acc[e][1] = z0.y; acc[e][2] = z0.z; acc[e][3] = z0.w;
          acc[e][4] = z1.x; acc[e][5] = z1.y; acc[e][6] = z1.z; acc[e][7] = z1.w;
          acc[e][8] = z2;
        } else {  // nine zeros from five 64-bit moves (v_mov_b64 on gfx940+)
#pragma unroll
          for (int q = 0; q < 8; q += 2) {
            unsigned long long z = 0ull;
            asm volatile("" : "+v"(z));   // materialise the pair in VGPRs, keep it from being split into two constants
            acc[e][q] = __uint_as_float((unsigned)z);
            acc[e][q + 1] = __uint_as_float((unsigned)(z >> 32));
          }
          acc[e][8] = 0.f;
        }
        if constexpr (EXTRA) acc[e][NQ - 1] = 0.f;
        while (todo != 0ull) {
        const int j = 63 - __clzll((long long)todo);
        todo &= ~(1ull << j);
        bool any_e = false;
        const int i = c * 64 + j;  // forward index of this entry in the tile list
        const int reach = __builtin_amdgcn_readlane(rl, j);  // lane j's register: no LDS round trip
        const float4 A = sA[j], B = sB[j], C = sC[j];
        float zj = 0.f;
        if constexpr (EXTRA) zj = sZ[j];
        bool inx[2] = {true, true}, iny[2] = {true, true};
        if (BOX) {
          const uint32_t bx = __float_as_uint(C.y), by = __float_as_uint(C.z);
          const int x0 = bx & 0xFFFF, x1 = bx >> 16, y0 = by & 0xFFFF, y1 = by >> 16;
#pragma unroll
          for (int b = 0; b < 2; ++b) {
            inx[b] = (pxb[b] >= x0) && (pxb[b] < x1);
            iny[b] = (pyb[b] >= y0) && (pyb[b] < y1);
          }
        }
        // LAZY: the exponent from scratch per evaluated block (7 full-rate instructions) instead of the separable
        // form (14 per entry up front + 2 per block): most entries reach one or two of the four blocks.
        // (Measured and dropped: skipping the floor / clamp v_med3 for entries with a positive-definite conic and
        // alpha <= 0.989 behind a wave-uniform flag -- the two scalar branches cost more than the two half-rate
        // instructions they save: +1.5 %.)
        float dx[2], dy[2], cxx[2], cxy[2], cyy[2];
        if (!LAZY) {
#pragma unroll
          for (int b = 0; b < 2; ++b) {
            dx[b] = A.x - fpx[b];
            cxx[b] = A.z * dx[b] * dx[b];
            cxy[b] = A.w * dx[b];
            dy[b] = A.y - fpy[b];
            cyy[b] = B.x * dy[b] * dy[b];
          }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int bx = k & 1, by = k >> 1;
          if (!(reach & (1 << k))) continue;  // scalar branch: block culled or past its last contributor
          float pw;
          if (LAZY) {
            dx[bx] = A.x - fpx[bx];
            dy[by] = A.y - fpy[by];
            float t = A.z * dx[bx];
            t = fmaf(A.w, dy[by], t);
            pw = t * dx[bx];
            pw = fmaf(B.x * dy[by], dy[by], pw);
          } else {
            pw = cxx[bx] + cyy[by] + cxy[bx] * dy[by];
          }
          bool hit = (i < cont[k]) && (pw >= C.w);  // kernel.cu:899,913
          if (BOX) hit = hit && inx[bx] && iny[by];
          if (hit) {
            const float g = __builtin_amdgcn_exp2f(FLOOR ? min_hi(pw, 0.f) : pw);
            float ap = B.y * g;
            if (CLAMP) ap = min_hi(ap, 0.99f);
            const float tk = tau[k] * __builtin_amdgcn_rcpf(1.f - ap);  // undo F.5.2
            tau[k] = tk;
            float dq;   // dL/dgamma . (color - gamma_cur2last)
            if constexpr (EXTRA) dq = fmaf(ld[k], zj, lr[k] * B.z + lg[k] * B.w + lb[k] * C.x) - lq[k];
            else dq = (lr[k] * B.z + lg[k] * B.w + lb[k] * C.x) - lq[k];
            const float dl_dap = tk * dq;  // B.5a
            acc[e][0] += dl_dap * g;  // dalpha'/dalpha = g, also where the clamp binds (kernel.cu:921)
            const float wgt = ap * tk;
            acc[e][1] += lr[k] * wgt; acc[e][2] += lg[k] * wgt; acc[e][3] += lb[k] * wgt;
            if constexpr (EXTRA) acc[e][NQ - 1] += ld[k] * wgt;   // dz
            const float w = dl_dap * ap;
            const float wx = w * dx[bx], wy = w * dy[by];
            acc[e][4] += wx; acc[e][5] += wy;
            acc[e][6] += wx * dx[bx]; acc[e][7] += wx * dy[by]; acc[e][8] += wy * dy[by];
            lq[k] += ap * dq;  // gamma_cur2last <- a' color + (1 - a') gamma_cur2last, dotted with dL/dgamma
            any_e = true;
          }
        }
        if (__any(any_e)) {  // wave-uniform: the entry contributed, the slot is taken
          je[e] = j;
          any = true;
          break;
        }
        }  // next reachable entry into the same (still zero) slot
      }
      if (any) {  // wave-uniform
        // quantity order chosen so that the two first moments meet in one quad (lanes 0 and 2):
        //   lane 0: M1x  2: M1y  4: dalpha  6,8,10: dcolor  12: M2xx  14: M2xy  odd: M2yy
        float rows[NQ];
        constexpr int ORDER[10] = {4, 2, 0, 6, 5, 3, 1, 7, 8, 9};   // acc index feeding leaf q0..q8 (EXTRA: q9)
#pragma unroll
        for (int q = 0; q < NQ; ++q)
          rows[q] = rows_of4(acc[0][ORDER[q]], acc[1][ORDER[q]], acc[2][ORDER[q]], acc[3][ORDER[q]]);
        const float v = (RED & 1) == 0 ? rows_to_lanes9(rows, c16) : rows_to_lanes9_bank(rows, c16);
        // row r of the wave holds the totals of slot e = {0,2,1,3}[r]
        const int row = lane >> 4;
        const int e = ((row & 1) << 1) | (row >> 1);
        const int j = (e == 0) ? je[0] : (e == 1) ? je[1] : (e == 2) ? je[2] : je[3];
        // an empty slot (the chunk ran out of entries) holds zeros and no entry: it must not touch memory
        const bool rowact = j >= 0;
        const float4 D = sD[j & 63];
        // B.5.2b / B.5.2c from the moments: du = -cinv (M1x, M1y) needs both first moments -> the partner
        // comes from the other lane of the pair (quad_perm [2,3,0,1]); dcinv = -(M2xx/2, M2xy, M2yy/2).
        // The 9 atomics of an entry are ONE instruction on ONE 48-byte gradient record.
        const float nb = dpp_get<0x4E>(v);
        const float c_own = (kind == 1) ? -D.x : ((kind == 2) ? -D.z : kscale);
        float val = v * c_own;
        if (kind != 0) val = fmaf(nb, -D.y, val);
        if (rowact && qoff >= 0 && val != 0.f)
          unsafeAtomicAdd(gpack + 12 * (size_t)__float_as_int(D.w) + qoff, val);
      }
    }
  }
