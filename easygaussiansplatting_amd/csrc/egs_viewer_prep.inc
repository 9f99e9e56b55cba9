// Body of the viewer kernels k_viewer_prep (AA = false) and k_viewer_prep_aa (AA = true, the alpha column is
// alpha comp: anti-aliased rendering, DESIGN §3.9), egs_viewer.hip.  Included inside the kernel: the parameters,
// NC and AA come from there.
  constexpr int K = 3 * NC, DIM = 11 + K;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;                                    // (the shader tests `>`: one row past the end)
  const float* __restrict__ g = gs_data + (size_t)DIM * i;
  float* __restrict__ o = gs_prep + 12 * (size_t)i;
  const f3 pw = {g[0], g[1], g[2]};
  const float* V = vp.V;
  const float* P = vp.P;
  const float pcx = V[0] * pw.x + V[1] * pw.y + V[2] * pw.z + V[3];
  const float pcy = V[4] * pw.x + V[5] * pw.y + V[6] * pw.z + V[7];
  const float pcz = V[8] * pw.x + V[9] * pw.y + V[10] * pw.z + V[11];
  const float pcw = V[12] * pw.x + V[13] * pw.y + V[14] * pw.z + V[15];
  depth[i] = pcz;                                        // gau_prep.glsl:188
  float u[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) u[r] = P[4 * r] * pcx + P[4 * r + 1] * pcy + P[4 * r + 2] * pcz + P[4 * r + 3] * pcw;
  const float ux = u[0] / u[3], uy = u[1] / u[3], uz = u[2] / u[3];
  if (fabsf(ux) > 1.3f || fabsf(uy) > 1.3f || fabsf(uz) > 1.f) {   // gau_prep.glsl:192-203
    o[0] = -100.f; o[1] = -100.f; o[2] = -100.f;
    return;
  }
  const float4 q = make_float4(g[3], g[4], g[5], g[6]);  // (w, x, y, z), used as is
  const Cov3 c3 = cov3d_f(q, f3{g[7], g[8], g[9]});
  // computeCov2D (gau_prep.glsl:93-112): T = J W, cov = T Sigma T^T, + 0.3 on the diagonal; no fov clamp
  const float z2 = pcz * pcz;
  const float j00 = vp.fx / pcz, j02 = -(vp.fx * pcx) / z2, j11 = vp.fy / pcz, j12 = -(vp.fy * pcy) / z2;
  float T0[3], T1[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    T0[c] = j00 * V[c] + j02 * V[8 + c];
    T1[c] = j11 * V[4 + c] + j12 * V[8 + c];
  }
  // Sigma from its 6 unique entries (xx, xy, xz, yy, yz, zz)
  const float* s = c3.c;
  const float S0[3] = {s[0] * T0[0] + s[1] * T0[1] + s[2] * T0[2], s[1] * T0[0] + s[3] * T0[1] + s[4] * T0[2],
                       s[2] * T0[0] + s[4] * T0[1] + s[5] * T0[2]};
  const float S1[3] = {s[0] * T1[0] + s[1] * T1[1] + s[2] * T1[2], s[1] * T1[0] + s[3] * T1[1] + s[4] * T1[2],
                       s[2] * T1[0] + s[4] * T1[1] + s[5] * T1[2]};
  const float c00 = T0[0] * S0[0] + T0[1] * S0[1] + T0[2] * S0[2] + 0.3f;
  const float c01 = T0[0] * S1[0] + T0[1] * S1[1] + T0[2] * S1[2];
  const float c11 = T1[0] * S1[0] + T1[1] * S1[1] + T1[2] * S1[2] + 0.3f;
  const float det = c00 * c11 - c01 * c01;
  if (det == 0.f) {                                      // gau_prep.glsl:219-223
    o[0] = -100.f; o[1] = -100.f; o[2] = -100.f;
    return;
  }
  const float det_inv = 1.f / det;
  // colour: SH of the normalised ray from the camera centre, + 0.5, not clamped (gau_prep.glsl:128-176, 231-237)
  float sh[K];
#pragma unroll
  for (int k = 0; k < K; ++k) sh[k] = g[11 + k];
  const float twc[3] = {vp.cam[0], vp.cam[1], vp.cam[2]};
  const ShDir<NC> d = sh_basis_f<NC>(pw, twc);
  float col[3];
  sh_color_f<NC>(d, sh, col);   // SH + 0.5, no clamp: the shader's computeColor
  o[0] = ux; o[1] = uy; o[2] = uz;
  o[3] = c11 * det_inv; o[4] = -c01 * det_inv; o[5] = c00 * det_inv;
  o[6] = col[0]; o[7] = col[1]; o[8] = col[2];
  o[9] = 3.f * sqrtf(c00); o[10] = 3.f * sqrtf(c11);     // drawing area: 3 sigma of x and y
  if constexpr (AA) {
    const float c2[3] = {c00, c01, c11};
    o[11] = g[10] * aa_comp_f(c2);
  } else {
    o[11] = g[10];
  }
