// The viewer's per-frame Gaussian preprocess (reference viewer/shaders/gau_prep.glsl, an OpenGL compute
// shader dispatched by viewer/custom_items/gaussian_item.py:264-272) as a consumer of the same device
// functions as the rasterizer (last item).  One Gaussian per lane:
//
//   gs_data [N, 11 + K]  = {pos 3, rot 4 (w,x,y,z), scale 3, alpha 1, sh K}      (gau_prep.glsl:33-37)
//   gs_prep [N, 12]      = {u 3 (NDC), covinv 3, color 3, area 2, alpha 1}       (gau_prep.glsl:39-44)
//   depth   [N]          = view-space z (the key of the viewer's sort)            (gau_prep.glsl:188)
//
// Semantics are the shader's, not gsplatcu's: cull when |u.xy| > 1.3 or |u.z| > 1 in NDC or det == 0
// (only u = -100 is written then, the rest of the row is left as it was, like the shader does); no fov
// clamp in the covariance projection; area = 3 sqrt(diag); colour = SH + 0.5 without clamping.
// Matrices are 4x4 row-major in the mathematical convention (pc = V pw, u = P pc) -- what
// gaussian_item.py holds before set_uniform_mat4 transposes them for OpenGL.
#include "egs_gaussian_math.h"

namespace egs {

struct ViewerParams {
  float V[16], P[16];      // row-major
  float cam[3];            // inverse(V)[:3, 3]
  float fx, fy;
};

template <int NC>
__global__ __launch_bounds__(256) void k_viewer_prep(int n, ViewerParams vp, const float* __restrict__ gs_data,
                                                     float* __restrict__ gs_prep, float* __restrict__ depth) {
  constexpr bool AA = false;
#include "egs_viewer_prep.inc"
}
template <int NC>
__global__ __launch_bounds__(256) void k_viewer_prep_aa(int n, ViewerParams vp, const float* __restrict__ gs_data,
                                                        float* __restrict__ gs_prep, float* __restrict__ depth) {
  constexpr bool AA = true;
#include "egs_viewer_prep.inc"
}

// 4x4 inverse (row-major) by Gauss-Jordan with partial pivoting; false if singular
static bool invert4(const float* m, double* inv) {
  double a[4][8];
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) { a[r][c] = m[4 * r + c]; a[r][4 + c] = r == c ? 1.0 : 0.0; }
  for (int col = 0; col < 4; ++col) {
    int piv = col;
    for (int r = col + 1; r < 4; ++r)
      if (fabs(a[r][col]) > fabs(a[piv][col])) piv = r;
    if (a[piv][col] == 0.0) return false;
    for (int c = 0; c < 8; ++c) { const double t = a[col][c]; a[col][c] = a[piv][c]; a[piv][c] = t; }
    const double d = a[col][col];
    for (int c = 0; c < 8; ++c) a[col][c] /= d;
    for (int r = 0; r < 4; ++r) {
      if (r == col) continue;
      const double f = a[r][col];
      for (int c = 0; c < 8; ++c) a[r][c] -= f * a[col][c];
    }
  }
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) inv[4 * r + c] = a[r][4 + c];
  return true;
}

}  // namespace egs

using namespace egs;

extern "C" int egs_viewer_prep(int n, int sh_dim, const float* gs_data, const float* view_matrix,
                               const float* projection_matrix, float focal_x, float focal_y, float* gs_prep,
                               float* depth, int flags, void* stream) {
  // flags & EGS_FUSED_ANTIALIASED: the alpha column is alpha comp (include/egs_hip.h)
  EGS_CHECK_ARG((flags & ~EGS_FUSED_ANTIALIASED) == 0);
  const bool aa = flags != 0;
  EGS_CHECK_ARG(n >= 0 && view_matrix && projection_matrix);
  EGS_CHECK_ARG(sh_dim == 3 || sh_dim == 12 || sh_dim == 27 || sh_dim == 48);
  if (n == 0) return 0;
  EGS_CHECK_ARG(gs_data && gs_prep && depth);
  ViewerParams vp;
  for (int k = 0; k < 16; ++k) { vp.V[k] = view_matrix[k]; vp.P[k] = projection_matrix[k]; }
  double inv[16];
  EGS_CHECK_ARG(invert4(view_matrix, inv));               // cam_pos = inverse(view_matrix)[3].xyz
  vp.cam[0] = (float)inv[3]; vp.cam[1] = (float)inv[7]; vp.cam[2] = (float)inv[11];
  vp.fx = focal_x; vp.fy = focal_y;
  hipStream_t s = (hipStream_t)stream;
  dim3 g(div_up(n, 256)), b(256);
#define EGS_VP(NC)                                                                                  \
  do {                                                                                              \
    if (aa) EGS_LAUNCH("k_viewer_prep_aa", k_viewer_prep_aa<NC>, g, b, s, n, vp, gs_data, gs_prep, depth); \
    else EGS_LAUNCH("k_viewer_prep", k_viewer_prep<NC>, g, b, s, n, vp, gs_data, gs_prep, depth);          \
  } while (0)
  switch (sh_dim) {
    case 3: EGS_VP(1); break;
    case 12: EGS_VP(4); break;
    case 27: EGS_VP(9); break;
    default: EGS_VP(16); break;
  }
#undef EGS_VP
  EGS_LAUNCH_OK();
  return 0;
}
