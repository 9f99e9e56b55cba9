// libegs_normalloss.so (include/egs_normalloss.h, which states the loss): surface-normal supervision and edge-aware normal
// smoothness on the render's depth and opacity maps, and their gradient.  Three passes over 32 x 8 tiles,
// a thread per pixel, a workgroup walking the tiles blockIdx.x, blockIdx.x + gridDim.x, ...:
//
//   k_normal_tile  : z = D / A and its validity with a one-pixel halo in LDS -> n and 1 / |c| of the tile's pixels into
//                    the workspace (and normals_out); per-workgroup partial sums {normal-valid pixels, Omega_p,
//                    sum omega_p (1 - n . qh)} in double
//   k_normal_pairs : every pixel with its right and its lower neighbour, n from the workspace -> partial sums {Omega_s,
//                    sum omega_a omega_b g_ab |n_a - n_b|^2 / 2}.  Not launched without the smoothness term.
//   k_normal_grad  : every workgroup reduces the partials (a thread's strided run, the wave, the four waves: the same bits
//                    in each), workgroup 0 writes the stats.  Then, in gather form: dL/dz of a pixel comes from the
//                    normals of its four neighbours only (a central difference does not see its centre), and dL/dn of
//                    each of those from the prior and from that normal's four pairs.  So a tile stages n, omega, the
//                    guide and z with a two-pixel halo, every pixel of the tile and its one-pixel ring turns its dL/dn
//                    into dL/d(dx) and dL/d(dy) (through the normalisation and the cross product) in LDS, and a pixel
//                    adds up the four that name it.  <false>: no gradient plane -- one workgroup, the stats alone.
//
// The per-pixel arithmetic is double: differences of neighbouring points cancel (a 10 m wall at 1080p keeps about four
// digits of them in float32), and double vector arithmetic is far below what the loads leave room for here.
#define EGS_SIDE_LIBRARY "egs_normalloss"
#include "egs_side_error.h"

#include <float.h>
#include <math.h>

#include "../../include/egs_normalloss.h"

namespace egs {

constexpr int TW = EGS_NORMALLOSS_TILE_W, TH = EGS_NORMALLOSS_TILE_H;
constexpr int NL_THREADS = TW * TH;
static_assert(NL_THREADS == 256, "a thread per pixel of a tile, four waves");
constexpr int NPART = 5;                  // the partial sums of a workgroup: the three of the tile pass, the two pairs'
constexpr int NL_MAX_GRID = 2048;         // the workspace holds this many workgroups' partials
// workgroups per CU: a tile is load, barrier, arithmetic, store, so a CU hides the loads of one workgroup behind the
// others'.  k_normal_tile fits eight and k_normal_pairs five (the rest of its grid follows); k_normal_grad's 40 KB of LDS
// leave room for four.
constexpr int NL_SUMS_PER_CU = 8, NL_GRAD_PER_CU = 4;
constexpr int R1W = TW + 2, R1H = TH + 2, R1N = R1W * R1H;      // a tile and its one-pixel ring
constexpr int R2W = TW + 4, R2H = TH + 4, R2N = R2W * R2H;      // ... and its two-pixel ring

struct NlCam { double ifx, ify, cx, cy; };
// what the workspace keeps of a pixel: its normal and 1 / |c|; all zeros where the pixel is not normal-valid
struct alignas(16) NlNrm { double x, y, z, ic; };

// z = D / A of a depth-valid pixel inside the image, -1 elsewhere (a valid z is >= 0; no NaN of the inputs gets further
// than the comparisons, which are false for it)
__device__ __forceinline__ double nl_z(const float* __restrict__ D, const float* __restrict__ A, int x, int y, int W,
                                       int H, float alpha_min) {
  if (x < 0 || y < 0 || x >= W || y >= H) return -1.0;
  const size_t i = (size_t)y * W + x;
  const float d = D[i], a = A[i];
  return (a > alpha_min && d > 0.f) ? (double)d / (double)a : -1.0;
}

// dx = p(x+1, y) - p(x-1, y), dy = p(x, y+1) - p(x, y-1) from the four neighbours' z
__device__ __forceinline__ void nl_diffs(double zl, double zr, double zu, double zd, int x, int y, const NlCam& cam,
                                         double (&dx)[3], double (&dy)[3]) {
  const double X = ((double)x - cam.cx) * cam.ifx, Y = ((double)y - cam.cy) * cam.ify;
  const double Xl = ((double)(x - 1) - cam.cx) * cam.ifx, Xr = ((double)(x + 1) - cam.cx) * cam.ifx;
  const double Yu = ((double)(y - 1) - cam.cy) * cam.ify, Yd = ((double)(y + 1) - cam.cy) * cam.ify;
  dx[0] = zr * Xr - zl * Xl;
  dx[1] = zr * Y - zl * Y;
  dx[2] = zr - zl;
  dy[0] = zd * X - zu * X;
  dy[1] = zd * Yd - zu * Yu;
  dy[2] = zd - zu;
}

__device__ __forceinline__ void nl_cross(const double (&a)[3], const double (&b)[3], double (&c)[3]) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

// the normal of a pixel from its own and its four neighbours' z (-1: not depth-valid, or outside the image)
__device__ __forceinline__ NlNrm nl_normal(double zc, double zl, double zr, double zu, double zd, int x, int y,
                                           const NlCam& cam) {
  NlNrm n = {0.0, 0.0, 0.0, 0.0};
  if (!(zc >= 0.0 && zl >= 0.0 && zr >= 0.0 && zu >= 0.0 && zd >= 0.0)) return n;
  double dx[3], dy[3], c[3];
  nl_diffs(zl, zr, zu, zd, x, y, cam, dx, dy);
  nl_cross(dy, dx, c);
  const double c2 = c[0] * c[0] + c[1] * c[1] + c[2] * c[2];
  if (!(c2 > 0.0 && c2 <= DBL_MAX)) return n;
  n.ic = 1.0 / sqrt(c2);
  n.x = c[0] * n.ic;
  n.y = c[1] * n.ic;
  n.z = c[2] * n.ic;
  return n;
}

// the normalised prior of pixel i; false: the pixel has no data (a non-finite component, or all three zero)
__device__ __forceinline__ bool nl_prior(const float* __restrict__ q, size_t i, size_t n, double (&qh)[3]) {
  const double a = (double)q[i], b = (double)q[n + i], c = (double)q[2 * n + i];
  const double q2 = a * a + b * b + c * c;      // (squares of floats: no overflow in double)
  if (!(q2 > 0.0 && q2 <= DBL_MAX)) return false;
  const double r = 1.0 / sqrt(q2);
  qh[0] = a * r;
  qh[1] = b * r;
  qh[2] = c * r;
  return true;
}

// g_ab = exp(-edge_gamma mean_c |I_a - I_b|)
__device__ __forceinline__ double nl_edge(float a0, float a1, float a2, float b0, float b1, float b2, double gamma) {
  const double m = (fabs((double)a0 - (double)b0) + fabs((double)a1 - (double)b1) + fabs((double)a2 - (double)b2)) *
                   (1.0 / 3.0);
  return exp(-gamma * m);
}

// every thread ends with the workgroup's total of each v[k]: the wave, then the four waves in order
template <int K>
__device__ __forceinline__ void nl_block_sum(double (&v)[K], double (*red)[4]) {
#pragma unroll
  for (int k = 0; k < K; ++k) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v[k] += __shfl_xor(v[k], d, 64);
    if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = red[k][0] + red[k][1] + red[k][2] + red[k][3];
  __syncthreads();
}

__global__ __launch_bounds__(NL_THREADS) void k_normal_tile(int H, int W, int tiles_x, int ntiles,
                                                            const float* __restrict__ D, const float* __restrict__ A,
                                                            NlCam cam, const float* __restrict__ q,
                                                            const float* __restrict__ w, float alpha_min,
                                                            NlNrm* __restrict__ nrm, float* __restrict__ normals_out,
                                                            double* __restrict__ parts) {
  __shared__ double s_z[R1N];
  __shared__ double red[3][4];
  const int tx = threadIdx.x % TW, ty = threadIdx.x / TW;
  const size_t npix = (size_t)H * W;
  double s[3] = {0.0, 0.0, 0.0};
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int x0 = (t % tiles_x) * TW, y0 = (t / tiles_x) * TH;
    for (int j = threadIdx.x; j < R1N; j += NL_THREADS)
      s_z[j] = nl_z(D, A, x0 - 1 + j % R1W, y0 - 1 + j / R1W, W, H, alpha_min);
    __syncthreads();
    const int x = x0 + tx, y = y0 + ty;
    if (x < W && y < H) {
      const int c = (ty + 1) * R1W + tx + 1;
      const NlNrm n = nl_normal(s_z[c], s_z[c - 1], s_z[c + 1], s_z[c - R1W], s_z[c + R1W], x, y, cam);
      const size_t i = (size_t)y * W + x;
      nrm[i] = n;
      if (normals_out) {
        normals_out[i] = (float)n.x;
        normals_out[npix + i] = (float)n.y;
        normals_out[2 * npix + i] = (float)n.z;
      }
      if (n.ic > 0.0) {
        s[0] += 1.0;
        double qh[3];
        if (q && nl_prior(q, i, npix, qh)) {
          const double om = w ? (double)w[i] : 1.0;
          s[1] += om;
          s[2] += om * (1.0 - (n.x * qh[0] + n.y * qh[1] + n.z * qh[2]));
        }
      }
    }
    __syncthreads();
  }
  nl_block_sum<3>(s, red);
  if (threadIdx.x == 0) {
    double* out = parts + (size_t)blockIdx.x * NPART;
    out[0] = s[0];
    out[1] = s[1];
    out[2] = s[2];
    out[3] = 0.0;      // (k_normal_pairs' two, when it runs)
    out[4] = 0.0;
  }
}

__global__ __launch_bounds__(NL_THREADS) void k_normal_pairs(int H, int W, int tiles_x, int ntiles,
                                                             const NlNrm* __restrict__ nrm,
                                                             const float* __restrict__ I,
                                                             const float* __restrict__ w, float edge_gamma,
                                                             double* __restrict__ parts) {
  __shared__ double red[2][4];
  const int tx = threadIdx.x % TW, ty = threadIdx.x / TW;
  const size_t npix = (size_t)H * W;
  const double gamma = (double)edge_gamma;
  double s[2] = {0.0, 0.0};
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int x = (t % tiles_x) * TW + tx, y = (t / tiles_x) * TH + ty;
    if (x >= W || y >= H) continue;
    const size_t i = (size_t)y * W + x;
    const NlNrm a = nrm[i];
    if (!(a.ic > 0.0)) continue;
    const double oa = w ? (double)w[i] : 1.0;
    // (a normal-valid pixel has all four neighbours inside the image)
#pragma unroll
    for (int side = 0; side < 2; ++side) {
      const size_t k = side == 0 ? i + 1 : i + (size_t)W;
      const NlNrm b = nrm[k];
      if (!(b.ic > 0.0)) continue;
      const double ob = w ? (double)w[k] : 1.0;
      const double g = I ? nl_edge(I[i], I[npix + i], I[2 * npix + i], I[k], I[npix + k], I[2 * npix + k], gamma) : 1.0;
      const double ex = a.x - b.x, ey = a.y - b.y, ez = a.z - b.z;
      s[0] += oa * ob;
      s[1] += oa * ob * g * (0.5 * (ex * ex + ey * ey + ez * ez));
    }
  }
  nl_block_sum<2>(s, red);
  if (threadIdx.x == 0) {
    double* out = parts + (size_t)blockIdx.x * NPART;
    out[3] = s[0];
    out[4] = s[1];
  }
}

template <bool WRITE>
__global__ __launch_bounds__(NL_THREADS) void k_normal_grad(int H, int W, int tiles_x, int ntiles,
                                                            const float* __restrict__ D, const float* __restrict__ A,
                                                            NlCam cam, const float* __restrict__ q,
                                                            const float* __restrict__ I, const float* __restrict__ w,
                                                            int smooth, float alpha_min, float edge_gamma,
                                                            float prior_scale, float smooth_scale,
                                                            const NlNrm* __restrict__ nrm, int nparts,
                                                            const double* __restrict__ parts, float* __restrict__ stats,
                                                            float* __restrict__ dD, float* __restrict__ dA) {
  __shared__ double red[NPART][4];
  __shared__ double s_n[4][WRITE ? R2N : 1];      // n and 1 / |c| (0: not normal-valid, or outside the image)
  __shared__ float s_om[WRITE ? R2N : 1];         // omega (a float32 input, or 1)
  __shared__ double s_z[WRITE ? R2N : 1];
  __shared__ float s_I[3][WRITE ? R2N : 1];
  __shared__ double s_g[6][WRITE ? R1N : 1];      // dL/d(dx), dL/d(dy) of the tile and its ring
  double S[NPART] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < nparts; i += NL_THREADS) {
    const double* in = parts + (size_t)i * NPART;
#pragma unroll
    for (int k = 0; k < NPART; ++k) S[k] += in[k];
  }
  nl_block_sum<NPART>(S, red);
  const bool has_p = q != nullptr && S[1] > 0.0, has_s = smooth != 0 && S[3] > 0.0;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    stats[0] = has_p ? (float)(S[2] / S[1]) : 0.f;
    stats[1] = has_s ? (float)(S[4] / S[3]) : 0.f;
    stats[2] = has_p ? (float)S[1] : 0.f;
    stats[3] = has_s ? (float)S[3] : 0.f;
    stats[4] = (float)S[0];
    stats[5] = (float)((q != nullptr && !has_p ? 1 : 0) + (smooth != 0 && !has_s ? 2 : 0));
  }
  if (!WRITE) return;

  const double kp = has_p ? (double)prior_scale / S[1] : 0.0, ks = has_s ? (double)smooth_scale / S[3] : 0.0;
  const double gamma = (double)edge_gamma;
  const size_t npix = (size_t)H * W;
  const int tx = threadIdx.x % TW, ty = threadIdx.x / TW;
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int x0 = (t % tiles_x) * TW, y0 = (t / tiles_x) * TH;
    // 1: the tile's surroundings
    for (int j = threadIdx.x; j < R2N; j += NL_THREADS) {
      const int x = x0 - 2 + j % R2W, y = y0 - 2 + j / R2W;
      NlNrm n = {0.0, 0.0, 0.0, 0.0};
      float om = 0.f;
      float i0 = 0.f, i1 = 0.f, i2 = 0.f;
      if (x >= 0 && y >= 0 && x < W && y < H) {
        const size_t i = (size_t)y * W + x;
        n = nrm[i];
        if (n.ic > 0.0) om = w ? w[i] : 1.f;
        if (I) {
          i0 = I[i];
          i1 = I[npix + i];
          i2 = I[2 * npix + i];
        }
      }
      s_n[0][j] = n.x;
      s_n[1][j] = n.y;
      s_n[2][j] = n.z;
      s_n[3][j] = n.ic;
      s_om[j] = om;
      s_z[j] = nl_z(D, A, x, y, W, H, alpha_min);
      s_I[0][j] = i0;
      s_I[1][j] = i1;
      s_I[2][j] = i2;
    }
    __syncthreads();
    // 2: dL/dn of the tile's pixels and its ring, taken through n = c / |c| and c = dy x dx
    for (int j = threadIdx.x; j < R1N; j += NL_THREADS) {
      const int rx = j % R1W, ry = j / R1W;
      const int c = (ry + 1) * R2W + rx + 1;
      double gdx[3] = {0.0, 0.0, 0.0}, gdy[3] = {0.0, 0.0, 0.0};
      const double ic = s_n[3][c];
      if (ic > 0.0) {      // (normal-valid: inside the image, and so are its four neighbours)
        const int x = x0 - 1 + rx, y = y0 - 1 + ry;
        const double n[3] = {s_n[0][c], s_n[1][c], s_n[2][c]};
        const double om = (double)s_om[c];
        double G[3] = {0.0, 0.0, 0.0};
        double qh[3];
        if (kp != 0.0 && nl_prior(q, (size_t)y * W + x, npix, qh)) {
          const double f = kp * om;
          G[0] -= f * qh[0];
          G[1] -= f * qh[1];
          G[2] -= f * qh[2];
        }
        if (ks != 0.0) {
          const int nb[4] = {c - 1, c + 1, c - R2W, c + R2W};
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const int b = nb[k];
            const double g = I ? nl_edge(s_I[0][c], s_I[1][c], s_I[2][c], s_I[0][b], s_I[1][b], s_I[2][b], gamma) : 1.0;
            const double f = ks * om * (double)s_om[b] * g;      // (omega = 0 and n = 0 at a neighbour without a normal)
            G[0] -= f * s_n[0][b];
            G[1] -= f * s_n[1][b];
            G[2] -= f * s_n[2][b];
          }
        }
        const double nG = n[0] * G[0] + n[1] * G[1] + n[2] * G[2];
        const double gc[3] = {(G[0] - n[0] * nG) * ic, (G[1] - n[1] * nG) * ic, (G[2] - n[2] * nG) * ic};
        double dx[3], dy[3];
        nl_diffs(s_z[c - 1], s_z[c + 1], s_z[c - R2W], s_z[c + R2W], x, y, cam, dx, dy);
        nl_cross(gc, dy, gdx);
        nl_cross(dx, gc, gdy);
      }
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        s_g[k][j] = gdx[k];
        s_g[3 + k][j] = gdy[k];
      }
    }
    __syncthreads();
    // 3: a pixel is the right end of its left neighbour's dx, the left end of its right neighbour's, and so on
    const int x = x0 + tx, y = y0 + ty;
    if (x < W && y < H) {
      const int c = (ty + 1) * R1W + tx + 1;
      const double gx = s_g[0][c - 1] - s_g[0][c + 1] + s_g[3][c - R1W] - s_g[3][c + R1W];
      const double gy = s_g[1][c - 1] - s_g[1][c + 1] + s_g[4][c - R1W] - s_g[4][c + R1W];
      const double gz = s_g[2][c - 1] - s_g[2][c + 1] + s_g[5][c - R1W] - s_g[5][c + R1W];
      const double X = ((double)x - cam.cx) * cam.ifx, Y = ((double)y - cam.cy) * cam.ify;
      const double g = gx * X + gy * Y + gz;
      const double z = s_z[(ty + 2) * R2W + tx + 2];
      const size_t i = (size_t)y * W + x;
      float od = 0.f, oa = 0.f;
      if (z >= 0.0 && g != 0.0) {      // dz/dD = 1 / A, dz/dA = -D / A^2 = -z / A
        const double ia = 1.0 / (double)A[i];
        od = (float)(g * ia);
        oa = (float)(-g * z * ia);
      }
      dD[i] = od;
      dA[i] = oa;
    }
    __syncthreads();
  }
}

// ---- host side of a launch -------------------------------------------------------------------------------------------
static inline int nl_tiles_x(int W) { return div_up(W, TW); }
static inline int nl_tiles(int H, int W) { return nl_tiles_x(W) * div_up(H, TH); }
static inline int nl_grid(int tiles, int per_cu) {
  static const int cus = [] {  // of the current device
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;
    return n;
  }();
  const int resident = per_cu * cus < NL_MAX_GRID ? per_cu * cus : NL_MAX_GRID;      // (within what the workspace holds)
  return tiles < resident ? tiles : resident;
}
// The workspace of a call, 256-B aligned pieces: n and 1 / |c| per pixel [H W] (32 B each), the partial sums
// [NL_MAX_GRID][NPART] (double).  ws == NULL asks for `bytes` alone.
struct NlWs { NlNrm* nrm; double* parts; size_t bytes; };
static inline NlWs nl_ws(void* ws, int H, int W) {
  const size_t o_p = align_up((size_t)H * W * sizeof(NlNrm), 256);
  char* base = (char*)ws;
  return {ws ? (NlNrm*)base : nullptr, ws ? (double*)(base + o_p) : nullptr,
          o_p + align_up((size_t)NL_MAX_GRID * NPART * sizeof(double), 256)};
}

}  // namespace egs

using namespace egs;

static bool aligned_to(const void* a, uintptr_t k) { return ((uintptr_t)a & (k - 1)) == 0; }
static bool finite_f(float v) { return v >= -FLT_MAX && v <= FLT_MAX; }

extern "C" int egs_normalloss_abi_version(void) { return EGS_NORMALLOSS_ABI_VERSION; }
extern "C" const char* egs_normalloss_last_error_string(void) { return egs_side::g_err; }

extern "C" size_t egs_normalloss_ws_bytes(int H, int W) {
  if (H <= 0 || W <= 0 || (int64_t)H * W > EGS_NORMALLOSS_MAX_PIXELS) return 256;
  return nl_ws(nullptr, H, W).bytes;
}

extern "C" int egs_normalloss(int H, int W, const float* depth, const float* alpha, float fx, float fy, float cx,
                              float cy, const float* normals, const float* guide, const float* weight, int smooth,
                              float alpha_min, float edge_gamma, float prior_scale, float smooth_scale, void* ws,
                              size_t ws_bytes, float* stats, float* normals_out, float* dloss_ddepth,
                              float* dloss_dalpha, void* stream) {
  SIDE_CHECK_ARG(H > 0 && W > 0);
  SIDE_CHECK_ARG((int64_t)H * W <= EGS_NORMALLOSS_MAX_PIXELS);
  SIDE_CHECK_ARG(depth != nullptr && aligned_to(depth, 4));
  SIDE_CHECK_ARG(alpha != nullptr && aligned_to(alpha, 4));
  SIDE_CHECK_ARG(fx > 0.f && fx <= FLT_MAX && fy > 0.f && fy <= FLT_MAX);
  SIDE_CHECK_ARG(finite_f(cx) && finite_f(cy));
  SIDE_CHECK_ARG(aligned_to(normals, 4) && aligned_to(guide, 4) && aligned_to(weight, 4));
  SIDE_CHECK_ARG(smooth == 0 || smooth == 1);
  SIDE_CHECK_ARG(alpha_min >= 0.f && alpha_min <= FLT_MAX);
  SIDE_CHECK_ARG(edge_gamma >= 0.f && edge_gamma <= FLT_MAX);
  SIDE_CHECK_ARG(finite_f(prior_scale) && finite_f(smooth_scale));
  SIDE_CHECK_ARG(ws != nullptr && aligned_to(ws, 16));
  SIDE_CHECK_ARG(stats != nullptr && aligned_to(stats, 4));
  SIDE_CHECK_ARG(aligned_to(normals_out, 4) && aligned_to(dloss_ddepth, 4) && aligned_to(dloss_dalpha, 4));
  SIDE_CHECK_ARG((dloss_ddepth == nullptr) == (dloss_dalpha == nullptr));
  SIDE_CHECK_ARG(dloss_ddepth == nullptr || dloss_ddepth != dloss_dalpha);
  SIDE_CHECK_ARG(normals_out == nullptr || (normals_out != dloss_ddepth && normals_out != dloss_dalpha));
  for (const float* out : {normals_out, dloss_ddepth, dloss_dalpha})
    if (out) SIDE_CHECK_ARG(out != depth && out != alpha && out != normals && out != guide && out != weight);
  if (ws_bytes < egs_normalloss_ws_bytes(H, W)) {
    egs_side::set_error(EGS_ERR_WORKSPACE, "normalloss workspace too small", __FILE__, __LINE__);
    return EGS_ERR_WORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  const NlWs m = nl_ws(ws, H, W);
  const NlCam cam = {1.0 / (double)fx, 1.0 / (double)fy, (double)cx, (double)cy};
  const int tiles_x = nl_tiles_x(W), ntiles = nl_tiles(H, W);
  const int grid = nl_grid(ntiles, NL_SUMS_PER_CU), ggrid = nl_grid(ntiles, NL_GRAD_PER_CU);
  hipLaunchKernelGGL(k_normal_tile, dim3(grid), dim3(NL_THREADS), 0, s, H, W, tiles_x, ntiles, depth, alpha, cam,
                     normals, weight, alpha_min, m.nrm, normals_out, m.parts);
  if (smooth)
    hipLaunchKernelGGL(k_normal_pairs, dim3(grid), dim3(NL_THREADS), 0, s, H, W, tiles_x, ntiles,
                       (const NlNrm*)m.nrm, guide, weight, edge_gamma, m.parts);
  if (dloss_ddepth)
    hipLaunchKernelGGL(k_normal_grad<true>, dim3(ggrid), dim3(NL_THREADS), 0, s, H, W, tiles_x, ntiles, depth, alpha,
                       cam, normals, guide, weight, smooth, alpha_min, edge_gamma, prior_scale, smooth_scale,
                       (const NlNrm*)m.nrm, grid, (const double*)m.parts, stats, dloss_ddepth, dloss_dalpha);
  else
    hipLaunchKernelGGL(k_normal_grad<false>, dim3(1), dim3(NL_THREADS), 0, s, H, W, tiles_x, ntiles, depth, alpha, cam,
                       normals, guide, weight, smooth, alpha_min, edge_gamma, prior_scale, smooth_scale,
                       (const NlNrm*)m.nrm, grid, (const double*)m.parts, stats, (float*)nullptr, (float*)nullptr);
  SIDE_HIP(hipGetLastError());
  return 0;
}
