// libegs_depthloss.so (include/egs_depthloss.h, which states the loss): the depth-prior loss on the render's depth and
// opacity maps and its gradient.  Two memory-bound passes over the planes, the fit solved on the device:
//
//   k_depth_sums : per-workgroup partial sums {valid pixels, Omega, sum omega q, q^2, r, q r, r^2, |r - q|} in double
//   k_depth_grad : every workgroup reduces the partials (a thread's strided run, the wave, the four waves: the same bits
//                  in each) and solves the fit / the correlation from them; then dloss/ddepth and dloss/dalpha.
//                  METRIC and PEARSON have their loss from the sums; AFFINE sums omega |e| under the fit here, per
//                  workgroup, and the workgroup that finishes last (an integer ticket) adds those up in a fixed order.
//                  <false>: no gradient plane -- one workgroup, or for AFFINE the grid again without the stores.
//
// Planes are walked flat, a float4 per thread and step where every plane is 16-B aligned, the n % 4 tail (or the whole
// plane) by scalars; the grid is at most two workgroups per CU.  The per-pixel arithmetic is double: one division per
// pixel and pass, far below what the loads leave room for, and the float32 results are then the rounded exact ones.
#define EGS_SIDE_LIBRARY "egs_depthloss"
#include "egs_side_error.h"

#include <float.h>
#include <math.h>

#include "../../include/egs_depthloss.h"

namespace egs {

constexpr int NSUM = 8;                   // the partial sums of a workgroup, the order of the list above
constexpr int DL_MAX_GRID = 512;          // the workspace holds this many workgroups' partials

// what the passes need of a pixel; an invalid one is all zeros (no NaN or inf of the inputs reaches a product)
struct DepthPx { double om, q, r, inv_d; bool valid; };

__device__ __forceinline__ DepthPx depth_px(float D, float A, float q, float w, float alpha_min) {
  DepthPx p;
  p.valid = q > 0.f && q <= FLT_MAX && A > alpha_min && D > 0.f;   // (every comparison false for NaN)
  p.om = p.valid ? (double)w : 0.0;
  p.q = p.valid ? (double)q : 0.0;
  p.inv_d = p.valid ? 1.0 / (double)D : 0.0;
  p.r = p.valid ? (double)A * p.inv_d : 0.0;
  return p;
}

__device__ __forceinline__ void depth_accumulate(double (&s)[NSUM], const DepthPx& p) {
  const double oq = p.om * p.q, orr = p.om * p.r;
  s[0] += p.valid ? 1.0 : 0.0;
  s[1] += p.om;
  s[2] += oq;
  s[3] += oq * p.q;
  s[4] += orr;
  s[5] += oq * p.r;
  s[6] += orr * p.r;
  s[7] += p.om * fabs(p.r - p.q);
}

// every thread ends with the workgroup's total of each v[k]: the wave, then the four waves in order
template <int K>
__device__ __forceinline__ void depth_block_sum(double (&v)[K], double (*red)[4]) {
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

typedef float DepthVec4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float4 depth_weight4(const float* __restrict__ w, int i) {
  return w ? ((const float4*)w)[i] : make_float4(1.f, 1.f, 1.f, 1.f);
}

__global__ __launch_bounds__(256) void k_depth_sums(int n, int n4, const float* __restrict__ D,
                                                    const float* __restrict__ A, const float* __restrict__ q,
                                                    const float* __restrict__ w, float alpha_min,
                                                    double* __restrict__ parts, unsigned* __restrict__ counter) {
  __shared__ double red[NSUM][4];
  double s[NSUM] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const int first = blockIdx.x * 256 + threadIdx.x, step = gridDim.x * 256;
  for (int i = first; i < n4; i += step) {
    const float4 d = ((const float4*)D)[i], a = ((const float4*)A)[i], p = ((const float4*)q)[i];
    const float4 ww = depth_weight4(w, i);
    depth_accumulate(s, depth_px(d.x, a.x, p.x, ww.x, alpha_min));
    depth_accumulate(s, depth_px(d.y, a.y, p.y, ww.y, alpha_min));
    depth_accumulate(s, depth_px(d.z, a.z, p.z, ww.z, alpha_min));
    depth_accumulate(s, depth_px(d.w, a.w, p.w, ww.w, alpha_min));
  }
  for (int i = 4 * n4 + first; i < n; i += step)
    depth_accumulate(s, depth_px(D[i], A[i], q[i], w ? w[i] : 1.f, alpha_min));
  depth_block_sum<NSUM>(s, red);
  if (threadIdx.x == 0) {
    double* out = parts + (size_t)blockIdx.x * NSUM;
#pragma unroll
    for (int k = 0; k < NSUM; ++k) out[k] = s[k];
    if (blockIdx.x == 0) *counter = 0u;      // k_depth_grad's ticket
  }
}

// the fit (or the correlation) of a call, from the totals: the same bits in whoever computes it
struct DepthFit { double s, t, rho, loss, omega, inv_omega, qm, rm, k1, k2; int degenerate; };

__device__ __forceinline__ DepthFit depth_solve(const double (&S)[NSUM], int kind) {
  DepthFit f = {1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0};
  if (!(S[1] > 0.0)) {
    f.degenerate = 1;
    return f;
  }
  f.omega = S[1];
  f.inv_omega = 1.0 / S[1];
  f.qm = S[2] * f.inv_omega;
  f.rm = S[4] * f.inv_omega;
  const double msq = S[3] * f.inv_omega, msr = S[6] * f.inv_omega;
  const double vq = msq - f.qm * f.qm, vr = msr - f.rm * f.rm, cov = S[5] * f.inv_omega - f.qm * f.rm;
  const bool flat_q = !(vq > 1e-12 * msq), flat_r = !(vr > 1e-12 * msr);
  if (kind == EGS_DEPTHLOSS_METRIC) {
    f.loss = S[7] * f.inv_omega;
  } else if (kind == EGS_DEPTHLOSS_AFFINE) {        // (its loss: sum omega |e| under this fit, k_depth_grad)
    if (flat_q || S[0] < 2.0) {
      f.degenerate = 1;
      f.s = S[5] / S[3];                            // (sum omega q^2 > 0: omega > 0 only where q > 0)
    } else {
      f.s = cov / vq;
      f.t = f.rm - f.s * f.qm;
    }
  } else if (flat_q || flat_r) {
    f.degenerate = 1;
    f.loss = 1.0;
  } else {
    const double sq = sqrt(vq), sr = sqrt(vr);
    f.k1 = 1.0 / (sq * sr);
    f.rho = cov * f.k1;
    f.k2 = f.rho * sq / sr;
    f.loss = 1.0 - f.rho;
  }
  return f;
}

__device__ __forceinline__ void depth_write_stats(float* __restrict__ stats, const DepthFit& f, double loss) {
  stats[0] = (float)loss;
  stats[1] = (float)f.s;
  stats[2] = (float)f.t;
  stats[3] = (float)f.omega;
  stats[4] = (float)f.rho;
  stats[5] = (float)f.degenerate;
}

// -> grad_scale dloss/dr of the pixel; L1 kinds: omega |e| is added to `eabs`
__device__ __forceinline__ double depth_dr(const DepthPx& p, const DepthFit& f, int kind, double grad_scale,
                                           double& eabs) {
  const double c = grad_scale * p.om * f.inv_omega;
  if (kind == EGS_DEPTHLOSS_PEARSON) return -c * f.k1 * ((p.q - f.qm) - f.k2 * (p.r - f.rm));
  const double e = p.r - (f.s * p.q + f.t);
  eabs += p.om * fabs(e);
  return e > 0.0 ? c : (e < 0.0 ? -c : 0.0);
}

__device__ __forceinline__ void depth_out(const DepthPx& p, double g, float& dd, float& da) {
  const bool on = p.om > 0.0;
  dd = on ? (float)(-g * p.r * p.inv_d) : 0.f;
  da = on ? (float)(g * p.inv_d) : 0.f;
}

template <bool WRITE>
__global__ __launch_bounds__(256) void k_depth_grad(int n, int n4, const float* __restrict__ D,
                                                    const float* __restrict__ A, const float* __restrict__ q,
                                                    const float* __restrict__ w, int kind, float alpha_min,
                                                    float grad_scale, int nparts, const double* __restrict__ parts,
                                                    double* eparts, unsigned* counter, float* __restrict__ stats,
                                                    float* __restrict__ dD, float* __restrict__ dA) {
  __shared__ double red[NSUM][4];
  __shared__ int s_last;
  double S[NSUM] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < nparts; i += 256) {
    const double* in = parts + (size_t)i * NSUM;
#pragma unroll
    for (int k = 0; k < NSUM; ++k) S[k] += in[k];
  }
  depth_block_sum<NSUM>(S, red);
  const DepthFit f = depth_solve(S, kind);
  const bool affine = kind == EGS_DEPTHLOSS_AFFINE;
  if (!affine && blockIdx.x == 0 && threadIdx.x == 0) depth_write_stats(stats, f, f.loss);
  if (!WRITE && !affine) return;          // (one workgroup: the finalize of a call without a gradient)

  const double gs = (double)grad_scale;
  double eabs[1] = {0.0};
  const int first = blockIdx.x * 256 + threadIdx.x, step = gridDim.x * 256;
  for (int i = first; i < n4; i += step) {
    const float4 d = ((const float4*)D)[i], a = ((const float4*)A)[i], p = ((const float4*)q)[i];
    const float4 ww = depth_weight4(w, i);
    const DepthPx p0 = depth_px(d.x, a.x, p.x, ww.x, alpha_min), p1 = depth_px(d.y, a.y, p.y, ww.y, alpha_min);
    const DepthPx p2 = depth_px(d.z, a.z, p.z, ww.z, alpha_min), p3 = depth_px(d.w, a.w, p.w, ww.w, alpha_min);
    const double g0 = depth_dr(p0, f, kind, gs, eabs[0]), g1 = depth_dr(p1, f, kind, gs, eabs[0]);
    const double g2 = depth_dr(p2, f, kind, gs, eabs[0]), g3 = depth_dr(p3, f, kind, gs, eabs[0]);
    if (WRITE) {
      float4 od, oa;
      depth_out(p0, g0, od.x, oa.x);
      depth_out(p1, g1, od.y, oa.y);
      depth_out(p2, g2, od.z, oa.z);
      depth_out(p3, g3, od.w, oa.w);
      // non-temporal: written once and read by a later kernel (2 us of 21 at 1080p against plain stores)
      __builtin_nontemporal_store(DepthVec4{od.x, od.y, od.z, od.w}, (DepthVec4*)dD + i);
      __builtin_nontemporal_store(DepthVec4{oa.x, oa.y, oa.z, oa.w}, (DepthVec4*)dA + i);
    }
  }
  for (int i = 4 * n4 + first; i < n; i += step) {
    const DepthPx p = depth_px(D[i], A[i], q[i], w ? w[i] : 1.f, alpha_min);
    const double g = depth_dr(p, f, kind, gs, eabs[0]);
    if (WRITE) depth_out(p, g, dD[i], dA[i]);
  }
  if (!affine) return;

  // AFFINE: loss = sum omega |e| / Omega.  Each workgroup leaves its share; the one that takes the last ticket sees them
  // all (release before the ticket, acquire after it) and adds them in index order -- whichever workgroup that is
  depth_block_sum<1>(eabs, red);
  if (threadIdx.x == 0) {
    eparts[blockIdx.x] = eabs[0];
    __threadfence();
    s_last = atomicAdd(counter, 1u) == gridDim.x - 1;
  }
  __syncthreads();
  if (!s_last) return;
  __threadfence();
  const volatile double* ep = eparts;
  double total[1] = {0.0};
  for (int i = threadIdx.x; i < (int)gridDim.x; i += 256) total[0] += ep[i];
  depth_block_sum<1>(total, red);
  if (threadIdx.x == 0) depth_write_stats(stats, f, total[0] * f.inv_omega);
}

// ---- host side of a launch -------------------------------------------------------------------------------------------
static inline int depth_blocks(int H, int W) { return div_up(div_up((int64_t)H * W, 4), 256); }
static inline int depth_grid(int blocks) {
  static const int resident = [] {  // two workgroups per CU of the current device, within what the workspace holds
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
      cus = 256;
    return 2 * cus < DL_MAX_GRID ? 2 * cus : DL_MAX_GRID;
  }();
  return blocks < resident ? blocks : resident;
}
// The workspace of a call, 256-B aligned pieces: the partial sums [g][NSUM], AFFINE's partial sums of omega |e| [g] (both
// double), the ticket; g = min(workgroups' worth of the plane, DL_MAX_GRID).  ws == NULL asks for `bytes` alone.
struct DepthWs { double *parts, *eparts; unsigned* counter; size_t bytes; };
static inline DepthWs depth_ws(void* ws, int H, int W) {
  const int blocks = depth_blocks(H, W);
  const size_t g = (size_t)(blocks < DL_MAX_GRID ? blocks : DL_MAX_GRID);
  const size_t o_e = align_up(g * NSUM * sizeof(double), 256), o_c = o_e + align_up(g * sizeof(double), 256);
  char* base = (char*)ws;
  return {ws ? (double*)base : nullptr, ws ? (double*)(base + o_e) : nullptr, ws ? (unsigned*)(base + o_c) : nullptr,
          o_c + 256 + 256};
}

}  // namespace egs

using namespace egs;

static bool aligned_to(const void* a, uintptr_t k) { return ((uintptr_t)a & (k - 1)) == 0; }

extern "C" int egs_depthloss_abi_version(void) { return EGS_DEPTHLOSS_ABI_VERSION; }
extern "C" const char* egs_depthloss_last_error_string(void) { return egs_side::g_err; }

extern "C" size_t egs_depthloss_ws_bytes(int H, int W) {
  if (H <= 0 || W <= 0 || (int64_t)H * W > EGS_DEPTHLOSS_MAX_PIXELS) return 256;
  return depth_ws(nullptr, H, W).bytes;
}

extern "C" int egs_depthloss(int H, int W, const float* depth, const float* alpha, const float* prior,
                             const float* weight, int kind, float alpha_min, float grad_scale, void* ws, size_t ws_bytes,
                             float* stats, float* dloss_ddepth, float* dloss_dalpha, void* stream) {
  SIDE_CHECK_ARG(H > 0 && W > 0);
  SIDE_CHECK_ARG((int64_t)H * W <= EGS_DEPTHLOSS_MAX_PIXELS);
  SIDE_CHECK_ARG(depth != nullptr && aligned_to(depth, 4));
  SIDE_CHECK_ARG(alpha != nullptr && aligned_to(alpha, 4));
  SIDE_CHECK_ARG(prior != nullptr && aligned_to(prior, 4));
  SIDE_CHECK_ARG(aligned_to(weight, 4));
  SIDE_CHECK_ARG(kind == EGS_DEPTHLOSS_METRIC || kind == EGS_DEPTHLOSS_AFFINE || kind == EGS_DEPTHLOSS_PEARSON);
  SIDE_CHECK_ARG(alpha_min >= 0.f && alpha_min <= FLT_MAX);
  SIDE_CHECK_ARG(grad_scale >= -FLT_MAX && grad_scale <= FLT_MAX);
  SIDE_CHECK_ARG(ws != nullptr && aligned_to(ws, 8));
  SIDE_CHECK_ARG(stats != nullptr && aligned_to(stats, 4));
  SIDE_CHECK_ARG(aligned_to(dloss_ddepth, 4) && aligned_to(dloss_dalpha, 4));
  SIDE_CHECK_ARG((dloss_ddepth == nullptr) == (dloss_dalpha == nullptr));
  if (dloss_ddepth) {
    SIDE_CHECK_ARG(dloss_ddepth != dloss_dalpha);
    for (const float* out : {dloss_ddepth, dloss_dalpha})
      SIDE_CHECK_ARG(out != depth && out != alpha && out != prior && out != weight);
  }
  if (ws_bytes < egs_depthloss_ws_bytes(H, W)) {
    egs_side::set_error(EGS_ERR_WORKSPACE, "depthloss workspace too small", __FILE__, __LINE__);
    return EGS_ERR_WORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  const DepthWs m = depth_ws(ws, H, W);
  const int n = H * W;
  bool vec = aligned_to(depth, 16) && aligned_to(alpha, 16) && aligned_to(prior, 16) && aligned_to(weight, 16) &&
             aligned_to(dloss_ddepth, 16) && aligned_to(dloss_dalpha, 16);
  const int n4 = vec ? n / 4 : 0;
  const int grid = depth_grid(depth_blocks(H, W));
  hipLaunchKernelGGL(k_depth_sums, dim3(grid), dim3(256), 0, s, n, n4, depth, alpha, prior, weight, alpha_min, m.parts,
                     m.counter);
  if (dloss_ddepth)
    hipLaunchKernelGGL(k_depth_grad<true>, dim3(grid), dim3(256), 0, s, n, n4, depth, alpha, prior, weight, kind,
                       alpha_min, grad_scale, grid, m.parts, m.eparts, m.counter, stats, dloss_ddepth, dloss_dalpha);
  else
    hipLaunchKernelGGL(k_depth_grad<false>, dim3(kind == EGS_DEPTHLOSS_AFFINE ? grid : 1), dim3(256), 0, s, n, n4, depth,
                       alpha, prior, weight, kind, alpha_min, grad_scale, grid, m.parts, m.eparts, m.counter, stats,
                       (float*)nullptr, (float*)nullptr);
  SIDE_HIP(hipGetLastError());
  return 0;
}
