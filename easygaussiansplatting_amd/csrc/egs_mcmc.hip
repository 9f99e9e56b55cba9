// MCMC densification for gfx950 (include/egs_mcmc.h has the formulas): "3D Gaussian Splatting as Markov Chain Monte
// Carlo" (Kheradmand et al., NeurIPS 2024) on the trainer's raw parameter tensors and Adam moments.
//
//   egs_mcmc_weights       opacity weights, dead flags, {n_dead, n_live}
//   egs_mcmc_sample        weighted sampling with replacement: a deterministic double prefix sum + binary search
//   egs_mcmc_relocate      dead rows (or appended rows) become copies of sampled rows; opacity / scale correction
//   egs_mcmc_add_reg_grad  closed-form gradient of the opacity and scale regularisers (per step)
//   egs_mcmc_add_noise     covariance-shaped position noise (per step)
//
// Built into libegs_mcmc.so, a library of its own: it shares headers with libegs_hip.so (the quaternion -> covariance
// math, the counter-based generator) but no symbol, and keeps its own last-error string.
#include <math.h>

#define EGS_SIDE_LIBRARY "egs_mcmc"
#include "egs_side_error.h"
#include "egs_gaussian_math.h"
#include "egs_rng.h"
#include "../../include/egs_mcmc.h"

static_assert(EGS_MCMC_ERR_BAD_ARG == EGS_ERR_BAD_ARG, "one bad-argument code across the libraries");

namespace egs_mcmc {

using egs::align_up;
using egs::div_up;

constexpr int NT = 6;                       // pws, low_shs, high_shs, alphas_raw, scales_raw, rots_raw
struct ParamSet { float* t[NT]; };          // same order as EgsGaussianParams
struct Widths { int w[NT]; };

__device__ __forceinline__ double sigmoid_d(float raw) { return 1.0 / (1.0 + exp(-(double)raw)); }
__device__ __forceinline__ float sigmoid_f(float raw) { return 1.f / (1.f + expf(-raw)); }

// ---- 1. weights -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_mcmc_weights(int n, const float* __restrict__ alphas_raw, float min_opacity,
                                                      int relocation, float* __restrict__ weight,
                                                      uint8_t* __restrict__ dead, int32_t* __restrict__ totals) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  bool is_dead = false;
  if (i < n) {
    const float o = sigmoid_f(alphas_raw[i]);
    is_dead = o <= min_opacity;
    dead[i] = is_dead ? 1 : 0;
    weight[i] = (relocation && is_dead) ? 0.f : o;
  }
  const unsigned long long b = __ballot(is_dead);                 // one integer atomic per wave
  const unsigned long long in = __ballot(i < n);
  if ((threadIdx.x & 63) == 0) {
    const int nd = __popcll(b), nr = __popcll(in);
    if (nd) atomicAdd(&totals[0], nd);
    if (nr - nd) atomicAdd(&totals[1], nr - nd);
  }
}

// ---- 2. sampling ----------------------------------------------------------------------------------------------------
constexpr int SCAN_ITEMS = 4;
constexpr int SCAN_ROWS = 256 * SCAN_ITEMS;   // rows per workgroup

// inclusive prefix sums (double) of this thread's SCAN_ITEMS consecutive weights within the workgroup's SCAN_ROWS rows;
// *block_total = the workgroup's sum.  The order of the additions is fixed by (n, position) alone.
__device__ __forceinline__ void block_scan_weights(const float* __restrict__ weight, int n, double out[SCAN_ITEMS],
                                                   double* smem /* >= 4 */, double* block_total) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t r0 = (int64_t)blockIdx.x * SCAN_ROWS + (int64_t)tid * SCAN_ITEMS;
  float w[SCAN_ITEMS];
  if (r0 + SCAN_ITEMS <= n) {             // rows r0.. are 16-B aligned: the torch allocator's base is, r0 % 4 == 0
    const float4 v = *(const float4*)(weight + r0);
    w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
  } else {
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) w[k] = (r0 + k < n) ? weight[r0 + k] : 0.f;
  }
  double run = 0.0;
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; ++k) { run += (double)w[k]; out[k] = run; }
  double inc = run;                       // inclusive scan of the threads' sums across the wave
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const double t = __shfl_up(inc, d, 64);
    if (lane >= d) inc += t;
  }
  if (lane == 63) smem[wave] = inc;
  __syncthreads();
  const double s0 = smem[0], s1 = smem[1], s2 = smem[2], s3 = smem[3];
  double off = 0.0;
  if (wave > 0) off += s0;
  if (wave > 1) off += s1;
  if (wave > 2) off += s2;
  *block_total = ((s0 + s1) + s2) + s3;
  __syncthreads();
  const double excl = off + (inc - run);
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; ++k) out[k] += excl;
}

__global__ __launch_bounds__(256) void k_mcmc_scan_blocks(int n, const float* __restrict__ weight,
                                                          double* __restrict__ blocksum) {
  __shared__ double sm[4];
  double out[SCAN_ITEMS], total;
  block_scan_weights(weight, n, out, sm, &total);
  if (threadIdx.x == 0) blocksum[blockIdx.x] = total;
}

// exclusive scan of the workgroup sums in place by ONE workgroup, 256 at a time with a carry; blocksum[nblocks] = total
__global__ __launch_bounds__(256) void k_mcmc_scan_sums(int nblocks, double* __restrict__ blocksum) {
  __shared__ double sm[4];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  double carry = 0.0;
  for (int base = 0; base < nblocks; base += 256) {
    const int i = base + tid;
    const double v = i < nblocks ? blocksum[i] : 0.0;
    double inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const double t = __shfl_up(inc, d, 64);
      if (lane >= d) inc += t;
    }
    if (lane == 63) sm[wave] = inc;
    __syncthreads();
    const double s0 = sm[0], s1 = sm[1], s2 = sm[2], s3 = sm[3];
    double off = 0.0;
    if (wave > 0) off += s0;
    if (wave > 1) off += s1;
    if (wave > 2) off += s2;
    __syncthreads();
    if (i < nblocks) blocksum[i] = carry + (off + (inc - v));
    carry += ((s0 + s1) + s2) + s3;
  }
  if (tid == 0) blocksum[nblocks] = carry;
}

__global__ __launch_bounds__(256) void k_mcmc_scan_apply(int n, const float* __restrict__ weight,
                                                         const double* __restrict__ blockoff,
                                                         double* __restrict__ cdf) {
  __shared__ double sm[4];
  double out[SCAN_ITEMS], total;
  block_scan_weights(weight, n, out, sm, &total);
  const double off = blockoff[blockIdx.x];
  const int64_t r0 = (int64_t)blockIdx.x * SCAN_ROWS + (int64_t)threadIdx.x * SCAN_ITEMS;
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; ++k)
    if (r0 + k < n) cdf[r0 + k] = off + out[k];
}

__global__ __launch_bounds__(256) void k_mcmc_draw(int n, int n_draws, const float* __restrict__ weight,
                                                   const double* __restrict__ cdf, const double* __restrict__ total,
                                                   uint64_t seed, uint64_t round, int32_t* __restrict__ idx) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n_draws) return;
  const double t = egs::uniform01(seed, EGS_MCMC_STREAM_SAMPLE + round, (uint64_t)j) * total[0];
  int lo = 0, hi = n - 1;                 // first i with cdf[i] > t; hi = n - 1 is the answer of last resort
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (cdf[mid] > t) hi = mid; else lo = mid + 1;
  }
  int i = lo;
  if (weight[i] == 0.f) {                 // only where rounding made cdf step across a row of weight 0 (egs_mcmc.h)
    int f = i + 1;
    while (f < n && weight[f] == 0.f) ++f;
    if (f >= n) { f = i - 1; while (f > 0 && weight[f] == 0.f) --f; }
    if (f >= 0 && f < n) i = f;
  }
  idx[j] = i;
}

// ---- 3. relocation --------------------------------------------------------------------------------------------------
// (o, s) of a Gaussian that is present N times instead of once -> raw values of each copy (egs_mcmc.h section 3)
__device__ __forceinline__ void corrected(float alpha_raw, const float* scales_raw, int N, float min_opacity,
                                          const double* __restrict__ rsq /* 1/sqrt(k+1), k < EGS_MCMC_N_MAX */,
                                          float* out_alpha_raw, float out_scales_raw[3]) {
  const double o = sigmoid_d(alpha_raw);
  double on = -expm1(log1p(-o) / (double)N);                 // 1 - (1 - o)^(1/N)
  double D = 0.0;
  for (int i = 1; i <= N; ++i) {
    double C = 1.0, p = on, sgn = 1.0;                         // C(i-1, k), o'^(k+1), (-1)^k
    for (int k = 0; k < i; ++k) {
      D += C * sgn * rsq[k] * p;
      C = C * (double)(i - 1 - k) / (double)(k + 1);           // exact in double for i - 1 <= 50
      p *= on;
      sgn = -sgn;
    }
  }
  const double ls = log(o / D);                                // s' = s o / D
#pragma unroll
  for (int c = 0; c < 3; ++c) out_scales_raw[c] = (float)((double)scales_raw[c] + ls);
  on = fmin(fmax(on, (double)min_opacity), 1.0 - 1e-6);
  *out_alpha_raw = (float)log(on / (1.0 - on));
}

__global__ __launch_bounds__(256) void k_mcmc_reloc_count(int n_rows, int n_draws, const int32_t* __restrict__ src,
                                                          int32_t* __restrict__ count) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n_draws) return;
  const int s = src[j];
  if (s >= 0 && s < n_rows) atomicAdd(&count[s], 1);
}

struct RelocArgs {
  ParamSet p, m, v;                        // m.t[0] == nullptr: no optimizer state
  Widths w;
  int n_rows, n_draws;
  const int32_t *src, *dst, *count;
  float min_opacity;
};

__global__ __launch_bounds__(256) void k_mcmc_reloc_draw(RelocArgs A) {
  __shared__ double s_rsq[EGS_MCMC_N_MAX];
  __shared__ int s_src[256], s_dst[256];
  const int tid = threadIdx.x;
  const int j = blockIdx.x * 256 + tid;
  if (tid < EGS_MCMC_N_MAX) s_rsq[tid] = 1.0 / sqrt((double)(tid + 1));
  int s = -1, d = -1;
  if (j < A.n_draws) {
    s = A.src[j]; d = A.dst[j];
    if (s < 0 || s >= A.n_rows || d < 0 || d >= A.n_rows || d == s) s = d = -1;
  }
  s_src[tid] = s; s_dst[tid] = d;
  __syncthreads();
  if (d >= 0) {
    const int N = min(A.count[s] + 1, EGS_MCMC_N_MAX);
    const float sr[3] = {A.p.t[4][3 * (size_t)s], A.p.t[4][3 * (size_t)s + 1], A.p.t[4][3 * (size_t)s + 2]};
    float a_out, s_out[3];
    corrected(A.p.t[3][s], sr, N, A.min_opacity, s_rsq, &a_out, s_out);
    A.p.t[3][d] = a_out;
#pragma unroll
    for (int c = 0; c < 3; ++c) A.p.t[4][3 * (size_t)d + c] = s_out[c];
  }
  // cooperative row copies and moment zeroing: consecutive threads move consecutive floats of a row
  const bool has_state = A.m.t[0] != nullptr;
  const int rows = min(256, A.n_draws - (int)blockIdx.x * 256);
#pragma unroll 1
  for (int t = 0; t < NT; ++t) {
    const int w = A.w.w[t];
    const bool copied = !(t == 3 || t == 4);
    for (int e = tid; e < rows * w; e += 256) {
      const int r = e / w, c = e - r * w;
      const int rd = s_dst[r];
      if (rd < 0) continue;
      const size_t at = (size_t)rd * w + c;
      if (copied) A.p.t[t][at] = A.p.t[t][(size_t)s_src[r] * w + c];
      if (has_state) { A.m.t[t][at] = 0.f; A.v.t[t][at] = 0.f; }
    }
  }
}

__global__ __launch_bounds__(256) void k_mcmc_reloc_src(RelocArgs A) {
  __shared__ double s_rsq[EGS_MCMC_N_MAX];
  const int tid = threadIdx.x;
  const int i = blockIdx.x * 256 + tid;
  if (tid < EGS_MCMC_N_MAX) s_rsq[tid] = 1.0 / sqrt((double)(tid + 1));
  __syncthreads();
  if (i >= A.n_rows) return;
  const int drawn = A.count[i];
  if (drawn < 1) return;                   // count == 1: the row stays bit for bit
  const int N = min(drawn + 1, EGS_MCMC_N_MAX);
  const float sr[3] = {A.p.t[4][3 * (size_t)i], A.p.t[4][3 * (size_t)i + 1], A.p.t[4][3 * (size_t)i + 2]};
  float a_out, s_out[3];
  corrected(A.p.t[3][i], sr, N, A.min_opacity, s_rsq, &a_out, s_out);
  A.p.t[3][i] = a_out;
#pragma unroll
  for (int c = 0; c < 3; ++c) A.p.t[4][3 * (size_t)i + c] = s_out[c];
  if (A.m.t[0] != nullptr) {
#pragma unroll 1
    for (int t = 0; t < NT; ++t) {
      const int w = A.w.w[t];
      for (int c = 0; c < w; ++c) { A.m.t[t][(size_t)i * w + c] = 0.f; A.v.t[t][(size_t)i * w + c] = 0.f; }
    }
  }
}

// ---- 4. regulariser gradients -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_mcmc_reg_grad(int n, const float* __restrict__ alphas_raw,
                                                       const float* __restrict__ scales_raw, float ko, float ks,
                                                       float* __restrict__ g_alpha, float* __restrict__ g_scale) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float o = sigmoid_f(alphas_raw[i]);
  g_alpha[i] += ko * (o * (1.f - o));
  const egs::f3 s = egs::ld3(scales_raw + 3 * (size_t)i);
  egs::f3 g = egs::ld3(g_scale + 3 * (size_t)i);
  g.x += ks * expf(s.x); g.y += ks * expf(s.y); g.z += ks * expf(s.z);
  egs::st3(g_scale + 3 * (size_t)i, g);
}

// ---- 5. position noise ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_mcmc_noise(int n, float* __restrict__ pws, const float* __restrict__ alphas_raw,
                                                    const float* __restrict__ scales_raw,
                                                    const float* __restrict__ rots_raw,
                                                    const float* __restrict__ unit_noise, float k_lr, uint64_t seed,
                                                    uint64_t step) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float z[3];
  if (unit_noise) {
#pragma unroll
    for (int c = 0; c < 3; ++c) z[c] = unit_noise[3 * (size_t)i + c];
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) z[c] = egs::unit_normal(seed, EGS_MCMC_STREAM_NOISE + step, 3ull * i + c);
  }
  const float o = sigmoid_f(alphas_raw[i]);
  const float w = 1.f / (1.f + expf(-100.f * ((1.f - o) - 0.995f)));
  const egs::f3 sr = egs::ld3(scales_raw + 3 * (size_t)i);
  const egs::f3 s = {expf(sr.x), expf(sr.y), expf(sr.z)};
  float4 q = *(const float4*)(rots_raw + 4 * (size_t)i);       // (w, x, y, z)
  const float nq = fmaxf(sqrtf(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w), 1e-12f);
  q.x /= nq; q.y /= nq; q.z /= nq; q.w /= nq;
  const egs::Cov3 cv = egs::cov3d_f(q, s);                      // c = upper triangle of R diag(s^2) R^T
  const float g = w * k_lr;
  const egs::f3 v = {z[0] * g, z[1] * g, z[2] * g};
  egs::f3 p = egs::ld3(pws + 3 * (size_t)i);
  p.x += cv.c[0] * v.x + cv.c[1] * v.y + cv.c[2] * v.z;
  p.y += cv.c[1] * v.x + cv.c[3] * v.y + cv.c[4] * v.z;
  p.z += cv.c[2] * v.x + cv.c[4] * v.y + cv.c[5] * v.z;
  egs::st3(pws + 3 * (size_t)i, p);
}

static ParamSet to_set(const EgsGaussianParams* p) {
  ParamSet s;
  if (!p) { for (int t = 0; t < NT; ++t) s.t[t] = nullptr; return s; }
  s.t[0] = p->pws; s.t[1] = p->low_shs; s.t[2] = p->high_shs;
  s.t[3] = p->alphas_raw; s.t[4] = p->scales_raw; s.t[5] = p->rots_raw;
  return s;
}

static size_t scan_blocks(int n) { return (size_t)div_up(n > 0 ? n : 1, SCAN_ROWS); }

}  // namespace egs_mcmc

using namespace egs_mcmc;

extern "C" int egs_mcmc_abi_version(void) { return EGS_MCMC_ABI_VERSION; }
extern "C" const char* egs_mcmc_last_error_string(void) { return egs_side::g_err; }

extern "C" int egs_mcmc_weights(int n, const float* alphas_raw, float min_opacity, int relocation, float* weight,
                                uint8_t* dead, int32_t* totals, void* stream) {
  SIDE_CHECK_ARG(n >= 0 && totals);
  SIDE_CHECK_ARG(n == 0 || (alphas_raw && weight && dead));
  SIDE_CHECK_ARG(min_opacity >= 0.f && min_opacity < 1.f);
  hipStream_t s = (hipStream_t)stream;
  SIDE_HIP(hipMemsetAsync(totals, 0, 2 * sizeof(int32_t), s));
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_mcmc_weights, dim3(div_up(n, 256)), dim3(256), 0, s, n, alphas_raw, min_opacity,
                     relocation != 0, weight, dead, totals);
  SIDE_HIP(hipGetLastError());
  return 0;
}

extern "C" size_t egs_mcmc_sample_ws_bytes(int n) {
  const size_t rows = n > 0 ? (size_t)n : 1;
  return align_up(rows * sizeof(double), 256) + align_up((scan_blocks(n) + 1) * sizeof(double), 256) + 256;
}

extern "C" int egs_mcmc_sample(int n, const float* weight, int n_positive, int n_draws, uint64_t seed, uint64_t round,
                               int32_t* idx, void* ws, size_t ws_bytes, void* stream) {
  SIDE_CHECK_ARG(n >= 0 && n_draws >= 0);
  if (n_draws == 0) return 0;
  SIDE_CHECK_ARG(n > 0 && n_positive > 0 && n_positive <= n);      // total == 0: nothing alive to draw from
  SIDE_CHECK_ARG(weight && idx && ws);
  SIDE_CHECK_ARG(((uintptr_t)weight & 15) == 0 && ((uintptr_t)ws & 255) == 0);
  SIDE_CHECK_ARG(ws_bytes >= egs_mcmc_sample_ws_bytes(n));
  SIDE_CHECK_ARG(round < (1ull << 61));
  const int nb = (int)scan_blocks(n);
  double* cdf = (double*)ws;
  double* blocksum = (double*)((char*)ws + align_up((size_t)n * sizeof(double), 256));
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_mcmc_scan_blocks, dim3(nb), dim3(256), 0, s, n, weight, blocksum);
  SIDE_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_mcmc_scan_sums, dim3(1), dim3(256), 0, s, nb, blocksum);
  SIDE_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_mcmc_scan_apply, dim3(nb), dim3(256), 0, s, n, weight, (const double*)blocksum, cdf);
  SIDE_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_mcmc_draw, dim3(div_up(n_draws, 256)), dim3(256), 0, s, n, n_draws, weight, (const double*)cdf,
                     (const double*)(blocksum + nb), seed, round, idx);
  SIDE_HIP(hipGetLastError());
  return 0;
}

extern "C" size_t egs_mcmc_relocate_ws_bytes(int n_rows) {
  return align_up((size_t)(n_rows > 0 ? n_rows : 1) * sizeof(int32_t), 256);
}

extern "C" int egs_mcmc_relocate(int n_rows, int n_draws, int high_sh_width, const int32_t* src, const int32_t* dst,
                                 const EgsGaussianParams* params, const EgsGaussianParams* exp_avg,
                                 const EgsGaussianParams* exp_avg_sq, float min_opacity, void* ws, size_t ws_bytes,
                                 void* stream) {
  SIDE_CHECK_ARG(n_rows >= 0 && n_draws >= 0 && high_sh_width >= 0);
  SIDE_CHECK_ARG(min_opacity >= 0.f && min_opacity < 1.f);
  SIDE_CHECK_ARG((exp_avg != nullptr) == (exp_avg_sq != nullptr));
  if (n_draws == 0 || n_rows == 0) return 0;
  SIDE_CHECK_ARG(src && dst && params && ws);
  SIDE_CHECK_ARG(ws_bytes >= egs_mcmc_relocate_ws_bytes(n_rows));
  RelocArgs A;
  A.p = to_set(params); A.m = to_set(exp_avg); A.v = to_set(exp_avg_sq);
  const bool has_state = exp_avg != nullptr;
  const int widths[NT] = {3, 3, high_sh_width, 1, 3, 4};
  for (int t = 0; t < NT; ++t) {
    A.w.w[t] = widths[t];
    if (widths[t] == 0) continue;
    SIDE_CHECK_ARG(A.p.t[t]);
    if (has_state) SIDE_CHECK_ARG(A.m.t[t] && A.v.t[t]);
  }
  if (!has_state) A.m.t[0] = nullptr;
  A.n_rows = n_rows; A.n_draws = n_draws; A.src = src; A.dst = dst; A.count = (const int32_t*)ws;
  A.min_opacity = min_opacity;
  hipStream_t s = (hipStream_t)stream;
  SIDE_HIP(hipMemsetAsync(ws, 0, (size_t)n_rows * sizeof(int32_t), s));
  hipLaunchKernelGGL(k_mcmc_reloc_count, dim3(div_up(n_draws, 256)), dim3(256), 0, s, n_rows, n_draws, src,
                     (int32_t*)ws);
  SIDE_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_mcmc_reloc_draw, dim3(div_up(n_draws, 256)), dim3(256), 0, s, A);
  SIDE_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_mcmc_reloc_src, dim3(div_up(n_rows, 256)), dim3(256), 0, s, A);
  SIDE_HIP(hipGetLastError());
  return 0;
}

extern "C" int egs_mcmc_add_reg_grad(int n, const float* alphas_raw, const float* scales_raw, float lambda_o,
                                     float lambda_s, float* g_alphas_raw, float* g_scales_raw, void* stream) {
  SIDE_CHECK_ARG(n >= 0);
  if (n == 0) return 0;
  SIDE_CHECK_ARG(alphas_raw && scales_raw && g_alphas_raw && g_scales_raw);
  hipLaunchKernelGGL(k_mcmc_reg_grad, dim3(div_up(n, 256)), dim3(256), 0, (hipStream_t)stream, n, alphas_raw,
                     scales_raw, (float)((double)lambda_o / n), (float)((double)lambda_s / (3.0 * n)), g_alphas_raw,
                     g_scales_raw);
  SIDE_HIP(hipGetLastError());
  return 0;
}

extern "C" int egs_mcmc_add_noise(int n, float* pws, const float* alphas_raw, const float* scales_raw,
                                  const float* rots_raw, const float* unit_noise, float noise_lr, float lr_pws,
                                  uint64_t seed, uint64_t step, void* stream) {
  SIDE_CHECK_ARG(n >= 0);
  if (n == 0) return 0;
  SIDE_CHECK_ARG(pws && alphas_raw && scales_raw && rots_raw);
  SIDE_CHECK_ARG(((uintptr_t)rots_raw & 15) == 0);
  SIDE_CHECK_ARG(step < (1ull << 60));
  hipLaunchKernelGGL(k_mcmc_noise, dim3(div_up(n, 256)), dim3(256), 0, (hipStream_t)stream, n, pws, alphas_raw,
                     scales_raw, rots_raw, unit_noise, noise_lr * lr_pws, seed, step);
  SIDE_HIP(hipGetLastError());
  return 0;
}
