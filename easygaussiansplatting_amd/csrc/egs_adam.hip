// Visibility-masked Adam for gfx950 (include/egs_adam.h has the contract): k_sparse_adam and k_sparse_adam_sh_factored are
// k_adam and k_adam_sh_factored of egs_density.hip with a per-Gaussian mask -- a Gaussian the step did not see is
// neither read nor written, a Gaussian it saw gets the element update of egs_adam_device.h, the one the dense kernels
// apply, so the two agree to the bit on every visible row.
//
// Built into libegs_adam.so, a library of its own: it shares headers with libegs_hip.so but no symbol, and keeps its own
// last-error string.
#define EGS_SIDE_LIBRARY "egs_adam"
#include "egs_side_error.h"
#include "egs_adam_device.h"
#include "egs_gaussian_math.h"
#include "../../include/egs_adam.h"

namespace egs_adam {

using namespace egs;

static_assert(EGS_SPARSE_ADAM_MAX_GROUPS == ADAM_MAX_GROUPS, "one launch holds every group");

// element index -> row: e / width as (e * magic) >> shift, exact for e < 2^31 (shift = 31 + ceil(log2 width), magic =
// ceil(2^shift / width) < 2^32: the quotient's error e (magic width - 2^shift) / (width 2^shift) stays below 1 / width)
struct RowDiv {
  uint32_t magic;
  int shift, width;
};
struct SparseArgs {
  AdamArgs A;
  RowDiv div[ADAM_MAX_GROUPS];
  const uint8_t* visible;
};

// k_adam's shape: one launch over all groups, 1024 contiguous floats per workgroup, one float4 per lane.  A lane finds
// the rows of its four elements with one division, reads their mask bytes, and issues no load and no store unless one
// of them is visible; otherwise it updates the visible elements and writes the float4 back whole (a float4 has one
// owner: the untouched elements are rewritten with their own bits).
__global__ __launch_bounds__(256) void k_sparse_adam(SparseArgs S) {
  const AdamArgs& A = S.A;
  int gi = 0;
#pragma unroll
  for (int k = 1; k < ADAM_MAX_GROUPS; ++k)
    if (k < A.n_groups && (int)blockIdx.x >= A.g[k].first_block) gi = k;
  const AdamGroupDev G = A.g[gi];
  const RowDiv D = S.div[gi];
  const int64_t e0 = ((int64_t)(blockIdx.x - G.first_block) * 256 + threadIdx.x) * 4;
  if (e0 >= G.count) return;
  // rows of e0 .. e0 + 3, as far as they lie inside the tensor (count = n width: every element has a row < n)
  const int nel = (int)(G.count - e0 < 4 ? G.count - e0 : 4);
  int row = (int)(((uint64_t)(uint32_t)e0 * D.magic) >> D.shift);
  int rem = (int)e0 - row * D.width;
  bool vis[4] = {false, false, false, false};
  bool cur = S.visible[row] != 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (q < nel) vis[q] = cur;
    if (++rem == D.width && q + 1 < nel) {
      rem = 0;
      cur = S.visible[++row] != 0;
    }
  }
  if (!(vis[0] | vis[1] | vis[2] | vis[3])) return;
  if (nel == 4) {                                   // tensors come from the torch allocator: 16-B aligned
    float4 p = *(float4*)(G.p + e0), m = *(float4*)(G.m + e0), v = *(float4*)(G.v + e0);
    const float4 g = *(const float4*)(G.g + e0);
    if (vis[0]) adam1(p.x, g.x, m.x, v.x, A, G.step_size, G.sqrt_bc2);
    if (vis[1]) adam1(p.y, g.y, m.y, v.y, A, G.step_size, G.sqrt_bc2);
    if (vis[2]) adam1(p.z, g.z, m.z, v.z, A, G.step_size, G.sqrt_bc2);
    if (vis[3]) adam1(p.w, g.w, m.w, v.w, A, G.step_size, G.sqrt_bc2);
    *(float4*)(G.p + e0) = p; *(float4*)(G.m + e0) = m; *(float4*)(G.v + e0) = v;
  } else {
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      if (q < nel && vis[q]) {
        const int64_t e = e0 + q;
        float p = G.p[e], m = G.m[e], v = G.v[e];
        adam1(p, G.g[e], m, v, A, G.step_size, G.sqrt_bc2);
        G.p[e] = p; G.m[e] = m; G.v[e] = v;
      }
    }
  }
}

// k_adam_sh_factored with a mask: one workgroup per ASH_ROWS = 64 Gaussians.  Every wave reads the 64 mask bytes itself
// (one cache line; no barrier) and a workgroup with nothing visible returns before it touches pws, rows or the tensors.
// Otherwise one wave forms the gradient rows of the VISIBLE Gaussians in LDS and all four waves update the float4s that
// hold a visible element (at width 45 a float4 can span two rows).
template <int NC>
__global__ __launch_bounds__(256) void k_sparse_adam_sh_factored(int n, int views, const float* __restrict__ pws,
                                                                 const float* __restrict__ rows, int64_t stride,
                                                                 float scale, const uint8_t* __restrict__ visible,
                                                                 AdamShTensor T0, AdamShTensor T1, AdamArgs A) {
  constexpr int K = 3 * NC;
  __shared__ float g[ASH_ROWS * K];
  const int base = blockIdx.x * ASH_ROWS;
  const int here = min(ASH_ROWS, n - base);
  const int lane = threadIdx.x & 63;
  const bool mine = lane < here && visible[base + lane] != 0;
  const unsigned long long mask = __ballot(mine);             // bit r: row base + r is visible; the same in every wave
  if (mask == 0ull) return;
  if (threadIdx.x < ASH_ROWS) {
    float gsh[K];
#pragma unroll
    for (int k = 0; k < K; ++k) gsh[k] = 0.f;
    const int i = base + threadIdx.x;
    if (mine) {
      const f3 pw = ld3(pws + 3 * (size_t)i);
      for (int v = 0; v < views; ++v) {
        const float* row = rows + (size_t)v * stride;
        const f3 gc = ld3(row + 3 * (size_t)i);
        if (gc.x == 0.f && gc.y == 0.f && gc.z == 0.f) continue;
        const ShDir<NC> d = sh_basis_f<NC>(pw, row + 3 * (size_t)n);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          gsh[3 * c] = __builtin_fmaf(gc.x, d.B[c], gsh[3 * c]);
          gsh[3 * c + 1] = __builtin_fmaf(gc.y, d.B[c], gsh[3 * c + 1]);
          gsh[3 * c + 2] = __builtin_fmaf(gc.z, d.B[c], gsh[3 * c + 2]);
        }
      }
#pragma unroll
      for (int k = 0; k < K; ++k) gsh[k] *= scale;
    }
#pragma unroll
    for (int k = 0; k < K; ++k) g[threadIdx.x * K + k] = gsh[k];
  }
  __syncthreads();
  auto update = [&](const AdamShTensor& T) {
    if (T.width == 0) return;
    const int cnt = here * T.width;                         // this workgroup's contiguous elements of the tensor
    const size_t off = (size_t)base * T.width;              // (64 rows: every offset is a multiple of 16 bytes)
    for (int e0 = threadIdx.x * 4; e0 < cnt; e0 += 1024) {
      float gg[4];
      bool vis[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int e = min(e0 + q, cnt - 1);
        const int r = e / T.width;
        gg[q] = g[r * K + T.col0 + e % T.width];
        vis[q] = e0 + q < cnt && ((mask >> r) & 1ull) != 0ull;
      }
      if (!(vis[0] | vis[1] | vis[2] | vis[3])) continue;
      if (e0 + 4 <= cnt) {
        float4 p = *(float4*)(T.p + off + e0), m = *(float4*)(T.m + off + e0), v = *(float4*)(T.v + off + e0);
        if (vis[0]) adam1(p.x, gg[0], m.x, v.x, A, T.step_size, T.sqrt_bc2);
        if (vis[1]) adam1(p.y, gg[1], m.y, v.y, A, T.step_size, T.sqrt_bc2);
        if (vis[2]) adam1(p.z, gg[2], m.z, v.z, A, T.step_size, T.sqrt_bc2);
        if (vis[3]) adam1(p.w, gg[3], m.w, v.w, A, T.step_size, T.sqrt_bc2);
        *(float4*)(T.p + off + e0) = p; *(float4*)(T.m + off + e0) = m; *(float4*)(T.v + off + e0) = v;
      } else {
        for (int q = 0; e0 + q < cnt; ++q) {
          if (!vis[q]) continue;
          float p = T.p[off + e0 + q], m = T.m[off + e0 + q], v = T.v[off + e0 + q];
          adam1(p, gg[q], m, v, A, T.step_size, T.sqrt_bc2);
          T.p[off + e0 + q] = p; T.m[off + e0 + q] = m; T.v[off + e0 + q] = v;
        }
      }
    }
  };
  update(T0);
  update(T1);
}

static void fill_betas(AdamArgs& A, double beta1, double beta2, double eps) {
  A.n_groups = 0; A.beta1 = (float)beta1; A.beta2 = (float)beta2; A.eps = (float)eps;
  A.omb1 = (float)(1.0 - beta1); A.omb2 = (float)(1.0 - beta2);
}

static bool aligned16(const void* a, const void* b, const void* c, const void* d = nullptr) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) == 0;
}

}  // namespace egs_adam

using namespace egs_adam;

extern "C" int egs_adam_abi_version(void) { return EGS_ADAM_ABI_VERSION; }
extern "C" const char* egs_adam_last_error_string(void) { return egs_side::g_err; }

extern "C" int egs_sparse_adam_step(int n_groups, const EgsSparseAdamGroup* groups, int n, const uint8_t* visible,
                                    double beta1, double beta2, double eps, void* stream) {
  SIDE_CHECK_ARG(n_groups >= 0 && n_groups <= ADAM_MAX_GROUPS);
  SIDE_CHECK_ARG(n_groups == 0 || groups);
  SIDE_CHECK_ARG(n >= 0);
  SparseArgs S;
  fill_betas(S.A, beta1, beta2, eps);
  S.visible = visible;
  int64_t blocks = 0;
  for (int k = 0; k < n_groups; ++k) {
    const EgsSparseAdamGroup& g = groups[k];
    SIDE_CHECK_ARG(g.width > 0);
    SIDE_CHECK_ARG(g.step >= 1);
    SIDE_CHECK_ARG((int64_t)n * g.width < (int64_t)1 << 31);
    if (n == 0) continue;                            // (an empty tensor has no storage: its pointers may be null)
    SIDE_CHECK_ARG(g.param && g.grad && g.exp_avg && g.exp_avg_sq);
    SIDE_CHECK_ARG(aligned16(g.param, g.grad, g.exp_avg, g.exp_avg_sq));
    AdamGroupDev& d = S.A.g[k];
    d.p = g.param; d.g = g.grad; d.m = g.exp_avg; d.v = g.exp_avg_sq; d.count = (int64_t)n * g.width;
    const double bc1 = 1.0 - pow(beta1, (double)g.step), bc2 = 1.0 - pow(beta2, (double)g.step);
    d.step_size = (float)((double)g.lr / bc1);
    d.sqrt_bc2 = (float)sqrt(bc2);
    d.first_block = (int)blocks;
    blocks += (d.count + ADAM_PER_BLOCK - 1) / ADAM_PER_BLOCK;
    RowDiv& r = S.div[k];
    int lg = 0;
    while (((int64_t)1 << lg) < g.width) ++lg;
    r.width = g.width;
    r.shift = 31 + lg;
    r.magic = (uint32_t)((((uint64_t)1 << r.shift) + (uint64_t)g.width - 1) / (uint64_t)g.width);
    S.A.n_groups = k + 1;
  }
  if (n == 0 || n_groups == 0) return 0;
  SIDE_CHECK_ARG(visible);
  hipLaunchKernelGGL(k_sparse_adam, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, S);
  SIDE_HIP(hipGetLastError());
  return 0;
}

extern "C" int egs_sparse_adam_sh_factored(int n, int sh_dim, int views, const float* pws, const float* rows,
                                           int64_t row_stride, float scale, const EgsAdamGroup* low,
                                           const EgsAdamGroup* high, const uint8_t* visible, double beta1,
                                           double beta2, double eps, void* stream) {
  SIDE_CHECK_ARG(n >= 0 && views >= 0 && low);
  SIDE_CHECK_ARG(sh_dim == 3 || sh_dim == 12 || sh_dim == 27 || sh_dim == 48);
  if (n == 0) return 0;
  SIDE_CHECK_ARG(pws && (views == 0 || rows) && row_stride >= 3 * (int64_t)n + 3);
  SIDE_CHECK_ARG(visible);
  const bool raw = high != nullptr && sh_dim > 3;
  AdamArgs A;
  fill_betas(A, beta1, beta2, eps);
  auto tensor = [&](const EgsAdamGroup* g, int width, int col0, AdamShTensor* t) -> bool {
    t->width = 0; t->col0 = col0; t->p = t->m = t->v = nullptr; t->step_size = 0.f; t->sqrt_bc2 = 1.f;
    if (!g) return true;
    if (!(g->param && g->exp_avg && g->exp_avg_sq && g->step >= 1 && g->count == (int64_t)n * width)) return false;
    if (!aligned16(g->param, g->exp_avg, g->exp_avg_sq)) return false;
    t->p = g->param; t->m = g->exp_avg; t->v = g->exp_avg_sq; t->width = width;
    const double bc1 = 1.0 - pow(beta1, (double)g->step), bc2 = 1.0 - pow(beta2, (double)g->step);
    t->step_size = (float)((double)g->lr / bc1);
    t->sqrt_bc2 = (float)sqrt(bc2);
    return true;
  };
  AdamShTensor T0, T1;
  SIDE_CHECK_ARG(tensor(low, raw ? 3 : sh_dim, 0, &T0));
  SIDE_CHECK_ARG(tensor(raw ? high : nullptr, sh_dim - 3, 3, &T1));
  decltype(&k_sparse_adam_sh_factored<1>) kern = nullptr;
  with_sh_dim(sh_dim, [&](auto nc) { kern = k_sparse_adam_sh_factored<nc.value>; });
  hipLaunchKernelGGL(kern, dim3(div_up(n, ASH_ROWS)), dim3(256), 0, (hipStream_t)stream, n, views, pws, rows,
                     row_stride, scale, visible, T0, T1, A);
  SIDE_HIP(hipGetLastError());
  return 0;
}
