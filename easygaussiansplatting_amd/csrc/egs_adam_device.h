// The Adam kernels and their host-side argument preparation, ONCE: egs_density.hip instantiates the dense forms
// (k_adam<false>, k_adam_sh_factored<NC, false>: libegs_hip.so, egs_adam_step / egs_adam_sh_factored) and egs_adam.hip the
// visibility-masked ones (k_adam<true>, k_adam_sh_factored<NC, true>: libegs_adam.so, include/egs_adam.h).  A Gaussian a
// masked step did not see is neither read nor written; one it saw goes through the very code of the dense instance, so the
// two agree to the bit on every visible row -- as the element update adam1, with its contraction pragma, and the gradient
// row sh_grad_row (egs_gaussian_math.h) are each written once.
#pragma once
#include <math.h>
#include <stdint.h>
#include <type_traits>

#include <hip/hip_runtime.h>

#include "egs_gaussian_math.h"

namespace egs {

constexpr int ADAM_MAX_GROUPS = 8;
constexpr int ADAM_PER_BLOCK = 256 * 4;           // floats per workgroup
struct AdamGroupDev {
  float* p; const float* g; float* m; float* v;
  int64_t count;
  float step_size, sqrt_bc2;                      // lr / (1 - b1^t), sqrt(1 - b2^t)
  int first_block;
};
struct AdamArgs {
  AdamGroupDev g[ADAM_MAX_GROUPS];
  int n_groups;
  float beta1, beta2, omb1, omb2, eps;            // omb = 1 - beta rounded from double, as torch does
};
// element index -> row: e / width as (e * magic) >> shift, exact for e < 2^31 (shift = 31 + ceil(log2 width), magic =
// ceil(2^shift / width) < 2^32: the quotient's error e (magic width - 2^shift) / (width 2^shift) stays below 1 / width)
struct RowDiv {
  uint32_t magic;
  int shift, width;
};
// What k_adam<true> takes in AdamArgs' place (k_adam<false> takes AdamArgs itself): every group is [n][div.width]
struct AdamMaskedArgs : AdamArgs {
  RowDiv div[ADAM_MAX_GROUPS];
  const uint8_t* visible;                         // [n]
};
// What k_adam_sh_factored<NC, false> takes where the masked instance takes `visible`: one byte in the padding behind
// `scale`, which nothing reads -- the other arguments stay where they were
struct NoMask {};
template <bool MASKED>
using RowMask = std::conditional_t<MASKED, const uint8_t* __restrict__, NoMask>;   // uint8 [n]

__device__ __forceinline__ void adam1(float& p, float g, float& m, float& v, const AdamArgs& A, float step_size,
                                      float sqrt_bc2) {
  // (no contraction: torch's kernels round every product, and k_adam / k_adam_sh_factored must agree to the bit
  // wherever the compiler inlines this)
#pragma clang fp contract(off)
  m = m + (g - m) * A.omb1;                       // exp_avg.lerp_(grad, 1 - beta1)
  v = v * A.beta2 + g * g * A.omb2;               // exp_avg_sq.mul_(b2).addcmul_(g, g, 1 - b2)
  const float denom = sqrtf(v) / sqrt_bc2 + A.eps;   // (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
  p -= step_size * (m / denom);
}

// ---- fused Adam -------------------------------------------------------------------------------------------------
// One launch over all groups, 1024 contiguous floats per workgroup, one float4 per lane.
// MASKED: a lane finds the rows of its four elements with one division, reads their mask bytes, and issues no load and
// no store unless one of them is visible; otherwise it updates the visible elements and writes the float4 back whole (a
// float4 has one owner: the untouched elements are rewritten with their own bits).
template <bool MASKED>
__global__ __launch_bounds__(256) void k_adam(std::conditional_t<MASKED, AdamMaskedArgs, AdamArgs> A) {
  int gi = 0;
#pragma unroll
  for (int k = 1; k < ADAM_MAX_GROUPS; ++k)
    if (k < A.n_groups && (int)blockIdx.x >= A.g[k].first_block) gi = k;
  const AdamGroupDev G = A.g[gi];
  const int64_t e0 = ((int64_t)(blockIdx.x - G.first_block) * 256 + threadIdx.x) * 4;
  if (e0 >= G.count) return;
  bool vis[4] = {!MASKED, !MASKED, !MASKED, !MASKED};
  [[maybe_unused]] int nel = 4;                   // MASKED: how many of e0 .. e0 + 3 lie inside the tensor
  if constexpr (MASKED) {
    // the rows of those elements (count = n width: every element has a row < n)
    const RowDiv D = A.div[gi];
    nel = (int)(G.count - e0 < 4 ? G.count - e0 : 4);
    int row = (int)(((uint64_t)(uint32_t)e0 * D.magic) >> D.shift);
    int rem = (int)e0 - row * D.width;
    bool cur = A.visible[row] != 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (q < nel) vis[q] = cur;
      if (++rem == D.width && q + 1 < nel) {
        rem = 0;
        cur = A.visible[++row] != 0;
      }
    }
    if (!(vis[0] | vis[1] | vis[2] | vis[3])) return;
  }
  auto one = [&](int64_t e) {                     // an element of the ragged tail
    float p = G.p[e], m = G.m[e], v = G.v[e];
    adam1(p, G.g[e], m, v, A, G.step_size, G.sqrt_bc2);
    G.p[e] = p; G.m[e] = m; G.v[e] = v;
  };
  // (the masked instance asks `nel` where the dense one asks G.count, here and in the tail: the same questions, but
  // with the count dead after the mask bytes are on their way, hipcc overlaps their latency with the row arithmetic --
  // 1.5 % of a step at 5 % visible rows)
  if (MASKED ? nel == 4 : e0 + 4 <= G.count) {    // tensors come from the torch allocator: 16-B aligned
    float4 p = *(float4*)(G.p + e0), m = *(float4*)(G.m + e0), v = *(float4*)(G.v + e0);
    const float4 g = *(const float4*)(G.g + e0);
    if (vis[0]) adam1(p.x, g.x, m.x, v.x, A, G.step_size, G.sqrt_bc2);
    if (vis[1]) adam1(p.y, g.y, m.y, v.y, A, G.step_size, G.sqrt_bc2);
    if (vis[2]) adam1(p.z, g.z, m.z, v.z, A, G.step_size, G.sqrt_bc2);
    if (vis[3]) adam1(p.w, g.w, m.w, v.w, A, G.step_size, G.sqrt_bc2);
    *(float4*)(G.p + e0) = p; *(float4*)(G.m + e0) = m; *(float4*)(G.v + e0) = v;
  } else if constexpr (MASKED) {
#pragma unroll
    for (int q = 0; q < 3; ++q)
      if (q < nel && vis[q]) one(e0 + q);
  } else {
    for (int64_t e = e0; e < G.count; ++e) one(e);
  }
}

// ---- Adam on the SH coefficients straight from the factored gradient -------------------------------------------
// A step that kept its SH gradient factored (EGS_BWD_FACTORED_SH: dL/dcolour [N][3] per view, egs_hip.h) never needs
// the 4 sh_dim-byte rows in HBM: one wave of the workgroup forms the rows of 64 Gaussians in LDS -- sh_grad_row, the
// arithmetic of k_sh_grad_views -- and all four waves run torch's Adam update over the 64 x K contiguous elements of
// param / exp_avg / exp_avg_sq (7 x 4 B per element instead of 8 plus the rows' write: 1344 + 12 V bytes per Gaussian at
// degree 3 where k_sh_grad_views + k_adam move 1728 + 12 V).
// MASKED: every wave reads the 64 mask bytes itself (one cache line; no barrier) and a workgroup with nothing visible
// returns before it touches pws, rows or the tensors.  Otherwise the rows of the VISIBLE Gaussians are formed and the
// float4s that hold a visible element are updated (at width 45 a float4 can span two rows).
constexpr int ASH_ROWS = 64;                      // Gaussians per workgroup
struct AdamShTensor {
  float *p, *m, *v;                               // [N][width]
  float step_size, sqrt_bc2;
  int width;                                      // floats per Gaussian; 0: tensor absent
  int col0;                                       // first column of the K-wide row it holds (0: low / whole, 3: high)
};

template <int NC, bool MASKED>
__global__ __launch_bounds__(256) void k_adam_sh_factored(int n, int views, const float* __restrict__ pws,
                                                          const float* __restrict__ rows, int64_t stride, float scale,
                                                          RowMask<MASKED> visible, AdamShTensor T0, AdamShTensor T1,
                                                          AdamArgs A) {
  constexpr int K = 3 * NC;
  __shared__ float g[ASH_ROWS * K];
  const int base = blockIdx.x * ASH_ROWS;
  const int here = min(ASH_ROWS, n - base);
  bool seen = true;                                 // MASKED: row base + lane exists and is visible
  unsigned long long mask = ~0ull;                  // bit r: row base + r is visible; the same in every wave
  if constexpr (MASKED) {
    const int lane = threadIdx.x & 63;
    seen = lane < here && visible[base + lane] != 0;
    mask = __ballot(seen);
    if (mask == 0ull) return;
  }
  if (threadIdx.x < ASH_ROWS) {
    float gsh[K];
#pragma unroll
    for (int k = 0; k < K; ++k) gsh[k] = 0.f;
    const int i = base + threadIdx.x;
    if (MASKED ? seen : i < n) sh_grad_row<NC>(ld3(pws + 3 * (size_t)i), rows, stride, views, n, i, scale, gsh);
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
        vis[q] = !MASKED || (e0 + q < cnt && ((mask >> r) & 1ull) != 0ull);
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

// ---- host side: what the four C entry points put into those arguments -------------------------------------------
// These report nothing: a caller wraps a `false` in its own library's argument check.
static inline void adam_fill_betas(AdamArgs& A, double beta1, double beta2, double eps) {
  A.n_groups = 0; A.beta1 = (float)beta1; A.beta2 = (float)beta2; A.eps = (float)eps;
  A.omb1 = (float)(1.0 - beta1); A.omb2 = (float)(1.0 - beta2);
}

// torch's bias corrections for the step-th update (1-based), in double as torch derives them
static inline void adam_bias(double lr, int step, double beta1, double beta2, float* step_size, float* sqrt_bc2) {
  const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
  *step_size = (float)(lr / bc1);
  *sqrt_bc2 = (float)sqrt(bc2);
}

// one group of k_adam; returns the workgroups it takes (the caller's next first_block)
static inline int64_t adam_fill_group(AdamGroupDev& d, float* p, const float* g, float* m, float* v, int64_t count,
                                      float lr, int step, double beta1, double beta2, int64_t first_block) {
  d.p = p; d.g = g; d.m = m; d.v = v; d.count = count;
  adam_bias((double)lr, step, beta1, beta2, &d.step_size, &d.sqrt_bc2);
  d.first_block = (int)first_block;
  return (count + ADAM_PER_BLOCK - 1) / ADAM_PER_BLOCK;
}

static inline bool adam_aligned16(const void* a, const void* b, const void* c, const void* d = nullptr) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) == 0;
}

// one tensor of k_adam_sh_factored from its group (`grad` ignored); g == NULL: the tensor is absent.  false: a null or
// misaligned pointer, step < 1, or a count that is not n x width.
static inline bool adam_fill_sh_tensor(AdamShTensor* t, const EgsAdamGroup* g, int n, int width, int col0, double beta1,
                                double beta2) {
  t->width = 0; t->col0 = col0; t->p = t->m = t->v = nullptr; t->step_size = 0.f; t->sqrt_bc2 = 1.f;
  if (!g) return true;
  if (!(g->param && g->exp_avg && g->exp_avg_sq && g->step >= 1 && g->count == (int64_t)n * width)) return false;
  if (!adam_aligned16(g->param, g->exp_avg, g->exp_avg_sq)) return false;
  t->p = g->param; t->m = g->exp_avg; t->v = g->exp_avg_sq; t->width = width;
  adam_bias((double)g->lr, g->step, beta1, beta2, &t->step_size, &t->sqrt_bc2);
  return true;
}

}  // namespace egs
