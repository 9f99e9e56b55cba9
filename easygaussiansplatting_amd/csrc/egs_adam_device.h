// Device code the Adam kernels share: egs_density.hip (k_adam, k_adam_sh_factored: libegs_hip.so) and egs_adam.hip (their
// visibility-masked forms: libegs_adam.so).  The element update lives here ONCE, with its contraction pragma, so that
// every kernel that applies it agrees with the others to the bit.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

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

// ---- Adam on the SH coefficients straight from the factored gradient (k_adam_sh_factored) ------------------------
constexpr int ASH_ROWS = 64;                      // Gaussians per workgroup
struct AdamShTensor {
  float *p, *m, *v;                               // [N][width]
  float step_size, sqrt_bc2;
  int width;                                      // floats per Gaussian; 0: tensor absent
  int col0;                                       // first column of the K-wide row it holds (0: low / whole, 3: high)
};

}  // namespace egs
