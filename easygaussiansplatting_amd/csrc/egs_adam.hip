// Visibility-masked Adam for gfx950 (include/egs_adam.h has the contract): the MASKED instances of the kernel templates of
// egs_adam_device.h, whose dense instances egs_density.hip launches -- a Gaussian the step did not see is neither read
// nor written, a Gaussian it saw goes through the same kernel body, element update and gradient row as in the dense
// step, so the two agree to the bit on every visible row.
//
// Built into libegs_adam.so, a library of its own: it shares headers with libegs_hip.so but no symbol, and keeps its own
// last-error string.
#define EGS_SIDE_LIBRARY "egs_adam"
#include "egs_side_error.h"
#include "egs_adam_device.h"
#include "../../include/egs_adam.h"

using namespace egs;

static_assert(EGS_SPARSE_ADAM_MAX_GROUPS == ADAM_MAX_GROUPS, "one launch holds every group");

extern "C" int egs_adam_abi_version(void) { return EGS_ADAM_ABI_VERSION; }
extern "C" const char* egs_adam_last_error_string(void) { return egs_side::g_err; }

extern "C" int egs_sparse_adam_step(int n_groups, const EgsSparseAdamGroup* groups, int n, const uint8_t* visible,
                                    double beta1, double beta2, double eps, void* stream) {
  SIDE_CHECK_ARG(n_groups >= 0 && n_groups <= ADAM_MAX_GROUPS);
  SIDE_CHECK_ARG(n_groups == 0 || groups);
  SIDE_CHECK_ARG(n >= 0);
  AdamMaskedArgs A;
  adam_fill_betas(A, beta1, beta2, eps);
  A.visible = visible;
  int64_t blocks = 0;
  for (int k = 0; k < n_groups; ++k) {
    const EgsSparseAdamGroup& g = groups[k];
    SIDE_CHECK_ARG(g.width > 0);
    SIDE_CHECK_ARG(g.step >= 1);
    SIDE_CHECK_ARG((int64_t)n * g.width < (int64_t)1 << 31);
    if (n == 0) continue;                            // (an empty tensor has no storage: its pointers may be null)
    SIDE_CHECK_ARG(g.param && g.grad && g.exp_avg && g.exp_avg_sq);
    SIDE_CHECK_ARG(adam_aligned16(g.param, g.grad, g.exp_avg, g.exp_avg_sq));
    blocks += adam_fill_group(A.g[k], g.param, g.grad, g.exp_avg, g.exp_avg_sq, (int64_t)n * g.width, g.lr, g.step,
                              beta1, beta2, blocks);
    RowDiv& r = A.div[k];
    int lg = 0;
    while (((int64_t)1 << lg) < g.width) ++lg;
    r.width = g.width;
    r.shift = 31 + lg;
    r.magic = (uint32_t)((((uint64_t)1 << r.shift) + (uint64_t)g.width - 1) / (uint64_t)g.width);
    A.n_groups = k + 1;
  }
  if (n == 0 || n_groups == 0) return 0;
  SIDE_CHECK_ARG(visible);
  hipLaunchKernelGGL(k_adam<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, A);
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
  adam_fill_betas(A, beta1, beta2, eps);
  AdamShTensor T0, T1;
  SIDE_CHECK_ARG(adam_fill_sh_tensor(&T0, low, n, raw ? 3 : sh_dim, 0, beta1, beta2));
  SIDE_CHECK_ARG(adam_fill_sh_tensor(&T1, raw ? high : nullptr, n, sh_dim - 3, 3, beta1, beta2));
  decltype(&k_adam_sh_factored<1, true>) kern = nullptr;
  with_sh_dim(sh_dim, [&](auto nc) { kern = k_adam_sh_factored<nc.value, true>; });
  hipLaunchKernelGGL(kern, dim3(div_up(n, ASH_ROWS)), dim3(256), 0, (hipStream_t)stream, n, views, pws, rows,
                     row_stride, scale, visible, T0, T1, A);
  SIDE_HIP(hipGetLastError());
  return 0;
}
