// libegs_wloss.so (include/egs_wloss.h): the fused L1 / SSIM training loss with a weight per pixel.
// The <true> instances of the kernel bodies of egs_loss_device.h, which explains them (egs_loss.hip wraps the <false>
// ones: every pixel counting once), plus the reduction for a call without a gradient:
//
//   k_ssim_fwd_w      : the forward maps times w, per-tile sums of w |x-y| and w S, and sum(w) of every channel-0 tile
//   k_ssim_bwd_w      : every workgroup reduces the tile sums of w to sum(w) (fixed order, the same bits in each) and
//                       takes 1 / (3 sum(w)) from it; workgroup 0 writes loss_out[4]
//   k_loss_finalize_w : loss_out[4] alone (dloss_dimage == NULL)
//
// One more plane read per kernel (8 MB on top of 275 MB at 1080p); 16 B of LDS more than k_ssim_fwd (the third row of
// the per-wave sums), three workgroups per CU as there.
#define EGS_SIDE_LIBRARY "egs_wloss"
#include "egs_side_error.h"
#include "egs_loss_device.h"
#include "../../include/egs_wloss.h"

namespace egs {

__global__ __launch_bounds__(256) void k_ssim_fwd_w(int H, int W, int gx, int gy, LossWin win,
                                                    const float* __restrict__ img, const float* __restrict__ gt,
                                                    const float* __restrict__ weight, float* __restrict__ Pm,
                                                    float* __restrict__ P11, float* __restrict__ P12,
                                                    float* __restrict__ partials, float* __restrict__ wparts) {
  ssim_fwd_body<true>(H, W, gx, gy, win, img, gt, Pm, P11, P12, partials, weight, wparts);
}

__global__ __launch_bounds__(256) void k_ssim_bwd_w(int H, int W, int gx, int gy, LossWin win,
                                                    const float* __restrict__ img, const float* __restrict__ gt,
                                                    const float* __restrict__ weight, const float* __restrict__ Pm,
                                                    const float* __restrict__ P11, const float* __restrict__ P12,
                                                    float* __restrict__ dimg, int nparts,
                                                    const float* __restrict__ partials,
                                                    const float* __restrict__ wparts, float lambda, float grad_scale,
                                                    float* __restrict__ loss_out) {
  ssim_bwd_body<true>(H, W, gx, gy, win, img, gt, Pm, P11, P12, 0.f, 0.f, dimg, nparts, partials, lambda, 0.f, loss_out,
                      weight, wparts, gx * gy, grad_scale);
}

__global__ __launch_bounds__(256) void k_loss_finalize_w(int nparts, const float* __restrict__ partials, int nw,
                                                         const float* __restrict__ wparts, float lambda,
                                                         float* __restrict__ loss_out) {
  __shared__ double red[2][4];
  const double sum_w = weight_total(nw, wparts, red[0]);
  loss_finalize_weighted(nparts, partials, lambda, weighted_scale(sum_w, lambda, 1.f).inv_count, sum_w, loss_out, red);
}

}  // namespace egs

using namespace egs;

static bool aligned4(const void* a) { return ((uintptr_t)a & 3) == 0; }

extern "C" int egs_wloss_abi_version(void) { return EGS_WLOSS_ABI_VERSION; }
extern "C" const char* egs_wloss_last_error_string(void) { return egs_side::g_err; }

extern "C" size_t egs_wloss_ws_bytes(int H, int W) {
  if (H <= 0 || W <= 0 || (int64_t)H * W > EGS_WLOSS_MAX_PIXELS) return 256;
  return loss_ws(nullptr, H, W, true).bytes;
}

extern "C" int egs_wloss(int H, int W, const float* image, const float* gt, const float* weight, float lambda,
                         float grad_scale, void* ws, size_t ws_bytes, float* loss_out, float* dloss_dimage,
                         void* stream) {
  SIDE_CHECK_ARG(H > 0 && W > 0);
  SIDE_CHECK_ARG((int64_t)H * W <= EGS_WLOSS_MAX_PIXELS);
  SIDE_CHECK_ARG(image != nullptr && aligned4(image));
  SIDE_CHECK_ARG(gt != nullptr && aligned4(gt));
  SIDE_CHECK_ARG(weight != nullptr && aligned4(weight));
  SIDE_CHECK_ARG(ws != nullptr && aligned4(ws));
  SIDE_CHECK_ARG(loss_out != nullptr && aligned4(loss_out));
  SIDE_CHECK_ARG(aligned4(dloss_dimage) && (dloss_dimage == nullptr || (dloss_dimage != image && dloss_dimage != gt)));
  if (ws_bytes < egs_wloss_ws_bytes(H, W)) {
    egs_side::set_error(EGS_ERR_WORKSPACE, "wloss workspace too small", __FILE__, __LINE__);
    return EGS_ERR_WORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  const LossWs m = loss_ws(ws, H, W, true);
  const int nb = loss_blocks(H, W), nw = nb / 3;
  const LossWin win = loss_window();
  const int gx = div_up(W, TW), gy = div_up(H, TH);
  const dim3 grid(loss_grid(nb));
  hipLaunchKernelGGL(k_ssim_fwd_w, grid, dim3(256), 0, s, H, W, gx, gy, win, image, gt, weight, m.Pm, m.P11, m.P12,
                     m.partials, m.wparts);
  if (dloss_dimage)
    hipLaunchKernelGGL(k_ssim_bwd_w, grid, dim3(256), 0, s, H, W, gx, gy, win, image, gt, weight, m.Pm, m.P11, m.P12,
                       dloss_dimage, nb, m.partials, m.wparts, lambda, grad_scale, loss_out);
  else
    hipLaunchKernelGGL(k_loss_finalize_w, dim3(1), dim3(256), 0, s, nb, m.partials, nw, m.wparts, lambda, loss_out);
  SIDE_HIP(hipGetLastError());
  return 0;
}
