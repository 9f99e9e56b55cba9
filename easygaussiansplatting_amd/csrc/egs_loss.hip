// egs_gau_loss (include/egs_hip.h): the fused L1 / SSIM training loss with every pixel counting once.  The <false>
// instances of the kernel bodies of egs_loss_device.h, which explains them -- the weighted arguments are nullptr / 0:
//
//   k_ssim_fwd      : the SSIM map's three derivative maps and the per-tile sums of |x-y| and S
//   k_ssim_bwd      : dL/dimage; workgroup 0 reduces the per-tile sums to loss_out[3] on its way
//   k_loss_finalize : loss_out[3] alone (dloss_dimage == NULL)
#include "egs_loss_device.h"

namespace egs {

__global__ __launch_bounds__(256) void k_ssim_fwd(int H, int W, int gx, int gy, LossWin win,
                                                  const float* __restrict__ img, const float* __restrict__ gt,
                                                  float* __restrict__ Pm, float* __restrict__ P11,
                                                  float* __restrict__ P12,
                                                  float* __restrict__ partials /* [ntiles][2] */) {
  ssim_fwd_body<false>(H, W, gx, gy, win, img, gt, Pm, P11, P12, partials, nullptr, nullptr);
}

__global__ __launch_bounds__(256) void k_loss_finalize(int nparts, const float* __restrict__ partials, float lambda,
                                                       float inv_count, float* __restrict__ loss_out) {
  __shared__ double red[2][4];
  loss_finalize(nparts, partials, lambda, inv_count, loss_out, red);
}

__global__ __launch_bounds__(256) void k_ssim_bwd(int H, int W, int gx, int gy, LossWin win,
                                                  const float* __restrict__ img, const float* __restrict__ gt,
                                                  const float* __restrict__ Pm, const float* __restrict__ P11,
                                                  const float* __restrict__ P12, float c_l1, float c_ssim,
                                                  float* __restrict__ dimg, int nparts,
                                                  const float* __restrict__ partials, float lambda, float inv_count,
                                                  float* __restrict__ loss_out) {
  ssim_bwd_body<false>(H, W, gx, gy, win, img, gt, Pm, P11, P12, c_l1, c_ssim, dimg, nparts, partials, lambda, inv_count,
                       loss_out, nullptr, nullptr, 0, 0.f);
}

}  // namespace egs

using namespace egs;

extern "C" size_t egs_gau_loss_ws_bytes(int height, int width) {
  if (height <= 0 || width <= 0) return 256;
  return loss_ws(nullptr, height, width, false).bytes;
}

extern "C" int egs_gau_loss(int height, int width, const float* image, const float* gt_image, float loss_lambda,
                            float grad_scale, void* ws, size_t ws_bytes, float* loss_out, float* dloss_dimage,
                            void* stream) {
  EGS_CHECK_ARG(height > 0 && width > 0 && image && gt_image && ws && loss_out);
  if (ws_bytes < egs_gau_loss_ws_bytes(height, width)) {
    set_error(EGS_ERR_WORKSPACE, "gau_loss workspace too small", __FILE__, __LINE__);
    return EGS_ERR_WORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  const LossWs m = loss_ws(ws, height, width, false);
  const int nb = loss_blocks(height, width);
  const LossWin win = loss_window();
  const int gx = div_up(width, TW), gy = div_up(height, TH);
  const dim3 grid(loss_grid(nb));
  EGS_LAUNCH("k_ssim_fwd", k_ssim_fwd, grid, dim3(256), s, height, width, gx, gy, win, image, gt_image, m.Pm, m.P11,
             m.P12, m.partials);
  const float inv_count = (float)(1.0 / (double)((size_t)3 * height * width));
  if (dloss_dimage) {   // (the gradient kernel's first workgroup reduces the partials on its way)
    const float c_l1 = grad_scale * (1.f - loss_lambda) * inv_count;
    const float c_ssim = -grad_scale * loss_lambda * inv_count;
    EGS_LAUNCH("k_ssim_bwd", k_ssim_bwd, grid, dim3(256), s, height, width, gx, gy, win, image, gt_image, m.Pm, m.P11,
               m.P12, c_l1, c_ssim, dloss_dimage, nb, m.partials, loss_lambda, inv_count, loss_out);
  } else {
    EGS_LAUNCH("k_loss_finalize", k_loss_finalize, dim3(1), dim3(256), s, nb, m.partials, loss_lambda, inv_count,
               loss_out);
  }
  EGS_LAUNCH_OK();
  return 0;
}
