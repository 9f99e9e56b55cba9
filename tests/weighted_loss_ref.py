"""References, weight patterns and the comparison rule for the weighted fused loss (csrc/egs_wloss.hip: k_ssim_fwd_w /
k_ssim_bwd_w).

The definition.  x, y [3,H,W], w [H,W] >= 0 shared by the channels, S the SSIM map of the UNWEIGHTED images (11 x 11
window, zero padding, C1 = 1e-4, C2 = 9e-4: what ``loss_cases._ref`` forms):

    l1 = sum w |x - y| / (3 sum w)      ssim = sum w S / (3 sum w)      loss = (1 - lam) l1 + lam (1 - ssim)

``ref64`` / ``ref32``: that, written as ``loss_cases._ref`` is (five depthwise F.conv2d with ``oracle.gs_oracle.ssim_window``,
then autograd), in float64 and in float32.  sum w == 0 is the kernel's convention, not a formula: loss 0, ssim 1,
gradient 0.

The rule is ``loss_cases``' (``errors`` / ``bounds`` / ``check_against``: the kernel may be as far from float64 as twice
what the float32 torch form of the same formula is on the same inputs, never held tighter than GRAD_FLOOR / LOSS_FLOOR)
with one change: the floor of the gradient's unit u is 1 / (3 sum w), one fully weighted pixel's L1 gradient per unit
weight, instead of 1 / M.
"""
import numpy as np
import torch
import torch.nn.functional as F

from easygaussiansplatting_amd import scene as S
from oracle import gs_oracle as O
from tests import loss_cases as LC

PATTERNS = ("ones", "uniform", "cols61", "checker", "border", "pixel")


def make_weight(pattern, H, W, seed=0):
    """-> float32 [H,W] numpy.  ``pixel``: one weighted pixel at a tile corner, (16, 64), where the image has one --
    otherwise its last pixel."""
    w = np.zeros((H, W), np.float32)
    if pattern == "ones":
        w[:] = 1.0
    elif pattern == "uniform":                      # i.i.d. U[0, 3)
        w[:] = (3.0 * S.uniform01(900 + seed, 1, (H, W))).astype(np.float32)
    elif pattern == "cols61":                       # the edge lies inside a tile, its halo crosses x = 64
        w[:, :61] = 1.0
    elif pattern == "checker":
        yy, xx = np.mgrid[0:H, 0:W]
        w[(yy + xx) % 2 == 0] = 1.0
    elif pattern == "border":
        w[0, :] = w[-1, :] = 1.0
        w[:, 0] = w[:, -1] = 1.0
    elif pattern == "pixel":
        w[min(16, H - 1), min(64, W - 1)] = 1.0
    else:
        raise ValueError("unknown weight pattern %r" % (pattern,))
    return w


def _ref(x, y, w, lam, device, dtype):
    """-> (loss, grad tensor [3,H,W] of ``dtype`` on ``device``, ssim, sum w)."""
    as_t = lambda a: torch.as_tensor(a).to(device=device, dtype=dtype)
    gw = torch.from_numpy(O.ssim_window().astype(np.float32 if dtype == torch.float32 else np.float64)).to(device)
    w2 = (gw[:, None] @ gw[None, :]).expand(3, 1, 11, 11).contiguous()
    xr = as_t(x).detach().clone().requires_grad_(True); yr = as_t(y).detach()
    wt = as_t(w).detach()
    sw = wt.sum()
    if float(sw) == 0.0:
        return 0.0, torch.zeros_like(xr), 1.0, 0.0
    conv = lambda t: F.conv2d(t[None], w2, padding=5, groups=3)[0]
    mu1, mu2 = conv(xr), conv(yr)
    s11 = conv(xr * xr) - mu1 * mu1; s22 = conv(yr * yr) - mu2 * mu2; s12 = conv(xr * yr) - mu1 * mu2
    ss = ((2 * mu1 * mu2 + 1e-4) * (2 * s12 + 9e-4)) / ((mu1 * mu1 + mu2 * mu2 + 1e-4) * (s11 + s22 + 9e-4))
    ssim = (wt[None] * ss).sum() / (3 * sw)
    loss = (1 - lam) * (wt[None] * (xr - yr).abs()).sum() / (3 * sw) + lam * (1 - ssim)
    loss.backward()
    return float(loss.detach()), xr.grad, float(ssim.detach()), float(sw)


def ref64(x, y, w, lam=0.2, device="cpu"):
    return _ref(x, y, w, lam, device, torch.float64)


def ref32(x, y, w, lam=0.2, device="cpu"):
    return _ref(x, y, w, lam, device, torch.float32)


def grad_error(grad, grad64, sum_w):
    """max|grad - grad64| / u, u = max(max|grad64|, 1 / (3 sum w)).  NaN stays NaN."""
    g64 = torch.as_tensor(grad64).double()
    g = torch.as_tensor(grad).to(g64.device).double()
    u = max(float(g64.abs().max()), 1.0 / (3.0 * sum_w))
    d = (g - g64).abs()
    return float("nan") if bool(torch.isnan(d).any()) else float(d.max()) / u


def errors(got, want64):
    """(loss, grad, ssim[, ...]) against the float64 quadruple of ``ref64`` -> dict(e_grad, d_loss, d_ssim)"""
    return dict(e_grad=grad_error(got[1], want64[1], want64[3]), d_loss=abs(got[0] - want64[0]),
                d_ssim=abs(got[2] - want64[2]))


bounds = LC.bounds
check_against = LC.check_against
