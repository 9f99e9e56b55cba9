"""Image pairs, references and the comparison rule for the fused loss (k_ssim_fwd / k_ssim_bwd of csrc/egs_loss.hip, whose
bodies are csrc/egs_loss_device.h's).

The pairs.  ``make_pair(kind, H, W)`` -> (x, y), float32 [3,H,W], seeded from scene.normal / scene.uniform01:

    noise      x = 0.5 + 0.3 n, y = clip(x + 0.1 n', 0, 1): window variances of about 0.1, nothing cancels
    flat       0.9 against itself + 1e-3 noise: E[x^2] - mu^2 is 0.81 - 0.81 with a variance of 1e-6
    identical  smooth ramps against themselves: L1 is exactly 0, SSIM 1, the exact gradient 0
    ramps      smooth colour ramps against themselves + 2e-3 noise
    shifted    the ramps against themselves moved one pixel to the right
    dark       black against values below 0.01: mu^2 of the order of C1
    quantised  both rounded to k/255 (a PNG target), x == y on about half of the pixels: sign(0) = 0 decides
    hdr        x in [-0.5, 4] (the renderer does not clamp colours) against y in [0, 1]
    rendered   the CPU oracle's image of small_scene(1500, W, H, 12) with base colours and opacities perturbed by a
               few per cent (x) against the image of the scene itself (y): an early-training pair

The references.  ``ref64`` / ``ref32``: the reference's formulation (gsplat/pytorch_ssim.py:24-66: five depthwise
11x11 F.conv2d, then autograd), in float64 and in float32, on the device the caller names.  ``ref64`` is tied to
the analytic numpy oracle ``gs_oracle.gau_loss`` by tests/test_loss_cases_cpu.py, so that a GPU test may use it
where the numpy oracle would be slow.

The rule (``check_against``).  With M = 3 H W, u = max(max|grad64|, 1 / M), e = max|grad - grad64| / u:

    e_hip <= max(1e-4, 2 e_ref)          |loss_hip - loss64| <= max(1e-5, 2 |loss32 - loss64|)      (SSIM likewise)

The floors are the bounds tests/test_gpu_parity.py has always held this kernel to.  Above them the bound comes from
the REFERENCE's float32 evaluation of the same pair (computed on every run, never stored), not from the kernel: both
are float32 evaluations of the same cancelling differences E[x^2] - mu^2 set against C2 = 9e-4, and another
summation order of the same 121 products moves such a rounding error by about 2, not by 10.  1 / M is one pixel's
L1 gradient: the floor of u keeps ``identical`` (exact gradient 0) measurable.

What the reference's float32 does (``ref32`` on the CPU against ``gs_oracle.gau_loss``, 70x150, lambda 0.2;
re-derived, not asserted, by test_loss_cases_cpu.py::test_ref32_error_table):

    kind        |loss32 - loss64|   max|grad32 - grad64| / u
    noise            1.6e-08              1.5e-06
    flat             6.6e-05              3.1e-04
    identical        0.0e+00              5.9e-05
    ramps            3.8e-07              2.9e-04
    shifted          4.7e-07              1.9e-04
    dark             1.2e-08              4.9e-07
    quantised        3.6e-06              3.7e-04
    hdr              8.6e-08              2.5e-07
    rendered         8.3e-09              2.3e-06

so on smooth images the reference itself is 200 times less exact than on the noise the suite used to feed this
kernel, and would break a flat 1e-4.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from easygaussiansplatting_amd import scene as S
from oracle import gs_oracle as O

KINDS = ("noise", "flat", "identical", "ramps", "shifted", "dark", "quantised", "hdr", "rendered")

GRAD_FLOOR = 1e-4      # tests/test_gpu_parity.py::test_gau_loss_vs_reference_fixture: gradient, of its largest entry
LOSS_FLOOR = 1e-5      # ... loss and SSIM, absolute
REF_FACTOR = 2.0


def _ramps(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    return np.stack([0.2 + 0.7 * xx / W, 0.9 - 0.5 * yy / H, 0.5 + 0.4 * np.sin(xx / 40.0) * np.cos(yy / 30.0)])


def _to255(a):
    """Rounded to k / 255 the way an 8-bit image is read: float32(k) / 255."""
    k = np.rint(np.clip(a, 0.0, 1.0) * 255.0).astype(np.float32)
    return k / np.float32(255.0)


def _rendered(H, W, seed):
    sc = S.small_scene(1500, W, H, 12)
    img = lambda shs, alphas: O.forward_pipeline((sc.pws, sc.rots, sc.scales, alphas, shs), sc.cam,
                                                 O.POLICY_G)["image"]
    y = img(sc.shs, sc.alphas)
    shs = sc.shs.copy()
    shs[:, :3] += (0.03 * S.normal(seed, 1, (sc.n, 3))).astype(np.float32)
    alphas = np.clip(sc.alphas * (1.0 + 0.03 * S.normal(seed, 2, (sc.n,))), 0.01, 0.99).astype(np.float32)
    return img(shs, alphas), y


def make_pair(kind, H, W, seed=0):
    """-> (x, y): float32 [3,H,W], C-contiguous.  A pure function of (kind, H, W, seed)."""
    shp = (3, H, W)
    s = 100 + 10 * seed + KINDS.index(kind)
    if kind == "noise":
        x = (0.5 + 0.3 * S.normal(s, 1, shp)).astype(np.float32)
        y = np.clip(x + 0.1 * S.normal(s, 2, shp), 0, 1)
    elif kind == "flat":
        x = np.full(shp, 0.9)
        y = x + 1e-3 * S.normal(s, 1, shp)
    elif kind == "identical":
        x = _ramps(H, W)
        y = x.copy()
    elif kind == "ramps":
        x = _ramps(H, W)
        y = x + 2e-3 * S.normal(s, 1, shp)
    elif kind == "shifted":
        x = _ramps(H, W)
        y = np.roll(x, 1, 2)
    elif kind == "dark":
        x = np.zeros(shp)
        y = 0.01 * S.uniform01(s, 1, shp)
    elif kind == "quantised":
        base = _ramps(H, W)
        y = _to255(base + 0.02 * S.normal(s, 1, shp))
        x = np.where(S.uniform01(s, 3, shp) < 0.5, y, _to255(base + 0.02 * S.normal(s, 2, shp)))
    elif kind == "hdr":
        x = -0.5 + 4.5 * S.uniform01(s, 1, shp)
        y = S.uniform01(s, 2, shp)
    elif kind == "rendered":
        x, y = _rendered(H, W, s)
    else:
        raise ValueError("unknown pair kind %r" % (kind,))
    return np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32)


@functools.lru_cache(maxsize=4)
def cached_pair(kind, H, W):
    return make_pair(kind, H, W)


def _ref(x, y, lam, device, dtype):
    """(1 - lam) mean|x - y| + lam (1 - mean SSIM) as gsplat/pytorch_ssim.py states it, differentiated by autograd.
    x, y: numpy arrays or tensors [3,H,W].  -> (loss, grad tensor [3,H,W] of ``dtype`` on ``device``, ssim)."""
    as_t = lambda a: torch.as_tensor(a).to(device=device, dtype=dtype)
    gw = torch.from_numpy(O.ssim_window().astype(np.float32 if dtype == torch.float32 else np.float64)).to(device)
    w2 = (gw[:, None] @ gw[None, :]).expand(3, 1, 11, 11).contiguous()
    xr = as_t(x).detach().clone().requires_grad_(True); yr = as_t(y).detach()
    conv = lambda t: F.conv2d(t[None], w2, padding=5, groups=3)[0]
    mu1, mu2 = conv(xr), conv(yr)
    s11 = conv(xr * xr) - mu1 * mu1; s22 = conv(yr * yr) - mu2 * mu2; s12 = conv(xr * yr) - mu1 * mu2
    ss = ((2 * mu1 * mu2 + 1e-4) * (2 * s12 + 9e-4)) / ((mu1 * mu1 + mu2 * mu2 + 1e-4) * (s11 + s22 + 9e-4))
    ssim = ss.mean()
    loss = (1 - lam) * (xr - yr).abs().mean() + lam * (1 - ssim)
    loss.backward()
    return float(loss.detach()), xr.grad, float(ssim.detach())


def ref64(x, y, lam=0.2, device="cpu"):
    return _ref(x, y, lam, device, torch.float64)


def ref32(x, y, lam=0.2, device="cpu"):
    return _ref(x, y, lam, device, torch.float32)


def grad_error(grad, grad64):
    """max|grad - grad64| / u, u = max(max|grad64|, 1 / M).  Tensors (any device) or arrays; NaN stays NaN."""
    g64 = torch.as_tensor(grad64).double()
    g = torch.as_tensor(grad).to(g64.device).double()
    u = max(float(g64.abs().max()), 1.0 / g64.numel())
    d = (g - g64).abs()
    return float("nan") if bool(torch.isnan(d).any()) else float(d.max()) / u


def errors(got, want64):
    """(loss, grad, ssim) triples -> dict(e_grad, d_loss, d_ssim) of ``got`` against the float64 triple."""
    return dict(e_grad=grad_error(got[1], want64[1]), d_loss=abs(got[0] - want64[0]), d_ssim=abs(got[2] - want64[2]))


def bounds(e_ref):
    """What the rule allows the kernel, from the reference's own float32 errors on the same pair."""
    return dict(e_grad=max(GRAD_FLOOR, REF_FACTOR * e_ref["e_grad"]),
                d_loss=max(LOSS_FLOOR, REF_FACTOR * e_ref["d_loss"]),
                d_ssim=max(LOSS_FLOOR, REF_FACTOR * e_ref["d_ssim"]))


def check_against(e_hip, e_ref, what=""):
    b = bounds(e_ref)
    for k in ("e_grad", "d_loss", "d_ssim"):
        assert e_hip[k] <= b[k], "%s %s: kernel %.3e > bound %.3e (reference float32: %.3e)" % (
            what, k, e_hip[k], b[k], e_ref[k])
