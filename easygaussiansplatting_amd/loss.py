"""Fused training loss: the counterpart of the reference's ``gau_loss``
(gsplat/pytorch_ssim.py:63-66: 0.8 * L1 + 0.2 * (1 - SSIM), 11x11 Gaussian window).

Same call, same value, same gradient; underneath two tiled HIP kernels
(csrc/egs_loss_device.h, launched by csrc/egs_loss.hip) that also produce dloss/dimage in the forward pass, so that
``loss.backward()`` hands splatB its ``dloss_dgammas`` without running five
depthwise conv2d backward passes (10.9 ms -> see DESIGN.md at 1920x1080).

    from easygaussiansplatting_amd.loss import gau_loss
    loss = gau_loss(image, gt_image)          # image: GSFunction output [3,H,W]
    loss.backward()
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._host import _chk, _lib_on, _ptr, _stream


def _weight(weight, image):
    """The weight plane of a call: [H,W] next to ``image`` [3,H,W], on its device; float32 as it is, bool / uint8 as
    0 / 1.  ValueError otherwise.  The VALUES are not looked at (that would be a host synchronisation per call)."""
    if not isinstance(weight, torch.Tensor):
        raise TypeError("weight must be a torch.Tensor, got %s" % type(weight).__name__)
    if weight.dtype not in (torch.float32, torch.bool, torch.uint8):
        raise ValueError("weight must be torch.float32, torch.bool or torch.uint8, got %s" % (weight.dtype,))
    if isinstance(image, torch.Tensor) and image.dim() == 3:
        H, W = int(image.shape[1]), int(image.shape[2])
        if tuple(weight.shape) != (H, W):
            raise ValueError("weight must have shape %s (one plane for the three channels), got %s"
                             % ([H, W], list(weight.shape)))
        if weight.device != image.device:
            raise ValueError("weight lives on %s, image on %s" % (weight.device, image.device))
    if weight.dtype != torch.float32:
        weight = (weight != 0).to(torch.float32)
    return weight.contiguous()


def gau_loss_with_grad(image, gt_image, loss_lambda=0.2, need_grad=True, grad_scale=1.0, weight=None):
    """-> (stats[3] = {loss, l1, ssim} device tensor, grad_scale * dloss_dimage [3,H,W] or None).
    A training loop that knows the factor in front of the loss (1 / views) passes it here and calls
    ``image.backward(grad)``: no autograd node for the loss, no ones-fill, no scaling pass over the image.

    ``weight`` [H,W] >= 0 (float32; bool / uint8: 0 / 1), shared by the three channels: the loss of DESIGN §3.16,
    l1 = sum w |x - y| / (3 sum w), ssim = sum w S / (3 sum w) with S the SSIM map of the unweighted images
    (csrc/egs_wloss.hip, libegs_wloss.so); ``stats`` then has 4 entries, {loss, l1, ssim, sum w}.  A pixel with w = 0
    still receives SSIM gradient from weighted pixels up to 5 px away; content more than 5 px from every weighted pixel
    influences nothing (dilate a mask by 5 px for a hard exclusion).  sum w == 0: stats {0, 0, 1, 0}, gradient 0.  Shape,
    dtype and device of ``weight`` are checked (ValueError), its values are not.  ``weight=None``: today's kernels,
    libegs_wloss.so is not loaded."""
    if weight is not None:
        weight = _weight(weight, image)
    image = _chk(image, "image", torch.float32, (3, None, None))
    H, W = int(image.shape[1]), int(image.shape[2])
    gt_image = _chk(gt_image, "gt_image", torch.float32, (3, H, W))
    lib = _lib_on(image)
    dev = image.device
    grad = torch.empty_like(image) if need_grad else None
    if weight is not None:
        from . import _wlosslib
        wlib = _wlosslib.load()
        stats = torch.empty(4, dtype=torch.float32, device=dev)
        ws_bytes = wlib.egs_wloss_ws_bytes(H, W)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        _wlosslib.check(wlib.egs_wloss(H, W, _ptr(image), _ptr(gt_image), _ptr(weight), float(loss_lambda),
                                       float(grad_scale), _ptr(ws), ws_bytes, _ptr(stats), _ptr(grad), _stream()))
        return stats, grad
    stats = torch.empty(3, dtype=torch.float32, device=dev)
    ws_bytes = lib.egs_gau_loss_ws_bytes(H, W)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    _lib.check(lib.egs_gau_loss(H, W, _ptr(image), _ptr(gt_image), float(loss_lambda), float(grad_scale), _ptr(ws),
                                ws_bytes, _ptr(stats), _ptr(grad), _stream()))
    return stats, grad


class _GauLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, gt_image, loss_lambda, weight):
        stats, grad = gau_loss_with_grad(image.detach(), gt_image.detach(), loss_lambda, image.requires_grad,
                                         weight=weight)
        ctx.save_for_backward(grad)
        return stats[0]

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return (grad * g if grad is not None else None), None, None, None


def gau_loss(image, gt_image, loss_lambda=0.2, weight=None):
    """Drop-in for reference gsplat/pytorch_ssim.py:63-66 (scalar tensor, differentiable in ``image``).  ``weight``:
    see ``gau_loss_with_grad`` (no gradient flows into it)."""
    return _GauLoss.apply(image, gt_image, loss_lambda, weight)
