"""Depth supervision: a loss between the render's depth / opacity maps (``RenderOptions(depth=True, alpha=True)``:
depth = sum w z, alpha = sum w) and a per-pixel depth PRIOR given as disparity (inverse depth; 0, negative or non-finite:
no data), DESIGN §3.17.  Two HIP launches (csrc/egs_depthloss.hip, libegs_depthloss.so) that also produce dloss/ddepth
and dloss/dalpha, the fit of a scale-and-shift-free prior solved on the device: the host reads nothing back.

The rendered disparity of a pixel is r = alpha / depth.  A pixel counts when its prior is positive and finite,
alpha > ``alpha_min`` and depth > 0.  ``kind``:

  "metric"   the prior is in the scene's units: loss = mean |r - q|
  "affine"   the prior is known up to scale and shift (a monocular network): loss = mean |r - (s q + t)| with (s, t) the
             least-squares fit of this call, held constant in the gradient
  "pearson"  loss = 1 - correlation(q, r), with its exact gradient

(means weighted by ``weight`` over the counting pixels).  ``alpha_min`` = 0.05 keeps the 1 / depth^2 factor of the
gradient away from almost-empty pixels; NOBODY HAS TUNED IT.

    from easygaussiansplatting_amd.depthloss import depth_loss
    image, mask, depth, alpha = GSFunction.apply(..., cam, RenderOptions(depth=True, alpha=True))
    (gau_loss(image, gt) + 0.1 * depth_loss(depth, alpha, prior)).backward()
"""
from __future__ import annotations

import torch

from . import _depthlosslib
from ._host import _chk, _lib_on, _ptr, _stream

KINDS = tuple(_depthlosslib.KINDS)
ALPHA_MIN = 0.05          # the default guard; untuned


def _kind(kind):
    if kind not in _depthlosslib.KINDS:
        raise ValueError("kind must be one of %s, got %r" % (list(KINDS), kind))
    return _depthlosslib.KINDS[kind]


def _plane(t, name, hw=None, like=None):
    """A float32 plane of a call as [H,W]: [H,W] or [1,H,W] in, of the size ``hw`` and on the device of ``like`` when
    given.  ValueError otherwise.  The VALUES are not looked at (that would be a host synchronisation per call)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor, got %s" % (name, type(t).__name__))
    if t.dtype != torch.float32:
        raise ValueError("%s must be torch.float32, got %s" % (name, t.dtype))
    if t.dim() == 3 and t.shape[0] == 1:
        t = t[0]
    if t.dim() != 2 or t.numel() == 0 or (hw is not None and tuple(t.shape) != tuple(hw)):
        raise ValueError("%s must have shape %s, got %s" % (name, "[H, W] or [1, H, W]" if hw is None else list(hw),
                                                            list(t.shape)))
    if like is not None and t.device != like.device:
        raise ValueError("%s lives on %s, depth on %s" % (name, t.device, like.device))
    return t


def depth_loss_with_grad(depth, alpha, prior, kind="affine", weight=None, alpha_min=ALPHA_MIN, grad_scale=1.0,
                         need_grad=True):
    """-> (stats[6] = {loss, s, t, sum of weights, rho (0 unless "pearson"), degenerate flag} device tensor,
    grad_scale * dloss/ddepth [1,H,W] or None, grad_scale * dloss/dalpha [1,H,W] or None).

    ``depth``, ``alpha``: [1,H,W] (or [H,W]) float32, the render's maps; ``prior`` [H,W] float32 disparity; ``weight``
    [H,W] float32 >= 0 or None.  Shapes, dtypes and devices are checked (ValueError), values are not.  A call without a
    counting pixel gives loss 0 and zero gradients; "affine" on a constant prior falls back to a scale alone, "pearson"
    on a constant prior or render gives loss 1 and zero gradients (stats[5] = 1 in each case).  A training loop that
    knows the factor in front of the loss passes it as ``grad_scale`` and hands the two planes to
    ``torch.autograd.backward`` next to dloss/dimage: no autograd node for the loss."""
    k = _kind(kind)
    d = _plane(depth, "depth")
    H, W = int(d.shape[0]), int(d.shape[1])
    a = _plane(alpha, "alpha", (H, W), d)
    q = _plane(prior, "prior", (H, W), d)
    w = None if weight is None else _plane(weight, "weight", (H, W), d)
    alpha_min, grad_scale = float(alpha_min), float(grad_scale)
    if not 0.0 <= alpha_min < float("inf"):
        raise ValueError("alpha_min must be finite and >= 0, got %r" % (alpha_min,))
    d = _chk(d, "depth", torch.float32, (H, W))
    _lib_on(d)
    a, q = a.contiguous(), q.contiguous()
    w = None if w is None else w.contiguous()
    lib = _depthlosslib.load()
    dev = d.device
    stats = torch.empty(6, dtype=torch.float32, device=dev)
    dd = torch.empty((1, H, W), dtype=torch.float32, device=dev) if need_grad else None
    da = torch.empty((1, H, W), dtype=torch.float32, device=dev) if need_grad else None
    ws_bytes = lib.egs_depthloss_ws_bytes(H, W)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    _depthlosslib.check(lib.egs_depthloss(H, W, _ptr(d), _ptr(a), _ptr(q), _ptr(w), k, alpha_min, grad_scale, _ptr(ws),
                                          ws_bytes, _ptr(stats), _ptr(dd), _ptr(da), _stream()))
    return stats, dd, da


class _DepthLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, alpha, prior, kind, weight, alpha_min):
        need = depth.requires_grad or alpha.requires_grad
        stats, dd, da = depth_loss_with_grad(depth.detach(), alpha.detach(), prior.detach(), kind,
                                             None if weight is None else weight.detach(), alpha_min, 1.0, need)
        ctx.save_for_backward(dd, da)
        ctx.shapes = (depth.shape, alpha.shape)
        return stats[0]

    @staticmethod
    def backward(ctx, g):
        dd, da = ctx.saved_tensors
        if dd is None:
            return None, None, None, None, None, None
        return ((dd * g).reshape(ctx.shapes[0]) if ctx.needs_input_grad[0] else None,
                (da * g).reshape(ctx.shapes[1]) if ctx.needs_input_grad[1] else None, None, None, None, None)


def depth_loss(depth, alpha, prior, kind="affine", weight=None, alpha_min=ALPHA_MIN):
    """The loss of ``depth_loss_with_grad`` as a scalar tensor, differentiable in ``depth`` and ``alpha`` (no gradient
    flows into ``prior`` or ``weight``)."""
    return _DepthLoss.apply(depth, alpha, prior, kind, weight, alpha_min)
