"""Surface-normal terms on the render's depth / opacity maps (``RenderOptions(depth=True, alpha=True)``: depth = sum w z,
alpha = sum w), DESIGN §3.18: supervision of the depth map's normal by a per-pixel normal PRIOR (a monocular network's),
and an edge-aware smoothness of that normal, which needs no prior.  At most three HIP launches
(csrc/egs_normalloss.hip, libegs_normalloss.so) that also produce dloss/ddepth and dloss/dalpha; the host reads nothing
back.

A pixel with alpha > ``alpha_min`` and depth > 0 is back-projected to p = (depth / alpha) ((x - cx) / fx, (y - cy) / fy, 1);
its normal n is the normalised cross product of the central differences of p (it needs its four neighbours), in the
CAMERA frame: x right, y down, z forward, so a surface facing the camera has n_z < 0.

  prior term       mean of 1 - n . q / |q| over the pixels whose prior has data (finite, not all zero)
  smoothness term  mean of g_ab (1 - n_a . n_b) over horizontal and vertical neighbour pairs, with
                   g_ab = exp(-edge_gamma mean_c |I_a - I_b|) for a guide image I (1 without one)

(means weighted by ``weight``; include/egs_normalloss.h has every rule).  ``alpha_min`` = 0.05 and ``edge_gamma`` = 10 are
defaults NOBODY HAS TUNED.

    from easygaussiansplatting_amd.normalloss import normal_loss
    image, mask, depth, alpha = GSFunction.apply(..., cam, RenderOptions(depth=True, alpha=True))
    (gau_loss(image, gt) + 0.05 * normal_loss(depth, alpha, cam, normals=prior, guide=gt)).backward()
"""
from __future__ import annotations

import math

import torch

from . import _normallosslib
from ._host import _chk, _lib_on, _ptr, _stream
from .depthloss import _plane

ALPHA_MIN = 0.05          # the default guard; untuned
EDGE_GAMMA = 10.0         # the default edge sharpness; untuned


def _planes3(t, name, hw, like):
    """A float32 [3,H,W] input of a call, of the size ``hw`` and on the device of ``like``.  ValueError otherwise.  The
    VALUES are not looked at."""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor, got %s" % (name, type(t).__name__))
    if t.dtype != torch.float32:
        raise ValueError("%s must be torch.float32, got %s" % (name, t.dtype))
    if tuple(t.shape) != (3,) + tuple(hw):
        raise ValueError("%s must have shape %s, got %s" % (name, [3] + list(hw), list(t.shape)))
    if t.device != like.device:
        raise ValueError("%s lives on %s, depth on %s" % (name, t.device, like.device))
    return t


def _intrinsics(cam):
    """(fx, fy, cx, cy) of a camera object (``function.Camera``, a scene camera) or of a 4-sequence"""
    try:
        k = (cam.fx, cam.fy, cam.cx, cam.cy) if hasattr(cam, "fx") else tuple(cam)
        k = tuple(float(v) for v in k)
    except (TypeError, ValueError):
        k = ()
    if len(k) != 4 or not all(math.isfinite(v) for v in k) or k[0] <= 0 or k[1] <= 0:
        raise ValueError("cam must give finite intrinsics (fx, fy, cx, cy) with fx, fy > 0, got %r" % (cam,))
    return k


def _call(depth, alpha, cam, normals, guide, smooth, weight, alpha_min, edge_gamma, prior_scale, smooth_scale,
          need_grad, want_normals):
    d = _plane(depth, "depth")
    H, W = int(d.shape[0]), int(d.shape[1])
    a = _plane(alpha, "alpha", (H, W), d)
    q = None if normals is None else _planes3(normals, "normals", (H, W), d)
    g = None if guide is None else _planes3(guide, "guide", (H, W), d)
    w = None if weight is None else _plane(weight, "weight", (H, W), d)
    fx, fy, cx, cy = _intrinsics(cam)
    alpha_min, edge_gamma = float(alpha_min), float(edge_gamma)
    prior_scale, smooth_scale = float(prior_scale), float(smooth_scale)
    if not 0.0 <= alpha_min < float("inf"):
        raise ValueError("alpha_min must be finite and >= 0, got %r" % (alpha_min,))
    if not 0.0 <= edge_gamma < float("inf"):
        raise ValueError("edge_gamma must be finite and >= 0, got %r" % (edge_gamma,))
    if not (math.isfinite(prior_scale) and math.isfinite(smooth_scale)):
        raise ValueError("prior_scale and smooth_scale must be finite, got %r, %r" % (prior_scale, smooth_scale))
    if H * W > _normallosslib.MAX_PIXELS:
        raise ValueError("depth has %d pixels, the normal loss takes at most %d" % (H * W, _normallosslib.MAX_PIXELS))
    d = _chk(d, "depth", torch.float32, (H, W))
    _lib_on(d)
    a = a.contiguous()
    q, g, w = (None if t is None else t.contiguous() for t in (q, g, w))
    lib = _normallosslib.load()
    dev = d.device
    stats = torch.empty(6, dtype=torch.float32, device=dev)
    dd = torch.empty((1, H, W), dtype=torch.float32, device=dev) if need_grad else None
    da = torch.empty((1, H, W), dtype=torch.float32, device=dev) if need_grad else None
    nout = torch.empty((3, H, W), dtype=torch.float32, device=dev) if want_normals else None
    ws_bytes = lib.egs_normalloss_ws_bytes(H, W)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    _normallosslib.check(lib.egs_normalloss(H, W, _ptr(d), _ptr(a), fx, fy, cx, cy, _ptr(q), _ptr(g), _ptr(w),
                                            1 if smooth else 0, alpha_min, edge_gamma, prior_scale, smooth_scale,
                                            _ptr(ws), ws_bytes, _ptr(stats), _ptr(nout), _ptr(dd), _ptr(da), _stream()))
    return stats, dd, da, nout


def normal_loss_with_grad(depth, alpha, cam, normals=None, guide=None, smooth=True, weight=None, alpha_min=ALPHA_MIN,
                          edge_gamma=EDGE_GAMMA, prior_scale=1.0, smooth_scale=1.0, need_grad=True):
    """-> (stats[6] = {L_p, L_s, Omega_p, Omega_s, number of pixels with a normal, degenerate flags} device tensor,
    d(prior_scale L_p + smooth_scale L_s)/ddepth [1,H,W] or None, .../dalpha [1,H,W] or None).

    ``depth``, ``alpha``: [1,H,W] (or [H,W]) float32, the render's maps; ``cam``: a camera with fx, fy, cx, cy (or those
    four numbers); ``normals`` [3,H,W] float32 camera-frame prior or None (no prior term; a pixel whose prior is
    non-finite or all zero has no data); ``guide`` [3,H,W] float32 or None; ``smooth``: whether the smoothness term is
    evaluated; ``weight`` [H,W] float32 >= 0 or None.  Shapes, dtypes and devices are checked (ValueError), values are
    not.  A term without a counting pixel is 0 with a zero gradient (bit 0 / bit 1 of stats[5]).  A training loop that
    knows the factors in front of the two terms passes them as the scales and hands the two planes to
    ``torch.autograd.backward`` next to dloss/dimage: no autograd node for the loss."""
    return _call(depth, alpha, cam, normals, guide, smooth, weight, alpha_min, edge_gamma, prior_scale, smooth_scale,
                 need_grad, False)[:3]


def depth_to_normals(depth, alpha, cam, alpha_min=ALPHA_MIN):
    """-> [3,H,W] float32: the camera-frame normal of the depth map, 0 where a pixel has none (the image border, a pixel
    or a neighbour with alpha <= ``alpha_min``).  For viewing: ``0.5 - 0.5 * n`` is the usual colouring.  No gradient."""
    return _call(depth, alpha, cam, None, None, False, None, alpha_min, EDGE_GAMMA, 1.0, 1.0, False, True)[3]


class _NormalLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, alpha, cam, normals, guide, smooth, weight, alpha_min, edge_gamma, prior_scale, smooth_scale):
        need = depth.requires_grad or alpha.requires_grad
        det = lambda t: None if t is None else t.detach()
        stats, dd, da = normal_loss_with_grad(depth.detach(), alpha.detach(), cam, det(normals), det(guide), smooth,
                                              det(weight), alpha_min, edge_gamma, prior_scale, smooth_scale, need)
        ctx.save_for_backward(dd, da)
        ctx.shapes = (depth.shape, alpha.shape)
        return prior_scale * stats[0] + smooth_scale * stats[1]

    @staticmethod
    def backward(ctx, g):
        dd, da = ctx.saved_tensors
        none = (None,) * 9
        if dd is None:
            return (None, None) + none
        return ((dd * g).reshape(ctx.shapes[0]) if ctx.needs_input_grad[0] else None,
                (da * g).reshape(ctx.shapes[1]) if ctx.needs_input_grad[1] else None) + none


def normal_loss(depth, alpha, cam, normals=None, guide=None, smooth=True, weight=None, alpha_min=ALPHA_MIN,
                edge_gamma=EDGE_GAMMA, prior_scale=1.0, smooth_scale=1.0):
    """``prior_scale`` L_p + ``smooth_scale`` L_s of ``normal_loss_with_grad`` as a scalar tensor, differentiable in
    ``depth`` and ``alpha`` (no gradient flows into ``normals``, ``guide`` or ``weight``)."""
    return _NormalLoss.apply(depth, alpha, cam, normals, guide, smooth, weight, alpha_min, edge_gamma,
                             float(prior_scale), float(smooth_scale))
