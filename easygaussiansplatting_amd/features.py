"""Per-Gaussian feature vectors rendered through the tile lists of a finished forward pass (DESIGN §3.13,
include/egs_feat.h).

The draw pass blends three colour channels with the weights ``w = tau alpha'``.  Semantic or language feature fields,
label lifting from 2D masks and attribute maps need an arbitrary per-Gaussian vector ``f_g`` in R^C carried through the
same weights.  ``egs_feature_render`` (libegs_feat.so) walks the lists of a finished forward pass again, bounded by its
``contrib``, and blends C channels; ``egs_feature_gather`` is its adjoint:

    image, mask, state = fused.forward(pws, shs, alphas, scales, rots, cam, need_grad=False)
    fmap = render_features(state, feats)                 # [C,H,W] = sum_k w_k feats[g_k]
    grad = gather_features(state, gmap)                  # [N,C]   = sum_p sum_k w_k gmap[:, p]
    fmap = FeatureRender.apply(feats, state)             # differentiable with respect to ``feats``
    feats, seen = lift(states, maps)                     # training-free lifting of 2D maps onto the Gaussians

GEOMETRY IS FROZEN: the render is differentiable with respect to the features only.  There is no background and no
normalisation: a caller who wants the expected feature divides by ``1 - state.final_tau``.  The render is bitwise
reproducible; the gather is one float atomic add per (tile, Gaussian, channel) and reproducible only when every Gaussian
lies on one tile of one view.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _featlib
from ._host import _chk, _pol, _ptr, _splat_lists, _state_lists, _stream


def _channels(c, what):
    if not 1 <= c <= _featlib.MAX_CHANNELS:
        raise ValueError("%s: the channel count must lie in [1, %d], got %d" % (what, _featlib.MAX_CHANNELS, c))
    return c


def _render(n, W, H, rec, ranges, gsid, contrib, flags, feats):
    c = feats.shape[1]
    fmap = torch.empty((c, H, W), dtype=torch.float32, device=feats.device)    # the kernel writes every pixel
    lib = _featlib.load()
    _featlib.check(lib.egs_feature_render(n, W, H, _ptr(rec), C.byref(_pol()), _ptr(ranges), _ptr(gsid), _ptr(contrib),
                                          flags, c, _ptr(feats), _ptr(fmap), _stream()))
    return fmap


def _gather(n, W, H, rec, ranges, gsid, contrib, flags, gmap, out):
    c = gmap.shape[0]
    if out is None:
        out = torch.zeros((n, c), dtype=torch.float32, device=gmap.device)
    else:
        if isinstance(out, torch.Tensor) and not out.is_contiguous():
            raise ValueError("out must be contiguous: the result is accumulated into the caller's own buffer")
        out = _chk(out, "out", torch.float32, (n, c))
        if out.device != gmap.device:
            raise ValueError("out lives on %s, gmap on %s" % (out.device, gmap.device))
    lib = _featlib.load()
    _featlib.check(lib.egs_feature_gather(n, W, H, _ptr(rec), C.byref(_pol()), _ptr(ranges), _ptr(gsid), _ptr(contrib),
                                          flags, c, _ptr(gmap), _ptr(out), _stream()))
    return out


def render_features(state, feats) -> torch.Tensor:
    """-> float32 [C,H,W]: ``feats`` ([N,C] float32) blended with the weights of one fused render.  ``state`` is the
    ``fused.FusedState`` of ``fused.forward(..., need_grad=False)`` or of a training forward, under the current raster
    policy.  Settles the render's ticket, then walks its own records and lists on the current stream."""
    feats = _chk(feats, "feats", torch.float32, (state.depths.shape[0], None))
    _channels(feats.shape[1], "render_features")
    if feats.device != state.depths.device:
        raise ValueError("feats lives on %s, the state on %s" % (feats.device, state.depths.device))
    return _render(*_state_lists(state), feats.detach())


def gather_features(state, gmap, out=None) -> torch.Tensor:
    """-> float32 [N,C]: the adjoint of ``render_features``, ``sum_p sum_k w_k(p) gmap[:, p]`` per Gaussian.  ``gmap``
    is float32 [C,H,W].  With ``out`` ([N,C] float32, contiguous) the result is ADDED to it and it is returned."""
    gmap = _chk(gmap, "gmap", torch.float32, (None, int(state.height), int(state.width)))
    _channels(gmap.shape[0], "gather_features")
    if gmap.device != state.depths.device:
        raise ValueError("gmap lives on %s, the state on %s" % (gmap.device, state.depths.device))
    return _gather(*_state_lists(state), gmap.detach(), out)


class FeatureRender(torch.autograd.Function):
    """``FeatureRender.apply(feats, state)`` -> [C,H,W], differentiable with respect to ``feats`` only: the render is
    linear in the features, so its backward is ``gather_features`` of the incoming map."""

    @staticmethod
    def forward(ctx, feats, state):
        ctx.state = state
        return render_features(state, feats)

    @staticmethod
    def backward(ctx, gmap):
        grad = gather_features(ctx.state, gmap.contiguous()) if ctx.needs_input_grad[0] else None
        return grad, None


def render(feats, pws, shs, alphas, scales, rots, cam, high_shs=None, antialiased=False) -> torch.Tensor:
    """One ``fused.forward`` of ``cam`` (no gradient: the geometry is frozen) plus ``FeatureRender``: -> [C,H,W],
    differentiable with respect to ``feats``.  Arguments after ``feats`` as ``fused.forward``."""
    from . import fused
    with torch.no_grad():
        out = fused.forward(pws, shs, alphas, scales, rots, cam, high_shs=high_shs, need_grad=False,
                            antialiased=antialiased)
    return FeatureRender.apply(feats, out[2])


def _splat_args(*args):
    """``_host._splat_lists`` as (n, H, W, rec, ranges, gsid, contrib), the form tests/test_gpu_features.py takes"""
    n, W, H, rec, ranges, gsid, contrib, _ = _splat_lists(*args)
    return n, H, W, rec, ranges, gsid, contrib


@torch.no_grad()
def splat_features(H, W, us, cinv2ds, alphas, depths, contrib, ranges, gsid, feats, areas=None) -> torch.Tensor:
    """-> [C,H,W]: ``feats`` ([N,C]) blended with the weights of one ``gsplatcu.splat`` under the current policy, from
    its inputs and its outputs ``contrib``, ``patch_range_per_tile`` and ``gsid_per_patch`` (plain lists).  ``areas``
    ([N,2] int32, as ``splat`` left them) is needed under the pixel-box policy, as for ``splatB``."""
    lists = _splat_lists(H, W, us, cinv2ds, alphas, depths, contrib, ranges, gsid, areas, "splat_features")
    feats = _chk(feats, "feats", torch.float32, (lists[0], None))
    _channels(feats.shape[1], "splat_features")
    return _render(*lists, feats)


@torch.no_grad()
def splat_gather(H, W, us, cinv2ds, alphas, depths, contrib, ranges, gsid, gmap, areas=None, out=None) -> torch.Tensor:
    """-> [N,C]: the adjoint of ``splat_features`` for ``gmap`` ([C,H,W]); with ``out`` the result is added to it."""
    lists = _splat_lists(H, W, us, cinv2ds, alphas, depths, contrib, ranges, gsid, areas, "splat_gather")
    gmap = _chk(gmap, "gmap", torch.float32, (None, lists[2], lists[1]))
    _channels(gmap.shape[0], "splat_gather")
    return _gather(*lists, gmap, out)


@torch.no_grad()
def lift(states, maps, eps=1e-8):
    """One-shot, training-free lifting of 2D maps onto the Gaussians:
    ``f_g = sum_v sum_p w F_v(p) / sum_v sum_p w`` over the views ``states`` (one ``FusedState`` each) and their maps
    (float32 [C,H_v,W_v] each).  One gather of C + 1 channels per view: the last plane is all ones and carries the
    denominator.  -> (feats float32 [N,C], seen bool [N]): ``seen`` marks the rows whose denominator reaches ``eps``,
    ``feats`` is 0 elsewhere."""
    states, maps = list(states), list(maps)
    if len(states) == 0 or len(states) != len(maps):
        raise ValueError("lift: %d states against %d maps (at least one of each)" % (len(states), len(maps)))
    acc, c = None, None
    for v, (state, fmap) in enumerate(zip(states, maps)):
        fmap = _chk(fmap, "maps[%d]" % v, torch.float32, (c, int(state.height), int(state.width)))
        if c is None:
            c = fmap.shape[0]
            _channels(c + 1, "lift")
        planes = torch.cat((fmap, torch.ones_like(fmap[:1])), 0)
        if acc is not None and acc.shape[0] != state.depths.shape[0]:
            raise ValueError("lift: view %d has %d Gaussians, the views before it %d"
                             % (v, state.depths.shape[0], acc.shape[0]))
        acc = gather_features(state, planes, out=acc)
    den = acc[:, c]
    seen = den >= eps
    feats = torch.where(seen[:, None], acc[:, :c] / den.clamp_min(eps)[:, None], torch.zeros_like(acc[:, :c]))
    return feats.contiguous(), seen
