"""Host plumbing every op module shares: the raster policy (module state), validation of the callers' tensors,
output allocation from torch's caching allocator, the current HIP stream."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._lib import DRAW_MASKED_LISTS, EgsPolicy

_policy_name = "gsplatcu"
_policy = None


def _pol() -> EgsPolicy:
    if _policy is None:
        set_policy(_policy_name)
    return _policy


def set_policy(name: str) -> None:
    """Select which of the reference's pipeline definitions the ops follow:
    ``"gsplatcu"`` (gsplatcu/kernel.cu; default) or ``"forward_cpu"``
    (gsplat/gausplat.py as driven by forward_cpu.py).  ``"gsplatcu_nan_skip"``: the default with one opt-in
    deviation -- a Gaussian whose conic holds a NaN is skipped instead of blended at min(0.99, alpha) (the CUDA
    extension's ``max(0.0f, NaN) == 0``, kernel.cu:243-246): no NaN colour can reach the image."""
    global _policy, _policy_name
    lib = _lib.load()
    p = EgsPolicy()
    if name in ("gsplatcu", "gsplatcu_nan_skip"):
        lib.egs_policy_gsplatcu(C.byref(p))
        p.nan_maha = 1 if name == "gsplatcu_nan_skip" else 0
    elif name == "forward_cpu":
        lib.egs_policy_forward_cpu(C.byref(p))
    else:
        raise ValueError("unknown raster policy %r (expected 'gsplatcu', 'gsplatcu_nan_skip' or 'forward_cpu')" % (name,))
    _policy, _policy_name = p, name


def get_policy() -> str:
    return _policy_name


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _chk(t, name, dtype, shape):
    """dtype/device/shape validation; returns a contiguous tensor (a copy only
    if the caller's tensor was not contiguous, like the reference's .contiguous())."""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor, got %s" % (name, type(t).__name__))
    if not t.is_cuda:
        raise ValueError("%s must live on the GPU (got device %s)" % (name, t.device))
    if t.dtype != dtype:
        raise ValueError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if len(shape) != t.dim() or any(s is not None and s != d for s, d in zip(shape, t.shape)):
        raise ValueError("%s must have shape %s, got %s" % (name, list(shape), list(t.shape)))
    return t.contiguous()


def _out(shape, like, dtype=torch.float32):
    """Output of an op: the kernels write EVERY row (culled Gaussians as zeros, what the reference's zero-filled
    ``torch::full(..., 0)`` outputs read as, gausplat.cu:170-178), so no fill kernel runs -- torch.zeros here cost
    528 B per Gaussian and training step of pure memset."""
    return torch.empty(shape, dtype=dtype, device=like.device)


def _lib_on(t):
    lib = _lib.load()
    if t.device.index is not None and t.device.index != torch.cuda.current_device():
        raise ValueError("tensors live on %s but the current device is cuda:%d"
                         % (t.device, torch.cuda.current_device()))
    return lib


def _tiles(width, height):
    return ((width + 15) // 16) * ((height + 15) // 16)


def _alphas(alphas, n):
    if not isinstance(alphas, torch.Tensor) or alphas.numel() != n:
        raise ValueError("alphas must be a tensor of shape [N] or [N,1] with N=%d" % n)
    return _chk(alphas.reshape(n), "alphas", torch.float32, (n,))


def _state_lists(state):
    """What a walk over the tile lists of a finished fused render needs, from its ``fused.FusedState``: settles the
    render's ticket -> (n, W, H, rec, ranges, gsid, contrib, flags)."""
    state.patch_count()
    flags = DRAW_MASKED_LISTS if state.culled else 0
    return (state.depths.shape[0], int(state.width), int(state.height), state.rec, state.ranges, state.gsid,
            state.contrib, flags)


def _splat_lists(H, W, us, cinv2ds, alphas, depths, contrib, ranges, gsid, areas, what):
    """The same for one ``gsplatcu.splat`` under the current policy, from its inputs and its outputs ``contrib``,
    ``patch_range_per_tile`` and ``gsid_per_patch`` (plain lists): validates them and packs the draw records (None when
    there are no Gaussians).  ``areas`` is needed under the pixel-box policy; ``what`` names the caller in that error."""
    H, W = int(H), int(W)
    if H <= 0 or W <= 0:
        raise ValueError("height and width must be positive")
    us = _chk(us, "us", torch.float32, (None, 2))
    n = us.shape[0]
    contrib = _chk(contrib, "contrib", torch.int32, (H, W))
    ranges = _chk(ranges, "patch_range_per_tile", torch.int32, (_tiles(W, H), 2))
    gsid = _chk(gsid, "gsid_per_patch", torch.int32, (None,))
    if n == 0:
        return n, W, H, None, ranges, gsid, contrib, 0
    cinv2ds = _chk(cinv2ds, "cinv2ds", torch.float32, (n, 3))
    alphas = _alphas(alphas, n)
    _chk(depths, "depths", torch.float32, (n,))
    pol = _pol()
    if pol.footprint == 1:
        if areas is None:
            raise ValueError("%s needs `areas` under the pixel-box policy" % what)
        areas = _chk(areas, "areas", torch.int32, (n, 2))
    else:
        areas = None
    lib = _lib.load()
    rec = torch.empty((n, 12), dtype=torch.float32, device=us.device)
    colors = torch.zeros((n, 3), dtype=torch.float32, device=us.device)     # the records' colour slots: never read here
    _lib.check(lib.egs_pack_records(n, W, H, _ptr(us), _ptr(cinv2ds), _ptr(alphas), _ptr(colors), _ptr(areas),
                                    C.byref(pol), _ptr(rec), _stream()))
    return n, W, H, rec, ranges, gsid, contrib, 0
