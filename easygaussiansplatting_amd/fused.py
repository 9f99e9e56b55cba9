"""Fused training path: what the reference's ``GSFunction``
(gsplat/gsmodel.py:6-93) computes, in three C-ABI calls per step and without the
436 B/Gaussian of Jacobians ever crossing HBM.

* ``forward``  = project + computeCov3D + computeCov2D + sh2Color + inverseCov2D
  in ONE kernel (which also does the binning's getRects and depth keys), then ``splat``'s sort and draw;
  from the second call on the draw stage is enqueued AHEAD of the read-back of the patch count (see below);
* ``backward`` = ``splatB``'s draw pass into packed per-Gaussian gradient records
  + ONE kernel that re-derives the Jacobians in registers and applies
  backward.md eq (3)(4)(5)(7) (gsmodel.py:71-85).

Results equal the seven-op path (same device functions, csrc/egs_gaussian_math.h);
``tests/test_gpu_parity.py`` checks fused == unfused == oracle.
"""
from __future__ import annotations

import collections
import ctypes as C
import os
import weakref

import torch

from . import _ahead, _lib
# (re-exported: the scheduling state's public names, and what tests and lab tools reach through this module)
from ._ahead import (_ctx, _seg_decision, _settle, _tls, _walk_word,  # noqa: F401
                     commit, deferred, expect_long_walks, seg_hint)  # noqa: F401
from ._host import _alphas, _chk, _lib_on, _pol, _ptr, _stream, _tiles
from .dist_views import flat_grad_buffer  # noqa: F401  (re-exported: the buffer is allocated here)


ENQUEUE_AHEAD = os.environ.get("EGS_ENQUEUE_AHEAD", "1") != "0"   # knob for A/B measurements and tests
MAILBOX_COPY = os.environ.get("EGS_MAILBOX_COPY", "0") == "1"     # A/B knob: read-back by copy instead of kernel stores
REUSE_ORDER = os.environ.get("EGS_BWD_REUSE_ORDER", "1") != "0"   # A/B knob: see KEEP_FORWARD_ORDER
KEEP_FORWARD_ORDER = 16   # include/egs_hip.h EGS_BWD_KEEP_FORWARD_ORDER
ORDER_REFRESH = max(2, int(os.environ.get("EGS_TILE_ORDER_REFRESH", "4")))   # renders of a camera between order refreshes
TILE_WORK_CACHE = os.environ.get("EGS_TILE_WORK_CACHE", "1") != "0"  # A/B knob: forward dispatch order by remembered work
SAVE_DCOLOR = os.environ.get("EGS_SAVE_DCOLOR", "1") != "0"          # A/B knob: forward keeps dcolor/dpw for backward
CULL_LISTS = os.environ.get("EGS_CULL_LISTS", "1") != "0"            # A/B knob: footprint-culled tile lists
# long tile lists split over several waves (include/egs_hip.h egs_splat_draw_rec_seg): "auto" = whenever the longest list
# of the scene's last render exceeded the split threshold (and at first sight), "1" always, "0" never
SEGMENTS = os.environ.get("EGS_SEGMENTS", "auto")
# egs_splat_draw_rec_seg's `flags` (both surfaces)
DRAW_CULLED_LISTS = 1     # include/egs_hip.h EGS_DRAW_CULLED_LISTS
DRAW_MASKED_LISTS = 2     # include/egs_hip.h EGS_DRAW_MASKED_LISTS (egs_splat_bwd_seg takes it too)
SEG_HISTORY = 4           # include/egs_hip.h EGS_DRAW_SEG_HISTORY
SEG_SPECULATE_FLAG = 8    # include/egs_hip.h EGS_DRAW_SEG_SPECULATE
# a camera without a walk on record on the segment path: "auto" = all its segments at once when the scene's recent renders
# walked at least half of their longest list (nothing saturates: reset_alpha), "1" always, "0" never (segment 0 only)
SEG_SPECULATE = os.environ.get("EGS_SEG_SPECULATE", "auto")
ACCUMULATE = 64           # include/egs_hip.h EGS_BWD_ACCUMULATE
FACTORED_SH = 128         # include/egs_hip.h EGS_BWD_FACTORED_SH
ABSGRAD = 1024            # include/egs_hip.h EGS_BWD_ABSGRAD
POSE_ONLY = 2048          # include/egs_hip.h EGS_BWD_POSE_ONLY
# the render's flags (FusedState.flags): egs_fused_forward's `flags`, OR-ed into every egs_fused_backward phase
CULLED_LISTS = 32         # include/egs_hip.h EGS_FUSED_CULLED_LISTS
ANTIALIASED = 256         # include/egs_hip.h EGS_FUSED_ANTIALIASED
RAW = 512                 # include/egs_hip.h EGS_FUSED_RAW
GSID_MASK = 0x0FFFFFFF    # csrc/egs_common.h EGS_GSID_MASK


class FusedState:
    """Tensors the backward pass needs (all produced by ``forward``).  ``ticket`` is set while the render's
    patch count has not been validated yet (deferred validation, see ``deferred``)."""
    __slots__ = ("us", "depths", "cinv2ds", "colors", "areas", "rec", "contrib", "final_tau", "ranges", "gsid",
                 "order", "order_by_work", "gpack", "dcw", "flags", "width", "height", "ticket", "_patches", "_keep",
                 "seg", "extras")

    @property
    def culled(self):
        """the tile lists are footprint-culled (``CULLED_LISTS``)"""
        return bool(self.flags & CULLED_LISTS)

    @property
    def antialiased(self):
        """the render was anti-aliased (``ANTIALIASED``)"""
        return bool(self.flags & ANTIALIASED)

    def patch_count(self) -> int:
        """P of this render (waits for its read-back if it has not been looked at yet)."""
        if self.ticket is not None:
            _settle(self.ticket, True)
        return self._patches

    def gaussian_ids(self):
        """The tile lists as Gaussian indices, int32[P].  With footprint-culled lists (``culled``) the raw ``gsid``
        values carry the tile's 4-bit block mask above the low 28 bits; this strips it."""
        g = self.gsid[:self.patch_count()]
        return (g & GSID_MASK) if self.culled else g

    def block_masks(self):
        """The 4-bit mask of 8x8 pixel blocks per list entry (bit k = block (k & 1, k >> 1)); 15 for unculled lists."""
        g = self.gsid[:self.patch_count()]
        return ((g >> 28) & 15) if self.culled else torch.full_like(g, 15)


class Extras(collections.namedtuple("Extras", ("depth", "alpha", "background"))):
    """Render extras of ``forward`` (include/egs_hip.h EgsExtras): ``depth`` / ``alpha`` request the maps
    depth = sum w_i z_i (camera-space z, NOT normalised: depth / alpha.clamp_min(eps) is the expected depth) and
    alpha = sum w_i = 1 - T_final; ``background`` (r, g, b) floats or None adds T_final * bg to the image.  A render
    with extras takes the unsplit draw kernels (never the segment path)."""
    __slots__ = ()

    def background_rgb(self):
        return (0.0, 0.0, 0.0) if self.background is None else tuple(float(v) for v in self.background)


def _egs_extras(depths, bg, depth_out=None, alpha_out=None, dloss_ddepth=None, dloss_dalpha=None):
    ex = _lib.EgsExtras()
    ex.depths = depths.data_ptr() if depths is not None else None
    ex.depth_out = depth_out.data_ptr() if depth_out is not None else None
    ex.alpha_out = alpha_out.data_ptr() if alpha_out is not None else None
    ex.background[:] = bg
    ex.dloss_ddepth = dloss_ddepth.data_ptr() if dloss_ddepth is not None else None
    ex.dloss_dalpha = dloss_dalpha.data_ptr() if dloss_dalpha is not None else None
    return ex


def pose_tensors(Rcw, tcw, like):
    """(Rcw [3,3], tcw [3]) of a pose gradient, validated: float32 tensors on the device of ``like``; -> contiguous"""
    pair = ((Rcw, "Rcw", (3, 3)), (tcw, "tcw", (3,)))
    for t, name, shape in pair:
        if not isinstance(t, torch.Tensor):
            raise ValueError("pose %s must be a torch.Tensor, got %s" % (name, type(t).__name__))
        if tuple(t.shape) != shape:
            raise ValueError("pose %s must have shape %s, got %s" % (name, list(shape), list(t.shape)))
        if t.dtype != torch.float32:
            raise ValueError("pose %s must be torch.float32, got %s" % (name, t.dtype))
    for t, name, _ in pair:
        if not t.is_cuda or t.device != like.device:
            raise ValueError("pose %s must live on the device of the Gaussians (%s), got %s" % (name, like.device,
                                                                                                 t.device))
    return Rcw.contiguous(), tcw.contiguous()


_exchange_hook = None    # dist_views.ChunkedExchange while attached (process-wide: backward runs on autograd's thread)
_sh_sink = None          # dist_views.FactoredShGrad while attached: the SH gradient of a view stays dL/dcolour [N,3]


def _split_sh(low_shs, high_shs, n):
    low = _chk(low_shs, "low_shs", torch.float32, (n, 3))
    high = _chk(high_shs, "high_shs", torch.float32, (n, None))
    K = 3 + high.shape[1]
    if K not in (3, 12, 27, 48):
        raise ValueError("low_shs + high_shs must have 3, 12, 27 or 48 columns, got %d" % K)
    return low, high, K


def forward(pws, shs, alphas, scales, rots, cam, high_shs=None, need_grad=False, extras=None, antialiased=False):
    """-> (image[3,H,W], mask[N] bool, state); with ``extras`` (``Extras``) -> (image, mask, state, depth, alpha), the
    two maps float32 [1,H,W] or None where not requested.  ``cam`` carries Rcw/tcw/twc device
    tensors and fx, fy, cx, cy, width, height (reference gausplat_dataset.py:14-26).
    ``need_grad``: a backward pass will follow (the draw kernel then also zeroes its gradient records).
    With ``high_shs`` the inputs are the RAW training tensors (``shs`` = low_shs, ``alphas`` =
    alphas_raw, ``scales`` = scales_raw, ``rots`` = rots_raw) and the activations of
    gsplat/utils.py:121-150 run inside the kernel (``RAW``).
    ``antialiased``: the opacity compensation of the 2D filter (``ANTIALIASED``) -- every
    Gaussian is binned and drawn with opacity alpha sqrt(det(Sigma) / det(Sigma + 0.3 I)); the state records it and
    ``backward`` follows."""
    raw = high_shs is not None
    pws = _chk(pws, "pws", torch.float32, (None, 3))
    n = pws.shape[0]
    if raw:
        shs, high_shs, K = _split_sh(shs, high_shs, n)
    else:
        shs = _chk(shs, "shs", torch.float32, (n, None))
        K = shs.shape[1]
        if K not in (3, 12, 27, 48):
            raise ValueError("shs must have 3, 12, 27 or 48 columns, got %d" % K)
    alphas = _alphas(alphas, n)
    scales = _chk(scales, "scales", torch.float32, (n, 3))
    rots = _chk(rots, "rots", torch.float32, (n, 4))
    Rcw = _chk(cam.Rcw, "cam.Rcw", torch.float32, (3, 3))
    tcw = _chk(cam.tcw, "cam.tcw", torch.float32, (3,))
    twc = _chk(cam.twc, "cam.twc", torch.float32, (3,))
    W, H = int(cam.width), int(cam.height)
    lib = _lib_on(pws)
    dev = pws.device
    pol = C.byref(_pol())
    st = _stream()
    f32, i32 = torch.float32, torch.int32
    S = FusedState()
    S.width, S.height = W, H
    S.ticket, S._patches, S._keep, S.seg, S.extras = None, None, None, None, None
    # the draw kernels (forward and backward) work from the packed records alone: us / cinv2ds / colors /
    # areas are not materialised
    S.us = S.cinv2ds = S.colors = S.areas = None
    # Footprint-culled lists: a Gaussian is listed only for the tiles of its rect that {alpha' >= alpha_skip} can
    # reach, and every list value carries the tile's block mask (include/egs_hip.h EGS_DRAW_CULLED_LISTS).  The
    # lists are internal to this path -- the seven-op surface always returns the reference's.
    pol_ = _pol()
    culled = CULL_LISTS and pol_.footprint == 0 and pol_.alpha_skip > 0 and n < (1 << 28)
    S.flags = (CULLED_LISTS if culled else 0) | (ANTIALIASED if antialiased else 0) | (RAW if raw else 0)
    S.depths = torch.empty((n,), dtype=f32, device=dev)
    S.rec = torch.empty((max(n, 1), 12), dtype=f32, device=dev)   # packed 2D records, reused by backward
    mask = torch.empty((n,), dtype=torch.bool, device=dev)        # depths > 0.2, written by the kernel
    ws_bin_bytes = lib.egs_splat_bin_ws_bytes(n)
    ws_bin = torch.empty(ws_bin_bytes, dtype=torch.uint8, device=dev)
    # (host_slot: the mailbox slot the binning kernels also write {P, max key} into on the enqueue-ahead path)
    enqueue_bin = lambda hint, total, host_slot: _lib.check(lib.egs_fused_forward(
        n, K, _ptr(pws), _ptr(rots), _ptr(scales), _ptr(shs), _ptr(high_shs), _ptr(alphas), _ptr(Rcw), _ptr(tcw),
        _ptr(twc), float(cam.fx), float(cam.fy), float(cam.cx), float(cam.cy), W, H, pol, _ptr(S.us), _ptr(S.depths),
        _ptr(S.cinv2ds), _ptr(S.colors), _ptr(S.areas), _ptr(S.rec), _ptr(mask), _ptr(S.dcw), S.flags, hint,
        _ptr(ws_bin), ws_bin_bytes, _ptr(total), host_slot, st))
    image = torch.empty((3, H, W), dtype=f32, device=dev)       # fully written by the draw stage
    depth_map = alpha_map = None
    ex = None           # EgsExtras of the draw stage (render extras), None: a plain render
    if extras is not None:
        S.extras = extras
        if extras.depth:
            depth_map = torch.empty((1, H, W), dtype=f32, device=dev)
        if extras.alpha:
            alpha_map = torch.empty((1, H, W), dtype=f32, device=dev)
        ex = _egs_extras(S.depths, extras.background_rgb(), depth_map, alpha_map)
    done = (lambda: (image, mask, S)) if extras is None else (lambda: (image, mask, S, depth_map, alpha_map))
    S.contrib = torch.empty((H, W), dtype=i32, device=dev)
    S.final_tau = torch.empty((H, W), dtype=f32, device=dev)
    S.ranges = torch.empty((_tiles(W, H), 2), dtype=i32, device=dev)
    S.order = None            # [tile dispatch order | per-tile work]: ONE buffer per camera, see below
    # packed gradient records of the backward pass: zeroed on the side by the forward draw kernel (one use)
    S.gpack = torch.empty((max(n, 1), 12), dtype=f32, device=dev) if (need_grad and n > 0) else None
    # dcolor/dpw per Gaussian, written by the preprocess kernel for the backward pass: that pass then never reads the
    # SH coefficients (36 B written + read instead of a 4K-byte row re-read; EGS_SAVE_DCOLOR=0: A/B knob)
    S.dcw = torch.empty((n, 9), dtype=f32, device=dev) if (need_grad and n > 0 and SAVE_DCOLOR) else None

    def draw(rows, total, redo):
        # buffers for ``rows`` patches, the count from the device words ``total`` if given; ``redo``: see _ahead.render
        S.gsid = torch.empty(rows, dtype=i32, device=dev)   # (entries past P are unused: the kernels walk `ranges`)
        ws_draw = torch.empty(lib.egs_splat_draw_ws_bytes(n, rows, W, H), dtype=torch.uint8, device=dev)
        if use_seg:
            S.seg = torch.empty(lib.egs_seg_ws_bytes(max(rows, 1), W, H), dtype=torch.uint8, device=dev)
        # (seg_ws NULL: the unsplit kernels; the hint slot still learns how far this camera's tiles are walked)
        _lib.check(lib.egs_splat_draw_rec_seg(
            n, rows, _ptr(total), W, H, _ptr(S.rec), pol, _ptr(ws_bin), _ptr(ws_draw), ws_draw.numel(), _ptr(image),
            _ptr(S.contrib), _ptr(S.final_tau), _ptr(S.ranges), _ptr(S.gsid), _ptr(S.order), _ptr(S.gpack), prev_work,
            order_ready, draw_flags, _ptr(S.seg), S.seg.numel() if S.seg is not None else 0,
            None if (redo and walk_word is not None) else seg_hint, _ptr(walk_word), None, st,
            None if ex is None else C.byref(ex)))
        remember_order()

    ctx = _ctx(dev)
    key = (n, W, H)
    S.ticket = None
    # Dispatch order of the tiles.  A camera keeps ONE [order | work] buffer across its renders (per stream): the
    # draw kernel leaves the work it measured per tile in the second half, and the order in the first half is
    #   first render of the camera   sorted by list length (inside the library),
    #   second render                sorted by the work the first one measured,
    #   later renders                used as it stands -- the work pattern of a camera drifts slowly -- and
    #                                refreshed from the latest work every ORDER_REFRESH-th render:
    # no order kernel at all on most renders (10 us forward, 8 us backward at 1080p).
    prev_work, order_ready = None, 0
    cache_entry = None        # registered only AFTER the draw stage that writes the order buffer was enqueued
    use_seg, seg_hint, speculate = _seg_decision(ctx, lib, key, pol_, SEGMENTS, SEG_SPECULATE) if n > 0 \
        else (False, None, False)
    if extras is not None:    # the extras exist on the unsplit kernels only (the hint slot still learns from the render)
        use_seg = False
    walk_word = _walk_word(ctx, key, dev, st, seg_hint is not None)
    walk_known = False        # the camera was rendered before: its walk lengths are on record
    if TILE_WORK_CACHE and n > 0:
        ck = (id(cam), int(st.value or 0))              # one entry per camera and stream, whatever the scene size
        olen = lib.egs_tile_order_len(W, H)
        with ctx.lock:
            hit = ctx.tile_work.get(ck)
            if hit is not None and hit[0]() is cam and hit[1].numel() == olen and hit[3] == (n, W, H):
                S.order = hit[1]
                # `renders` counts the renders that wrote the ORDER part (the segment path plans its own work items and
                # leaves it alone; work and walk are written by both paths)
                renders = hit[2] + (0 if use_seg else 1)
                walk_known = True
                if not use_seg:
                    if renders <= 2 or renders % ORDER_REFRESH == 0:   # [order | work | walk]: its own work part
                        prev_work = C.c_void_p(S.order.data_ptr() + 4 * (olen - 2 * _tiles(W, H)))
                    else:
                        order_ready = 1
            else:
                S.order = torch.empty(olen, dtype=i32, device=dev)
                renders = 0 if use_seg else 1
        cache_entry = (ck, renders)
    if S.order is None:
        S.order = torch.empty(lib.egs_tile_order_len(W, H), dtype=i32, device=dev)

    def remember_order():
        """The render that just enqueued its draw stage wrote [order | work] (every path of the library does,
        patches == 0 included): only now may the NEXT render of this camera rely on it (a redone draw registers the
        same entry again).  A render that raised before this point leaves the cache as it was.  The entry goes when
        the camera object dies (weakref callback): callers that build a Camera per frame do not pile up order buffers."""
        if cache_entry is None:
            return
        ck, renders = cache_entry
        tw = ctx.tile_work

        def drop(_ref, ck=ck, tw=tw, lock=ctx.lock):
            with lock:
                ent = tw.get(ck)
                if ent is not None and ent[0] is _ref:
                    del tw[ck]
        try:
            ref = weakref.ref(cam, drop)
        except TypeError:                               # a camera object that cannot be weakly referenced
            return
        with ctx.lock:
            tw[ck] = (ref, S.order, renders, (n, W, H))
    S.order_by_work = prev_work is not None or order_ready == 1
    draw_flags = (DRAW_CULLED_LISTS if culled else 0) | (SEG_HISTORY if (use_seg and walk_known) else 0) | \
        (SEG_SPECULATE_FLAG if (use_seg and speculate) else 0)
    # (SPECULATE with a walk on record: the plan distrusts a record that is far shorter than the tile's list while the
    # scene's recent renders walk most of theirs -- the renders right after reset_alpha, gsmodel.py:320-324)
    cap = ctx.capacity.get(key, 0) if (ENQUEUE_AHEAD and n > 0) else 0
    # inside a ``deferred()`` block the render stays pending (S.ticket) and commit() reports S if it was incomplete
    patches = _ahead.render(ctx, dev, key, st, cap, _ahead.wait_slot, enqueue_bin, draw, S,
                            getattr(_tls, "deferred", False), MAILBOX_COPY)
    if patches is not None:
        S._patches = patches
    return done()


_pad_index = {}    # (device, N, slice widths) -> positions of the alignment words of a flat gradient buffer


class accumulate_in_kernel:
    """``with fused.accumulate_in_kernel(): ...`` -- backward passes of ``GSFunction`` / ``GSRawFunction`` inside the
    block ADD their parameter gradients to the ``.grad`` the leaves already hold, inside the chain-rule kernel, and
    return ``None`` for them to autograd (which then leaves ``.grad`` alone) -- instead of handing autograd fresh
    tensors that it accumulates with separate kernels (976 B per Gaussian and view against 488).  For a rank that
    renders several views per step.  Only taken when every differentiated input is a leaf whose ``.grad`` came out
    of this module's backward (slices of one buffer, ``flat_grad_buffer``); the first view of a step, non-leaf inputs
    or foreign ``.grad`` tensors go the ordinary way.  Tensor hooks / post-accumulate hooks of the leaves do not
    fire for the views accumulated this way."""

    def __enter__(self):
        self._prev = getattr(_acc_flag, "on", False)
        _acc_flag.on = True
        return self

    def __exit__(self, et, ev, tb):
        _acc_flag.on = self._prev
        return False


class _AccFlag:          # process-wide, not thread-local: autograd runs backward on its own thread
    on = False


_acc_flag = _AccFlag()


def _engine_accumulates_into(node_ctx, count):
    """True when the running autograd pass will ACCUMULATE into ``.grad`` of the first ``count`` inputs of the node
    ``node_ctx`` (a ``.backward()`` that reaches all of them); False under ``torch.autograd.grad`` (gradients are
    captured and returned, ``.grad`` must stay untouched) or ``backward(inputs=[...])`` that leaves some out."""
    try:
        nodes = [fn for fn, _ in node_ctx.next_functions[:count]]
        return all(fn is not None and torch._C._will_engine_execute_node(fn) for fn in nodes)
    except Exception:      # "a leaf node was passed ... while running autograd.grad": captures, not accumulation
        return False


DEFAULT = object()       # "no per-call choice": the process-wide attach() state applies


def sh_sink_for(node_ctx, count, sh_tensors, explicit=None):
    """The attached ``dist_views.FactoredShGrad`` when the running backward pass may leave its SH gradient there: the
    SH inputs are leaves (``finish`` writes their ``.grad``; behind a torch ``cat`` the rows are needed here) and the
    engine accumulates into the node's ``count`` leaves (a ``.backward()`` of a training step -- never under
    ``torch.autograd.grad``, whose caller expects the rows returned)."""
    # explicit = (sink, exchange) of the call's RenderOptions; None: whatever is attached process-wide
    sink, hook = (_sh_sink, _exchange_hook) if explicit is None else explicit
    if sink is None or not all(t.is_leaf and t.requires_grad for t in sh_tensors) or \
            not _engine_accumulates_into(node_ctx, count):
        return None
    if hook is not None:
        raise RuntimeError("FactoredShGrad and ChunkedExchange cannot be attached together (the overlapped exchange "
                           "all-reduces the SH rows the factored form never writes)")
    return sink


def accumulation_targets(leaves, node_ctx=None, count=None, explicit=None):
    """The ``.grad`` tensors of ``leaves`` when the coming backward may add to them in place (see
    ``accumulate_in_kernel``), else None.  ``node_ctx``: the autograd node whose backward is running -- the in-kernel
    accumulation is only taken when the engine itself would accumulate into every leaf (never under
    ``torch.autograd.grad``, whose callers expect returned tensors and an untouched ``.grad``).  ``count``: how many
    inputs of the node are differentiated leaves (default ``len(leaves)``; larger when ``leaves`` leaves the SH
    tensors out because their gradient goes to a ``FactoredShGrad``)."""
    # explicit = (accumulate, exchange) of the call's RenderOptions; None: the process-wide block / attach() state
    on, hook = (getattr(_acc_flag, "on", False), _exchange_hook) if explicit is None else explicit
    if not on or hook is not None:
        return None
    if node_ctx is not None and not _engine_accumulates_into(node_ctx, len(leaves) if count is None else count):
        return None
    grads = []
    for t in leaves:
        g = t.grad if (t.is_leaf and t.requires_grad) else None
        if g is None or g.dtype != torch.float32 or not g.is_contiguous() or g.shape != t.shape or \
                (g.data_ptr() & 15) or g.device != t.device:
            return None
        grads.append(g)
    if flat_grad_buffer(leaves) is None:      # not the one-buffer layout this module's backward hands out
        return None
    return grads


def backward(pws, shs, alphas, scales, rots, cam, S: FusedState, dloss_dgammas, high_shs=None, accumulate=None,
             sh_sink=None, exchange=DEFAULT, dloss_ddepth=None, dloss_dalpha=None, pose=None, absgrad=False,
             pose_only=False):
    """-> (dloss_dpws[N,3], dloss_dshs[N,K], dloss_dalphas[N,1], dloss_dscales[N,3],
           dloss_drots[N,4], dloss_dus[N,2])  -- the gradient tuple of gsmodel.py:87-93.
    With ``high_shs`` (raw tensors, see ``forward``): -> (dpws, dlow_shs[N,3], dhigh_shs[N,K-3],
    dalphas_raw[N,1], dscales_raw, drots_raw, dus).
    ``accumulate``: the five (raw: six) gradient tensors of earlier views, in the order of the return tuple; this
    view's gradients are ADDED to them by the kernel and the same tensors are returned.
    ``sh_sink`` (``dist_views.FactoredShGrad``): the SH gradient of this view is left there as dL/dcolour [N,3]
    (``EGS_BWD_FACTORED_SH``); the SH entries of the return tuple are None, ``accumulate`` holds the other four
    tensors only, and the flat buffer is the 11 floats per Gaussian of pws, alphas, scales, rots.
    A render with extras (``forward(..., extras=...)``): ``dloss_ddepth`` / ``dloss_dalpha`` [1,H,W] or None (0); the
    background of the render is part of the gradient whatever they are.
    ``pose`` = (Rcw [3,3], tcw [3]), float32 on the device: the camera of the forward call (``cam.twc`` must be
    -Rcw^T tcw), whose gradient is also formed -> the usual tuple followed by (dloss_dRcw [3,3], dloss_dtcw [3]).  The
    pose gradient belongs to this view: always written, never added to ``accumulate``.  Excludes ``exchange``.
    An anti-aliased render (``forward(..., antialiased=True)``, recorded in ``S.flags``) takes the AA chain rule.
    ``absgrad``: the draw pass also sums the ABSOLUTE per-pixel terms of dloss_dus (``EGS_BWD_ABSGRAD``, DESIGN §3.10:
    AbsGS / gsplat's ``absgrad``) and ``dloss_dus_abs`` [N,2] -- this view's, never accumulated, a statistic and not a
    gradient -- is appended to the result.  Not for a render with extras.
    ``pose_only`` (``EGS_BWD_POSE_ONLY``; needs ``pose``): the map is frozen and only the camera moves --
    the chain rule forms nothing but the pose gradient, no per-Gaussian gradient is allocated or written, and the
    result is just (dloss_dRcw, dloss_dtcw).  Excludes ``accumulate``, ``sh_sink``, ``absgrad`` and an exchange."""
    raw = high_shs is not None
    pws = _chk(pws, "pws", torch.float32, (None, 3))
    n = pws.shape[0]
    if raw:
        shs, high_shs, K = _split_sh(shs, high_shs, n)
    else:
        shs = _chk(shs, "shs", torch.float32, (n, None))
        K = shs.shape[1]
    alphas = _alphas(alphas, n)
    scales = _chk(scales, "scales", torch.float32, (n, 3))
    rots = _chk(rots, "rots", torch.float32, (n, 4))
    if raw != bool(S.flags & RAW):
        raise ValueError("fused.backward: the inputs must have the layout of the forward call (raw tensors with "
                         "high_shs, or activated ones without)")
    W, H = S.width, S.height
    dl = _chk(dloss_dgammas, "dloss_dgammas", torch.float32, (3, H, W))
    rx = getattr(S, "extras", None)
    ex = None
    if rx is not None:
        dd = _chk(dloss_ddepth, "dloss_ddepth", torch.float32, (1, H, W)) if dloss_ddepth is not None else None
        da = _chk(dloss_dalpha, "dloss_dalpha", torch.float32, (1, H, W)) if dloss_dalpha is not None else None
        ex = _egs_extras(S.depths, rx.background_rgb(), dloss_ddepth=dd, dloss_dalpha=da)
    elif dloss_ddepth is not None or dloss_dalpha is not None:
        raise ValueError("fused.backward: depth / alpha gradients for a render without extras")
    if absgrad and rx is not None:
        raise ValueError("fused.backward: absgrad is not available for a render with extras (depth / alpha / background)")
    lib = _lib_on(pws)
    dev = pws.device
    f32 = torch.float32
    pg = None
    hook = _exchange_hook if exchange is DEFAULT else exchange      # (``exchange``: the call's own ChunkedExchange or None)
    if pose_only:
        if pose is None:
            raise ValueError("fused.backward: pose_only needs pose=(Rcw, tcw)")
        for v, name in ((accumulate, "accumulate"), (sh_sink, "sh_sink"), (absgrad or None, "absgrad"),
                        (hook, "a ChunkedExchange")):
            if v is not None:
                raise ValueError("fused.backward: pose_only writes no per-Gaussian gradient and does not combine with "
                                 + name)
    if pose is not None:
        if hook is not None:
            raise ValueError("fused.backward: a pose gradient cannot go with a ChunkedExchange (the chunked chain rule "
                             "has no single launch to reduce the camera gradient in)")
        Rcw, tcw = pose_tensors(pose[0], pose[1], pws)
        dRcw = torch.empty((3, 3), dtype=f32, device=dev)
        dtcw = torch.empty((3,), dtype=f32, device=dev)
        pose_ws = torch.empty(lib.egs_pose_ws_bytes(n), dtype=torch.uint8, device=dev)
        pg = _lib.EgsPoseGrad(dRcw.data_ptr(), dtcw.data_ptr(), pose_ws.data_ptr(), pose_ws.numel())
    else:
        Rcw, tcw = cam.Rcw, cam.tcw
    # The parameter gradients are slices of ONE allocation (order: pws, shs | low, high, alphas, scales,
    # rots): a data-parallel caller exchanges all 59 floats per Gaussian with a single all-reduce of
    # ``flat_grad_buffer(params)`` instead of five or six latency-bound ones (autograd adopts the slices as
    # ``.grad`` without copying).
    widths = [3, 3, K - 3, 1, 3, 4] if raw else [3, K, 1, 3, 4]
    if sh_sink is not None:
        widths = [3, 1, 3, 4]
    if pose_only:                     # nothing per Gaussian: the seven output pointers go down as NULL
        parts = [None] * len(widths)
    elif accumulate is not None:
        parts = [g.view(n, w) for g, w in zip(accumulate, widths)]
    else:
        starts, at = [], 0
        for w in widths:                      # every slice starts 16-B aligned (the kernels store dwordx4)
            starts.append(at)
            at += (n * w + 3) // 4 * 4
        flat = torch.empty(at, dtype=f32, device=dev)
        # the <= 3 alignment words behind a slice belong to nobody: zero, not whatever the allocator left there --
        # whole-buffer operations (ViewStreams.finish adds flat buffers, callers all-reduce / norm / isfinite them)
        # must never meet NaN garbage.  No padding (and no kernel) when N is a multiple of four.
        pad = [i for a, w in zip(starts, widths) for i in range(a + n * w, a + (n * w + 3) // 4 * 4)]
        if pad:
            pk = (dev, n, tuple(widths))
            idx = _pad_index.get(pk)
            if idx is None:
                # (one index tensor per device and layout: a densifying trainer changes N every few epochs, and the
                # entries of the sizes it left behind would pile up)
                for old in [q for q in _pad_index if q[0] == dev and q[2] == pk[2]]:
                    del _pad_index[old]
                idx = _pad_index[pk] = torch.tensor(pad, dtype=torch.int64, device=dev)
            flat.index_fill_(0, idx, 0.0)
        parts = [flat[a:a + n * w].view(n, w) for a, w in zip(starts, widths)]
    if sh_sink is not None:
        dpws, dalphas, dscales, drots = parts
        dshs, dhigh = sh_sink.slot(n, K, cam), None     # [N,3]: dL/dcolour of this view (written, never added to)
    elif raw:
        dpws, dshs, dhigh, dalphas, dscales, drots = parts
    else:
        dpws, dshs, dalphas, dscales, drots = parts
        dhigh = None
    dus = None if pose_only else torch.empty((n, 2), dtype=f32, device=dev)
    ws_bytes = lib.egs_fused_backward_ws_bytes(n)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    st = _stream()
    gpack, S.gpack = S.gpack, None      # zeroed by the forward draw kernel: good for ONE backward pass
    dus_abs = None
    if absgrad:
        dus_abs = torch.empty((n, 2), dtype=f32, device=dev)
        if gpack is None and n > 0:     # (the records are read back below: they must be the caller's)
            gpack = torch.zeros((n, 12), dtype=f32, device=dev)
    seg = getattr(S, "seg", None)       # the forward pass split its long lists: the backward pass walks its segments
    seg_bytes = seg.numel() if seg is not None else 0
    # every phase and chunk carries the render's flags (culled lists, anti-aliased, raw inputs) from the forward's state
    launch = lambda phase, b, c: _lib.check(lib.egs_fused_backward(
        n, K, S.gsid.shape[0], W, H, _ptr(pws), _ptr(rots), _ptr(scales), _ptr(shs), _ptr(high_shs), _ptr(alphas),
        _ptr(Rcw), _ptr(tcw), _ptr(cam.twc), float(cam.fx), float(cam.fy), float(cam.cx), float(cam.cy),
        C.byref(_pol()), _ptr(S.us), _ptr(S.cinv2ds), _ptr(S.colors), _ptr(S.areas), _ptr(S.rec), _ptr(S.depths),
        _ptr(S.contrib), _ptr(S.final_tau), _ptr(S.ranges), _ptr(S.gsid), _ptr(dl), _ptr(ws), ws_bytes, _ptr(dpws),
        _ptr(dshs), _ptr(dhigh), _ptr(dalphas), _ptr(dscales), _ptr(drots), _ptr(dus), _ptr(S.order), _ptr(gpack),
        _ptr(getattr(S, "dcw", None)), phase | S.flags, b, c, _ptr(seg), seg_bytes, st,
        None if ex is None else C.byref(ex), None if pg is None else C.byref(pg)))
    # the forward pass was dispatched by remembered work: the backward pass keeps its order (no second order kernel)
    keep = KEEP_FORWARD_ORDER if (REUSE_ORDER and getattr(S, "order_by_work", False)) else 0
    if accumulate is not None:
        keep |= ACCUMULATE            # the outputs hold earlier views' gradients: add to them
    if sh_sink is not None:
        keep |= FACTORED_SH
    if absgrad:
        keep |= ABSGRAD               # (a bit of the draw pass: phases 0 and 1)
    if pose_only:
        launch(POSE_ONLY | keep, 0, n)
        return dRcw, dtcw
    if hook is not None and sh_sink is not None:
        raise RuntimeError("fused.backward: sh_sink and an attached ChunkedExchange exclude each other")
    chunks = hook.chunks if hook is not None else 1
    rows = -(-n // (256 * chunks)) * 256 if chunks > 1 else n     # rows per chunk: whole workgroups
    if hook is not None:
        hook.begin_backward()              # one backward pass per attach()/finish(): raises on a second one
    if hook is None or chunks <= 1 or rows >= n:
        launch(0 | keep, 0, n)
        if hook is not None:
            # FRESH view objects: a second reference to the tensors returned below would make AccumulateGrad
            # clone them, and the reduced values would never reach .grad
            hook.on_chunk([p[:] for p in parts])
    else:
        # The chain rule runs in a few row chunks; each chunk's gradient slices go to the exchange as soon as
        # its kernel is enqueued, so the all-reduce of chunk k overlaps the computation of chunk k + 1
        launch(1 | keep, 0, 0)
        for b in range(0, n, rows):
            c = min(rows, n - b)
            launch(2 | (keep & (ACCUMULATE | FACTORED_SH)), b, c)
            hook.on_chunk([p[b:b + c] for p in parts])
    tail = () if pg is None else (dRcw, dtcw)
    if absgrad:
        _lib.check(lib.egs_grad_records_absgrad(n, _ptr(gpack), _ptr(dus_abs), st))
        tail = tail + (dus_abs,)
    if sh_sink is not None:
        return ((dpws, None, None, dalphas, dscales, drots, dus) if raw else (dpws, None, dalphas, dscales, drots, dus)) \
            + tail
    if raw:
        return (dpws, dshs, dhigh, dalphas, dscales, drots, dus) + tail
    return (dpws, dshs, dalphas, dscales, drots, dus) + tail
