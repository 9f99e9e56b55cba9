"""Autograd boundary: the counterpart of the reference's ``GSFunction``
(gsplat/gsmodel.py:6-93) on top of the MI355X op surface.

Identical inputs ``(pws, shs, alphas[N,1], scales, rots, us, cam)``, outputs
``(image[3,H,W], depths > 0.2)`` and gradient tuple order (gsmodel.py:87-93).
``GSFunction.mode`` selects how the same function is evaluated:

* ``"fused"`` (default) -- easygaussiansplatting_amd.fused: one preprocess kernel +
  splat forward; splatB's draw pass + one Jacobian-free chain-rule kernel backward
  (three C-ABI calls per step, no Jacobians in HBM);
* ``"ops"``  -- the reference's structure: six op calls with ``calc_J=True``, 17
  tensors saved, ``splatB`` + the chain-rule kernel over the stored Jacobians
  (``gsplatcu.chain_rule``; tests compare it with the batched-matmul spelling of gsmodel.py:71-85).
"""
from __future__ import annotations

import dataclasses
import math

import torch

from . import fused as _fused
from . import gsplatcu as gsc


class Camera:
    """Device-side camera, field names of reference gausplat_dataset.py:14-26."""

    def __init__(self, width, height, fx, fy, cx, cy, Rcw, tcw, device="cuda", id=0, path=""):
        self.id = id
        self.width = int(width)
        self.height = int(height)
        self.fx, self.fy, self.cx, self.cy = float(fx), float(fy), float(cx), float(cy)
        self.Rcw = torch.as_tensor(Rcw, dtype=torch.float32).to(device).contiguous()
        self.tcw = torch.as_tensor(tcw, dtype=torch.float32).to(device).contiguous()
        self.twc = (-torch.linalg.inv(self.Rcw.double().cpu()) @ self.tcw.double().cpu()).float().to(device)
        self.path = path

    @staticmethod
    def from_scene(cam, device="cuda"):
        return Camera(cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy, cam.Rcw, cam.tcw, device)


@dataclasses.dataclass(frozen=True)
class RenderOptions:
    """How ONE ``GSFunction.apply`` / ``GSRawFunction.apply`` call is evaluated -- carried by the autograd node, so two
    trainers (or a trainer and a viewer) in one process never share a switch.  Passed as the optional last argument of
    ``apply``; without it the call follows the process-wide defaults (``GSFunction.mode`` / ``ops_use_records`` and the
    ``fused.accumulate_in_kernel()`` / ``FactoredShGrad.attach()`` / ``ChunkedExchange.attach()`` blocks), which stay
    for callers that cannot change the seven-argument call of gsmodel.py:185-212."""
    mode: str = "fused"             # "fused": the fused kernels; "ops": the reference's seven-op structure
    ops_use_records: bool = True    # mode "ops": hand the forward's packed records to the backward's splatB
    accumulate: bool = False        # backward ADDS this view's gradients to the leaves' .grad inside the chain-rule kernel
    sh_sink: object = None          # dist_views.FactoredShGrad: the SH gradient of this view stays dL/dcolour [N,3]
    exchange: object = None         # dist_views.ChunkedExchange: all-reduce the gradient chunks from inside backward
    # render extras (fused path only): ``apply`` then returns image, mask, then depth [1,H,W] if requested, then alpha
    # [1,H,W] if requested.  depth = sum w_i z_i (camera-space z, not normalised: depth / alpha.clamp_min(eps) is the
    # expected depth), alpha = sum w_i = 1 - T_final; both differentiable.
    depth: bool = False             # also return the accumulated depth map
    alpha: bool = False             # also return the accumulated opacity map
    background: tuple = None        # (r, g, b) floats: the image gets T_final * bg added (not differentiable)
    # anti-aliased rendering (fused path only): the Mip-Splatting 2D filter -- the +0.3 px^2 dilation stays
    # and every Gaussian is drawn with opacity alpha sqrt(det(Sigma) / det(Sigma + 0.3 I)); differentiable
    antialiased: bool = False
    # absolute screen-space gradients (fused path only; AbsGS, gsplat's ``absgrad``): after ``backward`` the
    # ``us`` tensor handed to ``apply`` carries ``us.absgrad`` [N,2] = sum over pixels of |dL/du| of THIS view -- overwritten
    # by each backward, never accumulated, a densification statistic and not a gradient.  Not with depth / alpha /
    # background
    absgrad: bool = False
    # pose nodes only (fused path): the map is frozen -- backward forms nothing but dL/dRcw and dL/dtcw
    # (``EGS_BWD_POSE_ONLY``) and returns None for every Gaussian input and ``us``, whatever their requires_grad.  Chosen
    # here, never inferred.  Not with accumulate, sh_sink, exchange or absgrad
    pose_only: bool = False

    def __post_init__(self):
        if self.mode not in ("fused", "ops"):
            raise ValueError("RenderOptions.mode must be 'fused' or 'ops', got %r" % (self.mode,))
        if self.sh_sink is not None and self.exchange is not None:
            raise ValueError("RenderOptions: sh_sink and exchange exclude each other")
        if self.background is not None:
            try:
                bg = tuple(float(v) for v in self.background)
            except (TypeError, ValueError):
                bg = None
            if bg is None or len(bg) != 3 or not all(math.isfinite(v) for v in bg) or \
                    isinstance(self.background, (str, bytes)):
                raise ValueError("RenderOptions.background must be three finite floats, got %r" % (self.background,))
            object.__setattr__(self, "background", bg)
        if not isinstance(self.antialiased, (bool, int)) or self.antialiased not in (0, 1):
            raise ValueError("RenderOptions.antialiased must be a bool, got %r" % (self.antialiased,))
        object.__setattr__(self, "antialiased", bool(self.antialiased))
        if self.mode == "ops" and self.antialiased:
            raise ValueError("RenderOptions: antialiased needs mode='fused' (the seven-op structure mirrors the reference, "
                             "which has no opacity compensation)")
        if not isinstance(self.absgrad, (bool, int)) or self.absgrad not in (0, 1):
            raise ValueError("RenderOptions.absgrad must be a bool, got %r" % (self.absgrad,))
        object.__setattr__(self, "absgrad", bool(self.absgrad))
        if self.mode == "ops" and self.absgrad:
            raise ValueError("RenderOptions: absgrad needs mode='fused' (the seven-op structure mirrors the reference, "
                             "whose splatB returns the signed gradient only)")
        if self.absgrad and self.has_extras():
            raise ValueError("RenderOptions: absgrad does not combine with depth / alpha / background (the draw kernel "
                             "has no instance for both)")
        if not isinstance(self.pose_only, bool):
            raise ValueError("RenderOptions.pose_only must be a bool, got %r" % (self.pose_only,))
        if self.pose_only:
            if self.mode != "fused":
                raise ValueError("RenderOptions: pose_only needs mode='fused' (the pose nodes are the fused path)")
            for on, name in ((self.accumulate, "accumulate"), (self.sh_sink is not None, "sh_sink"),
                             (self.exchange is not None, "exchange"), (self.absgrad, "absgrad")):
                if on:
                    raise ValueError("RenderOptions: pose_only writes no per-Gaussian gradient and does not combine "
                                     "with " + name)
        if self.mode == "ops" and self.has_extras():
            raise ValueError("RenderOptions: depth / alpha / background need mode='fused' (the seven-op structure mirrors "
                             "the reference, which renders the image only)")

    def has_extras(self):
        return bool(self.depth) or bool(self.alpha) or self.background is not None

    def extras(self):
        """-> fused.Extras of this call, or None without extras."""
        return _fused.Extras(bool(self.depth), bool(self.alpha), self.background) if self.has_extras() else None


def _extra_outputs(ctx, image, mask, depth, alpha):
    """(image, mask[, depth][, alpha]) of a fused render with extras (ctx.extras)"""
    out = [image, mask]
    if ctx.extras.depth:
        out.append(depth)
    if ctx.extras.alpha:
        out.append(alpha)
    return tuple(out)


def _extra_grads(ctx, dloss_dgammas, rest):
    """-> (dL/dimage, dL/ddepth, dL/dalpha) from the grad outputs behind the mask's; dL/dimage is zeros when only the
    maps took part in the loss, None when nothing did"""
    rest = list(rest)
    dd = rest.pop(0) if ctx.extras.depth else None
    da = rest.pop(0) if ctx.extras.alpha else None
    if dloss_dgammas is None and (dd is not None or da is not None):
        ref = dd if dd is not None else da
        dloss_dgammas = torch.zeros((3, ctx.cam.height, ctx.cam.width), dtype=torch.float32, device=ref.device)
    return dloss_dgammas, dd, da


def _fused_forward(ctx, leaves, cam, us=None):
    """The fused-path forward of a node (``ctx.opts`` set): renders ``leaves`` -- the node's Gaussian inputs in its
    argument order, (pws, shs, alphas, scales, rots) or the raw (pws, low_shs, high_shs, alphas_raw, scales_raw,
    rots_raw) -- through ``cam``, saves them for ``_fused_backward`` and returns the node's outputs.  ``us``: the
    node's ``us`` input, on which ``RenderOptions.absgrad`` delivers its statistic"""
    o = ctx.opts
    if o is not None and o.pose_only and not isinstance(cam, _PoseCamera):
        raise ValueError("RenderOptions.pose_only is for GSPoseFunction / GSRawPoseFunction (this node has no pose "
                         "gradient to return)")
    ctx.extras = None if o is None else o.extras()
    ctx.us_ref = None
    if o is not None and o.absgrad:
        if not isinstance(us, torch.Tensor):
            raise ValueError("RenderOptions.absgrad needs a tensor as `us` (us.absgrad is where the statistic is left), "
                             "got %s" % type(us).__name__)
        ctx.us_ref = us
    pws, shs, *rest = leaves
    high_shs = rest.pop(0) if len(leaves) == 6 else None
    res = _fused.forward(pws, shs, *rest, cam, high_shs=high_shs, need_grad=True, extras=ctx.extras,
                         antialiased=o is not None and o.antialiased)
    image, mask, ctx.state = res[:3]
    ctx.cam = cam
    ctx.save_for_backward(*leaves)
    ctx.mark_non_differentiable(mask)
    if ctx.extras is not None:
        return _extra_outputs(ctx, image, mask, res[3], res[4])
    return image, mask


def _fused_backward(ctx, dloss_dgammas, rest, pose=False):
    """The fused-path backward of a node whose forward ran ``_fused_forward``: its gradient tuple (``ctx.n_inputs``
    entries).  ``pose``: a pose node -- the camera of the call is also differentiated (inputs Rcw, tcw behind ``us``)
    and the call never takes a ChunkedExchange."""
    dd = da = None
    if ctx.extras is not None:
        dloss_dgammas, dd, da = _extra_grads(ctx, dloss_dgammas, rest)
    if dloss_dgammas is None:  # the image did not take part in the loss
        return (None,) * ctx.n_inputs
    o = ctx.opts
    leaves = ctx.saved_tensors
    k = len(leaves)
    pws, sh, others = leaves[0], leaves[1:k - 3], leaves[k - 3:]    # sh: (shs,) or (low_shs, high_shs)
    if o is not None and o.pose_only:       # (a pose node: _fused_forward refuses the option elsewhere)
        cam = ctx.cam
        dRcw, dtcw = _fused.backward(
            pws, sh[0], *others, cam, ctx.state, dloss_dgammas.contiguous(), high_shs=sh[1] if len(sh) == 2 else None,
            exchange=None, dloss_ddepth=None if dd is None else dd.contiguous(),
            dloss_dalpha=None if da is None else da.contiguous(), pose=(cam.Rcw, cam.tcw), pose_only=True)
        return (None,) * (k + 1) + (dRcw if ctx.needs_input_grad[k + 1] else None,
                                    dtcw if ctx.needs_input_grad[k + 2] else None) + (None,) * (ctx.n_inputs - k - 3)
    exchange = None if (pose or o is None) else o.exchange
    # a training step that keeps its SH gradient factored (dist_views.FactoredShGrad): this view leaves dL/dcolour
    # [N,3] in the sink, autograd gets None for the SH inputs, the others go on as usual
    sink = _fused.sh_sink_for(ctx, k, sh, None if o is None else (o.sh_sink, exchange))
    acc = _fused.accumulation_targets((pws,) + others if sink is not None else leaves, ctx, k,
                                      None if o is None else (o.accumulate, exchange))
    cam = ctx.cam
    res = _fused.backward(
        pws, sh[0], *others, cam, ctx.state, dloss_dgammas.contiguous(), high_shs=sh[1] if len(sh) == 2 else None,
        accumulate=acc, sh_sink=sink, exchange=None if pose else (_fused.DEFAULT if o is None else o.exchange),
        dloss_ddepth=None if dd is None else dd.contiguous(), dloss_dalpha=None if da is None else da.contiguous(),
        pose=(cam.Rcw, cam.tcw) if pose else None, absgrad=ctx.us_ref is not None)
    if ctx.us_ref is not None:      # this view's statistic, overwritten by each backward (gsplat's means2d.absgrad)
        ctx.us_ref.absgrad = res[-1]
    # acc: added to the leaves' .grad inside the kernel, nothing for autograd to accumulate
    grads = res[:k + 1] if acc is None else (None,) * k + (res[k],)
    tail = [None] * (ctx.n_inputs - k - 1)      # us's gradient is the last of `grads`; then Rcw, tcw, cam, opts
    if pose:
        tail[:2] = (res[k + 1] if ctx.needs_input_grad[k + 1] else None,
                    res[k + 2] if ctx.needs_input_grad[k + 2] else None)
    return tuple(grads) + tuple(tail)


class GSFunction(torch.autograd.Function):
    # process-wide defaults of calls WITHOUT a RenderOptions argument
    mode = "fused"
    # mode "ops": hand the forward's packed records / masked list to the backward's splatB (gsplatcu.SplatRecords).
    # False = the plain public pair, what an UNMODIFIED reference GSFunction (gsmodel.py:6-93) gets by default.
    ops_use_records = True

    @staticmethod
    def forward(ctx, pws, shs, alphas, scales, rots, us, cam, opts=None):
        ctx.opts = opts            # None: the process-wide defaults, looked up where they are needed
        # always the maximal tuple (autograd drops surplus trailing Nones): apply(..., cam, None) passes `opts` explicitly
        ctx.n_inputs = 8
        ctx.mode = GSFunction.mode if opts is None else opts.mode
        use_records = GSFunction.ops_use_records if opts is None else opts.ops_use_records
        # the mask output never carries a gradient: do not let autograd zero-fill one per step
        ctx.set_materialize_grads(False)
        if ctx.mode == "fused":
            return _fused_forward(ctx, (pws, shs, alphas, scales, rots), cam, us)
        # forward.md steps 1-5 == gsmodel.py:21-39
        us, pcs, depths, du_dpcs = gsc.project(pws, cam.Rcw, cam.tcw, cam.fx, cam.fy, cam.cx, cam.cy, True)
        cov3ds, dcov3d_drots, dcov3d_dscales = gsc.computeCov3D(rots, scales, depths, True)
        cov2ds, dcov2d_dcov3ds, dcov2d_dpcs = gsc.computeCov2D(
            cov3ds, pcs, cam.Rcw, depths, cam.fx, cam.fy, cam.width, cam.height, True)
        colors, dcolor_dshs, dcolor_dpws = gsc.sh2Color(shs, pws, cam.twc, True)
        cinv2ds, areas, dcinv2d_dcov2ds = gsc.inverseCov2D(cov2ds, depths, True)
        # us / cinv2ds / colors are this node's own intermediates and never leave it: the packed records of the forward
        # draw stay valid for the backward draw (gsplatcu.SplatRecords; `alphas` is checked by version in splatB)
        if use_records:
            (image, contrib, final_tau, patch_range_per_tile, gsid_per_patch), ctx.records = gsc.splat_with_records(
                cam.height, cam.width, us, cinv2ds, alphas, depths, colors, areas)
        else:
            image, contrib, final_tau, patch_range_per_tile, gsid_per_patch = gsc.splat(
                cam.height, cam.width, us, cinv2ds, alphas, depths, colors, areas)
            ctx.records = None
        ctx.cam = cam
        ctx.save_for_backward(us, cinv2ds, alphas, depths, colors, contrib, final_tau, patch_range_per_tile,
                              gsid_per_patch, dcinv2d_dcov2ds, dcov2d_dcov3ds, dcov3d_drots, dcov3d_dscales,
                              dcolor_dshs, du_dpcs, dcov2d_dpcs, dcolor_dpws)
        # depths > 0.2 after the in-place culling of inverseCov2D / splat (gsmodel.py:50): the packing kernel of splat
        # left it in the handle; otherwise one compare kernel
        mask = ctx.records.visible if (ctx.records is not None and ctx.records.visible is not None) else depths > 0.2
        ctx.mark_non_differentiable(mask)
        return image, mask

    @staticmethod
    def backward(ctx, dloss_dgammas, _, *rest):
        if ctx.mode == "fused":
            return _fused_backward(ctx, dloss_dgammas, rest)
        if dloss_dgammas is None:  # the image did not take part in the loss
            return (None,) * ctx.n_inputs
        cam = ctx.cam
        pad = (None,) * (ctx.n_inputs - 6)      # cam (and the options)
        (us, cinv2ds, alphas, depths, colors, contrib, final_tau, patch_range_per_tile, gsid_per_patch,
         dcinv2d_dcov2ds, dcov2d_dcov3ds, dcov3d_drots, dcov3d_dscales, dcolor_dshs, du_dpcs, dcov2d_dpcs,
         dcolor_dpws) = ctx.saved_tensors
        dloss_dus, dloss_dcinv2ds, dloss_dalphas, dloss_dcolors = gsc.splatB(
            cam.height, cam.width, us, cinv2ds, alphas, depths, colors, contrib, final_tau,
            patch_range_per_tile, gsid_per_patch, dloss_dgammas.contiguous(), records=ctx.records)
        n = us.shape[0]
        dloss_dpws, dloss_dshs, dloss_dscales, dloss_drots = gsc.chain_rule(
            dloss_dus, dloss_dcinv2ds, dloss_dcolors, cam.Rcw, dcinv2d_dcov2ds, dcov2d_dcov3ds,
            dcov3d_drots, dcov3d_dscales, dcolor_dshs, du_dpcs, dcov2d_dpcs, dcolor_dpws)
        return (dloss_dpws, dloss_dshs, dloss_dalphas.reshape(n, 1), dloss_dscales, dloss_drots,
                dloss_dus.reshape(n, 2)) + pad


class GSRawFunction(torch.autograd.Function):
    """``GSModel.forward`` (gsmodel.py:185-212) as ONE autograd node on the optimizer's tensors:
    inputs ``(pws, low_shs, high_shs, alphas_raw, scales_raw, rots_raw, us, cam)`` -- the argument order
    of ``GSModel.forward`` -- outputs ``(image, depths > 0.2)``.  The activations (sigmoid, exp,
    normalize, cat; gsplat/utils.py:121-150) and their derivatives run inside the fused kernels."""

    @staticmethod
    def forward(ctx, pws, low_shs, high_shs, alphas_raw, scales_raw, rots_raw, us, cam, opts=None):
        ctx.opts = opts            # (``mode`` does not apply: this node IS the fused path)
        ctx.n_inputs = 9     # (as GSFunction: the maximal tuple)
        ctx.set_materialize_grads(False)
        return _fused_forward(ctx, (pws, low_shs, high_shs, alphas_raw, scales_raw, rots_raw), cam, us)

    @staticmethod
    def backward(ctx, dloss_dgammas, _, *rest):
        return _fused_backward(ctx, dloss_dgammas, rest)


def camera_centre(Rcw, tcw):
    """twc = -Rcw^T tcw on the device (no host sync): the camera centre the pose nodes render with.  ``Camera.twc`` is
    -inv(Rcw) tcw instead; on a true rotation the two agree."""
    return -(Rcw.t() @ tcw)


class _PoseCamera:
    """The camera of one pose-node call: size and intrinsics of ``cam``, extrinsics from the node's tensors"""

    def __init__(self, cam, Rcw, tcw):
        self.width, self.height = cam.width, cam.height
        self.fx, self.fy, self.cx, self.cy = cam.fx, cam.fy, cam.cx, cam.cy
        self.Rcw, self.tcw = Rcw, tcw
        self.twc = camera_centre(Rcw, tcw).contiguous()


def _pose_setup(ctx, opts, Rcw, tcw, cam, like):
    """checks shared by the pose nodes; -> the call's _PoseCamera"""
    if opts is not None and opts.mode == "ops":
        raise ValueError("the pose nodes need mode='fused' (the seven-op structure mirrors the reference, which has no "
                         "pose Jacobian)")
    if (opts.exchange if opts is not None else _fused._exchange_hook) is not None:
        raise ValueError("the pose nodes do not combine with a ChunkedExchange (the camera gradient needs the chain "
                         "rule in one launch)")
    Rcw, tcw = _fused.pose_tensors(Rcw, tcw, like)
    ctx.opts = opts
    ctx.set_materialize_grads(False)
    return _PoseCamera(cam, Rcw.detach(), tcw.detach())


class GSPoseFunction(torch.autograd.Function):
    """``GSFunction`` on the fused path with the camera pose as two more differentiable inputs:
    ``apply(pws, shs, alphas, scales, rots, us, Rcw, tcw, cam, opts=None)``.  ``cam`` supplies only the image size and
    the intrinsics; the extrinsics are ``Rcw`` [3,3] and ``tcw`` [3] (float32, on the device of the Gaussians), and the
    camera centre is twc = -Rcw^T tcw (``camera_centre``; ``Camera`` uses -inv(Rcw) tcw -- equal on a true rotation,
    and the gradient is that of the -Rcw^T tcw form).  Outputs are those of ``GSFunction`` (render extras included);
    the backward pass also returns dL/dRcw and dL/dtcw, formed by the chain-rule kernel in the same launch.
    ``RenderOptions(mode="ops")`` or an ``exchange`` raise ValueError."""

    @staticmethod
    def forward(ctx, pws, shs, alphas, scales, rots, us, Rcw, tcw, cam, opts=None):
        pcam = _pose_setup(ctx, opts, Rcw, tcw, cam, pws)
        ctx.n_inputs = 10
        return _fused_forward(ctx, (pws, shs, alphas, scales, rots), pcam, us)

    @staticmethod
    def backward(ctx, dloss_dgammas, _, *rest):
        return _fused_backward(ctx, dloss_dgammas, rest, pose=True)


class GSRawPoseFunction(torch.autograd.Function):
    """``GSRawFunction`` with the camera pose as two more differentiable inputs:
    ``apply(pws, low_shs, high_shs, alphas_raw, scales_raw, rots_raw, us, Rcw, tcw, cam, opts=None)``; ``cam``, the
    camera centre and the options as ``GSPoseFunction``."""

    @staticmethod
    def forward(ctx, pws, low_shs, high_shs, alphas_raw, scales_raw, rots_raw, us, Rcw, tcw, cam, opts=None):
        pcam = _pose_setup(ctx, opts, Rcw, tcw, cam, pws)
        ctx.n_inputs = 11
        return _fused_forward(ctx, (pws, low_shs, high_shs, alphas_raw, scales_raw, rots_raw), pcam, us)

    @staticmethod
    def backward(ctx, dloss_dgammas, _, *rest):
        return _fused_backward(ctx, dloss_dgammas, rest, pose=True)


def render(pws, shs, alphas, scales, rots, cam, calc_J=False):
    """Inference path of the reference's forward_gpu.py:47-60 (six op calls)."""
    us, pcs, depths = gsc.project(pws, cam.Rcw, cam.tcw, cam.fx, cam.fy, cam.cx, cam.cy, False)
    cov3ds = gsc.computeCov3D(rots, scales, depths, False)[0]
    cov2ds = gsc.computeCov2D(cov3ds, pcs, cam.Rcw, depths, cam.fx, cam.fy, cam.width, cam.height, False)[0]
    colors = gsc.sh2Color(shs, pws, cam.twc, False)[0]
    cinv2ds, areas = gsc.inverseCov2D(cov2ds, depths, False)
    return gsc.splat(cam.height, cam.width, us, cinv2ds, alphas, depths, colors, areas)
