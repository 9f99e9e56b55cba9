"""Data-parallel training step: the counterpart of the reference's ``train.py:30-83``
on the MI355X path (SURVEY.md §8a', §8e).

What it keeps from the reference
* the raw parameterisation and activations (gsplat/utils.py:121-150: sigmoid alphas,
  exp scales, normalised quaternions, SH = cat(low, high); gsmodel.py:96-129);
* Adam with the reference's per-group learning rates (gsmodel.py:114-127) and
  eps = 1e-15 (train.py:32), the exponential position-lr schedule (utils.py:7-44);
* the loss 0.8 L1 + 0.2 (1 - SSIM) (pytorch_ssim.py:63-66) -- through the fused HIP loss;
* checkpoints as a structured ``.npy`` of ACTIVATED parameters with the reference's
  record dtype (gau_io.py:7-12, 141-156).

What is new (the reference renders one view per optimizer step on one GPU)
* a step renders ``views_per_step`` views: each rank takes its share
  (dist_views.views_for_rank), accumulates the mean gradient over its local views,
  then ONE RCCL all-reduce (mean) of the 59 gradient floats per Gaussian and one
  all-reduce (sum) of the densification statistics;
* the optimizer is ``optim.FusedAdam`` (one HIP launch for all six groups) unless
  ``fused_adam=False``; densification / alpha reset (gsmodel.py:232-330) run on the device
  through ``density.DensityControl`` and are replica-consistent: every rank holds the same
  all-reduced statistics and the split offsets are a pure function of (seed, round, row).
"""
from __future__ import annotations

import contextlib
import dataclasses
import math
from typing import Dict, List, Sequence

import numpy as np
import torch
import torch.distributed as dist

from . import dist_views as DV
from . import fused as _fused
from . import features as _features
from . import importance as _importance
from .density import DensityControl, MCMCControl, expon_lr
from . import pose as _pose
from . import appearance as _appearance
from .function import (Camera, GSFunction, GSPoseFunction, GSRawFunction, GSRawPoseFunction,
                       RenderOptions)
from .loss import gau_loss, gau_loss_with_grad
from .optim import FusedAdam, adam_groups
from .scene import gsdata_type

SH_C0 = 0.28209479177387814


def raw_params_from_scene(scene, device="cuda", clamp_alpha: bool = True) -> Dict[str, torch.Tensor]:
    """gsmodel.py:96-113: un-activated leaf tensors; SH split into degree 0 (low) and the rest (high).
    ``clamp_alpha`` keeps the logit finite for opacities of exactly 0 or 1 (the reference does not clamp)."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(device)
    shs = t(scene.shs)
    n = shs.shape[0]
    high = torch.full((n, 45), 0.001, device=device)
    if shs.shape[1] > 3:
        high[:, : shs.shape[1] - 3] = shs[:, 3:]
    alphas = t(scene.alphas).reshape(-1, 1)
    if clamp_alpha:
        alphas = alphas.clamp(1e-4, 1 - 1e-4)
    p = {"pws": t(scene.pws), "low_shs": shs[:, :3].contiguous(), "high_shs": high,
         "alphas_raw": torch.log(alphas / (1 - alphas)), "scales_raw": torch.log(t(scene.scales)),
         "rots_raw": t(scene.rots)}
    for v in p.values():
        v.requires_grad_(True)
    return p


def activate(p):
    """utils.py:129-150 / gsmodel.py:198-207."""
    return (p["pws"], torch.cat((p["low_shs"], p["high_shs"]), dim=1), torch.sigmoid(p["alphas_raw"]),
            torch.exp(p["scales_raw"]), torch.nn.functional.normalize(p["rots_raw"]))


def make_optimizer(p, fused=True):
    """train.py:32 over the groups of gsmodel.py:114-127."""
    cls = FusedAdam if fused else torch.optim.Adam
    return cls(adam_groups(p), lr=0.0, eps=1e-15)


def _checked_pixel_weights(pixel_weights, gt_images, device):
    """``Trainer(pixel_weights=...)``, checked once (host synchronisations are fine here) -> None, or a list with one
    float32 [H,W] tensor on ``device`` or None per view.  ValueError names the view."""
    if pixel_weights is None:
        return None
    weights, gts = list(pixel_weights), list(gt_images)
    if len(weights) != len(gts):
        raise ValueError("Trainer(pixel_weights=...): %d entries for %d views (one per camera; None for a view that "
                         "counts every pixel)" % (len(weights), len(gts)))
    out = []
    for v, (w, gt) in enumerate(zip(weights, gts)):
        if w is None:
            out.append(None)
            continue
        what = "Trainer(pixel_weights=...): view %d" % v
        if not isinstance(w, torch.Tensor) or w.dtype not in (torch.float32, torch.bool, torch.uint8):
            raise ValueError("%s must be a float32, bool or uint8 tensor, got %s"
                             % (what, w.dtype if isinstance(w, torch.Tensor) else type(w).__name__))
        if tuple(w.shape) != tuple(gt.shape[-2:]):
            raise ValueError("%s has shape %s, its ground-truth image is %s"
                             % (what, list(w.shape), list(gt.shape[-2:])))
        w = (w if w.dtype == torch.float32 else (w != 0)).to(device=device, dtype=torch.float32).contiguous()
        if not bool(torch.isfinite(w).all()):
            raise ValueError("%s holds a non-finite weight" % what)
        if bool((w < 0).any()):
            raise ValueError("%s holds a negative weight" % what)
        if not bool((w > 0).any()):
            raise ValueError("%s is all zero: the view would have no loss (drop the view instead)" % what)
        out.append(w)
    return out


def _checked_depth_priors(depth_priors, gt_images, device):
    """``Trainer(depth_priors=...)``, checked once (host synchronisations are fine here) -> None, or a list with one
    float32 [H,W] disparity plane on ``device`` or None per view.  ValueError names the view."""
    if depth_priors is None:
        return None
    priors, gts = list(depth_priors), list(gt_images)
    if len(priors) != len(gts):
        raise ValueError("Trainer(depth_priors=...): %d entries for %d views (one per camera; None for a view without "
                         "a prior)" % (len(priors), len(gts)))
    out = []
    for v, (q, gt) in enumerate(zip(priors, gts)):
        if q is None:
            out.append(None)
            continue
        what = "Trainer(depth_priors=...): view %d" % v
        if not isinstance(q, torch.Tensor) or q.dtype != torch.float32:
            raise ValueError("%s must be a float32 tensor (disparity; 0 = no data), got %s"
                             % (what, q.dtype if isinstance(q, torch.Tensor) else type(q).__name__))
        if tuple(q.shape) != tuple(gt.shape[-2:]):
            raise ValueError("%s has shape %s, its ground-truth image is %s"
                             % (what, list(q.shape), list(gt.shape[-2:])))
        q = q.to(device=device).contiguous()
        if not bool(((q > 0) & torch.isfinite(q)).any()):
            raise ValueError("%s has no positive finite pixel: the view would have no depth term (pass None instead)"
                             % what)
        out.append(q)
    return out


def _checked_normal_priors(normal_priors, gt_images, device):
    """``Trainer(normal_priors=...)``, checked once (host synchronisations are fine here) -> None, or a list with one
    float32 [3,H,W] camera-frame normal map on ``device`` or None per view.  ValueError names the view."""
    if normal_priors is None:
        return None
    priors, gts = list(normal_priors), list(gt_images)
    if len(priors) != len(gts):
        raise ValueError("Trainer(normal_priors=...): %d entries for %d views (one per camera; None for a view without "
                         "a prior)" % (len(priors), len(gts)))
    out = []
    for v, (q, gt) in enumerate(zip(priors, gts)):
        if q is None:
            out.append(None)
            continue
        what = "Trainer(normal_priors=...): view %d" % v
        if not isinstance(q, torch.Tensor) or q.dtype != torch.float32:
            raise ValueError("%s must be a float32 tensor (camera-frame normals; all zero = no data), got %s"
                             % (what, q.dtype if isinstance(q, torch.Tensor) else type(q).__name__))
        if tuple(q.shape) != (3,) + tuple(gt.shape[-2:]):
            raise ValueError("%s has shape %s, its ground-truth image is %s"
                             % (what, list(q.shape), list(gt.shape[-2:])))
        q = q.to(device=device).contiguous()
        if not bool((torch.isfinite(q).all(0) & ((q * q).sum(0) > 0)).any()):
            raise ValueError("%s has no pixel with data: the view would have no prior term (pass None instead)" % what)
        out.append(q)
    return out


def _checked_depth_weight(depth_weight):
    """-> (init, final) of the depth term's weight; a single float is constant"""
    try:
        pair = (float(depth_weight),) * 2 if isinstance(depth_weight, (int, float)) else \
            tuple(float(x) for x in depth_weight)
    except (TypeError, ValueError):
        pair = ()
    if len(pair) != 2 or not all(math.isfinite(x) and x >= 0 for x in pair) or \
            (pair[0] != pair[1] and min(pair) <= 0):
        raise ValueError("Trainer(depth_weight=%r): expected a float >= 0 or (init, final), both > 0" % (depth_weight,))
    return pair


class Trainer:
    def __init__(self, scene, cameras: Sequence, gt_images: Sequence[torch.Tensor], max_steps: int,
                 scene_size: float = 1.0, device="cuda", fused_adam: bool = True, seed: int = 0,
                 fused_activations: bool = True, view_streams: int = 4, factored_sh: bool = True, mode: str = "fused",
                 antialiased: bool = False, absgrad: bool = False, grad_threshold: float = None,
                 pose_opt: bool = False, pose_lr=(_pose.LR_ROT, _pose.LR_TRANS), strategy: str = "default",
                 cap_max: int = None, mcmc_options: dict = None, sparse_adam: bool = False,
                 bilagrid: bool = False, bilagrid_shape=_appearance.DEFAULT_SHAPE, bilagrid_lr: float = 2e-3,
                 bilagrid_tv: float = 10.0, pixel_weights: Sequence = None, depth_priors: Sequence = None,
                 depth_kind: str = "affine", depth_weight=(1.0, 0.01), depth_alpha_min: float = 0.05,
                 normal_priors: Sequence = None, normal_weight: float = 0.05, normal_smooth: float = 0.0,
                 normal_alpha_min: float = 0.05, normal_edge_gamma: float = 10.0):
        """``strategy``: how Gaussians are added and removed.  "default" is the reference's clone / split / prune /
        alpha reset (``density.DensityControl``).  "mcmc" (needs ``cap_max``, the hard limit on the number
        of Gaussians) is ``density.MCMCControl``: every step adds the opacity / scale regularisers' gradient before the
        optimizer step and a covariance-shaped position noise after it, ``densify`` relocates dead Gaussians and grows
        the model by 5 % up to ``cap_max``, and ``fit`` never resets alpha.  ``mcmc_options``: further keyword arguments
        of ``MCMCControl`` (min_opacity, noise_lr, opacity_reg, scale_reg, growth).  With "default" nothing in a step
        differs.

        ``pose_opt``: also refine the camera poses (fused path only).  Every camera gets a twist on its
        stored pose (``pose.PoseTable``), every view renders through a pose node, and after the optimizer step the
        twists of the cameras rendered in the step take a per-row Adam step.  ``pose_lr`` = (rotation step in radians,
        translation step as a fraction of the camera distance); the defaults are those of examples/pose_refine.py --
        found for frozen-map refinement on a synthetic scene and NOT tuned for joint training, which nobody has
        measured.  With ``pose_opt`` the views of one ``step`` must be distinct cameras (a twist takes one Adam step
        per optimizer step; ``ValueError`` otherwise -- ``fit`` draws from a permutation and never repeats one).
        Without ``pose_opt`` nothing in a step differs: no pose node, no extra tensor.

        ``sparse_adam``: the visibility-masked optimizer step (needs ``fused_adam`` and the "default"
        strategy).  A Gaussian that no view of the step saw -- on any rank: the visibility count is taken after the
        all-reduce -- keeps its parameters and both Adam moments bit for bit and is neither read nor written; dense
        Adam, the reference's, keeps moving it on its old momentum.  With ``sparse_adam=False`` nothing in a step
        differs.

        ``bilagrid``: per-image appearance compensation (every ``mode``).  Every training image gets a
        bilateral grid of 3 x 4 affine colour transforms (``appearance.GridTable``, ``bilagrid_shape`` = (Gw, Gh, L),
        identity at the start); the loss of a view is taken on the render sliced through that view's grid
        (``appearance.slice_forward`` / ``slice_backward``, HIP, no autograd node), and after the optimizer step the
        grids of the views rendered in the step take a per-row Adam step on the gradient of image loss +
        ``bilagrid_tv`` x total variation.  ``step`` returns the image loss on the corrected image; the TV term of the
        step's grids is kept as ``last_tv``.  ``bilagrid_lr`` and ``bilagrid_tv`` are gsplat's defaults: NOT tuned here,
        and nobody has measured them on this code.  The views of one ``step`` must be distinct (a grid takes one Adam
        step per optimizer step; ``ValueError`` otherwise).  The grids belong to the training images: a novel view has
        none (``corrected`` exists for inspection).  With ``bilagrid=False`` nothing in a step differs: no table, no
        extra tensor, no extra launch.

        ``pixel_weights``: per-pixel loss weights (masks; every ``mode``).  A sequence with one entry per
        camera: a tensor [H,W] of the view's ground-truth size (float32 >= 0, or bool / uint8 read as 0 / 1), or None for
        a view that counts every pixel (it takes the unweighted kernels).  Checked once, here (shape, finite, >= 0, not
        all zero: ``ValueError`` naming the view).  A weighted view's loss is sum w |x - y| / (3 sum w) and
        sum w S / (3 sum w): EVERY VIEW IS NORMALISED BY ITS OWN sum w, so a view that is 90 % masked counts as much in
        the step's mean as an unmasked one.  A pixel with w = 0 still receives SSIM gradient from weighted pixels up to
        5 px away; for a hard exclusion dilate the mask by 5 px.  With ``bilagrid`` the weighted loss is taken on the
        corrected image.  ``step`` returns the mean of the (weighted) losses.  With ``pixel_weights=None`` nothing in a
        step differs: no extra tensor, no extra launch, libegs_wloss.so is not loaded.

        ``depth_priors``: depth supervision (fused path only).  A sequence with one entry per camera: a
        float32 tensor [H,W] of the view's ground-truth size holding the prior DISPARITY (inverse depth; 0, negative or
        non-finite: no data), or None for a view without a prior (it renders exactly as without the option).  Checked
        once, here (shape, dtype, at least one positive finite pixel: ``ValueError`` naming the view).  A view with a
        prior also renders its depth and opacity maps, ``depthloss.depth_loss_with_grad`` (``depth_kind``: "metric",
        "affine" -- scale and shift fitted per view and step, on the device -- or "pearson") turns them into
        dL/ddepth and dL/dalpha, and ONE backward pass takes these and dL/dimage.  The term enters the step with the
        weight init (final / init)^(iteration / max_steps) for ``depth_weight`` = (init, final) -- (1.0, 0.01) are the
        official code's values, NOT tuned here -- or a constant for a single float; ``pixel_weights[v]`` weights its
        pixels too.  ``depth_alpha_min`` = 0.05 (pixels with less opacity do not count) guards the 1 / depth^2 factor
        of the gradient; nobody has tuned it.  ``step`` still returns the image loss; the mean unweighted depth term of
        the step's views that have a prior is kept as ``last_depth_loss`` (a device tensor).  Not with ``absgrad`` (the
        draw kernel has no instance for absolute gradients and render extras) nor with ``mode`` other than "fused".
        A render with the maps takes the unsplit draw kernels.  With ``depth_priors=None`` nothing in a step differs: no
        extra tensor, no extra launch, libegs_depthloss.so is not loaded.

        ``normal_priors``, ``normal_smooth``: surface-normal terms on the rendered depth map (fused path
        only).  ``normal_priors``: a sequence with one entry per camera: a float32 tensor [3,H,W] of the view's
        ground-truth size holding CAMERA-frame normals (x right, y down, z forward; a pixel that is all zero or
        non-finite has no data), or None for a view without one.  Checked once, here (shape, dtype, at least one pixel
        with data: ``ValueError`` naming the view).  ``normal_smooth`` > 0 adds the edge-aware smoothness of the normal
        for EVERY view, guided by the view's ground-truth image; it needs no prior.  A view with either term also renders
        its depth and opacity maps, ``normalloss.normal_loss_with_grad`` turns them into dL/ddepth and dL/dalpha -- added
        to those of the depth term when both are on -- and ONE backward pass takes these and dL/dimage.  The terms enter
        the step as ``normal_weight`` x prior term + ``normal_smooth`` x smoothness term; ``pixel_weights[v]`` weights
        their pixels too.  ``normal_weight`` = 0.05, ``normal_alpha_min`` = 0.05 and ``normal_edge_gamma`` = 10 are
        defaults nobody has tuned.  ``step`` still returns the image loss; ``last_normal_loss`` is a device tensor [2]:
        the mean unweighted prior term over the step's views that have a prior, and the mean smoothness term over the
        step's views.  Not with ``absgrad`` nor with ``mode`` other than "fused", as for ``depth_priors``.  Without the two
        arguments nothing in a step differs: no extra tensor, no extra launch, libegs_normalloss.so is not loaded."""
        self.device = device
        self.pixel_weights = _checked_pixel_weights(pixel_weights, gt_images, device)
        self.depth_priors = _checked_depth_priors(depth_priors, gt_images, device)
        self.last_depth_loss = None
        self._depth_sum = None
        if self.depth_priors is not None:
            from . import depthloss as _depthloss
            if depth_kind not in _depthloss.KINDS:
                raise ValueError("Trainer(depth_kind=%r): expected one of %s" % (depth_kind, list(_depthloss.KINDS)))
            if absgrad:
                raise ValueError("Trainer(depth_priors=...) with absgrad=True: a view with a prior renders its depth and "
                                 "opacity maps, and the draw kernel has no instance for absolute gradients and render "
                                 "extras")
            if mode != "fused":
                raise ValueError("Trainer(depth_priors=...) needs mode='fused' (the depth and opacity maps are the "
                                 "fused path's), got %r" % (mode,))
            self.depth_kind = depth_kind
            self.depth_weight = _checked_depth_weight(depth_weight)
            self.depth_alpha_min = float(depth_alpha_min)
            if not 0.0 <= self.depth_alpha_min < float("inf"):
                raise ValueError("Trainer(depth_alpha_min=%r): expected a finite value >= 0" % (depth_alpha_min,))
            self._depth_loss_with_grad = _depthloss.depth_loss_with_grad
        self.normal_priors = _checked_normal_priors(normal_priors, gt_images, device)
        self.normal_smooth = float(normal_smooth)
        if not 0.0 <= self.normal_smooth < float("inf"):
            raise ValueError("Trainer(normal_smooth=%r): expected a finite value >= 0" % (normal_smooth,))
        self.normals_on = self.normal_priors is not None or self.normal_smooth > 0
        self.last_normal_loss = None
        self._normal_sum = None
        if self.normals_on:
            what = "normal_priors=..." if self.normal_priors is not None else "normal_smooth=%r" % (normal_smooth,)
            if absgrad:
                raise ValueError("Trainer(%s) with absgrad=True: a view with a normal term renders its depth and "
                                 "opacity maps, and the draw kernel has no instance for absolute gradients and render "
                                 "extras" % what)
            if mode != "fused":
                raise ValueError("Trainer(%s) needs mode='fused' (the depth and opacity maps are the "
                                 "fused path's), got %r" % (what, mode))
            self.normal_weight = float(normal_weight)
            if not 0.0 <= self.normal_weight < float("inf"):
                raise ValueError("Trainer(normal_weight=%r): expected a finite value >= 0" % (normal_weight,))
            self.normal_alpha_min = float(normal_alpha_min)
            if not 0.0 <= self.normal_alpha_min < float("inf"):
                raise ValueError("Trainer(normal_alpha_min=%r): expected a finite value >= 0" % (normal_alpha_min,))
            self.normal_edge_gamma = float(normal_edge_gamma)
            if not 0.0 <= self.normal_edge_gamma < float("inf"):
                raise ValueError("Trainer(normal_edge_gamma=%r): expected a finite value >= 0" % (normal_edge_gamma,))
            from . import normalloss as _normalloss
            self._normal_loss_with_grad = _normalloss.normal_loss_with_grad
        if strategy not in ("default", "mcmc"):
            raise ValueError("Trainer(strategy=%r): expected 'default' or 'mcmc'" % (strategy,))
        if strategy == "mcmc" and cap_max is None:
            raise ValueError("Trainer(strategy='mcmc') needs cap_max, the hard limit on the number of Gaussians")
        if sparse_adam and not fused_adam:
            raise ValueError("Trainer(sparse_adam=True) needs fused_adam=True (the masked step is FusedAdam's)")
        if sparse_adam and strategy == "mcmc":
            raise ValueError("Trainer(sparse_adam=True) with strategy='mcmc': MCMC's regularisers and noise act on every "
                             "Gaussian every step; combining the two is not supported")
        self.sparse_adam = bool(sparse_adam)
        self.bilagrid = bool(bilagrid)
        if self.bilagrid:
            try:
                self.bilagrid_shape = _appearance._shape3(bilagrid_shape)
            except (TypeError, ValueError) as e:
                raise ValueError("Trainer(bilagrid_shape=%r): %s" % (bilagrid_shape, e)) from e
        # how THIS trainer's renders are evaluated (function.RenderOptions.mode; "ops" needs fused_activations=False):
        # carried by every call, never by a process-wide switch -- two trainers in one process may differ
        self.mode = mode
        if mode != "fused" and fused_activations:
            raise ValueError("Trainer(mode=%r) needs fused_activations=False (GSRawFunction is the fused path)" % (mode,))
        if pose_opt and mode != "fused":
            raise ValueError("Trainer(pose_opt=True) needs mode='fused' (the pose nodes are the fused path), got %r"
                             % (mode,))
        # anti-aliased training (RenderOptions.antialiased; fused path only): every render of a step
        self.antialiased = bool(antialiased)
        # densify on the ABSOLUTE screen-space gradient (RenderOptions.absgrad; fused path only): the
        # statistic gathered per step is ||sum over pixels |dL/du| || instead of ||dL/du||, in which the pulls of
        # different pixels on a large Gaussian cannot cancel.  It is larger than the signed one (DESIGN §3.10 has the
        # measured ratio): set ``grad_threshold`` with it -- None keeps DensityControl's (the reference's 4e-7)
        self.absgrad = bool(absgrad)
        RenderOptions(mode=mode, antialiased=self.antialiased, absgrad=self.absgrad)   # (raises ValueError for mode="ops")
        # a rank's views of a step go round-robin to this many HIP streams (dist_views.ViewStreams); 1 = one after
        # the other on the caller's stream
        self.view_streams = max(1, int(view_streams))
        self._vs = None
        self.factored_sh = bool(factored_sh)     # see step(): the SH gradient of a step kept as dL/dcolour per view
        self._fx = None
        self._us = {}
        # True: GSRawFunction (activations inside the HIP kernels); False: torch activations + GSFunction,
        # the reference's structure (gsmodel.py:198-210)
        self.fused_activations = fused_activations
        self.params = raw_params_from_scene(scene, device)
        self.opt = make_optimizer(self.params, fused_adam)
        self.density = DensityControl(scene_size, max_steps, seed)
        self.strategy = strategy
        self.mcmc = MCMCControl(cap_max, seed=seed, **(mcmc_options or {})) if strategy == "mcmc" else None
        if grad_threshold is not None:
            self.density.grad_threshold = float(grad_threshold)
        self.cams = [c if isinstance(c, Camera) else Camera.from_scene(c, device) for c in cameras]
        self.gts = list(gt_images)
        self.max_steps = max_steps
        self.scene_size = scene_size
        self.iteration = 0
        self.world = dist.get_world_size() if dist.is_initialized() else 1
        self.rank = dist.get_rank() if dist.is_initialized() else 0
        n = self.params["pws"].shape[0]
        self.grad_accum = torch.zeros(n, device=device)             # gsmodel.py:214-230 statistics
        self.vis_count = torch.zeros(n, dtype=torch.int32, device=device)
        self.redone_steps = 0        # steps rendered twice because a view outgrew the enqueue-ahead buffers
        self.pose_opt = bool(pose_opt)
        self.pose_table = self.pose_grad = None
        if self.pose_opt:
            self.pose_table = _pose.PoseTable(self.cams, device, lr_rot=pose_lr[0], lr_trans=pose_lr[1])
            # dL/dtwist of the step, dense [V,6]: the rows of the views this rank rendered, zero elsewhere
            self.pose_grad = torch.zeros((len(self.cams), 6), device=device)
        # appearance compensation: the table, the step's gradient rows [len(view_ids), 12, L, Gh, Gw] (row k belongs to
        # view_ids[k]; this rank's rows, zero elsewhere -- never a dense [V, ...] tensor) and the TV term of the last step
        self.grid_table = self.grid_grad = self.last_tv = None
        self._grid_rows = {}
        self.bilagrid_tv = float(bilagrid_tv)
        if self.bilagrid:
            self.grid_table = _appearance.GridTable(len(self.cams), self.bilagrid_shape, lr=bilagrid_lr, device=device)

    _KEYS = ("pws", "low_shs", "high_shs", "alphas_raw", "scales_raw", "rots_raw")

    def depth_weight_at(self, iteration: int) -> float:
        """The weight of the depth term at optimizer step ``iteration``: init (final / init)^(iteration / max_steps),
        held at ``final`` from ``max_steps`` on.  Host arithmetic."""
        init, final = self.depth_weight
        if init == final:
            return init
        return init * (final / init) ** (min(max(int(iteration), 0), self.max_steps) / max(self.max_steps, 1))

    def _us_leaf(self, lane, n):
        """The zero ``us`` leaf of gsmodel.py:198-199, one per lane, kept across steps (only its ``.grad`` matters:
        dL/du of the view just rendered); a fresh ``torch.zeros`` per view is a fill kernel per view."""
        u = self._us.get(lane)
        if u is None or u.shape[0] != n:
            u = self._us[lane] = torch.zeros((n, 2), device=self.device, requires_grad=True)
        u.grad = None
        return u

    def _render_views(self, mine, n_views, opts=None):
        """forward + loss + backward of this rank's views; leaves accumulate the mean over ALL views of the step.
        Two or more views: dealt to ``view_streams`` HIP streams (one gradient accumulator and one set of
        statistics per stream, added up at the end)."""
        n = self.params["pws"].shape[0]
        lanes = min(self.view_streams, len(mine)) if str(self.device).startswith("cuda") else 1
        vs = None
        if lanes > 1:
            if self._vs is None or self._vs.n != lanes or \
                    any(a is not self.params[k] for a, k in zip(self._vs.params, self._KEYS)):
                self._vs = DV.ViewStreams([self.params[k] for k in self._KEYS], lanes)
            vs = self._vs
            vs.begin()
        loss_sum = [torch.zeros((), device=self.device) for _ in range(lanes)]
        depth_sum = depth_opts = normal_sum = None
        with_depth = self.depth_priors is not None and any(self.depth_priors[v] is not None for v in mine)
        with_normals = self.normals_on and (self.normal_smooth > 0 or
                                            any(self.normal_priors[v] is not None for v in mine))
        if with_depth or with_normals:
            depth_opts = dataclasses.replace(opts if opts is not None else RenderOptions(mode=self.mode), depth=True,
                                             alpha=True)
        if with_depth:
            depth_sum = [torch.zeros((), device=self.device) for _ in range(lanes)]
            depth_scale = self.depth_weight_at(self.iteration) / n_views
        if with_normals:     # (L_p, L_s) summed over the views of a lane
            normal_sum = [torch.zeros(2, device=self.device) for _ in range(lanes)]
        gnorm = [torch.zeros(n, device=self.device) for _ in range(lanes)]
        count = [torch.zeros(n, dtype=torch.int32, device=self.device) for _ in range(lanes)]
        if vs is not None:      # the accumulators above were zeroed on the caller's stream: the lanes start after that
            for s in vs.streams:
                s.wait_stream(torch.cuda.current_stream())
        for i, v in enumerate(mine):
            k = i % lanes
            with (vs.lane(i) if vs is not None else contextlib.nullcontext(None)) as lv:
                p = dict(zip(self._KEYS, lv)) if lv is not None else self.params
                us = self._us_leaf(k, n)                                             # gsmodel.py:198-199
                tw = None
                # a view with a depth prior also renders its depth and opacity maps (outputs 3 and 4 of the node)
                qv = None if self.depth_priors is None else self.depth_priors[v]
                # ... and so does a view with a normal term (a prior of its own, or the smoothness term of every view)
                nv = None if self.normal_priors is None else self.normal_priors[v]
                with_n = self.normals_on and (nv is not None or self.normal_smooth > 0)
                vopts = opts if qv is None and not with_n else depth_opts
                if self.pose_opt:     # the view's camera: its stored pose under its twist (a leaf of this render)
                    tw = self.pose_table.leaf(v)
                    Rcw, tcw = self.pose_table.pose(v, tw)
                    if self.fused_activations:
                        out = GSRawPoseFunction.apply(p["pws"], p["low_shs"], p["high_shs"], p["alphas_raw"],
                                                      p["scales_raw"], p["rots_raw"], us, Rcw, tcw, self.cams[v], vopts)
                    else:
                        out = GSPoseFunction.apply(*activate(p), us, Rcw, tcw, self.cams[v], vopts)
                elif self.fused_activations:
                    out = GSRawFunction.apply(p["pws"], p["low_shs"], p["high_shs"], p["alphas_raw"],
                                              p["scales_raw"], p["rots_raw"], us, self.cams[v], vopts)
                else:
                    out = GSFunction.apply(*activate(p), us, self.cams[v], vopts)
                image, mask = out[0], out[1]
                # loss / n_views (train.py:52-57 with the mean over the step's views): the loss kernels produce the
                # scaled dL/dimage themselves, backward starts at the image
                wv = None if self.pixel_weights is None else self.pixel_weights[v]    # (None: the unweighted kernels)
                if self.bilagrid:     # the loss sees the render through the view's grid; no autograd node
                    raw, grid = image.detach(), self.grid_table.grids[v]
                    stats, dcorrected = gau_loss_with_grad(_appearance.slice_forward(raw, grid), self.gts[v],
                                                           grad_scale=1.0 / n_views, weight=wv)
                    dimage = _appearance.slice_backward(raw, grid, dcorrected, dgrid=self.grid_grad[self._grid_rows[v]])
                else:
                    stats, dimage = gau_loss_with_grad(image.detach(), self.gts[v], grad_scale=1.0 / n_views,
                                                       weight=wv)
                if qv is None and not with_n:
                    image.backward(dimage)
                else:      # the map terms' gradients join dL/dimage: one fused backward pass
                    ddepth = dalpha = None
                    if qv is not None:
                        dstats, ddepth, dalpha = self._depth_loss_with_grad(
                            out[2].detach(), out[3].detach(), qv, self.depth_kind, weight=wv,
                            alpha_min=self.depth_alpha_min, grad_scale=depth_scale)
                        depth_sum[k] += dstats[0]
                    if with_n:
                        nstats, ndepth, nalpha = self._normal_loss_with_grad(
                            out[2].detach(), out[3].detach(), self.cams[v], normals=nv, guide=self.gts[v],
                            smooth=self.normal_smooth > 0, weight=wv, alpha_min=self.normal_alpha_min,
                            edge_gamma=self.normal_edge_gamma, prior_scale=self.normal_weight / n_views,
                            smooth_scale=self.normal_smooth / n_views)
                        normal_sum[k] += nstats[:2]
                        ddepth = ndepth if ddepth is None else ddepth.add_(ndepth)
                        dalpha = nalpha if dalpha is None else dalpha.add_(nalpha)
                    torch.autograd.backward([image, out[2], out[3]], [dimage, ddepth, dalpha])
                if tw is not None:      # (per view, never accumulated in the kernel; one row per camera)
                    self.pose_grad[v] += tw.grad
                loss_sum[k] += stats[0]
                with torch.no_grad():                       # per-view ||dL/du|| (undo the 1/len scaling)
                    g = torch.norm((us.absgrad if self.absgrad else us.grad) * n_views, dim=-1)
                    gnorm[k] += torch.where(mask, g, torch.zeros_like(g))
                    count[k] += mask.to(torch.int32)
        if vs is not None:
            vs.finish()                                    # the caller's stream now follows every lane
            for k in range(1, lanes):
                for t in (loss_sum[k], gnorm[k], count[k]):
                    t.record_stream(torch.cuda.current_stream())
                loss_sum[0] += loss_sum[k]; gnorm[0] += gnorm[k]; count[0] += count[k]
                if depth_sum is not None:
                    depth_sum[k].record_stream(torch.cuda.current_stream())
                    depth_sum[0] += depth_sum[k]
                if normal_sum is not None:
                    normal_sum[k].record_stream(torch.cuda.current_stream())
                    normal_sum[0] += normal_sum[k]
        # (the depth terms of this rank's views; a rank whose views have no prior still takes part in the all-reduce)
        self._depth_sum = None if self.depth_priors is None else \
            (depth_sum[0] if depth_sum is not None else torch.zeros((), device=self.device))
        self._normal_sum = None if not self.normals_on else \
            (normal_sum[0] if normal_sum is not None else torch.zeros(2, device=self.device))
        return loss_sum[0], gnorm[0], count[0]

    def step(self, view_ids: Sequence[int], sync: bool = True):
        """One optimizer step on the mean gradient over ``view_ids`` (all ranks pass the same list, which must
        give every rank at least one view: a rank without a view would have no gradient to contribute and
        its peers would wait in the all-reduce for ever).  Returns the mean loss: a float (``sync=True``: the
        ``loss.item()`` of train.py:58, one host-device synchronisation per step) or, with ``sync=False``, a
        0-dim device tensor -- the host then never waits for the GPU inside the step (``fit`` uses this and
        reads the losses once per epoch)."""
        if len(view_ids) < self.world:
            raise ValueError("step() got %d view(s) for %d ranks: every rank needs at least one view per step"
                             % (len(view_ids), self.world))
        if self.pose_opt and len(set(view_ids)) != len(view_ids):
            raise ValueError("step() with pose_opt: a camera appears twice in %r (its twist takes one step per step)"
                             % (list(view_ids),))
        if self.bilagrid and len(set(view_ids)) != len(view_ids):
            raise ValueError("step() with bilagrid: a view appears twice in %r (its grid takes one step per step)"
                             % (list(view_ids),))
        mine = [view_ids[i] for i in DV.views_for_rank(len(view_ids), self.rank, self.world)]
        self.opt.zero_grad(set_to_none=True)
        self._clear_pose_grad()
        self._clear_grid_grad(view_ids)
        # The views are rendered with deferred validation: the host does not wait for a patch count inside the
        # step.  commit() (one wait for the binning stage of the last view, while its draw and backward
        # kernels are still queued) tells whether some view outgrew the buffers sized from earlier renders;
        # that happens while the trainer still meets new views, and the step is then redone exactly.
        # (from the second local view on the chain-rule kernel adds to the leaves' .grad itself: accumulate_in_kernel)
        # The SH gradient of the step stays factored when that moves fewer bytes (dist_views.FactoredShGrad: a view
        # leaves dL/dcolour [N,3]; 12 B per Gaussian and view are all-gathered instead of 192 B per Gaussian
        # all-reduced, and on one rank V views write 12 V + 192 B instead of accumulating 192-B rows V times)
        fx = None
        vmax = -(-len(view_ids) // self.world)      # rows per rank: the same on every rank (one all-gather)
        # (on one rank it pays from the second view on -- or from the first when the optimizer consumes the factored
        # form directly, FusedAdam: the 192-B rows are then never written at all)
        if self.factored_sh and self.fused_activations and \
                (DV.factored_exchange_pays(self.world, vmax, 3 + self.params["high_shs"].shape[1]) or
                 (self.world == 1 and isinstance(self.opt, FusedAdam))):
            if self._fx is None or self._fx.views != vmax:
                self._fx = DV.FactoredShGrad(vmax)
            fx = self._fx
        # every render of the step carries its own options (no process-wide switch): gradients of further views are
        # added inside the chain-rule kernel, the SH gradient goes to this trainer's own FactoredShGrad
        opts = RenderOptions(mode=self.mode, accumulate=True, sh_sink=fx, antialiased=self.antialiased,
                             absgrad=self.absgrad)
        if fx is not None:     # (rows allocated here, on the caller's stream, before the views fork onto their lanes)
            fx.begin_step(self.params["pws"].shape[0], self.params["pws"].device)
        with _fused.deferred() as d:
            loss_sum, gnorm, count = self._render_views(mine, len(view_ids), opts)
            incomplete = d.commit()
        if incomplete:
            self.redone_steps += 1
            self.opt.zero_grad(set_to_none=True)
            self._clear_pose_grad()
            self._clear_grid_grad(view_ids)
            if fx is not None:
                fx.restart()
            loss_sum, gnorm, count = self._render_views(mine, len(view_ids), opts)   # validated render by render
        others = self.params
        sh_rows = None
        if fx is not None:   # (a collective when world > 1; the loss already carries 1 / views: a SUM over ranks)
            if isinstance(self.opt, FusedAdam):
                # the optimizer forms each Gaussian's SH gradient row in LDS (egs_adam_sh_factored): the 4 sh_dim-byte
                # rows are never written or read
                taken = fx.take()
                sh_rows = None if taken is None else (taken[0], 1.0, self.params["pws"], self.params["low_shs"],
                                                      self.params["high_shs"])
            else:
                fx.finish(self.params["pws"], self.params["low_shs"], self.params["high_shs"], average=False)
            others = {k: v for k, v in self.params.items() if k not in ("low_shs", "high_shs")}
        if self.bilagrid:    # TV of the step's grids, added by the rank that rendered the view: once per row
            self.last_tv = torch.zeros((), device=self.device)
            for v in mine:
                self.last_tv += _appearance.tv(self.grid_table.grids[v], self.bilagrid_tv,
                                               self.grid_grad[self._grid_rows[v]])
        if self.world > 1:   # sum over ranks of (sum over local views)/V == mean over all views
            DV.allreduce_sum_(DV.coalesce_grads(list(others.values())) + [gnorm, count, loss_sum] +
                              ([self.pose_grad] if self.pose_opt else []) +
                              ([self.grid_grad, self.last_tv] if self.bilagrid else []) +
                              ([self._depth_sum] if self.depth_priors is not None else []) +
                              ([self._normal_sum] if self.normals_on else []))
        self.grad_accum += gnorm
        self.vis_count += count
        if self.mcmc is not None:     # after the all-reduce: identical on every rank
            self.mcmc.add_regularisers(self.params)
        if self.sparse_adam:          # (count: after the all-reduce, so the mask is identical on every rank)
            self.opt.step(factored_sh=sh_rows, visible=count > 0)
        elif sh_rows is not None:
            self.opt.step(factored_sh=sh_rows)
        else:
            self.opt.step()
        if self.mcmc is not None:     # with the learning rate the step just used
            self.mcmc.inject_noise(self.params, [g["lr"] for g in self.opt.param_groups if g["name"] == "pws"][0])
        if self.pose_opt:       # the cameras of this step only: the others keep twist, moments and step count
            self.pose_table.step(view_ids, self.pose_grad)
        if self.bilagrid:       # the views of this step only: the other grids keep values, moments and step count
            self.grid_table.step(view_ids, self.grid_grad)
        self.density.update_pws_lr(self.opt)                                     # gsmodel.py:180-183, 332-338
        self.iteration += 1
        if self.depth_priors is not None:   # the mean unweighted depth term over the step's views that have a prior
            with_prior = sum(1 for v in view_ids if self.depth_priors[v] is not None)
            self.last_depth_loss = self._depth_sum / max(with_prior, 1)
        if self.normals_on:     # (L_p over the step's views that have a prior, L_s over the step's views)
            with_prior = 0 if self.normal_priors is None else \
                sum(1 for v in view_ids if self.normal_priors[v] is not None)
            self.last_normal_loss = torch.stack([self._normal_sum[0] / max(with_prior, 1),
                                                 self._normal_sum[1] / len(view_ids)])
        mean = loss_sum / len(view_ids)
        return float(mean) if sync else mean

    def _clear_pose_grad(self):
        """the pose gradients of a step start from zero -- also when the step is redone"""
        if self.pose_grad is not None:
            self.pose_grad.zero_()

    def _clear_grid_grad(self, view_ids):
        """the grid gradients of a step start from zero -- also when the step is redone.  One row per view of the step
        (kept across steps of the same size), and the view -> row map the renders use"""
        if not self.bilagrid:
            return
        rows = (len(view_ids),) + tuple(self.grid_table.grids.shape[1:])
        if self.grid_grad is None or tuple(self.grid_grad.shape) != rows:
            self.grid_grad = torch.zeros(rows, device=self.device)
        else:
            self.grid_grad.zero_()
        self._grid_rows = {int(v): k for k, v in enumerate(view_ids)}

    def grids(self):
        """-> [V,12,L,Gh,Gw]: the current bilateral grid of every training image (None without ``bilagrid``)"""
        return None if self.grid_table is None else self.grid_table.grids

    def save_grids(self, fn: str):
        """The grids as an ``.npz``: ``ids`` [V] (``Camera.id``), ``grids`` [V,12,L,Gh,Gw], ``shape`` = (Gw, Gh, L)."""
        if self.grid_table is None:
            raise ValueError("save_grids: this trainer has no grids (bilagrid=False)")
        self.grid_table.save(fn, ids=[getattr(c, "id", i) for i, c in enumerate(self.cams)])

    def corrected(self, view_id: int, image):
        """``image`` [3,H,W] through the grid of training image ``view_id`` -- what the loss of that view compares with
        its photograph.  For inspection: a novel view has no grid."""
        if self.grid_table is None:
            raise ValueError("corrected: this trainer has no grids (bilagrid=False)")
        return _appearance.slice_forward(image.detach(), self.grid_table.grids[int(view_id)])

    def poses(self):
        """-> (Rcw [V,3,3], tcw [V,3]): the current pose of every camera (the stored ones without ``pose_opt``)"""
        if self.pose_table is None:
            return torch.stack([c.Rcw for c in self.cams]), torch.stack([c.tcw for c in self.cams])
        return self.pose_table.poses()

    def save_poses(self, fn: str):
        """The current camera poses as an ``.npz``: ``ids`` [V] (``Camera.id``), ``Rcw`` [V,3,3], ``tcw`` [V,3]."""
        R, t = self.poses()
        ids = np.asarray([getattr(c, "id", i) for i, c in enumerate(self.cams)])
        np.savez(fn, ids=ids, Rcw=R.detach().cpu().numpy(), tcw=t.detach().cpu().numpy())

    def densify(self, verbose: bool = False):
        """Prune / clone / split on the statistics gathered since the last call (train.py:71-73 ->
        gsmodel.py:232-317).  Identical on every rank (statistics are already all-reduced).  With strategy "mcmc":
        relocate the dead Gaussians, then grow towards ``cap_max`` (the statistics are not used)."""
        if self.mcmc is not None:
            report = self.mcmc.relocate(self.params, self.opt)
            report.update(self.mcmc.grow(self.params, self.opt))
            if verbose:
                print("mcmc density update report: relocated %(relocated)d added %(added)d total %(total)d" % report)
        else:
            self.density.set_density_info(self.grad_accum, self.vis_count)
            report = self.density.update_gaussian_density(self.params, self.opt, verbose=verbose)
        n = self.params["pws"].shape[0]
        self.grad_accum = torch.zeros(n, device=self.device)
        self.vis_count = torch.zeros(n, dtype=torch.int32, device=self.device)
        return report

    def reset_alpha(self):
        """train.py:74-76 -> gsmodel.py:319-330."""
        self.density.reset_alpha(self.params, self.opt)

    def importance(self, view_ids: Sequence[int] = None):
        """-> ``importance.BlendStats``: sum / max / count of the blending weight every Gaussian receives over the views
        ``view_ids`` (default: all cameras).  Each rank renders its share, forward only, with this
        trainer's ``antialiased`` and -- with ``pose_opt`` -- the current poses; the statistics are then all-reduced, so
        every rank holds the same ones."""
        view_ids = list(range(len(self.cams))) if view_ids is None else [int(v) for v in view_ids]
        mine = [view_ids[i] for i in DV.views_for_rank(len(view_ids), self.rank, self.world)]
        p = self.params
        st = _importance.BlendStats(p["pws"].shape[0], p["pws"].device)
        with torch.no_grad():
            if self.fused_activations:
                args, high = (p["pws"], p["low_shs"], p["alphas_raw"], p["scales_raw"], p["rots_raw"]), p["high_shs"]
            else:
                args, high = activate(p), None
            poses = self.pose_table.poses() if self.pose_table is not None else None
            for v in mine:
                cam = self.cams[v]
                if poses is not None:
                    cam = Camera(cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy, poses[0][v].detach(),
                                 poses[1][v].detach(), self.device, id=cam.id, path=cam.path)
                _importance.render_weights(st, *args, cam, high_shs=high, antialiased=self.antialiased)
        if self.world > 1:
            st.allreduce_()
        return st

    def render_features(self, view_id: int, feats):
        """-> [C,H,W]: ``feats`` ([N,C] float32, one row per Gaussian) rendered into camera ``view_id`` with the current
        parameters (``features.render``), with this trainer's ``antialiased`` and -- with ``pose_opt`` --
        the current pose.  No gradient."""
        p = self.params
        with torch.no_grad():
            if self.fused_activations:
                args, high = (p["pws"], p["low_shs"], p["alphas_raw"], p["scales_raw"], p["rots_raw"]), p["high_shs"]
            else:
                args, high = activate(p), None
            cam = self.cams[int(view_id)]
            if self.pose_table is not None:
                poses = self.pose_table.poses()
                cam = Camera(cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy, poses[0][int(view_id)].detach(),
                             poses[1][int(view_id)].detach(), self.device, id=cam.id, path=cam.path)
            return _features.render(feats, *args, cam, high_shs=high, antialiased=self.antialiased)

    def extract_mesh(self, view_ids: Sequence[int] = None, voxel_size: float = None, bounds=None, trunc: float = None,
                     min_weight: float = None, color: bool = True, min_component_faces: int = None,
                     keep_largest: int = None, smooth_iterations: int = 0, simplify_voxels: float = None,
                     simplify_placement: str = "quadric", sparse: bool = False, **integrate_kwargs):
        """-> (vertices [V,3] float32, faces [F,3] int64, colors [V,3] float32 or None): the scene's surface as a triangle
        mesh (``mesh.TSDFVolume``).  Every view of ``view_ids`` (default: all cameras) is rendered with its
        depth and opacity maps, forward only, with this trainer's ``antialiased`` and -- with ``pose_opt`` -- the current
        poses, and fused into one volume with the rendered image as colour; the zero level set is then extracted.
        ``bounds`` = ((x0, y0, z0), (x1, y1, z1)) defaults to the 1st-99th percentile box of the Gaussian centres padded by
        the truncation distance, ``voxel_size`` to the longest side of that box / 256, ``trunc`` to 4 voxels,
        ``min_weight`` to 1; ``integrate_kwargs`` (``alpha_min`` = 0.5, ``near``, ``depth_max``, ``clip_to_frustum``) go to
        ``TSDFVolume.integrate``.  These defaults are values NOBODY HAS TUNED.  Parameters, gradients and optimizer state
        are left as they are; every rank that calls this fuses all the views itself.

        Cleaning (``mesh.clean_mesh``), all off by default -- a default call returns what it always did,
        bit for bit: ``min_component_faces`` drops the connected components with fewer faces (the floaters a TSDF of
        splat depth maps carries), ``keep_largest`` = k keeps only the k components with the most faces,
        ``smooth_iterations`` > 0 then runs that many Taubin iterations (lambda 0.5, mu -0.53: untuned too).

        Simplification (``mesh.simplify_vertex_clustering``), off by default and run after the cleaning:
        ``simplify_voxels`` = k merges the vertices of every cell of k x ``voxel_size`` on the grid that starts at the
        volume's origin into one vertex, placed by ``simplify_placement`` ("quadric", whose regulariser 1e-3 is untuned, or
        "mean"), and drops the faces that collapse.  Topology is not preserved.  (The grid's origin must not exceed the
        mesh's bounding box: smoothing that pushes a surface at the volume's wall below the origin ends in a ValueError.)

        ``sparse`` = True fuses into a ``mesh.SparseTSDFVolume``, which stores only the 8^3 blocks near the
        observed surfaces: the defaults stay what they are, but ``voxel_size`` may then be far finer than a dense
        volume could hold.  A block is updated only from the view that allocates it onwards, and the surface ends where
        the allocation ends.  ``sparse`` = False, the default, returns what it always did, bit for bit."""
        from . import mesh as _mesh
        if simplify_voxels is not None:
            _mesh._cell_size(simplify_voxels, "simplify_voxels")
            _mesh._placement(simplify_placement, "simplify_placement")
        view_ids = list(range(len(self.cams))) if view_ids is None else [int(v) for v in view_ids]
        p = self.params
        with torch.no_grad():
            if bounds is None:
                pw = p["pws"].detach()
                n = pw.shape[0]
                if n == 0:
                    raise ValueError("extract_mesh needs bounds: the scene has no Gaussian")
                srt = torch.sort(pw, dim=0).values
                lo = srt[min(n - 1, int(0.01 * (n - 1)))].double().cpu().numpy()
                hi = srt[int(math.ceil(0.99 * (n - 1)))].double().cpu().numpy()
                pad = None
            else:
                lo, hi = (np.asarray(b, np.float64).reshape(3) for b in bounds)
                pad = 0.0
            if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (hi > lo).all()):
                raise ValueError("bounds must be a finite box with a positive extent, got %r, %r" % (lo, hi))
            voxel = float(voxel_size) if voxel_size is not None else float((hi - lo).max()) / 256.0
            if not (math.isfinite(voxel) and voxel > 0):
                raise ValueError("voxel_size must be finite and > 0, got %r" % (voxel_size,))
            trunc = _mesh.TRUNC_VOXELS * voxel if trunc is None else float(trunc)
            pad = trunc if pad is None else pad
            lo, hi = lo - pad, hi + pad
            dims = tuple(int(math.ceil((h - l) / voxel - 1e-9)) + 1 for l, h in zip(lo, hi))
            vol = (_mesh.SparseTSDFVolume if sparse else _mesh.TSDFVolume)(tuple(lo), voxel, dims, trunc=trunc,
                                                                           color=color, device=self.device)
            if self.fused_activations:
                args, fn = (p["pws"], p["low_shs"], p["high_shs"], p["alphas_raw"], p["scales_raw"], p["rots_raw"]), \
                    GSRawFunction
            else:
                args, fn = activate(p), GSFunction
            opts = RenderOptions(mode=self.mode, depth=True, alpha=True, antialiased=self.antialiased)
            poses = self.pose_table.poses() if self.pose_table is not None else None
            us = torch.zeros((p["pws"].shape[0], 2), device=self.device)
            for v in view_ids:
                cam = self.cams[v]
                if poses is not None:
                    cam = Camera(cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy, poses[0][v].detach(),
                                 poses[1][v].detach(), self.device, id=cam.id, path=cam.path)
                out = fn.apply(*args, us, cam, opts)
                vol.integrate(out[2], out[3], cam, image=out[0].contiguous() if color else None, **integrate_kwargs)
            V, F, C = vol.extract(_mesh.MIN_WEIGHT if min_weight is None else min_weight)
            if min_component_faces is not None or keep_largest is not None or smooth_iterations:
                # (extract guarantees the index range: no aminmax readback)
                V, F, C, _ = _mesh.clean_mesh(V, F, C, min_faces=min_component_faces, keep_largest=keep_largest,
                                              smooth_iterations=smooth_iterations, check=False)
            if simplify_voxels is not None:
                V, F, C = _mesh.simplify_vertex_clustering(V, F, C, cell_size=float(simplify_voxels) * voxel,
                                                           origin=vol.origin, placement=simplify_placement, check=False)
            return V, F, C

    def prune_by_importance(self, score: str = "max", threshold=None, fraction=None, view_ids: Sequence[int] = None,
                            verbose: bool = False):
        """Remove the Gaussians whose ``score`` ("max", "sum" or "hits" of ``importance()``) lies below ``threshold``,
        or the ``fraction`` of them with the lowest score (``importance.keep_mask``).  Identical on every rank.
        -> dict(pruned, total)"""
        st = self.importance(view_ids)
        keep = _importance.keep_mask(st, score=score, threshold=threshold, fraction=fraction)
        report = self.density.prune(self.params, self.opt, keep)
        n = self.params["pws"].shape[0]
        self.grad_accum = torch.zeros(n, device=self.device)
        self.vis_count = torch.zeros(n, dtype=torch.int32, device=self.device)
        if verbose:
            print("importance pruning report (%s): pruned %d total %d" % (score, report["pruned"], report["total"]))
        return report

    def fit(self, epochs: int, views_per_step: int = None, rng_seed: int = 0, densify_every: int = 5,
            reset_alpha_every: int = 15, densify_until: int = 50, verbose: bool = False,
            prune_importance_at: Sequence[int] = (), prune_score: str = "max", prune_threshold=None,
            prune_fraction=None) -> List[float]:
        """The epoch loop of train.py:44-80: shuffled views, ``views_per_step`` views per optimizer step
        (1 in the reference), densification every 5th and alpha reset every 15th epoch in (1, 50].
        ``prune_importance_at``: epochs at whose end ``prune_by_importance(prune_score, prune_threshold,
        prune_fraction)`` runs over all cameras (after that epoch's densification, if any); empty: never."""
        prune_at = set(int(e) for e in prune_importance_at)
        vps = views_per_step or self.world
        if vps < self.world or len(self.cams) < self.world:
            raise ValueError("views_per_step=%d, %d cameras: every one of the %d ranks needs a view in each step"
                             % (vps, len(self.cams), self.world))
        order_rng = np.random.default_rng(rng_seed)            # same permutation on every rank
        history = []
        for epoch in range(epochs):
            idxs = order_rng.permutation(len(self.cams))
            total, steps = torch.zeros((), device=self.device), 0
            # every view is visited each epoch (train.py:48): the last step of an epoch takes the remaining
            # views when they still give every rank one, otherwise they join the step before it
            cuts = list(range(0, len(idxs), vps))
            if len(cuts) > 1 and len(idxs) - cuts[-1] < self.world:
                cuts.pop()
            for j, i in enumerate(cuts):
                end = cuts[j + 1] if j + 1 < len(cuts) else len(idxs)
                total += self.step([int(v) for v in idxs[i:end]], sync=False)
                steps += 1
            history.append(float(total) / max(steps, 1))
            if verbose and self.rank == 0:
                print("epoch:%d avg_loss:%f" % (epoch, history[-1]))
            if 1 < epoch <= densify_until:
                if epoch % densify_every == 0:
                    self.densify(verbose and self.rank == 0)
                if epoch % reset_alpha_every == 0 and self.mcmc is None:     # (MCMC: dead Gaussians are relocated)
                    self.reset_alpha()
            if epoch in prune_at:
                self.prune_by_importance(prune_score, prune_threshold, prune_fraction,
                                         verbose=verbose and self.rank == 0)
        return history

    def save(self, fn: str) -> np.ndarray:
        """Checkpoint of ACTIVATED parameters, dtype == gau_io.py:7-12 (gau_io.py:141-156)."""
        gs = self._records()
        np.save(fn, gs)
        return gs

    def _records(self) -> np.ndarray:
        """the ACTIVATED parameters as a record array (``gsdata_type``)"""
        with torch.no_grad():
            pws, shs, alphas, scales, rots = (x.detach().cpu().numpy() for x in activate(self.params))
        return np.rec.fromarrays([pws, rots, scales, alphas.reshape(-1), shs], dtype=gsdata_type(shs.shape[1]))

    def save_compressed(self, fn: str, clusters: int = None, iters: int = 10, weight_by: str = None):
        """The Gaussians ``save`` writes, as a compressed scene (``compress.save_compressed``): the SH rest
        against a k-means codebook of ``clusters`` centroids (default min(65536, N // 4): gsplat's figure, untuned here),
        the other attributes at 8 or 16 bits.  ``weight_by`` = "sum" or "max" weights the codebook by that blending-weight
        statistic of ``importance()`` over all cameras (LightGaussian's weighting).  -> the dict of arrays written.

        With ``weight_by`` set and several ranks this is a COLLECTIVE, unlike ``save``: ``importance()`` renders each
        rank's share of the views and all-reduces, so every rank must enter the call; rank 0 then clusters and writes the
        file and the other ranks return None.  Without ``weight_by`` nothing is exchanged: call it on the rank that writes."""
        from . import compress
        if weight_by not in (None, "sum", "max"):
            raise ValueError("weight_by must be None, 'sum' or 'max', got %r" % (weight_by,))
        weights = None
        if weight_by is not None:
            st = self.importance()
            if self.world > 1 and self.rank != 0:
                return None
            weights = (st.sum if weight_by == "sum" else st.max).contiguous()
        return compress.save_compressed(fn, self._records(), clusters=clusters, iters=iters, weights=weights)
