"""Camera pose parameters on top of the pose nodes (``GSPoseFunction`` / ``GSRawPoseFunction``).

A pose is refined as a twist (omega, rho) on a stored pose (R0, t0):

    R = exp([omega]x) R0,    t = exp([omega]x) t0 + rho

written in torch ops, so autograd carries the dL/dRcw and dL/dtcw of the fused backward pass to the six parameters.

* ``exp_so3`` / ``apply_twist``: the parameterisation;
* ``refine_pose``: one camera against a FROZEN map (tracking, relocalisation) -- by default with
  ``RenderOptions(pose_only=True)``, whose backward pass forms the camera gradient and nothing per Gaussian;
* ``PoseTable``: one twist per training camera with a per-row Adam, for ``Trainer(pose_opt=True)``.

Default learning rates (``LR_ROT`` per radian, ``LR_TRANS`` times the camera distance |tcw|) are those of
examples/pose_refine.py: found for frozen-map refinement on a synthetic scene, NOT tuned for joint training of map and
poses -- nobody has measured that.
"""
from __future__ import annotations

import math

import torch

LR_ROT = 2e-3       # Adam step of the rotation half (radians)
LR_TRANS = 4e-3     # Adam step of the translation half, as a fraction of the camera distance |tcw|


def hat(w):
    z = torch.zeros((), dtype=w.dtype, device=w.device)
    return torch.stack([torch.stack([z, -w[2], w[1]]), torch.stack([w[2], z, -w[0]]),
                        torch.stack([-w[1], w[0], z])])


def exp_so3(w):
    """Rodrigues' formula in torch ops (differentiable, also at w = 0)"""
    th2 = (w * w).sum()
    th = torch.sqrt(th2 + 1e-24)
    K = hat(w)
    a = torch.where(th2 > 1e-12, torch.sin(th) / th, 1.0 - th2 / 6.0)
    b = torch.where(th2 > 1e-12, (1.0 - torch.cos(th)) / (th2 + 1e-24), 0.5 - th2 / 24.0)
    return torch.eye(3, dtype=w.dtype, device=w.device) + a * K + b * (K @ K)


def apply_twist(R0, t0, omega, rho):
    """-> (R, t) = (exp([omega]x) R0, exp([omega]x) t0 + rho)"""
    E = exp_so3(omega)
    return E @ R0, E @ t0 + rho


def refine_pose(params, cam, target, steps=150, lr_rot=LR_ROT, lr_trans=None, decay=0.98, raw=False, opts=None,
                Rcw=None, tcw=None, pose_only=True, callback=None):
    """Refine one camera pose against ``target`` [3,H,W] with the map ``params`` held fixed: Adam on the twist of the
    starting pose, loss = mean |render - target|.

    ``params``: (pws, shs, alphas, scales, rots), or with ``raw`` the six raw tensors of ``GSRawPoseFunction``.
    ``cam``: size and intrinsics, and the starting pose unless ``Rcw`` / ``tcw`` (float32 device tensors) give it.
    ``lr_trans``: absolute step of the translation half; None = ``LR_TRANS`` x |tcw| of the starting pose.
    ``decay``: per-step exponential decay of both rates.  ``opts``: the ``RenderOptions`` of the renders (extras,
    antialiased); ``pose_only`` (default) is set on them -- the backward pass then writes no per-Gaussian gradient.
    ``callback(step, Rcw, tcw)`` is called before every step and once after the last.
    -> (Rcw [3,3], tcw [3], history = [loss of every step as 0-dim device tensors])."""
    import dataclasses
    from .function import GSPoseFunction, GSRawPoseFunction, RenderOptions
    node = GSRawPoseFunction if raw else GSPoseFunction
    if pose_only:
        opts = dataclasses.replace(RenderOptions() if opts is None else opts, pose_only=True)
    elif opts is not None and opts.pose_only:
        opts = dataclasses.replace(opts, pose_only=False)
    params = [p.detach() for p in params]
    dev = params[0].device
    R0 = (cam.Rcw if Rcw is None else Rcw).detach().to(dev)
    t0 = (cam.tcw if tcw is None else tcw).detach().to(dev)
    if lr_trans is None:
        lr_trans = LR_TRANS * float(torch.linalg.norm(t0))
    us = torch.zeros((params[0].shape[0], 2), device=dev)
    omega = torch.zeros(3, device=dev, requires_grad=True)
    rho = torch.zeros(3, device=dev, requires_grad=True)
    opt = torch.optim.Adam([{"params": [omega], "lr": lr_rot}, {"params": [rho], "lr": lr_trans}])
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, decay)
    history = []
    for step in range(steps):
        R, t = apply_twist(R0, t0, omega, rho)
        if callback is not None:
            callback(step, R.detach(), t.detach())
        img = node.apply(*params, us, R, t, cam, opts)[0]
        loss = (img - target).abs().mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        sched.step()
        history.append(loss.detach())
    with torch.no_grad():
        R, t = apply_twist(R0, t0, omega, rho)
    if callback is not None:
        callback(steps, R, t)
    return R, t, history


class PoseTable:
    """One twist (omega [3], rho [3]) per camera, all zero at the start, and an Adam that steps ROWS: a camera's twist,
    both moments and its step count move only in the steps that rendered it.  (A dense Adam over the table would
    decay the moments of every camera each step and move cameras on stale momentum.)

    A stepped row is ``torch.optim.Adam`` on that row alone -- the same torch ops in the same order, the rotation and
    the translation half as two parameter groups with learning rates ``lr_rot`` and ``lr_trans`` x |tcw| of the camera.

    ``twist`` [V,6], ``exp_avg`` [V,6], ``exp_avg_sq`` [V,6] live on ``device``; ``steps`` [V] int64 on the host (the
    bias corrections are host scalars: no device read-back in a step)."""

    def __init__(self, cameras, device="cuda", lr_rot=LR_ROT, lr_trans=LR_TRANS, betas=(0.9, 0.999), eps=1e-8):
        self.device = device
        f32 = torch.float32
        self.R0 = torch.stack([torch.as_tensor(c.Rcw, dtype=f32).reshape(3, 3) for c in cameras]).to(device)
        self.t0 = torch.stack([torch.as_tensor(c.tcw, dtype=f32).reshape(3) for c in cameras]).to(device)
        v = len(cameras)
        self.twist = torch.zeros((v, 6), dtype=f32, device=device)
        self.exp_avg = torch.zeros((v, 6), dtype=f32, device=device)
        self.exp_avg_sq = torch.zeros((v, 6), dtype=f32, device=device)
        self.steps = torch.zeros(v, dtype=torch.int64)
        dist = [float(torch.linalg.norm(torch.as_tensor(c.tcw, dtype=torch.float64).cpu())) for c in cameras]
        self.lr_rot = float(lr_rot)
        self.lr_trans = [float(lr_trans) * d for d in dist]      # per camera: a fraction of ITS distance
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)

    def __len__(self):
        return self.twist.shape[0]

    def leaf(self, v):
        """a fresh autograd leaf [6] holding camera v's twist (its ``.grad`` after backward is the row of ``step``)"""
        return self.twist[v].detach().clone().requires_grad_(True)

    def pose(self, v, twist=None):
        """-> (Rcw, tcw) of camera v under ``twist`` [6] (default: the table's row, no gradient)"""
        if twist is None:
            with torch.no_grad():
                return apply_twist(self.R0[v], self.t0[v], self.twist[v, :3], self.twist[v, 3:])
        return apply_twist(self.R0[v], self.t0[v], twist[:3], twist[3:])

    def poses(self):
        """-> (Rcw [V,3,3], tcw [V,3]) of every camera now"""
        pairs = [self.pose(v) for v in range(len(self))]
        return torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs])

    @torch.no_grad()
    def step(self, view_ids, grad):
        """One Adam step of the rows ``view_ids`` on ``grad`` [V,6] (rows outside ``view_ids`` are not read)."""
        b1, b2 = self.betas
        for v in sorted(set(int(i) for i in view_ids)):
            self.steps[v] += 1
            k = int(self.steps[v])
            bc1, bc2 = 1 - b1 ** k, 1 - b2 ** k
            g, m, s = grad[v], self.exp_avg[v], self.exp_avg_sq[v]
            m.lerp_(g, 1 - b1)                                   # torch/optim/adam.py _single_tensor_adam, op for op
            s.mul_(b2).addcmul_(g, g, value=1 - b2)
            denom = (s.sqrt() / math.sqrt(bc2)).add_(self.eps)
            for sl, lr in ((slice(0, 3), self.lr_rot), (slice(3, 6), self.lr_trans[v])):
                self.twist[v, sl].addcdiv_(m[sl], denom[sl], value=-(lr / bc1))
