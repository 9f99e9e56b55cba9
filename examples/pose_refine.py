#!/usr/bin/env python3
"""Photometric camera pose refinement through ``GSPoseFunction``: render a target at a true pose, perturb the pose by a
twist, and optimise the twist with Adam against the target image (the Gaussians stay fixed).

    python examples/pose_refine.py [--n 20000] [--steps 150] [--deg 2.0] [--shift 0.05] [--sh-dim 12] [--pose-only]

The twist (omega, rho) acts on the perturbed pose (R0, t0) as  R = exp([omega]x) R0,  t = exp([omega]x) t0 + rho,
written in torch ops (easygaussiansplatting_amd.pose), so autograd carries dL/dRcw and dL/dtcw of the fused backward pass
to the six twist parameters.
Prints the rotation error (degrees) and the translation error (relative to the camera distance) as it goes.
"""
import argparse
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402


def pose_error(R, t, R_true, t_true, dist):
    """-> (rotation error in degrees, translation error / camera distance)"""
    c = float(np.clip((np.trace(R_true.T @ R) - 1.0) / 2.0, -1.0, 1.0))
    return math.degrees(math.acos(c)), float(np.linalg.norm(t - t_true)) / dist


def make_scene(n=20_000, width=320, height=240, sh_dim=12, seed=0):
    """scene.small_scene with Gaussians three times as large: a smoother image, a wider basin for the photometric loss"""
    from easygaussiansplatting_amd import scene as S
    sc = S.small_scene(n, width, height, sh_dim, seed=seed)
    sc.scales = sc.scales * np.float32(3.0)
    return sc


def refine(sc, steps=150, deg=2.0, shift=0.05, lr_rot=2e-3, lr_trans=4e-3, decay=0.98, seed=0, log=None,
           pose_only=False):
    """Perturb the scene camera by a twist of ``deg`` degrees and ``shift`` x the camera distance, optimise it back
    (``pose.refine_pose``).  ``pose_only``: the backward pass forms the camera gradient alone.
    -> list of (step, rotation error deg, translation error rel) from before the first step to after the last."""
    import torch
    from easygaussiansplatting_amd.function import Camera, GSPoseFunction
    from easygaussiansplatting_amd.pose import exp_so3, refine_pose

    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    cam = Camera.from_scene(sc.cam)
    params = [dev(sc.pws), dev(sc.shs), dev(sc.alphas).reshape(-1, 1), dev(sc.scales), dev(sc.rots)]
    us = torch.zeros((sc.n, 2), device="cuda")
    R_true = np.asarray(sc.cam.Rcw, np.float64)
    t_true = np.asarray(sc.cam.tcw, np.float64)
    dist = float(np.linalg.norm(t_true))
    with torch.no_grad():
        target, _ = GSPoseFunction.apply(*params, us, dev(R_true), dev(t_true), cam)
    # the perturbation: a random rotation axis and translation direction
    rng = np.random.default_rng(seed)
    ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
    dr = rng.normal(size=3); dr /= np.linalg.norm(dr)
    w0 = torch.tensor(ax * math.radians(deg), dtype=torch.float64)
    R0 = exp_so3(w0).numpy() @ R_true
    t0 = exp_so3(w0).numpy() @ t_true + dr * shift * dist
    hist = []

    def record(step, R, t):
        hist.append((step,) + pose_error(R.double().cpu().numpy(), t.double().cpu().numpy(), R_true, t_true, dist))
        if log is not None and (step % 10 == 0 or step == steps):
            log("step %3d  rotation error %.4f deg  translation error %.5f" % hist[-1])
    refine_pose(params, cam, target, steps, lr_rot, lr_trans * dist, decay, Rcw=dev(R0), tcw=dev(t0),
                pose_only=pose_only, callback=record)
    return hist


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20_000)
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--sh-dim", type=int, default=12, choices=[3, 12, 27, 48])
    ap.add_argument("--steps", type=int, default=150)
    ap.add_argument("--deg", type=float, default=2.0, help="rotation of the perturbation, degrees")
    ap.add_argument("--shift", type=float, default=0.05, help="translation of the perturbation / camera distance")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--pose-only", action="store_true",
                    help="backward pass forms the camera gradient alone, no per-Gaussian gradients (DESIGN §3.8)")
    a = ap.parse_args()
    sc = make_scene(a.n, a.width, a.height, a.sh_dim, a.seed)
    hist = refine(sc, a.steps, a.deg, a.shift, seed=a.seed, log=print, pose_only=a.pose_only)
    (_, r0, t0), (_, r1, t1) = hist[0], hist[-1]
    print("rotation error %.4f -> %.4f deg (%.1fx), translation error %.5f -> %.5f (%.1fx)"
          % (r0, r1, r0 / max(r1, 1e-12), t0, t1, t0 / max(t1, 1e-12)))


if __name__ == "__main__":
    main()
