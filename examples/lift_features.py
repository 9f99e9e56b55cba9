"""Training-free lifting of 2D label maps onto the Gaussians, and rendering them into an unseen view.

    python examples/lift_features.py [--gaussians 20000] [--width 256] [--height 192]

A synthetic scene from ``scene.py``; every Gaussian gets a ground-truth one-hot label, the octant of its position.  The
label maps of 7 of 8 ring cameras are rendered (``features.render_features``), lifted back onto the Gaussians with
``features.lift`` -- f_g = sum_v sum_p w F_v(p) / sum_v sum_p w, no optimisation -- and the lifted labels are rendered
into the 8th view.  Prints the per-pixel arg-max agreement of that render with the ground-truth render of the view.
A demonstration, not a test."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=20000)
    ap.add_argument("--width", type=int, default=256)
    ap.add_argument("--height", type=int, default=192)
    a = ap.parse_args()
    import torch
    from easygaussiansplatting_amd import features, fused, scene as S
    from easygaussiansplatting_amd.function import Camera
    dev = torch.device("cuda:0")
    sc = S.small_scene(a.gaussians, a.width, a.height, 48)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)
    P = [t(sc.pws), t(sc.shs), t(sc.alphas), t(sc.scales), t(sc.rots)]
    octant = (sc.pws[:, 0] > 0).astype(np.int64) + 2 * (sc.pws[:, 1] > 0) + 4 * (sc.pws[:, 2] > 0)
    truth = torch.from_numpy(np.eye(8, dtype=np.float32)[octant]).to(dev)           # [N,8] one-hot
    cams = [Camera.from_scene(c, dev) for c in S.ring_cameras(sc.cam, 8, radius=5.0)]
    with torch.no_grad():
        states = [fused.forward(*P, cam, need_grad=False)[2] for cam in cams]
        maps = [features.render_features(st, truth) for st in states[:7]]
        lifted, seen = features.lift(states[:7], maps)
        want = features.render_features(states[7], truth)
        got = features.render_features(states[7], lifted)
    covered = want.sum(0) > 1e-3
    agree = (want.argmax(0) == got.argmax(0)) & covered
    per_gaussian = (lifted.argmax(1) == truth.argmax(1)) & seen
    print("lifted %d of %d Gaussians from 7 views; their arg-max label is the true one for %.1f %% of them"
          % (int(seen.sum()), sc.n, 100.0 * float(per_gaussian.sum()) / max(int(seen.sum()), 1)))
    print("held-out view: arg-max label agrees with the ground-truth render on %.1f %% of %d covered pixels"
          % (100.0 * float(agree.sum()) / max(int(covered.sum()), 1), int(covered.sum())))


if __name__ == "__main__":
    main()
