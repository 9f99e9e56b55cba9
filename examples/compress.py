#!/usr/bin/env python3
"""From a saved scene to a compressed one: the SH rest against a k-means codebook built on the GPU, every other
attribute at 8 or 16 bits, one deflated ``.gsz`` archive that ``gau_io.load_gs`` reads back.

    python examples/compress.py IN OUT.gsz [--clusters K] [--iters I] [--views 8] [--size 512]

``IN`` is a checkpoint of ``examples/train.py`` (.npy record array) or a 3DGS .ply.  Prints both file sizes and, on a GPU, the
PSNR between renders of the original and of the decoded scene from a ring of cameras around the scene's centre.  The PSNR is
printed only: nobody has measured what a real capture loses, and the default number of centroids (min(65536, N // 4), gsplat's
figure) is untuned here.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("inp", metavar="IN", help="the saved scene (.npy record array, 3DGS .ply or .gsz)")
    ap.add_argument("out", metavar="OUT.gsz")
    ap.add_argument("--clusters", type=int, default=None, help="centroids of the SH codebook (default min(65536, N // 4))")
    ap.add_argument("--iters", type=int, default=10, help="Lloyd iterations")
    ap.add_argument("--views", type=int, default=8, help="cameras of the PSNR ring")
    ap.add_argument("--size", type=int, default=512, help="width and height of the PSNR renders")
    a = ap.parse_args()

    import numpy as np
    import torch
    from easygaussiansplatting_amd import compress
    from easygaussiansplatting_amd import scene as S
    from easygaussiansplatting_amd.gau_io import load_gs

    gs = load_gs(a.inp)
    compress.save_compressed(a.out, gs, clusters=a.clusters, iters=a.iters)
    back = compress.load_compressed(a.out)
    n_in, n_out = os.path.getsize(a.inp), os.path.getsize(a.out)
    print("%s: %d B, %s: %d B (%.1f x smaller, %.1f B per Gaussian)" % (a.inp, n_in, a.out, n_out, n_in / max(n_out, 1),
                                                                      n_out / max(len(gs), 1)))
    if not torch.cuda.is_available() or len(gs) == 0:
        return
    from easygaussiansplatting_amd.function import Camera, render
    pw = np.asarray(gs["pw"], np.float64)
    centre = np.median(pw, axis=0)
    radius = 2.5 * float(np.percentile(np.linalg.norm(pw - centre, axis=1), 90)) + 1e-3
    base = S.Camera(a.size, a.size, float(a.size), float(a.size), a.size / 2.0, a.size / 2.0, np.eye(3), np.zeros(3))
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v, np.float32)).cuda()
    psnr = []
    with torch.no_grad():
        for cam in S.ring_cameras(base, a.views, radius=radius):
            cam.tcw = cam.tcw - cam.Rcw @ centre                      # the ring around the scene's centre
            c = Camera.from_scene(cam)
            ims = [render(dev(g["pw"]), dev(g["sh"].reshape(len(g), -1)), dev(g["alpha"]), dev(g["scale"]), dev(g["rot"]), c)[0]
                   for g in (gs, back)]
            mse = float(((ims[0] - ims[1]) ** 2).mean())
            psnr.append(10 * np.log10(1.0 / mse) if mse > 0 else float("inf"))
    print("PSNR of the decoded scene against the original over %d views: mean %.2f dB, worst %.2f dB" % (
        a.views, float(np.mean(psnr)), float(np.min(psnr))))


if __name__ == "__main__":
    main()
