#!/usr/bin/env python3
"""The block-allocated TSDF volume against the dense one, on the scene of tools/tsdf_bench.py.

    python tools/sparse_tsdf_bench.py [--height 1080 --width 1920] [--sizes 256 512 1024] [--reps 5] [--rounds 9]
                                      [--out profiles/sparse_tsdf_bench.json]

The scene: an analytic sphere (radius 0.7) in a volume over [-1, 1]^3, seen from 3 units away; six views around it are
fused with colour.  Per lattice size n^3:

    sparse/n/integrate      ``SparseTSDFVolume.integrate`` of one view into a volume that already holds all six: touch, mark,
                            scan, the one readback, and the fusion of every allocated block (no block is new, so the pool
                            does not grow while it is timed)
    dense/n/integrate       ``TSDFVolume.integrate`` of the same view (the frustum's sub-box), where the dense volume fits
    sparse/n/extract, dense/n/extract            ``extract_triangles`` (count, scan, one readback, emit)

and the allocated blocks against the blocks of the lattice, the bytes of the pools against the bytes of dense planes, and
the triangles.  A dense size that does not fit -- 2^31 samples or more, or more memory than the device has free -- is
recorded as "not measured" with the reason.  Times are per call, median / min / max over the rounds of HIP-event brackets.

This is not ``bench.py``; nothing here is a gate.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import numpy as np  # noqa: E402

from tools.bilagrid_bench import timed  # noqa: E402  (the rounds-of-reps timer)
from tools.tsdf_bench import look_at, sphere_view  # noqa: E402  (the TSDF benchmark's scene)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--reps", type=int, default=5, help="calls between one pair of events")
    ap.add_argument("--rounds", type=int, default=9, help="event pairs per variant")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512, 1024])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sparse_tsdf_bench.json"))
    a = ap.parse_args()

    import torch
    from easygaussiansplatting_amd.function import Camera
    from easygaussiansplatting_amd.mesh import SparseTSDFVolume, TSDFVolume
    if not torch.cuda.is_available():
        raise SystemExit("sparse_tsdf_bench needs a GPU: there is nothing to time without one")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    H, W = a.height, a.width
    f = 1.25 * H
    views = []
    for k in range(6):
        th = 2 * np.pi * k / 6 + 0.2
        Rk, tk = look_at((3.0 * np.cos(th), 0.9 * (-1) ** k, 3.0 * np.sin(th)), roll=0.2 * k)
        cam = Camera(W, H, f, f, W / 2.0 - 0.37, H / 2.0 + 0.21, Rk, tk)
        views.append((cam,) + sphere_view(torch, cam, dev, gen))

    res = {}
    for n in a.sizes:
        geo = ((-1.0, -1.0, -1.0), 2.0 / (n - 1), (n, n, n))
        sp = SparseTSDFVolume(*geo)
        for cam, depth, alpha, image in views:
            sp.integrate(depth, alpha, cam, image=image)
        torch.cuda.synchronize()
        cam, depth, alpha, image = views[0]
        total_blocks = sp.directory.numel()
        pool_bytes = sp.n_blocks * 512 * 4 * 5 + total_blocks * 4 + sp.n_blocks * 4
        info = {"allocated_blocks": sp.n_blocks, "total_blocks": total_blocks,
                "allocated_share": round(sp.n_blocks / total_blocks, 5), "pool_capacity": sp.capacity,
                "sparse_bytes_in_use": pool_bytes, "dense_bytes": n ** 3 * 4 * 5}
        variants = {"sparse/%d/integrate" % n: lambda v=sp: v.integrate(depth, alpha, cam, image=image)}
        ext = {"sparse/%d/extract" % n: sp.extract_triangles}
        dense, why = None, None
        if n ** 3 >= 1 << 31:
            why = "not measured: a dense volume takes fewer than 2^31 samples"
        else:
            free = torch.cuda.mem_get_info()[0]
            if n ** 3 * 4 * 5 * 1.5 > free:
                why = "not measured: %d bytes of dense planes and %d bytes free on the device" % (n ** 3 * 20, free)
        if why is None:
            dense = TSDFVolume(*geo)
            for c, d, al, im in views:
                dense.integrate(d, al, c, image=im)
            variants["dense/%d/integrate" % n] = lambda v=dense: v.integrate(depth, alpha, cam, image=image)
            ext["dense/%d/extract" % n] = dense.extract_triangles
        r = timed(variants, a.warmup, a.rounds, a.reps)
        r.update(timed(ext, 1, a.rounds, 1))
        for k in r:
            r[k].update(info)
        r["sparse/%d/extract" % n]["triangles"] = int(sp.extract_triangles()[0].shape[0])
        if dense is not None:
            r["dense/%d/extract" % n]["triangles"] = int(dense.extract_triangles()[0].shape[0])
            for what in ("integrate", "extract"):
                r["sparse/%d/%s" % (n, what)]["dense_over_sparse"] = round(
                    r["dense/%d/%s" % (n, what)]["median_us"] / r["sparse/%d/%s" % (n, what)]["median_us"], 2)
        else:
            r["dense/%d/integrate" % n] = r["dense/%d/extract" % n] = {"median_us": None, "note": why}
        res.update(r)
        del sp, dense, variants, ext
        torch.cuda.empty_cache()

    out = {"what": "SparseTSDFVolume (libegs_sparsetsdf.so) against TSDFVolume (libegs_tsdf.so) on the sphere of "
                   "tools/tsdf_bench.py, six views with colour: us per call of integrating one more view and of "
                   "extract_triangles, median / min / max over the rounds of HIP-event brackets; allocated against total "
                   "8^3 blocks; bytes of the pools in use against bytes of dense planes",
           "height": H, "width": W, "reps_per_bracket": a.reps, "rounds": a.rounds, "warmup_calls": a.warmup,
           "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "results": res}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print("%-26s %12s %12s %12s %10s %12s" % ("variant", "median us", "min", "max", "blocks", "triangles"))
    for k, r in res.items():
        if r["median_us"] is None:
            print("%-26s %s" % (k, r["note"]))
        else:
            print("%-26s %12.2f %12.2f %12.2f %10s %12s" % (k, r["median_us"], r["min_us"], r["max_us"],
                                                          r.get("allocated_blocks", ""), r.get("triangles", "")))


if __name__ == "__main__":
    main()
