#!/usr/bin/env python3
"""TSDF fusion and mesh extraction against the torch composition a user would write.

    python tools/tsdf_bench.py [--height 1080 --width 1920] [--reps 5] [--rounds 9] [--out profiles/tsdf_bench.json]

INTEGRATE: one view of an analytic sphere (radius 0.7, ray-cast on the device; opacity 0.9 where it is hit, a random
image) into a volume over [-1, 1]^3, from a camera 3 units away with a generic rotation:

    hip/256, hip/256+color, hip/512, hip/512+color    ``TSDFVolume.integrate`` (egs_tsdf_integrate on the frustum's sub-box)
    hip/256/full                                      the same on the full lattice (``clip_to_frustum=False``)
    torch/256, torch/256+color                        the plain composition: ``torch.meshgrid`` points projected, the
                                                      nearest pixel gathered, masked updates with ``torch.where``;
                                                      float32, no host readback

Reported per variant: time per view (median / min / max over the rounds of HIP-event brackets) and, for the HIP variants,
two byte counts over the median time as a share of the 8 TB/s HBM3E peak.  ``bytes_box`` is what a pass that streams the
planes would move: tsdf and weight (and the three colour planes) read and written for every sample of the sub-box, plus the
depth, opacity and image planes.  ``bytes_touched`` is what this kernel asks for: it decides a 16-B quad of samples from the
maps alone and reads and writes the planes only of quads with an updated sample (counted here from the weights a first
view changes), plus the maps.  The gathers from the maps are not streams and a volume of 256^3 fits the last-level cache:
the shares are effective rates, not DRAM counters.

EXTRACT: on a 256^3 volume fused from six views of the sphere, ``extract_triangles`` (count, scan, one readback, emit) and
``extract`` (the same and the welding by ``torch.unique``), timed as whole calls.

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

HBM_PEAK = 8.0e12       # B/s, MI355X HBM3E specification
RADIUS = 0.7


def look_at(eye, roll=0.35):
    eye = np.asarray(eye, np.float64)
    zc = -eye / np.linalg.norm(eye)
    xc = np.cross(np.array([0.13, 1.0, -0.21]), zc)
    xc /= np.linalg.norm(xc)
    yc = np.cross(zc, xc)
    c, s = np.cos(roll), np.sin(roll)
    R = np.stack([c * xc + s * yc, -s * xc + c * yc, zc])
    return R, -R @ eye


def sphere_view(torch, cam, dev, gen):
    """-> depth = alpha z [1,H,W], alpha [1,H,W], image [3,H,W] of the sphere seen by ``cam``"""
    H, W = cam.height, cam.width
    R, t = cam.Rcw.double(), cam.tcw.double()
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64),
                            torch.arange(W, device=dev, dtype=torch.float64), indexing="ij")
    d = torch.stack([(xs - cam.cx) / cam.fx, (ys - cam.cy) / cam.fy, torch.ones_like(xs)], -1) @ R      # R^T d
    eye = -(R.T @ t)
    a, b, c = (d * d).sum(-1), 2.0 * (d @ eye), eye @ eye - RADIUS ** 2
    disc = b * b - 4 * a * c
    z = torch.where(disc > 0, (-b - torch.sqrt(disc.clamp_min(0))) / (2 * a), torch.zeros_like(a))
    alpha = torch.where(z > 0, torch.full_like(z, 0.9), torch.zeros_like(z))
    return ((alpha * z).float()[None].contiguous(), alpha.float()[None].contiguous(),
            torch.rand((3, H, W), device=dev, generator=gen))


def torch_integrate(torch, vol, depth, alpha, image, cam, alpha_min=0.5, near=0.01):
    """the composition a user writes; ``vol``: dict(tsdf, weight, color or None, grid [3,nz,ny,nx], trunc)"""
    R, t = cam.Rcw, cam.tcw
    x, y, z = vol["grid"]
    pc = [R[k, 0] * x + R[k, 1] * y + R[k, 2] * z + t[k] for k in range(3)]
    H, W = depth.shape[-2:]
    ok = pc[2] > near
    zsafe = torch.where(ok, pc[2], torch.ones_like(pc[2]))
    px = torch.floor(cam.fx * pc[0] / zsafe + cam.cx + 0.5)
    py = torch.floor(cam.fy * pc[1] / zsafe + cam.cy + 0.5)
    ok = ok & (px >= 0) & (px < W) & (py >= 0) & (py < H)
    pix = (torch.where(ok, py, torch.zeros_like(py)) * W + torch.where(ok, px, torch.zeros_like(px))).long()
    a = alpha.reshape(-1)[pix]
    ok = ok & (a > alpha_min)
    zs = depth.reshape(-1)[pix] / torch.where(ok, a, torch.ones_like(a))
    sdf = zs - pc[2]
    ok = ok & torch.isfinite(zs) & (zs > 0) & (sdf >= -vol["trunc"])
    tt = torch.clamp(sdf / vol["trunc"], max=1.0)
    w0 = vol["weight"]
    nw = w0 + 1.0
    vol["tsdf"] = torch.where(ok, (w0 * vol["tsdf"] + tt) / nw, vol["tsdf"])
    if vol["color"] is not None:
        img = image.reshape(3, -1)[:, pix]
        vol["color"] = torch.where(ok[None], (w0[None] * vol["color"] + img) / nw[None], vol["color"])
    vol["weight"] = torch.where(ok, nw, w0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--reps", type=int, default=5, help="calls between one pair of events")
    ap.add_argument("--rounds", type=int, default=9, help="event pairs per variant")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tsdf_bench.json"))
    a = ap.parse_args()
    if any(n % 4 or n < 8 for n in a.sizes):
        ap.error("--sizes: multiples of 4 (the touched quads are counted on whole rows)")

    import torch
    from easygaussiansplatting_amd.function import Camera
    from easygaussiansplatting_amd.mesh import TSDFVolume
    if not torch.cuda.is_available():
        raise SystemExit("tsdf_bench needs a GPU: there is nothing to time without one")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    H, W = a.height, a.width
    f = 1.25 * H           # the volume's 2 units at distance 3 fill about five sixths of the image height
    R, t = look_at((1.9, 0.8, -2.2))
    cam = Camera(W, H, f, f, W / 2.0 - 0.37, H / 2.0 + 0.21, R, t)
    depth, alpha, image = sphere_view(torch, cam, dev, gen)

    def volume(n, color):
        return TSDFVolume((-1.0, -1.0, -1.0), 2.0 / (n - 1), (n, n, n), color=color)

    variants, moved, info = {}, {}, {}
    for n in a.sizes:
        for color in (False, True):
            name = "hip/%d%s" % (n, "+color" if color else "")
            vol = volume(n, color)
            vol.integrate(depth, alpha, cam, image=image if color else None)
            torch.cuda.synchronize()
            x0, x1, y0, y1, z0, z1 = vol.last_box
            box = (x1 - x0) * (y1 - y0) * (z1 - z0)
            quads = int((vol.weight.reshape(-1, 4) > 0).any(1).sum())      # (n % 4 == 0: a row is whole quads)
            maps = H * W * (8 + (12 if color else 0))
            per = 16 + (24 if color else 0)
            moved[name] = {"bytes_box": box * per + maps, "bytes_touched": quads * 4 * per + maps}
            info[name] = {"box": list(vol.last_box), "box_samples": box, "updated_samples": int((vol.weight > 0).sum()),
                          "touched_quads": quads}
            variants[name] = lambda v=vol, c=color: v.integrate(depth, alpha, cam, image=image if c else None)
    n0 = a.sizes[0]
    full = volume(n0, False)
    variants["hip/%d/full" % n0] = lambda: full.integrate(depth, alpha, cam, clip_to_frustum=False)
    moved["hip/%d/full" % n0] = {"bytes_box": n0 ** 3 * 16 + H * W * 8,
                                "bytes_touched": moved["hip/%d" % n0]["bytes_touched"]}
    g = -1.0 + (2.0 / (n0 - 1)) * torch.arange(n0, device=dev)
    grid = torch.stack(torch.meshgrid(g, g, g, indexing="ij")[::-1])           # x fastest: [3,nz,ny,nx] of (x, y, z)
    tvols = {}
    for color in (False, True):
        name = "torch/%d%s" % (n0, "+color" if color else "")
        tvols[name] = dict(tsdf=torch.ones((n0,) * 3, device=dev), weight=torch.zeros((n0,) * 3, device=dev),
                           color=torch.zeros((3,) + (n0,) * 3, device=dev) if color else None, grid=grid,
                           trunc=4 * 2.0 / (n0 - 1))
        variants[name] = lambda v=tvols[name]: torch_integrate(torch, v, depth, alpha, image, cam)
    # the two agree before anything is timed: the same samples updated but for threshold cases, tsdf close
    ref = volume(n0, True)
    ref.integrate(depth, alpha, cam, image=image)
    chk = dict(tvols["torch/%d+color" % n0])
    torch_integrate(torch, chk, depth, alpha, image, cam)
    differ = int(((ref.weight > 0) != (chk["weight"] > 0)).sum())
    both = (ref.weight > 0) & (chk["weight"] > 0)
    off = float((ref.tsdf - chk["tsdf"])[both].abs().max())
    print("torch composition against the kernel: %d of %d samples updated on one side only, tsdf within %.2e" % (
        differ, n0 ** 3, off))
    assert differ <= 1e-3 * n0 ** 3 and off <= 1e-3, (differ, off)

    res = timed(variants, a.warmup, a.rounds, a.reps)
    for k, r in res.items():
        if k in moved:
            r.update(moved[k])
            r.update(info.get(k, {}))
            for nm in ("box", "touched"):
                r["share_of_hbm_peak_" + nm] = round(moved[k]["bytes_" + nm] / (r["median_us"] * 1e-6) / HBM_PEAK, 4)
        else:
            r["over_hip"] = round(r["median_us"] / res[k.replace("torch", "hip")]["median_us"], 2)

    # extraction: six views of the sphere fused into n0^3
    vol = volume(n0, True)
    for k in range(6):
        th = 2 * np.pi * k / 6 + 0.2
        Rk, tk = look_at((3.0 * np.cos(th), 0.9 * (-1) ** k, 3.0 * np.sin(th)), roll=0.2 * k)
        ck = Camera(W, H, f, f, W / 2.0 - 0.37, H / 2.0 + 0.21, Rk, tk)
        vol.integrate(*sphere_view(torch, ck, dev, gen)[:2], ck, image=image)
    V, F, _ = vol.extract()
    ext = timed({"extract_triangles/%d" % n0: vol.extract_triangles, "extract/%d" % n0: vol.extract}, 2, a.rounds, 1)
    for r in ext.values():
        r.update({"triangles": int(F.shape[0]), "vertices": int(V.shape[0]),
                  "bytes_planes_read": n0 ** 3 * 8 * 2, "bytes_written": int(F.shape[0]) * (36 + 24 + 36)})
    res.update(ext)
    out = {"what": "TSDF fusion of one view (TSDFVolume.integrate, libegs_tsdf.so) against a float32 torch composition "
                   "(meshgrid projection, nearest-pixel gather, masked updates), and mesh extraction of a fused sphere; us "
                   "per call, median / min / max over the rounds of HIP-event brackets; share_of_hbm_peak_* = bytes_* / "
                   "median / 8 TB/s (effective rates, see the tool's docstring)",
           "height": H, "width": W, "reps_per_bracket": a.reps, "rounds": a.rounds, "warmup_calls": a.warmup,
           "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "results": res}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print("%-24s %10s %10s %10s %8s %9s %9s %9s" % ("variant", "median us", "min", "max", "spread", "HBM box", "HBM tch",
                                                  "over hip"))
    for k, r in res.items():
        print("%-24s %10.2f %10.2f %10.2f %8.4f %9s %9s %9s" % (
            k, r["median_us"], r["min_us"], r["max_us"], r["spread"], r.get("share_of_hbm_peak_box", ""),
            r.get("share_of_hbm_peak_touched", ""), r.get("over_hip", "")))


if __name__ == "__main__":
    main()
