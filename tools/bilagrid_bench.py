#!/usr/bin/env python3
"""The bilateral-grid slice against what users have today, and what it adds to a training step.

    python tools/bilagrid_bench.py [--height 1080 --width 1920] [--shape 16 16 8] [--reps 20] [--rounds 9]
                                   [--gaussians 1000000] [--no-step] [--out profiles/bilagrid_bench.json]

1. The HIP forward + backward pair (egs_bilagrid_slice, then egs_bilagrid_slice_bwd writing dimage and accumulating
   dgrid; the C entry points are called directly with preallocated outputs) against the torch composition: the same
   slice written with ``torch.nn.functional.grid_sample`` in float32 on the same device and the same inputs, forward
   plus ``autograd`` backward to the image and the grid.  Two images: ``smooth`` (low-frequency, as a render is: most
   waves of 64 pixels share one lattice cell) and ``noise`` (i.i.d. colours: every lane its own luminance layer).
   The two forms are first compared on these inputs (outputs and gradients, relative to the largest entry).
2. One ``Trainer.step`` of one view at the bench.py scene (big_scene: 1 M Gaussians, degree-3 SH) with ``bilagrid``
   off -- the step of the parent commit, which this option leaves as it is -- and on.

Timing: every variant is warmed up, then ``rounds`` rounds visit the variants in turn (the forms alternate inside one
process and one round); a visit brackets ``reps`` back-to-back calls with HIP events.  Reported per variant: the median
over the rounds of the time per call, its minimum and maximum; ``spread`` is (max - min) / median.  This is not
``bench.py``; nothing here is a gate.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

LUMA = (0.299, 0.587, 0.114)


def torch_slice(image, grid):
    """the composition gsplat's users run: grid_sample (bilinear, border, align_corners) of the 12 affine entries at
    (x, y, luma), then the per-pixel affine transform"""
    import torch
    import torch.nn.functional as F
    H, W = image.shape[1:]
    ys = torch.arange(H, dtype=image.dtype, device=image.device)
    xs = torch.arange(W, dtype=image.dtype, device=image.device)
    ny = (2 * ys / max(H - 1, 1) - 1)[:, None].expand(H, W)
    nx = (2 * xs / max(W - 1, 1) - 1)[None, :].expand(H, W)
    nz = 2 * (LUMA[0] * image[0] + LUMA[1] * image[1] + LUMA[2] * image[2]) - 1
    A = F.grid_sample(grid[None], torch.stack((nx, ny, nz), -1)[None, None], mode="bilinear", padding_mode="border",
                      align_corners=True)[0, :, 0].reshape(3, 4, H, W)
    return (A[:, :3] * image[None]).sum(1) + A[:, 3]


def make_image(kind, H, W, dev, gen):
    import torch
    if kind == "noise":
        return torch.rand((3, H, W), device=dev, generator=gen) * 1.5 - 0.25
    y = torch.linspace(0, 1, H, device=dev)[:, None]
    x = torch.linspace(0, 1, W, device=dev)[None, :]
    planes = [0.5 + 0.45 * torch.sin(6.0 * x + 2.0 * c) * torch.cos(4.0 * y - c) for c in range(3)]
    return (torch.stack(planes) + 0.01 * torch.randn((3, H, W), device=dev, generator=gen)).contiguous()


def timed(variants, warmup, rounds, reps):
    import torch
    for f in variants.values():                   # code objects loaded, clocks up, every shape seen
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, f in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / reps * 1e3)         # us per call
    res = {}
    for k, v in times.items():
        med = float(np.median(v))
        res[k] = {"median_us": round(med, 2), "min_us": round(float(np.min(v)), 2), "max_us": round(float(np.max(v)), 2),
                  "spread": round((float(np.max(v)) - float(np.min(v))) / med, 4)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--shape", type=int, nargs=3, default=(16, 16, 8), metavar=("GW", "GH", "L"))
    ap.add_argument("--reps", type=int, default=20, help="calls between one pair of events")
    ap.add_argument("--rounds", type=int, default=9, help="event pairs per variant")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--gaussians", type=int, default=1_000_000, help="Gaussians of the Trainer.step leg")
    ap.add_argument("--step-reps", type=int, default=10)
    ap.add_argument("--no-step", action="store_true", help="skip the Trainer.step leg")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bilagrid_bench.json"))
    a = ap.parse_args()

    import torch
    from easygaussiansplatting_amd import _bilagridlib, appearance
    if not torch.cuda.is_available():
        raise SystemExit("bilagrid_bench needs a GPU: there is nothing to time without one")
    dev = torch.device("cuda:0")
    lib = _bilagridlib.load()
    H, W = a.height, a.width
    gw, gh, L = a.shape
    gen = torch.Generator(device=dev).manual_seed(0)
    grid = appearance.identity_grids(1, a.shape, dev)[0] + 0.1 * torch.randn((12, L, gh, gw), device=dev, generator=gen)
    dout = torch.randn((3, H, W), device=dev, generator=gen) / (H * W)
    st = torch.cuda.current_stream().cuda_stream
    check = {}
    variants = {}
    keep = []
    for kind in ("smooth", "noise"):
        image = make_image(kind, H, W, dev, gen)
        out, dimage, dgrid = torch.empty_like(image), torch.empty_like(image), torch.zeros_like(grid)
        keep.append((image, out, dimage, dgrid))
        args = (0, st, H, W, gw, gh, L, image.data_ptr(), grid.data_ptr())

        def hip_fwd(args=args, out=out):
            _bilagridlib.check(lib.egs_bilagrid_slice(*args, out.data_ptr()))

        def hip_bwd(args=args, dimage=dimage, dgrid=dgrid):
            _bilagridlib.check(lib.egs_bilagrid_slice_bwd(*args, dout.data_ptr(), dimage.data_ptr(), dgrid.data_ptr()))

        def hip_pair(f=hip_fwd, b=hip_bwd):
            f()
            b()
        ti, tg = image.clone().requires_grad_(True), grid.clone().requires_grad_(True)

        def torch_pair(ti=ti, tg=tg):
            ti.grad = tg.grad = None
            torch_slice(ti, tg).backward(dout)
        # the two forms on these inputs, relative to the largest entry (float32 against float32)
        hip_pair()
        torch_pair()
        rel = lambda x, y: float((x - y).abs().max() / y.abs().max())
        check[kind] = {"out": rel(out, torch_slice(image, grid)), "dimage": rel(dimage, ti.grad),
                       "dgrid": rel(dgrid, tg.grad)}
        variants["hip/forward/" + kind] = hip_fwd
        variants["hip/backward/" + kind] = hip_bwd
        variants["hip/pair/" + kind] = hip_pair
        variants["torch/pair/" + kind] = torch_pair
    res = timed(variants, a.warmup, a.rounds, a.reps)
    for kind in ("smooth", "noise"):
        h, t = res["hip/pair/" + kind], res["torch/pair/" + kind]
        h["over_torch"] = round(h["median_us"] / t["median_us"], 4)
    box = appearance.largest_box(H, W, a.shape)
    bw, bh = _bilagridlib.BLOCK_W, _bilagridlib.BLOCK_H
    blocks = -(-W // bw) * -(-H // bh)
    out = {"what": "bilateral-grid slice, forward + backward: HIP (libegs_bilagrid.so) against the torch grid_sample "
                   "composition with autograd; us per call, median / min / max over the rounds of HIP-event brackets",
           "height": H, "width": W, "shape": list(a.shape), "path": appearance.slice_path(H, W, a.shape),
           "largest_box_floats": box, "workgroups": blocks,
           "flushed_bytes_upper_bound": 4 * box * blocks, "naive_atomic_bytes": 96 * 4 * H * W,
           "reps_per_bracket": a.reps, "rounds": a.rounds, "warmup_calls": a.warmup,
           "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"),
           "hip_against_torch_max_rel": check, "results": res}

    if not a.no_step:
        from easygaussiansplatting_amd import scene as S
        from easygaussiansplatting_amd.function import Camera, render
        from easygaussiansplatting_amd.trainer import Trainer
        sc = S.big_scene(a.gaussians, W, H, 48)
        cam = Camera.from_scene(sc.cam, dev)
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)
        with torch.no_grad():
            gt = (render(t(sc.pws), t(sc.shs), t(sc.alphas), t(sc.scales), t(sc.rots), cam)[0] * 0.9 + 0.02).contiguous()
        trainers = {"step/off": Trainer(sc, [cam], [gt], max_steps=100000),
                    "step/on": Trainer(sc, [cam], [gt], max_steps=100000, bilagrid=True, bilagrid_shape=tuple(a.shape))}
        steps = {k: (lambda tr=tr: tr.step([0], sync=False)) for k, tr in trainers.items()}
        out["step"] = timed(steps, a.warmup, a.rounds, a.step_reps)
        out["step"]["added_us"] = round(out["step"]["step/on"]["median_us"] - out["step"]["step/off"]["median_us"], 2)
        out["step_gaussians"] = a.gaussians
        out["redone_steps"] = {k: tr.redone_steps for k, tr in trainers.items()}

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("%-28s %10s %10s %10s %8s" % ("variant", "median us", "min", "max", "spread"))
    for k, r in list(res.items()) + [(k, r) for k, r in out.get("step", {}).items() if isinstance(r, dict)]:
        print("%-28s %10.2f %10.2f %10.2f %8.4f %s" % (k, r["median_us"], r["min_us"], r["max_us"], r["spread"],
                                                     r.get("over_torch", "")))
    print("hip against torch, max relative difference:", json.dumps(check))


if __name__ == "__main__":
    main()
