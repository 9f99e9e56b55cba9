#!/usr/bin/env python3
"""The weighted fused loss against the unweighted one and against what users had before it.

    python tools/weighted_loss_bench.py [--height 1080 --width 1920] [--reps 20] [--rounds 9]
                                        [--parent-lib PATH/libegs_hip.so] [--out profiles/weighted_loss_bench.json]
                                        [--append]

``--append`` adds this process's run to the ``runs`` the output file already holds: a comparison against the parent
commit's library takes several processes, and the spread of ``gau_loss/parent`` between them is its noise floor.

Variants, all on one image pair (noise, as tests/loss_cases.py makes it) with the C entry points called directly on
preallocated buffers, loss and gradient (lambda 0.2):

    wloss/random      egs_wloss, weights i.i.d. U[0, 3)
    wloss/half        egs_wloss, the left half of the plane weighted 1, the right half 0
    gau_loss          egs_gau_loss of this commit's libegs_hip.so
    gau_loss/parent   egs_gau_loss of the library ``--parent-lib`` names (the parent commit's, built in a scratch
                      checkout): what the loss cost before this option existed.  Left out without the argument.
    torch_workaround  what a user did without the option: both images multiplied by the mask (two torch passes), the
                      unweighted kernels, the gradient multiplied by the mask (a third pass) -- which is also a
                      DIFFERENT loss (an edge at the mask border that SSIM scores, the full pixel count as divisor)

Timing: every variant is warmed up, then ``rounds`` rounds visit the variants in turn; a visit brackets ``reps``
back-to-back calls with HIP events.  Reported per variant: the median over the rounds of the time per call, its minimum
and maximum; ``spread`` is (max - min) / median.  This is not ``bench.py``; nothing here is a gate.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tools.bilagrid_bench import timed  # noqa: E402  (the rounds-of-reps timer)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--reps", type=int, default=20, help="calls between one pair of events")
    ap.add_argument("--rounds", type=int, default=9, help="event pairs per variant")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="libegs_hip.so of the parent commit")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "weighted_loss_bench.json"))
    ap.add_argument("--append", action="store_true", help="add this process's run to the runs --out already holds")
    a = ap.parse_args()

    import torch
    from easygaussiansplatting_amd import _lib, _wlosslib
    from tests import loss_cases as LC
    if not torch.cuda.is_available():
        raise SystemExit("weighted_loss_bench needs a GPU: there is nothing to time without one")
    dev = torch.device("cuda:0")
    lib, wlib = _lib.load(), _wlosslib.load()
    H, W = a.height, a.width
    x, y = (torch.from_numpy(t).to(dev) for t in LC.make_pair("noise", H, W))
    gen = torch.Generator(device=dev).manual_seed(0)
    weights = {"random": 3.0 * torch.rand((H, W), device=dev, generator=gen), "half": torch.zeros((H, W), device=dev)}
    weights["half"][:, :W // 2] = 1.0
    st = torch.cuda.current_stream().cuda_stream
    grad = torch.empty_like(x)
    stats = torch.empty(4, device=dev)
    wws = torch.empty(int(wlib.egs_wloss_ws_bytes(H, W)), dtype=torch.uint8, device=dev)
    ws = torch.empty(int(lib.egs_gau_loss_ws_bytes(H, W)), dtype=torch.uint8, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())

    def wloss(w):
        _wlosslib.check(wlib.egs_wloss(H, W, p(x), p(y), p(w), 0.2, 1.0, p(wws), wws.numel(), p(stats), p(grad), st))

    def gau_loss_of(lib_, xi=x, yi=y):
        rc = lib_.egs_gau_loss(H, W, p(xi), p(yi), 0.2, 1.0, p(ws), ws.numel(), p(stats), p(grad), st)
        if rc != 0:
            raise RuntimeError("egs_gau_loss returned %d" % rc)

    def workaround(m=weights["half"]):
        gau_loss_of(lib, x * m, y * m)
        grad.mul_(m)

    variants = {"wloss/random": lambda: wloss(weights["random"]), "wloss/half": lambda: wloss(weights["half"]),
                "gau_loss": lambda: gau_loss_of(lib)}
    if a.parent_lib:
        parent = C.CDLL(os.path.abspath(a.parent_lib))
        for name in ("egs_gau_loss", "egs_gau_loss_ws_bytes"):
            getattr(parent, name).restype, getattr(parent, name).argtypes = _lib.SIGNATURES[name]
        assert int(parent.egs_gau_loss_ws_bytes(H, W)) == ws.numel()
        variants["gau_loss/parent"] = lambda: gau_loss_of(parent)
    variants["torch_workaround"] = workaround
    res = timed(variants, a.warmup, a.rounds, a.reps)
    base = res["gau_loss"]["median_us"]
    for k, r in res.items():
        r["over_gau_loss"] = round(r["median_us"] / base, 4)
    run = {"height": H, "width": W, "reps_per_bracket": a.reps, "rounds": a.rounds, "warmup_calls": a.warmup,
           "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"),
           "parent_lib": bool(a.parent_lib), "results": res}
    out = {"what": "fused L1/SSIM loss + gradient, lambda 0.2: egs_wloss (libegs_wloss.so) against egs_gau_loss "
                   "(libegs_hip.so, this commit's and the parent's) and the torch mask workaround; us per call, median / "
                   "min / max over the rounds of HIP-event brackets; one entry of `runs` per process",
           "runs": [run]}
    if a.append and os.path.exists(a.out):
        with open(a.out) as f:
            out["runs"] = json.load(f)["runs"] + [run]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("%-20s %10s %10s %10s %8s %14s" % ("variant", "median us", "min", "max", "spread", "over gau_loss"))
    for k, r in res.items():
        print("%-20s %10.2f %10.2f %10.2f %8.4f %14.4f" % (k, r["median_us"], r["min_us"], r["max_us"], r["spread"],
                                                          r["over_gau_loss"]))


if __name__ == "__main__":
    main()
