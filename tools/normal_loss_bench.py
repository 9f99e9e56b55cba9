#!/usr/bin/env python3
"""The fused normal loss against a torch composition of the same formula.

    python tools/normal_loss_bench.py [--height 1080 --width 1920] [--reps 20] [--rounds 9]
                                      [--out profiles/normal_loss_bench.json]

Variants on one generated case (tests/normal_loss_ref.make_case, "wavy": 3 % of the pixels below alpha_min, 10 % of the
prior missing), loss and both gradient planes, on preallocated buffers:

    hip/both       egs_normalloss called directly: prior and smoothness term, guide image (three launches)
    hip/both+w     the same with a weight plane
    hip/prior      the prior term alone (two launches)
    hip/smooth     the smoothness term alone, with the guide
    torch/<...>    the formula of include/egs_normalloss.h in float32 torch operations and their autograd, written
                   without a host readback -- what a user composes without the library

Timing: every variant is warmed up, then ``rounds`` rounds visit the variants in turn; a visit brackets ``reps``
back-to-back calls with HIP events.  Reported per variant: the median over the rounds of the time per call, its minimum
and maximum; ``spread`` is (max - min) / median.  For the HIP variants also the bytes the passes of a call move (per pixel:
the tile pass reads D, A, the prior and writes 32 B of workspace; the pair pass reads those 32 B and the guide; the
gradient pass reads the 32 B, D, A, prior and guide and writes both planes; a weight plane is read by each) over the
median time, as a share of the 8 TB/s HBM3E peak.  Halo reads are not counted, and a later pass may find the workspace in
the last-level cache: the share is an effective rate, not a DRAM counter.  This is not ``bench.py``; nothing here is a
gate.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tools.bilagrid_bench import timed  # noqa: E402  (the rounds-of-reps timer)

HBM_PEAK = 8.0e12       # B/s, MI355X HBM3E specification


def torch_composition(torch, D, A, cam, q, I, w, smooth, alpha_min=0.05, gamma=10.0):
    """-> (L_p, L_s, dD, dA): the definition in float32 torch operations and autograd, nothing read back to the host"""
    F = torch.nn.functional
    H, W = D.shape
    D = D.detach().requires_grad_(True)
    A = A.detach().requires_grad_(True)
    fx, fy, cx, cy = cam
    dv = (A > alpha_min) & (D > 0)
    z = torch.where(dv, D / torch.where(dv, A, torch.ones_like(A)), torch.ones_like(D))
    xs = torch.arange(W, device=D.device, dtype=D.dtype)[None, :]
    ys = torch.arange(H, device=D.device, dtype=D.dtype)[:, None]
    p = torch.stack([z * ((xs - cx) / fx), z * ((ys - cy) / fy), z])
    c = torch.cross(p[:, 2:, 1:-1] - p[:, :-2, 1:-1], p[:, 1:-1, 2:] - p[:, 1:-1, :-2], dim=0)
    c2 = (c * c).sum(0)
    nv = dv[1:-1, 1:-1] & dv[1:-1, 2:] & dv[1:-1, :-2] & dv[2:, 1:-1] & dv[:-2, 1:-1] & (c2 > 0) & torch.isfinite(c2)
    n = F.pad(torch.where(nv, c / torch.sqrt(torch.where(nv, c2, torch.ones_like(c2))), torch.zeros_like(c)),
              (1, 1, 1, 1))
    om = F.pad(nv, (1, 1, 1, 1)).to(D.dtype)
    if w is not None:
        om = om * w
    zero = torch.zeros((), device=D.device)
    Lp = Ls = zero
    if q is not None:
        q2 = (q * q).sum(0)
        data = torch.isfinite(q).all(0) & (q2 > 0)
        qh = torch.where(data, q / torch.sqrt(torch.where(data, q2, torch.ones_like(q2))), torch.zeros_like(q))
        omp = torch.where(data, om, torch.zeros_like(om))
        Lp = (omp * (1 - (n * qh).sum(0))).sum() / omp.sum().clamp_min(1e-30)
    if smooth:
        num = den = zero
        for a, b in (((slice(None), slice(0, -1)), (slice(None), slice(1, None))),
                     ((slice(0, -1), slice(None)), (slice(1, None), slice(None)))):
            oo = om[a] * om[b]
            g = torch.exp(-gamma * (I[(slice(None),) + a] - I[(slice(None),) + b]).abs().mean(0)) if I is not None else 1.0
            num = num + (oo * g * (1 - (n[(slice(None),) + a] * n[(slice(None),) + b]).sum(0))).sum()
            den = den + oo.sum()
        Ls = num / den.clamp_min(1e-30)
    dD, dA = torch.autograd.grad(Lp + Ls, [D, A])
    return Lp.detach(), Ls.detach(), torch.where(dv, dD, torch.zeros_like(dD)), torch.where(dv, dA, torch.zeros_like(dA))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--reps", type=int, default=20, help="calls between one pair of events")
    ap.add_argument("--rounds", type=int, default=9, help="event pairs per variant")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "normal_loss_bench.json"))
    a = ap.parse_args()

    import torch
    from easygaussiansplatting_amd import _normallosslib
    from tests import normal_loss_ref as NR
    if not torch.cuda.is_available():
        raise SystemExit("normal_loss_bench needs a GPU: there is nothing to time without one")
    dev = torch.device("cuda:0")
    lib = _normallosslib.load()
    H, W = a.height, a.width
    case, cam = NR.make_case(H, W, "wavy")
    D, A, q, I, w = (torch.from_numpy(case[k]).to(dev) for k in ("D", "A", "q", "I", "w"))
    st = torch.cuda.current_stream().cuda_stream
    dD, dA = torch.empty_like(D), torch.empty_like(D)
    stats = torch.empty(6, device=dev)
    ws = torch.empty(int(lib.egs_normalloss_ws_bytes(H, W)), dtype=torch.uint8, device=dev)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def hip(prior, smooth, weight):
        _normallosslib.check(lib.egs_normalloss(H, W, p(D), p(A), *[float(v) for v in cam], p(q) if prior else None,
                                                p(I) if smooth else None, p(weight), 1 if smooth else 0, 0.05, 10.0, 1.0,
                                                1.0, p(ws), ws.numel(), p(stats), None, p(dD), p(dA), st))

    px = H * W
    cfg = {"both": (True, True, None), "both+w": (True, True, w), "prior": (True, False, None),
           "smooth": (False, True, None)}
    variants, moved = {}, {}
    for name, (prior, smooth, weight) in cfg.items():
        variants["hip/" + name] = lambda c=(prior, smooth, weight): hip(*c)
        variants["torch/" + name] = lambda c=(prior, smooth, weight): torch_composition(
            torch, D, A, cam, q if c[0] else None, I if c[1] else None, c[2], c[1])
        per_px = (8 + 32) + (32 + 8 + 8) + (12 + 12 if prior else 0) + ((32 + 12) + 12 if smooth else 0)
        per_px += 0 if weight is None else 4 * (3 if smooth else 2)
        moved["hip/" + name] = per_px * px
    # the two agree before anything is timed
    for name, (prior, smooth, weight) in cfg.items():
        hip(prior, smooth, weight)
        Lp, Ls, gD, gA = torch_composition(torch, D, A, cam, q if prior else None, I if smooth else None, weight, smooth)
        got = stats.tolist()
        assert abs(got[0] - float(Lp)) <= 1e-4 and abs(got[1] - float(Ls)) <= 1e-4, (name, got, float(Lp), float(Ls))
        # (float32 loses digits in the differences of neighbouring points, DESIGN §3.18: a loose sanity bound)
        off = float((gD - dD).abs().max()) / float(dD.abs().max())
        print("%-8s torch float32 against the kernel: L_p %.2e L_s %.2e, dD %.2e of its largest entry" % (
            name, abs(got[0] - float(Lp)), abs(got[1] - float(Ls)), off))
        assert off <= 2e-2, (name, off)
    res = timed(variants, a.warmup, a.rounds, a.reps)
    for k, r in res.items():
        if k in moved:
            r["bytes_moved"] = moved[k]
            r["share_of_hbm_peak"] = round(moved[k] / (r["median_us"] * 1e-6) / HBM_PEAK, 4)
        else:
            r["over_hip"] = round(r["median_us"] / res["hip/" + k.split("/")[1]]["median_us"], 2)
    out = {"what": "normal loss + both gradient planes: egs_normalloss (libegs_normalloss.so) against a float32 torch "
                   "composition of the same formula (forward and autograd) without a host readback; us per call, median "
                   "/ min / max over the rounds of HIP-event brackets; share_of_hbm_peak = bytes_moved / median / 8 TB/s",
           "height": H, "width": W, "reps_per_bracket": a.reps, "rounds": a.rounds, "warmup_calls": a.warmup,
           "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "results": res}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("%-18s %10s %10s %10s %8s %10s %9s" % ("variant", "median us", "min", "max", "spread", "HBM share", "over hip"))
    for k, r in res.items():
        print("%-18s %10.2f %10.2f %10.2f %8.4f %10s %9s" % (k, r["median_us"], r["min_us"], r["max_us"], r["spread"],
                                                           r.get("share_of_hbm_peak", ""), r.get("over_hip", "")))


if __name__ == "__main__":
    main()
