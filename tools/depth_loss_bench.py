#!/usr/bin/env python3
"""The fused depth-prior loss against a torch composition of the same formula.

    python tools/depth_loss_bench.py [--height 1080 --width 1920] [--reps 20] [--rounds 9]
                                     [--out profiles/depth_loss_bench.json]

Variants, per kind ("metric", "affine", "pearson"), on one generated case (tests/depth_loss_ref.make_case: 10 % of the
prior missing), loss and both gradient planes, on preallocated buffers:

    hip/<kind>       egs_depthloss called directly (two launches)
    hip/<kind>+w     the same with a weight plane
    torch/<kind>     the formula of include/egs_depthloss.h in float32 torch operations, written without a host
                     readback (the fit is solved in 0-dim device tensors) -- what a user composes without the library

Timing: every variant is warmed up, then ``rounds`` rounds visit the variants in turn; a visit brackets ``reps``
back-to-back calls with HIP events.  Reported per variant: the median over the rounds of the time per call, its minimum
and maximum; ``spread`` is (max - min) / median.  For the HIP variants also the bytes a call must move (every input plane
read by both passes, both gradient planes written once) over the median time, as a share of the 8 TB/s HBM3E peak; at
1080p a plane is 8.3 MB, so the second pass may find its inputs in the last-level cache and the share is an effective
rate, not a DRAM counter.  This is not ``bench.py``; nothing here is a gate.
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


def torch_composition(torch, D, A, q, kind, alpha_min=0.05):
    """-> (loss, dD, dA): the definition in float32 torch operations, nothing read back to the host"""
    valid = (q > 0) & torch.isfinite(q) & (A > alpha_min) & (D > 0)
    om = valid.to(torch.float32)
    inv_d = torch.where(valid, 1.0 / D, torch.zeros_like(D))
    r = torch.where(valid, A * inv_d, torch.zeros_like(D))
    qv = torch.where(valid, q, torch.zeros_like(q))
    Om = om.sum().clamp_min(1.0)
    if kind == "pearson" or kind == "affine":
        qm, rm = (om * qv).sum() / Om, (om * r).sum() / Om
        vq = (om * qv * qv).sum() / Om - qm * qm
        cov = (om * qv * r).sum() / Om - qm * rm
    if kind == "pearson":
        vr = (om * r * r).sum() / Om - rm * rm
        sq, sr = vq.sqrt(), vr.sqrt()
        rho = cov / (sq * sr)
        loss = 1.0 - rho
        dr = -(om / Om) / (sq * sr) * ((qv - qm) - rho * sq / sr * (r - rm))
    else:
        if kind == "affine":
            s = cov / vq
            t = rm - s * qm
            e = r - (s * qv + t)
        else:
            e = r - qv
        loss = (om * e.abs()).sum() / Om
        dr = om * torch.sign(e) / Om
    return loss, -dr * r * inv_d, dr * inv_d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--reps", type=int, default=20, help="calls between one pair of events")
    ap.add_argument("--rounds", type=int, default=9, help="event pairs per variant")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "depth_loss_bench.json"))
    a = ap.parse_args()

    import torch
    from easygaussiansplatting_amd import _depthlosslib
    from tests import depth_loss_ref as DR
    if not torch.cuda.is_available():
        raise SystemExit("depth_loss_bench needs a GPU: there is nothing to time without one")
    dev = torch.device("cuda:0")
    lib = _depthlosslib.load()
    H, W = a.height, a.width
    D, A, q = (torch.from_numpy(t).to(dev) for t in DR.make_case(H, W))
    w = 2.0 * torch.rand((H, W), device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    st = torch.cuda.current_stream().cuda_stream
    dD, dA = torch.empty_like(D), torch.empty_like(D)
    stats = torch.empty(6, device=dev)
    ws = torch.empty(int(lib.egs_depthloss_ws_bytes(H, W)), dtype=torch.uint8, device=dev)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def hip(kind, weight):
        _depthlosslib.check(lib.egs_depthloss(H, W, p(D), p(A), p(q), p(weight), _depthlosslib.KINDS[kind], 0.05, 1.0,
                                              p(ws), ws.numel(), p(stats), p(dD), p(dA), st))

    variants, moved = {}, {}
    for kind in DR.KINDS:
        variants["hip/" + kind] = lambda kind=kind: hip(kind, None)
        variants["hip/%s+w" % kind] = lambda kind=kind: hip(kind, w)
        variants["torch/" + kind] = lambda kind=kind: torch_composition(torch, D, A, q, kind)
        moved["hip/" + kind] = (2 * 3 + 2) * 4 * H * W
        moved["hip/%s+w" % kind] = (2 * 4 + 2) * 4 * H * W
    # the two agree before anything is timed
    for kind in DR.KINDS:
        hip(kind, None)
        loss, gD, gA = torch_composition(torch, D, A, q, kind)
        assert abs(float(stats[0]) - float(loss)) <= 1e-4 * max(1e-3, abs(float(loss))), (kind, float(stats[0]), float(loss))
        if kind == "pearson":       # (the L1 kinds flip signs where float32 puts e on the other side of zero)
            assert float((gD - dD).abs().max()) <= 1e-3 * float(dD.abs().max())
    res = timed(variants, a.warmup, a.rounds, a.reps)
    for k, r in res.items():
        if k in moved:
            r["bytes_moved"] = moved[k]
            r["share_of_hbm_peak"] = round(moved[k] / (r["median_us"] * 1e-6) / HBM_PEAK, 4)
        else:
            r["over_hip"] = round(r["median_us"] / res["hip/" + k.split("/")[1]]["median_us"], 2)
    out = {"what": "depth-prior loss + both gradient planes: egs_depthloss (libegs_depthloss.so) against a float32 torch "
                   "composition of the same formula without a host readback; us per call, median / min / max over the "
                   "rounds of HIP-event brackets; share_of_hbm_peak = bytes_moved / median / 8 TB/s",
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
