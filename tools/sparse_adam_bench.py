#!/usr/bin/env python3
"""Dense against visibility-masked Adam on the trainer's six groups: 1 M Gaussians, degree-3 SH.

    python tools/sparse_adam_bench.py [--n 1000000] [--reps 50] [--rounds 9] [--out profiles/sparse_adam.json]

Two forms of the optimizer step, as ``FusedAdam`` issues them:
  plain      one launch over the six groups with their gradient rows (egs_adam_step / egs_sparse_adam_step)
  factored   the default one-rank ``Trainer`` step with one view: one launch over the four small groups, and the SH
             tensors from the factored gradient (egs_adam_sh_factored / egs_sparse_adam_sh_factored)
for visible fractions 1.0, 0.5, 0.25, 0.05 under two mask kinds: i.i.d. random rows, and contiguous runs of 4096 rows (a
stand-in for a spatially sorted model).  The C entry points are called directly with prebuilt arguments, so that the
figure is the kernels' time and not the optimizer's Python; the dense calls are libegs_hip.so's, the kernels every
earlier measurement of this repository ran.

Timing: every variant is warmed up, then ``rounds`` rounds visit the variants in turn (dense and masked alternate inside
one process and one round); a visit brackets ``reps`` back-to-back steps with HIP events.  Reported per variant: the
median over the rounds of the time per step, its minimum and maximum, and the masked step's median over the dense one's.
This is not ``bench.py``; nothing here is a gate.
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

WIDTHS = (3, 3, 45, 1, 3, 4)
FRACTIONS = (1.0, 0.5, 0.25, 0.05)
RUN = 4096


def make_mask(kind, n, fraction, rng):
    if fraction >= 1.0:
        return np.ones(n, dtype=bool)
    if kind == "iid":
        return rng.random(n) < fraction
    runs = -(-n // RUN)
    on = np.zeros(runs, dtype=bool)
    on[rng.permutation(runs)[:max(1, int(round(fraction * runs)))]] = True
    return np.repeat(on, RUN)[:n]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=50, help="steps between one pair of events")
    ap.add_argument("--rounds", type=int, default=9, help="event pairs per variant")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sparse_adam.json"))
    a = ap.parse_args()

    import torch
    from easygaussiansplatting_amd import _adamlib, _lib, dist_views as DV
    from easygaussiansplatting_amd.optim import REFERENCE_LRS
    if not torch.cuda.is_available():
        raise SystemExit("sparse_adam_bench needs a GPU: there is nothing to time without one")
    dev = torch.device("cuda:0")
    lib, alib = _lib.load(), _adamlib.load()
    n = a.n
    gen = torch.Generator(device=dev).manual_seed(0)
    rn = lambda *s: torch.randn(*s, device=dev, generator=gen)
    P = [rn(n, w) for w in WIDTHS]
    G = [rn(n, w) * 1e-3 for w in WIDTHS]
    M = [torch.zeros_like(p) for p in P]
    V = [torch.zeros_like(p) for p in P]
    stride = DV.FactoredShGrad.row_stride(n)
    rows = rn(1, stride) * 1e-3
    rows[:, 3 * n:3 * n + 3] = torch.tensor([[0.0, 0.0, -6.0]], device=dev)
    st = torch.cuda.current_stream().cuda_stream
    b1, b2, eps, step = 0.9, 0.999, 1e-15, 100

    def dense_groups(idx):
        return (_lib.EgsAdamGroup * len(idx))(*[
            _lib.EgsAdamGroup(P[k].data_ptr(), G[k].data_ptr(), M[k].data_ptr(), V[k].data_ptr(), P[k].numel(),
                              REFERENCE_LRS[k], step) for k in idx])

    def sparse_groups(idx):
        return (_adamlib.EgsSparseAdamGroup * len(idx))(*[
            _adamlib.EgsSparseAdamGroup(P[k].data_ptr(), G[k].data_ptr(), M[k].data_ptr(), V[k].data_ptr(), WIDTHS[k],
                                        REFERENCE_LRS[k], step) for k in idx])
    ALL, SMALL = (0, 1, 2, 3, 4, 5), (0, 3, 4, 5)
    d_all, d_small, s_all, s_small = dense_groups(ALL), dense_groups(SMALL), sparse_groups(ALL), sparse_groups(SMALL)
    low = _lib.EgsAdamGroup(P[1].data_ptr(), None, M[1].data_ptr(), V[1].data_ptr(), P[1].numel(), REFERENCE_LRS[1], step)
    high = _lib.EgsAdamGroup(P[2].data_ptr(), None, M[2].data_ptr(), V[2].data_ptr(), P[2].numel(), REFERENCE_LRS[2], step)

    def dense_plain():
        _lib.check(lib.egs_adam_step(6, d_all, b1, b2, eps, st))

    def dense_factored():
        _lib.check(lib.egs_adam_sh_factored(n, 48, 1, P[0].data_ptr(), rows.data_ptr(), stride, 1.0, low, high, b1, b2,
                                            eps, st))
        _lib.check(lib.egs_adam_step(4, d_small, b1, b2, eps, st))

    def sparse_plain(vis):
        return lambda: _adamlib.check(alib.egs_sparse_adam_step(6, s_all, n, vis.data_ptr(), b1, b2, eps, st))

    def sparse_factored(vis):
        def f():
            _adamlib.check(alib.egs_sparse_adam_sh_factored(n, 48, 1, P[0].data_ptr(), rows.data_ptr(), stride, 1.0, low,
                                                            high, vis.data_ptr(), b1, b2, eps, st))
            _adamlib.check(alib.egs_sparse_adam_step(4, s_small, n, vis.data_ptr(), b1, b2, eps, st))
        return f
    rng = np.random.default_rng(0)
    variants = {"dense/plain": dense_plain, "dense/factored": dense_factored}
    masks = {}
    for kind in ("iid", "runs4096"):
        for fr in FRACTIONS:
            m = make_mask(kind, n, fr, rng)
            vis = torch.from_numpy(m).to(dev)
            masks["%s/%.2f" % (kind, fr)] = (vis, float(m.mean()))
            variants["sparse/plain/%s/%.2f" % (kind, fr)] = sparse_plain(vis)
            variants["sparse/factored/%s/%.2f" % (kind, fr)] = sparse_factored(vis)
    for f in variants.values():                   # code objects loaded, clocks up, every shape seen
        for _ in range(a.warmup):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, f in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / a.reps * 1e3)         # us per step
    res = {k: {"median_us": round(float(np.median(v)), 2), "min_us": round(float(np.min(v)), 2),
               "max_us": round(float(np.max(v)), 2)} for k, v in times.items()}
    for k, r in res.items():
        if k.startswith("sparse/"):
            form, mask = k.split("/")[1], k.split("/", 2)[2]
            r["visible_fraction"] = round(masks[mask][1], 4)
            r["over_dense"] = round(r["median_us"] / res["dense/" + form]["median_us"], 3)
    floats = sum(WIDTHS)
    out = {"what": "Adam step over the trainer's six groups, dense (libegs_hip.so) against visibility-masked "
                   "(libegs_adam.so); us per step, median / min / max over the rounds of HIP-event brackets",
           "gaussians": n, "floats_per_gaussian": floats, "dense_bytes_per_step": 28 * floats * n,
           "reps_per_bracket": a.reps, "rounds": a.rounds, "warmup_steps": a.warmup,
           "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "results": res}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("%-36s %10s %10s %10s %8s" % ("variant", "median us", "min", "max", "/dense"))
    for k, r in res.items():
        print("%-36s %10.2f %10.2f %10.2f %8s" % (k, r["median_us"], r["min_us"], r["max_us"], r.get("over_dense", "")))


if __name__ == "__main__":
    main()
