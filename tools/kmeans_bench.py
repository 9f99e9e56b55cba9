#!/usr/bin/env python3
"""k-means for the SH codebook of a compressed scene: N = 1 M rows of D = 45 floats (the SH rest of degree 3)
against K = 4096 and K = 65536 centroids.

    python tools/kmeans_bench.py [--rows 1000000] [--dim 45] [--clusters 4096 65536] [--reps 2] [--rounds 7]
                                 [--out profiles/kmeans_bench.json]

Per K, timed with HIP-event brackets (median / min / max over the rounds):

    assign                 ``egs_kmeans_assign`` (C ABI): the norms pre-kernel and the MFMA assign kernel
    assign/torch           the composition a user writes: ``(c.square().sum(1) - 2 * x @ c.T).argmin(1)`` in row chunks that
                           keep the score block under 1 GiB
    torch/sort             the stable sort of the labels and the ``searchsorted`` (the incidence of the update)
    update                 ``egs_kmeans_update`` (C ABI): the chunk kernel and the combine kernel
    iteration              one whole Lloyd iteration: the three above, as ``compress.kmeans`` runs them

The update writes centroids in place, so ``update`` and ``iteration`` write a scratch table that each call first resets to
the stated centroids (a K x D copy inside the bracket: 12 MB at K = 65536): every variant of every round sees the same input.

``assign`` is reported as a fraction of the FP32 peak (157.3 TFLOP/s) on 2 N K D FLOP -- the useful arithmetic, not the padded
D = 48 the kernel multiplies.  The rows are normal, the centroids rows plus noise, the labels fed to sort and update are the
kernel's own.  Before anything is timed the kernel's labels are compared with the composition's: the count of rows where they
differ is reported (both are float32 orders of the same formula; they differ where two centroids are within rounding).
At K >= 32768, where a call takes tens of milliseconds, a bracket holds one call and the warm-up is one call.
Nothing here is a gate and no ratio is asserted.
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

FP32_PEAK = 157.3e12


def torch_assign(torch, x, c):
    rows = max(1, (1 << 30) // (4 * c.shape[0]))
    n = c.square().sum(1)
    ct = c.T.contiguous()
    out = torch.empty(x.shape[0], dtype=torch.int64, device=x.device)
    for i in range(0, x.shape[0], rows):
        out[i:i + rows] = (n - 2 * (x[i:i + rows] @ ct)).argmin(1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=45)
    ap.add_argument("--clusters", type=int, nargs="+", default=(4096, 65536))
    ap.add_argument("--reps", type=int, default=2, help="calls between one pair of events")
    ap.add_argument("--rounds", type=int, default=7, help="event pairs per variant")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "kmeans_bench.json"))
    a = ap.parse_args()

    import torch
    from easygaussiansplatting_amd import _kmeanslib
    if not torch.cuda.is_available():
        raise SystemExit("kmeans_bench needs a GPU: there is nothing to time without one")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    N, D = a.rows, a.dim
    x = torch.randn((N, D), device=dev, generator=gen)
    lib = _kmeanslib.load()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    per_k = {}
    for K in a.clusters:
        c0 = (x[torch.randperm(N, device=dev, generator=gen)[:K]] + 0.1 * torch.randn((K, D), device=dev, generator=gen)).contiguous()
        c = c0                                   # read only below
        cw = c0.clone()                          # the centroids update and iteration write
        labels = torch.empty(N, dtype=torch.int32, device=dev)
        cnorm = torch.empty(K, dtype=torch.float32, device=dev)
        wsum = torch.empty(K, dtype=torch.float64, device=dev)
        count = torch.empty(K, dtype=torch.int32, device=dev)
        nb = int(lib.egs_kmeans_update_ws_bytes(N, D, K))
        ws = torch.empty(nb // 8, dtype=torch.float64, device=dev)
        edges = torch.arange(K + 1, dtype=torch.int32, device=dev)

        def assign():
            return lib.egs_kmeans_assign(N, D, K, p(x), p(c), p(cnorm), p(labels), None, 0, stream())

        def sort():
            srt, order = torch.sort(labels, stable=True)
            return order, torch.searchsorted(srt, edges).contiguous()

        assert assign() == 0
        order, offsets = sort()

        # the update writes centroids in place: update and iteration write `cw`, reset to c0 by every call (a K x D copy inside
        # its bracket), so every variant is timed on the stated input and `order` / `offsets` stay the labels of `c`
        def update():
            cw.copy_(c0)
            return lib.egs_kmeans_update(N, D, K, p(x), None, p(order), p(offsets), p(cw), p(wsum), p(count), p(ws), nb, 0, stream())

        def iteration():
            cw.copy_(c0)
            assign()
            o, off = sort()
            return lib.egs_kmeans_update(N, D, K, p(x), None, p(o), p(off), p(cw), p(wsum), p(count), p(ws), nb, 0, stream())

        differ = int((torch_assign(torch, x, c) != labels.long()).sum())
        big = K >= 32768
        res = timed({"assign": assign, "assign/torch": lambda: torch_assign(torch, x, c), "torch/sort": sort, "update": update,
                     "iteration": iteration}, 1 if big else a.warmup, a.rounds, 1 if big else a.reps)
        flop = 2.0 * N * K * D
        res["assign"]["flop"] = flop
        res["assign"]["share_of_fp32_peak"] = round(flop / (res["assign"]["median_us"] * 1e-6) / FP32_PEAK, 4)
        res["assign/torch"]["share_of_fp32_peak"] = round(flop / (res["assign/torch"]["median_us"] * 1e-6) / FP32_PEAK, 4)
        res["assign/torch"]["over_assign"] = round(res["assign/torch"]["median_us"] / res["assign"]["median_us"], 2)
        res["torch/sort"]["share_of_iteration"] = round(res["torch/sort"]["median_us"] / res["iteration"]["median_us"], 4)
        per_k[str(K)] = {"reps_per_bracket": 1 if big else a.reps, "warmup_calls": 1 if big else a.warmup,
                         "labels_that_differ_from_the_composition": differ, "largest_cluster": int(count.max()),
                         "empty_clusters": int((count == 0).sum()), "results": res}
        print("K = %d: %d of %d labels differ from the torch composition's" % (K, differ, N))
        print("%-16s %12s %12s %12s %8s %9s" % ("variant", "median us", "min", "max", "spread", "FP32"))
        for k, r in res.items():
            print("%-16s %12.2f %12.2f %12.2f %8.4f %9s" % (k, r["median_us"], r["min_us"], r["max_us"], r["spread"],
                                                            r.get("share_of_fp32_peak", "")))
    outj = {"what": "k-means (libegs_kmeans.so) on N rows of D floats per number of centroids K; us per call, median / min / max "
                    "over the rounds of HIP-event brackets; share_of_fp32_peak = 2 N K D / median / 157.3 TFLOP/s; assign/torch "
                    "is the chunked torch composition on the same device",
            "rows": N, "dim": D, "reps_per_bracket": a.reps, "rounds": a.rounds, "warmup_calls": a.warmup,
            "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "clusters": per_k}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(outj, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
