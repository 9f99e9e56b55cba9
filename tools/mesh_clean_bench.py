#!/usr/bin/env python3
"""Mesh cleaning on the mesh of the TSDF benchmark: the 256^3 volume fused from six views of a sphere
(tools/tsdf_bench.py), about 0.9 M triangles.

    python tools/mesh_clean_bench.py [--size 256] [--reps 5] [--rounds 9] [--out profiles/mesh_clean_bench.json]

Timed as whole calls of the Python layer, with HIP-event brackets (median / min / max over the rounds):

    components            ``mesh.connected_components(check=False)``: init, hook, flatten, count
    removal               ``mesh.remove_small_components(min_faces=100, check=False)``: the components, the flags, two
                          ``torch.cumsum``, ONE readback (the kept counts), the scatter
    normals               ``mesh.vertex_normals(check=False)``: the incidence (a stable ``torch.sort`` of 3F keys and a
                          ``searchsorted``) and the gather kernel
    normals/kernel        the gather kernel alone on a prebuilt incidence (the C ABI)
    taubin10              ``mesh.smooth_taubin(iterations=10, check=False)``: the incidence and 20 step kernels
    taubin10/kernels      the 20 step kernels alone

and two baselines for the components:

    torch/components      min-label propagation over the edge list with ``scatter_reduce(amin)`` and one pointer jump per
                          round, to a fixed point, with the readback per round that needs (event brackets)
    scipy/components      ``scipy.sparse.csgraph.connected_components`` on the host including the copy of the faces off the
                          device and of the labels back (host clock around a device synchronise); only where scipy imports

For the gather kernels the bytes the algorithm asks for -- per row entry the entry (8 B), the face (24 B) and the vertices
it reads (36 B for a normal, 24 B for a smoothing step), per vertex its row bounds (16 B), its position (smoothing, 12 B)
and its output (12 B) -- over the median time, as a share of the 8 TB/s HBM3E peak.  The mesh fits the last-level cache:
the shares are effective rates, not DRAM counters.  Nothing here is a gate and no ratio is asserted.
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

import numpy as np  # noqa: E402

from tools.bilagrid_bench import timed  # noqa: E402  (the rounds-of-reps timer)
from tools.tsdf_bench import HBM_PEAK, look_at, sphere_view  # noqa: E402


def torch_components(torch, faces, n_vertices):
    """the composition a user writes -> (labels int64 [V], rounds)"""
    a, b, c = faces[:, 0], faces[:, 1], faces[:, 2]
    src, dst = torch.cat([a, b, a, c]), torch.cat([b, a, c, a])
    label = torch.arange(n_vertices, device=faces.device)
    rounds = 0
    while True:
        new = label.scatter_reduce(0, dst, label[src], "amin", include_self=True)
        new = new[new]
        rounds += 1
        if torch.equal(new, label):          # the readback of a round
            return label, rounds
        label = new


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256, help="samples per side of the volume")
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--reps", type=int, default=5, help="calls between one pair of events")
    ap.add_argument("--rounds", type=int, default=9, help="event pairs per variant")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mesh_clean_bench.json"))
    a = ap.parse_args()

    import torch
    from easygaussiansplatting_amd import _meshopslib
    from easygaussiansplatting_amd import mesh as M
    from easygaussiansplatting_amd.function import Camera
    if not torch.cuda.is_available():
        raise SystemExit("mesh_clean_bench needs a GPU: there is nothing to time without one")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    H, W, n = a.height, a.width, a.size
    f = 1.25 * H
    vol = M.TSDFVolume((-1.0, -1.0, -1.0), 2.0 / (n - 1), (n, n, n), color=True)
    image = torch.rand((3, H, W), device=dev, generator=gen)
    for k in range(6):
        th = 2 * np.pi * k / 6 + 0.2
        Rk, tk = look_at((3.0 * np.cos(th), 0.9 * (-1) ** k, 3.0 * np.sin(th)), roll=0.2 * k)
        ck = Camera(W, H, f, f, W / 2.0 - 0.37, H / 2.0 + 0.21, Rk, tk)
        vol.integrate(*sphere_view(torch, ck, dev, gen)[:2], ck, image=image)
    V, F, Cc = vol.extract()
    nv, nf = int(V.shape[0]), int(F.shape[0])
    comp = M.connected_components(F, nv)
    sizes = comp.comp_faces[comp.comp_faces > 0].sort(descending=True).values
    print("mesh: %d vertices, %d faces, %d components (largest %s)" % (nv, nf, sizes.numel(), sizes[:4].tolist()))

    lib = _meshopslib.load()
    row_start, rows = M._incidence(F, nv)
    out, tmp = torch.empty_like(V), torch.empty_like(V)
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    variants = {
        "components": lambda: M.connected_components(F, nv, check=False),
        "removal": lambda: M.remove_small_components(V, F, Cc, min_faces=100, check=False),
        "normals": lambda: M.vertex_normals(V, F, check=False),
        "normals/kernel": lambda: lib.egs_meshops_vertex_normals(nv, nf, p(V), p(F), p(row_start), p(rows), p(out), 0, stream()),
        "taubin10": lambda: M.smooth_taubin(V, F, 10, check=False),
        "taubin10/kernels": lambda: lib.egs_meshops_taubin(nv, nf, p(V), p(F), p(row_start), p(rows), 10, 0.5, -0.53, p(out),
                                                          p(tmp), 0, stream()),
    }
    res = timed(variants, a.warmup, a.rounds, a.reps)
    entries = 3 * nf
    moved = {"normals/kernel": entries * (8 + 24 + 36) + nv * (16 + 12),
             "taubin10/kernels": 20 * (entries * (8 + 24 + 24) + nv * (16 + 12 + 12))}
    for k, b in moved.items():
        res[k]["bytes_asked"] = b
        res[k]["bytes_per_s"] = round(b / (res[k]["median_us"] * 1e-6), 1)
        res[k]["share_of_hbm_peak"] = round(b / (res[k]["median_us"] * 1e-6) / HBM_PEAK, 4)

    # the baselines agree with the kernel before anything is timed
    tl, t_rounds = torch_components(torch, F, nv)
    assert torch.equal(tl.int(), comp.label), "the torch composition gives other labels"
    base = timed({"torch/components": lambda: torch_components(torch, F, nv)}, 1, a.rounds, 1)
    base["torch/components"]["rounds_to_fixed_point"] = t_rounds
    try:
        import scipy.sparse as sp
        from scipy.sparse.csgraph import connected_components as sp_cc
    except ImportError:
        sp = None
        print("scipy is not importable here: the host baseline is skipped")
    if sp is not None:
        def host():
            fh = F.cpu().numpy()
            e = np.concatenate([fh[:, [0, 1]], fh[:, [0, 2]]])
            g = sp.coo_matrix((np.ones(len(e), np.int8), (e[:, 0], e[:, 1])), shape=(nv, nv))
            _, lab = sp_cc(g, directed=False)
            return torch.from_numpy(lab).to(dev)
        lab = host().cpu().numpy()
        first = np.full(int(lab.max()) + 1, nv, np.int64)
        np.minimum.at(first, lab, np.arange(nv))
        assert np.array_equal(first[lab], comp.label.cpu().numpy()), "scipy gives other components"
        ts = []
        for _ in range(a.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e6)
        med = float(np.median(ts))
        base["scipy/components"] = {"median_us": round(med, 2), "min_us": round(min(ts), 2), "max_us": round(max(ts), 2),
                                    "spread": round((max(ts) - min(ts)) / med, 4)}
    for r in base.values():
        r["over_hip"] = round(r["median_us"] / res["components"]["median_us"], 2)
    res.update(base)
    outj = {"what": "mesh cleaning (libegs_meshops.so) on the mesh of the TSDF benchmark's volume; us per call, median / min / "
                    "max over the rounds of HIP-event brackets (scipy: host clock); share_of_hbm_peak = bytes_asked / median "
                    "/ 8 TB/s (an effective rate, see the tool's docstring); over_hip = a baseline's median over "
                    "'components'",
            "size": n, "vertices": nv, "faces": nf, "components": int(sizes.numel()), "largest_components": sizes[:8].tolist(),
            "reps_per_bracket": a.reps, "rounds": a.rounds, "warmup_calls": a.warmup,
            "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "results": res}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(outj, fh, indent=1)
        fh.write("\n")
    print("%-20s %12s %12s %12s %8s %9s %9s" % ("variant", "median us", "min", "max", "spread", "HBM", "over hip"))
    for k, r in res.items():
        print("%-20s %12.2f %12.2f %12.2f %8.4f %9s %9s" % (k, r["median_us"], r["min_us"], r["max_us"], r["spread"],
                                                            r.get("share_of_hbm_peak", ""), r.get("over_hip", "")))


if __name__ == "__main__":
    main()
