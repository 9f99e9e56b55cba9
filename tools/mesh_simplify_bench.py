#!/usr/bin/env python3
"""Vertex-clustering simplification on the mesh of the TSDF benchmark: the 256^3 volume fused from six views
of a sphere (tools/tsdf_bench.py), about 0.9 M triangles, at cells of 1, 2 and 4 voxels on the volume's grid.

    python tools/mesh_simplify_bench.py [--size 256] [--cells 1 2 4] [--reps 5] [--rounds 9]
                                        [--out profiles/mesh_simplify_bench.json]

Per cell size, timed with HIP-event brackets (median / min / max over the rounds):

    whole/quadric, whole/mean   ``mesh.simplify_vertex_clustering(check=False)``: everything below plus its three readbacks
    keys                        the key kernel (C ABI)
    torch/unique                ``torch.unique(keys, return_inverse=True)`` (a readback inside)
    torch/members               the stable sort of the cluster ids and the ``searchsorted`` (the member CSR)
    torch/incidence             the stable sort of the 3F corners and the ``searchsorted`` (quadric placement only)
    torch/face-sort             the two stable sorts of the 2 x int64 face keys
    quadrics/kernel             the vertex-parallel pass: 9 doubles per vertex (two-pass form)
    clusters/two-pass           the cluster kernel reading those partials
    clusters/fused              the cluster kernel forming each member's quadric itself (no partials)
    clusters/mean               the cluster kernel with placement "mean"
    faces/remap, faces/flags    the two face kernels (flags: a clear and the first-of-run pass)
    compact                     ``egs_meshops_compact`` behind two ``torch.cumsum`` (the scans are timed with it)

and the baseline a user would write for the mean placement in torch (``unique`` + ``index_add_`` + ``unique(dim=0)``), whose
face count is checked against the library's before anything is timed; the host route through Open3D
(``simplify_vertex_clustering`` with Quadric contraction, copies included) is timed only where ``open3d`` imports.

For the two gather kernels the bytes the algorithm asks for -- quadrics/kernel: per row entry the entry (8 B), the face
(24 B) and its three vertices (36 B), per vertex its row bounds (16 B), its key (8 B) and its 9 doubles (72 B);
clusters/two-pass: per member its index (8 B), key (8 B), position (12 B), colour (12 B) and partial (72 B), per cluster
its bounds (16 B) and its outputs (28 B) -- over the median time, as a share of the 8 TB/s HBM3E peak.  The mesh fits the
last-level cache: the shares are effective rates, not DRAM counters.  Nothing here is a gate and no ratio is asserted.
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


def torch_mean(torch, V, F, Cc, origin, cell):
    """the composition a user writes for the mean placement -> (vertices, faces, colours)"""
    o = torch.tensor(origin, dtype=torch.float64, device=V.device)
    idx = torch.floor((V.double() - o) / cell).long()
    key = idx[:, 0] | (idx[:, 1] << 21) | (idx[:, 2] << 42)
    uniq, inv = torch.unique(key, return_inverse=True)
    n = uniq.shape[0]
    cnt = torch.zeros(n, dtype=torch.float64, device=V.device).index_add_(0, inv, torch.ones_like(inv, dtype=torch.float64))
    pos = torch.zeros((n, 3), dtype=torch.float64, device=V.device).index_add_(0, inv, V.double()) / cnt[:, None]
    col = torch.zeros((n, 3), dtype=torch.float64, device=V.device).index_add_(0, inv, Cc.double()) / cnt[:, None]
    f = inv[F]
    f = f[(f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])]
    k = torch.argmin(f, 1, keepdim=True)
    f = torch.gather(f, 1, (k + torch.arange(3, device=V.device)) % 3)
    f = torch.unique(f, dim=0)
    used, f = torch.unique(f, return_inverse=True)
    return pos[used].float(), f, col[used].float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256, help="samples per side of the volume")
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--cells", type=float, nargs="+", default=(1.0, 2.0, 4.0), help="cell sizes in voxels")
    ap.add_argument("--reps", type=int, default=5, help="calls between one pair of events")
    ap.add_argument("--rounds", type=int, default=9, help="event pairs per variant")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mesh_simplify_bench.json"))
    a = ap.parse_args()

    import torch
    from easygaussiansplatting_amd import _meshopslib, _simplifylib
    from easygaussiansplatting_amd import mesh as M
    from easygaussiansplatting_amd.function import Camera
    if not torch.cuda.is_available():
        raise SystemExit("mesh_simplify_bench needs a GPU: there is nothing to time without one")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    H, W, n = a.height, a.width, a.size
    f = 1.25 * H
    voxel = 2.0 / (n - 1)
    vol = M.TSDFVolume((-1.0, -1.0, -1.0), voxel, (n, n, n), color=True)
    image = torch.rand((3, H, W), device=dev, generator=gen)
    for k in range(6):
        th = 2 * np.pi * k / 6 + 0.2
        Rk, tk = look_at((3.0 * np.cos(th), 0.9 * (-1) ** k, 3.0 * np.sin(th)), roll=0.2 * k)
        ck = Camera(W, H, f, f, W / 2.0 - 0.37, H / 2.0 + 0.21, Rk, tk)
        vol.integrate(*sphere_view(torch, ck, dev, gen)[:2], ck, image=image)
    V, F, Cc = vol.extract()
    nv, nf = int(V.shape[0]), int(F.shape[0])
    row_start, rows = M._incidence(F, nv)
    valence = int((row_start[1:] - row_start[:-1]).max())
    print("mesh: %d vertices, %d faces, largest valence %d" % (nv, nf, valence))
    try:
        import open3d as o3d
    except ImportError:
        o3d = None
        print("open3d is not importable here: the host baseline is skipped")

    lib, mo = _simplifylib.load(), _meshopslib.load()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    origin = vol.origin
    i64 = lambda *s: torch.empty(s, dtype=torch.int64, device=dev)
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)
    f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
    cells = {}
    for kv in a.cells:
        cell = kv * voxel
        keys = i64(nv)
        M._simplifylib.check(lib.egs_simplify_keys(nv, p(V), *origin, cell, p(keys), 0, stream()))
        uniq, cluster = torch.unique(keys, return_inverse=True)
        cluster = cluster.contiguous()
        Vc = int(uniq.shape[0])
        srt, members = torch.sort(cluster, stable=True)
        member_start = torch.searchsorted(srt, torch.arange(Vc + 1, dtype=torch.int64, device=dev)).contiguous()
        counts = member_start[1:] - member_start[:-1]
        quad = torch.empty((nv, 9), dtype=torch.float64, device=dev)
        pos, col, placed = f32(Vc, 3), f32(Vc, 3), i32(Vc)
        rot, valid, hi, lo = i64(nf, 3), i32(nf), i64(nf), i64(nf)
        fkeep, ckeep = i32(nf), i32(Vc)

        def face_sort():
            o = torch.sort(lo, stable=True).indices
            return o[torch.sort(hi[o], stable=True).indices].contiguous()

        def clusters(q, place, fused=False):
            return lib.egs_simplify_clusters(nv, nf, Vc, p(V), p(Cc), p(keys), p(member_start), p(members), p(q),
                                             p(F) if fused else None, p(row_start) if fused else None,
                                             p(rows) if fused else None, *origin, cell, place, p(pos), p(col), p(placed), 0,
                                             stream())

        # everything once, in order, so that every stage below times real inputs; the two forms agree to the bit
        assert lib.egs_simplify_vertex_quadrics(nv, nf, p(V), p(F), p(row_start), p(rows), p(keys), *origin, cell, p(quad), 0,
                                                stream()) == 0
        assert clusters(None, 0, fused=True) == 0
        fused_pos = pos.clone()
        assert clusters(quad, 0) == 0
        assert torch.equal(fused_pos.view(torch.int32), pos.view(torch.int32)), "the fused form gives other bits"
        assert lib.egs_simplify_remap_faces(nv, nf, Vc, p(F), p(cluster), p(rot), p(valid), p(hi), p(lo), 0, stream()) == 0
        order = face_sort()
        assert lib.egs_simplify_keep_flags(nf, Vc, p(order), p(rot), p(valid), p(hi), p(lo), p(fkeep), p(ckeep), 0,
                                           stream()) == 0
        Vk, Fk = int(ckeep.sum()), int(fkeep.sum())
        ov, oc, of = f32(Vk, 3), f32(Vk, 3), i64(Fk, 3)

        def compact():
            vs, fs = torch.cumsum(ckeep, 0, dtype=torch.int64), torch.cumsum(fkeep, 0, dtype=torch.int64)
            return mo.egs_meshops_compact(Vc, nf, p(pos), p(col), None, p(rot), p(ckeep), p(fkeep), p(vs), p(fs), Vk, Fk, p(ov),
                                          p(oc), None, p(of), 0, stream())

        got = M.simplify_vertex_clustering(V, F, Cc, cell_size=cell, origin=origin, placement="mean", check=False,
                                           return_info=True)
        base = torch_mean(torch, V, F, Cc, origin, cell)
        assert base[1].shape[0] == got[1].shape[0] == Fk, "the torch composition keeps another number of faces"
        assert base[0].shape[0] == got[0].shape[0] == Vk, "the torch composition keeps another number of vertices"
        variants = {
            "whole/quadric": lambda: M.simplify_vertex_clustering(V, F, Cc, cell_size=cell, origin=origin, check=False),
            "whole/mean": lambda: M.simplify_vertex_clustering(V, F, Cc, cell_size=cell, origin=origin, placement="mean",
                                                               check=False),
            "keys": lambda: lib.egs_simplify_keys(nv, p(V), *origin, cell, p(keys), 0, stream()),
            "torch/unique": lambda: torch.unique(keys, return_inverse=True),
            "torch/members": lambda: torch.searchsorted(torch.sort(cluster, stable=True).values,
                                                        torch.arange(Vc + 1, dtype=torch.int64, device=dev)),
            "torch/incidence": lambda: M._incidence(F, nv),
            "torch/face-sort": face_sort,
            "quadrics/kernel": lambda: lib.egs_simplify_vertex_quadrics(nv, nf, p(V), p(F), p(row_start), p(rows), p(keys),
                                                                        *origin, cell, p(quad), 0, stream()),
            "clusters/two-pass": lambda: clusters(quad, 0),
            "clusters/fused": lambda: clusters(None, 0, fused=True),
            "clusters/mean": lambda: clusters(None, 1),
            "faces/remap": lambda: lib.egs_simplify_remap_faces(nv, nf, Vc, p(F), p(cluster), p(rot), p(valid), p(hi), p(lo),
                                                                0, stream()),
            "faces/flags": lambda: lib.egs_simplify_keep_flags(nf, Vc, p(order), p(rot), p(valid), p(hi), p(lo), p(fkeep),
                                                               p(ckeep), 0, stream()),
            "compact": compact,
            "torch/mean-composition": lambda: torch_mean(torch, V, F, Cc, origin, cell),
        }
        res = timed(variants, a.warmup, a.rounds, a.reps)
        moved = {"quadrics/kernel": 3 * nf * (8 + 24 + 36) + nv * (16 + 8 + 72),
                 "clusters/two-pass": nv * (8 + 8 + 12 + 12 + 72) + Vc * (16 + 28)}
        for k, b in moved.items():
            res[k]["bytes_asked"] = b
            res[k]["bytes_per_s"] = round(b / (res[k]["median_us"] * 1e-6), 1)
            res[k]["share_of_hbm_peak"] = round(b / (res[k]["median_us"] * 1e-6) / HBM_PEAK, 4)
        res["torch/mean-composition"]["over_whole_mean"] = round(res["torch/mean-composition"]["median_us"] /
                                                                 res["whole/mean"]["median_us"], 2)
        if o3d is not None:
            def host():
                m = o3d.geometry.TriangleMesh(o3d.utility.Vector3dVector(V.double().cpu().numpy()),
                                              o3d.utility.Vector3iVector(F.int().cpu().numpy()))
                m.vertex_colors = o3d.utility.Vector3dVector(Cc.double().cpu().numpy())
                s = m.simplify_vertex_clustering(cell, o3d.geometry.SimplificationContraction.Quadric)
                return torch.from_numpy(np.asarray(s.vertices)).to(dev), torch.from_numpy(np.asarray(s.triangles)).to(dev)
            host()
            ts = []
            for _ in range(a.rounds):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                host()
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e6)
            med = float(np.median(ts))
            res["open3d/quadric"] = {"median_us": round(med, 2), "min_us": round(min(ts), 2), "max_us": round(max(ts), 2),
                                     "spread": round((max(ts) - min(ts)) / med, 4),
                                     "over_whole_quadric": round(med / res["whole/quadric"]["median_us"], 2)}
        info = got[3]
        cells["%g" % kv] = {"cell": cell, "clusters": Vc, "kept_vertices": Vk, "kept_faces": Fk,
                            "members_mean": round(nv / max(Vc, 1), 2), "members_max": int(counts.max()),
                            "faces_degenerate": info["faces_degenerate"], "faces_duplicate": info["faces_duplicate"],
                            "results": res}
        print("cell of %g voxels: %d clusters (largest %d members) -> %d vertices, %d faces" % (kv, Vc, int(counts.max()), Vk, Fk))
        print("%-24s %12s %12s %12s %8s %9s" % ("variant", "median us", "min", "max", "spread", "HBM"))
        for k, r in res.items():
            print("%-24s %12.2f %12.2f %12.2f %8.4f %9s" % (k, r["median_us"], r["min_us"], r["max_us"], r["spread"],
                                                            r.get("share_of_hbm_peak", "")))
    outj = {"what": "vertex-clustering simplification (libegs_simplify.so) of the mesh of the TSDF benchmark's volume, per "
                    "cell size in voxels; us per call, median / min / max over the rounds of HIP-event brackets (open3d: host "
                    "clock); share_of_hbm_peak = bytes_asked / median / 8 TB/s (an effective rate, see the tool's docstring)",
            "size": n, "vertices": nv, "faces": nf, "largest_valence": valence, "open3d": o3d is not None,
            "reps_per_bracket": a.reps, "rounds": a.rounds, "warmup_calls": a.warmup,
            "device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "cells": cells}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(outj, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
