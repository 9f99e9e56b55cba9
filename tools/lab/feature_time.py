"""Time ``features.render_features`` / ``gather_features`` (k_feature_render, k_feature_gather) beside the
same process's k_draw and k_draw_bwd.

    python tools/lab/feature_time.py [--scene big|skewed] [--channels 3 8 32] [--warmup 5] [--calls 20]

HIP events around each call on the state of one fused forward of the scene at its own resolution; the two draw kernels
from the library's per-kernel timer (egs_prof_*) over three forward + backward steps of the same scene, after the
warm-up steps that also bring the clocks to their steady state.  Prints one JSON line."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", choices=("big", "skewed"), default="big")
    ap.add_argument("--channels", type=int, nargs="+", default=[3, 8, 32])
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    import torch
    from easygaussiansplatting_amd import _lib, features, fused, scene as S
    from easygaussiansplatting_amd.function import Camera, GSFunction
    from tools.benchlib import parse_report
    dev = torch.device("cuda:0")
    sc = S.big_scene() if a.scene == "big" else S.skewed_scene()
    cam = Camera.from_scene(sc.cam, dev)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)
    P = [t(sc.pws), t(sc.shs), t(sc.alphas).reshape(-1, 1).clone(), t(sc.scales), t(sc.rots)]
    for p in P:
        p.requires_grad_(True)
    us0 = torch.zeros((sc.n, 2), device=dev, requires_grad=True)
    W, H = sc.cam.width, sc.cam.height
    dl = torch.from_numpy(S.normal(1, 77, (3, H, W)).astype(np.float32)).to(dev) / (3 * H * W)
    lib = _lib.load()
    GSFunction.mode = "fused"

    def step():
        for p in P:
            p.grad = None
        us0.grad = None
        img, _ = GSFunction.apply(*P, us0, cam)
        img.backward(dl)

    for _ in range(6):
        step()
    torch.cuda.synchronize()
    lib.egs_prof_set_filter(None); lib.egs_prof_reset(); lib.egs_prof_enable(1)
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    lib.egs_prof_enable(0)
    need = lib.egs_prof_report(None, 0)
    buf = ctypes.create_string_buffer(need + 16)
    lib.egs_prof_report(buf, need + 16)
    rep = parse_report(buf.value.decode())
    lib.egs_prof_reset()
    kern = {k: round(tot / c * 1e3, 1) for k, (c, tot) in rep.items() if k.startswith("k_draw") or k.startswith("k_seg")}

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.calls)]
        for e0, e1 in ev:
            e0.record()
            fn()
            e1.record()
        torch.cuda.synchronize()
        us = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev)
        return {"median": round(us[len(us) // 2], 1), "min": round(us[0], 1), "max": round(us[-1], 1)}

    times = {}
    with torch.no_grad():
        _, _, st = fused.forward(*[p.detach() for p in P], cam, need_grad=False)
        st.patch_count()
        for c in a.channels:
            feats = t(2.0 * S.uniform01(5, c, (sc.n, c)) - 1.0)
            gmap = t(2.0 * S.uniform01(6, c, (c, H, W)) - 1.0)
            out = torch.zeros((sc.n, c), dtype=torch.float32, device=dev)
            times["C=%d" % c] = {"render_us": timed(lambda: features.render_features(st, feats)),
                                 "gather_us": timed(lambda: features.gather_features(st, gmap, out=out))}
    lens = (st.ranges[:, 1] - st.ranges[:, 0]).clamp_min(0)
    print(json.dumps({"scene": a.scene, "gaussians": sc.n, "width": W, "height": H, "patches": int(st.patch_count()),
                      "max_list_len": int(lens.max()), "max_walk": int(st.contrib.max()), "culled_lists": bool(st.culled),
                      "calls": a.calls, "warmup": a.warmup, "features": times, "draw_kernels_avg_us": kern}))


if __name__ == "__main__":
    main()
