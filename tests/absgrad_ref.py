"""Float64 reference of the absolute screen-space gradient (AbsGS; ``RenderOptions.absgrad``).

A restatement of the backward walk of ``oracle/gs_oracle.py:draw_backward`` (kernel.cu:809-950) -- the same lists,
``contrib``, ``final_tau``, activity mask, skip test, clamp and NaN rule -- that keeps the per-pixel screen-space terms

    t_x = dL/dalpha' alpha' (-cinv0 dx - cinv1 dy)        t_y = dL/dalpha' alpha' (-cinv1 dx - cinv2 dy)

apart long enough to sum them twice: signed (``dus``, what ``draw_backward`` returns) and in absolute value
(``dus_abs``).  Per view, not normalised, with the scale of the upstream dL/dimage.  ``tests/test_absgrad_cpu.py`` ties
the signed sum to the oracle's, which makes this the oracle's walk."""
import numpy as np

from oracle import gs_oracle as O


def draw_backward_abs(width, height, ranges, gsid, us, cinv2ds, alphas, colors, contrib, final_tau, dloss_dgammas,
                      areas=None, policy=O.POLICY_G, tiles=None):
    """-> (dus [N,2], dus_abs [N,2]) in float64; arguments as ``O.draw_backward``."""
    dtype = np.float64
    gx, gy = O.tile_grid(width, height)
    us = np.asarray(us, dtype); cinv2ds = np.asarray(cinv2ds, dtype)
    alphas = np.asarray(alphas, dtype).reshape(-1); colors = np.asarray(colors, dtype)
    dLdg = np.asarray(dloss_dgammas, dtype)
    n = us.shape[0]
    dus = np.zeros((n, 2), dtype); dus_abs = np.zeros((n, 2), dtype)
    if policy.footprint == O.FOOT_BOX:
        bx0, bx1, by0, by1 = O.pixel_box(us, areas, width, height)
    T = O.TILE
    for t in (range(gx * gy) if tiles is None else tiles):
        r0, r1 = int(ranges[t, 0]), int(ranges[t, 1])
        if r1 - r0 == 0:
            continue
        ty, tx = divmod(int(t), gx)
        y0, x0 = ty * T, tx * T
        hh, ww = min(T, height - y0), min(T, width - x0)
        py, px = np.meshgrid(np.arange(y0, y0 + hh, dtype=dtype), np.arange(x0, x0 + ww, dtype=dtype), indexing="ij")
        tau = np.array(final_tau[y0:y0 + hh, x0:x0 + ww], dtype)
        cont = np.asarray(contrib[y0:y0 + hh, x0:x0 + ww])
        dl = dLdg[:, y0:y0 + hh, x0:x0 + ww]
        gcl = np.zeros((3, hh, ww), dtype)        # gamma_cur2last
        for k in range(r0 + int(cont.max()) - 1, r0 - 1, -1):
            g = int(gsid[k])
            ap, _, dx, dy = O._alpha_prime(alphas[g], cinv2ds[g], us[g], px, py, policy, dtype)
            act = (k - r0) < cont
            if policy.footprint == O.FOOT_BOX:
                act &= (px >= bx0[g]) & (px < bx1[g]) & (py >= by0[g]) & (py < by1[g])
            if policy.alpha_skip > 0:
                act &= ~(ap < dtype(policy.alpha_skip))
            if O.NAN_MAHA in ("skip", "entry"):
                act &= ~np.isnan(ap)
            if not act.any():
                continue
            with np.errstate(all="ignore"):
                tau_n = np.where(act, tau / (1 - ap), tau)
            c = colors[g][:, None, None]
            dl_dap = np.where(act, (dl * (tau_n[None] * (c - gcl))).sum(0), 0)
            ci = cinv2ds[g]
            t_x = dl_dap * (-ci[0] * dx - ci[1] * dy) * ap
            t_y = dl_dap * (-ci[1] * dx - ci[2] * dy) * ap
            dus[g, 0] += t_x.sum(); dus[g, 1] += t_y.sum()
            dus_abs[g, 0] += np.abs(t_x).sum(); dus_abs[g, 1] += np.abs(t_y).sum()
            gcl = np.where(act[None], ap[None] * c + (1 - ap)[None] * gcl, gcl)
            tau = tau_n
    return dus, dus_abs


# ---- the same walk over many tiles on the host's cores (the full-size tests; tests/oracle_parallel.py's scheme) --------
_NAMES = ("ranges", "gsid", "us", "cinv2ds", "alphas", "colors", "contrib", "final_tau", "dl")


def _worker(job):
    import os
    import sys
    tmp, width, height, tiles, repo = job
    if repo not in sys.path:
        sys.path.insert(0, repo)
    from tests.absgrad_ref import draw_backward_abs as walk
    a = {k: np.load(os.path.join(tmp, k + ".npy"), mmap_mode="r") for k in _NAMES}
    dus, dus_abs = walk(width, height, a["ranges"], a["gsid"], a["us"], a["cinv2ds"], a["alphas"], a["colors"],
                        a["contrib"], a["final_tau"], a["dl"], None, O.POLICY_G, tiles=tiles)
    rg = a["ranges"]
    ids = np.unique(np.concatenate([np.asarray(a["gsid"][rg[t, 0]:rg[t, 1]]) for t in tiles])).astype(np.int64)
    return ids, dus[ids], dus_abs[ids]


def draw_backward_abs_tiles(width, height, ranges, gsid, us, cinv2ds, alphas, colors, contrib, final_tau, dl, tiles,
                            procs=16):
    """``draw_backward_abs`` (policy G) with ``tiles`` dealt to worker processes (``spawn``: the parent may hold a HIP
    context); the per-tile sums are additive (tests/test_absgrad_cpu.py) and are added here in float64."""
    import multiprocessing as mp
    import os
    import shutil
    import tempfile
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ranges = np.asarray(ranges); tiles = np.asarray(tiles)
    lens = (ranges[tiles, 1] - ranges[tiles, 0]).astype(np.int64)
    tiles = tiles[lens > 0][np.argsort(-lens[lens > 0], kind="stable")]
    n = np.asarray(us).shape[0]
    dus = np.zeros((n, 2)); dus_abs = np.zeros((n, 2))
    if len(tiles) == 0:
        return dus, dus_abs
    procs = max(1, min(procs, os.cpu_count() or 1, len(tiles)))
    chunks = [tiles[i::4 * procs] for i in range(min(len(tiles), 4 * procs))]
    arrays = dict(ranges=ranges, gsid=np.asarray(gsid), us=np.asarray(us, np.float64),
                  cinv2ds=np.asarray(cinv2ds, np.float64), alphas=np.asarray(alphas, np.float64).reshape(-1),
                  colors=np.asarray(colors, np.float64), contrib=np.asarray(contrib),
                  final_tau=np.asarray(final_tau, np.float64), dl=np.asarray(dl, np.float64))
    tmp = tempfile.mkdtemp(prefix="egs_absgrad_")
    try:
        for k, v in arrays.items():
            np.save(os.path.join(tmp, k + ".npy"), v)
        jobs = [(tmp, width, height, c, repo) for c in chunks]
        pool = mp.get_context("spawn").Pool(procs) if procs > 1 else None
        try:
            for ids, a, b in (pool.imap_unordered(_worker, jobs) if pool is not None else map(_worker, jobs)):
                np.add.at(dus, ids, a); np.add.at(dus_abs, ids, b)
        finally:
            if pool is not None:
                pool.close(); pool.join()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return dus, dus_abs
