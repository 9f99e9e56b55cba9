"""Float64 reference of the per-Gaussian blend-weight statistics (include/egs_prune.h).  CPU only;
tests/test_gpu_blend_weights.py runs the kernel.

The walk is ``oracle/gs_oracle.py:draw``'s, restated with ``O._alpha_prime`` and bounded by a GIVEN ``contrib`` instead
of a stop test of its own: entry k of a tile's list is live at pixel p iff k < contrib[p] (pixel-box policies: and p lies
in the Gaussian's box), a hit iff live and not alpha' < alpha_skip; on a hit w = tau alpha', tau <- tau (1 - alpha').
Per Gaussian: sum of w, largest w, number of hits, and ``near`` = the number of live pixels whose alpha' lies within
SKIP_MARGIN (relative) of alpha_skip -- pixels whose hit decision a float32 evaluation may take the other way.

Two forms: ``image_stats`` over (ranges, gsid) of a whole image, ``case_stats`` over the hand-built one-tile lists of
tests/draw_tile_ref.py.  ``distance`` says how far the number format and the kernel's legitimate operations move a row.
"""
import functools

import numpy as np

from oracle import gs_oracle as O
from tests import draw_tile_ref as D

SKIP_MARGIN = D.SKIP_MARGIN
f32 = np.float32


def _alpha_poly(g, us, cinv, alphas, policy, tx, ty, hh, ww, fma, hw=None, key=0):
    """alpha' [hh, ww] and the skip decision as k_blend_weights / k_draw form them in float32 (``D.blend(poly=True)``).
    ``hw`` (1, -1 or 0 = a random sign per use, stream ``key``): the two one-ulp operations of the kernel that NumPy
    rounds correctly, each moved by its ulp in that direction, exactly as ``D.blend(hw=...)`` models them for k_draw --
    the DERIVED log2(alpha) (lskip - thr: one ulp of v_log_f32 at |thr| and the rounding of the quotient; one value per
    entry, so it moves every pixel of the entry the same way) and the exponential (v_exp_f32)."""
    q = (D.NHL2E * cinv[g, 0]).astype(f32), (f32(2) * D.NHL2E * cinv[g, 1]).astype(f32), (D.NHL2E * cinv[g, 2]).astype(f32)
    with np.errstate(all="ignore"):
        if policy.alpha_skip > 0:
            lskip = f32(np.log2(policy.alpha_skip))
            la = (lskip - np.log2(f32(policy.alpha_skip) / alphas[g]).astype(f32)).astype(f32)
        else:
            lskip = f32(-np.inf)
            la = np.log2(alphas[g]).astype(f32)
        if hw is not None:
            sg = f32(hw) if hw else (f32(1) if D.S.uniform01(4243, key, (1,))[0] < 0.5 else f32(-1))
            thr = np.log2(f32(policy.alpha_skip) / alphas[g]) if policy.alpha_skip > 0 else la
            la = (la + sg * f32(2.0 ** -23 * abs(float(thr)) + 2.0 ** -24 * 1.4427)).astype(f32)
        e = D.poly_exponent(*[np.reshape(v, (1, 1, 1)) for v in q + (us[g, 0], us[g, 1], la)],
                            np.array(tx), np.array(ty), fma=fma)[0, :hh, :ww]
        cap = f32(np.inf)
        if policy.maha_floor:
            cap = la
        if policy.alpha_clamp:
            cap = min(cap, np.log2(f32(0.99)))
        ap = np.exp2(np.minimum(e, cap)).astype(f32)
        if hw is not None:
            ap = D._ulp(ap, hw, 250000 + key)
        skip = ((e < lskip) | (alphas[g] < f32(policy.alpha_skip))) if policy.alpha_skip > 0 \
            else np.zeros((hh, ww), bool)
    return ap, skip


def walk(W, H, lists, us, cinv2ds, alphas, areas, contrib, policy, dtype=np.float64, poly=None, blocks_out=None,
         hw=None):
    """``lists``: one array of Gaussian ids per tile (row-major tiles of 16 x 16).  ``poly``: None -- ``O._alpha_prime`` in
    ``dtype``, tau <- tau (1 - alpha') as ``O.draw``; False / True -- float32 with k_draw's polynomial exponent (NumPy's
    two roundings per step / the kernel's fmaf), tau <- tau - tau alpha'; ``hw`` (with ``poly``): see ``_alpha_poly``.  ``blocks_out`` (a list): receives, per tile,
    an int array with one 4-bit mask per list entry -- bit b set iff the entry hits a pixel of 8x8 block b = (b & 1, b >> 1).
    -> sum [N], max [N] (``dtype``), hits [N] int64, near [N] int64, final_tau [H, W] (0 on empty tiles, as ``O.draw``)"""
    if poly is not None:
        dtype = np.float32
    us = np.asarray(us, dtype); cinv = np.asarray(cinv2ds, dtype); alphas = np.asarray(alphas, dtype).reshape(-1)
    n = us.shape[0]
    gx = (W + 15) // 16
    wsum = np.zeros(n, dtype); wmax = np.zeros(n, dtype)
    hits = np.zeros(n, np.int64); near = np.zeros(n, np.int64)
    final_tau = np.zeros((H, W), dtype)
    if policy.footprint == O.FOOT_BOX:
        bx0, bx1, by0, by1 = O.pixel_box(us, areas, W, H)
    for t, ids in enumerate(lists):
        if len(ids) == 0:
            if blocks_out is not None:
                blocks_out.append(np.zeros(0, np.int32))
            continue
        ty, tx = divmod(t, gx)
        y0, x0 = 16 * ty, 16 * tx
        hh, ww = min(16, H - y0), min(16, W - x0)
        py, px = np.meshgrid(np.arange(y0, y0 + hh, dtype=dtype), np.arange(x0, x0 + ww, dtype=dtype), indexing="ij")
        cont = np.asarray(contrib[y0:y0 + hh, x0:x0 + ww])
        tau = np.ones((hh, ww), dtype)
        blocks = np.zeros(len(ids), np.int32)
        if blocks_out is not None:
            blocks_out.append(blocks)
        for k in range(min(int(cont.max()), len(ids))):
            g = int(ids[k])
            if poly is None:
                ap = O._alpha_prime(alphas[g], cinv[g], us[g], px, py, policy, dtype)[0]
                skip = ap < dtype(policy.alpha_skip) if policy.alpha_skip > 0 else np.zeros((hh, ww), bool)
            else:
                ap, skip = _alpha_poly(g, us, cinv, alphas, policy, tx, ty, hh, ww, poly, hw, 1000 * t + k)
            live = k < cont
            if policy.footprint == O.FOOT_BOX:
                live = live & (px >= bx0[g]) & (px < bx1[g]) & (py >= by0[g]) & (py < by1[g])
            hit = live & ~skip
            if policy.alpha_skip > 0:
                with np.errstate(all="ignore"):
                    near[g] += int((live & (np.abs(ap - dtype(policy.alpha_skip)) < SKIP_MARGIN * policy.alpha_skip)).sum())
            if not hit.any():
                continue
            w = np.where(hit, tau * ap, 0).astype(dtype)
            tau = np.where(hit, (tau - w) if poly is not None else tau * (1 - ap), tau).astype(dtype)
            wsum[g] += w.sum(dtype=dtype)
            wmax[g] = max(wmax[g], w.max())
            hits[g] += int(hit.sum())
            for b in range(4):
                if hit[8 * (b >> 1):8 * (b >> 1) + 8, 8 * (b & 1):8 * (b & 1) + 8].any():
                    blocks[k] |= 1 << b
        final_tau[y0:y0 + hh, x0:x0 + ww] = tau
    return wsum, wmax, hits, near, final_tau


def image_stats(W, H, ranges, gsid, us, cinv2ds, alphas, areas, contrib, policy, dtype=np.float64, blocks_out=None):
    """the statistics of a whole image over its (ranges, gsid) -> (sum, max, hits, near, final_tau)"""
    ranges = np.asarray(ranges); gsid = np.asarray(gsid)
    T = ((W + 15) // 16) * ((H + 15) // 16)
    lists = [gsid[int(ranges[t, 0]):int(ranges[t, 1])] if ranges[t, 1] > ranges[t, 0] else gsid[:0] for t in range(T)]
    return walk(W, H, lists, us, cinv2ds, alphas, areas, contrib, policy, dtype, blocks_out=blocks_out)


def case_stats(name, pname, dtype=np.float64, arrays=None, poly=None, seed=0, hw=None):
    """the statistics of set ``name`` of tests/draw_tile_ref.py under policy ``pname``, bounded by the REFERENCE's contrib
    (the builder keeps every evaluation's contrib equal to it) -> (sum, max, hits, near, final_tau)"""
    c = D.case(name, seed)
    a = c.arrays if arrays is None else arrays
    ls = D.lists(c, pname)[0]
    contrib = D.reference(name, pname, seed)["contrib"]
    return walk(D.W, D.H, ls, a["us"], a["cinv2ds"], a["alphas"], a["areas"], contrib, D.POLICIES[pname], dtype, poly,
                hw=hw)


@functools.lru_cache(maxsize=None)
def reference(name, pname, seed=0):
    """float64, computed once -> dict(sum, max, hits, near, final_tau), read-only"""
    out = dict(zip(("sum", "max", "hits", "near", "final_tau"), case_stats(name, pname, seed=seed)))
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def distance(name, pname, seed=0):
    """Per row, the largest absolute distance from the float64 reference of
      (a) the float32 evaluation,
      (b) ``D.N_PERT`` float32 evaluations of the inputs moved by one ulp (``D.perturbed``),
      (c) the float32 evaluation with ``D.poly_exponent`` for the exponent (``fma`` False and True), tau -= tau alpha',
      (d) (c) with the kernel's fmaf and its two one-ulp operations -- the derived log2(alpha) and v_exp_f32 -- an ulp
          off, all up, all down, or a random sign per use (``_alpha_poly(hw=...)``, the model ``D.distances`` (e) uses for
          k_draw).  The derived logarithm is ONE value per entry: its ulp, 2^-23 |log2(alpha_skip / alpha)|, moves every
          pixel's weight of the entry the same way, up to 7e-7 of a row's sum for alpha ~ 1 -- which (a)-(c), whose
          logarithm NumPy rounds correctly, do not contain (measured on MI355X: without (d) two rows of lengths0 stood
          at 1.25 x their bound, 6.7 float32 ulps off on a sum of 128 weights)
    -> dict(sum [N], max [N], hits_equal: every one of them gave the reference's hits on every row)"""
    c = D.case(name, seed)
    ref = reference(name, pname, seed)
    d = dict(sum=np.zeros(c.n), max=np.zeros(c.n), hits_equal=True)

    def take(res):
        d["sum"] = np.maximum(d["sum"], np.abs(res[0].astype(np.float64) - ref["sum"]))
        d["max"] = np.maximum(d["max"], np.abs(res[1].astype(np.float64) - ref["max"]))
        d["hits_equal"] &= bool(np.array_equal(res[2], ref["hits"]))

    for j in range(D.N_PERT + 1):
        take(case_stats(name, pname, np.float32, None if j == 0 else D.perturbed(c.arrays, j), seed=seed))
    for fma in (False, True):
        take(case_stats(name, pname, poly=fma, seed=seed))
    for hw in (1, -1, 0):
        take(case_stats(name, pname, poly=True, seed=seed, hw=hw))
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def row_floor(name, pname, seed=0):
    """``D.pixel_floor``'s rule carried over to a row: one float32 ulp of the row's magnitude per entry blended in front
    of it and for its own accumulation, 2^-23 (2 + position of the row in its list) |ref| -- a count of roundings, not a
    measurement -> dict(sum [N], max [N])"""
    c = D.case(name, seed)
    ref = reference(name, pname, seed)
    pos = np.zeros(c.n)
    for l in D.lists(c, pname)[0]:
        pos[l] = np.arange(len(l))
    return {k: 2.0 ** -23 * (2 + pos) * np.abs(ref[k]) for k in ("sum", "max")}
