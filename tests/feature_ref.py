"""Float64 reference of the per-Gaussian feature render and its adjoint (include/egs_feat.h).  CPU only;
tests/test_gpu_features.py runs the kernels.

The walk is ``tests/blend_weights_ref.walk``'s: ``O._alpha_prime``, bounded by a GIVEN ``contrib`` instead of a stop test
of its own.  Entry k of a tile's list is live at pixel p iff k < contrib[p] (pixel-box policies: and p lies in the
Gaussian's box), a hit iff live and not alpha' < alpha_skip; on a hit w = tau alpha', tau <- tau (1 - alpha').
  feature map   fmap[c, p]  = sum_k w_k(p) feats[g_k, c]
  gather        out[g, c]  += sum_p w(p) gmap[c, p]          (and ``absg``: the same sum over |gmap|, for the floors)
  near [H, W]   live entries whose alpha' lies within SKIP_MARGIN (relative) of alpha_skip -- entries whose hit decision
                a float32 evaluation may take the other way at that pixel.

Two forms: ``image_walk`` over (ranges, gsid) of a whole image, ``case_walk`` over the hand-built one-tile lists of
tests/draw_tile_ref.py.  ``reference`` / ``distance`` are computed ONCE per (set, policy) at C_MAX channels; a test of
C channels reads the first C (``feats`` and ``gmap`` of C channels ARE the first C of C_MAX, so are their results).
"""
import functools

import numpy as np

from easygaussiansplatting_amd import scene as S
from oracle import gs_oracle as O
from tests import blend_weights_ref as B
from tests import draw_tile_ref as D

SKIP_MARGIN = D.SKIP_MARGIN
C_MAX = 20
f32 = np.float32


def walk(W, H, lists, us, cinv2ds, alphas, areas, contrib, policy, feats, gmap=None, dtype=np.float64, poly=None,
         hw=None):
    """``lists``: one array of Gaussian ids per tile (row-major tiles of 16 x 16); ``feats`` [N,C]; ``gmap`` [C',H,W] or
    None (the two operators are independent: C' need not be C).  ``poly`` / ``hw``: as ``B.walk`` (float32 with k_draw's
    polynomial exponent, tau <- tau - tau alpha'; the kernel's two one-ulp operations an ulp off).
    -> fmap [C,H,W], gathered [N,C'] (None without ``gmap``), absg [N,C'] (likewise), near [H,W] int64"""
    if poly is not None:
        dtype = np.float32
    us = np.asarray(us, dtype); cinv = np.asarray(cinv2ds, dtype); alphas = np.asarray(alphas, dtype).reshape(-1)
    feats = np.asarray(feats, dtype)
    n, C = feats.shape
    gx = (W + 15) // 16
    fmap = np.zeros((C, H, W), dtype)
    near = np.zeros((H, W), np.int64)
    gath = absg = None
    if gmap is not None:
        gmap = np.asarray(gmap, dtype)
        gath = np.zeros((n, gmap.shape[0]), dtype); absg = np.zeros((n, gmap.shape[0]), dtype)
    if policy.footprint == O.FOOT_BOX:
        bx0, bx1, by0, by1 = O.pixel_box(us, areas, W, H)
    for t, ids in enumerate(lists):
        if len(ids) == 0:
            continue
        ty, tx = divmod(t, gx)
        y0, x0 = 16 * ty, 16 * tx
        hh, ww = min(16, H - y0), min(16, W - x0)
        py, px = np.meshgrid(np.arange(y0, y0 + hh, dtype=dtype), np.arange(x0, x0 + ww, dtype=dtype), indexing="ij")
        cont = np.asarray(contrib[y0:y0 + hh, x0:x0 + ww])
        tau = np.ones((hh, ww), dtype)
        acc = np.zeros((C, hh, ww), dtype)
        gm = gmap[:, y0:y0 + hh, x0:x0 + ww] if gmap is not None else None
        for k in range(min(int(cont.max()), len(ids))):
            g = int(ids[k])
            if poly is None:
                ap = O._alpha_prime(alphas[g], cinv[g], us[g], px, py, policy, dtype)[0]
                skip = ap < dtype(policy.alpha_skip) if policy.alpha_skip > 0 else np.zeros((hh, ww), bool)
            else:
                ap, skip = B._alpha_poly(g, us, cinv, alphas, policy, tx, ty, hh, ww, poly, hw, 1000 * t + k)
            live = k < cont
            if policy.footprint == O.FOOT_BOX:
                live = live & (px >= bx0[g]) & (px < bx1[g]) & (py >= by0[g]) & (py < by1[g])
            hit = live & ~skip
            if policy.alpha_skip > 0:
                with np.errstate(all="ignore"):
                    near[y0:y0 + hh, x0:x0 + ww] += live & (np.abs(ap - dtype(policy.alpha_skip))
                                                            < SKIP_MARGIN * policy.alpha_skip)
            if not hit.any():
                continue
            w = np.where(hit, tau * ap, 0).astype(dtype)
            tau = np.where(hit, (tau - w) if poly is not None else tau * (1 - ap), tau).astype(dtype)
            acc += w[None] * feats[g][:, None, None]
            if gm is not None:
                gath[g] += (w[None] * gm).sum((1, 2), dtype=dtype)
                absg[g] += (w[None] * np.abs(gm)).sum((1, 2), dtype=dtype)
        fmap[:, y0:y0 + hh, x0:x0 + ww] = acc
    return fmap, gath, absg, near


def image_walk(W, H, ranges, gsid, us, cinv2ds, alphas, areas, contrib, policy, feats, gmap=None, dtype=np.float64):
    """the walk of a whole image over its (ranges, gsid) -> (fmap, gathered, absg, near)"""
    ranges = np.asarray(ranges); gsid = np.asarray(gsid)
    T = ((W + 15) // 16) * ((H + 15) // 16)
    lists = [gsid[int(ranges[t, 0]):int(ranges[t, 1])] if ranges[t, 1] > ranges[t, 0] else gsid[:0] for t in range(T)]
    return walk(W, H, lists, us, cinv2ds, alphas, areas, contrib, policy, feats, gmap, dtype)


# ------------------------------------------------------------------------------------------------------ test inputs
def case_feats(name, seed=0):
    """[N, C_MAX] float32 in [-1, 1] from scene.py's counter generator (fixed keys; a pure function of the set)"""
    n = D.case(name, seed).n
    return (2.0 * S.uniform01(7100 + 16 * D.SETS.index(name) + seed, 1, (n, C_MAX)) - 1.0).astype(f32)


def case_gmap(name, seed=0):
    """[C_MAX, H, W] float32 in [-1, 1]: the pixel gradients of the gather"""
    return (2.0 * S.uniform01(7100 + 16 * D.SETS.index(name) + seed, 2, (C_MAX, D.H, D.W)) - 1.0).astype(f32)


def case_walk(name, pname, feats, gmap=None, dtype=np.float64, arrays=None, poly=None, seed=0, hw=None):
    """the walk of set ``name`` of tests/draw_tile_ref.py under policy ``pname``, bounded by the REFERENCE's contrib"""
    c = D.case(name, seed)
    a = c.arrays if arrays is None else arrays
    ls = D.lists(c, pname)[0]
    contrib = D.reference(name, pname, seed)["contrib"]
    return walk(D.W, D.H, ls, a["us"], a["cinv2ds"], a["alphas"], a["areas"], contrib, D.POLICIES[pname], feats, gmap,
                dtype, poly, hw)


@functools.lru_cache(maxsize=None)
def reference(name, pname, seed=0):
    """float64, C_MAX channels, computed once -> dict(map [C,H,W], gather [N,C], absg [N,C], near [H,W]), read-only"""
    out = dict(zip(("map", "gather", "absg", "near"),
                   case_walk(name, pname, case_feats(name, seed), case_gmap(name, seed), seed=seed)))
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def distance(name, pname, seed=0):
    """Per pixel and channel (``map``) and per row and channel (``gather``), the largest absolute distance from the
    float64 reference of the evaluations (a)-(d) of ``B.distance``:
      (a) the float32 evaluation,
      (b) ``D.N_PERT`` float32 evaluations of the inputs moved by one ulp (``D.perturbed``),
      (c) the float32 evaluation with ``D.poly_exponent`` for the exponent (``fma`` False and True), tau -= tau alpha',
      (d) (c) with the kernel's fmaf and its two one-ulp operations -- the derived log2(alpha) and v_exp_f32 -- an ulp
          off, all up, all down, or a random sign per use (``B._alpha_poly(hw=...)``).
    Features and pixel gradients are float32 inputs and enter every evaluation unchanged.
    -> dict(map [C_MAX,H,W], gather [N,C_MAX]); a test of C channels takes the largest of a pixel's first C planes."""
    c = D.case(name, seed)
    ref = reference(name, pname, seed)
    feats, gmap = case_feats(name, seed), case_gmap(name, seed)
    d = dict(map=np.zeros(ref["map"].shape), gather=np.zeros(ref["gather"].shape))

    def take(res):
        d["map"] = np.maximum(d["map"], np.abs(res[0].astype(np.float64) - ref["map"]))
        d["gather"] = np.maximum(d["gather"], np.abs(res[1].astype(np.float64) - ref["gather"]))

    for j in range(D.N_PERT + 1):
        take(case_walk(name, pname, feats, gmap, np.float32, None if j == 0 else D.perturbed(c.arrays, j), seed=seed))
    for fma in (False, True):
        take(case_walk(name, pname, feats, gmap, poly=fma, seed=seed))
    for hw in (1, -1, 0):
        take(case_walk(name, pname, feats, gmap, poly=True, seed=seed, hw=hw))
    for v in d.values():
        v.setflags(write=False)
    return d


def pixel_floor(name, pname, feats, seed=0):
    """``D.pixel_floor`` with the features in the colours' place: one float32 ulp of a pixel's largest running magnitude
    per blended entry, 2^-23 (2 + contrib) max(1, max |feat| of the tile's list) -- a count of roundings, not a
    measurement -> [H,W]"""
    c = D.case(name, seed)
    contrib = D.reference(name, pname, seed)["contrib"]
    fmax = np.ones((D.H, D.W))
    for t, l in enumerate(D.lists(c, pname)[0]):
        tx, ty, x0, y0, ww, hh = D.geom(t)
        if len(l):
            fmax[y0:y0 + hh, x0:x0 + ww] = max(1.0, float(np.abs(np.asarray(feats)[l]).max()))
    return 2.0 ** -23 * (2 + contrib) * fmax


def row_floor(name, pname, seed=0):
    """``B.row_floor``'s rule on the gather: one float32 ulp of the row's magnitude per entry blended in front of it and
    for its own accumulation, 2^-23 (2 + position in list) |ref| with |ref| taken on sum_p w |gmap| (a signed sum may
    cancel, its roundings do not) -> [N, C_MAX]"""
    c = D.case(name, seed)
    pos = np.zeros(c.n)
    for l in D.lists(c, pname)[0]:
        pos[l] = np.arange(len(l))
    return 2.0 ** -23 * (2 + pos)[:, None] * reference(name, pname, seed)["absg"]
