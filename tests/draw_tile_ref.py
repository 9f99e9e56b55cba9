"""Hand-built one-tile lists for the draw kernels (k_draw / k_draw_bwd and the segment kernels that share their
bodies, csrc/egs_draw.hip), and their float64 reference.  CPU only; tests/test_gpu_draw_tiles.py runs the kernels.

``areas`` is an input of ``splat`` independent of ``cinv2ds``: a Gaussian whose ``us +- areas`` stays inside one tile is
binned to exactly that tile whatever its conic, and depths 1 + 0.01 (position in list) fix the list order.  So every
tile of a 72 x 40 image (5 x 3 tiles; the right column 8 px wide, the bottom row 8 px high) carries ONE scenario: a list
of a chosen length whose entries hit, miss, stop and clamp where the scenario says.  Every Gaussian sits on one tile and
therefore receives one atomic set: its gradient row is deterministic.

``case(name, seed)`` is a pure function on scene.py's counter generator.  The builder enforces, on the reference alone
(never on a kernel's output), that no decision of the blend is close enough to its threshold for a float32 evaluation
to take it the other way:
  * the float64 ``O.draw``, the float32 ``O.draw`` and four float32 evaluations of the inputs moved by one ulp
    (``pergaussian_ref.perturbed``) give the same ``contrib`` on every pixel, under policy G and policy A;
  * no live (entry, pixel) has alpha' within SKIP_MARGIN (relative) of ``alpha_skip``: five times the largest exponent
    error tests/test_exponent_polynomial.py admits (2e-4 in log2 = 1.4e-4 relative);
  * no post-blend transmittance lies within STOP_MARGIN (relative) of ``tau_stop``: 1 - alpha' amplifies the rounding of
    alpha' up to 100-fold next to the 0.99 clamp.
A Gaussian that violates one is RE-DRAWN from its next counter stream (bounded); none is excluded, so no pixel and no row
is left out of any comparison.  ``report(name)`` states the re-draws, list lengths, per-block stop indices and the hit /
clamp / floor counts; ``check_claims`` asserts that every scenario still is what it says.

Render extras (``case(name, seed, extras=True)``; tests/test_gpu_draw_tiles_extras.py runs the EXTRA instances of the
kernels on them).  No decision of the blend depends on z, the background or the upstream gradients of the depth and
opacity maps, so the geometry, the lists and every claim are those of the plain case: nothing is re-drawn.  Added, all
from the counter generator: a per-Gaussian camera-space ``z`` (log-uniform over 0.2 .. 100, independent of the list-order
``depths``: a z taken from the wrong entry is orders of magnitude off), ``dloss_ddepth`` / ``dloss_dalpha`` drawn like
``dloss_dgammas`` and zero on the same block, and the background BG.  ``reference``, ``distances`` and ``pixel_floor``
with ``extras=True`` also cover ``depth``, ``alpha`` and ``dz``; ``blend`` and ``backward_hw`` restate the EXTRA kernels'
own operations (cd += w z, alpha = 1 - tau, fmaf(tau, bg, c); dq = fmaf(dL/ddepth, z, ..) - lq, dz += dL/ddepth w).
``distances`` also carries ``dus_abs``: the rows of the absolute screen-space gradient (tests/absgrad_ref.py)."""
import functools

import numpy as np

from easygaussiansplatting_amd import scene as S
from oracle import gs_oracle as O

W, H = 72, 40
GX, GY = 5, 3
T = GX * GY
SETS = ("lengths0", "lengths1", "stops", "reach", "values")
POLICIES = {"gsplatcu": O.POLICY_G, "forward_cpu": O.POLICY_A}
SKIP_MARGIN = 1e-3
STOP_MARGIN = 1e-2
MAX_ROUNDS = 12
N_PERT = 4
NU = 12                                      # uniforms per (Gaussian, retry)
f32 = np.float32
NHL2E = f32(-0.72134752044)                  # -0.5 log2(e): the record's pre-scaled conic (egs_gaussian_math.h)
STEEP = 1.0 / 0.3                            # the steepest legal conic: cov2d carries the +0.3 dilation
BG = (0.2, 0.5, 0.9)                         # the background of the extras cases


def geom(t):
    """-> tx, ty, x0, y0, visible width, visible height of tile ``t``"""
    ty, tx = divmod(t, GX)
    return tx, ty, 16 * tx, 16 * ty, min(16, W - 16 * tx), min(16, H - 16 * ty)


# ----------------------------------------------------------------------------------------------------------- entries
# An entry is (kind, parameter).  What its Gaussian is, as a function of the tile and NU uniforms:
#   wide   a      sigma 20..30 px, |rho| <= 0.6, centre within 1.5 px of the tile's middle, opacity (0.6..1) a
#   out    a      sigma ~500 px, the centre 300 px outside the image through the tile's own image edge, opacity (0.6..1) a
#   near   a      sigma 60..80 px, the centre 9..20 px outside the image (inside 1.3 x the image: policy A keeps it)
#   opq    a      sigma ~500 px, centre near the middle, opacity exactly a: full coverage at (almost) a
#   blk    (b,a)  sigma 0.8..1.05 px at the middle of 8x8 block b: confined to that block, opacity (0.5..1) a
#   sub    -      sub-pixel (cinv = 1/0.3) between four pixel centres, opacity 0.0025: above the skip threshold at its
#                 centre, below it on every pixel -- reaches a block, hits nothing
#   skip   -      wide, opacity 0.0015 < alpha_skip: never blends
#   two    -      sigma 0.8..1 px on the border of blocks 0 and 1
#   none   -      sigma 5 px, 300 px outside: reaches no block
#   clamp  a      sigma 30 px, opacity exactly a (0.99, 0.995, 1.0): the 0.99 clamp binds around the centre only
#   indef  -      indefinite conic: the maha >= 0 floor binds on two quadrants of the tile
#   steep  c      cinv = 1/0.3 on the corner pixel c (0..3) of the tile's visible part: the polynomial exponent's worst case
#   wall   -      sigma_x 4 px, sigma_y 500 px over the visible half of a ragged tile, opacity 1
# Expected hits of the entry under policy G while nothing has stopped: A all visible pixels, S some, N none.
KIND_CODE = dict(wide="A", out="A", near="A", opq="A", blk="S", sub="N", skip="N", two="S", none="N", clamp="A", indef="*",
                 steep="S", wall="*")


def _sig2cinv(sx, sy, rho):
    d = 1.0 - rho * rho
    return np.array([1.0 / (sx * sx * d), -rho / (sx * sy * d), 1.0 / (sy * sy * d)])


def _outside(t, U, mid, far=True):
    """a centre outside the image, through an image edge the tile touches: 300 px, or (not ``far``) few enough to stay
    inside 1.3 x the image, where policy A's far cull (gausplat.py:208) leaves it alone"""
    tx, ty, x0, y0, ww, hh = geom(t)
    u = mid.copy()
    if tx == 0:
        u[0] = -(300.0 if far else 15.0) - 5.0 * U[6]
    elif tx == GX - 1:
        u[0] = W + (300.0 if far else 15.0) + 5.0 * U[6]
    elif ty == 0:
        u[1] = -(300.0 if far else 15.0) - 5.0 * U[6]
    elif ty == GY - 1:
        u[1] = H + (300.0 if far else 8.5) + 2.5 * U[6]
    else:
        raise ValueError("tile %d touches no image edge" % t)
    return u


def _gaussian(kind, par, t, U):
    """-> u [2], cinv [3], alpha, colour [3] (float64; rounded to float32 by the caller)"""
    tx, ty, x0, y0, ww, hh = geom(t)
    mid = np.array([x0 + 8.0 + 3.0 * (U[0] - 0.5), y0 + 8.0 + 3.0 * (U[1] - 0.5)])
    col = -0.3 + 1.3 * U[3:6]                       # negative components included
    sym = lambda v: 2.0 * v - 1.0
    if kind in ("wide", "skip"):
        a = 0.0015 if kind == "skip" else par * (0.6 + 0.4 * U[2])
        return mid, _sig2cinv(20 + 10 * U[7], 20 + 10 * U[8], 0.6 * sym(U[9])), a, col
    if kind == "out":
        s = 500.0 * (0.8 + 0.4 * U[7])
        return _outside(t, U, mid), _sig2cinv(s, s * (0.9 + 0.2 * U[8]), 0.3 * sym(U[9])), par * (0.6 + 0.4 * U[2]), col
    if kind == "near":
        return (_outside(t, U, mid, far=False), _sig2cinv(60 + 20 * U[7], 60 + 20 * U[8], 0.3 * sym(U[9])),
                par * (0.6 + 0.4 * U[2]), col)
    if kind == "none":
        return _outside(t, U, mid), _sig2cinv(5.0, 5.0, 0.0), 0.5, col
    if kind == "opq":
        s = 500.0 * (0.8 + 0.4 * U[7])
        return mid, _sig2cinv(s, s * (0.9 + 0.2 * U[8]), 0.3 * sym(U[9])), par, col
    if kind == "clamp":
        return mid, _sig2cinv(30.0, 30.0 * (0.9 + 0.2 * U[8]), 0.2 * sym(U[9])), par, col
    if kind == "blk":
        b, a = par
        u = np.array([x0 + 8 * (b & 1) + 3.5 + sym(U[0]) * 0.5, y0 + 8 * (b >> 1) + 3.5 + sym(U[1]) * 0.5])
        s = 0.8 + 0.25 * U[7]
        return u, _sig2cinv(s, s, 0.0), a * (0.5 + 0.5 * U[2]), col
    if kind == "two":
        u = np.array([x0 + 7.5 + 0.2 * sym(U[0]), y0 + 3.5 + sym(U[1])])
        s = 0.8 + 0.2 * U[7]
        return u, _sig2cinv(s, s, 0.0), 0.3 + 0.3 * U[2], col
    if kind == "sub":
        i, j = 2 + int(U[0] * (ww - 4)), 2 + int(U[1] * (hh - 4))
        return np.array([x0 + i + 0.5, y0 + j + 0.5]), np.array([STEEP, 0.0, STEEP]), 0.0025, col
    if kind == "indef":
        s = 0.5 + U[7]
        return mid, np.array([0.01 * s, 0.016 * s * (1 if U[9] < 0.5 else -1), 0.01 * s]), 0.05, col
    if kind == "steep":
        # (the corner pixel itself would need areas = 1 to reach over the tile's low edge: one pixel in, where the
        # polynomial's monomials are 6.5 instead of 7.5; the high corner is exact)
        dx = (1.02 + 0.05 * U[0]) if not (par & 1) else (ww - 1.07 + 0.05 * U[0])
        dy = (1.02 + 0.05 * U[1]) if not (par >> 1) else (hh - 1.07 + 0.05 * U[1])
        return np.array([x0 + dx, y0 + dy]), np.array([STEEP, 0.0, STEEP]), 0.3 + 0.5 * U[2], col
    if kind == "wall":
        u = np.array([x0 + 3.5 + 0.5 * sym(U[0]), mid[1]]) if ww < 16 else np.array([mid[0], y0 + 3.5 + 0.5 * sym(U[1])])
        c = _sig2cinv(4.0, 500.0, 0.0) if ww < 16 else _sig2cinv(500.0, 4.0, 0.0)
        return u, c, 1.0, col
    raise ValueError(kind)


def _fit_area(u, t):
    """the largest ``areas`` (<= 8 per axis) that keeps ``u +- areas`` on tile ``t`` alone (kernel.cu:82-122)"""
    tx, ty, x0, y0, ww, hh = geom(t)
    r = [0, 0]
    for ax, (c, o, size, last) in enumerate(((u[0], x0, W, tx == GX - 1), (u[1], y0, H, ty == GY - 1))):
        d = c - o
        if c < 0:
            r[ax] = int(np.floor(-c)) + 10                 # u + r in [10, 11): column / row 0 only
        elif c > size and last:
            r[ax] = int(np.floor(d - 0.5))                 # u - r in [o + 0.5, o + 1.5); the far side is clipped
        else:
            assert 1.01 <= d <= 14.99, (u, t)
            r[ax] = int(min(8, np.floor(d - 0.01), np.floor(16.99 - d)))
    return r


# --------------------------------------------------------------------------------------------------------- scenarios
def _w(n, a=0.02):
    return [("wide", a)] * n


def _mix(n, t, kind="out"):
    """a lengths list of ``n`` entries: wide ones, on image-edge tiles every fifth with its centre outside the image
    (``kind`` out: 300 px, which policy A culls; near: inside 1.3 x the image, so policy A walks the same list)"""
    tx, ty = geom(t)[:2]
    edge = tx in (0, GX - 1) or ty in (0, GY - 1)
    return [(kind, 0.02) if (edge and i % 5 == 3) else ("wide", 0.02) for i in range(n)]


def _stop_at(k, tail=70):
    """every pixel finishes exactly at entry ``k`` (contrib = k): thin entries, then 0.95, 0.95, 0.99 -- tau falls to
    0.0025 and then to 2.5e-5 of what it was --, then ``tail`` entries that must stay inert"""
    return _w(k - 3, 0.01) + [("opq", 0.95), ("opq", 0.95), ("opq", 1.0)] + _w(tail, 0.5)


def _runs():
    out = [("wide", 0.02)]
    for r in (1, 3, 4, 5, 9):
        out += [("sub", None) if i % 2 == 0 else ("skip", None) for i in range(r)] + [("wide", 0.02)]
    return out


def _hits_among(h, n=70):
    """exactly ``h`` hitting entries among ``n``, spread over both chunks"""
    at = {int(round((i + 0.5) * n / h)) % n for i in range(h)}
    assert len(at) == h
    return [("wide", 0.05) if i in at else (("sub", None) if i % 3 else ("skip", None)) for i in range(n)]


def _scenarios(name):
    """-> list of T scenarios: dict(entries=[(kind, par)], and what is claimed of the realised blend under policy G:
    ``codes`` per entry (A / S / N as KIND_CODE, I: inert behind a stop, *: unclaimed), ``contrib``: every visible pixel's
    contributor count, ``bmax``: largest contrib per 8x8 block (None: not visible), ``partial``: entries whose clamp /
    floor binds on some but not all pixels)"""
    sc = [dict(entries=[]) for _ in range(T)]

    def put(t, entries, **claims):
        sc[t] = dict(entries=list(entries), **claims)

    if name == "lengths0":
        # tile 4 is the ragged column's top, 10..13 the ragged row, 14 the 8 x 8 corner
        for t, n in enumerate((1, 2, 3, 4, 63, 5, 7, 8, 9, 64, 65, 127, 128, 129, 192)):
            put(t, _mix(n, t, "near"), contrib=n)
    elif name == "lengths1":
        for t, n in enumerate((193, 0, 65, 129, 300, 64, 9, 0, 5, 128, 8, 63, 1, 0, 300)):
            put(t, _mix(n, t), contrib=n)
    elif name == "stops":
        # blocks that finish at very different indices: three wide entries, then 127 confined to block 3
        put(0, _w(3) + [("blk", (3, 0.03))] * 127, bmax=[3, 3, 3, 130])
        put(1, [("blk", (0, 0.03))] * 66 + _w(2) + [("blk", (2, 0.03))] * 62, bmax=[68, 68, 130, 68])
        for t, k in ((2, 8), (3, 9), (5, 64), (6, 65), (7, 8), (8, 65)):
            e = _stop_at(k)
            put(t, e, contrib=k, codes="".join("A" if i < k else "I" for i in range(len(e))))
        # ragged tiles: full stops there too, and lists whose in-image pixels all finish while the lanes outside the
        # image (clamped loads) would still be alive
        e = _stop_at(9, 20)
        put(4, e, contrib=9, codes="A" * 9 + "I" * 20)
        e = _stop_at(64, 20)
        put(12, e, contrib=64, codes="A" * 64 + "I" * 20)
        for t in (9, 14, 11):
            e = _w(2) + [("wall", None)] * 12 + _w(10, 0.5)
            put(t, e, codes="AA" + "*" * 12 + "I" * 10)
        put(10, _w(66) + [("blk", (1, 0.03))] * 64, bmax=[66, 130, None, None])
        put(13, [("blk", (0, 0.9))] * 40 + _w(30), codes="*" * 40 + "S" * 30)
    elif name == "reach":
        put(0, [("blk", (b % 4, 0.5)) for b in range(12)], bmax=[9, 10, 11, 12])
        put(1, [("two", None)] * 6 + [("blk", (2, 0.4))] * 3, bmax=[6, 6, 9, 0])
        put(2, [("none", None)] * 3 + _w(2) + [("none", None)] * 3, contrib=5)
        put(3, [("skip", None)] * 5 + _w(1) + [("skip", None)] * 66, contrib=6)
        put(4, _runs(), contrib=len(_runs()))
        put(5, _runs(), contrib=len(_runs()))
        put(6, [("sub", None)] * 20, contrib=0)
        put(7, [("sub", None) if i % 2 else ("skip", None) for i in range(70)], contrib=0)
        for t, h in ((8, 1), (9, 2), (10, 3), (11, 4), (12, 5)):
            put(t, _hits_among(h), hitting=h)
        put(13, [("sub", None)] * 65 + _w(1), contrib=66)
        put(14, [("none", None)] * 4 + [("sub", None)] * 4 + _w(3) + [("skip", None)] * 2, contrib=11)
    elif name == "values":
        for t, a in ((0, 0.99), (1, 0.995), (2, 1.0), (4, 1.0), (13, 0.995)):
            put(t, _w(2) + [("clamp", a)] + _w(3), contrib=6, partial=[2] if a > 0.99 else [])
        put(3, _w(1) + [("indef", None)] * 4 + _w(2), contrib=7, partial=[1, 2, 3, 4])
        put(5, [("steep", c) for c in (0, 1, 2, 3, 3, 2, 1, 0)] + _w(1), contrib=9)
        put(9, [("steep", c) for c in (3, 1, 2, 0)] + _w(2), contrib=6)
        put(14, [("steep", c) for c in (0, 3, 3, 0)] + _w(1), contrib=5)
        put(6, [("opq", 0.3), ("opq", 0.5)] + _w(3), contrib=5)
        put(7, _w(66) + [("indef", None)] * 3 + _w(1), contrib=70, partial=[66, 67, 68])
        put(8, [("opq", 0.2)] * 3, contrib=3)
        put(10, [("out", 0.3), ("out", 0.6)] + _w(2) + [("out", 0.4)], contrib=5)
        put(11, [("out", 0.5)] + [("indef", None)] + [("clamp", 1.0)], contrib=3, partial=[1, 2])
        put(12, [("opq", 0.4), ("out", 0.4), ("steep", 1), ("steep", 2)] + _w(1), contrib=5)
    else:
        raise ValueError(name)
    for s in sc:
        s.setdefault("codes", "".join(KIND_CODE[k] for k, _ in s["entries"]))
        assert len(s["codes"]) == len(s["entries"])
    return sc


def _zero_block(name):
    """(tile, 8x8 block) on which dloss_dgammas is exactly zero"""
    return {"lengths0": (9, 1), "lengths1": (4, 0), "stops": (1, 2), "reach": (0, 2), "values": (5, 3)}[name]


# ------------------------------------------------------------------------------------------------------------ builder
class Case:
    """One image: the seven read-only float32 / int32 input arrays, the intended lists and what the builder found."""


def _seed_of(name, seed):
    return 1000 * (seed + 1) + 16 * SETS.index(name)


def _assemble(name, seed, retry):
    """the arrays of set ``name`` with Gaussian g drawn from counter stream ``retry[g]``"""
    sc = _scenarios(name)
    n = sum(len(s["entries"]) for s in sc)
    # Gaussian indices are scattered over the lists, so that gsid_per_patch is no arange
    perm = np.argsort(S.uniform01(_seed_of(name, seed), 9999, (n,)), kind="stable")
    us = np.zeros((n, 2)); cinv = np.zeros((n, 3)); alphas = np.zeros(n); colors = np.zeros((n, 3))
    depths = np.zeros(n); areas = np.zeros((n, 2), np.int32)
    tile_of = np.zeros(n, np.int32); pos_of = np.zeros(n, np.int32)
    lists, at = [], 0
    streams = {}
    for t, s in enumerate(sc):
        ids = perm[at:at + len(s["entries"])]
        at += len(s["entries"])
        lists.append(ids.astype(np.int32))
        for pos, ((kind, par), g) in enumerate(zip(s["entries"], ids)):
            r = int(retry[g])
            if (t, r) not in streams:
                streams[(t, r)] = S.uniform01(_seed_of(name, seed) + t, r, (max(len(s["entries"]), 1), NU))
            u, c, a, col = _gaussian(kind, par, t, streams[(t, r)][pos])
            us[g], cinv[g], alphas[g], colors[g] = u, c, a, col
            depths[g] = 1.0 + 0.01 * pos
            tile_of[g], pos_of[g] = t, pos
    us = us.astype(f32)
    for g in range(n):
        areas[g] = _fit_area(us[g].astype(np.float64), int(tile_of[g]))
    return dict(us=us, cinv2ds=cinv.astype(f32), alphas=alphas.astype(f32), colors=colors.astype(f32),
                depths=depths.astype(f32), areas=areas), lists, tile_of, pos_of, sc


def lists_to_arrays(lists):
    """-> patch_range_per_tile [T,2] int32 (empty tiles 0, 0 as getRanges leaves them), gsid_per_patch [P] int32"""
    ranges = np.zeros((T, 2), np.int32)
    at = 0
    for t, l in enumerate(lists):
        if len(l):
            ranges[t] = (at, at + len(l))
        at += len(l)
    return ranges, (np.concatenate(lists) if at else np.zeros(0)).astype(np.int32)


def _fma(a, b, c):
    """fmaf(a, b, c): the product of two float32 is exact in float64, the sum is rounded once more on the way back"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def poly_exponent(qxx, qxy, qyy, ux, uy, la, tx, ty, fma=False):
    """log2 alpha' of the 16 x 16 pixels of tile (tx, ty) as k_draw forms it, in float32 with the kernel's operation
    order: the polynomial about the TILE CENTRE with per-lane constant monomials,
        e = c0 + c1 X + c2 Y + qxx XX + qxy XY + qyy YY,   c0 = log2(alpha) + E(D), (c1, c2) = grad E(D).
    Inputs broadcast against a trailing [16 (y), 16 (x)]; q* = the record's pre-scaled conic, la = log2(alpha).
    ``fma``: the five steps per pixel as the fmaf calls the kernel's source spells out (one rounding each, where NumPy
    rounds the product and the sum), and the coefficients with the sums of products contracted the same way."""
    l16 = np.arange(16, dtype=f32)
    cx0, cy0 = (tx * 16).astype(f32) + f32(7.5), (ty * 16).astype(f32) + f32(7.5)
    Dx, Dy = (cx0 - ux).astype(f32), (cy0 - uy).astype(f32)
    X = (l16 - f32(7.5))[None, None, :]; Y = (l16 - f32(7.5))[None, :, None]
    if fma:
        c0 = (la + _fma((qyy * Dy).astype(f32), Dy, _fma((qxy * Dx).astype(f32), Dy, ((qxx * Dx).astype(f32) * Dx).astype(f32)))).astype(f32)
        c1 = _fma((f32(2) * qxx).astype(f32), Dx, (qxy * Dy).astype(f32)); c2 = _fma((f32(2) * qyy).astype(f32), Dy, (qxy * Dx).astype(f32))
        e = _fma(c2, Y, c0); e = _fma(c1, X, e); e = _fma(qyy, (Y * Y).astype(f32), e)
        e = _fma(qxy, (X * Y).astype(f32), e)
        return _fma(qxx, (X * X).astype(f32), e)
    c0 = (la + (qxx * Dx * Dx + qxy * Dx * Dy + qyy * Dy * Dy)).astype(f32)
    c1 = (f32(2) * qxx * Dx + qxy * Dy).astype(f32); c2 = (f32(2) * qyy * Dy + qxy * Dx).astype(f32)
    e = (c2 * Y + c0).astype(f32); e = (c1 * X + e).astype(f32); e = (qyy * (Y * Y).astype(f32) + e).astype(f32)
    e = (qxy * (X * Y).astype(f32) + e).astype(f32)
    return (qxx * (X * X).astype(f32) + e).astype(f32)


def blend(arrays, lists, policy, dtype=np.float64, poly=False, diag=None, hw=None, fma=False, extras=None):
    """``O.draw`` restated tile by tile (tests/test_draw_tile_ref_cpu.py pins it to ``O.draw`` bit for bit) with two
    additions.  ``poly``: float32, alpha' = exp2(e) of ``poly_exponent`` capped as k_draw caps it (min(e, log2 alpha)
    where the floor applies, log2 0.99 where the clamp does), the skip test in the exponent domain, tau -= tau alpha'.
    ``fma``: ``poly_exponent(fma=True)``.  ``hw`` (with ``poly``; 1, -1 or 0 = a random sign per use): the two one-ulp
    operations of k_draw that NumPy rounds correctly, each moved by its ulp in that direction -- the derived log2(alpha)
    and the exponential (v_exp_f32).  ``diag``: a dict
    that receives, per Gaussian, hits / clamped / floored pixel counts, the smallest relative distance of a live alpha'
    from alpha_skip and of a post-blend tau from tau_stop.  -> image, contrib, final_tau
    ``extras``: the background [3]; z is ``arrays["z"]`` -> image over the background, contrib, final_tau, depth, alpha.  In
    float64 (no ``poly``) in the way of the oracle's composition -- ``O.draw`` on the colours (z, 1, 0), then image +
    (1 - alpha) bg; tests/test_draw_tile_ref_cpu.py pins it bit for bit --, in float32 in k_draw's own way: cd += w z
    (``fma``: contracted), alpha = 1 - tau, image = fmaf(tau, bg, c), an empty tile the background itself."""
    kway = extras is not None and (poly or dtype != np.float64)
    if extras is not None:
        zs = np.asarray(arrays["z"], dtype); bgv = np.asarray(extras, dtype)
        depth = np.zeros((H, W), dtype); alpha = np.zeros((H, W), dtype)
    us = np.asarray(arrays["us"], dtype); cinv = np.asarray(arrays["cinv2ds"], dtype)
    alphas = np.asarray(arrays["alphas"], dtype).reshape(-1); colors = np.asarray(arrays["colors"], dtype)
    n = us.shape[0]
    image = np.zeros((3, H, W), dtype); contrib = np.zeros((H, W), np.int32); final_tau = np.zeros((H, W), dtype)
    if policy.footprint == O.FOOT_BOX:
        bx0, bx1, by0, by1 = O.pixel_box(us, arrays["areas"], W, H)
    if diag is not None:
        diag.update(hits=np.zeros(n, np.int64), clamped=np.zeros(n, np.int64), floored=np.zeros(n, np.int64),
                    skip_dist=np.full(n, np.inf), stop_dist=np.full(n, np.inf))
    for t, ids in enumerate(lists):
        if len(ids) == 0:
            continue
        tx, ty, x0, y0, ww, hh = geom(t)
        py, px = np.meshgrid(np.arange(y0, y0 + hh, dtype=dtype), np.arange(x0, x0 + ww, dtype=dtype), indexing="ij")
        tau = np.ones((hh, ww), dtype); col = np.zeros((3, hh, ww), dtype)
        cont = np.zeros((hh, ww), np.int32); done = np.zeros((hh, ww), bool)
        cd = np.zeros((hh, ww), dtype); ca = np.zeros((hh, ww), dtype)
        for k, g in enumerate(ids):
            if done.all():
                break
            g = int(g)
            if poly:
                q = (NHL2E * cinv[g, 0]).astype(f32), (f32(2) * NHL2E * cinv[g, 1]).astype(f32), (NHL2E * cinv[g, 2]).astype(f32)
                with np.errstate(all="ignore"):
                    lskip = f32(np.log2(policy.alpha_skip)) if policy.alpha_skip > 0 else f32(-np.inf)
                    # log2(alpha) as the kernel derives it from the record's threshold (test_exponent_polynomial.py)
                    la = (lskip - np.log2(f32(policy.alpha_skip) / alphas[g]).astype(f32)).astype(f32) \
                        if policy.alpha_skip > 0 else np.log2(alphas[g]).astype(f32)
                    if hw is not None:
                        sg = f32(hw) if hw else (f32(1) if S.uniform01(4243, 1000 * t + k, (1,))[0] < 0.5 else f32(-1))
                        # log2(alpha) is not read but DERIVED, lskip - thr, from the record's threshold thr =
                        # log2f(alpha_skip / alpha): one ulp of v_log_f32 at |thr| (9.5e-7 for alpha ~ 1, where the
                        # difference is ~0) and the rounding of the quotient, 2^-24 log2(e)
                        thr = np.log2(f32(policy.alpha_skip) / alphas[g]) if policy.alpha_skip > 0 else la
                        dla = f32(2.0 ** -23 * abs(float(thr)) + 2.0 ** -24 * 1.4427)
                        la = (la + sg * dla).astype(f32)          # (one value per entry: the staging lane's)
                    e = poly_exponent(*[np.reshape(v, (1, 1, 1)) for v in q + (us[g, 0], us[g, 1], la)],
                                      np.array(tx), np.array(ty), fma=fma)[0, :hh, :ww]
                    cap = f32(np.inf)
                    if policy.maha_floor:
                        cap = la
                    if policy.alpha_clamp:
                        cap = min(cap, np.log2(f32(0.99)))
                    ap = np.exp2(np.minimum(e, cap)).astype(f32)
                    if hw is not None:
                        ap = _ulp(ap, hw, 250000 + 1000 * t + k)
                    # (alpha < alpha_skip never blends: the record's threshold is +inf, egs_gaussian_math.h make_record)
                    skip = ((e < lskip) | (alphas[g] < f32(policy.alpha_skip))) if policy.alpha_skip > 0 \
                        else np.zeros_like(done)
            else:
                ap, gg, dx, dy = O._alpha_prime(alphas[g], cinv[g], us[g], px, py, policy, dtype)
                skip = ap < dtype(policy.alpha_skip) if policy.alpha_skip > 0 else np.zeros_like(done)
            act = ~done
            if policy.footprint == O.FOOT_BOX:
                act = act & (px >= bx0[g]) & (px < bx1[g]) & (py >= by0[g]) & (py < by1[g])
            live = act
            act = act & ~skip
            w = np.where(act, tau * ap, 0)
            col += w[None] * colors[g][:, None, None]
            if extras is not None:
                if kway:
                    cd = _fma(w, zs[g], cd) if fma else cd + w * zs[g]
                else:
                    cd += w * zs[g]; ca += w * dtype(1)
            cont = np.where(act, k + 1, cont)
            tau = np.where(act, (tau - w) if poly else tau * (1 - ap), tau)
            if policy.tau_stop > 0:
                done |= act & (tau < dtype(policy.tau_stop))
            if diag is not None and not poly:
                diag["hits"][g] = act.sum()
                if policy.alpha_clamp:
                    diag["clamped"][g] = (act & (alphas[g] * gg > dtype(0.99))).sum()
                if policy.maha_floor:
                    m = cinv[g, 0] * dx * dx + cinv[g, 2] * dy * dy + 2 * cinv[g, 1] * dx * dy
                    diag["floored"][g] = (act & (m < 0)).sum()
                if policy.alpha_skip > 0 and live.any():
                    diag["skip_dist"][g] = (np.abs(ap - policy.alpha_skip) / policy.alpha_skip)[live].min()
                if policy.tau_stop > 0 and act.any():
                    diag["stop_dist"][g] = (np.abs(tau - policy.tau_stop) / policy.tau_stop)[act].min()
        image[:, y0:y0 + hh, x0:x0 + ww] = col
        contrib[y0:y0 + hh, x0:x0 + ww] = cont
        final_tau[y0:y0 + hh, x0:x0 + ww] = tau
        if extras is not None:
            depth[y0:y0 + hh, x0:x0 + ww] = cd
            alpha[y0:y0 + hh, x0:x0 + ww] = (dtype(1) - tau) if kway else ca
            if kway:
                image[:, y0:y0 + hh, x0:x0 + ww] = np.stack([_fma(tau, bgv[ch], col[ch]) for ch in range(3)]).astype(dtype)
    if extras is None:
        return image, contrib, final_tau
    if kway:
        for t, ids in enumerate(lists):
            if len(ids) == 0:
                tx, ty, x0, y0, ww, hh = geom(t)
                image[:, y0:y0 + hh, x0:x0 + ww] = bgv[:, None, None]
    else:
        image = image + (1.0 - alpha)[None] * bgv[:, None, None]
    return image, contrib, final_tau, depth, alpha


def perturbed(arrays, j):
    """the four float tensors of the draw (and ``z`` of an extras case: sorted behind them, their streams stay) moved by
    one ulp (``pergaussian_ref.perturbed``); lists, areas and depths stay"""
    from tests.pergaussian_ref import perturbed as P
    out = dict(arrays)
    out.update(P({k: arrays[k] for k in ("us", "cinv2ds", "alphas", "colors", "z") if k in arrays}, j))
    return out


def _lists_of(arrays, lists, policy):
    """the lists of ``policy``: the intended ones under G; under A ``O.bin_tiles`` (pixel boxes; its far cull drops the
    Gaussians whose centre lies outside 1.3 x the image)"""
    if policy is O.POLICY_G:
        return lists
    r, g, _, _ = O.bin_tiles(arrays["us"], arrays["areas"].copy(), arrays["depths"].copy(), W, H, policy)
    return [g[r[t, 0]:r[t, 1]] for t in range(T)]


def _violators(arrays, lists):
    """Gaussians that break one of the builder's conditions -> (set of ids, contrib of the float64 blend per policy)"""
    bad = set()
    for pol in POLICIES.values():
        ls = _lists_of(arrays, lists, pol)
        rg, gs = lists_to_arrays(ls)
        d = {}
        c64 = blend(arrays, ls, pol, np.float64, diag=d)[1]
        if pol.alpha_skip > 0:
            bad |= set(np.nonzero(d["skip_dist"] < SKIP_MARGIN)[0].tolist())
        if pol.tau_stop > 0:
            bad |= set(np.nonzero(d["stop_dist"] < STOP_MARGIN)[0].tolist())
        for j in range(N_PERT + 1):
            a = arrays if j == 0 else perturbed(arrays, j)
            c = O.draw(W, H, rg, gs, a["us"], a["cinv2ds"], a["alphas"], a["colors"], a["areas"], pol, np.float32)[1]
            for y, x in zip(*np.nonzero(c != c64)):        # the entry either evaluation stopped at or took last
                l = ls[(y // 16) * GX + x // 16]
                bad |= {int(l[k - 1]) for k in (int(c[y, x]), int(c64[y, x])) if k > 0}
    return bad


def _normalised(f):
    """``f(name, [pname,] seed=0, extras=False)`` cached on its full argument tuple, however the caller spelt it"""
    cached = functools.lru_cache(maxsize=None)(f)
    npos = f.__code__.co_argcount - 2

    @functools.wraps(f)
    def g(*args, seed=0, extras=False):
        args = args + (seed, extras)[len(args) - npos:] if len(args) < npos + 2 else args
        return cached(*args[:npos], int(args[npos]), bool(args[npos + 1]))
    g.__wrapped__ = f
    return g


@_normalised
def case(name, seed=0, extras=None):
    """-> Case of set ``name``: ``arrays`` (us, cinv2ds, alphas, colors, depths, areas, dloss_dgammas; read-only),
    ``lists`` (intended Gaussian ids per tile, policy G), ``tile_of`` / ``pos_of`` per Gaussian, ``scenarios``,
    ``redrawn`` (how many Gaussians were drawn again) -- a pure function of its arguments.
    ``extras`` true: the same Case object's arrays (nothing is re-drawn) plus ``z`` [N], ``dloss_ddepth`` and
    ``dloss_dalpha`` [H, W]; ``bg`` = float32(BG), ``extras`` = True."""
    if extras:
        return _with_extras(case(name, seed))
    n = sum(len(s["entries"]) for s in _scenarios(name))
    retry = np.zeros(n, np.int64)
    for _ in range(MAX_ROUNDS):
        arrays, lists, tile_of, pos_of, sc = _assemble(name, seed, retry)
        bad = _violators(arrays, lists)
        if not bad:
            break
        retry[sorted(bad)] += 1
    else:
        raise AssertionError("set %s: Gaussians %s still break a condition after %d re-draws" % (name, sorted(bad), MAX_ROUNDS))
    dl = S.normal(_seed_of(name, seed), 77, (3, H, W)) * 10.0 ** (-6.0 * S.uniform01(_seed_of(name, seed), 78, (3, H, W)))
    zt, zb = _zero_block(name)
    tx, ty, x0, y0, _, _ = geom(zt)
    dl[:, y0 + 8 * (zb >> 1):y0 + 8 * (zb >> 1) + 8, x0 + 8 * (zb & 1):x0 + 8 * (zb & 1) + 8] = 0.0
    arrays["dloss_dgammas"] = dl.astype(f32)
    for v in arrays.values():
        v.setflags(write=False)
    c = Case()
    c.name, c.seed, c.arrays, c.lists, c.tile_of, c.pos_of, c.scenarios = name, seed, arrays, lists, tile_of, pos_of, sc
    c.redrawn, c.retries, c.n = int((retry > 0).sum()), int(retry.sum()), n
    c.extras, c.bg = False, None
    return c


def _with_extras(base):
    """the Case ``base`` with what the render extras add, from counter streams of their own"""
    c = Case()
    c.__dict__.update(base.__dict__)
    s = _seed_of(base.name, base.seed)
    arrays = dict(base.arrays)
    arrays["z"] = (0.2 * 500.0 ** S.uniform01(s, 79, (base.n,))).astype(f32)
    zt, zb = _zero_block(base.name)
    tx, ty, x0, y0, _, _ = geom(zt)
    for key, stream in (("dloss_ddepth", 80), ("dloss_dalpha", 82)):
        w = S.normal(s, stream, (H, W)) * 10.0 ** (-6.0 * S.uniform01(s, stream + 1, (H, W)))
        w[y0 + 8 * (zb >> 1):y0 + 8 * (zb >> 1) + 8, x0 + 8 * (zb & 1):x0 + 8 * (zb & 1) + 8] = 0.0
        arrays[key] = w.astype(f32)
    for v in arrays.values():
        v.setflags(write=False)
    c.arrays, c.extras, c.bg = arrays, True, np.array(BG, f32)
    c.bg.setflags(write=False)
    return c


def lists(c, pname):
    """the lists of case ``c`` under policy ``pname`` -> (list of id arrays per tile, ranges, gsid)"""
    ls = _lists_of(c.arrays, c.lists, POLICIES[pname])
    return (ls,) + lists_to_arrays(ls)


# --------------------------------------------------------------------------------------------------------- reference
def forward(c, pname, dtype=np.float64, arrays=None):
    """image, contrib, final_tau of ``O.draw`` on the lists of the case; an extras case: image over the background,
    contrib, final_tau, depth, alpha by the composition of tests/test_gpu_render_extras.py::oracle -- ``O.draw`` on the
    colours (z, 1, 0), then image + (1 - alpha) bg"""
    a = c.arrays if arrays is None else arrays
    _, rg, gs = lists(c, pname)
    img, cont, tau = O.draw(W, H, rg, gs, a["us"], a["cinv2ds"], a["alphas"], a["colors"], a["areas"], POLICIES[pname],
                            dtype)
    if not c.extras:
        return img, cont, tau
    ez = O.draw(W, H, rg, gs, a["us"], a["cinv2ds"], a["alphas"], _zcolors(a["z"], dtype), a["areas"], POLICIES[pname],
                dtype)[0]
    return img + (1.0 - ez[1])[None] * np.asarray(c.bg, dtype)[:, None, None], cont, tau, ez[0], ez[1]


def _zcolors(z, dtype):
    z = np.asarray(z, dtype)
    return np.stack([z, np.ones_like(z), np.zeros_like(z)], 1)


def backward(c, pname, contrib, final_tau, dtype=np.float64, arrays=None):
    """dloss_dus [N,2], dloss_dcinv2ds [N,3], dloss_dalphas [N], dloss_dcolors [N,3] of ``O.draw_backward``; an extras
    case: the gradient of <Wi, image> + <Wd, depth> + <Wa, alpha> -- ``O.draw_backward`` on the real colours with Wi plus
    ``O.draw_backward`` on the colours (z, 1, 0) with (Wd, Wa - Wi . bg, 0) --, and dz [N], the first column of the second
    call's colour gradient"""
    a = c.arrays if arrays is None else arrays
    _, rg, gs = lists(c, pname)
    g1 = O.draw_backward(W, H, rg, gs, a["us"], a["cinv2ds"], a["alphas"], a["colors"], contrib, final_tau,
                         c.arrays["dloss_dgammas"], a["areas"], POLICIES[pname], dtype)
    if not c.extras:
        return g1
    Wi = np.asarray(c.arrays["dloss_dgammas"], dtype)
    Wd, Wa = np.asarray(c.arrays["dloss_ddepth"], dtype), np.asarray(c.arrays["dloss_dalpha"], dtype)
    dl2 = np.stack([Wd, Wa - (Wi * np.asarray(c.bg, dtype)[:, None, None]).sum(0), np.zeros_like(Wd)])
    g2 = O.draw_backward(W, H, rg, gs, a["us"], a["cinv2ds"], a["alphas"], _zcolors(a["z"], dtype), contrib, final_tau,
                         dl2, a["areas"], POLICIES[pname], dtype)
    return g1[0] + g2[0], g1[1] + g2[1], g1[2] + g2[2], g1[3], g2[3][:, 0].copy()


GRADS = ("dus", "dcinv2ds", "dalphas", "dcolors")
GRADS_X = GRADS + ("dz",)                                    # an extras case
HW_MODES = ((1, 1), (1, -1), (-1, 1), (-1, -1), (0, 0))      # (sign of the rcp ulp, sign of the exp ulp); 0: random


def _ulp(x, sign, key):
    """float32 ``x`` moved by one ulp: up (sign 1), down (-1), or either way by the counter generator's stream ``key``"""
    x = np.asarray(x, f32)
    up = np.full(x.shape, sign > 0) if sign else S.uniform01(4242, key, x.shape) < 0.5
    return np.where(up, np.nextafter(x, f32(np.inf)), np.nextafter(x, f32(-np.inf))).astype(f32)


def backward_hw(c, pname, contrib, final_tau, mode=None, arrays=None, abs_out=None):
    """``O.draw_backward`` restated in float32 (``mode`` None: bit for bit, tests/test_draw_tile_ref_cpu.py); with a
    ``mode`` the Gaussian is formed as k_draw_bwd forms it (pre-scaled conic, fmaf, exp2), gamma_cur2last is carried as
    the kernel's scalar lq, and the two operations it does NOT round correctly are an ulp off: it recovers the transmittance as tau * v_rcp_f32(1 - alpha') where
    NumPy divides (one correctly rounded operation), and takes the Gaussian from v_exp_f32 where NumPy's exp is
    correctly rounded to the last bit or so.  Both instructions are accurate to ONE ulp, in a direction nobody
    documents; ``mode`` = (sign of the reciprocal's ulp, sign of the exponential's ulp), 0 = a random sign per use.
    The same sign at every use is the systematic drift a 1-ulp instruction is entitled to: over a walk of 120 entries the
    recovered tau then leaves the float64 one by 120 ulps, which a cancelling dL/dalpha row magnifies.
    An extras case (-> the four tensors and dz [N]): without a ``mode`` the oracle's walk over the five colours (c, z, 1)
    with dL/dgamma = (Wi, Wd, Wa - Wi . bg); with one, k_draw_bwd<EXTRA>'s own operations: lq starts at Wi . bg - Wa,
    dq = fmaf(Wd, z, Wi . c) - lq, dz += Wd w.
    ``abs_out`` ([N, 2], added to): the sums of |t_x|, |t_y| whose signed sums are dus (tests/absgrad_ref.py)."""
    a = c.arrays if arrays is None else arrays
    policy = POLICIES[pname]
    ls, _, _ = lists(c, pname)
    us = np.asarray(a["us"], f32); cinv = np.asarray(a["cinv2ds"], f32)
    alphas = np.asarray(a["alphas"], f32).reshape(-1); colors = np.asarray(a["colors"], f32)
    dLdg = np.asarray(c.arrays["dloss_dgammas"], f32)
    n = us.shape[0]
    dus = np.zeros((n, 2), f32); dcinv = np.zeros((n, 3), f32); dalpha = np.zeros(n, f32); dcolor = np.zeros((n, 3), f32)
    x = c.extras
    if x:
        zs = np.asarray(a["z"], f32); bg = np.asarray(c.bg, f32); dz = np.zeros(n, f32)
        Wd, Wa = np.asarray(c.arrays["dloss_ddepth"], f32), np.asarray(c.arrays["dloss_dalpha"], f32)
    if policy.footprint == O.FOOT_BOX:
        bx0, bx1, by0, by1 = O.pixel_box(us, a["areas"], W, H)
    for t, ids in enumerate(ls):
        if len(ids) == 0:
            continue
        tx, ty, x0, y0, ww, hh = geom(t)
        py, px = np.meshgrid(np.arange(y0, y0 + hh, dtype=f32), np.arange(x0, x0 + ww, dtype=f32), indexing="ij")
        tau = np.array(final_tau[y0:y0 + hh, x0:x0 + ww], f32)
        cont = np.asarray(contrib[y0:y0 + hh, x0:x0 + ww])
        dl = dLdg[:, y0:y0 + hh, x0:x0 + ww]
        gcl = np.zeros((5 if x else 3, hh, ww), f32)
        lq = np.zeros((hh, ww), f32)
        dlx = dl
        if x:
            ld, la = Wd[y0:y0 + hh, x0:x0 + ww], Wa[y0:y0 + hh, x0:x0 + ww]
            dlx = np.concatenate([dl, ld[None], (la - (dl * bg[:, None, None]).sum(0))[None]]).astype(f32)
            lq = (((dl[0] * bg[0] + dl[1] * bg[1]).astype(f32) + dl[2] * bg[2]).astype(f32) - la).astype(f32)
        for k in range(int(cont.max()) - 1, -1, -1):
            g = int(ids[k])
            ap, gg, dx, dy = O._alpha_prime(alphas[g], cinv[g], us[g], px, py, policy, f32)
            if mode is not None:
                # the Gaussian as k_draw_bwd forms it: the record's pre-scaled conic, two products and two fmaf, exp2
                q0, q1, q2 = (NHL2E * cinv[g, 0]).astype(f32), (f32(2) * NHL2E * cinv[g, 1]).astype(f32), (NHL2E * cinv[g, 2]).astype(f32)
                with np.errstate(all="ignore"):
                    pw = ((q0 * dx).astype(f32))
                    pw = (_fma(q1, dy, pw) * dx).astype(f32)
                    pw = _fma((q2 * dy).astype(f32), dy, pw)
                    gg = np.exp2(np.minimum(pw, f32(0)) if policy.maha_floor else pw).astype(f32)
                gg = _ulp(gg, mode[1], 1000 * t + k)
                ap = alphas[g] * gg
                if policy.alpha_clamp:
                    ap = np.minimum(ap, f32(0.99))
            act = k < cont
            if policy.footprint == O.FOOT_BOX:
                act &= (px >= bx0[g]) & (px < bx1[g]) & (py >= by0[g]) & (py < by1[g])
            if policy.alpha_skip > 0:
                act &= ~(ap < f32(policy.alpha_skip))
            if not act.any():
                continue
            with np.errstate(all="ignore"):
                if mode is None:
                    tau_n = np.where(act, tau / (1 - ap), tau)
                else:
                    tau_n = np.where(act, tau * _ulp(f32(1) / (1 - ap), mode[0], 500000 + 1000 * t + k), tau)
            col = colors[g][:, None, None]
            colx = np.concatenate([colors[g], f32([zs[g], 1])])[:, None, None] if x else col
            if mode is None:
                dgam_dap = tau_n[None] * (colx - gcl)
                dl_dap = np.where(act, (dlx * dgam_dap).sum(0), 0)
            else:
                # k_draw_bwd carries gamma_cur2last as ONE scalar, lq = dL/dgamma . gamma_cur2last: dq = dL/dgamma . c - lq
                # is a difference of two rounded dot products, where the oracle subtracts the colours first
                dq = _fma(dl[2], col[2], _fma(dl[1], col[1], (dl[0] * col[0]).astype(f32)))
                if x:
                    dq = _fma(ld, zs[g], dq)
                dq = (dq - lq).astype(f32)
                dl_dap = np.where(act, tau_n * dq, 0).astype(f32)
                lq = np.where(act, _fma(ap, dq, lq), lq)
            dalpha[g] += (dl_dap * gg).sum()
            dcolor[g] += (np.where(act, ap * tau_n, 0)[None] * dl).sum((1, 2))
            if x:
                dz[g] += (np.where(act, ap * tau_n, 0) * ld).sum()
            ci = cinv[g]
            t_x, t_y = dl_dap * (-ci[0] * dx - ci[1] * dy) * ap, dl_dap * (-ci[1] * dx - ci[2] * dy) * ap
            dus[g, 0] += t_x.sum()
            dus[g, 1] += t_y.sum()
            if abs_out is not None:
                abs_out[g, 0] += np.abs(t_x).sum(); abs_out[g, 1] += np.abs(t_y).sum()
            dcinv[g, 0] += (dl_dap * (-0.5 * ap * dx * dx)).sum()
            dcinv[g, 1] += (dl_dap * (-1.0 * ap * dx * dy)).sum()
            dcinv[g, 2] += (dl_dap * (-0.5 * ap * dy * dy)).sum()
            gcl = np.where(act[None], ap[None] * colx + (1 - ap)[None] * gcl, gcl)
            tau = tau_n
    return (dus, dcinv, dalpha, dcolor, dz) if x else (dus, dcinv, dalpha, dcolor)


@_normalised
def reference(name, pname, seed=0, extras=False):
    """the float64 result of set ``name`` under policy ``pname``, computed once -> dict: image, contrib, final_tau, the
    four gradient tensors (GRADS), ``diag`` (per-Gaussian hits / clamped / floored counts), ``walked`` [N] (entries
    between a Gaussian's own and the largest contrib of its tile); without ``extras`` also ``dus_abs`` [N, 2], the absolute
    screen-space gradient (tests/absgrad_ref.py); with ``extras`` the image over the background, ``depth``, ``alpha`` and
    the five tensors GRADS_X (``dz`` [N])"""
    c = case(name, seed, True if extras else None)
    ls, rg, gs = lists(c, pname)
    fwd = forward(c, pname)
    image, contrib, tau = fwd[:3]
    out = dict(image=image, contrib=contrib, final_tau=tau)
    out.update(zip(GRADS_X, backward(c, pname, contrib, tau)))
    if extras:
        out.update(depth=fwd[3], alpha=fwd[4])
    else:
        from tests.absgrad_ref import draw_backward_abs
        a = c.arrays
        out["dus_abs"] = draw_backward_abs(W, H, rg, gs, a["us"], a["cinv2ds"], a["alphas"], a["colors"], contrib, tau,
                                           a["dloss_dgammas"], a["areas"], POLICIES[pname])[1]
    d = {}
    blend(c.arrays, ls, POLICIES[pname], np.float64, diag=d)
    out["diag"] = d
    walked = np.zeros(c.n)
    for t, l in enumerate(ls):
        tx, ty, x0, y0, ww, hh = geom(t)
        if len(l):
            walked[l] = np.maximum(0, int(contrib[y0:y0 + hh, x0:x0 + ww].max()) - np.arange(len(l)))
    out["walked"] = walked
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def _rows(got, ref):
    """per row: max_j |got - ref| / max_j |ref| (0 where the row's reference is 0)"""
    got = np.asarray(got, np.float64).reshape(len(ref), -1); ref = np.asarray(ref, np.float64).reshape(len(ref), -1)
    scale = np.abs(ref).max(1)
    return np.where(scale == 0, 0.0, np.abs(got - ref).max(1) / np.where(scale == 0, 1.0, scale))


@_normalised
def distances(name, pname, seed=0, extras=False):
    """How far the number format and the kernels' legitimate operations move the result, without any kernel -> dict:
    per PIXEL for image (largest of the three channels) and final_tau the largest absolute distance from the float64
    reference of
      (a) the float32 ``O.draw``,
      (b) N_PERT float32 evaluations of the inputs moved by one ulp,
      (c) the float32 blend whose exponent is k_draw's polynomial about the tile centre (``blend(poly=True)``), restated
          operation by operation: with NumPy's two roundings per step and with the kernel's fmaf;
    per Gaussian ROW and gradient tensor the largest relative distance (of max_j |ref row|), under ``<tensor>_alone``, of
      (a), (b) the float32 ``O.draw_backward`` fed its own float32 forward,
      (d) the float32 backward with the reciprocal and the exponential one ulp off as the hardware's are
          (``backward_hw``, HW_MODES)
    -- what bounds k_draw_bwd fed the reference's contrib / final_tau -- and under ``<tensor>`` of those and
      (e) that backward fed the contrib / final_tau of the forwards (c), as restated and with k_draw's two one-ulp
          operations (derived log2(alpha), v_exp_f32) an ulp off: k_draw_bwd forms alpha' directly, k_draw by the
          polynomial, so the transmittance the backward divides its way up from belongs to slightly different alpha' --
          a difference that 1 / (1 - alpha') magnifies 100-fold next to the clamp (forward and backward signs opposed)
    -- what bounds the pair.  ``contrib_equal``: every one of these evaluations gave the reference's contrib.
    Without ``extras`` also the rows ``dus_abs`` (and ``dus_abs_alone``) of the absolute screen-space gradient, from the
    same float32 walks ((a), (b) are then ``backward_hw`` without a mode, which IS the float32 ``O.draw_backward``).
    With ``extras`` (an extras case; z is moved by its ulp in (b) too) also ``depth`` and ``alpha`` per pixel and the rows
    ``dz``: (a), (b) are the float32 compositions of ``forward`` / ``backward``, (c) - (e) carry the EXTRA kernels' own
    operations -- cd += w z with two roundings and contracted, alpha = 1 - tau, fmaf(tau, bg, c); fmaf(dL/ddepth, z, ..)."""
    c = case(name, seed, True if extras else None)
    ref = reference(name, pname, seed, extras)
    ls, rg, gs = lists(c, pname)
    pix = ("image", "final_tau") + (("depth", "alpha") if extras else ())
    keys = GRADS_X if extras else GRADS + ("dus_abs",)
    d = dict(contrib_equal=True)
    d.update({k: np.zeros((H, W)) for k in pix})
    d.update({k: np.zeros(c.n) for k in keys})
    bg = c.bg if extras else None

    def take(img, cont, tau, depth=None, alpha=None):
        d["contrib_equal"] &= bool(np.array_equal(cont, ref["contrib"]))
        d["image"] = np.maximum(d["image"], np.abs(img.astype(np.float64) - ref["image"]).max(0))
        for k, v in (("final_tau", tau), ("depth", depth), ("alpha", alpha)):
            if v is not None:
                d[k] = np.maximum(d[k], np.abs(v.astype(np.float64) - ref[k]))

    def rows(grads):
        for k, g in zip(keys, grads):
            d[k] = np.maximum(d[k], _rows(g, ref[k]))

    def hw_rows(cont, tau, mode, arrays=None):
        ab = None if extras else np.zeros((c.n, 2), f32)
        rows(backward_hw(c, pname, cont, tau, mode, arrays, abs_out=ab) + (() if extras else (ab,)))

    for j in range(N_PERT + 1):                                                                     # (a), (b)
        a = c.arrays if j == 0 else perturbed(c.arrays, j)
        fwd = forward(c, pname, np.float32, a)
        take(*fwd)
        cont, tau = fwd[1], fwd[2]
        if extras:
            rows(backward(c, pname, cont, tau, np.float32, a))
        else:
            hw_rows(cont, tau, None, a)
        if j == 0:                                                                                  # (d)
            for mode in HW_MODES:
                hw_rows(cont, tau, mode)
    d.update({k + "_alone": d[k].copy() for k in keys})
    for fma in (False, True):                                                                       # (c)
        fwd = blend(c.arrays, ls, POLICIES[pname], np.float32, poly=True, fma=fma, extras=bg)
        take(*fwd)
        hw_rows(fwd[1], fwd[2], (0, 0))
    for hw, modes in ((0, ((0, 0),)), (1, ((1, -1), (-1, -1))), (-1, ((1, 1), (-1, 1)))):             # (e)
        fwd = blend(c.arrays, ls, POLICIES[pname], np.float32, poly=True, hw=hw, fma=True, extras=bg)
        d["contrib_equal"] &= bool(np.array_equal(fwd[1], ref["contrib"]))
        for mode in modes:
            hw_rows(fwd[1], fwd[2], mode)
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def pixel_floor(name, pname, seed=0, extras=False):
    """one float32 ulp of a pixel's largest running magnitude per blended entry: 2^-23 (2 + contrib) max(1, max |colour|
    of the tile's list) -- a count of the roundings of the accumulation, not a measurement.  ``extras``: -> dict, the same
    form per output: image with the background's magnitude among the colours', final_tau as without extras, depth with
    max(1, max |z| of the tile's list), alpha with 1"""
    c = case(name, seed, True if extras else None)
    ref = reference(name, pname, seed, extras)
    cmax = np.ones((H, W)); zmax = np.ones((H, W))
    for t, l in enumerate(lists(c, pname)[0]):
        tx, ty, x0, y0, ww, hh = geom(t)
        if len(l):
            cmax[y0:y0 + hh, x0:x0 + ww] = max(1.0, float(np.abs(c.arrays["colors"][l]).max()))
            if extras:
                zmax[y0:y0 + hh, x0:x0 + ww] = max(1.0, float(np.abs(c.arrays["z"][l]).max()))
    one = 2.0 ** -23 * (2 + ref["contrib"])
    if not extras:
        return one * cmax
    return dict(image=one * np.maximum(cmax, float(np.abs(c.bg).max())), final_tau=one * cmax, depth=one * zmax, alpha=one)


# ------------------------------------------------------------------------------------------------------------ claims
def block_max(contrib, t):
    """largest contrib of the four 8x8 blocks of tile ``t`` (None where the block lies outside the image)"""
    tx, ty, x0, y0, ww, hh = geom(t)
    out = []
    for b in range(4):
        xs, ys = x0 + 8 * (b & 1), y0 + 8 * (b >> 1)
        out.append(int(contrib[ys:ys + 8, xs:xs + 8].max()) if (xs < W and ys < H) else None)
    return out


def check_claims(name, seed=0):
    """every scenario of the set is what it says, on the float64 blend under policy G"""
    c = case(name, seed)
    ref = reference(name, "gsplatcu", seed)
    d = ref["diag"]
    for t, s in enumerate(c.scenarios):
        tx, ty, x0, y0, ww, hh = geom(t)
        l = c.lists[t]
        cont = ref["contrib"][y0:y0 + hh, x0:x0 + ww]
        if "contrib" in s:
            assert (cont == s["contrib"]).all(), (name, t, "contrib", np.unique(cont), s["contrib"])
        if "bmax" in s:
            assert block_max(ref["contrib"], t) == list(s["bmax"]), (name, t, block_max(ref["contrib"], t), s["bmax"])
        if "hitting" in s:
            assert int((d["hits"][l] > 0).sum()) == s["hitting"], (name, t, d["hits"][l])
        for pos, (code, g) in enumerate(zip(s["codes"], l)):
            h = int(d["hits"][g])
            ok = {"A": h == ww * hh, "S": 0 < h < ww * hh, "N": h == 0, "I": h == 0, "*": True}[code]
            assert ok, (name, t, pos, s["entries"][pos], code, h)
        for pos in s.get("partial", ()):
            g, (kind, _) = l[pos], s["entries"][pos]
            cnt = int(d["clamped" if kind == "clamp" else "floored"][g])
            assert 0 < cnt < int(d["hits"][g]), (name, t, pos, kind, cnt, int(d["hits"][g]))
        if len(l) == 0:
            assert (ref["image"][:, y0:y0 + hh, x0:x0 + ww] == 0).all() and (cont == 0).all() \
                and (ref["final_tau"][y0:y0 + hh, x0:x0 + ww] == 0).all()


def report(name, seed=0):
    """what the builder made of set ``name``: one line per policy"""
    c = case(name, seed)
    lines = ["set %s: %d Gaussians, %d re-drawn (%d re-draws)" % (name, c.n, c.redrawn, c.retries)]
    for pname in POLICIES:
        ref = reference(name, pname, seed)
        ls = lists(c, pname)[0]
        d = ref["diag"]
        lines.append("  %-11s lengths %s" % (pname, [len(l) for l in ls]))
        lines.append("  %-11s per-block largest contrib %s" % ("", [block_max(ref["contrib"], t) for t in range(T)]))
        lines.append("  %-11s entries that hit %d of %d, hit pixels %d, clamped %d, floored %d"
                     % ("", int((d["hits"] > 0).sum()), sum(len(l) for l in ls), int(d["hits"].sum()),
                        int(d["clamped"].sum()), int(d["floored"].sum())))
    return "\n".join(lines)
