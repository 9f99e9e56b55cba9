"""Float64 reference of the footprint cull (csrc/egs_gaussian_math.h foot_*, the emission forms of k_bin_emit), written
from the DEFINITION of the footprint -- not a transcription of the device code -- and the hand-built cases it is run on.

For a 2D Gaussian (u, conic c0 c1 c2, alpha), the skip threshold s = float32(0.002) and an 8x8 block of pixel centres
[X, X + 7] x [Y, Y + 7] two bounds bracket what the device may list:

  must   some integer pixel centre of the block has alpha exp(-maha / 2) >= s (1 + 1e-3): the block blends for certain
         (1e-3: the margin tests/test_gpu_parity.py check_culled_lists uses for the float32 device test);
  may    the ellipse maha <= m* = 2 ln(alpha / s) meets the rectangle [X - e, X + 7 + e] x [Y - e, Y + 7 + e].  The
         minimum of the convex quadratic over the rectangle is closed-form (``quad_min_rect``): 0 if the centre lies
         inside, else the best of the four edges, each a clamped 1D minimum.  e = 1.25 eps, eps = 0.05 + 0.01 max(x
         half-extent, y half-extent) the slack the code documents; the extra quarter is for float32 rounding of the slab
         extents (worst: the square root near tangency, ~1e-3 of the half-extent = 0.1 eps).  The device's clamp to its
         tile rect only shrinks its set.

Rules that make ``may`` everything or nothing (the device's, csrc/egs_gaussian_math.h make_binrec, in its order): a conic
the code refuses to cull (det <= 1e-4 c0 c2, c0 or c2 non-positive, alpha NaN) reaches every block of its rect; else
alpha < s never blends.  Per-tile masks: four bits, bit k = block (k & 1, k >> 1).  The reference list of a tile: the
Gaussians whose rect (``O.get_rects``) covers it, in (depth key, index) order (``O.depth_keys``).

A case is a small image plus 2D targets (centre, covariance INCLUDING the 0.3 I the device adds, opacity, depth); ``lift``
turns the targets into inputs of the fused path (identity camera, a flat Gaussian at depth Z facing the camera, rotated
about the optical axis).  The lift is not exact and need not be: the GPU tests compute all truth from the 2D Gaussians
the device reports; the CPU tests use ``project`` (the oracle's float64 stages on the lifted inputs).

Image sizes: the switches between the record forms are rects of 4 | 5 and 8 | 9 tiles, and a rect is clipped to the tile
grid, so the sets that need a 9-tile rect (or a big-walk Gaussian) live on 160 x 160 (10 x 10 tiles)."""
import numpy as np

from oracle import gs_oracle as O

SKIP = float(np.float32(0.002))     # the device's threshold (EgsPolicy.alpha_skip is a float)
MUST_MARGIN = 1e-3
SLACK = 1.25
REFUSE = 1e-4
TILE = 16
RADIUS_MARGIN = 2e-5                # tests/pergaussian_ref.py RADIUS_MARGIN
EDGE_MARGIN = 1e-3
FOCAL = 256.0
THIN = 1e-4                         # third scale of a lifted Gaussian, in pixels at its depth
SETS = ("forms", "tangent", "faint", "needles", "uncullable", "tall", "wide", "order")
CAPPED = ("forms", "tangent", "faint", "needles", "order")     # sets under the sharpness cap (0.20)


# ------------------------------------------------------------------------------------------------ the two bounds
def quad_min_rect(c0, c1, c2, ux, uy, xa, xb, ya, yb):
    """min over [xa, xb] x [ya, yb] of c0 dx^2 + 2 c1 dx dy + c2 dy^2, (dx, dy) = (x - ux, y - uy); convex conics"""
    ax, bx, ay, by = xa - ux, xb - ux, ya - uy, yb - uy
    q = lambda dx, dy: c0 * dx * dx + 2 * c1 * dx * dy + c2 * dy * dy
    ex = lambda dx: q(dx, np.clip(-c1 * dx / c2, ay, by))          # an edge x = const: the 1D minimum in y, clamped
    ey = lambda dy: q(np.clip(-c1 * dy / c0, ax, bx), dy)
    best = np.minimum(np.minimum(ex(ax), ex(bx)), np.minimum(ey(ay), ey(by)))
    inside = (ax <= 0) & (bx >= 0) & (ay <= 0) & (by >= 0)
    return np.where(inside, 0.0, best)


def classify(cinv, alpha, skip=SKIP):
    """-> ("all" | "never" | "cull", m*, eps)"""
    c0, c1, c2 = (float(v) for v in cinv)
    alpha = float(alpha)
    det = c0 * c2 - c1 * c1
    if not (det > REFUSE * c0 * c2 and c0 > 0 and c2 > 0) or alpha != alpha:
        return "all", np.inf, np.inf
    if alpha < skip:
        return "never", -1.0, 0.0
    m = 2 * np.log(alpha / skip)
    if not np.isfinite(m):
        return "all", np.inf, np.inf
    return "cull", m, 0.05 + 0.01 * np.sqrt(m * max(c2, c0) / det)


def _pack(blk):
    """bool [2h, 2w] blocks -> int [h, w] masks, bit k = block (k & 1, k >> 1)"""
    m = np.zeros((blk.shape[0] // 2, blk.shape[1] // 2), np.int64)
    for k in range(4):
        m |= blk[(k >> 1)::2, (k & 1)::2].astype(np.int64) << k
    return m


def gaussian_masks(u, cinv, alpha, rect, skip=SKIP):
    """(must, may) masks [h, w] over the tiles of ``rect`` = (x0, y0, x1, y1)"""
    x0, y0, x1, y1 = (int(v) for v in rect)
    ux, uy = float(u[0]), float(u[1])
    c0, c1, c2 = (float(v) for v in cinv)
    dx = ux - np.arange(TILE * x0, TILE * x1, dtype=np.float64)[None, :]
    dy = uy - np.arange(TILE * y0, TILE * y1, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        ap = float(alpha) * np.exp(-0.5 * np.maximum(c0 * dx * dx + c2 * dy * dy + 2 * c1 * dx * dy, 0))
        hit = ap >= skip * (1 + MUST_MARGIN)
    must = _pack(hit.reshape(2 * (y1 - y0), 8, 2 * (x1 - x0), 8).any((1, 3)))
    kind, m, eps = classify(cinv, alpha, skip)
    if kind != "cull":
        return must, np.full_like(must, 15 if kind == "all" else 0)
    e = SLACK * eps
    X = 8.0 * np.arange(2 * x0, 2 * x1)[None, :]
    Y = 8.0 * np.arange(2 * y0, 2 * y1)[:, None]
    return must, _pack(quad_min_rect(c0, c1, c2, ux, uy, X - e, X + 7 + e, Y - e, Y + 7 + e) <= m)


class Lists:
    """the reference lists of an image, entry by entry in (tile, depth key, index) order, with both bounds"""
    pass


def reference_lists(us, cinv2ds, alphas, areas, depths, width, height, skip=SKIP):
    """us / cinv2ds / alphas / areas / depths: the 2D Gaussians (float32 values); -> Lists"""
    us32 = np.ascontiguousarray(us, np.float32)
    d = np.array(depths, np.float32)
    a = np.array(areas, np.int32)
    L = Lists()
    L.width, L.height = width, height
    L.gx, L.gy = O.tile_grid(width, height)
    L.rects, L.counts = O.get_rects(us32, a, d, width, height, O.POLICY_G)
    L.rects = L.rects.astype(np.int64)
    L.keys = O.depth_keys(d, O.POLICY_G).astype(np.int64)
    L.us, L.cinv, L.alphas = np.asarray(us32, np.float64), np.asarray(cinv2ds, np.float64), np.asarray(alphas, np.float64)
    L.kind = np.array([classify(c, al, skip)[0] for c, al in zip(L.cinv, L.alphas)])
    t, g, mu, ma = [], [], [], []
    for i in np.nonzero(L.counts)[0]:
        x0, y0, x1, y1 = L.rects[i]
        must, may = gaussian_masks(L.us[i], L.cinv[i], L.alphas[i], L.rects[i], skip)
        ty, tx = np.meshgrid(np.arange(y0, y1), np.arange(x0, x1), indexing="ij")
        t.append((ty * L.gx + tx).ravel()); g.append(np.full(must.size, i, np.int64))
        mu.append(must.ravel()); ma.append(may.ravel())
    cat = lambda v: np.concatenate(v) if v else np.zeros(0, np.int64)
    t, g, mu, ma = cat(t), cat(g), cat(mu), cat(ma)
    o = np.lexsort((g, L.keys[g], t))
    L.tile, L.gsid, L.must, L.may = t[o], g[o], mu[o], ma[o]
    T = L.gx * L.gy
    L.ranges = np.stack([np.searchsorted(L.tile, np.arange(T), "left"), np.searchsorted(L.tile, np.arange(T), "right")], 1)
    return L


def popcount(m):
    m = np.asarray(m, np.int64)
    return int(sum(((m >> k) & 1).sum() for k in range(4)))


def describe(L, e):
    """entry ``e`` of the reference lists for a failure message: u, conic, alpha, tile and the two bounds"""
    g = int(L.gsid[e])
    ty, tx = divmod(int(L.tile[e]), L.gx)
    return ("Gaussian %d (%s) u=(%.9g, %.9g) conic=(%.9g, %.9g, %.9g) alpha=%.9g rect=%s tile=(x %d, y %d) must=%d may=%d"
            % (g, L.kind[g], L.us[g, 0], L.us[g, 1], L.cinv[g, 0], L.cinv[g, 1], L.cinv[g, 2], L.alphas[g],
               L.rects[g].tolist(), tx, ty, int(L.must[e]), int(L.may[e])))


def check_culled(L, ranges, ids, masks, what=""):
    """The device's culled lists (ranges [T, 2], ids [P], masks [P]) against the reference lists, EVERY tile and entry:
    an ordered subsequence; every entry with must != 0 present, none with may == 0; must <= mask <= may bitwise; tiles
    without a reference entry (or without a listed one) have range (0, 0).  -> dict of counts"""
    ranges, ids, masks = np.asarray(ranges, np.int64), np.asarray(ids, np.int64), np.asarray(masks, np.int64)
    T = L.gx * L.gy
    assert ranges.shape == (T, 2), (what, ranges.shape)
    lens = ranges[:, 1] - ranges[:, 0]
    assert (lens >= 0).all() and lens.sum() == ids.size == masks.size, (what, "the ranges do not cover the list", lens.sum(), ids.size)
    nz = lens > 0
    assert not ranges[~nz].any(), (what, "an empty tile whose range is not (0, 0)", np.nonzero(~nz & ranges.any(1))[0][:8])
    st = ranges[nz, 0]
    assert (st[0] == 0 if st.size else True) and np.array_equal(st[1:], ranges[nz, 1][:-1]), (what, "ranges do not tile the list")
    assert not nz[L.ranges[:, 1] == L.ranges[:, 0]].any(), (what, "a tile without a reference entry has a list")
    dev_tile = np.repeat(np.arange(T), lens)
    N = max(len(L.alphas), 1)
    ref_key = L.tile * N + L.gsid                                        # (inside a tile the entries are in depth order)
    order = np.argsort(ref_key, kind="stable")
    key = dev_tile * N + ids
    at = np.searchsorted(ref_key[order], key)
    ok = (at < ref_key.size) & (ref_key[order][np.minimum(at, ref_key.size - 1)] == key) if ref_key.size else np.zeros(key.size, bool)
    assert ok.all(), (what, "listed for a tile its rect does not cover (tile, Gaussian):",
                      [(int(dev_tile[i]), int(ids[i])) for i in np.nonzero(~ok)[0][:8]])
    where = order[at]
    assert (np.diff(where) > 0).all(), (what, "not an ordered subsequence of the reference list, first at device entry",
                                        int(np.nonzero(np.diff(where) <= 0)[0][0]) if where.size > 1 else -1)
    listed = np.zeros(L.gsid.size, bool)
    listed[where] = True
    dm = np.zeros(L.gsid.size, np.int64)
    dm[where] = masks
    bad = np.nonzero(~listed & (L.must != 0))[0]
    assert bad.size == 0, (what, "%d contributing entries were dropped; first: %s" % (bad.size, describe(L, bad[0]) if bad.size else ""))
    bad = np.nonzero(listed & (L.may == 0))[0]
    assert bad.size == 0, (what, "%d entries listed that `may` cannot reach; first: %s" % (bad.size, describe(L, bad[0]) if bad.size else ""))
    bad = np.nonzero(listed & ((L.must & ~dm) != 0))[0]
    assert bad.size == 0, (what, "%d masks miss a contributing block; first: device mask %d, %s"
                           % (bad.size, dm[bad[0]] if bad.size else 0, describe(L, bad[0]) if bad.size else ""))
    bad = np.nonzero(listed & ((dm & ~L.may) != 0))[0]
    assert bad.size == 0, (what, "%d masks exceed `may`; first: device mask %d, %s"
                           % (bad.size, dm[bad[0]] if bad.size else 0, describe(L, bad[0]) if bad.size else ""))
    never = np.nonzero(L.kind == "never")[0]
    assert not np.isin(ids, never).any(), (what, "a Gaussian that never blends is listed")
    full = np.isin(L.gsid, np.nonzero(L.kind == "all")[0])
    assert listed[full].all() and (dm[full] == 15).all(), (what, "an uncullable Gaussian misses a tile of its rect or a block")
    return dict(entries=int(L.gsid.size), dropped=int((~listed).sum()), must=popcount(L.must), device=popcount(dm),
                may=popcount(L.may))


def ambiguity(L):
    """share of (entry, block) pairs in ``may`` and not in ``must``"""
    return popcount(L.may & ~L.must) / max(4 * L.gsid.size, 1)


# --------------------------------------------------------------------------------------------------------- cases
class Case:
    """an image and its 2D targets; ``extra2d``: hand-written 2D Gaussians only the 2D-input route can be fed exactly"""

    def __init__(self, name, width, height):
        self.name, self.width, self.height = name, width, height
        self.u, self.cov, self.alpha, self.depth, self.tag = [], [], [], [], []
        self.extra2d = None

    def add(self, ux, uy, sxx, sxy, syy, alpha, depth=None, tag=""):
        assert min(sxx, syy) > 0.3 and (sxx - 0.3) * (syy - 0.3) > sxy * sxy, (self.name, sxx, sxy, syy)
        self.u.append((ux, uy)); self.cov.append((sxx, sxy, syy)); self.alpha.append(alpha)
        self.depth.append(depth); self.tag.append(tag)
        return len(self.u) - 1

    def ell(self, ux, uy, s_long, s_short, deg, alpha, depth=None, tag=""):
        """an ellipse of sigmas (s_long, s_short), the long axis ``deg`` degrees from +x"""
        c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
        a, b = s_long * s_long, s_short * s_short
        return self.add(ux, uy, a * c * c + b * s * s, (a - b) * s * c, a * s * s + b * c * c, alpha, depth, tag)

    def finish(self):
        """depths left open become 2 + 0.004 rank in order of addition (distinct mm keys); the clearances the builder
        guarantees are made to hold by growing an offending covariance by 0.3 % steps"""
        self.u = np.array(self.u, np.float64).reshape(-1, 2); self.cov = np.array(self.cov, np.float64).reshape(-1, 3)
        self.alpha = np.array(self.alpha, np.float64)
        self.depth = np.array([2.0 + 0.004 * i if d is None else d for i, d in enumerate(self.depth)], np.float64)
        for i in range(len(self.alpha)):
            if self.tag[i].startswith("fixed"):
                continue
            for _ in range(50):
                radius_ok, edge_ok = clear_of_edges(self.u[i], self.cov[i])
                if radius_ok and edge_ok:
                    break
                if not radius_ok:
                    self.cov[i] *= 1.003
                else:
                    self.u[i] += 0.037
        self.n = len(self.alpha)
        return self


def radii(cov):
    return 3 * np.sqrt(cov[0]), 3 * np.sqrt(cov[2])


def clear_of_edges(u, cov):
    """(no radius within 4 RADIUS_MARGIN (relative) of an integer, no rect edge (u +- r) / 16 within 2 EDGE_MARGIN of one)"""
    radius_ok = edge_ok = True
    for uu, r in zip(u, radii(cov)):
        radius_ok &= abs(r - round(r)) > RADIUS_MARGIN * max(r, 1.0) * 4
        for e in ((uu - np.ceil(r)) / TILE, (uu + np.ceil(r)) / TILE):
            edge_ok &= abs(e - round(e)) > EDGE_MARGIN * 2
    return radius_ok, edge_ok


def lift(case):
    """-> dict of float32 inputs of the fused path (pws, rots, scales, alphas, shs [n, 3]) + the camera numbers"""
    W, H = case.width, case.height
    cx, cy = W / 2.0, H / 2.0
    n = case.n
    Z = case.depth
    pws = np.stack([(case.u[:, 0] - cx) * Z / FOCAL, (case.u[:, 1] - cy) * Z / FOCAL, Z], 1)
    sxx, sxy, syy = case.cov[:, 0] - 0.3, case.cov[:, 1], case.cov[:, 2] - 0.3
    mean, half = 0.5 * (sxx + syy), np.hypot(0.5 * (sxx - syy), sxy)
    th = 0.5 * np.arctan2(2 * sxy, sxx - syy)
    k = np.abs(Z) / FOCAL
    scales = np.stack([np.sqrt(mean + half) * k, np.sqrt(np.maximum(mean - half, 1e-12)) * k, THIN * k], 1)
    rots = np.stack([np.cos(th / 2), np.zeros(n), np.zeros(n), np.sin(th / 2)], 1)
    rng = np.random.default_rng(len(case.name) + 7 * n)
    f = lambda a: np.ascontiguousarray(a, np.float32)
    return dict(pws=f(pws), rots=f(rots), scales=f(scales), alphas=f(case.alpha), shs=f(rng.uniform(0.3, 2.5, (n, 3))),
                width=W, height=H, fx=FOCAL, fy=FOCAL, cx=cx, cy=cy, Rcw=np.eye(3), tcw=np.zeros(3))


def project(inp, dtype=np.float64):
    """the oracle's per-Gaussian stages (policy G) on lifted inputs -> us, cinv2ds, areas, depths"""
    P = O.POLICY_G
    us, pcs, depths = O.project(inp["pws"], inp["Rcw"], inp["tcw"], inp["fx"], inp["fy"], inp["cx"], inp["cy"], P, False, dtype)[:3]
    c3 = O.compute_cov3d(inp["rots"], inp["scales"], depths, P, False, dtype)
    c2 = O.compute_cov2d(c3, pcs, inp["Rcw"], depths, inp["fx"], inp["fy"], inp["width"], inp["height"], P, False, dtype)
    depths = np.array(depths)
    cinv, areas = O.inverse_cov2d(c2, depths, P, False, dtype)
    return np.asarray(us, np.float64), np.asarray(cinv, np.float64), np.asarray(areas), np.asarray(depths, np.float64), \
        np.asarray(c2, np.float64)


# ---- building blocks
G10 = 160                                         # the 10 x 10-tile image
CENTRES = (79.5, 71.5, 83.3)                      # on a tile corner, on a block corner, mid-block (pixel centres: integers)
SIZES = (1, 4, 5, 8, 9)


def radius_for(u, w, tiles):
    """an integer radius r that gives a rect of exactly ``w`` tiles around centre ``u`` inside a grid of ``tiles``
    (the middle one of those that do), or None"""
    ok = []
    for r in range(2, 16 * tiles):
        x0, x1 = np.floor((u - r) / TILE), np.floor((u + r + TILE - 1) / TILE)
        if x0 >= 0 and x1 <= tiles and x1 - x0 == w:
            ok.append(r)
    return ok[len(ok) // 2] if ok else None


def var_of_radius(r):
    """a variance whose radius ceil(3 sigma) is r, half a pixel clear of the integers"""
    return ((r - 0.5) / 3.0) ** 2


def centre_and_radius(w, first):
    for j in range(3):
        u = CENTRES[(first + j) % 3]
        r = radius_for(u, w, G10 // TILE)
        if r is not None:
            return u, r
    raise AssertionError(w)


def rotated(sxx, syy, deg):
    """the covariance with these diagonal entries whose long axis lies ``deg`` degrees from +x, or None"""
    tot = sxx + syy
    c2 = np.cos(np.radians(2 * deg))
    if abs(c2) < 1e-9:
        if abs(sxx - syy) > 1e-9 * tot:
            return None
        d = 0.8 * (tot - 0.6)
    else:
        d = (sxx - syy) / c2
        if d < 0 or d > 0.9 * (tot - 0.6):
            return None
    return sxx, 0.5 * d * np.sin(np.radians(2 * deg)), syy


def build_forms():
    c = Case("forms", G10, G10)
    k = 0
    for w in SIZES:
        for h in SIZES:
            ux, rx = centre_and_radius(w, k)
            uy, ry = centre_and_radius(h, k // 3 + 1)
            sxx, syy = var_of_radius(rx), var_of_radius(ry)
            shapes = [(sxx, 0.0, syy)] + [s for s in (rotated(sxx, syy, a) for a in (30, 45, 60)) if s is not None]
            for j, (a, b, d) in enumerate(shapes):
                # well inside the rect (m* = 3.2 .. 6.4 < 9) in front, overflowing it (m* = 12.4) behind
                c.add(ux, uy, a, b, d, 0.01 + 0.04 * ((k + j) % 5) / 4.0, 2.0 + 0.004 * (8 * k + j), "fixed in %dx%d" % (w, h))
                c.add(ux, uy, a, b, d, 0.99, 6.0 + 0.004 * (8 * k + j), "fixed over %dx%d" % (w, h))
            k += 1
    # centres up to 12 px outside each border and corner
    v = var_of_radius(24)
    out = (-12.3, G10 - 1 + 11.7)
    spots = [(x, 80.2) for x in out] + [(80.2, y) for y in out] + [(x, y) for x in out for y in out] + [(-5.4, 40.7), (90.1, G10 + 3.3)]
    for j, (x, y) in enumerate(spots):
        c.add(x, y, v, 0.0 if j % 2 else 0.4 * v, v, 0.3 if j % 3 else 0.99, 9.0 + 0.004 * j, "fixed border")
    return c.finish()


def _clear_centre(j, r, base):
    """the j-th integer centre from ``base`` on whose rect edges c +- r are no multiple of the tile"""
    ok = [c for c in range(base, base + 40) if (c - r) % TILE and (c + r) % TILE]
    return float(ok[3 * j % len(ok)])


# (radius along the tangent axis, radius across, alpha): the footprint stays some 7 px long, so that half a pixel is 4 to
# 10 eps -- rects of at most 4 x 4 tiles (block bitmap), of 6 x 6 (tile bitmap) and clipped to 10 x 10 (row walk)
TANGENT_SHAPES = ((8, 6, 0.05), (5, 4, 0.05), (36, 40, 0.0023), (70, 65, 0.00209))


def build_tangent():
    """axis-aligned ellipses whose extreme point in +-x / +-y lies 0.5 px inside / outside a block and a tile boundary
    (4 to 10 eps at these sizes: must and may agree), in each form of the bin record"""
    c = Case("tangent", G10, G10)
    c.marks = []          # (target, axis, the pixel its extreme point faces, direction, reaches it)
    j = 0
    for r_long, r_other, alpha in TANGENT_SHAPES:
        m = 2 * np.log(alpha / SKIP)
        va, vb = var_of_radius(r_long), var_of_radius(r_other)
        ext = np.sqrt(m * va)
        for first in (88, 96):                    # first pixel beyond a block boundary inside a tile / a tile boundary
            for off in (0.5, -0.5):               # the extreme point past that pixel's centre / short of it
                for sign in (1, -1):
                    # +: the footprint sits on the low side and reaches up to pixel `first`; -: mirrored about it
                    edge = first if sign > 0 else first - 1
                    a = edge + sign * off - sign * ext
                    ix = c.add(a, _clear_centre(j, r_other, 70), va, 0.0, vb, alpha, None, "fixed x")
                    iy = c.add(_clear_centre(j, r_other, 60), a, vb, 0.0, va, alpha, None, "fixed y")
                    c.marks += [(ix, 0, edge, sign, off > 0), (iy, 1, edge, sign, off > 0)]
                    j += 1
    return c.finish()


def build_faint():
    c = Case("faint", G10, G10)
    for a in (0.0015, 0.002 * (1 + 2.0 ** -20), 0.0021, 0.0025):
        for w in (1, 5, 9):
            ux, rx = centre_and_radius(w, 0)
            uy, ry = centre_and_radius(w, 1)
            c.add(ux, uy, var_of_radius(rx), 0.0, var_of_radius(ry), a, None, "fixed")
    c.finish()
    # alpha exactly s with u exactly on a pixel centre and exactly between four: 2D values, exact only as given
    s32 = np.float32(0.002)
    c.extra2d = dict(us=np.array([[80.0, 80.0], [80.5, 80.5], [41.0, 99.0], [41.5, 99.5]], np.float32),
                     cinv2ds=np.array([[0.25, 0.0, 0.25], [0.25, 0.0, 0.25], [0.04, 0.01, 0.0625], [0.04, 0.01, 0.0625]], np.float32),
                     alphas=np.array([s32, s32, s32, s32], np.float32), areas=np.array([[6, 6], [6, 6], [17, 13], [17, 13]], np.int32),
                     depths=np.array([9.0, 9.1, 9.2, 9.3], np.float32))
    return c


def build_needles():
    c = Case("needles", 320, 208)
    rng = np.random.default_rng(11)
    j = 0
    for deg in (0, 30, 45, 60, 90, 120, 135, 150):
        for s_long in (10.0, 20.0, 30.0):
            for var_short in (0.35, 0.6, 1.0):
                c.ell(rng.uniform(20, 300), rng.uniform(20, 188), s_long, np.sqrt(var_short), deg,
                      (0.05, 0.3, 0.9)[j % 3], None, "needle")
                j += 1
    return c.finish()


def build_uncullable():
    c = Case("uncullable", G10, G10)
    for j, (s_long, deg) in enumerate(((150.0, 45), (200.0, 135), (250.0, 45), (200.0, 40))):
        c.ell(70.3 + 5 * j, 81.7 - 3 * j, s_long, np.sqrt(0.32), deg, 0.4, None, "refused")
    c.ell(50.2, 60.4, 6.0, 3.0, 20, float("nan"), None, "nan")
    rng = np.random.default_rng(5)
    for _ in range(12):
        c.ell(rng.uniform(0, G10), rng.uniform(0, G10), rng.uniform(2, 8), rng.uniform(1, 2), rng.uniform(0, 180),
              rng.uniform(0.05, 0.9), None, "plain")
    return c.finish()


def build_strip(name):
    """``tall`` 48 x 1088 (3 x 68 tiles) / ``wide`` 1088 x 48: elongated cullable Gaussians along the strip and at +-3
    degrees to it -- centred, at its end, beyond its end; one covers tile rows 0..67, others only the far end"""
    tall = name == "tall"
    c = Case(name, 48 if tall else 1088, 1088 if tall else 48)
    L = 1088
    along = 90 if tall else 0

    def put(pos, across, s_long, s_short, tilt, alpha, tag):
        x, y = (across, pos) if tall else (pos, across)
        c.ell(x, y, s_long, s_short, along + tilt, alpha, None, tag)
    put(544.3, 24.2, 400.0, 8.0, 0, 0.5, "all rows")                 # 3 sigma = 1200: every row of the strip
    put(544.3, 20.1, 450.0, 10.0, 3, 0.3, "all rows tilted")
    put(500.7, 28.3, 420.0, 9.0, -3, 0.3, "all rows tilted")
    put(1080.2, 24.4, 300.0, 25.0, 3, 0.2, "at the end")
    put(6.1, 22.0, 350.0, 15.0, -3, 0.2, "at the end")
    put(1088 + 900 - 120.5 + 0.3, 24.0, 300.0, 12.0, 0, 0.5, "rows 60..67")       # u - r = 967.8: tile row 60
    put(1088 + 900 - 280.5 + 0.3, 23.0, 300.0, 8.0, 3, 0.5, "rows 50..67")
    put(-700.2, 25.0, 330.0, 20.0, -3, 0.6, "beyond the start")
    rng = np.random.default_rng(3 if tall else 4)
    for _ in range(50):
        put(rng.uniform(0, L), rng.uniform(0, 48), rng.uniform(1.5, 5), rng.uniform(1, 1.5), rng.uniform(0, 180),
            rng.uniform(0.05, 0.9), "small")
    return c.finish()


BIG = dict(s_long=24.0, s_short=20.0, alpha=0.05)          # rect of 9 x 9 tiles or more, cullable: the wave walk


def build_order(n, variant=""):
    """n targets on 160 x 160 whose depths fix each one's place in the sorted order.  ``rank[i]``: place of target i.
    Never-listed at a CHOSEN place: alpha < s (an empty rect -- off screen, behind the near plane -- has depth key 0 and
    sorts to the front whatever its depth)."""
    c = Case("order_n%d%s" % (n, variant and "_" + variant), G10, G10)
    rng = np.random.default_rng(1000 + n + len(variant))
    perm = rng.permutation(n)                                # place -> target index
    never, big, offscreen = set(), set(), set()
    if variant == "":
        if n >= 255:
            at = {255: 0, 256: 100, 257: 216, 515: 256 + 216}[n]           # front, middle, end of a 256-block
            never = set(range(at, at + 40))
            if n == 255:
                offscreen = set(range(0, 40, 3))                           # key 0: they sort to the front by themselves
        if n == 515:
            big = {64 + 3, 64 + 20, 64 + 41, 255}                          # three in one wave, one in the last lane
    elif variant == "dead":
        never = set(range(256, 512))                                       # a workgroup whose span is empty
    levels = None
    if variant == "ties":
        levels = rng.integers(0, 5, n)                                     # a handful of depths: ties resolve by index
    tgt = [None] * n
    for place in range(n):
        i = int(perm[place])
        depth = 2.0 + 0.004 * place if levels is None else 2.0 + 0.5 * int(levels[i])
        x, y = rng.uniform(2, G10 - 2), rng.uniform(2, G10 - 2)
        if variant in ("p4", "p5") and place == 0:                         # one Gaussian over 2 / 3 tiles: P = n + 1, n + 2
            tgt[i] = ("ell", 83.3 if variant == "p4" else 87.7, 87.2, 3.2, 1.1, 0, 0.5, depth, "plain")
            continue
        if place in big:
            tgt[i] = ("ell", 80.3 + (place % 7), 78.6 - (place % 5), BIG["s_long"], BIG["s_short"], 25.0 * (place % 6), BIG["alpha"], depth, "big")
        elif place in offscreen:
            tgt[i] = ("ell", -300.0, -300.0, 3.0, 2.0, 0.0, 0.5, 0.1 if place % 2 else depth, "offscreen")
        elif place in never:
            tgt[i] = ("ell", x, y, rng.uniform(1.5, 6), rng.uniform(1, 1.5), rng.uniform(0, 180), 0.0015, depth, "never")
        else:
            s = 1.0 if n <= 3 else rng.uniform(1.5, 6)
            tgt[i] = ("ell", x if n > 3 else 20.3 + 32 * place, y if n > 3 else 24.6, s, 1.0 if n <= 3 else rng.uniform(1, 1.5),
                      rng.uniform(0, 180), rng.uniform(0.05, 0.9), depth, "plain")
    for t in tgt:
        c.ell(*t[1:])
    c.finish()
    c.places = dict(never=never - offscreen, big=big, offscreen=offscreen, perm=perm)
    return c


ORDER_CASES = tuple((n, "") for n in (1, 2, 3, 255, 256, 257, 515)) + ((3, "p4"), (3, "p5"), (515, "dead"), (515, "ties"))
_cache = {}


def cases(name):
    """the cases of a set (built once, never modified)"""
    if name not in _cache:
        if name == "order":
            _cache[name] = tuple(build_order(n, v) for n, v in ORDER_CASES)
        elif name in ("tall", "wide"):
            _cache[name] = (build_strip(name),)
        else:
            _cache[name] = (dict(forms=build_forms, tangent=build_tangent, faint=build_faint, needles=build_needles,
                                 uncullable=build_uncullable)[name](),)
    return _cache[name]


def all_cases():
    return [c for s in SETS for c in cases(s)]
