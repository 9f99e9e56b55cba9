"""The float64 footprint reference (tests/footprint_ref.py) and its hand-built cases, checked on the CPU: the closed-form
minimum against dense sampling, must within may, that every set realises the forms it was built for (counted from the
float64 rects of the oracle's stages on the lifted inputs), the sharpness of the two bounds, the clearances the builder
promises, and the list checker itself on lists made from the bounds.

Shares of (entry, block) pairs in ``may`` and not in ``must``, measured here: forms 0.018, tangent 0.002, faint 0.000,
needles 0.027, order 0.000 .. 0.018 (cap 0.20); exempt and printed: uncullable 0.820, tall 0.102, wide 0.100."""
import numpy as np
import pytest

from tests import footprint_ref as F
from tests.pergaussian_ref import RADIUS_MARGIN

_memo = {}


def lists_of(case):
    """(projected 2D Gaussians, reference lists) of a case, computed once"""
    if case.name not in _memo:
        inp = F.lift(case)
        us, cinv, areas, depths, cov = F.project(inp)
        f32 = lambda a: np.asarray(a, np.float32)
        L = F.reference_lists(f32(us), f32(cinv), inp["alphas"], areas, f32(depths), case.width, case.height)
        _memo[case.name] = (dict(us=us, cinv=cinv, areas=areas, depths=depths, cov=cov), L)
    return _memo[case.name]


def test_closed_form_minimum_equals_dense_sampling():
    rng = np.random.default_rng(0)
    n, k = 2000, 200
    s1, s2, th = rng.uniform(0.6, 30, n), rng.uniform(0.6, 30, n), rng.uniform(0, np.pi, n)
    a, b = 1 / (s1 * s1), 1 / (s2 * s2)
    c0, c1, c2 = a * np.cos(th) ** 2 + b * np.sin(th) ** 2, (a - b) * np.sin(th) * np.cos(th), a * np.sin(th) ** 2 + b * np.cos(th) ** 2
    ux, uy = rng.uniform(-25, 25, n), rng.uniform(-25, 25, n)
    xa, ya = rng.uniform(-35, 15, n), rng.uniform(-35, 15, n)
    xb, yb = xa + rng.uniform(0.1, 30, n), ya + rng.uniform(0.1, 30, n)
    closed = F.quad_min_rect(c0, c1, c2, ux, uy, xa, xb, ya, yb)
    t = np.linspace(0, 1, k)
    inside = 0
    for i in range(n):
        dx = (xa[i] + t * (xb[i] - xa[i]) - ux[i])[None, :]
        dy = (ya[i] + t * (yb[i] - ya[i]) - uy[i])[:, None]
        q = c0[i] * dx * dx + 2 * c1[i] * dx * dy + c2[i] * dy * dy
        # the sample nearest the minimiser is at most d away: q there <= q* + |grad q| d + lambda_max d^2 / 2, and the
        # gradient of a convex quadratic is largest at a corner of the rectangle
        d = 0.5 * np.hypot(xb[i] - xa[i], yb[i] - ya[i]) / (k - 1)
        gx, gy = 2 * (c0[i] * dx + c1[i] * dy), 2 * (c1[i] * dx + c2[i] * dy)
        g = np.hypot(gx, gy)[[0, 0, -1, -1], [0, -1, 0, -1]].max()
        step = g * d + 0.5 * (c0[i] + c2[i]) * d * d
        assert -1e-12 * (1 + q.min()) <= q.min() - closed[i] <= step, (i, q.min(), closed[i], step)
        inside += closed[i] == 0
    assert 100 < inside < 1900         # both branches taken


@pytest.mark.parametrize("name", F.SETS)
def test_must_within_may_and_sharpness(name):
    for case in F.cases(name):
        _, L = lists_of(case)
        bad = np.nonzero((L.must & ~L.may) != 0)[0]
        assert bad.size == 0, (case.name, F.describe(L, bad[0]) if bad.size else "")
        share = F.ambiguity(L)
        print("%s: %d entries, blocks must %d may %d, may-not-must share %.3f" % (case.name, L.gsid.size, F.popcount(L.must),
                                                                                 F.popcount(L.may), share))
        if name in F.CAPPED:
            assert share <= 0.20, (case.name, share)


def _wh(L):
    return (L.rects[:, 2] - L.rects[:, 0]), (L.rects[:, 3] - L.rects[:, 1])


def test_forms_set_realises_every_rect_size_in_both_variants():
    case, = F.cases("forms")
    p, L = lists_of(case)
    w, h = _wh(L)
    m = np.array([F.classify(c, a)[1] for c, a in zip(p["cinv"], case.alpha)])
    over = np.array([t.startswith("fixed over") for t in case.tag])
    inside = np.array([t.startswith("fixed in") for t in case.tag])
    for a in F.SIZES:
        for b in F.SIZES:
            for sel in (over, inside):
                assert ((w == a) & (h == b) & sel).any(), (a, b)
    assert (L.kind[over | inside] == "cull").all()
    assert (m[over] > 9).all() and (m[inside] < 9).all()           # footprint beyond / inside the 3-sigma rect
    assert set(case.tag[i].split()[-1] for i in np.nonzero(over)[0]) >= {"4x9", "9x4", "4x4", "5x5", "8x8", "9x9"}
    rotated = (np.abs(case.cov[:, 1]) > 0).sum()
    assert rotated >= 20 and (case.cov[:, 1] == 0).sum() >= 20
    border = np.array([t == "fixed border" for t in case.tag])
    assert border.sum() == 10 and (L.counts[border] > 0).all()
    out = (case.u[border] < 0) | (case.u[border] > F.G10 - 1)
    assert out.any(0).all() and out.all(1).sum() == 4                # every border, all four corners


def test_tangent_set_sits_half_a_pixel_either_side_of_its_boundary():
    case, = F.cases("tangent")
    p, L = lists_of(case)
    assert case.n == 64 and (L.kind == "cull").all()
    w, h = _wh(L)
    form = np.where((w <= 4) & (h <= 4), 0, np.where((w <= 8) & (h <= 8), 1, 2))
    seen = set()
    for i, ax, px, sign, reached in case.marks:
        ext = np.sqrt(2 * np.log(case.alpha[i] / F.SKIP) * case.cov[i, 2 * ax])
        extreme = case.u[i, ax] + sign * ext
        assert abs(sign * (extreme - px) - (0.5 if reached else -0.5)) < 1e-9, (i, extreme, px)
        other = int(round(case.u[i, 1 - ax]))
        assert other == case.u[i, 1 - ax]                  # the extreme point lies on a row / column of pixel centres
        bx, by = (px // 8, other // 8) if ax == 0 else (other // 8, px // 8)
        sel = np.nonzero((L.gsid == i) & (L.tile == (by // 2) * L.gx + bx // 2))[0]
        seen.add((int(form[i]), ax, px, reached))
        if sel.size == 0:                                  # the 3-sigma rect ends in front of the boundary
            assert not reached, (i, bx, by)
            continue
        bit = 1 << ((by & 1) * 2 + (bx & 1))
        assert bool(L.must[sel[0]] & bit) == reached and bool(L.may[sel[0]] & bit) == reached, (i, F.describe(L, sel[0]), reached)
    assert len(case.marks) == case.n
    # 3 record forms x 2 axes x (block | tile boundary from either side) x (inside | outside)
    assert len(seen) == 48, sorted(seen)
    eps = np.array([F.classify(c, a)[2] for c, a in zip(p["cinv"], case.alpha)])
    assert (0.5 / eps >= 4).all() and (0.5 / eps <= 10).all(), (0.5 / eps.max(), 0.5 / eps.min())


def test_faint_set():
    case, = F.cases("faint")
    p, L = lists_of(case)
    w, h = _wh(L)
    for a in np.unique(case.alpha):
        assert sorted(w[case.alpha == a]) == [1, 5, 9] and sorted(h[case.alpha == a]) == [1, 5, 9]
    assert (L.kind[case.alpha < 0.002] == "never").all() and (L.kind[case.alpha > 0.002] == "cull").all()
    assert np.float32(0.002 * (1 + 2.0 ** -20)) > np.float32(0.002)                   # survives the float32 input
    x = case.extra2d
    assert (x["alphas"] == np.float32(0.002)).all()
    Lx = F.reference_lists(x["us"], x["cinv2ds"], x["alphas"], x["areas"], x["depths"], case.width, case.height)
    assert (Lx.kind == "cull").all() and F.popcount(Lx.must) == 0
    assert [F.popcount(Lx.may[Lx.gsid == i]) for i in range(4)] == [1, 1, 1, 1]        # the block that holds u, m* = 0


def test_needles_and_uncullable_sets():
    case, = F.cases("needles")
    p, L = lists_of(case)
    assert (L.kind == "cull").all() and case.n == 72
    lam = np.linalg.eigvalsh(np.stack([case.cov[:, [0, 1]], case.cov[:, [1, 2]]], 1))
    assert (lam[:, 0] >= 0.35 - 1e-9).all() and (lam[:, 0] <= 1.02).all() and (lam[:, 1] >= 99).all() and (lam[:, 1] <= 930).all()
    case, = F.cases("uncullable")
    p, L = lists_of(case)
    tags = np.array(case.tag)
    assert (L.kind[tags == "refused"] == "all").all() and (L.kind[tags == "nan"] == "all").all()
    assert (L.kind[tags == "plain"] == "cull").all()
    c = p["cinv"][tags == "refused"]
    ratio = (c[:, 0] * c[:, 2] - c[:, 1] ** 2) / (c[:, 0] * c[:, 2])
    assert (ratio < F.REFUSE / 1.5).all(), ratio                     # clear of the refusal threshold in float32 too
    for k in ("needles", "forms", "tangent", "faint", "tall", "wide", "order"):
        for cs in F.cases(k):
            pp, LL = lists_of(cs)
            cc = pp["cinv"][pp["depths"] > 0.2]
            r = (cc[:, 0] * cc[:, 2] - cc[:, 1] ** 2) / (cc[:, 0] * cc[:, 2])
            assert (r > F.REFUSE * 1.5).all(), (cs.name, r.min())
    full = np.isin(L.gsid, np.nonzero(L.kind == "all")[0])
    assert (L.may[full] == 15).all() and full.sum() >= 4 * 100


@pytest.mark.parametrize("name", ["tall", "wide"])
def test_strips_hold_the_long_walks(name):
    case, = F.cases(name)
    p, L = lists_of(case)
    w, h = _wh(L)
    along, across = (h, w) if name == "tall" else (w, h)
    big = (L.kind == "cull") & ((w > 8) | (h > 8))
    assert (big & (along > 64)).sum() >= 3, along[big]                # more than 64 rows / a row wider than 64 tiles
    assert (along[big] == 68).any() and (across[big] == 3).all()
    first = (L.rects[:, 1] if name == "tall" else L.rects[:, 0])
    tags = np.array(case.tag)
    assert first[tags == "rows 60..67"][0] == 60 and along[tags == "rows 60..67"][0] == 8
    assert first[tags == "rows 50..67"][0] == 50 and big[tags == "rows 50..67"][0]
    # rows differ: a tilted one reaches different tile columns along the strip
    i = int(np.nonzero(tags == "all rows tilted")[0][0])
    sel = L.gsid == i
    rows = (L.tile[sel] // L.gx) if name == "tall" else (L.tile[sel] % L.gx)
    sig = {tuple(L.must[sel][rows == r].tolist()) for r in np.unique(rows)}
    assert len(sig) >= 3, sig
    assert (tags == "small").sum() == 50 and (L.counts[tags == "small"] > 0).all()


def test_order_set_places():
    by = {c.name: c for c in F.cases("order")}
    assert [by["order_n%d" % n].n for n in (1, 2, 3, 255, 256, 257, 515)] == [1, 2, 3, 255, 256, 257, 515]
    for name, P in (("order_n1", 1), ("order_n2", 2), ("order_n3", 3), ("order_n3_p4", 4), ("order_n3_p5", 5)):
        assert lists_of(by[name])[1].gsid.size == P, name
    for case in by.values():
        p, L = lists_of(case)
        order = np.lexsort((np.arange(case.n), L.keys))              # the sorted order of the binning stage
        never = (L.kind == "never") | (L.counts == 0)
        pl = case.places
        if case.name.endswith("ties"):
            assert np.unique(L.keys).size == 5
            continue
        got = set(np.nonzero(never[order])[0].tolist())
        if pl["offscreen"]:                                          # (an empty rect has key 0: at the front by itself)
            assert got == set(range(40)) and pl["never"] | pl["offscreen"] == got      # the front run, whatever kind
        else:
            assert got == pl["never"], (case.name, sorted(got)[:5])
        w, h = _wh(L)
        walk = (L.kind == "cull") & ((w > 8) | (h > 8))
        assert set(np.nonzero(walk[order])[0].tolist()) == pl["big"], case.name
    assert by["order_n255"].places["never"] | by["order_n255"].places["offscreen"] == set(range(40))
    assert by["order_n256"].places["never"] == set(range(100, 140))
    assert by["order_n257"].places["never"] == set(range(216, 256))
    assert by["order_n515_dead"].places["never"] == set(range(256, 512))
    big = sorted(by["order_n515"].places["big"])
    assert big[-1] == 255 and len({b // 64 for b in big[:3]}) == 1 and len(big) == 4


@pytest.mark.parametrize("name", F.SETS)
def test_builder_clearances(name):
    for case in F.cases(name):
        p, L = lists_of(case)
        live = p["depths"] > 0.2
        r = 3 * np.sqrt(p["cov"][live][:, [0, 2]])
        assert (np.abs(r - np.round(r)) > RADIUS_MARGIN * np.maximum(r, 1.0)).all(), case.name
        assert np.array_equal(np.ceil(r).astype(np.int64), p["areas"][live])
        for sgn in (-1, 1):
            e = (p["us"][live] + sgn * np.ceil(r)) / F.TILE
            assert (np.abs(e - np.round(e)) > F.EDGE_MARGIN).all(), (case.name, np.abs(e - np.round(e)).min())
        # the lift reproduces its targets (it need not be exact: truth never depends on it)
        assert np.abs(p["us"][live] - case.u[live]).max() < 2e-4, case.name
        assert (np.abs(p["cov"][live] - case.cov[live]).max(1) <= 1e-5 * np.abs(case.cov[live]).max(1)).all(), case.name


def test_the_list_checker_on_lists_made_from_the_bounds():
    case, = F.cases("forms")
    _, L = lists_of(case)
    # the largest and the smallest lists the bounds allow both pass
    for m in (L.may, L.must):
        keep = m != 0
        lens = np.bincount(L.tile[keep], minlength=L.gx * L.gy)
        end = np.cumsum(lens)
        rg = np.stack([end - lens, end], 1)
        rg[lens == 0] = 0
        r = F.check_culled(L, rg, L.gsid[keep], m[keep])
        assert r["entries"] == L.gsid.size and r["dropped"] == (~keep).sum() and r["must"] <= r["device"] <= r["may"]
    keep = L.may != 0
    lens = np.bincount(L.tile[keep], minlength=L.gx * L.gy)
    end = np.cumsum(lens)
    rg = np.stack([end - lens, end], 1)
    rg[lens == 0] = 0
    ids, masks = L.gsid[keep], L.may[keep]
    j = int(np.nonzero(L.must[keep] != 0)[0][7])
    cases = []
    m2 = masks.copy(); m2[j] &= ~(L.must[keep][j] & -L.must[keep][j]); cases.append((rg, ids, m2))          # a contributing block lost
    j2 = int(np.nonzero(masks != 15)[0][3])
    m3 = masks.copy(); m3[j2] = 15; cases.append((rg, ids, m3))                                                # a block beyond may
    t = int(L.tile[keep][j])
    rg4 = rg.copy(); rg4[t, 1] -= 1; rg4[t + 1:][rg4[t + 1:].any(1)] -= 1                                       # an entry dropped
    last = rg[t, 1] - 1
    if L.must[keep][last] != 0:
        cases.append((rg4, np.delete(ids, last), np.delete(masks, last)))
    sw = np.nonzero((rg[:, 1] - rg[:, 0]) >= 2)[0][0]
    ids5 = ids.copy(); ids5[[rg[sw, 0], rg[sw, 0] + 1]] = ids5[[rg[sw, 0] + 1, rg[sw, 0]]]; cases.append((rg, ids5, masks))   # out of order
    assert len(cases) >= 3
    for c in cases:
        with pytest.raises(AssertionError):
            F.check_culled(L, *c)
