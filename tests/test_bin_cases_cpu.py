"""The inputs of tests/test_gpu_bin_lists.py checked without a GPU (tests/bin_cases.py): for every case, that the builder
hit the tile rects and depth keys it was asked for (by the oracle's getRects / depth key, which the golden fixtures pin),
that the case holds the n, P, pass counts and boundary positions its set claims for it, and that the lists written down
by definition (``reference_lists``) equal ``O.bin_tiles`` -- one stable sort of (tile, key, id) triples -- on the same
arrays: ranges, ids and the depths / areas after the in-place cull.  The two ``large`` cases get the same checks on their
first 5000 Gaussians.  A failing assertion prints the case: its set, name, and what it was supposed to contain."""
import numpy as np
import pytest

from oracle import gs_oracle as O
from tests import bin_cases as BC

POL = {"gsplatcu": O.POLICY_G, "forward_cpu": O.POLICY_A}


def _check_builder(c):
    us, areas, depths = BC.build(c)
    pol = POL[c.policy]
    a2, d2 = areas.copy(), depths.copy()
    rects, counts = O.get_rects(us, a2, d2, c.W, c.H, pol)
    has = c.form == BC.FORM_PATCH
    x0, y0, w, h = (c.rect[:, j] for j in range(4))
    want = np.stack([x0, y0, x0 + w, y0 + h], 1)
    gx, gy = BC.grid(c.W, c.H)
    assert (want[has, 2] <= gx).all() and (want[has, 3] <= gy).all() and (c.rect[has, 2:] >= 1).all(), c
    bad = np.nonzero(has & ((rects.astype(np.int64) != want).any(1) | (counts != w * h)))[0]
    assert bad.size == 0, (c, "rect missed", bad[:5], rects[bad[:5]], want[bad[:5]])
    bad = np.nonzero(~has & (counts != 0))[0]
    assert bad.size == 0, (c, "patches where none were meant", bad[:5], [BC.FORM_NAMES[f] for f in c.form[bad[:5]]])
    if c.policy == "gsplatcu":
        keys = O.depth_keys(depths, pol)
    else:                                                   # (the oracle keeps the depth itself: value order == bit order)
        keys = np.asarray(O.depth_keys(depths, pol), np.float32).view(np.uint32)
        assert (depths[has] > 0).all(), c
    bad = np.nonzero(has & (keys != c.key))[0]
    assert bad.size == 0, (c, "key missed", bad[:5], keys[bad[:5]], c.key[bad[:5]])
    # every way of having no patches does what the docstring of bin_cases says it does
    ref = BC.reference_lists(c)
    assert np.array_equal(ref["depths"], d2, equal_nan=True) and np.array_equal(ref["areas"], a2), (c, "in-place cull")
    if c.policy == "gsplatcu":
        assert (ref["depths"][c.form >= BC.FORM_OFF] == -1).all() and (ref["depths"][c.form == BC.FORM_NEAR] == np.float32(0.1)).all(), c
    else:
        assert np.array_equal(ref["depths"], depths, equal_nan=True) and np.array_equal(ref["areas"], areas), c
    return us, areas, depths


def _check_prop(c, ref, prop):
    kind, a = prop[0], prop[1:]
    ranges = ref["ranges"]
    lens = ranges[:, 1] - ranges[:, 0]
    gx, gy = BC.grid(c.W, c.H)
    has = c.form == BC.FORM_PATCH
    if kind == "run_end":
        return bool((ranges[lens > 0, 1] == a[0]).any())
    if kind == "tile_len":
        return int(lens[a[0]]) == a[1]
    if kind == "tile_has":
        return bool(lens[a[0]] > 0)
    if kind == "column_has":
        return bool((lens.reshape(gy, gx)[:, a[0]] > 0).any())
    if kind == "row_has":
        return bool((lens.reshape(gy, gx)[a[0]] > 0).any())
    if kind in ("zero_index", "patch_index"):
        return bool(has[a[0]]) == (kind == "patch_index")
    if kind in ("zero_sorted", "patch_sorted"):
        return bool(BC.sorted_has(c)[a[0]]) == (kind == "patch_sorted")
    if kind == "span_over":
        return bool((c.rect[has, 2] * c.rect[has, 3] > a[0]).any())
    if kind == "count_is":
        return bool(has[a[0]]) and int(c.rect[a[0], 2] * c.rect[a[0], 3]) == a[1]
    raise ValueError(prop)


def _check_claims(c):
    ref = BC.reference_lists(c)
    gx, gy = BC.grid(c.W, c.H)
    T = gx * gy
    measured = dict(n=c.n, P=ref["P"], maxkey=ref["maxkey"], depth_passes=BC.real_depth_passes(ref["maxkey"]), T=T,
                    tile_key_bits=BC.tile_key_bits(T), tile_passes=BC.sort_passes(BC.tile_key_bits(T)),
                    sort_ipt=8 if c.n <= BC.RS_SHORT else 16)
    for k, v in c.claims.items():
        assert measured[k] == v, (c, "claims %s = %r, has %r" % (k, v, measured[k]))
    for prop in c.props:
        assert _check_prop(c, ref, prop), (c, "lacks", prop)
    assert ref["P"] == int((ref["ranges"][:, 1] - ref["ranges"][:, 0]).sum()) == ref["ids"].shape[0], c


def _check_against_oracle(c, us, areas, depths):
    ref = BC.reference_lists(c)
    a2, d2 = areas.copy(), depths.copy()
    ranges, ids, _, _ = O.bin_tiles(us, a2, d2, c.W, c.H, POL[c.policy])
    assert np.array_equal(ranges, ref["ranges"]), (c, "ranges")
    assert np.array_equal(ids, ref["ids"]), (c, "ids", np.nonzero(ids != ref["ids"])[0][:5])
    assert np.array_equal(d2, ref["depths"], equal_nan=True) and np.array_equal(a2, ref["areas"]), (c, "in-place cull")


@pytest.mark.parametrize("cset", ["counts", "totals", "keys", "grid"])
def test_cases_are_what_they_claim(cset):
    cases = BC.cases(cset)
    assert len({c.name for c in cases}) == len(cases)
    for c in cases:
        us, areas, depths = _check_builder(c)
        _check_claims(c)
        _check_against_oracle(c, us, areas, depths)


def test_sets_hold_the_stated_sizes():
    counts = {c.name: c for c in BC.cases("counts")}
    for n in BC.COUNT_N:
        for pattern in BC.COUNT_PATTERNS:
            assert "n%d_%s_mm" % (n, pattern) in counts
            assert ("n%d_%s_nan" % (n, pattern) in counts) == (pattern != "none")
    forms = np.concatenate([c.form for c in counts.values()])
    assert set(np.unique(forms)) == {0, 1, 2, 3, 4}          # every way of having no patches is used
    assert {c.claims["P"] for c in counts.values()} >= {0, 1}
    totals = BC.cases("totals")
    assert sorted({c.claims["P"] for c in totals}) == sorted(BC.TOTAL_P) and len(totals) == 2 * len(BC.TOTAL_P)
    assert {P % 4 for P in BC.TOTAL_P} == {0, 1, 2, 3}
    for border in (BC.RANGE_WG, BC.SC_TILE, 2 * BC.SC_TILE):   # a run that ends exactly there, with more behind it
        assert any(("run_end", border) in c.props and c.claims["P"] > border for c in totals), border
    keys = {c.name: c for c in BC.cases("keys")}
    for K in BC.KEY_MAXES:
        assert keys["max%d" % K].claims["depth_passes"] == (BC.bit_length(K) + 7) // 8
    assert [keys["max%d" % K].claims["depth_passes"] for K in BC.KEY_MAXES] == [1, 2, 2, 3, 3, 4]
    assert {c.policy for c in keys.values()} == {"gsplatcu", "forward_cpu"}
    sat = keys["saturate"]
    d = BC.build(sat)[2]
    assert np.isposinf(d).sum() == 2 and np.isnan(d).sum() == 1 and (d == np.float32(5e6)).sum() == 2
    grid = BC.cases("grid")
    assert [c.claims["tile_key_bits"] for c in grid] == [1, 1, 8, 8, 9, 13, 14, 17]
    assert [c.claims["tile_passes"] for c in grid] == [1, 1, 1, 1, 2, 2, 2, 3]
    assert [BC.pass_widths(c.claims["tile_key_bits"]) for c in grid[4:]] == [[5, 4], [7, 6], [7, 7], [6, 6, 5]]
    assert any(c.W % 16 and c.H % 16 for c in grid)


def test_depth_for_key_hits_every_border_key():
    keys = np.array([200, 201, 255, 256, 257, 65535, 65536, (1 << 24) - 1, 1 << 24] + list(range(200, 5200, 7)))
    d = BC.depth_for_key(keys)
    assert d.dtype == np.float32 and np.array_equal(O.depth_keys(d), keys) and (d >= np.float32(0.2)).all()


@pytest.mark.parametrize("n", BC.LARGE_N)
def test_large_case_prefix(n):
    c = BC.large_case(n)
    assert c.n == n and c.claims["sort_ipt"] == (8 if n <= 2621440 else 16)
    assert c.claims["P"] == int((c.form == BC.FORM_PATCH).sum()) and (c.form[3::7] != BC.FORM_PATCH).all()
    assert np.unique(c.key).size <= 3000 < n // 500             # ties abound
    p = c.prefix(5000)
    us, areas, depths = _check_builder(p)
    _check_claims(p)
    _check_against_oracle(p, us, areas, depths)
