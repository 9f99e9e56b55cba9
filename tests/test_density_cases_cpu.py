"""tests/density_cases.py does what it claims, and the float64 mode of oracle/density_oracle.densify is the float32
mode's formulas: the ground under tests/test_gpu_density_rows.py, checked without a GPU.

``test_float32_distances_of_the_appended_rows`` prints (pytest -s) the figures quoted in the GPU test's docstring."""
import numpy as np
import pytest

from oracle import density_oracle as D
from tests import density_cases as DC
from tests.conftest import load_golden

F = np.float32
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 65_535, 65_536, 65_537, 131_073)
MATRIX = ([(n, p) for n in SIZES for p in ("iid", "block", "all3")] +
          [(n, p) for n in (257, 513, 65_537) for p in DC.PATTERNS if p not in ("iid", "block", "all3")])


@pytest.mark.parametrize("n,pattern", MATRIX)
def test_builder_realises_the_intended_classes_with_every_margin(n, pattern):
    hw = 45 if n <= 513 else 9                        # the classes do not depend on the SH width
    c = DC.build(n, hw, pattern, DC.case_seed(n, pattern))
    p, cls = c["params"], c["cls"].astype(np.int64)
    np.testing.assert_array_equal(DC.oracle_classes(c), c["cls"])
    a = p["alphas_raw"].reshape(-1).astype(np.float64)
    smax = p["scales_raw"].astype(np.float64).max(1)
    pruned, reason = cls == DC.PRUNE, c["reason"]
    # opacity and size: MARGIN clear of the threshold, on the side the class (and the prune reason) says
    by_alpha = pruned & (reason != 1)
    by_size = pruned & (reason >= 1)
    assert (a[by_alpha] <= DC.LA - DC.MARGIN).all() and (a[~by_alpha] >= DC.LA + DC.MARGIN).all()
    assert (a[~by_alpha] <= DC.A_MAX).all()
    assert (smax[by_size] >= DC.LB + DC.MARGIN).all() and (smax[~by_size] <= DC.LB - DC.MARGIN).all()
    if pruned.sum() >= 3:
        assert set(reason[pruned]) == {0, 1, 2}
    # clone / split: one per cent clear of scale_thr
    assert (np.exp(smax[cls == DC.CLONE]) <= 0.99 * DC.TH.scale).all()
    assert (np.exp(smax[cls == DC.SPLIT]) >= 1.01 * DC.TH.scale).all()
    # gradient, as the device divides: float32 acc / float32(cnt); a factor of two clear either way
    with np.errstate(divide="ignore", invalid="ignore"):
        g = c["grad_accum"] / c["cunt"].astype(F)
    g[np.isnan(g)] = 0
    assert g.dtype == F
    dens = cls >= DC.CLONE
    assert (g[dens] >= 2 * DC.TH.grad).all() and (g[(cls == DC.KEEP)] <= DC.TH.grad / 2).all()
    assert ((g >= 2 * DC.TH.grad) | (g <= DC.TH.grad / 2)).all()
    assert np.array_equal(g >= 2 * DC.TH.grad, c["by_grad"])
    # the degenerate statistics: a fixed share of the keep rows is 0 / 0, of the densified rows x / 0
    never = c["cunt"] == 0
    for k in (DC.KEEP, DC.CLONE, DC.SPLIT):
        rows = cls == k
        if rows.any():
            assert (never & rows).sum() == (rows.sum() + 4) // 5
    assert (c["grad_accum"][never & (cls == DC.KEEP)] == 0).all()
    assert np.isinf(g[never & dens]).all() and not never[pruned].any()
    # kept opacities reach the near-opaque end on any model that is large enough to
    if n >= 511 and (~pruned).sum() > n // 8:
        assert a[~pruned].max() > 8.5 and a[~pruned].min() < DC.LA + 0.5
    # shapes, types, determinism
    for j, k in enumerate(DC.NAMES):
        for t in (p, c["m"], c["v"]):
            assert t[k].shape == (n, DC.widths(hw)[j]) and t[k].dtype == F and t[k].flags.c_contiguous
        assert (c["v"][k] >= 0.1).all()
    assert c["unit_noise"].shape == (n, 3) and c["cunt"].dtype == np.int32
    if n <= 513:
        c2 = DC.build(n, 45, pattern, DC.case_seed(n, pattern))
        assert all(np.array_equal(c2["params"][k], p[k]) for k in DC.NAMES)


def test_patterns_are_what_their_names_say():
    for n in (257, 513, 65_537):
        tail = ((n - 1) // 256) * 256
        cl = {p: DC.classes(n, p, 1) for p in DC.PATTERNS}
        assert np.bincount(cl["iid"], minlength=4).min() > n // 6
        for k in range(4):
            assert (cl["all%d" % k] == k).all()
        assert np.array_equal(cl["wave"][:320], np.repeat([0, 1, 2, 3, 0], 64)[:n])
        blocks = cl["block"][:tail].reshape(-1, 256)
        assert (blocks == blocks[:, :1]).all() and np.array_equal(blocks[:, 0], np.arange(len(blocks)) % 4)
        assert cl["first"][0] == 3 and not cl["first"][1:].any()
        assert cl["last"][-1] == 2 and not cl["last"][:-1].any()
        assert (cl["tail_only"][tail:] == 3).all() and not cl["tail_only"][:tail].any() and tail < n
        assert not cl["tail_gone"][tail:].any() and (cl["tail_gone"][:tail] == 1).all()


@pytest.mark.parametrize("hw", [45, 0])
def test_edges_classify_as_written(hw):
    c = DC.edges(hw)
    got = DC.oracle_classes(c)
    for i, label in enumerate(c["labels"]):
        assert got[i] == c["cls"][i], (i, label, int(got[i]))
    p = c["params"]
    la, lb, g = F(DC.LA), F(DC.LB), F(DC.TH.grad)
    lab = lambda s: [i for i, l in enumerate(c["labels"]) if l.startswith(s)]
    assert p["alphas_raw"][lab("alpha at its threshold: kept")[0], 0] == la
    assert p["alphas_raw"][lab("alpha one ulp below: pruned")[0], 0] == np.nextafter(la, F(-np.inf))
    assert p["scales_raw"][lab("smax at log(big): kept")[0]].max() == lb
    assert p["scales_raw"][lab("smax one ulp above")[0]].max() == np.nextafter(lb, F(np.inf))
    for i in lab("acc == grad_thr"):
        assert c["grad_accum"][i] / F(c["cunt"][i]) == g and c["cunt"][i] in (1, 2, 4)
    for i in lab("acc one ulp below"):
        assert c["grad_accum"][i] / F(c["cunt"][i]) == np.nextafter(g, F(0)) and c["cunt"][i] in (1, 2, 4)
    assert sorted(int(c["cunt"][i]) for i in lab("acc == grad_thr") if c["cls"][i] == DC.CLONE) == [1, 2, 4]
    # what the special rows append, in float32 (the reference's own arithmetic) and in float64
    p32, _, _, info = DC.reference(c, dtype=F)
    p64, _, _, _ = DC.reference(c)
    new = np.concatenate([info["clone"], info["split"]])
    at = lambda i: info["n_keep"] + int(np.nonzero(new == i)[0][0])
    for i in lab("zero quaternion"):
        assert not p32["rots_raw"][at(i)].any() and not p64["rots_raw"][at(i)].any()
        np.testing.assert_array_equal(p32["pws"][at(i)], p["pws"][i])
        np.testing.assert_array_equal(p64["pws"][at(i)], p["pws"][i])
    for i in lab("alphas_raw 20 on"):
        assert p32["alphas_raw"][at(i), 0] == np.inf and abs(p64["alphas_raw"][at(i), 0] - 20) < 1e-6
    assert np.isinf(p32["alphas_raw"]).sum() == 2 and np.isfinite(p64["alphas_raw"]).all()
    d = DC.distances(c, info)
    assert np.isinf(d["alphas_raw"]).sum() == 2 and all(np.isfinite(d[k]).all() for k in ("pws", "scales_raw", "rots_raw"))


@pytest.mark.parametrize("n,pattern", [(513, "iid"), (65_537, "iid"), (513, "block"), (257, "all3"), (257, "all0")])
def test_float64_mode_moves_the_same_rows_bit_for_bit(n, pattern):
    c = DC.build(n, 45, pattern, DC.case_seed(n, pattern))
    p32, m32, v32, i32 = DC.reference(c, dtype=F)
    p64, m64, v64, i64 = DC.reference(c)
    nk = i32["n_keep"]
    assert all(np.array_equal(i32[k], i64[k]) for k in ("remain", "clone", "split"))
    for k in DC.NAMES:
        assert p32[k].dtype == F and p64[k].dtype == np.float64 and p32[k].shape == p64[k].shape
        np.testing.assert_array_equal(p64[k][:nk], c["params"][k][i32["remain"]])
        np.testing.assert_array_equal(p32[k][:nk], p64[k][:nk])
        np.testing.assert_array_equal(m32[k], m64[k])
        np.testing.assert_array_equal(v32[k], v64[k])
        assert not m32[k][nk:].any() and not v32[k][nk:].any()
    for k in ("low_shs", "high_shs"):                 # copied, not computed: the same in either mode
        np.testing.assert_array_equal(p32[k], p64[k])
        np.testing.assert_array_equal(p32[k][nk:], c["params"][k][np.concatenate([i32["clone"], i32["split"]])])


def test_float64_mode_on_the_g8_fixture():
    g = load_golden("g8_densify.npz")
    p = {k: g["pre_" + k] for k in D.NAMES}
    m = {k: g["pre_m_" + k] for k in D.NAMES}
    v = {k: g["pre_v_" + k] for k in D.NAMES}
    p32, m32, v32, info = D.densify(p, m, v, g["grad_accum"], g["cunt"], g["unit_noise"], D.Thresholds(1.0))
    p64, m64, v64, _ = D.densify(p, m, v, g["grad_accum"], g["cunt"], g["unit_noise"], D.Thresholds(1.0), np.float64)
    nk = int(info["remain"].sum())
    for k in D.NAMES:
        np.testing.assert_array_equal(p64[k][:nk], p32[k][:nk])
        np.testing.assert_allclose(p64[k][nk:], p32[k][nk:], rtol=3e-6, atol=3e-6)      # the fixture's own bound
        np.testing.assert_allclose(p64[k][nk:], g["post_" + k][nk:], rtol=3e-6, atol=3e-6)
        np.testing.assert_array_equal(m64[k], g["post_m_" + k])
        np.testing.assert_array_equal(v64[k], g["post_v_" + k])


def test_float32_distances_of_the_appended_rows():
    """per tensor, over every case of the GPU matrix: the largest per-row distance of the float32 oracle from the
    float64 one, as given and with the inputs one ulp away.  Bounds the figures from above by what the formats allow:
    alphas_raw by the 7e-5 of a = 9 (twice, for the ulp moves); the others stay below the 1e-5 floor of the GPU rule,
    which therefore governs them (pws is the largest: a child that lands near the origin has a small row magnitude)."""
    worst = {k: [0.0, 0.0] for k in DC.TOLERANCED}
    cases = [DC.build(n, 0, p, DC.case_seed(n, p)) for n, p in MATRIX] + [DC.edges(0)]     # SH rows are only copied
    for c in cases:
        info = DC.reference(c, with_state=False)[3]
        if info["n_clone"] + info["n_split"] == 0:
            continue
        ref = DC.appended_reference(c, info)
        f32 = DC.appended_reference(c, info, F)
        d = DC.distances(c, info)
        for k in DC.TOLERANCED:
            fin = np.isfinite(d[k])
            as_given = DC.row_error(k, f32[k], ref[k])
            assert (as_given[fin] <= d[k][fin]).all()
            worst[k][0] = max(worst[k][0], as_given[fin].max(initial=0))
            worst[k][1] = max(worst[k][1], d[k][fin].max(initial=0))
    print("\nappended rows, largest float32 distance of a row over %d cases: as given | with the one-ulp moves" % len(cases))
    for k in DC.TOLERANCED:
        print("  %-11s %.3g | %.3g" % (k, worst[k][0], worst[k][1]))
    assert 1e-5 < worst["alphas_raw"][1] < 2e-4
    for k in ("pws", "scales_raw", "rots_raw"):
        assert 0 < worst[k][1] < 1e-5, k
