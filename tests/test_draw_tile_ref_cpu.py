"""CPU checks of tests/draw_tile_ref.py, the hand-built one-tile lists of tests/test_gpu_draw_tiles.py: the builder's
conditions hold on the reference (both policies, every set), ``O.bin_tiles`` returns exactly the intended lists, every
scenario is what it claims, the float64 backward is the derivative of the float64 forward, never-hit rows are exactly
zero.  Each set prints what the builder made of it (re-draws, list lengths, per-block stop indices, hit / clamp / floor
counts).  The extras cases (``case(name, extras=True)``): the geometry is the plain case's, the extended ``blend`` is the
oracle's composition bit for bit in float64, and dz and the dalphas / dus rows under dL/ddepth, dL/dalpha and the
background are the central differences of that blend."""
import time

import numpy as np
import pytest

from oracle import gs_oracle as O
from tests import draw_tile_ref as D
from tests.test_numeric_diff import check

LENGTHS = {0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 127, 128, 129, 192, 193, 300}


@pytest.mark.parametrize("name", D.SETS)
def test_builder_conditions_lists_and_claims(name):
    t0 = time.perf_counter()
    c = D.case(name)
    print("\n" + D.report(name))
    a = c.arrays
    # one patch per Gaussian, on its own tile, in list order: O.bin_tiles returns exactly the intended lists
    ranges, gsid, rects, counts = O.bin_tiles(a["us"], a["areas"].copy(), a["depths"].copy(), D.W, D.H, O.POLICY_G)
    want_r, want_g = D.lists_to_arrays(c.lists)
    assert (counts == 1).all() and np.array_equal(ranges, want_r) and np.array_equal(gsid, want_g)
    assert sorted(np.concatenate(c.lists).tolist()) == list(range(c.n))
    assert not np.array_equal(gsid, np.arange(c.n))
    # policy A (pixel boxes, far cull): the same lists without the Gaussians centred far outside the image
    for l, la in zip(c.lists, D.lists(c, "forward_cpu")[0]):
        far = np.abs(a["us"][l] / np.array([D.W, D.H], np.float32)).max(1) > 1.3
        assert np.array_equal(l[~far], la)
    for pname, pol in D.POLICIES.items():
        ls, rg, gs = D.lists(c, pname)
        ref = D.reference(name, pname)
        # the restated blend the diagnostics come from IS O.draw
        for x, y in zip(D.blend(a, ls, pol), (ref["image"], ref["contrib"], ref["final_tau"])):
            assert np.array_equal(x, y)
        d = D.distances(name, pname)
        assert d["contrib_equal"], (name, pname)
        if pol.alpha_skip > 0:
            assert ref["diag"]["skip_dist"].min() >= D.SKIP_MARGIN
            assert ref["diag"]["stop_dist"].min() >= D.STOP_MARGIN
        # rows that no pixel hits have an exactly zero reference (and only finite numbers anywhere)
        never = ref["diag"]["hits"] == 0
        for k in D.GRADS:
            assert np.isfinite(ref[k]).all()
            assert not np.asarray(ref[k]).reshape(c.n, -1)[never].any(), (name, pname, k)
        print("  %-11s float32 distance: image %.2g, final_tau %.2g, rows (median / max) %s" % (
            pname, d["image"].max(), d["final_tau"].max(),
            {k: "%.2g / %.2g" % (np.median(d[k]), d[k].max()) for k in D.GRADS}))
    D.check_claims(name)
    if name.startswith("lengths"):
        assert all(s["contrib"] == len(l) for s, l in zip(c.scenarios, c.lists))
    print("  evaluated in %.1f s" % (time.perf_counter() - t0))


def test_every_length_of_the_issue_is_there():
    got = {len(l) for n in ("lengths0", "lengths1") for l in D.case(n).lists}
    assert got == LENGTHS
    # lengths0 keeps its outside centres within 1.3 x the image: the BOX instances (policy A) walk the very same lists
    c = D.case("lengths0")
    assert all(np.array_equal(a, b) for a, b in zip(c.lists, D.lists(c, "forward_cpu")[0]))
    assert {63, 64, 65, 127, 128, 129, 192} <= {len(l) for l in D.lists(c, "forward_cpu")[0]}
    assert (np.abs(c.arrays["us"]) > np.array([D.W, D.H])).any() or (c.arrays["us"] < 0).any()
    ragged = {len(D.case(n).lists[t]) for n in ("lengths0", "lengths1") for t in (4, 9, 10, 11, 12, 13, 14)}
    assert {0, 1, 8, 63, 64, 65, 127, 128, 129, 192, 300} <= ragged


def test_case_is_a_pure_function_and_read_only():
    c = D.case("stops")
    again = D.case.__wrapped__("stops")            # (past the cache: built a second time, re-draws included)
    assert again is not c and c.redrawn > 0 and again.redrawn == c.redrawn
    for k, v in c.arrays.items():
        assert v.tobytes() == again.arrays[k].tobytes(), k
    assert all(np.array_equal(a, b) for a, b in zip(c.lists, again.lists))
    c = D.case("reach")
    with pytest.raises(ValueError):
        c.arrays["us"][0, 0] = 0.0
    assert D.case("reach", 1).arrays["us"].tobytes() != c.arrays["us"].tobytes()


@pytest.mark.parametrize("name", ["lengths0", "reach"])
def test_float64_backward_is_the_derivative_of_the_forward(name):
    """central differences of L = sum(dL/dgamma . image) (float64 ``O.draw`` on the Gaussian's tile) against the
    float64 ``O.draw_backward``, by the rule of tests/test_numeric_diff.py applied to the row divided by its largest
    entry; sets without stops and without the clamp (whose derivative the reference defines as g, kernel.cu:921)"""
    c = D.case(name)
    ref = D.reference(name, "gsplatcu")
    _, rg, gs = D.lists(c, "gsplatcu")
    a = {k: np.asarray(v, np.float64) for k, v in c.arrays.items() if k != "areas"}
    dl = a["dloss_dgammas"]
    assert ref["diag"]["clamped"].sum() == 0 and (ref["final_tau"][ref["contrib"] > 0] > 1e-3).all()
    hit = np.nonzero((ref["diag"]["hits"] > 0) & (ref["walked"] <= 12))[0]
    rows = hit[:: max(1, len(hit) // 10)][:12]
    assert len(rows) >= 8
    for g in rows:
        g, t = int(g), int(c.tile_of[g])

        def loss(key, j, h):
            b = dict(a)
            b[key] = a[key].copy()
            b[key].reshape(c.n, -1)[g, j] += h
            img = O.draw(D.W, D.H, rg, gs, b["us"], b["cinv2ds"], b["alphas"], b["colors"], None, O.POLICY_G,
                         np.float64, tiles=[t])[0]
            return float((img * dl).sum())

        for key, gk in (("us", "dus"), ("cinv2ds", "dcinv2ds"), ("alphas", "dalphas"), ("colors", "dcolors")):
            ana = np.asarray(ref[gk]).reshape(c.n, -1)[g]
            # steps: small against the parameter (the conics of the wide entries are ~1e-3, the opacities down to 0.012) and
            # against the builder's margins (2e-5 px moves the alpha' of a 0.8 px Gaussian by 1e-4 of itself), large
            # against the rounding of L (1e-16 / h of it, next to gradients of 1e-7)
            h = {"us": 2e-5, "colors": 1e-4}.get(key) or 1e-4 * float(np.abs(a[key].reshape(c.n, -1)[g]).max())
            num = np.array([(loss(key, j, h) - loss(key, j, -h)) / (2 * h) for j in range(ana.size)])
            scale = max(np.abs(ana).max(), 1e-300)
            assert check(num / scale, ana / scale), (name, g, key, num, ana)


@pytest.mark.parametrize("pname", list(D.POLICIES))
def test_hardware_restatement_is_the_float32_oracle_without_its_ulps(pname):
    """``D.backward_hw`` with no ulp moved is ``O.draw_backward`` in float32, bit for bit (every set: parts (a), (b) of
    ``D.distances`` take their rows from it)"""
    for name in D.SETS:
        c = D.case(name)
        _, cont, tau = D.forward(c, pname, np.float32)
        for a, b in zip(D.backward_hw(c, pname, cont, tau), D.backward(c, pname, cont, tau, np.float32)):
            assert a.dtype == np.float32 and np.array_equal(a, b.astype(np.float32))


# ------------------------------------------------------------------------------------------------------ render extras
@pytest.mark.parametrize("name", D.SETS)
def test_extras_keep_the_geometry_and_blend_is_the_oracle_composition(name):
    c, cx = D.case(name), D.case(name, extras=True)
    assert cx is D.case(name, 0, True) and cx.extras and not c.extras
    # nothing is re-drawn: the very arrays, lists and claims of the plain case
    for k, v in c.arrays.items():
        assert cx.arrays[k] is v, k
    assert cx.lists is c.lists and cx.redrawn == c.redrawn and cx.scenarios is c.scenarios
    D.check_claims(name)
    assert set(cx.arrays) - set(c.arrays) == {"z", "dloss_ddepth", "dloss_dalpha"}
    z = cx.arrays["z"]
    assert z.dtype == np.float32 and z.shape == (c.n,) and 0.2 <= z.min() and z.max() <= 100.0
    assert z.max() / z.min() > 50 and np.abs(np.corrcoef(np.log(z), c.arrays["depths"])[0, 1]) < 0.3
    zero = c.arrays["dloss_dgammas"][0] == 0       # (the block of lengths0 lies outside the image: its ragged column)
    assert zero.sum() == (0 if name == "lengths0" else 64)
    for k in ("dloss_ddepth", "dloss_dalpha"):
        w = cx.arrays[k]
        assert w.dtype == np.float32 and w.shape == (D.H, D.W) and not w[zero].any() and w[~zero].all()
        with pytest.raises(ValueError):
            w[0, 0] = 0.0
    assert np.array_equal(cx.bg, np.float32(D.BG))
    for pname, pol in D.POLICIES.items():
        ls = D.lists(cx, pname)[0]
        ref, plain = D.reference(name, pname, extras=True), D.reference(name, pname)
        # no decision depends on the extras: contrib and final_tau are the plain case's
        assert np.array_equal(ref["contrib"], plain["contrib"]) and np.array_equal(ref["final_tau"], plain["final_tau"])
        got = D.blend(cx.arrays, ls, pol, extras=cx.bg)
        for k, x in zip(("image", "contrib", "final_tau", "depth", "alpha"), got):
            assert np.array_equal(x, ref[k]), (name, pname, k)
        for t, l in enumerate(ls):
            if len(l) == 0:
                tx, ty, x0, y0, ww, hh = D.geom(t)
                win = (slice(y0, y0 + hh), slice(x0, x0 + ww))
                assert all((ref["image"][ch][win] == np.float64(cx.bg[ch])).all() for ch in range(3))
                assert not ref["depth"][win].any() and not ref["alpha"][win].any() and not ref["final_tau"][win].any()
        never = ref["diag"]["hits"] == 0
        for k in D.GRADS_X:
            assert np.isfinite(ref[k]).all() and not np.asarray(ref[k]).reshape(c.n, -1)[never].any(), (name, pname, k)
        assert ref["dz"].shape == (c.n,) and ref["dz"].any()
        fl = D.pixel_floor(name, pname, extras=True)
        assert set(fl) == {"image", "final_tau", "depth", "alpha"} and (fl["depth"] >= fl["alpha"]).all()


def test_extras_distances_keep_contrib_and_restate_the_kernels_way():
    """the float32 restatements of an extras case (``D.distances``) decide as the reference does, and in float32 the
    extended blend forms alpha as 1 - tau and the image with one fmaf, the empty tiles as the background itself"""
    name = "lengths1"                               # (three empty tiles)
    cx = D.case(name, extras=True)
    for pname, pol in D.POLICIES.items():
        d = D.distances(name, pname, extras=True)
        assert d["contrib_equal"]
        assert set(d) >= {"image", "final_tau", "depth", "alpha"} | set(D.GRADS_X) | {k + "_alone" for k in D.GRADS_X}
        ls = D.lists(cx, pname)[0]
        img, cont, tau, depth, alpha = D.blend(cx.arrays, ls, pol, np.float32, poly=True, fma=True, extras=cx.bg)
        assert img.dtype == np.float32 and depth.dtype == np.float32
        live = np.zeros((D.H, D.W), bool)
        for t, l in enumerate(ls):
            tx, ty, x0, y0, ww, hh = D.geom(t)
            live[y0:y0 + hh, x0:x0 + ww] = len(l) > 0
        assert np.array_equal(alpha[live], (np.float32(1) - tau)[live]) and not alpha[~live].any()
        assert all((img[ch][~live] == cx.bg[ch]).all() for ch in range(3)) and (~live).any()


@pytest.mark.parametrize("name", D.SETS)
def test_extras_backward_is_the_derivative_of_the_extended_blend(name):
    """central differences of L = <Wi, image> + <Wd, depth> + <Wa, alpha> of the float64 extended ``D.blend`` (on the
    Gaussian's tile) against dz and the dalphas / dus rows of the extras reference, by the rule of
    tests/test_numeric_diff.py applied to the row divided by its largest entry; rows whose own clamp or floor never binds
    (the reference defines the clamp's derivative as g, kernel.cu:921), a few per set"""
    cx = D.case(name, extras=True)
    ref = D.reference(name, "gsplatcu", extras=True)
    a = {k: np.asarray(v, np.float64) for k, v in cx.arrays.items() if k != "areas"}
    Wi, Wd, Wa = a["dloss_dgammas"], a["dloss_ddepth"], a["dloss_dalpha"]
    d = ref["diag"]
    ok = np.nonzero((d["hits"] > 0) & (ref["walked"] <= 12) & (d["clamped"] == 0) & (d["floored"] == 0)
                    & (np.abs(ref["dz"]) > 0))[0]
    rows = ok[:: max(1, len(ok) // 4)][:4]
    assert len(rows) >= 3, (name, len(ok))
    for g in rows:
        g, t = int(g), int(cx.tile_of[g])
        tx, ty, x0, y0, ww, hh = D.geom(t)
        win = (slice(y0, y0 + hh), slice(x0, x0 + ww))
        only = [l if i == t else l[:0] for i, l in enumerate(cx.lists)]

        def loss(key, j, h):
            b = dict(a)
            b[key] = a[key].copy()
            b[key].reshape(cx.n, -1)[g, j] += h
            img, _, _, depth, alpha = D.blend(b, only, O.POLICY_G, np.float64, extras=cx.bg)
            return float((img[:, win[0], win[1]] * Wi[:, win[0], win[1]]).sum() + (depth[win] * Wd[win]).sum()
                         + (alpha[win] * Wa[win]).sum())

        for key, gk in (("z", "dz"), ("alphas", "dalphas"), ("us", "dus")):
            ana = np.asarray(ref[gk]).reshape(cx.n, -1)[g]
            h = 2e-5 if key == "us" else 1e-4 * float(np.abs(a[key].reshape(cx.n, -1)[g]).max())
            num = np.array([(loss(key, j, h) - loss(key, j, -h)) / (2 * h) for j in range(ana.size)])
            scale = max(np.abs(ana).max(), 1e-300)
            assert check(num / scale, ana / scale), (name, g, key, num, ana)
