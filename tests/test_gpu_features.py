"""k_feature_render / k_feature_gather (csrc/egs_feat.hip) through ``easygaussiansplatting_amd.features``,
against the float64 reference of tests/feature_ref.py.

1. One-tile lists (tests/draw_tile_ref.py: five sets x policies gsplatcu / forward_cpu on the 72 x 40 image) x C in
   {1, 3, 8, 9, 20} channels -- a tail-only chunk, a tail of 3, an exact chunk, a chunk plus a tail of 1 with a 36-byte
   row stride, two chunks plus a tail of 4: ``gsplatcu.splat``, whose ``contrib`` must equal the reference's on every
   pixel, then ``splat_features`` and ``splat_gather``:
     * map: |got - ref| <= max(pixel floor, 2 x distance) on EVERY pixel (the rule of test_gpu_draw_tiles.py and
       test_gpu_blend_weights.py; floor 2^-23 (2 + contrib) max(1, max |feat| of the tile's list), distance (a)-(d) of
       ``F.distance``); pixels of empty tiles are +0.0 bit for bit;
     * gather: |got - ref| <= max(row floor, 2 x distance) on every row and channel (floor 2^-23 (2 + position in list)
       sum_p w |gmap|); rows whose reference ``hits`` are 0 stay zero bit for bit; two runs from zeroed buffers are
       bitwise equal (every Gaussian lies on one tile); a second call into the same buffer gives exactly twice the first;
     * C = 3 with the colours as features: the map is also held to ``D.reference``'s image by k_draw's own rule
       (``D.pixel_floor``, ``D.distances``).
2. Every output pixel is written: a raw ``egs_feature_render`` into a NaN-filled [9, 40, 72] buffer (ragged right column
   and bottom row; set lengths1 adds empty tiles) leaves it finite and the NaN guard band behind it untouched.
3. A fused state with culled, masked lists (20 000 Gaussians, 128 x 96, C = 9) against the float64 walk of the seven
   ops' 2D tensors over the state's own lists and contrib; an all-ones channel against 1 - final_tau and against
   ``importance``'s sum.
4. Adjointness on the device.  5. Autograd through ``FeatureRender``.  6. ``lift`` over two views.  7. n = 0.
9. The gather of a one-channel all-ones map beside ``importance.splat_weights``' ``sum`` on the one-tile sets: both
   kernels take the walk of csrc/egs_list_walk.h (see the test's docstring for what they still do not share).

Test 1 prints, per tensor, the largest distance | the largest kernel error | the largest error / bound.
Measured on MI355X, largest over the five sets, two policies and five
channel counts (58 tests pass, 0 pixels and 0 rows excluded; distances and errors absolute, features and pixel gradients
in [-1, 1]):
                                  distance   kernel error   error / bound
  map                             1.4e-05    1.4e-05        0.52
  gather                          2.0e-05    1.4e-05        0.60
  colours as features (k_draw's)  7.4e-06    6.9e-06        0.85
(the largest on the steepest conics of set values and on set stops; lengths0 / lengths1 stand at 0.04 for the map and 0.56
for the gather).  Two gathers were bitwise equal and the second call doubled the first exactly on every case.
Test 3 on MI355X: P = 11 753 after culling, 12 288 covered pixels, 122 of them with a near entry (0.99 %), at most 2 on one
pixel; map: largest error 1.02e-5, 0.10 of its bound; gather 1.1e-6 .. 2.3e-6 of a column's largest entry (median relative
1.0e-6 .. 1.1e-6); all-ones channel within 3.8e-7 of 1 - final_tau, its gather 6.2e-8 of importance's largest sum.
Test 4: relative difference 6.7e-10.  Test 6: 8.8e-6 .. 1.2e-5 of a column's largest entry, median relative 1.0e-6 .. 1.1e-6.
"""
import ctypes as C

import numpy as np
import pytest

from tests import blend_weights_ref as B
from tests import draw_tile_ref as D
from tests import feature_ref as F

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from easygaussiansplatting_amd import _featlib, features            # noqa: E402

CHANNELS = (1, 3, 8, 9, 20)


@pytest.fixture
def gpu():
    """the policy, the segment switch and the splat memo put back afterwards (as tests/test_gpu_draw_tiles.py does)"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from easygaussiansplatting_amd import fused, gsplatcu, importance
    gsplatcu.set_policy("gsplatcu")
    keep = fused.SEGMENTS
    yield gsplatcu, fused, importance
    fused.SEGMENTS = keep
    gsplatcu.set_policy("gsplatcu")
    gsplatcu.clear_memo()


def _t(a):
    return torch.from_numpy(np.array(a)).cuda()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _host(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _nonempty(c, pname):
    m = np.zeros((D.H, D.W), bool)
    for t, l in enumerate(D.lists(c, pname)[0]):
        if len(l):
            tx, ty, x0, y0, ww, hh = D.geom(t)
            m[y0:y0 + hh, x0:x0 + ww] = True
    return m


def _splat(gsc, fused, name, pname):
    """one ``gsplatcu.splat`` of the set, its contrib checked -> the arguments of splat_features / splat_gather"""
    a = D.case(name).arrays
    gsc.set_policy(pname)
    fused.SEGMENTS = "0"
    us, cinv, alphas, colors = (_t(a[k]) for k in ("us", "cinv2ds", "alphas", "colors"))
    depths, areas = _t(a["depths"]), _t(a["areas"])
    image, contrib, tau, ranges, gsid = gsc.splat(D.H, D.W, us, cinv, alphas, depths, colors, areas)
    assert np.array_equal(_host(contrib), D.reference(name, pname)["contrib"]), (name, pname, "contrib")
    return (D.H, D.W, us, cinv, alphas, depths, contrib, ranges, gsid), dict(areas=areas if pname == "forward_cpu" else None)


# ------------------------------------------------------------------------------------------------------ 1. one-tile lists
@pytest.mark.parametrize("C_", CHANNELS)
@pytest.mark.parametrize("pname", list(D.POLICIES))
@pytest.mark.parametrize("name", D.SETS)
def test_one_tile_lists(gpu, name, pname, C_):
    gsc, fused, imp = gpu
    c = D.case(name)
    ref, dist = F.reference(name, pname), F.distance(name, pname)
    feats_h = np.ascontiguousarray(F.case_feats(name)[:, :C_])
    gmap_h = np.ascontiguousarray(F.case_gmap(name)[:C_])
    args, kw = _splat(gsc, fused, name, pname)
    feats, gmap = _t(feats_h), _t(gmap_h)
    fmap = features.splat_features(*args, feats, **kw)
    gath = features.splat_gather(*args, gmap, **kw)
    torch.cuda.synchronize()
    assert tuple(fmap.shape) == (C_, D.H, D.W) and tuple(gath.shape) == (c.n, C_)
    got_m, got_g = _host(fmap), _host(gath)
    assert np.isfinite(got_m).all() and np.isfinite(got_g).all()
    # the map: every pixel
    err = np.abs(got_m.astype(np.float64) - ref["map"][:C_]).max(0)
    d = dist["map"][:C_].max(0)
    bound = np.maximum(F.pixel_floor(name, pname, feats_h), 2 * d)
    ratio = err / bound
    y, x = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    print("%-8s %-11s C=%-2d map    distance %.2g | error %.2g | error / bound %.2f"
          % (name, pname, C_, d.max(), err.max(), ratio.max()))
    assert ratio.max() <= 1, (name, pname, C_, "map: %d pixels beyond their bound; worst (y, x) = (%d, %d): error %.3g, "
                              "bound %.3g (distance %.3g)" % (int((ratio > 1).sum()), y, x, err[y, x], bound[y, x], d[y, x]))
    empty = ~_nonempty(c, pname)
    assert not _bits(got_m)[:, empty].any(), (name, pname, "pixels of empty tiles are not +0.0")
    # the gather: every row and channel
    want = ref["gather"][:, :C_]
    err = np.abs(got_g.astype(np.float64) - want)
    d = dist["gather"][:, :C_]
    bound = np.maximum(F.row_floor(name, pname)[:, :C_], 2 * d)
    ratio = np.where(err == 0, 0.0, err / np.where(bound == 0, 1e-300, bound))
    g, ch = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    print("%-8s %-11s C=%-2d gather distance %.2g | error %.2g | error / bound %.2f"
          % (name, pname, C_, d.max(), err.max(), ratio.max()))
    assert ratio.max() <= 1, (name, pname, C_, "gather: %d entries beyond their bound; worst: Gaussian %d = tile %d, entry "
                              "%d, channel %d: got %.9g, reference %.9g, error %.3g, bound %.3g (distance %.3g)"
                              % (int((ratio > 1).sum()), g, c.tile_of[g], c.pos_of[g], ch, got_g[g, ch], want[g, ch],
                                 err[g, ch], bound[g, ch], d[g, ch]))
    zero = B.reference(name, pname)["hits"] == 0
    assert not _bits(got_g)[zero].any(), (name, pname, "rows that hit nothing are not zero bit for bit")
    # two runs from zeroed buffers are bitwise equal: every Gaussian lies on one tile
    again = features.splat_gather(*args, gmap, **kw)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(_host(again)), _bits(got_g))
    # a second call into the same buffer: exactly twice the first
    assert features.splat_gather(*args, gmap, out=again, **kw) is again
    torch.cuda.synchronize()
    assert np.array_equal(_host(again), 2 * got_g)
    # the render is a pure function of its inputs
    assert np.array_equal(_bits(_host(features.splat_features(*args, feats, **kw))), _bits(got_m))
    if C_ == 3:
        # the colours as features: the draw pass's image, by k_draw's own rule
        colors = _t(c.arrays["colors"])
        img = _host(features.splat_features(*args, colors, **kw)).astype(np.float64)
        dref, ddist = D.reference(name, pname), D.distances(name, pname)
        err = np.abs(img - dref["image"]).max(0)
        ratio = err / np.maximum(D.pixel_floor(name, pname), 2 * ddist["image"])
        print("%-8s %-11s colours       distance %.2g | error %.2g | error / bound %.2f"
              % (name, pname, ddist["image"].max(), err.max(), ratio.max()))
        assert ratio.max() <= 1, (name, pname, "colours as features", float(ratio.max()))


# ---------------------------------------------------------------------------------------- 2. every output pixel is written
@pytest.mark.parametrize("name", ("lengths0", "lengths1"))
def test_every_output_pixel_is_written(gpu, name):
    gsc, fused, imp = gpu
    c = D.case(name)
    assert name != "lengths1" or not _nonempty(c, "gsplatcu").all()          # lengths1 has empty tiles
    args, kw = _splat(gsc, fused, name, "gsplatcu")
    n, H, W, rec, ranges, gsid, contrib = features._splat_args(*args, None, "test")
    feats = _t(np.ascontiguousarray(F.case_feats(name)[:, :9]))
    size, guard = 9 * H * W, 64
    buf = torch.full((size + guard,), float("nan"), dtype=torch.float32, device="cuda")
    lib = _featlib.load()
    P = lambda t: C.c_void_p(t.data_ptr())
    from easygaussiansplatting_amd._host import _pol, _stream
    rc = lib.egs_feature_render(n, W, H, P(rec), C.byref(_pol()), P(ranges), P(gsid), P(contrib), 0, 9, P(feats), P(buf),
                                _stream())
    assert rc == 0, lib.egs_feat_last_error_string()
    torch.cuda.synchronize()
    out = _host(buf)
    assert (H, W) == (40, 72) and np.isfinite(out[:size]).all()
    assert np.isnan(out[size:]).all(), "the guard band behind the map was written"
    ref = F.reference(name, "gsplatcu")["map"][:9]
    assert np.abs(out[:size].reshape(9, H, W) - ref).max() <= 1e-4


# ------------------------------------------------------------------------------------- 3. fused state, culled masked lists
def _tensors(sc):
    return tuple(_dev(x) for x in (sc.pws, sc.shs, sc.alphas, sc.scales, sc.rots))


def _rand(key, stream, shape, lo=-1.0):
    """float32 in [lo, 1] from scene.py's counter generator"""
    from easygaussiansplatting_amd import scene as S
    return (lo + (1.0 - lo) * S.uniform01(key, stream, shape)).astype(np.float32)


def _fused_state(gpu, cam_index=None):
    """the 20 000-Gaussian scene at 128 x 96 -> scene, camera, tensors, state of one fused forward"""
    gsc, fused, imp = gpu
    from easygaussiansplatting_amd import scene as S
    from easygaussiansplatting_amd.function import Camera
    sc = S.small_scene(20000, 128, 96, 48)
    cam = sc.cam if cam_index is None else S.ring_cameras(sc.cam, 2, radius=5.0)[cam_index]
    P = _tensors(sc)
    fused.SEGMENTS = "0"
    image, mask, state = fused.forward(*P, Camera.from_scene(cam, "cuda"), need_grad=False)
    state.patch_count()
    assert state.culled
    return sc, cam, P, state


def _oracle_inputs(gsc, cam, P, state):
    """the 2D tensors of the seven ops and the state's own lists, on the host (as test_fused_state_culled_lists)"""
    pws, shs, alphas, scales, rots = P
    W, H = cam.width, cam.height
    Rcw, tcw = _dev(cam.Rcw), _dev(cam.tcw)
    us, pcs, depths, _ = gsc.project(pws, Rcw, tcw, cam.fx, cam.fy, cam.cx, cam.cy, True)
    cov3 = gsc.computeCov3D(rots, scales, depths, True)[0]
    cov2 = gsc.computeCov2D(cov3, pcs, Rcw, depths, cam.fx, cam.fy, W, H, True)[0]
    cinv = gsc.inverseCov2D(cov2, depths, True)[0]
    torch.cuda.synchronize()
    return (W, H, _host(state.ranges), _host(state.gaussian_ids()), _host(us), _host(cinv), _host(alphas), None,
            _host(state.contrib))


def _gradcheck_columns(got, want, what):
    """the rule of tests/gradcheck.py per channel column: 2e-4 of the largest entry, median 1e-4 on entries >= 1 % of it"""
    got = np.asarray(got, np.float64); want = np.asarray(want, np.float64)
    assert got.shape == want.shape and np.isfinite(got).all()
    for ch in range(want.shape[1]):
        top = np.abs(want[:, ch]).max()
        err = np.abs(got[:, ch] - want[:, ch])
        big = np.abs(want[:, ch]) >= 1e-2 * top
        med = float(np.median(err[big] / np.abs(want[big, ch])))
        print("%s channel %d: largest error %.3g of the largest entry, median relative error %.3g on %d rows"
              % (what, ch, err.max() / top, med, int(big.sum())))
        assert top > 0 and err.max() <= 2e-4 * top, (what, ch, err.max() / top)
        assert med <= 1e-4, (what, ch, med)


def test_fused_state_culled_lists(gpu):
    gsc, fused, imp = gpu
    from oracle import gs_oracle as O
    sc, cam, P, state = _fused_state(gpu)
    W, H, C_ = cam.width, cam.height, 9
    feats_h, gmap_h = _rand(811, 1, (sc.n, C_)), _rand(811, 2, (C_, H, W))
    fmap = features.render_features(state, _t(feats_h))
    gath = features.gather_features(state, _t(gmap_h))
    torch.cuda.synchronize()
    assert tuple(fmap.shape) == (C_, H, W) and tuple(gath.shape) == (sc.n, C_)
    inputs = _oracle_inputs(gsc, cam, P, state)
    contrib = inputs[-1]
    rmap, rgath, _, near = F.image_walk(*inputs, O.POLICY_G, feats_h, gmap_h)
    # a condition on the inputs, on the reference alone: few pixels have an entry next to the skip threshold
    covered = contrib > 0
    n_near = int(((near > 0) & covered).sum())
    print("P = %d, %d covered pixels, %d of them with a near entry (%.2f %%), at most %d on one pixel"
          % (len(inputs[3]), int(covered.sum()), n_near, 100.0 * n_near / covered.sum(), int(near.max())))
    assert covered.sum() > 10000 and int((near > 0).sum()) <= 0.02 * covered.sum()
    fmax = float(np.abs(feats_h).max())
    askip = O.POLICY_G.alpha_skip
    err = np.abs(_host(fmap).astype(np.float64) - rmap).max(0)
    bound = 1e-4 * fmax + near * 2 * askip * (1 + F.SKIP_MARGIN) * fmax
    print("map: largest error %.3g (bound without a near entry %.3g), largest error / bound %.3f"
          % (err.max(), 1e-4 * fmax, (err / bound).max()))
    assert (err <= bound).all(), ("map", int((err > bound).sum()), float((err / bound).max()))
    _gradcheck_columns(_host(gath), rgath, "gather")
    # on the device's own outputs: an all-ones channel is the opacity 1 - final_tau, its gather the weight sum
    ones = features.render_features(state, torch.ones((sc.n, 1), device="cuda"))
    wsum = features.gather_features(state, torch.ones((1, H, W), device="cuda"))
    st = imp.from_state(state)
    torch.cuda.synchronize()
    ranges, tau = inputs[2], _host(state.final_tau).astype(np.float64)
    gx = (W + 15) // 16
    m = np.zeros((H, W), bool)
    for t in range(len(ranges)):
        if ranges[t, 1] > ranges[t, 0]:
            ty, tx = divmod(t, gx)
            m[16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16] = True
    e1 = np.abs(_host(ones)[0].astype(np.float64) - (1.0 - tau))[m].max()
    s = _host(st.sum).astype(np.float64)
    e2 = np.abs(_host(wsum)[:, 0].astype(np.float64) - s).max() / s.max()
    print("all-ones channel: |F - (1 - final_tau)| <= %.3g; gathered ones against importance.sum: %.3g of its largest" % (e1, e2))
    assert m.any() and e1 <= 1e-4
    assert s.max() > 0 and e2 <= 2e-4


# ---------------------------------------------------------------------------------------------- 4. adjointness on the device
def test_render_and_gather_are_adjoint_on_the_device(gpu):
    sc, cam, P, state = _fused_state(gpu)
    W, H, C_ = cam.width, cam.height, 9
    feats_h, gmap_h = _rand(812, 1, (sc.n, C_), lo=0.0), _rand(812, 2, (C_, H, W), lo=0.0)     # nothing cancels
    fmap = features.render_features(state, _t(feats_h))
    gath = features.gather_features(state, _t(gmap_h))
    torch.cuda.synchronize()
    lhs = float((gmap_h.astype(np.float64) * _host(fmap).astype(np.float64)).sum())
    rhs = float((_host(gath).astype(np.float64) * feats_h.astype(np.float64)).sum())
    print("<gmap, render(f)> = %.9g, <gather(gmap), f> = %.9g, relative difference %.3g" % (lhs, rhs, abs(lhs - rhs) / lhs))
    assert lhs > 0 and abs(lhs - rhs) <= 2e-4 * lhs


# ---------------------------------------------------------------------------------------------------------- 5. autograd
def test_autograd_through_feature_render(gpu):
    sc, cam, P, state = _fused_state(gpu)
    W, H, C_ = cam.width, cam.height, 9
    feats = _t(_rand(813, 1, (sc.n, C_))).requires_grad_()
    gmap = _t(_rand(813, 2, (C_, H, W))).requires_grad_()
    want = _host(features.gather_features(state, gmap))
    out = features.FeatureRender.apply(feats, state)
    assert out.requires_grad and tuple(out.shape) == (C_, H, W)
    assert torch.equal(out.detach(), features.render_features(state, feats))
    out.backward(gmap.detach())
    torch.cuda.synchronize()
    assert gmap.grad is None and not hasattr(state, "grad")
    _gradcheck_columns(_host(feats.grad), want, "feats.grad")
    features.FeatureRender.apply(feats, state).backward(gmap.detach())           # a fresh call accumulates
    torch.cuda.synchronize()
    _gradcheck_columns(_host(feats.grad), 2 * want.astype(np.float64), "feats.grad after two backward passes")
    # without a feature that requires a gradient there is nothing to differentiate
    assert not features.FeatureRender.apply(feats.detach(), state).requires_grad


# -------------------------------------------------------------------------------------------------------------- 6. lift
def test_lift_over_two_views(gpu):
    gsc, fused, imp = gpu
    from oracle import gs_oracle as O
    C_, eps = 4, 1e-8
    views = [_fused_state(gpu, i) for i in range(2)]
    sc = views[0][0]
    maps_h = [_rand(814 + i, 1, (C_, v[1].height, v[1].width)) for i, v in enumerate(views)]
    feats, seen = features.lift([v[3] for v in views], [_t(m) for m in maps_h], eps=eps)
    stats = imp.BlendStats(sc.n, "cuda")
    for v in views:
        imp.from_state(v[3], stats)
    torch.cuda.synchronize()
    assert tuple(feats.shape) == (sc.n, C_) and feats.dtype == torch.float32
    assert tuple(seen.shape) == (sc.n,) and seen.dtype == torch.bool
    num, den = np.zeros((sc.n, C_)), np.zeros(sc.n)
    ones_f = np.ones((sc.n, 1), np.float32)
    for (sc_, cam, P, state), m in zip(views, maps_h):
        planes = np.concatenate((m, np.ones_like(m[:1])), 0)
        g = F.image_walk(*_oracle_inputs(gsc, cam, P, state), O.POLICY_G, ones_f, planes)[1]
        num += g[:, :C_]; den += g[:, C_]
    # a condition on the reference alone: no denominator within a factor 2 of eps, so ``seen`` has no row to argue about
    assert not ((den > eps / 2) & (den < 2 * eps)).any()
    seen_h, hits = _host(seen), _host(stats.hits)
    assert 5000 < seen_h.sum() < sc.n
    assert np.array_equal(seen_h, hits > 0) and np.array_equal(seen_h, den >= eps)
    want = num[seen_h] / den[seen_h][:, None]
    _gradcheck_columns(_host(feats)[seen_h], want, "lifted features")
    assert not _bits(_host(feats))[~seen_h].any(), "unseen rows are not zero bit for bit"


# ------------------------------------------------------------------- 9. the all-ones gather beside importance's sum
@pytest.mark.parametrize("pname", list(D.POLICIES))
@pytest.mark.parametrize("name", D.SETS)
def test_all_ones_gather_is_the_weight_sum(gpu, name, pname):
    """``splat_gather`` of one all-ones channel against ``splat_weights``' ``sum``, row by row.  k_feature_gather and
    k_blend_weights stage an entry, form its exponent and reduce a group of four with the same code
    (csrc/egs_list_walk.h, total_of4), fmaf(w, 1, acc) is acc + w, and every Gaussian of these sets lies on one tile
    (one atomic per row), so the two columns were expected to be equal bit for bit.  They are not: on MI355X they
    differ on 0 .. 139 rows of a set (none on reach / gsplatcu), by at most 2 ulps.  The staging and the exponent ARE
    the same instructions in both kernels; the difference is in the accumulation behind them.  k_blend_weights'
    ``ws += w`` is contracted with ``w = tau alpha'`` into one v_fmac_f32 (ws = fma(tau, alpha', ws), one rounding) --
    as it was before the walk was shared: its words are the same bit for bit -- while the gather multiplies the ROUNDED
    w (v_mul_f32) with the pixel's gradient (acc = fma(w, 1, acc), two roundings).  So the rows are held to the rule of
    tests/test_gpu_blend_weights.py for ``sum`` instead: |gather - sum| <= max(floor, 2 x distance) of
    tests/blend_weights_ref.py.  Rows that hit nothing are zero bit for bit in both."""
    gsc, fused, imp = gpu
    ref, dist, floor = B.reference(name, pname), B.distance(name, pname), B.row_floor(name, pname)
    args, kw = _splat(gsc, fused, name, pname)
    st = imp.splat_weights(*args, **kw)
    gath = features.splat_gather(*args, torch.ones((1, D.H, D.W), device="cuda"), **kw)
    torch.cuda.synchronize()
    got, want = _host(gath), _host(st.sum)
    assert tuple(got.shape) == (D.case(name).n, 1) and want.any()
    got = got[:, 0]
    ulps = np.abs(_bits(got).astype(np.int64) - _bits(want).astype(np.int64))
    print("%-8s %-11s gather != sum on %d of %d rows, largest difference %d ulps"
          % (name, pname, int((ulps > 0).sum()), ulps.size, int(ulps.max())))
    zero = ref["hits"] == 0
    assert not _bits(got)[zero].any() and not _bits(want)[zero].any()
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    bound = np.maximum(floor["sum"], 2 * dist["sum"])
    bad = np.nonzero(err > bound)[0]
    assert bad.size == 0, (name, pname, "%d rows beyond their bound; first: Gaussian %d: gather %.9g, sum %.9g, bound %.3g"
                           % (bad.size, bad[0], got[bad[0]], want[bad[0]], bound[bad[0]]))


# ------------------------------------------------------------------------------------------------------------ 7. n == 0
def test_no_gaussians(gpu):
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device="cuda")
    args = (40, 72, z(0, 2), z(0, 3), z(0), z(0), z(40, 72, dt=torch.int32), z(15, 2, dt=torch.int32), z(0, dt=torch.int32))
    fmap = features.splat_features(*args, z(0, 5))
    gath = features.splat_gather(*args, torch.ones((5, 40, 72), device="cuda"))
    torch.cuda.synchronize()
    assert tuple(fmap.shape) == (5, 40, 72) and not _bits(_host(fmap)).any()
    assert tuple(gath.shape) == (0, 5) and gath.dtype == torch.float32


# ---------------------------------------------------------------------------------------- 8. shapes and dtypes are checked
def test_python_refuses_wrong_shapes_and_dtypes(gpu):
    sc, cam, P, state = _fused_state(gpu)
    W, H = cam.width, cam.height
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device="cuda")
    for bad in (z(sc.n - 1, 3), z(sc.n), z(sc.n, 3, dt=torch.float64), z(sc.n, 3, dt=torch.float16), z(sc.n, 0),
                z(sc.n, 4097)):
        with pytest.raises(ValueError):
            features.render_features(state, bad)
    for bad in (z(3, H, W + 1), z(3, H - 1, W), z(H, W), z(3, H, W, dt=torch.float64), z(0, H, W)):
        with pytest.raises(ValueError):
            features.gather_features(state, bad)
    with pytest.raises(ValueError):
        features.gather_features(state, z(3, H, W), out=z(sc.n, 4))
    with pytest.raises(ValueError):
        features.gather_features(state, z(3, H, W), out=z(sc.n, 6)[:, ::2])     # not contiguous: would add to a copy
    with pytest.raises(ValueError):
        features.lift([state], [z(3, H, W + 1)])
    # a non-contiguous feature tensor is accepted (copied), as the reference's .contiguous()
    f = _t(_rand(815, 1, (sc.n, 6)))
    assert torch.equal(features.render_features(state, f[:, ::2]), features.render_features(state, f[:, ::2].contiguous()))
