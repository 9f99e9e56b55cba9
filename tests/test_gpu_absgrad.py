"""Absolute screen-space gradients on the GPU (``RenderOptions.absgrad``, ``EGS_BWD_ABSGRAD``): the ABS
instances of k_draw_bwd (unsplit and segment walks) against the float64 restatement ``tests/absgrad_ref.py``, the signed
outputs of the same call against the oracle, every path that delivers ``us.absgrad``, and the trainer's statistic.

Every parity check uses the suite's rule (tests/gradcheck.py) with its defaults (near_frac = 0.02 included): the absolute sums have no cancellation,
so no wider bound is justified.  As in the like-for-like gradient tests the restatement is fed the device's own
``contrib`` / ``final_tau`` and the oracle's stages in float32; threshold-flip rows are named by ``O.draw_backward``."""
import ctypes as C

import numpy as np
import pytest

from easygaussiansplatting_amd import scene as S
from oracle import gs_oracle as O
from tests.absgrad_ref import draw_backward_abs
from tests.gradcheck import assert_grad_close, assert_grad_close_flips

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NAMES = ("pws", "shs", "alphas", "scales", "rots")


@pytest.fixture(scope="module")
def fx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from easygaussiansplatting_amd import _lib, fused, gsplatcu
    from easygaussiansplatting_amd.function import GSFunction
    gsplatcu.set_policy("gsplatcu")
    GSFunction.mode = "fused"
    lib = _lib.load()
    before = (C.c_int * 2)()
    _lib.check(lib.egs_seg_config(0, 0, before))
    keep = (fused.SEGMENTS, fused.SEG_SPECULATE)
    yield fused, lib
    fused.SEGMENTS, fused.SEG_SPECULATE = keep
    _lib.check(lib.egs_seg_config(before[0], before[1], None))


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def leaves(sc):
    P = dict(pws=dev(sc.pws), shs=dev(sc.shs), alphas=dev(sc.alphas).reshape(-1, 1), scales=dev(sc.scales),
             rots=dev(sc.rots))
    for p in P.values():
        p.requires_grad_(True)
    return P


def render(sc, cam, dl, absgrad, renders=1, **opts):
    """forward + backward through GSFunction -> dict(image, grads incl. "us", absgrad or None)"""
    from easygaussiansplatting_amd.function import GSFunction, RenderOptions
    for _ in range(renders):
        P = leaves(sc)
        us0 = torch.zeros((sc.n, 2), device="cuda", requires_grad=True)
        image, mask = GSFunction.apply(*[P[k] for k in NAMES], us0, cam, RenderOptions(absgrad=absgrad, **opts))
        image.backward(dl)
    if absgrad:
        assert us0.absgrad.shape == (sc.n, 2) and us0.absgrad.dtype == torch.float32
    else:
        assert not hasattr(us0, "absgrad")
    return dict(image=host(image), mask=host(mask), grads={k: host(v.grad) for k, v in P.items()} | {"us": host(us0.grad)},
                absgrad=host(us0.absgrad) if absgrad else None)


def state_of(fused, sc, cam, antialiased=False):
    """contrib / final_tau / lists of an identical render (the same kernels)"""
    with torch.no_grad():
        img, _, st = fused.forward(dev(sc.pws), dev(sc.shs), dev(sc.alphas).reshape(-1, 1), dev(sc.scales), dev(sc.rots),
                                   cam, need_grad=True, antialiased=antialiased)
    return dict(contrib=host(st.contrib), tau=host(st.final_tau), ranges=host(st.ranges), ids=host(st.gaussian_ids()),
                seg=st.seg is not None)


def reference(sc, st, dl, tiles=None, parallel=False, u_ulps=None):
    """(dus, dus_abs, near, rows): the restatement and the oracle's walk over ``tiles`` from the device's contrib /
    final_tau and the oracle's stages in float32 (like for like), the threshold-flip rows named by the oracle with the
    margins of the like-for-like tests; rows = the Gaussians whose every patch lies in ``tiles`` (all of them: None)"""
    from tests.test_gpu_parity import LIKE_MARGIN, LIKE_U_ULPS, _oracle_2d, complete_inside
    W, H = sc.cam.width, sc.cam.height
    u_ulps = LIKE_U_ULPS if u_ulps is None else u_ulps
    q_us, q_ci, q_col, _, _ = _oracle_2d(sc, sc.cam, dtype=np.float32)
    a64 = sc.alphas.astype(np.float64)
    d64 = np.asarray(dl, np.float64)
    if parallel:            # (the full-size scenes: the tiles dealt to the host's cores)
        from tests.absgrad_ref import draw_backward_abs_tiles
        from tests.oracle_parallel import draw_backward_tiles
        o = draw_backward_tiles(W, H, st["ranges"], st["ids"], q_us, q_ci, a64, q_col, st["contrib"], st["tau"], d64,
                                tiles=tiles, near_margin=LIKE_MARGIN, near_u_ulps=u_ulps, procs=16)
        signed, near = o[0], o[4]
        dus, dus_abs = draw_backward_abs_tiles(W, H, st["ranges"], st["ids"], q_us, q_ci, a64, q_col, st["contrib"],
                                               st["tau"], d64, tiles)
    else:
        near = np.zeros(sc.n, bool)
        signed = O.draw_backward(W, H, st["ranges"], st["ids"], q_us, q_ci, a64, q_col, st["contrib"], st["tau"], d64,
                                 None, O.POLICY_G, tiles=tiles, near_out=near, near_margin=LIKE_MARGIN,
                                 near_u_ulps=u_ulps)[0]
        dus, dus_abs = draw_backward_abs(W, H, st["ranges"], st["ids"], q_us, q_ci, a64, q_col, st["contrib"], st["tau"],
                                         d64, None, O.POLICY_G, tiles=tiles)
    assert np.abs(dus - signed).max() <= 1e-12 * np.abs(signed).max()
    rows = slice(None) if tiles is None else complete_inside(st["ids"], st["ranges"], tiles, sc.n)
    return signed, dus_abs, near, rows


# ---------------------------------------------------------------------------------- parity at test scale
_CASES = {"256x256": (3000, 256, 256, 11), "250x170": (2500, 250, 170, 12)}
_cache = {}


def small_case(fused, tag):
    """one scene per shape: the two runs (with and without the flag) and the float64 references, computed once"""
    if tag not in _cache:
        from easygaussiansplatting_amd.function import Camera
        n, W, H, seed = _CASES[tag]
        sc = S.small_scene(n, W, H, 12, seed=seed)
        cam = Camera.from_scene(sc.cam)
        dl = S.normal(3, 31, (3, H, W)).astype(np.float32) / (3 * H * W)
        fused.SEGMENTS = "0"
        plain = render(sc, cam, dev(dl), False)
        flag = render(sc, cam, dev(dl), True)
        st = state_of(fused, sc, cam)
        assert not st["seg"]
        _cache[tag] = (sc, cam, dl, plain, flag, st, reference(sc, st, dl))
    return _cache[tag]


@pytest.mark.parametrize("tag", list(_CASES))
def test_absgrad_equals_the_float64_restatement(fx, tag):
    """256 x 256 and the odd 250 x 170 (ragged right and bottom tiles): sum |dL/du| of every Gaussian by the default rule"""
    fused, _ = fx
    sc, cam, dl, plain, flag, st, (signed, dus_abs, near, rows) = small_case(fused, tag)
    r = assert_grad_close_flips(flag["absgrad"], dus_abs, near, "absgrad:" + tag)
    assert r["n_big"] > 100, r
    # the statistic bounds the signed gradient of the same call (float32 sums: a few ulps of the larger one)
    assert (flag["absgrad"] >= np.abs(flag["grads"]["us"]) - 1e-5 * flag["absgrad"].max()).all()
    assert (flag["absgrad"] >= 0).all() and (flag["absgrad"][~flag["mask"]] == 0).all()


@pytest.mark.parametrize("tag", list(_CASES))
def test_signed_outputs_are_what_they_are_without_the_flag(fx, tag):
    """every other output of the backward: against the same oracle by the same rule with and without the flag, and the
    two runs against each other (not bit-equality: the instances may contract FMAs differently)"""
    from tests.test_gpu_parity import _oracle_param_grads
    fused, _ = fx
    sc, cam, dl, plain, flag, st, (signed, dus_abs, near, rows) = small_case(fused, tag)
    assert np.array_equal(plain["image"], flag["image"])
    o_img, o_mask, o_g = _oracle_param_grads(sc, sc.cam, dl.astype(np.float64))
    for run, label in ((plain, "plain"), (flag, "absgrad")):
        for k in NAMES + ("us",):
            assert_grad_close(run["grads"][k], o_g[k], "absgrad_signed[%s/%s]:%s" % (tag, label, k))
        assert_grad_close_flips(run["grads"]["us"], signed, near, "absgrad_signed_like[%s/%s]:us" % (tag, label))
    for k in NAMES + ("us",):
        assert_grad_close(flag["grads"][k], plain["grads"][k], "absgrad_vs_plain[%s]:%s" % (tag, k))


def test_records_without_the_flag_keep_their_pads_zero(fx):
    fused, lib = fx
    from easygaussiansplatting_amd.function import Camera
    sc = S.small_scene(3000, 250, 170, 12, seed=12)
    cam = Camera.from_scene(sc.cam)
    dl = dev(S.normal(3, 31, (3, 170, 250)).astype(np.float32) / (3 * 170 * 250))
    args = [dev(sc.pws), dev(sc.shs), dev(sc.alphas).reshape(-1, 1), dev(sc.scales), dev(sc.rots)]
    fused.SEGMENTS = "0"
    for absgrad in (False, True):
        img, mask, st = fused.forward(*args, cam, need_grad=True)
        rec = st.gpack
        out = fused.backward(*args, cam, st, dl, absgrad=absgrad)
        torch.cuda.synchronize()
        assert len(out) == (7 if absgrad else 6)
        assert bool(rec[:, :9].any())
        if absgrad:
            assert torch.equal(rec[:, 10:12], out[-1]) and bool((out[-1] > 0).any())
        else:
            assert not bool(rec[:, 9:12].any())
    # a render with extras has no ABS instance
    img, mask, st, _, _ = fused.forward(*args, cam, need_grad=True, extras=fused.Extras(True, False, None))
    with pytest.raises(ValueError, match="absgrad"):
        fused.backward(*args, cam, st, dl, absgrad=True)


def test_output_between_guard_bands(fx):
    """egs_grad_records_absgrad writes every row of its [N,2] output and nothing else (an N that is no multiple of 256)"""
    fused, lib = fx
    from easygaussiansplatting_amd import _lib
    n, G = 3001, 4096
    rec = torch.arange(n * 12, dtype=torch.float32, device="cuda").reshape(n, 12)
    base = torch.full((2 * G + n * 8,), 0xA5, dtype=torch.uint8, device="cuda")
    out = base[G:G + n * 8].view(torch.float32).reshape(n, 2)
    _lib.check(lib.egs_grad_records_absgrad(n, rec.data_ptr(), out.data_ptr(), None))
    torch.cuda.synchronize()
    assert bool((base[:G] == 0xA5).all()) and bool((base[G + n * 8:] == 0xA5).all())
    assert torch.equal(out, rec[:, 10:12])


# ---------------------------------------------------------------------------------- forced segment path
def _seg_scene(reset):
    sc = S.small_scene(30000, 64, 48, 12, seed=5)
    sc.scales[:] = sc.scales * 2.2
    if reset:
        sc.alphas[:] = np.minimum(sc.alphas, 0.01)
    return sc


@pytest.mark.parametrize("seg", [(64, 64), (128, 128)])
@pytest.mark.parametrize("reset", [False, True])
def test_forced_segments(fx, seg, reset):
    """k_draw_bwd_seg_abs on a dense small scene, opaque and after reset_alpha, at first sight and with history: equal to
    the unsplit kernel's statistic to the segment suite's bound (2e-4 of the maximum) and to the restatement by the default
    rule, every Gaussian of the scene (4 x 3 tiles)"""
    fused, lib = fx
    from easygaussiansplatting_amd import _lib
    from easygaussiansplatting_amd.function import Camera
    sc = _seg_scene(reset)
    W, H = sc.cam.width, sc.cam.height
    dl = S.normal(3, 21, (3, H, W)).astype(np.float32) / (3 * H * W)
    fused.SEGMENTS = "0"
    ref = render(sc, Camera.from_scene(sc.cam), dev(dl), True)
    lens = np.diff(state_of(fused, sc, Camera.from_scene(sc.cam))["ranges"], axis=1)
    assert lens.max() > 3 * seg[0], int(lens.max())
    fused.SEGMENTS = "1"
    _lib.check(lib.egs_seg_config(seg[0], seg[1], None))
    for renders in (1, 3):
        cam = Camera.from_scene(sc.cam)
        got = render(sc, cam, dev(dl), True, renders)
        st = state_of(fused, sc, cam)
        assert st["seg"]
        label = "absgrad_seg%d/%s/r%d" % (seg[0], "reset" if reset else "opaque", renders)
        e = np.abs(got["absgrad"] - ref["absgrad"]).max() / np.abs(ref["absgrad"]).max()
        print(label, "segments vs unsplit: %.2e of the maximum" % e)
        assert e <= 2e-4, (label, e)
        signed, dus_abs, near, rows = reference(sc, st, dl)
        r = assert_grad_close_flips(got["absgrad"], dus_abs, near, label)
        assert r["n_big"] > 100, r
        assert_grad_close_flips(got["grads"]["us"], signed, near, label + ":us")


# ---------------------------------------------------------------------------------- the other ways in and out
def _raw_leaves(sc):
    a = torch.from_numpy(sc.alphas.astype(np.float32)).clamp(1e-4, 1 - 1e-4)
    raw = dict(pws=dev(sc.pws), low_shs=dev(sc.shs[:, :3]), high_shs=dev(sc.shs[:, 3:]),
               alphas_raw=torch.log(a / (1 - a)).reshape(-1, 1).cuda(), scales_raw=torch.log(dev(sc.scales)),
               rots_raw=dev(sc.rots) * 1.7)
    return {k: v.clone().requires_grad_(True) for k, v in raw.items()}


@pytest.mark.parametrize("aa", [False, True])
def test_function_variants_deliver_the_same_statistic(fx, aa):
    """GSRawFunction on the raw tensors == GSFunction on the activated ones (also anti-aliased); the pose functions give
    what the plain ones give"""
    fused, _ = fx
    from easygaussiansplatting_amd.function import (Camera, GSFunction, GSPoseFunction, GSRawFunction, GSRawPoseFunction,
                                                    RenderOptions)
    sc = S.small_scene(3000, 250, 170, 12, seed=12)
    cam = Camera.from_scene(sc.cam)
    cam.twc = (-(cam.Rcw.t() @ cam.tcw)).contiguous()       # the pose nodes' camera centre, for all four
    dl = dev(S.normal(3, 31, (3, 170, 250)).astype(np.float32) / (3 * 170 * 250))
    o = RenderOptions(absgrad=True, antialiased=aa)
    fused.SEGMENTS = "0"
    got = {}
    for name in ("act", "raw", "act_pose", "raw_pose"):
        p = _raw_leaves(sc)
        us = torch.zeros((sc.n, 2), device="cuda", requires_grad=True)
        R = cam.Rcw.clone().requires_grad_(True); t = cam.tcw.clone().requires_grad_(True)
        act = (p["pws"], torch.cat((p["low_shs"], p["high_shs"]), 1), torch.sigmoid(p["alphas_raw"]),
               torch.exp(p["scales_raw"]), torch.nn.functional.normalize(p["rots_raw"]))
        rawt = tuple(p[k] for k in ("pws", "low_shs", "high_shs", "alphas_raw", "scales_raw", "rots_raw"))
        if name == "act":
            img = GSFunction.apply(*act, us, cam, o)[0]
        elif name == "raw":
            img = GSRawFunction.apply(*rawt, us, cam, o)[0]
        elif name == "act_pose":
            img = GSPoseFunction.apply(*act, us, R, t, cam, o)[0]
        else:
            img = GSRawPoseFunction.apply(*rawt, us, R, t, cam, o)[0]
        img.backward(dl)
        if "pose" in name:
            assert R.grad is not None and bool(R.grad.abs().max() > 0)
        got[name] = host(us.absgrad)
        assert bool((us.absgrad >= us.grad.abs() - 1e-5 * us.absgrad.max()).all())
    # the pose nodes run the plain nodes' kernels on the same inputs: the default rule, nothing excused
    assert_grad_close(got["act_pose"], got["act"], "absgrad_variants[aa=%d]:act_pose" % aa)
    assert_grad_close(got["raw_pose"], got["raw"], "absgrad_variants[aa=%d]:raw_pose" % aa)
    assert_grad_close(got["raw"], got["act"], "absgrad_variants[aa=%d]:raw" % aa)


def test_accumulate_overwrites_the_statistic_and_sums_the_gradients(fx):
    """two views with accumulate=True: each backward leaves ITS view's us.absgrad, the leaves' .grad is the sum"""
    fused, _ = fx
    from easygaussiansplatting_amd.function import Camera, GSFunction, RenderOptions
    sc = S.small_scene(3000, 200, 120, 12, seed=9)
    cams = [Camera.from_scene(c) for c in S.ring_cameras(sc.cam, 2, radius=5.0)]
    dl = dev(S.normal(3, 33, (3, 120, 200)).astype(np.float32) / (3 * 120 * 200))
    fused.SEGMENTS = "0"
    single = []
    for c in cams:
        r = render(sc, c, dl, True)
        single.append(r)
    P = leaves(sc)
    us = torch.zeros((sc.n, 2), device="cuda", requires_grad=True)
    o = RenderOptions(absgrad=True, accumulate=True)
    seen = []
    for c in cams:
        us.grad = None
        GSFunction.apply(*[P[k] for k in NAMES], us, c, o)[0].backward(dl)
        seen.append(host(us.absgrad))
    for k, (a, b) in enumerate(zip(seen, single)):
        assert_grad_close(a, b["absgrad"], "absgrad_accumulate:view%d" % k)
    assert np.abs(seen[0] - seen[1]).max() > 0.1 * seen[0].max()          # two different views
    for k in NAMES:
        assert_grad_close(host(P[k].grad), single[0]["grads"][k] + single[1]["grads"][k], "absgrad_accumulate:" + k)


def test_redone_render_and_chunked_phases(fx):
    """a render whose draw was redone after an enqueue-ahead overflow, and the chunked backward (phase 1 + chunks of phase
    2, as dist_views.ChunkedExchange drives it): the same us.absgrad as the validated one-phase render"""
    fused, _ = fx
    from easygaussiansplatting_amd.function import Camera, GSFunction, RenderOptions
    n, W, H = 6000, 200, 120
    sc = S.small_scene(n, W, H, 12, seed=4)
    cam = Camera.from_scene(sc.cam)
    dl = dev(S.normal(3, 35, (3, H, W)).astype(np.float32) / (3 * H * W))
    fused.SEGMENTS = "0"
    ref = render(sc, cam, dl, True, renders=2)
    cap = fused._ctx(torch.device("cuda", 0)).capacity
    assert cap[(n, W, H)] > 1000
    cap[(n, W, H)] = 64                                   # far too small: the draw stage is redone
    redone = render(sc, cam, dl, True)
    assert cap[(n, W, H)] > 1000
    assert np.array_equal(redone["image"], ref["image"])
    assert_grad_close(redone["absgrad"], ref["absgrad"], "absgrad_redo", tol_max=2e-5, med_rel=1e-5, max_rel=1e-3)

    from easygaussiansplatting_amd.dist_views import ChunkedExchange

    class Counted(ChunkedExchange):          # the real exchange (one process: nothing to reduce), its chunks counted
        got = 0

        def on_chunk(self, tensors):
            self.got += 1
            assert len(tensors) == 5 and all(t.shape[0] <= 2048 for t in tensors)
            return super().on_chunk(tensors)
    hook = Counted(world=1, chunks=3).begin_step()
    P = leaves(sc)
    us = torch.zeros((n, 2), device="cuda", requires_grad=True)
    GSFunction.apply(*[P[k] for k in NAMES], us, cam, RenderOptions(absgrad=True, exchange=hook))[0].backward(dl)
    assert hook.got == 3 and hook.backwards == 1
    hook.finish()
    assert_grad_close(host(us.absgrad), ref["absgrad"], "absgrad_chunked", tol_max=2e-5, med_rel=1e-5, max_rel=1e-3)
    for k in NAMES:
        assert_grad_close(host(P[k].grad), ref["grads"][k], "absgrad_chunked:" + k, tol_max=2e-5, med_rel=1e-5,
                          max_rel=1e-3)


# ---------------------------------------------------------------------------------- trainer
def _trainer(absgrad, **kw):
    from easygaussiansplatting_amd.function import Camera, render as render_ops
    from easygaussiansplatting_amd.trainer import Trainer
    sc = S.small_scene(3000, 96, 64, 48, seed=17)
    cams = [Camera.from_scene(c) for c in S.ring_cameras(sc.cam, 4, radius=5.0)]
    with torch.no_grad():
        gts = [render_ops(dev(sc.pws), dev(sc.shs), dev(sc.alphas), dev(sc.scales), dev(sc.rots), c)[0] for c in cams]
    start = S.small_scene(3000, 96, 64, 48, seed=17)
    start.shs[:, :3] += 0.8 * S.normal(5, 3, (3000, 3)).astype(np.float32)
    start.alphas[:] = np.clip(start.alphas * 0.6, 0.05, 0.9)
    return Trainer(start, cams, gts, max_steps=200, scene_size=4.0, absgrad=absgrad, **kw)


def test_trainer_gathers_the_absolute_statistic(fx):
    """one step on one parameter state: grad_accum == the masked norms of separately computed dus_abs, row-wise >= that
    of the signed trainer; the parameters after the step agree (the statistic does not touch the gradients)"""
    fused, _ = fx
    from easygaussiansplatting_amd.function import GSRawFunction, RenderOptions
    from easygaussiansplatting_amd.loss import gau_loss_with_grad
    fused.SEGMENTS = "0"
    views = [0, 1, 2, 3]
    ta, ts = _trainer(True), _trainer(False)
    want = torch.zeros(3000, device="cuda")
    for v in views:       # the statistic of every view, computed apart from the trainer on its starting state
        p = {k: t.detach().clone().requires_grad_(True) for k, t in ta.params.items()}
        us = torch.zeros((3000, 2), device="cuda", requires_grad=True)
        image, mask = GSRawFunction.apply(*[p[k] for k in ta._KEYS], us, ta.cams[v], RenderOptions(absgrad=True))
        _, dimage = gau_loss_with_grad(image.detach(), ta.gts[v], grad_scale=1.0)
        image.backward(dimage)
        g = torch.norm(us.absgrad, dim=-1)
        want += torch.where(mask, g, torch.zeros_like(g))
    ta.step(views); ts.step(views)
    assert_grad_close(host(ta.grad_accum), host(want), "absgrad_trainer:grad_accum")
    a, s = host(ta.grad_accum), host(ts.grad_accum)
    assert (a >= s - 1e-5 * a.max()).all() and a.sum() > 1.05 * s.sum()
    assert torch.equal(ta.vis_count, ts.vis_count)
    for k in ta._KEYS:
        assert_grad_close(host(ta.params[k]), host(ts.params[k]), "absgrad_trainer:" + k)


@pytest.mark.parametrize("segments", ["0", "1"])
def test_trainer_densifies_on_the_absolute_statistic(fx, segments):
    fused, lib = fx
    from easygaussiansplatting_amd import _lib
    fused.SEGMENTS = segments
    if segments == "1":
        _lib.check(lib.egs_seg_config(64, 64, None))
    tr = _trainer(True, grad_threshold=1e-6)
    assert tr.density.grad_threshold == 1e-6
    losses = [tr.step([0, 1, 2, 3]) for _ in range(6)]
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    assert bool(torch.isfinite(tr.grad_accum).all()) and float(tr.grad_accum.max()) > 0
    tr.densify()
    n = tr.params["pws"].shape[0]
    assert n > 0 and tr.grad_accum.shape[0] == n and not bool(tr.grad_accum.any())
    assert np.isfinite(tr.step([0, 1, 2, 3]))


# ---------------------------------------------------------------------------------- full size
@pytest.fixture(scope="module")
def big(fx):
    return S.big_scene()


def test_full_size_bench_scene(fx, big):
    """1 M Gaussians at 1080p: the Gaussians complete inside three 6 x 4-tile windows (centre, ragged bottom row, longest
    list) against the restatement, the signed dL/du of the same call against O.draw_backward, by the default rule"""
    fused, _ = fx
    from easygaussiansplatting_amd.function import Camera
    from tests.test_gpu_parity import gradient_windows
    sc = big
    W, H = sc.cam.width, sc.cam.height
    cam = Camera.from_scene(sc.cam)
    dl = S.normal(8, 1, (3, H, W)).astype(np.float32) / (H * W)
    fused.SEGMENTS = "0"
    got = render(sc, cam, dev(dl), True)
    st = state_of(fused, sc, cam)
    sub = gradient_windows(st["ranges"], (W + 15) // 16, (H + 15) // 16)
    signed, dus_abs, near, rows = reference(sc, st, dl, sub, parallel=True)
    assert rows.size > 2000, rows.size
    r = assert_grad_close_flips(got["absgrad"][rows], dus_abs[rows], near[rows], "absgrad_full_size")
    assert r["n_big"] > 100, r
    assert_grad_close_flips(got["grads"]["us"][rows], signed[rows], near[rows], "absgrad_full_size:us")
    vis = got["mask"] & (np.linalg.norm(got["grads"]["us"], axis=1) > 0)
    ratio = np.linalg.norm(got["absgrad"][vis], axis=1) / np.linalg.norm(got["grads"]["us"][vis], axis=1)
    print("bench scene: ||dus_abs|| / ||dus|| median %.2f, 90th percentile %.2f over %d visible Gaussians"
          % (np.median(ratio), np.percentile(ratio, 90), int(vis.sum())))
    assert (ratio >= 1 - 1e-4).all()


def test_full_size_skewed_scene_segments(fx):
    """scene.skewed_scene right after reset_alpha at the production setting: the segment path's statistic equals the
    unsplit kernels' to the segment suite's bound, and the restatement's on the Gaussians complete inside the windows"""
    fused, _ = fx
    from easygaussiansplatting_amd.function import Camera
    from tests.test_gpu_parity import gradient_windows
    sc = S.skewed_scene(reset_alpha=True)
    W, H = sc.cam.width, sc.cam.height
    dl = S.normal(3, 22, (3, H, W)).astype(np.float32) / (3 * H * W)
    fused.SEGMENTS = "0"
    ref = render(sc, Camera.from_scene(sc.cam), dev(dl), True)
    fused.SEGMENTS = "auto"
    cam = Camera.from_scene(sc.cam)
    got = render(sc, cam, dev(dl), True, renders=2)
    st = state_of(fused, sc, cam)
    assert st["seg"]
    e = np.abs(got["absgrad"] - ref["absgrad"]).max() / np.abs(ref["absgrad"]).max()
    print("skewed scene: segments vs unsplit %.2e of the maximum" % e)
    assert e <= 2e-4, e
    sub = gradient_windows(st["ranges"], (W + 15) // 16, (H + 15) // 16)      # (test_gpu_round5_vs_oracle.py's windows)
    assert int(np.argmax(np.diff(st["ranges"], axis=1))) in sub
    # (the margin of that file's dloss_dus check on this scene: the oracle's flat 1e-4, no per-pixel widening)
    signed, dus_abs, near, rows = reference(sc, st, dl, sub, parallel=True, u_ulps=0.0)
    assert rows.size > 1000, rows.size
    assert_grad_close_flips(got["absgrad"][rows], dus_abs[rows], near[rows], "absgrad_skewed_seg")
    vis = got["mask"] & (np.linalg.norm(got["grads"]["us"], axis=1) > 0)
    ratio = np.linalg.norm(got["absgrad"][vis], axis=1) / np.linalg.norm(got["grads"]["us"][vis], axis=1)
    print("skewed scene: ||dus_abs|| / ||dus|| median %.2f, 90th percentile %.2f over %d visible Gaussians"
          % (np.median(ratio), np.percentile(ratio, 90), int(vis.sum())))
