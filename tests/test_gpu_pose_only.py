"""The pose-only backward pass (``RenderOptions(pose_only=True)`` / ``EGS_BWD_POSE_ONLY``): against the
float64 reference of tests/pose_ref.py, against the full pose node, through the raw C ABI with NaN-filled and NULL
per-Gaussian outputs, on the sizes where the reduction can go wrong, on both SH paths, on the segment path, and the
host layer (``fused.backward``, autograd, ``pose.refine_pose``)."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

from easygaussiansplatting_amd import scene as S
from oracle import gs_oracle as O
from tests import aa_ref
from tests.pose_ref import pose_vjp
from tests.test_gpu_pose_grad import (NAMES, SCENES, assert_pose_close, dev, host, leaves, pose_leaves, posed,
                                      single_tile_scene, term_scale, weights)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

RAW = ("pws", "low_shs", "high_shs", "alphas_raw", "scales_raw", "rots_raw")
BG = (0.2, 0.5, 0.9)


@pytest.fixture(scope="module")
def gsc():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from easygaussiansplatting_amd import gsplatcu
    gsplatcu.set_policy("gsplatcu")
    yield gsplatcu
    gsplatcu.set_policy("gsplatcu")


def raw_leaves(sc):
    a = sc.alphas.astype(np.float64)
    p = dict(pws=dev(sc.pws), low_shs=dev(sc.shs[:, :3]), high_shs=dev(sc.shs[:, 3:]),
             alphas_raw=dev(np.log(a / (1 - a))).reshape(-1, 1), scales_raw=dev(np.log(sc.scales.astype(np.float64))),
             rots_raw=dev(sc.rots))
    for v in p.values():
        v.requires_grad_(True)
    return p


def options(mode, pose_only):
    from easygaussiansplatting_amd.function import RenderOptions
    kw = dict(extras=dict(depth=True, alpha=True, background=BG), aa=dict(antialiased=True)).get(mode, {})
    return RenderOptions(pose_only=pose_only, **kw)


def run(sc, mode, pose_only, wts, raw=False, p=None):
    """backward of <Wi,image> (+ <Wd,depth> + <Wa,alpha> with extras) -> (dRcw, dtcw as float64 arrays, leaves, out)"""
    from easygaussiansplatting_amd.function import Camera, GSPoseFunction, GSRawPoseFunction
    cam = Camera.from_scene(sc.cam)
    R, t = pose_leaves(sc)
    us = torch.zeros((sc.n, 2), device="cuda", requires_grad=True)
    opts = options(mode, pose_only)
    if raw:
        p = raw_leaves(sc) if p is None else p
        out = GSRawPoseFunction.apply(*[p[k] for k in RAW], us, R, t, cam, opts)
    else:
        p = leaves(sc) if p is None else p
        out = GSPoseFunction.apply(*[p[k] for k in NAMES], us, R, t, cam, opts)
    Wi, Wd, Wa = wts
    loss = (out[0] * dev(Wi)).sum()
    if mode == "extras":
        loss = loss + (out[2][0] * dev(Wd)).sum() + (out[3][0] * dev(Wa)).sum()
    loss.backward()
    p["us"] = us
    return host(R.grad), host(t.grad), p, out


@functools.lru_cache(maxsize=None)
def reference(key, mode):
    """float64 per-Gaussian pose terms [N,12] of scene ``key`` under ``mode`` -- computed once, shared, never changed"""
    sc = scene_of(key)
    Wi, Wd, Wa = weights(sc, 7)
    ex = mode == "extras"
    o = aa_ref.aa_oracle(sc, sc.cam, BG if ex else None, Wi, Wd if ex else None, Wa if ex else None,
                         antialiased=mode == "aa")
    terms = pose_vjp(sc.pws, o["cov3ds"], sc.shs, sc.cam.Rcw, sc.cam.tcw, sc.cam, O.POLICY_G, o["us"], o["dcov2d"],
                     o["dcolour"], o["dz"] if ex else None, depths=o["depths"])
    terms.setflags(write=False)
    return terms


def scene_of(key):
    if key in SCENES:
        return SCENES[key]()
    kind, n, sh = key
    assert kind == "small"
    return posed(S.small_scene(n, 48, 32, sh, seed=31))


def check_vs_reference(key, mode, raw=False, label=""):
    sc = scene_of(key)
    gR, gt, _, _ = run(sc, "plain" if mode == "raw" else mode, True, weights(sc, 7), raw=raw)
    gap = assert_pose_close(gR, gt, reference(key, "plain" if mode == "raw" else mode), 1e-4, (key, mode, raw, label))
    print("pose-only vs float64 reference %s %s raw=%s %s: max gap %.3g of sum |terms|" % (key, mode, raw, label, gap))


# ------------------------------------------------------------------------------------- 1. against the float64 reference
@pytest.mark.parametrize("name", list(SCENES))
@pytest.mark.parametrize("mode", ["plain", "extras", "raw", "aa"])
def test_pose_only_vs_reference(gsc, name, mode):
    check_vs_reference(name, mode, raw=mode == "raw")


# ------------------------------------------------------------------------------------- 2. against the full pose node
@pytest.mark.parametrize("mode", ["plain", "extras", "aa"])
def test_pose_only_equals_the_full_node(gsc, mode):
    """single-tile scene (bit-reproducible gradient records): two pose-only calls agree bitwise; pose-only and the full
    node agree to 4e-6 of the term scale, the jitter bound of test_pose_gradient_is_bitwise_reproducible (the two
    instances are free to contract FMAs differently)"""
    sc = single_tile_scene()
    wts = weights(sc, 9)
    a = np.concatenate([x.reshape(-1) for x in run(sc, mode, True, wts)[:2]])
    b = np.concatenate([x.reshape(-1) for x in run(sc, mode, True, wts)[:2]])
    assert np.array_equal(a, b)
    fR, ft, p, _ = run(sc, mode, False, wts)
    full = np.concatenate([fR.reshape(-1), ft])
    gap = (np.abs(a - full) / term_scale(sc, host(p["pws"].grad))).max()
    print("pose-only vs full pose node (%s): max gap %.3g of the term scale" % (mode, gap))
    assert np.abs(full).max() > 0 and gap <= 4e-6


# ------------------------------------------------------------------------------------------ 3. nothing else is written
GUARD = 1024    # floats


def _raw_backward(lib, tensors, high, cam, St, dl, outs, pg, phase):
    """egs_fused_backward as fused.backward calls it; ``outs`` = the seven per-Gaussian outputs in the order of the
    argument list (dpws, dshs, dhigh_shs, dalphas, dscales, drots, dus), tensors or None"""
    from easygaussiansplatting_amd._host import _pol, _ptr, _stream
    pws, shs, alphas, scales, rots = tensors
    n, K = pws.shape[0], shs.shape[1] + (high.shape[1] if high is not None else 0)
    ws_bytes = lib.egs_fused_backward_ws_bytes(n)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    gpack, St.gpack = St.gpack, None
    o = [None if t is None else C.c_void_p(t.data_ptr()) for t in outs]
    rc = lib.egs_fused_backward(
        n, K, St.gsid.shape[0], St.width, St.height, _ptr(pws), _ptr(rots), _ptr(scales), _ptr(shs), _ptr(high),
        _ptr(alphas), _ptr(cam.Rcw), _ptr(cam.tcw), _ptr(cam.twc), float(cam.fx), float(cam.fy), float(cam.cx),
        float(cam.cy), C.byref(_pol()), None, None, None, None, _ptr(St.rec), _ptr(St.depths), _ptr(St.contrib),
        _ptr(St.final_tau), _ptr(St.ranges), _ptr(St.gsid), _ptr(dl), _ptr(ws), ws_bytes, o[0], o[1], o[2], o[3], o[4],
        o[5], o[6], _ptr(St.order), _ptr(gpack), _ptr(St.dcw), phase | St.flags, 0, n, _ptr(St.seg),
        St.seg.numel() if St.seg is not None else 0, _stream(), None, C.byref(pg))
    torch.cuda.synchronize()
    return rc


def _abi_inputs(sc, raw):
    """-> (the five tensors of the argument list, high_shs or None) in the activated or the raw layout"""
    if raw:
        a = sc.alphas.astype(np.float64)
        return [dev(sc.pws), dev(sc.shs[:, :3]), dev(np.log(a / (1 - a))), dev(np.log(sc.scales.astype(np.float64))),
                dev(sc.rots)], dev(sc.shs[:, 3:])
    return [dev(sc.pws), dev(sc.shs), dev(sc.alphas), dev(sc.scales), dev(sc.rots)], None


def _pose_out(lib, n):
    from easygaussiansplatting_amd import _lib
    dR = torch.full((3, 3), float("nan"), device="cuda")
    dt = torch.full((3,), float("nan"), device="cuda")
    nbytes = lib.egs_pose_ws_bytes(n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    return dR, dt, ws, _lib.EgsPoseGrad(dR.data_ptr(), dt.data_ptr(), ws.data_ptr(), nbytes)


@pytest.mark.parametrize("jw", [True, False])
@pytest.mark.parametrize("raw", [False, True])
def test_nothing_but_the_pose_gradient_is_written(gsc, monkeypatch, raw, jw):
    """raw C ABI: the per-Gaussian outputs once as NaN-filled buffers between guard bands, once as NULL.  Every buffer
    still holds its fill, the guards are intact, and the two pose gradients are bitwise equal (single-tile scene).
    Raw layout (EGS_FUSED_RAW): all seven outputs, widths 3, 3, K-3, 1, 3, 4, 2.  Activated layout: six -- the layout
    demands dloss_dhigh_shs == NULL.  With the forward's dcolor_dpws (jw) and without it."""
    from easygaussiansplatting_amd import _lib, fused
    from easygaussiansplatting_amd.function import Camera, _PoseCamera
    monkeypatch.setattr(fused, "SAVE_DCOLOR", jw)
    lib = _lib.load()
    sc = posed(single_tile_scene(), w=(0.0, 0.0, 0.0), t=(0.0, 0.0, 5.0))
    base = Camera.from_scene(sc.cam)
    cam = _PoseCamera(base, base.Rcw, base.tcw)
    tensors, high = _abi_inputs(sc, raw)
    n, K = sc.n, sc.shs.shape[1]
    widths = (3, 3, K - 3, 1, 3, 4, 2) if raw else (3, K, 0, 1, 3, 4, 2)     # (width 0: the pointer stays NULL)
    dl = dev(weights(sc, 4)[0])
    got = []
    for null in (False, True):
        _, _, St = fused.forward(*tensors, cam, high_shs=high, need_grad=True)
        assert bool(St.flags & fused.RAW) == raw and (St.dcw is not None) == jw
        keep = fused.KEEP_FORWARD_ORDER if St.order_by_work else 0
        bufs = []
        for w in widths:
            b = torch.full((2 * GUARD + n * w,), float("nan"), device="cuda")
            b[:GUARD] = 12345.0
            b[GUARD + n * w:] = 12345.0
            bufs.append(b)
        outs = [None if (null or w == 0) else b[GUARD:] for b, w in zip(bufs, widths)]
        dR, dt, _ws, pg = _pose_out(lib, n)
        assert _raw_backward(lib, tensors, high, cam, St, dl, outs, pg, fused.POSE_ONLY | keep) == 0
        for b, w in zip(bufs, widths):
            assert bool(torch.isnan(b[GUARD:GUARD + n * w]).all()), w
            assert bool((b[:GUARD] == 12345.0).all()) and bool((b[GUARD + n * w:] == 12345.0).all()), w
        got.append(np.concatenate([host(dR).reshape(-1), host(dt)]))
    assert np.isfinite(got[0]).all() and np.abs(got[0]).max() > 0
    assert np.array_equal(got[0], got[1])


def test_near_culled_gaussians_with_records_contribute_nothing(gsc):
    """the kernel's own near-cull branch: the whole scene behind the camera, but gradient records filled by hand with
    non-zero values (the draw pass lists nothing and leaves them alone) -- the pose gradient is still exactly zero"""
    from easygaussiansplatting_amd import _lib, fused
    from easygaussiansplatting_amd.function import Camera, _PoseCamera
    lib = _lib.load()
    sc = posed(S.small_scene(300, 48, 32, 12, seed=31), t=(0.05, -0.08, -5.0))
    base = Camera.from_scene(sc.cam)
    cam = _PoseCamera(base, base.Rcw, base.tcw)
    tensors, _ = _abi_inputs(sc, False)
    _, mask, St = fused.forward(*tensors, cam, need_grad=True)
    assert not bool(mask.any())
    St.gpack.copy_(dev(S.normal(3, 9, (sc.n, 12))))
    dR, dt, _ws, pg = _pose_out(lib, sc.n)
    assert _raw_backward(lib, tensors, None, cam, St, dev(weights(sc, 4)[0]), [None] * 7, pg, fused.POSE_ONLY) == 0
    assert not host(dR).any() and not host(dt).any()


# ------------------------------------------------------------------------- 4. shapes where the reduction can go wrong
@pytest.mark.parametrize("n", [1, 63, 255, 256, 257, 3001])
def test_partial_waves_and_workgroups(gsc, n):
    """partial last wave, partial last workgroup, more than one partial row: each n against the float64 reference
    (rule 1: 1e-4 of sum |terms|; a component no Gaussian contributes to must be exactly zero)"""
    check_vs_reference(("small", n, 12), "plain", label="n=%d" % n)


def test_every_gaussian_near_culled_gives_exact_zeros(gsc):
    sc = posed(S.small_scene(300, 48, 32, 12, seed=31), t=(0.05, -0.08, -5.0))     # the whole scene behind the camera
    gR, gt, _, out = run(sc, "plain", True, weights(sc, 7))
    assert not bool(out[1].any())
    assert not gR.any() and not gt.any()


# --------------------------------------------------------------------------------------------------- 5. both SH paths
@pytest.mark.parametrize("raw", [False, True])
@pytest.mark.parametrize("sh_dim,jw", [(48, True), (3, False), (12, False), (27, False), (48, False)])
def test_sh_paths(gsc, monkeypatch, raw, sh_dim, jw):
    """with the forward's dcolor_dpws (JW) and without it, where the kernel stages the SH rows itself: KH = 0, 9, 24,
    45 (no high rows, the odd span staging, the even row staging, odd again), raw and activated"""
    from easygaussiansplatting_amd import fused
    monkeypatch.setattr(fused, "SAVE_DCOLOR", jw)
    check_vs_reference(("small", 160, sh_dim), "raw" if raw else "plain", raw=raw, label="jw=%s" % jw)


# ----------------------------------------------------------------------------------------------------- 6. segment path
def test_segment_path_gives_the_same_pose_only_gradient(gsc):
    """as test_segment_path_gives_the_same_pose_gradient, pose-only: unsplit against split lists, 1e-3 of the term scale
    (the scale from the full node's dL/dpw on the unsplit path).  Scene: ``skewed_scene`` at 60 k Gaussians, 320 x 240,
    SH 12, segments of 64 entries (egs_seg_config(64, 64)) -- the 1.5 M / 1080p original takes far longer than a few
    seconds and splits no differently"""
    from easygaussiansplatting_amd import _lib, fused
    lib = _lib.load()
    sc = S.skewed_scene(60_000, 320, 240, 12, reset_alpha=True)
    wts = (weights(sc, 8)[0], None, None)
    before = (C.c_int * 2)()
    _lib.check(lib.egs_seg_config(0, 0, before))
    prev = fused.SEGMENTS
    got, seg_used = {}, {}
    try:
        _lib.check(lib.egs_seg_config(64, 64, None))
        fused.SEGMENTS = "0"
        _, _, p, _ = run(sc, "plain", False, wts)
        scale = term_scale(sc, host(p["pws"].grad))
        for seg in ("0", "1"):
            fused.SEGMENTS = seg
            gR, gt, _, out = run(sc, "plain", True, wts)
            seg_used[seg] = out[0].grad_fn.state.seg is not None
            got[seg] = np.concatenate([gR.reshape(-1), gt])
    finally:
        fused.SEGMENTS = prev
        _lib.check(lib.egs_seg_config(before[0], before[1], None))
    assert seg_used == {"0": False, "1": True}
    gap = np.abs(got["1"] - got["0"]) / scale
    print("segment vs unsplit pose-only gradient: max gap %.3g of the term scale" % gap.max())
    assert np.abs(got["0"]).max() > 0 and (gap <= 1e-3).all(), (gap, got)


# -------------------------------------------------------------------------------------------------------------- 7. host
def test_fused_backward_returns_the_pose_pair(gsc):
    from easygaussiansplatting_amd import fused
    from easygaussiansplatting_amd.function import Camera, _PoseCamera
    sc = SCENES["g5"]()
    base = Camera.from_scene(sc.cam)
    cam = _PoseCamera(base, base.Rcw, base.tcw)
    tensors = [dev(sc.pws), dev(sc.shs), dev(sc.alphas), dev(sc.scales), dev(sc.rots)]
    dl = dev(weights(sc, 7)[0])
    _, _, St = fused.forward(*tensors, cam, need_grad=True)
    res = fused.backward(*tensors, cam, St, dl, pose=(cam.Rcw, cam.tcw), pose_only=True)
    assert isinstance(res, tuple) and len(res) == 2 and res[0].shape == (3, 3) and res[1].shape == (3,)
    assert_pose_close(host(res[0]), host(res[1]), reference("g5", "plain"), 1e-4, "fused.backward")
    _, _, St = fused.forward(*tensors, cam, need_grad=True)
    with pytest.raises(ValueError, match="pose_only needs pose"):
        fused.backward(*tensors, cam, St, dl, pose_only=True)
    with pytest.raises(ValueError, match="absgrad"):
        fused.backward(*tensors, cam, St, dl, pose=(cam.Rcw, cam.tcw), pose_only=True, absgrad=True)


@pytest.mark.parametrize("raw", [False, True])
def test_autograd_leaves_the_gaussians_alone(gsc, raw):
    """Gaussian leaves that require grad get no ``.grad`` (the node returns None for them and for ``us``)"""
    sc = SCENES["g5"]()
    gR, gt, p, _ = run(sc, "plain", True, weights(sc, 7), raw=raw)
    assert all(v.requires_grad and v.grad is None for v in p.values()), [k for k, v in p.items() if v.grad is not None]
    assert np.abs(gR).max() > 0 and np.abs(gt).max() > 0


def test_refine_pose_recovers_the_pose(gsc):
    """``pose.refine_pose`` (pose-only by default) on the example's scene and perturbation: the thresholds of
    test_pose_refine_example_recovers_the_pose"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    try:
        import pose_refine
    finally:
        sys.path.pop(0)
    sc = pose_refine.make_scene(20_000, 320, 240, 12, seed=0)
    hist = pose_refine.refine(sc, steps=150, deg=2.0, shift=0.05, seed=0, pose_only=True)
    (_, r0, t0), (_, r1, t1) = hist[0], hist[-1]
    print("pose-only refine: rotation %.4f -> %.4f deg, translation %.5f -> %.5f" % (r0, r1, t0, t1))
    assert r0 > 1.9 and t0 > 0.04
    assert r1 * 5 <= r0 and t1 * 5 <= t0, (r0, r1, t0, t1)
