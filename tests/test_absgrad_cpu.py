"""Absolute screen-space gradients (``RenderOptions.absgrad``, ``EGS_BWD_ABSGRAD``) without a GPU: the
float64 restatement ``tests/absgrad_ref.py`` against the oracle's walk, the properties of the statistic it defines, the
C ABI and the validation of the Python surface."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from easygaussiansplatting_amd import scene as S
from oracle import gs_oracle as O
from tests.absgrad_ref import draw_backward_abs
from tests.conftest import load_golden

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------------------- 1. the restatement
@pytest.fixture(scope="module")
def small():
    """scene.small_scene through the oracle's stages and forward blend: everything draw_backward takes"""
    sc = S.small_scene(400, 64, 48, 3, seed=5)
    cam, P = sc.cam, O.POLICY_G
    us, pcs, depths = O.project(sc.pws, cam.Rcw, cam.tcw, cam.fx, cam.fy, cam.cx, cam.cy, P, False)[:3]
    c3 = O.compute_cov3d(sc.rots, sc.scales, depths, P, False)
    c2 = O.compute_cov2d(c3, pcs, cam.Rcw, depths, cam.fx, cam.fy, cam.width, cam.height, P, False)
    col = O.sh2color(sc.shs, sc.pws, cam.twc, False)
    ci, areas = O.inverse_cov2d(c2, depths, P, False)[:2]
    img, cont, tau, ranges, gsid = O.splat(cam.height, cam.width, us, ci, sc.alphas, depths, col, areas, P)
    dl = S.normal(3, 2, (3, cam.height, cam.width)) / (3 * cam.height * cam.width)
    return dict(W=cam.width, H=cam.height, ranges=ranges, gsid=gsid, us=us, ci=ci, alphas=sc.alphas, col=col,
                cont=cont, tau=tau, dl=dl)


@pytest.fixture(scope="module")
def g5():
    """the multi-tile raster fixture G5 (48 x 32: 3 x 2 tiles): the inputs of the reference's backward walk"""
    g = load_golden("g5_raster_b_multitile.npz")
    return dict(W=48, H=32, ranges=g["ranges"], gsid=g["gsid"], us=g["us"], ci=g["cinv2ds"], alphas=g["alphas"],
                col=g["colors"], cont=g["contrib"], tau=g["final_tau"] if "final_tau" in g else None,
                dl=g["dloss_dgammas"], depths=g["depths"], areas=g["areas"])


def _walk(d, tiles=None):
    return draw_backward_abs(d["W"], d["H"], d["ranges"], d["gsid"], d["us"], d["ci"], d["alphas"], d["col"],
                             d["cont"], d["tau"], d["dl"], None, O.POLICY_G, tiles=tiles)


def _g5_complete(g5):
    if g5["tau"] is None:      # the fixture keeps the image, not the transmittance: the oracle's own forward blend
        _, cont, tau = O.draw(g5["W"], g5["H"], g5["ranges"], g5["gsid"], g5["us"], g5["ci"], g5["alphas"], g5["col"],
                              None, O.POLICY_G)
        g5["cont"], g5["tau"] = cont, tau
    return g5


@pytest.mark.parametrize("which", ["small", "g5"])
def test_restatement_is_the_oracles_walk(which, small, g5):
    d = small if which == "small" else _g5_complete(g5)
    want = O.draw_backward(d["W"], d["H"], d["ranges"], d["gsid"], d["us"], d["ci"], d["alphas"], d["col"], d["cont"],
                           d["tau"], d["dl"], None, O.POLICY_G)[0]
    dus, dus_abs = _walk(d)
    assert np.abs(want).max() > 0
    assert np.abs(dus - want).max() <= 1e-12 * np.abs(want).max()
    # the absolute sum bounds the signed one, row by row and component by component
    assert (dus_abs >= np.abs(dus) - 1e-12 * dus_abs.max()).all()
    assert (dus_abs > np.abs(dus) * (1 + 1e-6)).any()          # ... and is not the same thing
    assert dus_abs.min() >= 0


@pytest.mark.parametrize("which", ["small", "g5"])
def test_sum_over_disjoint_tile_subsets_is_the_whole(which, small, g5):
    d = small if which == "small" else _g5_complete(g5)
    T = d["ranges"].shape[0]
    whole = _walk(d)
    a = _walk(d, tiles=list(range(0, T, 2)))
    b = _walk(d, tiles=list(range(1, T, 2)))
    for w, x, y in zip(whole, a, b):
        assert np.abs(w - (x + y)).max() <= 1e-12 * np.abs(w).max()


def test_symmetric_footprint_cancels_in_the_signed_sum_only():
    """The case the feature exists for: one isolated, symmetric Gaussian centred on a pixel under a uniform dL/dimage
    is pulled equally in every direction -- the signed gradient vanishes, the absolute one does not."""
    W = H = 48
    us = np.array([[24.0, 24.0]]); ci = np.array([[0.08, 0.0, 0.08]])
    alphas = np.array([0.6]); col = np.array([[0.5, 0.4, 0.3]])
    depths = np.array([2.0]); areas = np.array([[20, 20]], np.int32)
    img, cont, tau, ranges, gsid = O.splat(H, W, us, ci, alphas, depths.copy(), col, areas.copy(), O.POLICY_G)
    assert cont.max() == 1 and (ranges[:, 1] - ranges[:, 0]).sum() >= 4       # the footprint spans several tiles
    dl = np.full((3, H, W), 1.0 / (3 * H * W))
    dus, dus_abs = draw_backward_abs(W, H, ranges, gsid, us, ci, alphas, col, cont, tau, dl, None, O.POLICY_G)
    assert (dus_abs > 0).all()
    assert np.abs(dus).max() < 1e-9 * dus_abs.max()


# ------------------------------------------------------------------------------------------------ 2. C ABI
@pytest.fixture(scope="module")
def lib():
    from easygaussiansplatting_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_absgrad_abi_is_additive(lib):
    from easygaussiansplatting_amd import _lib, fused
    hdr = open(os.path.join(REPO, "include", "egs_hip.h")).read()
    assert int(re.search(r"#define EGS_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION == 12
    assert lib.egs_abi_version() == 12
    bits = {k: int(v) for k, v in re.findall(r"#define (EGS_(?:BWD|FUSED)_\w+) (\d+)", hdr)}
    ab = bits.pop("EGS_BWD_ABSGRAD")
    assert ab == fused.ABSGRAD and ab & (ab - 1) == 0 and ab & 3 == 0          # one bit, clear of the base phase
    for k, v in bits.items():
        assert ab & v == 0, k
    assert "int egs_grad_records_absgrad(int n, const float* grad_records, float* dloss_dus_abs" in hdr
    assert _lib.SIGNATURES["egs_grad_records_absgrad"] == (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p])
    # nothing that existed moved: the argument list of the backward entry point and the structs it takes
    P, i, f = C.c_void_p, C.c_int, C.c_float
    assert _lib.SIGNATURES["egs_fused_backward"] == (
        i, [i, i, C.c_int64, i, i] + [P] * 9 + [f] * 4 + [C.POINTER(_lib.EgsPolicy)] + [P] * 11 + [P, C.c_size_t]
        + [P] * 7 + [P, P, P, i, i, i, P, C.c_size_t, P, C.POINTER(_lib.EgsExtras), C.POINTER(_lib.EgsPoseGrad)])
    assert C.sizeof(_lib.EgsPolicy) == 52 and C.sizeof(_lib.EgsExtras) == 56 and C.sizeof(_lib.EgsPoseGrad) == 32
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert "egs_grad_records_absgrad" in exported and "egs_fused_backward" in exported
    from tests.test_cabi_and_host import REMOVED_IN_ABI_12, egs_names
    for name in REMOVED_IN_ABI_12:      # ABI 12 only removed: the splat-stage variants nothing called
        assert name not in exported and name not in _lib.SIGNATURES and name not in egs_names(hdr), name


def test_absgrad_refusals_before_the_device(lib):
    """the flag without the caller's records, or with render extras: refused before anything is read"""
    from easygaussiansplatting_amd import _lib, fused
    n = 1000
    pol = _lib.EgsPolicy()
    lib.egs_policy_gsplatcu(C.byref(pol))
    fake = C.c_void_p(256)      # never dereferenced: every check below fails first

    def call(phase, records, extras):
        args = [n, 12, 0, 64, 64] + [fake] * 4 + [None] + [fake] * 4 + [256.0, 256.0, 32.0, 32.0] + \
            [C.byref(pol)] + [fake] * 11 + [fake, 1 << 30] + [fake, fake, None] + [fake] * 4 + \
            [None, records, None, phase, 0, n, None, 0, None, extras, None]
        return lib.egs_fused_backward(*args)
    ex = _lib.EgsExtras()
    for phase in (0, 1):
        assert call(phase | fused.ABSGRAD, None, None) == 10001                      # EGS_ERR_BAD_ARG
        assert call(phase | fused.ABSGRAD, fake, C.byref(ex)) == 10001
    assert call(3 | fused.ABSGRAD, fake, None) == 10001                              # (the base phase is still checked)
    assert lib.egs_grad_records_absgrad(-1, fake, fake, None) == 10001
    assert lib.egs_grad_records_absgrad(n, None, fake, None) == 10001
    assert lib.egs_grad_records_absgrad(n, fake, None, None) == 10001
    assert lib.egs_grad_records_absgrad(0, None, None, None) == 0


# ---------------------------------------------------------------------------------------- 3. Python surface
def test_render_options_absgrad_validation():
    from easygaussiansplatting_amd.function import RenderOptions
    assert RenderOptions().absgrad is False
    assert RenderOptions(absgrad=True).absgrad is True and RenderOptions(absgrad=1).absgrad is True
    assert RenderOptions(absgrad=True, antialiased=True, accumulate=True).absgrad
    for bad in ("yes", 2, None, 0.5):
        with pytest.raises(ValueError, match="absgrad"):
            RenderOptions(absgrad=bad)
    with pytest.raises(ValueError, match="absgrad"):
        RenderOptions(mode="ops", absgrad=True)
    for extra in (dict(depth=True), dict(alpha=True), dict(background=(0, 0, 0))):
        with pytest.raises(ValueError, match="absgrad"):
            RenderOptions(absgrad=True, **extra)
    RenderOptions(mode="ops", absgrad=False)            # the default stays legal everywhere


def test_absgrad_needs_a_tensor_for_us():
    torch = pytest.importorskip("torch")
    from easygaussiansplatting_amd.function import Camera, GSFunction, GSRawFunction, RenderOptions
    cam = Camera(64, 48, 256.0, 256.0, 32.0, 24.0, np.eye(3), np.zeros(3), device="cpu")
    z = lambda *s: torch.zeros(*s, dtype=torch.float32)
    o = RenderOptions(absgrad=True)
    with pytest.raises(ValueError, match="us"):
        GSFunction.apply(z(8, 3), z(8, 3), z(8, 1), z(8, 3), z(8, 4), None, cam, o)
    with pytest.raises(ValueError, match="us"):
        GSRawFunction.apply(z(8, 3), z(8, 3), z(8, 0), z(8, 1), z(8, 3), z(8, 4), None, cam, o)


def test_trainer_absgrad_arguments():
    from easygaussiansplatting_amd.trainer import Trainer
    sc = S.small_scene(10, 16, 16, 3, seed=1)
    with pytest.raises(ValueError, match="absgrad"):
        Trainer(sc, [sc.cam], [None], max_steps=1, device="cpu", fused_activations=False, mode="ops", absgrad=True)
    tr = Trainer(sc, [sc.cam], [None], max_steps=1, device="cpu", absgrad=True, grad_threshold=2e-6)
    assert tr.absgrad is True and tr.density.grad_threshold == 2e-6
    tr = Trainer(sc, [sc.cam], [None], max_steps=1, device="cpu")
    assert tr.absgrad is False and tr.density.grad_threshold == 4e-7          # the reference's, no new default


def test_train_example_has_the_switches():
    """the example's own argument parser: both switches exist, --grad-threshold takes a float"""
    import sys
    r = subprocess.run([sys.executable, os.path.join(REPO, "examples", "train.py"), "--help"], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr
    assert "--absgrad" in r.stdout and "--grad-threshold GRAD_THRESHOLD" in r.stdout
    r = subprocess.run([sys.executable, os.path.join(REPO, "examples", "train.py"), "--path", "x", "--absgrad",
                        "--grad-threshold", "not-a-number"], capture_output=True, text=True)
    assert r.returncode == 2 and "--grad-threshold" in r.stderr
