"""Anti-aliased rendering without a GPU: the float64 reference of the opacity compensation (tests/aa_ref.py) against
central differences and against the mass identity it exists for, the RenderOptions rule, and the C-ABI additions."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from easygaussiansplatting_amd import scene as S
from oracle import gs_oracle as O
from tests import aa_ref
from tests.test_cabi_and_host import REMOVED_IN_ABI_12, egs_names

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# ABI 11 folded the anti-aliased entry points into egs_fused_forward / egs_viewer_prep (flag EGS_FUSED_ANTIALIASED)
REMOVED_SYMBOLS = ("egs_fused_forward_aa", "egs_fused_forward_raw_aa", "egs_viewer_prep_aa")


def _spd(rng, n, lo, hi):
    """n dilated cov2d rows (a, b, c): Sigma with eigenvalues in [lo, hi] px^2 and a random orientation, plus 0.3 I"""
    th = rng.uniform(0, np.pi, n)
    l1, l2 = rng.uniform(lo, hi, n), rng.uniform(lo, hi, n)
    c, s = np.cos(th), np.sin(th)
    a = l1 * c * c + l2 * s * s
    b = (l1 - l2) * c * s
    d = l1 * s * s + l2 * c * c
    return np.stack([a + 0.3, b, d + 0.3], 1)


def _central(cov, g, eps):
    out = np.zeros_like(cov)
    for k in range(3):
        e = np.zeros(3)
        e[k] = eps
        out[:, k] = g * (aa_ref.comp(cov + e) - aa_ref.comp(cov - e)) / (2 * eps)
    return out


# ------------------------------------------------------------------------------------------- 1. comp VJP vs differences
@pytest.mark.parametrize("kind", ["general", "tiny", "det_to_zero", "large"])
def test_comp_vjp_matches_central_differences(kind):
    rng = np.random.default_rng(11)
    if kind == "general":
        cov = _spd(rng, 400, 0.01, 20.0)
    elif kind == "tiny":           # much smaller than a pixel
        cov = _spd(rng, 400, 1e-4, 1e-2)
    elif kind == "large":          # comp -> 1
        cov = _spd(rng, 400, 50.0, 5e3)
    else:                          # det(Sigma) -> 0+: one eigenvalue near zero
        th = rng.uniform(0, np.pi, 400)
        l1, l2 = rng.uniform(1e-6, 1e-4, 400), rng.uniform(0.5, 5.0, 400)
        c, s = np.cos(th), np.sin(th)
        cov = np.stack([l1 * c * c + l2 * s * s + 0.3, (l1 - l2) * c * s, l1 * s * s + l2 * c * c + 0.3], 1)
    g = rng.normal(size=cov.shape[0])
    cm = aa_ref.comp(cov)
    assert (cm > 0).all() and (cm <= 1).all()
    if kind == "large":
        assert cm.min() > 0.98
    if kind == "tiny":
        assert cm.max() < 0.05
    # step well inside the distance to det(Sigma) = 0 (the smallest eigenvalue of Sigma)
    lam = np.linalg.eigvalsh(np.stack([np.stack([cov[:, 0] - 0.3, cov[:, 1]], 1),
                                       np.stack([cov[:, 1], cov[:, 2] - 0.3], 1)], 1))[:, 0]
    got = aa_ref.comp_vjp(cov, g)
    for i in range(cov.shape[0]):
        eps = min(1e-5, 1e-3 * lam[i])
        ref = _central(cov[i:i + 1], g[i:i + 1], eps)[0]
        scale = np.abs(ref).max() + 1e-12
        assert np.abs(got[i] - ref).max() <= 1e-5 * scale + 1e-9, (kind, i, got[i], ref)


def test_comp_degenerate_rule():
    cov = np.array([[0.3, 0.0, 0.5],            # det(Sigma) = 0
                    [0.2, 0.0, 0.8],            # det(Sigma) < 0
                    [np.nan, 0.1, 0.5],         # a NaN conic (no nan_cull)
                    [0.0, 0.0, 0.0],            # a near-culled row of the oracle (zeros)
                    [1.3, 0.0, 1.3]])           # Sigma = I: comp = 1 / 1.3
    cm = aa_ref.comp(cov)
    assert cm[:4].tolist() == [0.0, 0.0, 0.0, 0.0]
    assert abs(cm[4] - 1 / 1.3) < 1e-15
    g = aa_ref.comp_vjp(cov, np.ones(5))
    assert (g[:4] == 0).all() and np.isfinite(g).all()


# ---------------------------------------------------------------------------------------------- 2. the mass identity
@pytest.mark.parametrize("s3", [0.002, 0.004, 0.008])
def test_mass_identity_of_one_isolated_tiny_gaussian(s3):
    """sum over pixels of alpha' = alpha comp G equals alpha 2 pi sqrt(det Sigma): the mass of the UNdilated Gaussian;
    without compensation it is the dilated one's, alpha 2 pi sqrt(det(Sigma + 0.3 I))"""
    cam = S.Camera(64, 64, 256.0, 256.0, 32.0, 32.0, np.eye(3), np.array([0.0, 0.0, 5.0]))
    pws = np.array([[0.0013, -0.0021, 0.0]])
    rots = np.array([[0.9, 0.1, 0.3, 0.2]]) / np.linalg.norm([0.9, 0.1, 0.3, 0.2])
    scales = np.array([[s3, 1.6 * s3, s3]])
    al = 0.8
    P = O.POLICY_G
    us, pcs, depths = O.project(pws, cam.Rcw, cam.tcw, cam.fx, cam.fy, cam.cx, cam.cy, P)
    c3 = O.compute_cov3d(rots, scales, depths, P)
    c2 = O.compute_cov2d(c3, pcs, cam.Rcw, depths, cam.fx, cam.fy, cam.width, cam.height, P)
    ci, _ = O.inverse_cov2d(c2, depths, P)
    cm = aa_ref.comp(c2)[0]
    a, b, c = c2[0]
    det_sigma = (a - 0.3) * (c - 0.3) - b * b
    assert 0 < det_sigma and a - 0.3 < 1.0 and c - 0.3 < 1.0       # smaller than a pixel
    py, px = np.mgrid[0:64, 0:64].astype(np.float64)
    dx, dy = px - us[0, 0], py - us[0, 1]
    G = np.exp(-0.5 * (ci[0, 0] * dx * dx + 2 * ci[0, 1] * dx * dy + ci[0, 2] * dy * dy))
    mass_aa = (al * cm * G).sum()
    mass_plain = (al * G).sum()
    want = al * 2 * np.pi * np.sqrt(det_sigma)
    assert abs(mass_aa / want - 1) < 0.01, (mass_aa, want)
    assert abs(mass_plain / (al * 2 * np.pi * np.sqrt(a * c - b * b)) - 1) < 0.01
    assert mass_plain > 1.5 * want


# ------------------------------------------------------------------------------------------------ 3. RenderOptions
def test_render_options_antialiased():
    from easygaussiansplatting_amd.function import RenderOptions
    assert RenderOptions().antialiased is False
    assert RenderOptions(antialiased=True).antialiased is True
    o = RenderOptions(antialiased=True, depth=True, alpha=True, background=(1, 1, 1), accumulate=True)
    assert o.antialiased and o.has_extras()
    with pytest.raises(ValueError, match="antialiased"):
        RenderOptions(mode="ops", antialiased=True)
    with pytest.raises(ValueError, match="antialiased"):
        RenderOptions(antialiased="yes")
    RenderOptions(mode="ops", antialiased=False)        # the default stays legal everywhere


def test_trainer_refuses_antialiased_ops_mode():
    from easygaussiansplatting_amd.trainer import Trainer
    sc = S.small_scene(10, 16, 16, 3, seed=1)
    with pytest.raises(ValueError, match="antialiased"):
        Trainer(sc, [sc.cam], [None], max_steps=1, device="cpu", fused_activations=False, mode="ops",
                antialiased=True)


# ------------------------------------------------------------------------------------------------------ 4. C ABI
def test_antialiased_flag_abi():
    from easygaussiansplatting_amd import _lib, fused
    hdr = open(os.path.join(REPO, "include", "egs_hip.h")).read()
    assert int(re.search(r"#define EGS_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION == 12
    for name in REMOVED_SYMBOLS:
        assert name not in hdr and name not in _lib.SIGNATURES, name
    for name in REMOVED_IN_ABI_12:      # (whole identifiers: egs_splat_draw_rec is a prefix of the call that stays)
        assert name not in egs_names(hdr) and name not in _lib.SIGNATURES, name
    # the flag rides on the one forward entry point (`flags`) and the viewer's (`flags`, in front of the stream)
    assert "int egs_fused_forward(" in hdr and "int egs_viewer_prep(" in hdr
    assert _lib.SIGNATURES["egs_viewer_prep"][1][-2:] == [C.c_int, C.c_void_p]
    # the render flags share `phase` with the per-call backward bits: one bit each, none overlapping
    bits = {k: int(v) for k, v in re.findall(r"#define (EGS_(?:BWD|FUSED)_\w+) (\d+)", hdr)}
    assert "EGS_BWD_ANTIALIASED" not in bits and "EGS_BWD_CULLED_LISTS" not in bits
    aa = bits.pop("EGS_FUSED_ANTIALIASED")
    assert aa == 256 == fused.ANTIALIASED and aa & (aa - 1) == 0
    assert aa & 3 == 0                                  # the base phase 0 / 1 / 2
    for k, v in bits.items():
        assert aa & v == 0, k
    assert C.sizeof(_lib.EgsPolicy) == 52 and C.sizeof(_lib.EgsExtras) == 56 and C.sizeof(_lib.EgsPoseGrad) == 32


@pytest.fixture(scope="module")
def lib():
    from easygaussiansplatting_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_antialiased_variants_folded_in_exports(lib):
    from easygaussiansplatting_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in REMOVED_SYMBOLS + REMOVED_IN_ABI_12:
        assert name not in exported, name
    assert "egs_fused_forward" in exported and "egs_viewer_prep" in exported
    assert lib.egs_abi_version() == 12


def _forward(lib, n, flags, high, rec):
    """egs_fused_forward on fake pointers (every call here is refused before one is dereferenced)"""
    from easygaussiansplatting_amd import _lib
    pol = _lib.EgsPolicy()
    lib.egs_policy_gsplatcu(C.byref(pol))
    dummy = C.c_void_p(16)
    # pws, rots, scales, shs | low_shs, high_shs, alphas, Rcw, tcw, twc
    args = [n, 3 if high is None else 12] + [dummy] * 4 + [high] + [dummy] * 4
    args += [256.0, 256.0, 128.0, 128.0, 256, 256, C.byref(pol)]
    # us, depths, cinv2ds, colors, areas, rec, visible, dcolor_dpws
    args += [dummy, dummy, dummy, dummy, dummy, rec, dummy, None]
    args += [flags, 32, dummy, 1 << 20, dummy, None, None]
    return lib.egs_fused_forward(*args)


def test_antialiased_flag_requires_records(lib):
    """rec == NULL is refused by the C ABI before anything reaches the device, for activated and raw inputs, n == 0
    included"""
    from easygaussiansplatting_amd import fused
    for n in (1000, 0):
        for flags, high in ((fused.ANTIALIASED, None), (fused.ANTIALIASED | fused.RAW, C.c_void_p(16))):
            assert _forward(lib, n, flags, high, None) == 10001
            assert "rec" in lib.egs_last_error_string().decode()


def test_forward_flags_are_checked(lib):
    """high_shs belongs to raw inputs; bits outside the EGS_FUSED_* set are refused; so is a raw render without rec"""
    from easygaussiansplatting_amd import fused
    dummy = C.c_void_p(16)
    assert _forward(lib, 1000, 0, dummy, dummy) == 10001
    assert "shs_high" in lib.egs_last_error_string().decode()
    assert _forward(lib, 1000, fused.ANTIALIASED, dummy, dummy) == 10001
    assert _forward(lib, 1000, fused.RAW, dummy, None) == 10001
    assert "rec" in lib.egs_last_error_string().decode()
    assert _forward(lib, 1000, 1, None, dummy) == 10001
    assert _forward(lib, 1000, 1024, None, dummy) == 10001


def test_viewer_prep_flags_are_checked(lib):
    """egs_viewer_prep takes EGS_FUSED_ANTIALIASED and nothing else"""
    from easygaussiansplatting_amd import fused
    m = (C.c_float * 16)(*np.eye(4, dtype=np.float32).ravel())
    dummy = C.c_void_p(16)
    for flags in (fused.CULLED_LISTS, fused.RAW, fused.ANTIALIASED | 1):
        assert lib.egs_viewer_prep(10, 3, dummy, m, m, 100.0, 100.0, dummy, dummy, flags, None) == 10001
    # n == 0: nothing to launch, and the flag is accepted
    assert lib.egs_viewer_prep(0, 3, None, m, m, 100.0, 100.0, None, None, fused.ANTIALIASED, None) == 0
