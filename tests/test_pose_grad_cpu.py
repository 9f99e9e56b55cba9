"""Camera pose gradients, CPU part: the float64 pose VJP of tests/pose_ref.py against central differences of the
oracle's stages, and the host side of the new API (exports, ctypes signatures, workspace size, argument checks)."""
import ctypes as C
import os

import numpy as np
import pytest

from easygaussiansplatting_amd import scene as S
from oracle import gs_oracle as O
from tests.pose_ref import pose_grad, pose_vjp
from tests.test_numeric_diff import central, check


def rodrigues(w):
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / max(th, 1e-300)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def _setup(sh_dim, seed, n=12, w=64, h=48):
    sc = S.small_scene(n, w, h, sh_dim, seed=seed)
    R = rodrigues([0.08, -0.15, 0.05]) @ np.asarray(sc.cam.Rcw, np.float64)
    t = np.array([0.1, -0.2, 5.0])
    f64 = lambda a: np.asarray(a, np.float64)
    pws, shs = f64(sc.pws), f64(sc.shs)
    cov3 = O.compute_cov3d(f64(sc.rots), f64(sc.scales))
    rng = np.random.default_rng(seed)
    up = dict(dus=rng.normal(size=(n, 2)), dcov2ds=rng.normal(size=(n, 3)), dcolors=rng.normal(size=(n, 3)),
              dz=rng.normal(size=n))
    return sc, pws, shs, cov3, R, t, up


def _loss(x, sc, pws, shs, cov3, up, P, parts=("u", "cov", "col", "z"), R_in_J=None):
    """<upstream, stage outputs> at pose x = (Rcw row-major, tcw), twc = -Rcw^T tcw.  ``R_in_J``: hold the rotation
    the projection sees (only the W factor of cov2d moves)"""
    R, t = x[:9].reshape(3, 3), x[9:]
    cam = sc.cam
    Rp = R if R_in_J is None else R_in_J
    us, pcs, depths = O.project(pws, Rp, t, cam.fx, cam.fy, cam.cx, cam.cy, P)
    L = 0.0
    if "u" in parts:
        L += (up["dus"] * us).sum()
    if "cov" in parts:
        c2 = O.compute_cov2d(cov3, pcs, R, depths, cam.fx, cam.fy, cam.width, cam.height, P)
        L += (up["dcov2ds"] * c2).sum()
    if "col" in parts:
        L += (up["dcolors"] * O.sh2color(shs, pws, -R.T @ t)).sum()
    if "z" in parts:
        L += (up["dz"] * pcs[:, 2]).sum()
    return L


@pytest.mark.parametrize("sh_dim", [3, 12, 27, 48])
def test_pose_vjp_matches_central_differences(sh_dim):
    """all 12 components, every stage at once, no clamp (POLICY_B): the VJP is the exact derivative"""
    sc, pws, shs, cov3, R, t, up = _setup(sh_dim, seed=sh_dim)
    P = O.POLICY_B
    x0 = np.concatenate([R.reshape(-1), t])
    num = central(lambda x: _loss(x, sc, pws, shs, cov3, up, P), x0)[0]
    terms = pose_vjp(pws, cov3, shs, R, t, sc.cam, P, up["dus"], up["dcov2ds"], up["dcolors"], up["dz"])
    dR, dt, _ = pose_grad(terms)
    got = np.concatenate([dR.reshape(-1), dt])
    assert check(num, got), (num, got)
    # and every stage alone (the sum could hide two compensating errors)
    for part in ("u", "cov", "col", "z"):
        num = central(lambda x: _loss(x, sc, pws, shs, cov3, up, P, parts=(part,)), x0)[0]
        z = {k: np.zeros_like(v) for k, v in up.items()}
        key = dict(u="dus", cov="dcov2ds", col="dcolors", z="dz")[part]
        z[key] = up[key]
        dR, dt, _ = pose_grad(pose_vjp(pws, cov3, shs, R, t, sc.cam, P, z["dus"], z["dcov2ds"], z["dcolors"],
                                       z["dz"]))
        assert check(num, np.concatenate([dR.reshape(-1), dt])), part
    if sh_dim == 3:     # degree 0: the colour does not see the camera
        assert np.abs(pose_vjp(pws, cov3, shs, R, t, sc.cam, P, 0 * up["dus"], 0 * up["dcov2ds"], up["dcolors"])
                      ).max() == 0


@pytest.mark.parametrize("sh_dim", [3, 48])
def test_pose_vjp_with_the_fov_clamp_binding(sh_dim):
    """POLICY_G (fov clamp, near cull) on a 64 x 48 image at fx = 256: the clamp binds for most Gaussians.
    * the W = Rcw factor of cov2d (J held): the derivative of compute_cov2d in its Rcw argument at fixed p_c, exact
      with the clamp binding;
    * the camera centre term: exact;
    * the whole VJP on the Gaussians the clamp leaves alone: exact."""
    sc, pws, shs, cov3, R, t, up = _setup(sh_dim, seed=40 + sh_dim, n=16)
    P = O.POLICY_G
    cam = sc.cam
    limx, limy = O.fov_limits(cam.fx, cam.fy, cam.width, cam.height, P)
    pc = pws @ R.T + t
    clamped = (np.abs(pc[:, 0] / pc[:, 2]) > limx) | (np.abs(pc[:, 1] / pc[:, 2]) > limy)
    assert 0 < clamped.sum() < len(clamped)
    x0 = np.concatenate([R.reshape(-1), t])
    _, parts = pose_vjp(pws, cov3, shs, R, t, cam, P, up["dus"], up["dcov2ds"], up["dcolors"], up["dz"], parts=True)
    # W factor: move R only where it multiplies Sigma (the projection keeps R0)
    num = central(lambda x: _loss(x, sc, pws, shs, cov3, up, P, parts=("cov",), R_in_J=R), x0)[0]
    assert check(num[:9], parts["W"].sum(0)), (num[:9], parts["W"].sum(0))
    # camera centre: d<gcol, sh2color(pws, twc)>/dtwc
    num = central(lambda c: (up["dcolors"] * O.sh2color(shs, pws, c)).sum(), -R.T @ t)[0]
    assert check(num, parts["twc"].sum(0))
    # everything, on the Gaussians inside the clamp window
    keep = ~clamped
    sub = {k: v[keep] for k, v in up.items()}
    sc2 = sc.subsample(keep)
    num = central(lambda x: _loss(x, sc2, pws[keep], shs[keep], cov3[keep], sub, P), x0)[0]
    dR, dt, _ = pose_grad(pose_vjp(pws[keep], cov3[keep], shs[keep], R, t, cam, P, sub["dus"], sub["dcov2ds"],
                                   sub["dcolors"], sub["dz"]))
    assert check(num, np.concatenate([dR.reshape(-1), dt]))


def test_translation_identity_of_the_reference():
    """Rcw^T dL/dtcw = sum_i dL/dpw_i, exact in math: moving the camera by d is moving every Gaussian by -Rcw^T d"""
    sc, pws, shs, cov3, R, t, up = _setup(27, seed=5, n=20)
    P = O.POLICY_B
    terms = pose_vjp(pws, cov3, shs, R, t, sc.cam, P, up["dus"], up["dcov2ds"], up["dcolors"], up["dz"])
    _, dt, _ = pose_grad(terms)
    # sum_i dL/dpw_i by central differences of a common shift of every Gaussian
    num = central(lambda s: _loss(np.concatenate([R.reshape(-1), t]), sc, pws + s[None, :], shs, cov3, up, P),
                  np.zeros(3))[0]
    assert check(R.T @ dt, num)


# ------------------------------------------------------------------------------------------------- host side, no GPU
@pytest.fixture(scope="module")
def lib():
    from easygaussiansplatting_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_pose_argument_of_fused_backward(lib):
    from easygaussiansplatting_amd import _lib
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in ("egs_pose_ws_bytes", "egs_fused_backward"):
        assert name in exported and name in _lib.SIGNATURES, name
    # ABI 11: the pose is the last, nullable argument of egs_fused_backward, behind the EgsExtras
    from tests.test_cabi_and_host import REMOVED_IN_ABI_12
    for name in ("egs_fused_backward_pose", "egs_fused_backward_raw_pose") + REMOVED_IN_ABI_12:
        assert name not in exported and name not in _lib.SIGNATURES, name
    assert _lib.SIGNATURES["egs_fused_backward"][1][-2:] == [C.POINTER(_lib.EgsExtras), C.POINTER(_lib.EgsPoseGrad)]
    assert _lib.SIGNATURES["egs_fused_backward"][0] is C.c_int
    assert C.sizeof(_lib.EgsPoseGrad) == 32
    assert [f for f, _ in _lib.EgsPoseGrad._fields_] == ["dloss_dRcw", "dloss_dtcw", "ws", "ws_bytes"]
    assert lib.egs_abi_version() == 12 and C.sizeof(_lib.EgsExtras) == 56


def test_pose_ws_bytes_is_monotone(lib):
    sizes = [lib.egs_pose_ws_bytes(n) for n in (0, 1, 255, 256, 257, 10_000, 1_000_000, 4_000_000)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
    assert lib.egs_pose_ws_bytes(1_000_000) >= 16 * 4 * ((1_000_000 + 255) // 256)
    assert lib.egs_pose_ws_bytes(257) >= 2 * 16 * 4


def test_pose_argument_refusals_before_the_device(lib):
    """phase != 0 with a pose, a missing or short pose workspace: refused by the C ABI before anything is read"""
    from easygaussiansplatting_amd import _lib, fused
    n = 1000
    pol = _lib.EgsPolicy()
    lib.egs_policy_gsplatcu(C.byref(pol))
    fake = C.c_void_p(256)      # never dereferenced: every check below fails first

    def call(phase, pg, raw):
        # shs_high / dloss_dhigh_shs: the raw layout only
        high, flags = (fake, fused.RAW) if raw else (None, 0)
        args = [n, 12, 0, 64, 64] + [fake] * 4 + [high] + [fake] * 4 + [256.0, 256.0, 32.0, 32.0] + \
            [C.byref(pol)] + [fake] * 11 + [fake, 1 << 30] + [fake, fake, high] + [fake] * 4 + \
            [None, None, None, phase | flags, 0, n, None, 0, None, None, C.byref(pg)]
        return lib.egs_fused_backward(*args)
    ok_ws = lib.egs_pose_ws_bytes(n)
    for raw in (False, True):
        assert call(1, _lib.EgsPoseGrad(256, 256, 256, ok_ws), raw) == 10001      # EGS_ERR_BAD_ARG
        assert call(2, _lib.EgsPoseGrad(256, 256, 256, ok_ws), raw) == 10001
        assert call(0, _lib.EgsPoseGrad(256, 256, 256, ok_ws - 1), raw) == 10002  # EGS_ERR_WORKSPACE
        assert call(0, _lib.EgsPoseGrad(256, 256, None, ok_ws), raw) == 10002
        assert call(0, _lib.EgsPoseGrad(None, 256, 256, ok_ws), raw) == 10001


def _cpu_inputs(n=8):
    import torch
    z = lambda *s: torch.zeros(*s, dtype=torch.float32)
    return (z(n, 3), z(n, 3), z(n, 1), z(n, 3), z(n, 4), z(n, 2))


def test_pose_nodes_refuse_ops_mode_and_exchange():
    torch = pytest.importorskip("torch")
    from easygaussiansplatting_amd.function import GSPoseFunction, GSRawPoseFunction, RenderOptions, Camera
    cam = Camera(64, 48, 256.0, 256.0, 32.0, 24.0, np.eye(3), np.zeros(3), device="cpu")
    R, t = torch.eye(3), torch.zeros(3)
    p = _cpu_inputs()
    with pytest.raises(ValueError, match="mode='fused'"):
        GSPoseFunction.apply(*p, R, t, cam, RenderOptions(mode="ops"))
    with pytest.raises(ValueError, match="ChunkedExchange"):
        GSPoseFunction.apply(*p, R, t, cam, RenderOptions(exchange=object()))
    raw = (p[0], p[1], torch.zeros(8, 0), p[2], p[3], p[4], p[5])
    with pytest.raises(ValueError, match="mode='fused'"):
        GSRawPoseFunction.apply(*raw, R, t, cam, RenderOptions(mode="ops"))
    with pytest.raises(ValueError, match="ChunkedExchange"):
        GSRawPoseFunction.apply(*raw, R, t, cam, RenderOptions(exchange=object()))


@pytest.mark.parametrize("bad, match", [
    (lambda torch: (torch.eye(4)[:3], torch.zeros(3)), "Rcw must have shape"),
    (lambda torch: (torch.eye(3), torch.zeros(3, 1)), "tcw must have shape"),
    (lambda torch: (torch.eye(3, dtype=torch.float64), torch.zeros(3)), "Rcw must be torch.float32"),
    (lambda torch: (torch.eye(3), torch.zeros(3, dtype=torch.float16)), "tcw must be torch.float32"),
    (lambda torch: (torch.eye(3), torch.zeros(3)), "Rcw must live on the device"),
    (lambda torch: (torch.eye(3).numpy(), torch.zeros(3)), "Rcw must be a torch.Tensor"),
])
def test_pose_nodes_refuse_bad_pose_tensors(bad, match):
    torch = pytest.importorskip("torch")
    from easygaussiansplatting_amd.function import GSPoseFunction, Camera
    from easygaussiansplatting_amd import fused
    cam = Camera(64, 48, 256.0, 256.0, 32.0, 24.0, np.eye(3), np.zeros(3), device="cpu")
    R, t = bad(torch)
    with pytest.raises(ValueError, match=match):
        GSPoseFunction.apply(*_cpu_inputs(), R, t, cam)
    with pytest.raises(ValueError, match=match):      # the same checks in fused.backward
        fused.pose_tensors(R, t, torch.zeros(1, 3))
