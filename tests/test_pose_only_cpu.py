"""Pose-only backward pass and the pose module, host side (no GPU): the EGS_BWD_POSE_ONLY bit of the C ABI and its
refusals before the device, ``RenderOptions(pose_only=True)``, ``pose.exp_so3`` against a float64 Rodrigues, and the
per-row Adam of ``pose.PoseTable`` against ``torch.optim.Adam`` on a row alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.test_cabi_and_host import BAD_ARG, HEADER, WORKSPACE, declared_functions
from tests.test_pose_grad_cpu import rodrigues

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def lib():
    from easygaussiansplatting_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------- the C ABI
def test_the_bit_is_declared_and_the_abi_is_unchanged(lib):
    from easygaussiansplatting_amd import _lib, fused
    src = open(HEADER).read()
    assert re.search(r"^#define\s+EGS_BWD_POSE_ONLY\s+2048\s*$", src, re.M)
    assert fused.POSE_ONLY == 2048
    assert re.search(r"^#define\s+EGS_ABI_VERSION\s+12\s*$", src, re.M) and lib.egs_abi_version() == 12
    assert set(_lib.SIGNATURES) == set(declared_functions())
    # no other phase bit shares it
    others = (fused.KEEP_FORWARD_ORDER, fused.ACCUMULATE, fused.FACTORED_SH, fused.ABSGRAD, fused.CULLED_LISTS,
              fused.ANTIALIASED, fused.RAW, 1, 2)
    assert all(fused.POSE_ONLY & b == 0 for b in others)


def _backward(lib, phase, pose=True, pose_ws_bytes=None, outputs=None, raw=False, n=1000):
    """egs_fused_backward on pointers nobody dereferences.  The MAIN workspace is 16 bytes: a call that passed every
    argument check would still end in EGS_ERR_WORKSPACE, never in a launch."""
    from easygaussiansplatting_amd import _lib, fused
    pol = _lib.EgsPolicy()
    lib.egs_policy_gsplatcu(C.byref(pol))
    fake = C.c_void_p(4096)
    high, flags = (fake, fused.RAW) if raw else (None, 0)
    pg = None
    if pose:
        pg = C.byref(_lib.EgsPoseGrad(4096, 4096, 4096, lib.egs_pose_ws_bytes(n) if pose_ws_bytes is None
                                      else pose_ws_bytes))
    args = [n, 12, 0, 64, 64] + [fake] * 4 + [high] + [fake] * 4 + [256.0, 256.0, 32.0, 32.0] + \
        [C.byref(pol)] + [fake] * 11 + [fake, 16] + [outputs] * 2 + [outputs if raw else None] + [outputs] * 4 + \
        [None, fake, None, phase | flags, 0, n, None, 0, None, None, pg]
    return lib.egs_fused_backward(*args)


@pytest.mark.parametrize("raw", [False, True])
def test_excluded_combinations_are_refused_before_the_device(lib, raw):
    from easygaussiansplatting_amd.fused import ABSGRAD, ACCUMULATE, FACTORED_SH, POSE_ONLY
    fake = C.c_void_p(4096)
    assert _backward(lib, POSE_ONLY, pose=False, outputs=fake, raw=raw) == BAD_ARG
    for extra in (1, 2, ACCUMULATE, FACTORED_SH, ABSGRAD):
        for outputs in (fake, None):
            assert _backward(lib, POSE_ONLY | extra, outputs=outputs, raw=raw) == BAD_ARG, (extra, outputs)


@pytest.mark.parametrize("raw", [False, True])
def test_null_outputs_pass_the_argument_check(lib, raw):
    """the bit, a pose, a short pose workspace, NULL per-Gaussian outputs: EGS_ERR_WORKSPACE (without the bit in the
    phase mask the call was a bad argument); with a good pose workspace the NULLs get through the output check, which
    stands behind it, as far as the size of the main workspace -- where the same NULLs without the bit are refused"""
    from easygaussiansplatting_amd.fused import POSE_ONLY
    short = lib.egs_pose_ws_bytes(1000) - 1
    assert _backward(lib, POSE_ONLY, pose_ws_bytes=short, outputs=None, raw=raw) == WORKSPACE
    assert b"pose workspace" in lib.egs_last_error_string()
    assert _backward(lib, POSE_ONLY, outputs=None, raw=raw) == WORKSPACE
    assert b"pose" not in lib.egs_last_error_string()
    assert _backward(lib, 0, outputs=None, raw=raw) == BAD_ARG


# ------------------------------------------------------------------------------------------------------ RenderOptions
def test_render_options_pose_only():
    from easygaussiansplatting_amd.function import RenderOptions
    assert RenderOptions().pose_only is False
    o = RenderOptions(pose_only=True, antialiased=True, depth=True, background=(0.1, 0.2, 0.3))
    assert o.pose_only is True and o.mode == "fused"
    for bad in (dict(mode="ops"), dict(accumulate=True), dict(sh_sink=object()), dict(exchange=object()),
                dict(absgrad=True)):
        with pytest.raises(ValueError):
            RenderOptions(pose_only=True, **bad)
    for not_bool in (1, 0, "yes", None):
        with pytest.raises(ValueError, match="pose_only must be a bool"):
            RenderOptions(pose_only=not_bool)


def test_non_pose_nodes_refuse_the_option():
    from easygaussiansplatting_amd.function import Camera, GSFunction, GSRawFunction, RenderOptions
    cam = Camera(64, 48, 256.0, 256.0, 32.0, 24.0, np.eye(3), np.zeros(3), device="cpu")
    z = lambda *s: torch.zeros(*s, dtype=torch.float32)
    n = 8
    o = RenderOptions(pose_only=True)
    with pytest.raises(ValueError, match="pose_only"):
        GSFunction.apply(z(n, 3), z(n, 3), z(n, 1), z(n, 3), z(n, 4), z(n, 2), cam, o)
    with pytest.raises(ValueError, match="pose_only"):
        GSRawFunction.apply(z(n, 3), z(n, 3), z(n, 9), z(n, 1), z(n, 3), z(n, 4), z(n, 2), cam, o)


# ---------------------------------------------------------------------------------------------------- the pose module
@pytest.mark.parametrize("theta", [0.0, 1e-7, 1e-3, 1.0])
def test_exp_so3_against_float64_rodrigues(theta):
    """float64 torch against the float64 Rodrigues of tests/test_pose_grad_cpu.py: 1e-14 (both sides round a handful
    of float64 operations on entries <= 1; the series branch below |w|^2 = 1e-12 drops terms of order |w|^4 / 120 <
    1e-26); float32: 4 float32 ulps of 1 (5e-7)"""
    from easygaussiansplatting_amd.pose import apply_twist, exp_so3
    axis = np.array([0.3, -0.5, 0.81]); axis /= np.linalg.norm(axis)
    w = axis * theta
    ref = rodrigues(w)
    got = exp_so3(torch.tensor(w, dtype=torch.float64)).numpy()
    assert np.abs(got - ref).max() <= 1e-14
    got32 = exp_so3(torch.tensor(w, dtype=torch.float32)).double().numpy()
    assert np.abs(got32 - ref).max() <= 5e-7
    R0, t0, rho = rodrigues([0.2, 0.1, -0.3]), np.array([0.1, -0.2, 5.0]), np.array([0.01, 0.02, -0.03])
    R, t = apply_twist(*(torch.tensor(a, dtype=torch.float64) for a in (R0, t0, w, rho)))
    assert np.abs(R.numpy() - ref @ R0).max() <= 1e-14 and np.abs(t.numpy() - (ref @ t0 + rho)).max() <= 1e-13


@pytest.mark.parametrize("theta", [0.0, 1e-7, 1e-3, 1.0])
def test_exp_so3_autograd_against_central_differences(theta):
    """d<G, exp(w)>/dw in float64 against central differences of the float64 Rodrigues with h = 1e-6 (truncation
    h^2 |f'''| / 6 ~ 1e-13, rounding 1e-16 / h = 1e-10): held to 1e-8"""
    from easygaussiansplatting_amd.pose import exp_so3
    axis = np.array([-0.6, 0.2, 0.77]); axis /= np.linalg.norm(axis)
    w0 = axis * theta
    G = np.random.default_rng(3).normal(size=(3, 3))
    w = torch.tensor(w0, dtype=torch.float64, requires_grad=True)
    (exp_so3(w) * torch.tensor(G)).sum().backward()
    assert torch.isfinite(w.grad).all()
    h = 1e-6
    num = np.zeros(3)
    for k in range(3):
        d = np.zeros(3); d[k] = h
        num[k] = ((rodrigues(w0 + d) - rodrigues(w0 - d)) * G).sum() / (2 * h)
    assert np.abs(w.grad.numpy() - num).max() <= 1e-8, (w.grad.numpy(), num)


class _Cam:
    def __init__(self, k):
        self.Rcw = rodrigues([0.1 * k, -0.05, 0.02 * k]).astype(np.float32)
        self.tcw = np.array([0.1 * k, -0.2, 4.0 + k], np.float32)


def test_pose_table_steps_rows_like_adam_on_the_row_alone():
    """five steps with a changing subset of the cameras.  Rows outside a step: twist, both moments and the step count
    bitwise unchanged.  A stepped row: ``torch.equal`` to ``torch.optim.Adam`` (single-tensor implementation, the two
    halves as two parameter groups) that saw this row's gradients alone -- the table issues the same torch ops in the
    same order with the same host scalars, so not even one ulp is granted."""
    from easygaussiansplatting_amd.pose import LR_ROT, LR_TRANS, PoseTable
    cams = [_Cam(k) for k in range(4)]
    tab = PoseTable(cams, "cpu")
    assert len(tab) == 4 and tab.twist.shape == (4, 6) and not tab.twist.any()
    refs = []
    for c in cams:
        om, rh = torch.zeros(3, requires_grad=True), torch.zeros(3, requires_grad=True)
        dist = float(np.linalg.norm(c.tcw.astype(np.float64)))
        opt = torch.optim.Adam([{"params": [om], "lr": LR_ROT}, {"params": [rh], "lr": LR_TRANS * dist}], foreach=False)
        refs.append((om, rh, opt))
    gen = torch.Generator().manual_seed(5)
    schedule = ([0, 2], [2], [1, 2, 3], [0], [2, 3])
    for ids in schedule:
        grad = torch.randn((4, 6), generator=gen) * 1e-3
        grad[[v for v in range(4) if v not in ids]] = float("nan")     # rows outside the step are not even read
        before = [t.clone() for t in (tab.twist, tab.exp_avg, tab.exp_avg_sq, tab.steps)]
        tab.step(ids, grad)
        for v in range(4):
            if v in ids:
                om, rh, opt = refs[v]
                om.grad, rh.grad = grad[v, :3].clone(), grad[v, 3:].clone()
                opt.step()
                assert torch.equal(tab.twist[v, :3], om.detach()) and torch.equal(tab.twist[v, 3:], rh.detach()), v
                assert torch.equal(tab.exp_avg[v, :3], opt.state[om]["exp_avg"])
                assert torch.equal(tab.exp_avg_sq[v, 3:], opt.state[rh]["exp_avg_sq"])
                assert int(tab.steps[v]) == int(opt.state[om]["step"]) == int(before[3][v]) + 1
            else:
                for now, was in zip((tab.twist, tab.exp_avg, tab.exp_avg_sq, tab.steps), before):
                    assert torch.equal(now[v], was[v]), v
    assert tab.steps.tolist() == [2, 1, 4, 2] and torch.isfinite(tab.twist).all()
    R, t = tab.poses()
    assert R.shape == (4, 3, 3) and t.shape == (4, 3)
    Rv, tv = tab.pose(2)
    want = rodrigues(tab.twist[2, :3].double().numpy()) @ cams[2].Rcw.astype(np.float64)
    assert np.abs(Rv.double().numpy() - want).max() <= 5e-7 and torch.equal(R[2], Rv) and torch.equal(t[2], tv)


def test_trainer_pose_opt_needs_the_fused_path():
    from easygaussiansplatting_amd import scene as S
    from easygaussiansplatting_amd.trainer import Trainer
    sc = S.small_scene(16, 32, 32, 3, seed=1)
    with pytest.raises(ValueError, match="pose_opt"):
        Trainer(sc, [], [], max_steps=1, device="cpu", mode="ops", fused_activations=False, pose_opt=True)
