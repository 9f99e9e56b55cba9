"""Depth supervision, host side (no GPU): the float64 reference of tests/depth_loss_ref.py checked on itself (central
differences, invariance of "affine" and "pearson" under a scale and shift of the prior, the degenerate rules, the share
of pixels its comparison rule leaves out), the C surface of libegs_depthloss.so against include/egs_depthloss.h and its
refusals before any HIP call, the refusals of ``depth_loss_with_grad`` and ``Trainer(depth_priors=...)``,
``GSplatDataset(depths=True)`` and the flags of examples/train.py."""
import inspect
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import depth_loss_ref as DR
from tests import weighted_loss_ref as WR

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "egs_depthloss.h")
BAD_ARG, ERR_WORKSPACE = 10001, 10002
_FAKE = 4096                    # a pointer nobody dereferences: every call below is refused before any HIP call
NAMES = ["egs_depthloss", "egs_depthloss_abi_version", "egs_depthloss_last_error_string", "egs_depthloss_ws_bytes"]


# -------------------------------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("kind", DR.KINDS)
def test_reference_gradient_against_central_differences(kind, weighted):
    H, W = 7, 9
    D, A, q = DR.make_case(H, W, seed=1)
    A[2, 3] = 0.01                                       # below alpha_min: no gradient there
    w = WR.make_weight("uniform", H, W) if weighted else None
    base = DR.ref(D, A, q, kind, w, grad_scale=0.7)
    fit = (base["s"], base["t"]) if kind == "affine" else None      # (the gradient holds the fit constant)
    loss = lambda d, a: DR.ref(d, a, q, kind, w, fit=fit)["loss"]
    assert abs(loss(D, A) - base["loss"]) <= 1e-15
    D64, A64 = D.astype(np.float64), A.astype(np.float64)
    eps, worst, n = 1e-7, 0.0, 0
    for idx in np.ndindex(H, W):
        if base["e"] is not None and abs(base["e"][idx]) < 1e-4 and base["valid"][idx]:
            continue                                     # (the L1 kinds have a kink at e = 0)
        for name, P in (("dD", D64), ("dA", A64)):
            hi, lo = P.copy(), P.copy()
            hi[idx] += eps; lo[idx] -= eps
            fd = (loss(hi, A64) - loss(lo, A64)) if name == "dD" else (loss(D64, hi) - loss(D64, lo))
            worst = max(worst, abs(0.7 * fd / (2 * eps) - base[name][idx]))
            n += 1
    # the loss carries 1e-16 of rounding: 5e-10 in the quotient; the third derivative's term is eps^2
    assert n > 100 and worst <= 1e-8, worst
    assert np.abs(base["dD"]).max() > 1e-5 and np.abs(base["dA"]).max() > 1e-4
    assert base["dD"][2, 3] == 0 and base["dA"][2, 3] == 0 and not base["valid"][2, 3]


@pytest.mark.parametrize("kind", ["affine", "pearson"])
def test_scale_and_shift_of_the_prior_change_nothing(kind):
    D, A, q = DR.make_case(17, 65, seed=2)
    q = np.where(q > 0, q, 0).astype(np.float32)
    base = DR.ref(D, A, q, kind)
    for a, b in ((3.0, 0.25), (0.01, 0.0), (1.0, 7.0)):
        q2 = np.where(q > 0, a * q.astype(np.float64) + b, 0.0)       # (no data stays no data)
        got = DR.ref(D, A, q2, kind)
        assert abs(got["loss"] - base["loss"]) <= 1e-12, (a, b)
        for k in ("dD", "dA"):
            assert np.abs(got[k] - base[k]).max() <= 1e-9 * np.abs(base[k]).max(), (a, b, k)
    # "metric" is not
    assert abs(DR.ref(D, A, 3.0 * q, "metric")["loss"] - DR.ref(D, A, q, "metric")["loss"]) > 1e-3


def test_metric_on_the_rendered_disparity_is_zero():
    D, A, _ = DR.make_case(11, 11, seed=3)
    q = A.astype(np.float64) / D.astype(np.float64)
    got = DR.ref(D, A, q, "metric")
    assert got["loss"] == 0.0 and not got["dD"].any() and not got["dA"].any() and got["omega"] == 121.0
    fit = DR.ref(D, A, (q - 0.2) / 5.0, "affine")
    assert abs(fit["s"] - 5.0) <= 1e-9 and abs(fit["t"] - 0.2) <= 1e-9 and fit["loss"] <= 1e-12
    assert abs(DR.ref(D, A, (q - 0.2) / 5.0, "pearson")["loss"]) <= 1e-12


def test_degenerate_rules():
    H, W = 6, 8
    D, A, q = DR.make_case(H, W, seed=4)
    for kind in DR.KINDS:                                 # no valid pixel, however it comes about
        for bad in (np.zeros_like(q), -q - 1, np.full_like(q, np.nan), np.full_like(q, np.inf)):
            got = DR.ref(D, A, bad, kind)
            assert (got["loss"], got["s"], got["t"], got["omega"], got["rho"], got["degenerate"]) == (0, 1, 0, 0, 0, 1)
            assert not got["dD"].any() and not got["dA"].any()
        assert DR.ref(D, np.full_like(A, 0.05), np.abs(q) + 1, kind)["omega"] == 0        # A == alpha_min does not count
        assert DR.ref(D, np.nextafter(np.full_like(A, 0.05), np.float32(1)), np.abs(q) + 1, kind)["omega"] == H * W
        assert DR.ref(-D, A, np.abs(q) + 1, kind)["omega"] == 0
        w0 = np.zeros((H, W), np.float32)                 # valid pixels, but no weight
        assert DR.ref(D, A, np.abs(q) + 1, kind, w0)["degenerate"] == 1
    const = np.full((H, W), 0.3, np.float32)
    r = A.astype(np.float64) / D
    got = DR.ref(D, A, const, "affine")                   # a constant prior: a scale alone
    assert got["degenerate"] == 1 and got["t"] == 0.0 and abs(got["s"] - r.mean() / 0.3) <= 1e-6
    assert np.abs(got["dD"]).max() > 0
    one = np.zeros((H, W), np.float32); one[2, 5] = 0.4
    got = DR.ref(D, A, one, "affine")                     # fewer than two valid pixels
    assert got["degenerate"] == 1 and got["t"] == 0.0 and abs(got["s"] - r[2, 5] / np.float32(0.4)) <= 1e-12
    assert got["loss"] <= 1e-16 and got["omega"] == 1.0
    assert DR.ref(D, A, np.abs(q) + 0.1, "affine")["degenerate"] == 0
    for qq, dd in ((const, D), (np.abs(q) + 0.1, 2.0 * A)):      # pearson: a constant prior, a constant render
        got = DR.ref(dd, A, qq, "pearson")
        assert (got["loss"], got["rho"], got["degenerate"]) == (1.0, 0.0, 1)
        assert not got["dD"].any() and not got["dA"].any()
    assert DR.ref(D, A, np.abs(q) + 0.1, "metric")["degenerate"] == 0


@pytest.mark.parametrize("shape", DR.SHAPES, ids=lambda s: "%dx%d" % s)
def test_generated_cases_stay_within_the_exclusion_cap(shape):
    """in float64 and in the float32 restatement, which flips no sign outside the excluded set"""
    H, W = shape
    D, A, q = DR.make_case(H, W)
    # (1x1 is degenerate and 1x2 an exact fit: "affine" leaves residuals of rounding there, its stats are what is compared)
    for kind in ("metric", "affine") if H * W > 2 else ("metric",):
        want = DR.ref(D, A, q, kind)
        keep, n_out, n_valid = DR.compared(want)
        assert n_out <= DR.EXCLUDED_CAP * n_valid, (kind, n_out, n_valid)
        got = DR.ref(D, A, q, kind, dtype=np.float32)
        assert np.array_equal(np.sign(got["e"])[keep], np.sign(want["e"])[keep]), kind
    if H * W >= 100:
        assert 0.8 * H * W <= n_valid <= 0.95 * H * W


def test_rule_accepts_the_restatement_and_refuses_a_wrong_result():
    D, A, q = DR.make_case(33, 129)
    w = WR.make_weight("uniform", 33, 129)
    for kind in DR.KINDS:
        want = DR.ref(D, A, q, kind, w)
        f32 = DR.ref(D, A, q, kind, w, dtype=np.float32)
        e_ref = DR.errors(f32, want)
        DR.check_against(f32, want, kind, e_ref)
        bad = dict(f32); bad["dD"] = f32["dD"] * np.float32(1.001)
        with pytest.raises(AssertionError, match="dD off by"):
            DR.check_against(bad, want, kind, e_ref)
        bad = dict(f32); bad["loss"] = f32["loss"] * 1.001
        with pytest.raises(AssertionError, match="loss off by"):
            DR.check_against(bad, want, kind, e_ref)


# -------------------------------------------------------------------------------------------------------- the C surface
@pytest.fixture(scope="module")
def lib():
    from easygaussiansplatting_amd import _depthlosslib, _lib
    if not os.path.exists(_depthlosslib.LIB_PATH):
        _lib.build()
    return _depthlosslib.load()


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    return sorted(ln.split()[-1] for ln in out.splitlines() if ln.strip() and ln.split()[-1].startswith("egs_"))


def test_library_exports_what_its_header_declares(lib):
    from easygaussiansplatting_amd import _depthlosslib
    assert _exports(_depthlosslib.LIB_PATH) == NAMES
    assert sorted(_depthlosslib.SIGNATURES) == NAMES
    hdr = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(set(re.findall(r"\b(egs_[a-z0-9_]+)\s*\(", code))) == NAMES
    assert re.search(r"^#define\s+EGS_DEPTHLOSS_ABI_VERSION\s+1\s*$", hdr, re.M)
    assert lib.egs_depthloss_abi_version() == 1 == _depthlosslib.ABI_VERSION
    m = re.search(r"^#define\s+EGS_DEPTHLOSS_MAX_PIXELS\s+\(1 << (\d+)\)\s*$", hdr, re.M)
    assert m and 1 << int(m.group(1)) == _depthlosslib.MAX_PIXELS
    for name, value in _depthlosslib.KINDS.items():
        assert re.search(r"^#define\s+EGS_DEPTHLOSS_%s\s+%d\s*$" % (name.upper(), value), hdr, re.M), name
    assert "stop-gradient" in hdr


def test_libegs_hip_is_untouched():
    from easygaussiansplatting_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    assert _lib.ABI_VERSION == 12 and _lib.load().egs_abi_version() == 12
    assert not any("depthloss" in n for n in _lib.SIGNATURES)


def test_workspace_size(lib):
    for H, W in ((1, 1), (17, 65), (1080, 1920), (4000, 6000)):
        g = min(-(-(-(-H * W // 4)) // 256), 512)
        got = int(lib.egs_depthloss_ws_bytes(H, W))
        assert got % 256 == 0 and 72 * g + 4 <= got <= 72 * g + 5 * 256
    assert lib.egs_depthloss_ws_bytes(0, 5) == 256 and lib.egs_depthloss_ws_bytes(5, -1) == 256


def test_bad_arguments_and_a_short_workspace_are_refused_without_a_device(lib):
    P = _FAKE
    H, W = 17, 65
    need = int(lib.egs_depthloss_ws_bytes(H, W))

    def call(H=H, W=W, depth=P, alpha=2 * P, prior=3 * P, weight=4 * P, kind=1, alpha_min=0.05, scale=1.0, ws=5 * P,
             ws_bytes=need, out=6 * P, dd=7 * P, da=8 * P):
        return lib.egs_depthloss(H, W, depth, alpha, prior, weight, kind, alpha_min, scale, ws, ws_bytes, out, dd, da,
                                 None)

    def refused(rc):
        assert rc == BAD_ARG, rc
        msg = lib.egs_depthloss_last_error_string().decode()
        assert msg.startswith("egs_depthloss error 10001: bad argument"), msg

    for size in ("H", "W"):
        for bad in (0, -3):
            refused(call(**{size: bad}))
    refused(call(H=1 << 15, W=(1 << 13) + 1))           # beyond EGS_DEPTHLOSS_MAX_PIXELS
    for name in ("depth", "alpha", "prior", "ws", "out"):
        refused(call(**{name: None}))
        refused(call(**{name: P + 2}))                  # not 4-B aligned
    refused(call(ws=5 * P + 4))                         # the workspace holds doubles
    refused(call(weight=P + 2))
    for bad in (-1, 3):
        refused(call(kind=bad))
    for bad in (-0.1, float("nan"), float("inf")):
        refused(call(alpha_min=bad))
    for bad in (float("nan"), float("inf")):
        refused(call(scale=bad))
    refused(call(dd=7 * P + 1))
    refused(call(dd=None))                              # one gradient plane without the other
    refused(call(da=None))
    refused(call(da=7 * P))                             # the two planes are one
    for inp in (P, 2 * P, 3 * P, 4 * P):                # a gradient plane may not overwrite an input
        refused(call(dd=inp))
        refused(call(da=inp))
    for short in (need - 1, 0):
        assert call(ws_bytes=short) == ERR_WORKSPACE
        msg = lib.egs_depthloss_last_error_string().decode()
        assert msg.startswith("egs_depthloss error 10002") and "workspace" in msg, msg
        assert call(ws_bytes=short, dd=None, da=None, weight=None) == ERR_WORKSPACE


def test_source_reads_no_environment_variable_and_adds_no_float_atomic():
    src = open(os.path.join(REPO, "easygaussiansplatting_amd", "csrc", "egs_depthloss.hip")).read()
    assert "getenv" not in src
    assert re.findall(r"atomic\w*\(", src) == ["atomicAdd("] and "atomicAdd(counter, 1u)" in src


# ---------------------------------------------------------------------------------------------------- the Python surface
def test_signatures():
    from easygaussiansplatting_amd import depthloss
    from easygaussiansplatting_amd.trainer import Trainer
    assert list(inspect.signature(depthloss.depth_loss_with_grad).parameters) == [
        "depth", "alpha", "prior", "kind", "weight", "alpha_min", "grad_scale", "need_grad"]
    d = {k: v.default for k, v in inspect.signature(depthloss.depth_loss_with_grad).parameters.items()}
    assert (d["kind"], d["weight"], d["alpha_min"], d["grad_scale"], d["need_grad"]) == ("affine", None, 0.05, 1.0, True)
    assert list(inspect.signature(depthloss.depth_loss).parameters)[:3] == ["depth", "alpha", "prior"]
    p = inspect.signature(Trainer.__init__).parameters
    assert (p["depth_priors"].default, p["depth_kind"].default, p["depth_weight"].default,
            p["depth_alpha_min"].default) == (None, "affine", (1.0, 0.01), 0.05)
    assert "tuned" in depthloss.__doc__.lower() and "tuned" in Trainer.__init__.__doc__.lower()


def test_depth_loss_refusals():
    from easygaussiansplatting_amd.depthloss import depth_loss, depth_loss_with_grad
    H, W = 6, 8
    d, a, q = torch.ones((1, H, W)), torch.ones((1, H, W)), torch.ones((H, W))
    bad = [
        (dict(depth=torch.ones((3, H, W))), "depth must have shape"),
        (dict(depth=torch.ones((H,))), "depth must have shape"),
        (dict(depth=d.double()), "depth must be torch.float32"),
        (dict(alpha=torch.ones((1, H, W + 1))), "alpha must have shape"),
        (dict(alpha=a.half()), "alpha must be torch.float32"),
        (dict(prior=torch.ones((W, H))), "prior must have shape"),
        (dict(prior=q.to(torch.int32)), "prior must be torch.float32"),
        (dict(weight=torch.ones((H, W), dtype=torch.bool)), "weight must be torch.float32"),
        (dict(weight=torch.ones((1, H + 1, W))), "weight must have shape"),
        (dict(kind="l2"), "kind must be one of"),
        (dict(alpha_min=-1.0), "alpha_min must be finite"),
    ]
    for kw, msg in bad:
        args = dict(depth=d, alpha=a, prior=q)
        args.update(kw)
        for fn in (depth_loss, depth_loss_with_grad):
            with pytest.raises(ValueError, match=msg):
                fn(**args)
    with pytest.raises(TypeError, match="prior must be a torch.Tensor"):
        depth_loss_with_grad(d, a, np.ones((H, W), np.float32))
    # good planes pass their own checks; the call is then refused for want of a GPU tensor
    for dd in (d, d[0]):
        with pytest.raises(ValueError, match="depth must live on the GPU"):
            depth_loss_with_grad(dd, a, q, weight=q)


def test_trainer_refusals_and_the_prior_checker():
    from easygaussiansplatting_amd.trainer import Trainer, _checked_depth_priors
    H, W = 6, 8
    gts = [torch.zeros((3, H, W)) for _ in range(3)]
    ones = torch.ones((H, W))
    make = lambda dp, **kw: Trainer(None, [], gts, 10, device="cpu", depth_priors=dp, **kw)
    with pytest.raises(ValueError, match="2 entries for 3 views"):
        make([ones, ones])
    with pytest.raises(ValueError, match=r"view 1 has shape \[8, 6\]"):
        make([ones, ones.t(), None])
    with pytest.raises(ValueError, match="view 2 has shape"):
        make([None, None, torch.ones((1, H, W))])
    with pytest.raises(ValueError, match="view 0 must be a float32 tensor"):
        make([ones.double(), None, None])
    with pytest.raises(ValueError, match="view 0 must be a float32 tensor"):
        make([np.ones((H, W), np.float32), None, None])
    for fill in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="view 1 has no positive finite pixel"):
            make([ones, torch.full((H, W), fill), None])
    with pytest.raises(ValueError, match="absgrad"):
        make([ones, None, None], absgrad=True)
    with pytest.raises(ValueError, match="needs mode='fused'"):
        make([ones, None, None], mode="ops", fused_activations=False)
    with pytest.raises(ValueError, match="depth_kind"):
        make([ones, None, None], depth_kind="l2")
    for bad in ((1.0, 0.0), (0.0, 1.0), (1.0,), "x", -1.0, (1.0, float("inf"))):
        with pytest.raises(ValueError, match="depth_weight"):
            make([ones, None, None], depth_weight=bad)
    with pytest.raises(ValueError, match="depth_alpha_min"):
        make([ones, None, None], depth_alpha_min=-0.5)
    # what passes: a plane with holes, NaNs and one good pixel stays as it is
    holes = torch.zeros((H, W)); holes[1, 2] = 0.5; holes[0, 0] = float("nan"); holes[3, 3] = -2.0
    got = _checked_depth_priors([holes, None, ones], gts, "cpu")
    assert got[1] is None and got[0].dtype == torch.float32 and torch.equal(got[2], ones)
    assert torch.equal(got[0].nan_to_num(7.0), holes.nan_to_num(7.0))
    assert _checked_depth_priors(None, gts, "cpu") is None
    # the constructor calls of the other host-side tests still end where they did
    with pytest.raises(ValueError, match="cap_max"):
        Trainer(None, [], [], 10, strategy="mcmc", depth_priors=[])


def test_weight_schedule():
    from easygaussiansplatting_amd.trainer import Trainer
    tr = Trainer.__new__(Trainer)
    tr.max_steps, tr.depth_weight = 200, (1.0, 0.01)
    assert tr.depth_weight_at(0) == 1.0
    assert abs(tr.depth_weight_at(100) - 0.1) <= 1e-15 and abs(tr.depth_weight_at(50) - 10 ** -0.5) <= 1e-15
    assert abs(tr.depth_weight_at(200) - 0.01) <= 1e-17 and tr.depth_weight_at(500) == tr.depth_weight_at(200)
    tr.depth_weight = (0.3, 0.3)
    assert tr.depth_weight_at(0) == tr.depth_weight_at(77) == 0.3


# ------------------------------------------------------------------------------------------------------------ the dataset
def test_dataset_collects_depth_priors(tmp_path):
    from PIL import Image
    from easygaussiansplatting_amd import scene as S
    from easygaussiansplatting_amd.dataset import GSplatDataset, _nearest
    from tests.colmap_fixture import write_scene
    Hh, Ww = 16, 24
    sc = S.small_scene(50, Ww, Hh, 3, seed=4)
    cams = S.ring_cameras(sc.cam, 4, radius=5.0)
    rng = np.random.default_rng(3)
    imgs = [rng.integers(0, 256, (Hh, Ww, 3), dtype=np.uint8) for _ in cams]
    root = str(tmp_path / "scene")
    write_scene(root, cams, imgs, sc.pws, np.full((50, 3), 128, np.uint8))
    # (the initial Gaussians come from the cache the dataset keeps next to the model: building it is a GPU kNN)
    np.save(os.path.join(root, "sparse", "0", "points3D.npy"), np.zeros(50, np.float32))
    os.makedirs(os.path.join(root, "depths"))
    q0 = rng.uniform(0.05, 2.0, (Hh, Ww)).astype(np.float32); q0[::2, 1::2] = 0.0          # holes on every other pixel
    q1 = rng.integers(1, 65536, (Hh, Ww)).astype(np.uint16); q1[4:9, 3:11] = 0
    q2 = rng.uniform(0.05, 2.0, (Hh // 2, Ww // 2)).astype(np.float32)                     # a prior at half the size
    np.save(os.path.join(root, "depths", "view_00.npy"), q0)
    Image.fromarray(q1).save(os.path.join(root, "depths", "view_01.png"))
    assert Image.open(os.path.join(root, "depths", "view_01.png")).mode == "I;16"
    np.save(os.path.join(root, "depths", "view_02.npy"), q2)
    plain = GSplatDataset(root, device="cpu")
    assert plain.depth_priors is None and plain.depth_kind is None and len(plain) == 4
    ds = GSplatDataset(root, device="cpu", depths=True)
    assert ds.depth_kind == "affine" and len(ds.depth_priors) == 4 and ds.depth_priors[3] is None
    for got in ds.depth_priors[:3]:
        assert got.dtype == torch.float32 and tuple(got.shape) == (Hh, Ww) and got.is_contiguous()
    assert np.array_equal(ds.depth_priors[0].numpy(), q0)
    assert np.array_equal(ds.depth_priors[1].numpy(), (q1.astype(np.float64) / 65536.0).astype(np.float32))
    assert np.array_equal(ds.depth_priors[2].numpy(), np.repeat(np.repeat(q2, 2, 0), 2, 1))
    for a, b in zip(ds.images, plain.images):                                     # the images are what they were
        assert torch.equal(a, b)
    # .npy wins over .png
    Image.fromarray(q1).save(os.path.join(root, "depths", "view_00.png"))
    assert np.array_equal(GSplatDataset(root, device="cpu", depths=True).depth_priors[0].numpy(), q0)
    # resized with the image, by nearest sampling: every value is one of the source's, a hole stays a hole
    half = GSplatDataset(root, resize_rate=0.5, device="cpu", depths=True)
    for k in range(3):
        assert tuple(half.depth_priors[k].shape) == (Hh // 2, Ww // 2) == tuple(half.images[k].shape[1:])
    h0 = half.depth_priors[0].numpy()
    assert np.array_equal(h0, q0[1::2, 1::2]) and (h0[:, :] == 0).sum() == 0
    third = _nearest(q0, 7, 5)
    assert third.shape == (5, 7) and np.isin(third, q0).all() and (third == 0).any() and (third > 0).any()
    assert np.array_equal(half.depth_priors[2].numpy(), q2)
    # depth_params.json: the priors become metric; an image it does not list has none
    with open(os.path.join(root, "sparse", "0", "depth_params.json"), "w") as f:
        json.dump({"view_00": {"scale": 2.0, "offset": 0.5}, "view_01": {"scale": 0.5, "offset": 0.0}}, f)
    met = GSplatDataset(root, device="cpu", depths=True)
    assert met.depth_kind == "metric" and met.depth_priors[2] is None and met.depth_priors[3] is None
    assert np.array_equal(met.depth_priors[0].numpy(), np.where(q0 > 0, np.float32(2) * q0 + np.float32(0.5), 0))
    assert np.array_equal(met.depth_priors[1].numpy(), np.float32(0.5) * ds.depth_priors[1].numpy())
    assert GSplatDataset(root, device="cpu").depth_kind is None


def test_train_example_lists_the_flags():
    r = subprocess.run([sys.executable, os.path.join(REPO, "examples", "train.py"), "--help"], capture_output=True,
                       text=True, cwd=REPO)
    assert r.returncode == 0, r.stderr
    for flag in ("--depths", "--depth-kind", "--depth-weight INIT FINAL"):
        assert flag in r.stdout, flag
