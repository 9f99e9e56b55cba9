"""The normal terms, host side (no GPU): the float64 reference of tests/normal_loss_ref.py checked on itself (central
differences, the analytic normal of a plane, the degenerate rules, its comparison rule), the C surface of
libegs_normalloss.so against include/egs_normalloss.h and its refusals before any HIP call, the refusals of
``normal_loss_with_grad`` and ``Trainer(normal_priors=..., normal_smooth=...)``, ``GSplatDataset(normals=True)`` and the
flags of examples/train.py."""
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import normal_loss_ref as NR

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "egs_normalloss.h")
BAD_ARG, ERR_WORKSPACE = 10001, 10002
_FAKE = 4096                    # a pointer nobody dereferences: every call below is refused before any HIP call
NAMES = ["egs_normalloss", "egs_normalloss_abi_version", "egs_normalloss_last_error_string", "egs_normalloss_ws_bytes"]


# -------------------------------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("kind", NR.KINDS)
def test_reference_gradient_against_central_differences(kind, weighted):
    H, W = 7, 9
    case, cam = NR.make_case(H, W, kind, seed=1)
    case["A"] = np.where(case["A"] < 0.06, np.float32(0.3), case["A"]).astype(np.float32)
    case["A"][2, 3] = 0.01                               # below alpha_min: no gradient there, no normal around it
    base = NR.ref(case, cam, weighted=weighted, prior_scale=0.7, smooth_scale=1.3)
    assert base["count"] == 5 * 7 - 5 and not base["dvalid"][2, 3]

    def loss(D, A):
        o = NR.forward(torch.from_numpy(D), torch.from_numpy(A), cam, torch.from_numpy(case["q"]).double(),
                       torch.from_numpy(case["I"]).double(), torch.from_numpy(case["w"]).double() if weighted else None)
        return 0.7 * float(o["Lp"]) + 1.3 * float(o["Ls"])

    D64, A64 = case["D"].astype(np.float64), case["A"].astype(np.float64)
    assert abs(loss(D64, A64) - (0.7 * base["Lp"] + 1.3 * base["Ls"])) <= 1e-15
    eps, worst, n = 1e-6, 0.0, 0
    for idx in np.ndindex(H, W):
        for name, P in (("dD", D64), ("dA", A64)):
            hi, lo = P.copy(), P.copy()
            hi[idx] += eps; lo[idx] -= eps
            fd = (loss(hi, A64) - loss(lo, A64)) if name == "dD" else (loss(D64, hi) - loss(D64, lo))
            worst = max(worst, abs(fd / (2 * eps) - base[name][idx]))
            n += 1
    top = max(np.abs(base["dD"]).max(), np.abs(base["dA"]).max())
    # the loss carries 1e-16 of rounding: 1e-10 in the quotient; the third derivative's term is eps^2 x O(top / z^2)
    assert n == 2 * H * W and top > 1e-3 and worst <= 1e-8 * max(top, 1.0), (worst, top)
    assert base["dD"][2, 3] == 0 and base["dA"][2, 3] == 0
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        assert base["dD"][y, x] == 0 and base["dA"][y, x] == 0      # a corner is nobody's neighbour
    # a border pixel is the end of its inner neighbour's difference ((0, 3): that neighbour lost its normal to the hole)
    assert np.all(base["dD"][0, [1, 2, 4, 5, 6, 7]] != 0) and base["dD"][0, 3] == 0 and np.all(base["dD"][1:-1, 0] != 0)


def test_plane_has_its_analytic_normal_and_no_smoothness_loss():
    H, W = 17, 65
    case, cam = NR.make_case(H, W, "plane")
    z = case["D"].astype(np.float64) / case["A"]
    case = dict(case, A=np.ones((H, W), np.float32), D=z.astype(np.float32))
    got = NR.ref(case, cam, prior=False, guide=False)
    # z (1 + 0.4 X - 0.25 Y) = 4 is the plane (0.4, -0.25, 1) . p = 4; the normal faces the camera
    want = -np.array([0.4, -0.25, 1.0]) / np.linalg.norm([0.4, -0.25, 1.0])
    assert got["count"] == (H - 2) * (W - 2) and got["nvalid"][1:-1, 1:-1].all() and not got["nvalid"][0].any()
    err = np.abs(got["n"][:, 1:-1, 1:-1] - want[:, None, None]).max()
    assert err <= 1e-5, err                              # (the inputs are float32: the issue's prototype showed 2.3e-6)
    assert 0 <= got["Ls"] <= 1e-10, got["Ls"]
    assert not got["n"][:, 0].any() and not got["n"][:, :, -1].any()
    front = dict(case, D=np.full((H, W), 3.0, np.float32))
    n = NR.ref(front, cam, prior=False)["n"][:, 1:-1, 1:-1]
    assert np.abs(n - np.array([0.0, 0.0, -1.0])[:, None, None]).max() <= 1e-15      # fronto-parallel: (0, 0, -1)


def test_degenerate_rules_and_small_planes():
    for H, W in ((1, 1), (1, 7), (7, 1), (2, 2), (2, 9)):
        case, cam = NR.make_case(H, W, "noise")
        got = NR.ref(case, cam)
        assert (got["count"], got["Lp"], got["Ls"], got["Op"], got["Os"], got["flags"]) == (0, 0, 0, 0, 0, 3)
        assert not got["dD"].any() and not got["dA"].any() and not got["n"].any()
    case, cam = NR.make_case(3, 3, "plane")
    case["A"][:] = 0.5
    case["D"][:] = 1.0
    case["q"][:] = np.array([0, 0, -2], np.float32)[:, None, None]      # (normalised by the loss)
    got = NR.ref(case, cam)
    assert got["count"] == 1 and got["Op"] == 1 and got["Os"] == 0 and got["flags"] == 2 and abs(got["Lp"]) <= 1e-15
    for bad in (0.0, np.nan, np.inf):
        c2 = dict(case, q=np.full_like(case["q"], bad))
        got = NR.ref(c2, cam)
        assert got["Op"] == 0 and got["flags"] == 3 and got["Lp"] == 0
    assert NR.ref(case, cam, prior=False, smooth=False)["flags"] == 0
    # alpha_min is exclusive
    c2 = dict(case, A=np.full((3, 3), 0.05, np.float32))
    assert NR.ref(c2, cam)["count"] == 0
    c2 = dict(case, A=np.full((3, 3), np.nextafter(np.float32(0.05), np.float32(1)), np.float32))
    assert NR.ref(c2, cam)["count"] == 1


def test_rule_accepts_the_restatement_and_refuses_a_wrong_result():
    case, cam = NR.make_case(17, 65, "wavy")
    want = NR.ref(case, cam, weighted=True)
    f32 = NR.ref(case, cam, weighted=True, dtype=torch.float32)
    e_ref = NR.errors(f32, want)
    NR.check_against(f32, want, "wavy", e_ref)
    bad = dict(f32); bad["dD"] = f32["dD"] * np.float32(1.001)
    with pytest.raises(AssertionError, match="dD off by"):
        NR.check_against(bad, want, "wavy", e_ref)
    bad = dict(f32); bad["Ls"] = f32["Ls"] * 1.01
    with pytest.raises(AssertionError, match="Ls off by"):
        NR.check_against(bad, want, "wavy", e_ref)
    bad = dict(f32); bad["nvalid"] = f32["nvalid"].copy(); bad["nvalid"][3, 3] ^= True
    with pytest.raises(AssertionError, match="set of pixels"):
        NR.check_against(bad, want, "wavy", e_ref)


@pytest.mark.parametrize("shape", [(3, 3), (3, 4), (5, 5), (17, 65), (70, 150)], ids=lambda s: "%dx%d" % s)
def test_generated_cases_leave_no_pixel_out(shape):
    """float32 and float64 agree on every pixel's validity"""
    for kind in NR.KINDS:
        case, cam = NR.make_case(*shape, kind)
        assert np.array_equal(NR.ref(case, cam)["nvalid"], NR.ref(case, cam, dtype=torch.float32)["nvalid"]), kind


# -------------------------------------------------------------------------------------------------------- the C surface
@pytest.fixture(scope="module")
def lib():
    from easygaussiansplatting_amd import _lib, _normallosslib
    if not os.path.exists(_normallosslib.LIB_PATH):
        _lib.build()
    return _normallosslib.load()


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    return sorted(ln.split()[-1] for ln in out.splitlines() if ln.strip() and ln.split()[-1].startswith("egs_"))


def test_library_exports_what_its_header_declares(lib):
    from easygaussiansplatting_amd import _normallosslib
    assert _exports(_normallosslib.LIB_PATH) == NAMES
    assert sorted(_normallosslib.SIGNATURES) == NAMES
    hdr = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(set(re.findall(r"\b(egs_[a-z0-9_]+)\s*\(", code))) == NAMES
    assert re.search(r"^#define\s+EGS_NORMALLOSS_ABI_VERSION\s+1\s*$", hdr, re.M)
    assert lib.egs_normalloss_abi_version() == 1 == _normallosslib.ABI_VERSION
    m = re.search(r"^#define\s+EGS_NORMALLOSS_MAX_PIXELS\s+\(1 << (\d+)\)\s*$", hdr, re.M)
    assert m and 1 << int(m.group(1)) == _normallosslib.MAX_PIXELS
    for name, value in (("TILE_W", _normallosslib.TILE_W), ("TILE_H", _normallosslib.TILE_H)):
        assert re.search(r"^#define\s+EGS_NORMALLOSS_%s\s+%d\s*$" % (name, value), hdr, re.M), name
    # the argument count of the call is the header's
    decl = re.search(r"int egs_normalloss\((.*?)\);", code, re.S).group(1)
    assert len(decl.split(",")) == len(_normallosslib.SIGNATURES["egs_normalloss"][1]) == 23
    assert "NOBODY HAS TUNED" in hdr


def test_the_other_libraries_are_untouched():
    from easygaussiansplatting_amd import _depthlosslib, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    assert _lib.ABI_VERSION == 12 and _lib.load().egs_abi_version() == 12
    assert not any("normalloss" in n for n in _lib.SIGNATURES)
    assert _depthlosslib.ABI_VERSION == 1 and not any("normal" in n for n in _depthlosslib.SIGNATURES)


def test_workspace_size(lib):
    for H, W in ((1, 1), (17, 65), (1080, 1920), (4000, 6000)):
        got = int(lib.egs_normalloss_ws_bytes(H, W))
        assert got % 256 == 0 and 32 * H * W + 2048 * 5 * 8 <= got <= 32 * H * W + 2048 * 5 * 8 + 2 * 256
    assert lib.egs_normalloss_ws_bytes(0, 5) == 256 and lib.egs_normalloss_ws_bytes(5, -1) == 256
    assert lib.egs_normalloss_ws_bytes(1 << 14, (1 << 12) + 1) == 256


def test_bad_arguments_and_a_short_workspace_are_refused_without_a_device(lib):
    P = _FAKE
    H, W = 17, 65
    need = int(lib.egs_normalloss_ws_bytes(H, W))

    def call(H=H, W=W, depth=P, alpha=2 * P, fx=80.0, fy=85.0, cx=30.0, cy=9.0, normals=3 * P, guide=4 * P,
             weight=5 * P, smooth=1, alpha_min=0.05, gamma=10.0, ps=1.0, ss=1.0, ws=6 * P, ws_bytes=need, out=7 * P,
             nout=8 * P, dd=9 * P, da=10 * P):
        return lib.egs_normalloss(H, W, depth, alpha, fx, fy, cx, cy, normals, guide, weight, smooth, alpha_min, gamma,
                                  ps, ss, ws, ws_bytes, out, nout, dd, da, None)

    def refused(rc):
        assert rc == BAD_ARG, rc
        msg = lib.egs_normalloss_last_error_string().decode()
        assert msg.startswith("egs_normalloss error 10001: bad argument"), msg

    for size in ("H", "W"):
        for bad in (0, -3):
            refused(call(**{size: bad}))
    refused(call(H=1 << 14, W=(1 << 12) + 1))           # beyond EGS_NORMALLOSS_MAX_PIXELS
    for name in ("depth", "alpha", "ws", "out"):
        refused(call(**{name: None}))
        refused(call(**{name: P + 2}))                  # not 4-B aligned
    refused(call(ws=6 * P + 8))                         # the workspace holds 16-B records
    for name in ("normals", "guide", "weight", "nout"):
        refused(call(**{name: P + 2}))
    for name in ("fx", "fy"):
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            refused(call(**{name: bad}))
    for name in ("cx", "cy", "ps", "ss"):
        for bad in (float("nan"), float("inf")):
            refused(call(**{name: bad}))
    for name in ("alpha_min", "gamma"):
        for bad in (-0.1, float("nan"), float("inf")):
            refused(call(**{name: bad}))
    for bad in (-1, 2):
        refused(call(smooth=bad))
    refused(call(dd=9 * P + 1))
    refused(call(dd=None))                              # one gradient plane without the other
    refused(call(da=None))
    refused(call(da=9 * P))                             # the two planes are one
    refused(call(nout=9 * P))
    for inp in (P, 2 * P, 3 * P, 4 * P, 5 * P):         # an output may not overwrite an input
        refused(call(dd=inp))
        refused(call(da=inp))
        refused(call(nout=inp))
    for short in (need - 1, 0):
        assert call(ws_bytes=short) == ERR_WORKSPACE
        msg = lib.egs_normalloss_last_error_string().decode()
        assert msg.startswith("egs_normalloss error 10002") and "workspace" in msg, msg
        assert call(ws_bytes=short, dd=None, da=None, weight=None, normals=None, guide=None, nout=None) == ERR_WORKSPACE


def test_source_reads_no_environment_variable_and_has_no_atomic():
    src = open(os.path.join(REPO, "easygaussiansplatting_amd", "csrc", "egs_normalloss.hip")).read()
    assert "getenv" not in src and re.findall(r"atomic\w*\(", src) == []
    assert "hipMalloc" not in src and "Synchronize" not in src
    assert len(re.findall(r"hipLaunchKernelGGL\(", src)) == 4      # tile, pairs, and one of the two gradient forms


# ---------------------------------------------------------------------------------------------------- the Python surface
def test_signatures():
    from easygaussiansplatting_amd import normalloss
    from easygaussiansplatting_amd.dataset import GSplatDataset
    from easygaussiansplatting_amd.trainer import Trainer
    assert list(inspect.signature(normalloss.normal_loss_with_grad).parameters) == [
        "depth", "alpha", "cam", "normals", "guide", "smooth", "weight", "alpha_min", "edge_gamma", "prior_scale",
        "smooth_scale", "need_grad"]
    d = {k: v.default for k, v in inspect.signature(normalloss.normal_loss_with_grad).parameters.items()}
    assert (d["normals"], d["guide"], d["smooth"], d["weight"], d["alpha_min"], d["edge_gamma"], d["prior_scale"],
            d["smooth_scale"], d["need_grad"]) == (None, None, True, None, 0.05, 10.0, 1.0, 1.0, True)
    assert list(inspect.signature(normalloss.normal_loss).parameters)[:3] == ["depth", "alpha", "cam"]
    assert list(inspect.signature(normalloss.depth_to_normals).parameters)[:3] == ["depth", "alpha", "cam"]
    p = inspect.signature(Trainer.__init__).parameters
    assert (p["normal_priors"].default, p["normal_smooth"].default, p["normal_alpha_min"].default,
            p["normal_edge_gamma"].default) == (None, 0.0, 0.05, 10.0)
    assert p["normal_weight"].default > 0
    assert "tuned" in normalloss.__doc__.lower() and "nobody has tuned" in Trainer.__init__.__doc__.lower()
    g = inspect.signature(GSplatDataset.__init__).parameters
    assert (g["normals"].default, g["normals_convention"].default) == (False, "opencv")


def test_normal_loss_refusals():
    from easygaussiansplatting_amd.normalloss import depth_to_normals, normal_loss, normal_loss_with_grad
    H, W = 6, 8
    d, a, q = torch.ones((1, H, W)), torch.ones((1, H, W)), torch.ones((3, H, W))
    cam = (10.0, 10.0, 4.0, 3.0)
    bad = [
        (dict(depth=torch.ones((3, H, W))), "depth must have shape"),
        (dict(depth=d.double()), "depth must be torch.float32"),
        (dict(alpha=torch.ones((1, H, W + 1))), "alpha must have shape"),
        (dict(normals=torch.ones((H, W, 3))), "normals must have shape"),
        (dict(normals=torch.ones((H, W))), "normals must have shape"),
        (dict(normals=q.double()), "normals must be torch.float32"),
        (dict(guide=torch.ones((1, H, W))), "guide must have shape"),
        (dict(guide=q.to(torch.uint8)), "guide must be torch.float32"),
        (dict(weight=torch.ones((H, W), dtype=torch.bool)), "weight must be torch.float32"),
        (dict(weight=torch.ones((1, H + 1, W))), "weight must have shape"),
        (dict(alpha_min=-1.0), "alpha_min must be finite"),
        (dict(edge_gamma=float("nan")), "edge_gamma must be finite"),
        (dict(prior_scale=float("inf")), "prior_scale and smooth_scale must be finite"),
        (dict(cam=(10.0, 0.0, 1.0, 1.0)), "cam must give finite intrinsics"),
        (dict(cam=(10.0, 10.0, 1.0)), "cam must give finite intrinsics"),
        (dict(cam="x"), "cam must give finite intrinsics"),
    ]
    for kw, msg in bad:
        args = dict(depth=d, alpha=a, cam=cam, normals=q)
        args.update(kw)
        for fn in (normal_loss, normal_loss_with_grad):
            with pytest.raises(ValueError, match=msg):
                fn(**args)
    with pytest.raises(TypeError, match="normals must be a torch.Tensor"):
        normal_loss_with_grad(d, a, cam, normals=np.ones((3, H, W), np.float32))
    # good arguments pass their own checks; the call is then refused for want of a GPU tensor
    for dd in (d, d[0]):
        with pytest.raises(ValueError, match="depth must live on the GPU"):
            normal_loss_with_grad(dd, a, cam, normals=q, guide=q, weight=d[0])
    with pytest.raises(ValueError, match="depth must live on the GPU"):
        depth_to_normals(d, a, cam)


def test_trainer_refusals_and_the_prior_checker():
    from easygaussiansplatting_amd.trainer import Trainer, _checked_normal_priors
    H, W = 6, 8
    gts = [torch.zeros((3, H, W)) for _ in range(3)]
    up = torch.zeros((3, H, W)); up[2] = -1.0
    make = lambda nq, **kw: Trainer(None, [], gts, 10, device="cpu", normal_priors=nq, **kw)
    with pytest.raises(ValueError, match="2 entries for 3 views"):
        make([up, up])
    with pytest.raises(ValueError, match=r"view 1 has shape \[6, 8\]"):
        make([up, up[0], None])
    with pytest.raises(ValueError, match="view 2 has shape"):
        make([None, None, torch.zeros((3, W, H))])
    with pytest.raises(ValueError, match="view 0 must be a float32 tensor"):
        make([up.double(), None, None])
    for fill in (0.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="view 1 has no pixel with data"):
            make([up, torch.full((3, H, W), fill), None])
    # the two refusals, in the wording of the depth priors'
    with pytest.raises(ValueError, match=r"Trainer\(normal_priors=\.\.\.\) with absgrad=True: a view with a normal term"):
        make([up, None, None], absgrad=True)
    with pytest.raises(ValueError, match=r"Trainer\(normal_priors=\.\.\.\) needs mode='fused'"):
        make([up, None, None], mode="ops", fused_activations=False)
    with pytest.raises(ValueError, match=r"Trainer\(normal_smooth=0.5\) with absgrad=True"):
        make(None, normal_smooth=0.5, absgrad=True)
    with pytest.raises(ValueError, match=r"Trainer\(normal_smooth=0.5\) needs mode='fused'"):
        make(None, normal_smooth=0.5, mode="ops", fused_activations=False)
    for name in ("normal_weight", "normal_smooth", "normal_alpha_min", "normal_edge_gamma"):
        for bad_value in (-0.5, float("nan"), float("inf")):
            with pytest.raises(ValueError, match=name):
                make([up, None, None], **{name: bad_value})
    # what passes: holes and NaNs stay as they are
    holes = up.clone(); holes[:, 1, 2] = 0.0; holes[0, 0, 0] = float("nan")
    got = _checked_normal_priors([holes, None, up], gts, "cpu")
    assert got[1] is None and torch.equal(got[2], up) and torch.equal(got[0].nan_to_num(7.0), holes.nan_to_num(7.0))
    assert _checked_normal_priors(None, gts, "cpu") is None
    # the constructor calls of the other host-side tests still end where they did
    with pytest.raises(ValueError, match="cap_max"):
        Trainer(None, [], [], 10, strategy="mcmc", normal_priors=[])


# ------------------------------------------------------------------------------------------------------------ the dataset
def test_dataset_collects_normal_priors(tmp_path):
    from PIL import Image
    from easygaussiansplatting_amd import scene as S
    from easygaussiansplatting_amd.dataset import GSplatDataset
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
    os.makedirs(os.path.join(root, "normals"))
    n0 = rng.normal(size=(Hh, Ww, 3)).astype(np.float32); n0[::2, 1::2] = 0.0             # [H,W,3] with holes
    n1 = rng.integers(0, 256, (Hh, Ww, 3), dtype=np.uint8)
    n2 = rng.normal(size=(3, Hh // 2, Ww // 2)).astype(np.float32)                         # [3,h,w] at half the size
    np.save(os.path.join(root, "normals", "view_00.npy"), n0)
    Image.fromarray(n1).save(os.path.join(root, "normals", "view_01.png"))
    np.save(os.path.join(root, "normals", "view_02.npy"), n2)
    plain = GSplatDataset(root, device="cpu")
    assert plain.normal_priors is None and len(plain) == 4
    ds = GSplatDataset(root, device="cpu", normals=True)
    assert len(ds.normal_priors) == 4 and ds.normal_priors[3] is None              # a view without a file
    for got in ds.normal_priors[:3]:
        assert got.dtype == torch.float32 and tuple(got.shape) == (3, Hh, Ww) and got.is_contiguous()
    assert np.array_equal(ds.normal_priors[0].numpy(), n0.transpose(2, 0, 1))
    assert np.array_equal(ds.normal_priors[1].numpy(),
                          (n1.astype(np.float32) / np.float32(127.5) - np.float32(1)).transpose(2, 0, 1))
    assert float(ds.normal_priors[1].min()) >= -1 and float(ds.normal_priors[1].max()) <= 1
    assert np.array_equal(ds.normal_priors[2].numpy(), np.repeat(np.repeat(n2, 2, 1), 2, 2))
    for a, b in zip(ds.images, plain.images):                                      # the images are what they were
        assert torch.equal(a, b)
    gl = GSplatDataset(root, device="cpu", normals=True, normals_convention="opengl")
    flip = np.array([1, -1, -1], np.float32)[:, None, None]
    for k in range(3):
        assert np.array_equal(gl.normal_priors[k].numpy(), ds.normal_priors[k].numpy() * flip)
    assert gl.normal_priors[3] is None
    # .npy wins over .png; resized with the image by nearest sampling: a hole stays a hole
    Image.fromarray(n1).save(os.path.join(root, "normals", "view_00.png"))
    half = GSplatDataset(root, resize_rate=0.5, device="cpu", normals=True)
    assert np.array_equal(half.normal_priors[0].numpy(), n0.transpose(2, 0, 1)[:, 1::2, 1::2])
    assert np.array_equal(half.normal_priors[2].numpy(), n2)
    with pytest.raises(ValueError, match="normals_convention"):
        GSplatDataset(root, device="cpu", normals=True, normals_convention="blender")
    np.save(os.path.join(root, "normals", "view_03.npy"), np.zeros((Hh, Ww), np.float32))
    with pytest.raises(ValueError, match="expected a"):
        GSplatDataset(root, device="cpu", normals=True)


def test_train_example_lists_the_flags():
    r = subprocess.run([sys.executable, os.path.join(REPO, "examples", "train.py"), "--help"], capture_output=True,
                       text=True, cwd=REPO)
    assert r.returncode == 0, r.stderr
    for flag in ("--normals", "--normal-weight W", "--normal-smooth S", "--normals-convention"):
        assert flag in r.stdout, flag
