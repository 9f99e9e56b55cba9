"""Per-pixel loss weights, host side (no GPU): the float64 reference of tests/weighted_loss_ref.py checked on itself
(w == 1 is the unweighted reference, central differences, the 11 x 11 support of one weighted pixel, the 5-pixel reach of
the ground truth), the C surface of libegs_wloss.so against include/egs_wloss.h and its refusals before any HIP call,
the refusals of ``gau_loss_with_grad(weight=...)`` and ``Trainer(pixel_weights=...)``, ``GSplatDataset(masks=True)``
and the flag of examples/train.py."""
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import loss_cases as LC
from tests import weighted_loss_ref as WR

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "egs_wloss.h")
BAD_ARG, ERR_WORKSPACE = 10001, 10002
_FAKE = 4096                    # a pointer nobody dereferences: every call below is refused before any HIP call
NAMES = ["egs_wloss", "egs_wloss_abi_version", "egs_wloss_last_error_string", "egs_wloss_ws_bytes"]


# -------------------------------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("kind", ["noise", "quantised", "hdr"])
def test_reference_with_unit_weights_is_the_unweighted_reference(kind):
    H, W = 23, 70
    x, y = LC.make_pair(kind, H, W)
    for lam in (0.2, 1.0):
        loss, grad, ssim, sw = WR.ref64(x, y, np.ones((H, W), np.float32), lam)
        loss0, grad0, ssim0 = LC.ref64(x, y, lam)
        assert sw == H * W
        assert loss == loss0 and ssim == ssim0
        assert torch.equal(grad, grad0)


def test_reference_gradient_against_central_differences():
    H, W = 12, 13
    x, y = LC.make_pair("noise", H, W)
    w = WR.make_weight("uniform", H, W)
    w[3:6, 2:9] = 0.0
    lam = 0.3
    _, grad, _, _ = WR.ref64(x, y, w, lam)
    x64 = x.astype(np.float64)
    eps = 1e-6
    worst = 0.0
    for idx in np.ndindex(3, H, W):
        xp, xm = x64.copy(), x64.copy()
        xp[idx] += eps; xm[idx] -= eps
        fd = (WR.ref64(xp, y, w, lam)[0] - WR.ref64(xm, y, w, lam)[0]) / (2 * eps)
        worst = max(worst, abs(fd - float(grad[idx])))
    # float(loss) carries 1e-16 of rounding: 1e-16 / 2e-6 = 5e-11 in the quotient; the third derivative's term is eps^2
    assert worst <= 1e-8, worst
    assert float(grad.abs().max()) > 1e-4


def test_one_weighted_pixel_reaches_its_window_and_no_further():
    H, W = 33, 129
    x, y = LC.make_pair("noise", H, W)
    w = WR.make_weight("pixel", H, W)
    assert w[16, 64] == 1.0 and w.sum() == 1.0
    _, grad, _, sw = WR.ref64(x, y, w, 0.2)
    assert sw == 1.0
    support = (grad != 0).any(0)
    want = torch.zeros((H, W), dtype=torch.bool)
    want[11:22, 59:70] = True
    assert torch.equal(support, want)


def test_ground_truth_reaches_five_columns_and_no_further():
    H, W = 20, 90
    x, y = LC.make_pair("noise", H, W)
    w = WR.make_weight("cols61", H, W)                  # the last weighted column is 60
    base = WR.ref64(x, y, w, 0.2)

    def changed_from(col):
        y2, x2 = y.copy(), x.copy()
        y2[:, :, col:] = 1.0 - y2[:, :, col:]
        x2[:, :, col:] = 0.5 * x2[:, :, col:]
        return WR.ref64(x2, y2, w, 0.2)

    far = changed_from(66)                              # 6 columns from column 60
    assert far[0] == base[0] and far[2] == base[2] and torch.equal(far[1], base[1])
    near = changed_from(65)                             # 5 columns: inside the window of column 60
    assert near[0] != base[0] and not torch.equal(near[1], base[1])


def test_zero_weight_sum_is_the_stated_convention():
    x, y = LC.make_pair("noise", 7, 9)
    loss, grad, ssim, sw = WR.ref64(x, y, np.zeros((7, 9), np.float32), 0.2)
    assert (loss, ssim, sw) == (0.0, 1.0, 0.0) and not bool(grad.any())


# -------------------------------------------------------------------------------------------------------- the C surface
@pytest.fixture(scope="module")
def lib():
    from easygaussiansplatting_amd import _lib, _wlosslib
    if not os.path.exists(_wlosslib.LIB_PATH):
        _lib.build()
    return _wlosslib.load()


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    return sorted(ln.split()[-1] for ln in out.splitlines() if ln.strip() and ln.split()[-1].startswith("egs_"))


def test_library_exports_what_its_header_declares(lib):
    from easygaussiansplatting_amd import _wlosslib
    assert _exports(_wlosslib.LIB_PATH) == NAMES
    assert sorted(_wlosslib.SIGNATURES) == NAMES
    hdr = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(set(re.findall(r"\b(egs_[a-z0-9_]+)\s*\(", code))) == NAMES
    assert re.search(r"^#define\s+EGS_WLOSS_ABI_VERSION\s+1\s*$", hdr, re.M)
    assert lib.egs_wloss_abi_version() == 1 == _wlosslib.ABI_VERSION
    m = re.search(r"^#define\s+EGS_WLOSS_MAX_PIXELS\s+\(1 << (\d+)\)\s*$", hdr, re.M)
    assert m and 1 << int(m.group(1)) == _wlosslib.MAX_PIXELS


def test_libegs_hip_is_untouched():
    from easygaussiansplatting_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    assert _lib.ABI_VERSION == 12 and _lib.load().egs_abi_version() == 12
    assert not any("wloss" in n for n in _lib.SIGNATURES)


def test_workspace_size(lib):
    for H, W in ((1, 1), (17, 65), (1080, 1920)):
        nb = ((W + 63) // 64) * ((H + 15) // 16) * 3
        got = int(lib.egs_wloss_ws_bytes(H, W))
        assert got % 256 == 0 and got >= 3 * 12 * H * W + 8 * nb + 4 * (nb // 3)
        assert got <= 3 * 12 * H * W + 8 * nb + 4 * (nb // 3) + 6 * 256
    assert lib.egs_wloss_ws_bytes(0, 5) == 256 and lib.egs_wloss_ws_bytes(5, -1) == 256


def test_bad_arguments_and_a_short_workspace_are_refused_without_a_device(lib):
    P = _FAKE
    H, W = 17, 65
    need = int(lib.egs_wloss_ws_bytes(H, W))

    def call(H=H, W=W, image=P, gt=2 * P, weight=3 * P, ws=4 * P, ws_bytes=need, out=5 * P, grad=6 * P):
        return lib.egs_wloss(H, W, image, gt, weight, 0.2, 1.0, ws, ws_bytes, out, grad, None)

    def refused(rc):
        assert rc == BAD_ARG, rc
        msg = lib.egs_wloss_last_error_string().decode()
        assert msg.startswith("egs_wloss error 10001: bad argument"), msg

    for size in ("H", "W"):
        for bad in (0, -3):
            refused(call(**{size: bad}))
    refused(call(H=1 << 15, W=(1 << 13) + 1))           # beyond EGS_WLOSS_MAX_PIXELS
    for name in ("image", "gt", "weight", "ws", "out"):
        refused(call(**{name: None}))
        refused(call(**{name: P + 2}))                  # not 4-B aligned
    refused(call(grad=P + 1))
    refused(call(grad=P))                               # the gradient may not overwrite the image
    for short in (need - 1, 0):
        assert call(ws_bytes=short) == ERR_WORKSPACE
        msg = lib.egs_wloss_last_error_string().decode()
        assert msg.startswith("egs_wloss error 10002") and "workspace" in msg, msg
        assert call(ws_bytes=short, grad=None) == ERR_WORKSPACE


def test_source_reads_no_environment_variable():
    for name in ("egs_wloss.hip", "egs_loss.hip", "egs_loss_device.h"):
        assert "getenv" not in open(os.path.join(REPO, "easygaussiansplatting_amd", "csrc", name)).read()


# ---------------------------------------------------------------------------------------------------- the Python surface
def test_loss_functions_take_a_weight():
    from easygaussiansplatting_amd import loss
    for fn in (loss.gau_loss_with_grad, loss.gau_loss):
        assert inspect.signature(fn).parameters["weight"].default is None
    assert list(inspect.signature(loss.gau_loss_with_grad).parameters) == [
        "image", "gt_image", "loss_lambda", "need_grad", "grad_scale", "weight"]


def test_weight_refusals():
    from easygaussiansplatting_amd.loss import gau_loss, gau_loss_with_grad
    H, W = 6, 8
    x, y = torch.zeros((3, H, W)), torch.zeros((3, H, W))
    bad = [
        (torch.ones((H, W + 1)), "weight must have shape"),
        (torch.ones((W, H)), "weight must have shape"),
        (torch.ones((3, H, W)), "weight must have shape"),
        (torch.ones((1, H, W)), "weight must have shape"),
        (torch.ones((H, W), dtype=torch.float64), "weight must be torch.float32, torch.bool or torch.uint8"),
        (torch.ones((H, W), dtype=torch.float16), "weight must be torch.float32, torch.bool or torch.uint8"),
        (torch.ones((H, W), dtype=torch.int64), "weight must be torch.float32, torch.bool or torch.uint8"),
    ]
    for w, msg in bad:
        for fn in (gau_loss, gau_loss_with_grad):
            with pytest.raises(ValueError, match=msg):
                fn(x, y, weight=w)
    with pytest.raises(TypeError, match="weight must be a torch.Tensor"):
        gau_loss_with_grad(x, y, weight=np.ones((H, W), np.float32))
    # a good weight passes its own check; the images are then refused as ever (no GPU tensor here)
    for w in (torch.ones((H, W)), torch.ones((H, W), dtype=torch.bool), torch.ones((H, W), dtype=torch.uint8)):
        with pytest.raises(ValueError, match="image must live on the GPU"):
            gau_loss_with_grad(x, y, weight=w)


def test_weight_conversion():
    from easygaussiansplatting_amd.loss import _weight
    image = torch.zeros((3, 2, 3))
    f = torch.tensor([[0.0, 0.5, 2.0], [1.0, 0.0, 3.0]])
    assert _weight(f, image) is f
    for t in (torch.tensor([[0, 7, 255], [1, 0, 2]], dtype=torch.uint8), f != 0):
        got = _weight(t, image)
        assert got.dtype == torch.float32 and got.tolist() == [[0.0, 1.0, 1.0], [1.0, 0.0, 1.0]]
    assert _weight(f.t().contiguous().t(), image).is_contiguous()


def test_trainer_refusals():
    from easygaussiansplatting_amd.trainer import Trainer
    params = inspect.signature(Trainer.__init__).parameters
    assert params["pixel_weights"].default is None
    H, W = 6, 8
    gts = [torch.zeros((3, H, W)) for _ in range(3)]
    ones = torch.ones((H, W))
    make = lambda pw: Trainer(None, [], gts, 10, device="cpu", pixel_weights=pw)
    with pytest.raises(ValueError, match="2 entries for 3 views"):
        make([ones, ones])
    with pytest.raises(ValueError, match=r"view 1 has shape \[8, 6\]"):
        make([ones, ones.t(), None])
    with pytest.raises(ValueError, match="view 2 has shape"):
        make([None, None, torch.ones((3, H, W))])
    with pytest.raises(ValueError, match="view 0 must be a float32, bool or uint8 tensor"):
        make([ones.double(), None, None])
    with pytest.raises(ValueError, match="view 0 must be a float32, bool or uint8 tensor"):
        make([np.ones((H, W), np.float32), None, None])
    neg = ones.clone(); neg[2, 3] = -1e-3
    with pytest.raises(ValueError, match="view 2 holds a negative weight"):
        make([ones, None, neg])
    for bad in (float("nan"), float("inf")):
        nf = ones.clone(); nf[0, 0] = bad
        with pytest.raises(ValueError, match="view 1 holds a non-finite weight"):
            make([ones, nf, None])
    with pytest.raises(ValueError, match="view 1 is all zero"):
        make([ones, torch.zeros((H, W)), None])
    with pytest.raises(ValueError, match="view 0 is all zero"):
        make([torch.zeros((H, W), dtype=torch.bool), None, None])
    # the constructor calls of the other host-side tests still end where they did
    with pytest.raises(ValueError, match="cap_max"):
        Trainer(None, [], [], 10, strategy="mcmc")
    with pytest.raises(ValueError, match="cap_max"):
        Trainer(None, [], [], 10, strategy="mcmc", pixel_weights=[])


def test_checked_weights_are_float32_planes():
    from easygaussiansplatting_amd.trainer import _checked_pixel_weights
    H, W = 4, 5
    gts = [torch.zeros((3, H, W)) for _ in range(3)]
    m = torch.zeros((H, W), dtype=torch.uint8); m[1, 2] = 255
    f = torch.rand((H, W)) + 0.1
    got = _checked_pixel_weights([m, None, f], gts, "cpu")
    assert got[1] is None and got[0].dtype == torch.float32 and float(got[0].sum()) == 1.0 and got[0][1, 2] == 1.0
    assert torch.equal(got[2], f)
    assert _checked_pixel_weights(None, gts, "cpu") is None


# ------------------------------------------------------------------------------------------------------------ the dataset
def test_dataset_collects_masks(tmp_path):
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
    os.makedirs(os.path.join(root, "masks"))
    m0 =rng.integers(0, 256, (Hh, Ww), dtype=np.uint8); m0[:, :5] = 0
    m1 = np.zeros((Hh, Ww), np.uint8); m1[4:12, 6:18] = 255
    Image.fromarray(m0).save(os.path.join(root, "masks", "view_00.png.png"))      # COLMAP: <image file name>.png
    Image.fromarray(m1).save(os.path.join(root, "masks", "view_01.png"))          # by stem
    a2 = rng.integers(0, 256, (Hh, Ww), dtype=np.uint8)
    Image.fromarray(np.dstack([imgs[2], a2])).save(os.path.join(root, "images", "view_02.png"))     # RGBA
    plain = GSplatDataset(root, device="cpu")
    assert plain.weights is None and len(plain) == 4
    ds = GSplatDataset(root, device="cpu", masks=True)
    assert len(ds.weights) == 4 and ds.weights[3] is None
    for got, want in zip(ds.weights[:3], (m0, m1, a2)):
        assert got.dtype == torch.float32 and tuple(got.shape) == (Hh, Ww) and got.is_contiguous()
        assert torch.equal(got, torch.from_numpy(want).to(torch.float32) / 255.0)
    for a, b in zip(ds.images, plain.images):                                     # the images are what they were
        assert torch.equal(a, b) and tuple(a.shape) == (3, Hh, Ww)
    # a name match wins over the stem, both over the alpha channel
    Image.fromarray(m1).save(os.path.join(root, "masks", "view_00.png"))
    Image.fromarray(m1).save(os.path.join(root, "masks", "view_02.png"))
    again = GSplatDataset(root, device="cpu", masks=True)
    assert torch.equal(again.weights[0], ds.weights[0])
    assert torch.equal(again.weights[2], ds.weights[1])
    os.remove(os.path.join(root, "masks", "view_00.png"))
    os.remove(os.path.join(root, "masks", "view_02.png"))
    # resized with the image
    half = GSplatDataset(root, resize_rate=0.5, device="cpu", masks=True)
    assert half.weights[3] is None
    for k in range(3):
        assert tuple(half.weights[k].shape) == (Hh // 2, Ww // 2) == tuple(half.images[k].shape[1:])
        assert 0.0 <= float(half.weights[k].min()) and float(half.weights[k].max()) <= 1.0
    want = np.asarray(Image.fromarray(m1).resize((Ww // 2, Hh // 2)), np.float32) / np.float32(255.0)
    assert np.array_equal(half.weights[1].numpy(), want)
    assert float(half.weights[1][4, 6]) == 1.0 and float(half.weights[1][0, 0]) == 0.0


def test_train_example_lists_the_flag():
    r = subprocess.run([sys.executable, os.path.join(REPO, "examples", "train.py"), "--help"], capture_output=True,
                       text=True, cwd=REPO)
    assert r.returncode == 0, r.stderr
    assert "--masks" in r.stdout
