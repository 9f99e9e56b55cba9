"""The fused loss kernels (k_ssim_fwd, k_ssim_bwd, k_loss_finalize of csrc/egs_loss.hip: the unweighted instances of
the kernel bodies of csrc/egs_loss_device.h) against float64, where float32 SSIM is hard and where the tile walk changes.

Precision by regime: every pair kind of tests/loss_cases.py (noise is the only one the suite used to feed this kernel)
at 70x150 and 1080x1920, under the rule stated there: the kernel may be as far from float64 as twice what the
reference's own float32 formulation is on the same pair, and never needs to be closer than the suite's old bounds.

Every tile walk: the C ABI called directly on buffers the test owns (NaN-filled, with guard bands), at shapes chosen
for the number of tiles nb = ceil(W/64) ceil(H/16) 3 and the grid G = min(nb, 3 CUs): strided (G < 16), one band per
XCD (G == nb), persistent workgroups (nb > 3 CUs); one-pixel and sub-window images, every tile-edge remainder, UHD.

No buffer is ever smaller than the ABI asks for: the too-small workspace is an error code returned before any launch.
"""
import json
import os

import numpy as np
import pytest

from tests import loss_cases as LC

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.loss_abi import EGS_ERR_WORKSPACE, abi_loss, bits, dev, nb_of  # noqa: E402  (the guarded C-ABI call; needs torch)


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from easygaussiansplatting_amd import _lib
    return _lib.load()


def record(name, **figures):
    """Measurement only (the mechanism of test_gpu_parity.record_grad_error): one JSON line per case in the file
    EGS_GRAD_STATS names, nothing otherwise."""
    path = os.environ.get("EGS_GRAD_STATS")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(dict(name=str(name), measurement_only=True, **figures)) + "\n")


def hip_loss(x, y, lam, **kw):
    """-> ((loss, grad, ssim), stats) through the Python wrapper."""
    from easygaussiansplatting_amd.loss import gau_loss_with_grad
    stats, grad = gau_loss_with_grad(x, y, lam, **kw)
    torch.cuda.synchronize()
    return (float(stats[0]), grad, float(stats[2])), stats


# --------------------------------------------------------------------------- precision by regime
@pytest.mark.parametrize("size", [(70, 150), (1080, 1920)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("kind", LC.KINDS)
def test_precision_by_regime(lib, kind, size):
    H, W = size
    M = 3 * H * W
    xn, yn = LC.cached_pair(kind, H, W)
    x, y = dev(xn), dev(yn)
    for lam in (0.2, 1.0):
        want = LC.ref64(x, y, lam, "cuda")
        e_ref = LC.errors(LC.ref32(x, y, lam, "cuda"), want)
        got, stats = hip_loss(x, y, lam)
        e_hip = LC.errors(got, want)
        what = "%s %dx%d lambda %.1f" % (kind, H, W, lam)
        print("%s: e_ref %.2e e_hip %.2e | loss: ref %.2e hip %.2e | ssim: ref %.2e hip %.2e | max|grad64| M = %.3g" % (
            what, e_ref["e_grad"], e_hip["e_grad"], e_ref["d_loss"], e_hip["d_loss"], e_ref["d_ssim"], e_hip["d_ssim"],
            float(want[1].abs().max()) * M))
        record("gau_loss_by_regime:" + what, kind=kind, height=H, width=W, loss_lambda=lam,
               e_ref=e_ref["e_grad"], e_hip=e_hip["e_grad"], loss_err_ref=e_ref["d_loss"], loss_err_hip=e_hip["d_loss"],
               ssim_err_ref=e_ref["d_ssim"], ssim_err_hip=e_hip["d_ssim"])
        assert bool(torch.isfinite(got[1]).all()), what
        LC.check_against(e_hip, e_ref, what)
        if kind == "identical":
            assert float(stats[1]) == 0.0 and abs(float(stats[2]) - 1.0) <= 1e-5, (what, stats.tolist())
    if kind == "quantised":      # the L1 part alone: exact, sign(0) = 0 on the half of the pixels where x == y
        got, stats = hip_loss(x, y, 0.0)
        unit = np.float32(1.0 / M)
        want = torch.sign(x - y) * float(unit)
        assert float((want == 0).float().mean()) > 0.4
        assert torch.equal(bits(got[1] + 0.0), bits(want + 0.0)), "L1 gradient is not sign(x - y) / M"   # (+ 0.0: -0 is 0)
        assert set(torch.unique(got[1]).tolist()) == {-float(unit), 0.0, float(unit)}
        assert float(stats[0]) == float(stats[1])


# --------------------------------------------------------------------------- every tile walk, every edge (C ABI)
def check_shape(lib, H, W, tag=""):
    what = "%s%dx%d (nb %d)" % (tag, H, W, nb_of(H, W))
    xn, yn = LC.make_pair("noise", H, W)
    x, y = dev(xn), dev(yn)
    rc, grad, stats = abi_loss(lib, x, y)
    assert rc == 0, what
    n_bad = int((~torch.isfinite(grad)).sum())
    assert n_bad == 0 and bool(torch.isfinite(stats).all()), "%s: %d gradient entries never written" % (what, n_bad)
    want = LC.ref64(x, y, 0.2, "cuda")
    e_ref = LC.errors(LC.ref32(x, y, 0.2, "cuda"), want)
    e_hip = LC.errors((float(stats[0]), grad, float(stats[2])), want)
    print("%s: e_ref %.2e e_hip %.2e loss %.2e ssim %.2e" % (what, e_ref["e_grad"], e_hip["e_grad"], e_hip["d_loss"],
                                                             e_hip["d_ssim"]))
    LC.check_against(e_hip, e_ref, what)
    rc2, grad2, stats2 = abi_loss(lib, x, y)      # fresh NaN-filled buffers: the same bits
    assert rc2 == 0 and torch.equal(bits(grad), bits(grad2)) and torch.equal(bits(stats), bits(stats2)), what


@pytest.mark.parametrize("shape", [(1, 1), (1, 300), (300, 1), (5, 200), (10, 10), (11, 11)], ids=lambda s: "%dx%d" % s)
def test_one_pixel_and_sub_window(lib, shape):
    check_shape(lib, *shape)


@pytest.mark.parametrize("W", [63, 64, 65, 128, 129])
@pytest.mark.parametrize("H", [15, 16, 17, 32, 33])
def test_tile_edges(lib, H, W):
    check_shape(lib, H, W)


def shape_of_grid(gx, gy):
    """A gx x gy tile grid whose last tile row and column are partial."""
    return 16 * gy - 3, 64 * gx - 7


def grid_of(k):
    """k tiles per channel as gx x gy, as square as k's divisors allow."""
    gy = max(d for d in range(1, int(k ** 0.5) + 1) if k % d == 0)
    return k // gy, gy


@pytest.mark.parametrize("nb", [15, 18, 21, 27, 48, 324])
def test_strided_and_band_walks(lib, nb):
    """G == nb: strided up to its end (nb 15: G < 16), then one contiguous band per XCD, also where 8 does not divide nb."""
    H, W = shape_of_grid(*grid_of(nb // 3))
    assert nb_of(H, W) == nb
    check_shape(lib, H, W)


def test_around_the_persistent_switch(lib):
    """nb the largest value <= R = 3 CUs (the last grid with one tile per workgroup), the smallest above it (the first
    workgroup that takes two), and about 2.5 R with nb % 8 in {1, 7} (bands and shares of unequal length)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    R = 3 * cus
    ks = [R // 3, R // 3 + 1]
    for rem in (1, 7):
        cand = [k for k in range(5 * cus // 2, 5 * cus // 2 + 64) if (3 * k) % 8 == rem]
        ks.append(max(cand, key=lambda k: (min(grid_of(k)[1], 8), -k)))       # a two-dimensional grid where one exists
    assert 3 * ks[0] <= R < 3 * ks[1] and [(3 * k) % 8 for k in ks[2:]] == [1, 7]
    for k in ks:
        H, W = shape_of_grid(*grid_of(k))
        assert nb_of(H, W) == 3 * k
        check_shape(lib, H, W, "R = %d: " % R)


def test_uhd(lib):
    """2160x3840: plane offsets beyond 2^24 elements, nb 24 300."""
    check_shape(lib, 2160, 3840)


def test_short_workspace_is_an_error_code_before_any_launch(lib):
    x, y = map(dev, LC.make_pair("noise", 40, 70))
    rc, grad, stats = abi_loss(lib, x, y, ws_short=1)
    assert rc == EGS_ERR_WORKSPACE
    assert bool(torch.isnan(grad).all()) and bool(torch.isnan(stats).all())      # nothing ran
    assert b"workspace" in lib.egs_last_error_string()


# --------------------------------------------------------------------------- the Python wrapper
MID = (200, 700)      # nb 429 > 256: k_loss_finalize and the gradient kernel's reduction loop over the partials


@pytest.fixture(scope="module")
def mid(lib):
    x, y = map(dev, LC.make_pair("noise", *MID))
    return x, y


def test_stats_do_not_depend_on_need_grad(lib, mid):
    assert nb_of(*MID) > 256
    x, y = mid
    (_, g, _), with_grad = hip_loss(x, y, 0.2)
    (_, none, _), without = hip_loss(x, y, 0.2, need_grad=False)
    assert none is None and g is not None
    assert torch.equal(bits(with_grad), bits(without))


def test_grad_scale(lib, mid):
    x, y = mid
    (_, g1, _), s1 = hip_loss(x, y, 0.2)
    for scale in (0.125, 4.0):
        (_, g, _), s = hip_loss(x, y, 0.2, grad_scale=scale)
        assert torch.equal(bits(g), bits(g1 * scale)) and torch.equal(bits(s), bits(s1)), scale
    third = float(np.float32(1.0 / 3.0))
    (_, g, _), s = hip_loss(x, y, 0.2, grad_scale=third)
    assert torch.equal(bits(s), bits(s1))
    want = g1.double() * third
    ulp = torch.from_numpy(np.spacing(np.abs(want.cpu().numpy()).astype(np.float32)).astype(np.float64)).cuda()
    off = ((g.double() - want).abs() / ulp).max()
    print("grad_scale 1/3: max %.2f float32 ulps of the entry" % float(off))
    assert float(off) <= 2.0


def test_lambda_ends(lib, mid):
    x, y = mid
    M = x.numel()
    (_, g, _), s = hip_loss(x, y, 0.0)
    assert torch.equal(bits(g + 0.0), bits(torch.sign(x - y) * float(np.float32(1.0 / M)) + 0.0))
    assert float(s[0]) == float(s[1])
    (l1, g, ssim), s = hip_loss(x, y, 1.0)
    assert abs(float(s[0]) - (1.0 - float(s[2]))) <= 2.0 ** -23
    want = LC.ref64(x, y, 1.0, "cuda")
    LC.check_against(LC.errors((l1, g, ssim), want), LC.errors(LC.ref32(x, y, 1.0, "cuda"), want), "lambda 1")


def test_backward_on_another_stream(lib, mid):
    from easygaussiansplatting_amd.loss import gau_loss
    x, y = mid

    def run():
        xr = x.clone().requires_grad_(True)
        loss = gau_loss(xr, y)
        (2.5 * loss).backward()
        return loss.detach().clone(), xr.grad

    l0, g0 = run()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        l1, g1 = run()
    side.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(bits(l0.reshape(1)), bits(l1.reshape(1))) and torch.equal(bits(g0), bits(g1))
    (_, g, _), _ = hip_loss(x, y, 0.2)
    assert torch.equal(bits(g0), bits(g * 2.5))


def test_strided_view_is_made_contiguous(lib, mid):
    x, y = mid
    H, W = MID
    big = torch.zeros((3, H + 3, W + 5), device="cuda")
    big[:, :H, :W] = x
    view = big[:, :H, :W]
    assert not view.is_contiguous()
    (_, g, _), s = hip_loss(view, y, 0.2)
    (_, g0, _), s0 = hip_loss(x, y, 0.2)
    assert torch.equal(bits(g), bits(g0)) and torch.equal(bits(s), bits(s0))


def test_rejected_inputs_never_reach_the_kernel(lib, mid, monkeypatch):
    from easygaussiansplatting_amd.loss import gau_loss, gau_loss_with_grad
    x, y = mid
    H, W = MID
    calls = []
    real = lib.egs_gau_loss
    monkeypatch.setattr(lib, "egs_gau_loss", lambda *a: calls.append(a) or real(*a))
    bad = [
        (x.double(), y, "image must be torch.float32"),
        (x, y.double(), "gt_image must be torch.float32"),
        (x.permute(1, 2, 0), y, r"image must have shape \[3, None, None\]"),
        (x, y[:, :, :W - 1], r"gt_image must have shape \[3, %d, %d\]" % (H, W)),
        (x, y[:, :H - 1], r"gt_image must have shape \[3, %d, %d\]" % (H, W)),
        (x[0], y, r"image must have shape \[3, None, None\]"),
        (x.cpu(), y, "image must live on the GPU"),
        (x, y.cpu(), "gt_image must live on the GPU"),
    ]
    for a, b, msg in bad:
        for fn in (gau_loss, gau_loss_with_grad):
            with pytest.raises(ValueError, match=msg):
                fn(a, b)
    with pytest.raises(TypeError, match="image must be a torch.Tensor"):
        gau_loss_with_grad(x.cpu().numpy(), y)
    assert calls == []
    gau_loss_with_grad(x, y)                 # the spy does see a call that passes
    torch.cuda.synchronize()
    assert len(calls) == 1
