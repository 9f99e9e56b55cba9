"""The weighted fused loss (csrc/egs_wloss.hip: k_ssim_fwd_w, k_ssim_bwd_w, k_loss_finalize_w) against the
float64 form of its definition (tests/weighted_loss_ref.py), on every tile walk and on weight patterns that put the edge
of the weighted region inside a tile, on a tile corner and on every other pixel.

The C ABI is called directly on buffers the test owns, as tests/test_gpu_loss.py does: workspace, gradient and
``loss_out`` NaN-filled between guard bands that must be intact afterwards.  No buffer is ever smaller than the ABI asks
for: the too-small workspace is an error code returned before any launch.

Shapes, by nb = ceil(W/64) ceil(H/16) 3: 1x1, 5x200, 11x11 (below the window), 17x65 (nb 12: the strided walk, every
tile-edge remainder), 33x129 (nb 27: one band per XCD), 272x1024 (nb 816 > 3 x 256 CUs: persistent workgroups).

w == 1 against egs_gau_loss (the guarded call of tests/loss_abi.py): bit-identical stats[0:3] and gradient, stats[3] ==
H W.  Both libraries instantiate the kernel bodies of csrc/egs_loss_device.h, so this pins that everything WEIGHTED adds is
a multiplication by 1.0: the per-tile sum(w) <= 1024 is exact in float32 and the sum of the tile sums is exact in double.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import loss_cases as LC
from tests import weighted_loss_ref as WR

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.loss_abi import EGS_ERR_WORKSPACE, abi_loss, bits, dev, guarded, guards_intact, nb_of  # noqa: E402  (needs torch)

SHAPES = [(1, 1), (5, 200), (11, 11), (17, 65), (33, 129), (272, 1024)]
sid = lambda s: "%dx%d" % s


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from easygaussiansplatting_amd import _wlosslib
    return _wlosslib.load()


@pytest.fixture(scope="module")
def hiplib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from easygaussiansplatting_amd import _lib
    return _lib.load()


def abi_wloss(lib, x, y, w, lam=0.2, scale=1.0, ws_short=0, need_grad=True, stream=None):
    """egs_wloss on buffers this test owns: workspace, gradient and stats NaN-filled between guard bands.
    -> (rc, grad [3,H,W] or None, stats [4]); asserts the guards."""
    H, W = int(x.shape[1]), int(x.shape[2])
    assert tuple(w.shape) == (H, W) and w.dtype == torch.float32 and w.is_contiguous()
    ws_bytes = int(lib.egs_wloss_ws_bytes(H, W))
    assert ws_bytes % 4 == 0 and ws_bytes >= 3 * 12 * H * W + 8 * nb_of(H, W) + 4 * (nb_of(H, W) // 3)
    ws_all, ws = guarded(ws_bytes)
    g_all, g = guarded(12 * H * W)
    s_all, s = guarded(16)
    for inner in (ws, g, s):
        inner.view(torch.float32).fill_(float("nan"))
    p = lambda t: C.c_void_p(t.data_ptr())
    st = stream if stream is not None else torch.cuda.current_stream()
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())      # the fills above
    rc = lib.egs_wloss(H, W, p(x), p(y), p(w), float(lam), float(scale), p(ws), ws_bytes - ws_short, p(s),
                       p(g) if need_grad else None, C.c_void_p(st.cuda_stream))
    st.synchronize()
    torch.cuda.synchronize()
    for whole, nm in ((ws_all, "workspace"), (g_all, "dloss_dimage"), (s_all, "loss_out")):
        assert guards_intact(whole), "%dx%d: the kernels wrote outside %s" % (H, W, nm)
    grad = g.view(torch.float32).reshape(3, H, W).clone()
    if not need_grad:
        assert bool(torch.isnan(grad).all()), "a gradient was written though none was asked for"
        grad = None
    return rc, grad, s.view(torch.float32).clone()


@functools.lru_cache(maxsize=4)
def pair(kind, H, W):
    xn, yn = LC.make_pair(kind, H, W)
    return dev(xn), dev(yn)


def check_case(lib, x, y, w, lams, what):
    """the kernel against float64 under the rule, every gradient entry and stat written, the same bits twice"""
    for lam in lams:
        rc, grad, stats = abi_wloss(lib, x, y, w, lam)
        tag = "%s lambda %.1f" % (what, lam)
        assert rc == 0, tag
        n_bad = int((~torch.isfinite(grad)).sum())
        assert n_bad == 0 and bool(torch.isfinite(stats).all()), "%s: %d gradient entries never written" % (tag, n_bad)
        want = WR.ref64(x, y, w, lam, "cuda")
        e_ref = WR.errors(WR.ref32(x, y, w, lam, "cuda"), want)
        e_hip = WR.errors((float(stats[0]), grad, float(stats[2])), want)
        print("%s: sum w %.6g | e_ref %.2e e_hip %.2e | loss: ref %.2e hip %.2e | ssim: ref %.2e hip %.2e" % (
            tag, want[3], e_ref["e_grad"], e_hip["e_grad"], e_ref["d_loss"], e_hip["d_loss"], e_ref["d_ssim"],
            e_hip["d_ssim"]))
        WR.check_against(e_hip, e_ref, tag)
        # sum w: the tile sums are float32 sums of at most 1024 weights, their total a double
        assert abs(float(stats[3]) - want[3]) <= 1024 * 2.0 ** -24 * max(want[3], 1.0), (tag, float(stats[3]), want[3])
        rc2, grad2, stats2 = abi_wloss(lib, x, y, w, lam)      # fresh NaN-filled buffers: the same bits
        assert rc2 == 0 and torch.equal(bits(grad), bits(grad2)) and torch.equal(bits(stats), bits(stats2)), tag
    return grad, stats


# --------------------------------------------------------------------------- shape x pattern against float64
@pytest.mark.parametrize("pattern", WR.PATTERNS)
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_shape_by_pattern(lib, shape, pattern):
    H, W = shape
    x, y = pair("noise", H, W)
    w = dev(WR.make_weight(pattern, H, W))
    check_case(lib, x, y, w, (0.2, 1.0), "noise %dx%d (nb %d) %s" % (H, W, nb_of(H, W), pattern))


@pytest.mark.parametrize("kind", LC.KINDS)
def test_pair_kinds(lib, kind):
    """the regimes of tests/loss_cases.py (float32 SSIM is hardest on the smooth ones) under random weights"""
    H, W = 33, 129
    x, y = pair(kind, H, W)
    check_case(lib, x, y, dev(WR.make_weight("uniform", H, W)), (0.2, 1.0), "%s %dx%d uniform" % (kind, H, W))


@pytest.mark.parametrize("shape", [(17, 65), (33, 129), (272, 1024)], ids=sid)
def test_l1_gradient_alone_is_exact(lib, shape):
    """lambda 0 on the quantised pair: the gradient is exactly +-w unit or 0, unit = float32(1 / (3 sum w)).  Weights in
    eighths, so that sum w is exact in every summation order."""
    H, W = shape
    kind = "quantised" if H * W < 100000 else "noise"
    x, y = pair(kind, H, W)
    wn = np.floor(8.0 * WR.make_weight("uniform", H, W)) / 8.0
    wn[:, 40:50] = 0.0
    w = dev(wn)
    rc, grad, stats = abi_wloss(lib, x, y, w, 0.0)
    assert rc == 0
    sum_w = float(wn.astype(np.float64).sum())
    assert float(stats[3]) == float(np.float32(sum_w))
    unit = np.float32(1.0 / (3.0 * sum_w))
    want = torch.sign(x - y) * (w * float(unit))[None]
    if kind == "quantised":
        assert float((torch.sign(x - y) == 0).float().mean()) > 0.4
    assert torch.equal(bits(grad + 0.0), bits(want + 0.0)), "L1 gradient is not w sign(x - y) / (3 sum w)"   # (+ 0.0: -0 is 0)
    assert float(stats[0]) == float(stats[1])
    l1 = float((w[None].double() * (x - y).abs().double()).sum()) / (3.0 * sum_w)
    assert abs(float(stats[1]) - l1) <= LC.LOSS_FLOOR


# --------------------------------------------------------------------------- w == 1 is egs_gau_loss
@pytest.mark.parametrize("kind", ["noise", "quantised"])
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_unit_weights_give_the_bits_of_the_unweighted_kernels(lib, hiplib, shape, kind):
    H, W = shape
    if kind == "quantised" and H * W > 100000:
        kind = "rendered"
    x, y = pair(kind, H, W)
    ones = torch.ones((H, W), device="cuda")
    for lam, scale in ((0.2, 1.0), (1.0, 1.0 / 3.0), (0.0, 0.25)):
        rc, grad, stats = abi_wloss(lib, x, y, ones, lam, scale)
        assert rc == 0
        rc0, grad0, stats0 = abi_loss(hiplib, x, y, lam, scale)      # (guard bands of the unweighted call included)
        assert rc0 == 0
        what = "%s %dx%d lambda %.1f scale %.3f" % (kind, H, W, lam, scale)
        assert float(stats[3]) == H * W, what
        assert torch.equal(bits(stats[:3]), bits(stats0)), (what, stats.tolist(), stats0.tolist())
        n_diff = int((bits(grad) != bits(grad0)).sum())
        assert n_diff == 0, "%s: %d gradient entries differ, by at most %.3e" % (
            what, n_diff, float((grad - grad0).abs().max()))


# --------------------------------------------------------------------------- what lies outside the weighted region
def test_one_weighted_pixel_at_a_tile_corner(lib):
    H, W = 33, 129
    x, y = pair("noise", H, W)
    wn = WR.make_weight("pixel", H, W)
    assert wn[16, 64] == 1.0 and wn.sum() == 1.0
    grad, stats = check_case(lib, x, y, dev(wn), (0.2,), "one pixel")          # (the rule inside the window)
    assert float(stats[3]) == 1.0
    inside = torch.zeros((H, W), dtype=torch.bool, device="cuda")
    inside[11:22, 59:70] = True
    assert bool((grad[:, ~inside] == 0).all()), "gradient outside the 11 x 11 window of the weighted pixel"
    assert bool((grad[:, inside] != 0).all())


def test_content_beyond_five_pixels_changes_nothing(lib):
    """columns below 61 weighted: image and ground truth changed from column 67 on leave every bit as it was; changed
    from column 65 on (inside the window of column 60) they do not"""
    H, W = 33, 129
    x, y = pair("noise", H, W)
    w = dev(WR.make_weight("cols61", H, W))
    _, grad, stats = abi_wloss(lib, x, y, w)

    def changed_from(col):
        x2, y2 = x.clone(), y.clone()
        y2[:, :, col:] = 1.0 - y2[:, :, col:]
        x2[:, :, col:] = -0.5 * x2[:, :, col:]
        rc, g, s = abi_wloss(lib, x2, y2, w)
        assert rc == 0
        return g, s

    g67, s67 = changed_from(67)
    assert torch.equal(bits(s67), bits(stats)) and torch.equal(bits(g67), bits(grad))
    g65, s65 = changed_from(65)
    assert not torch.equal(bits(s65), bits(stats)) and not torch.equal(bits(g65), bits(grad))
    assert bool((g65[:, :, :55] == grad[:, :, :55]).all())          # (and only within reach of column 65)


@pytest.mark.parametrize("shape", [(1, 1), (33, 129), (272, 1024)], ids=sid)
def test_zero_weight_sum(lib, shape):
    H, W = shape
    x, y = pair("noise", H, W)
    zeros = torch.zeros((H, W), device="cuda")
    for need_grad in (True, False):
        rc, grad, stats = abi_wloss(lib, x, y, zeros, need_grad=need_grad)
        assert rc == 0 and stats.tolist() == [0.0, 0.0, 1.0, 0.0]
        if need_grad:
            assert bool((grad == 0).all())


# --------------------------------------------------------------------------- the calling conventions
MID = (200, 700)      # nb 429 > 256, 143 tile sums of w: the reductions loop over the partials


@pytest.fixture(scope="module")
def mid(lib):
    x, y = map(dev, LC.make_pair("noise", *MID))
    return x, y, dev(WR.make_weight("uniform", *MID))


def test_stats_do_not_depend_on_need_grad(lib, mid):
    x, y, w = mid
    for lam in (0.2, 1.0):
        _, g, with_grad = abi_wloss(lib, x, y, w, lam)
        _, none, without = abi_wloss(lib, x, y, w, lam, need_grad=False)
        assert none is None and g is not None
        assert torch.equal(bits(with_grad), bits(without)), lam


def test_grad_scale(lib, mid):
    """the rule of tests/test_gpu_loss.py::test_grad_scale: powers of two scale the bits, 1/3 stays within 2 ulps of the
    entry.  An entry is a + b = c_l1 w sign + c_ssim dS, and grad_scale reaches it through the two coefficients, each
    rounded on its own, so the entry's ulp is a unit for that error only where a and b do not cancel: with weights down
    to 0, a shrinks until it meets an opposing b -- (|a| + |b|) / |a + b| reaches 3000 on this pair in float64, against
    1.8 with w == 1 -- and the same roundings were 1900 ulps of what is left.  The 1/3 case therefore takes the two
    inputs for which the bound has a reason: w == 1, the case the rule was written on (and the bits of the kernel it was
    written for), and lambda 0 under random weights, where the entry is the single product c_l1 (w sign): half an ulp for
    its rounding, at most 2/3 for that of the unscaled entry (three times as large) and at most one for the
    coefficient's two roundings, of which this plane's sum w leaves 0.1."""
    x, y, w = mid
    _, g1, s1 = abi_wloss(lib, x, y, w)
    for scale in (0.125, 4.0):
        _, g, s = abi_wloss(lib, x, y, w, scale=scale)
        assert torch.equal(bits(g), bits(g1 * scale)) and torch.equal(bits(s), bits(s1)), scale
    third = float(np.float32(1.0 / 3.0))
    for what, wt, lam in (("w == 1, lambda 0.2", torch.ones_like(w), 0.2), ("random weights, lambda 0", w, 0.0)):
        _, g1, s1 = abi_wloss(lib, x, y, wt, lam)
        _, g, s = abi_wloss(lib, x, y, wt, lam, scale=third)
        assert torch.equal(bits(s), bits(s1)), what
        want = g1.double() * third
        ulp = torch.from_numpy(np.spacing(np.abs(want.cpu().numpy()).astype(np.float32)).astype(np.float64)).cuda()
        off = ((g.double() - want).abs() / ulp).max()
        print("grad_scale 1/3, %s: max %.2f float32 ulps of the entry" % (what, float(off)))
        assert float(off) <= 2.0, what


def test_on_another_stream(lib, mid):
    x, y, w = mid
    _, g0, s0 = abi_wloss(lib, x, y, w)
    _, g1, s1 = abi_wloss(lib, x, y, w, stream=torch.cuda.Stream())
    assert torch.equal(bits(g0), bits(g1)) and torch.equal(bits(s0), bits(s1))


def test_short_workspace_is_an_error_code_before_any_launch(lib, mid):
    x, y, w = mid
    rc, grad, stats = abi_wloss(lib, x, y, w, ws_short=1)
    assert rc == EGS_ERR_WORKSPACE
    assert bool(torch.isnan(grad).all()) and bool(torch.isnan(stats).all())      # nothing ran
    assert b"workspace" in lib.egs_wloss_last_error_string()


# --------------------------------------------------------------------------- the Python wrapper
def test_python_wrapper(lib, mid):
    from easygaussiansplatting_amd.loss import gau_loss, gau_loss_with_grad
    x, y, w = mid
    H, W = MID
    _, g0, s0 = abi_wloss(lib, x, y, w, 0.3, 0.5)
    stats, grad = gau_loss_with_grad(x, y, 0.3, grad_scale=0.5, weight=w)
    torch.cuda.synchronize()
    assert tuple(stats.shape) == (4,) and torch.equal(bits(stats), bits(s0)) and torch.equal(bits(grad), bits(g0))
    stats2, none = gau_loss_with_grad(x, y, 0.3, need_grad=False, weight=w)
    assert none is None and torch.equal(bits(stats2), bits(s0))
    # bool and uint8 masks are 0 / 1 weights; a strided view is made contiguous
    mask = w > 1.5
    _, gm, sm = abi_wloss(lib, x, y, mask.float())
    for m in (mask, mask.to(torch.uint8) * 255):
        st, gr = gau_loss_with_grad(x, y, weight=m)
        assert torch.equal(bits(st), bits(sm)) and torch.equal(bits(gr), bits(gm))
    big = torch.zeros((H + 2, W + 3), device="cuda")
    big[:H, :W] = w
    st, gr = gau_loss_with_grad(x, y, 0.3, grad_scale=0.5, weight=big[:H, :W])
    assert torch.equal(bits(st), bits(s0)) and torch.equal(bits(gr), bits(g0))
    # the autograd form: no gradient into the weight, the image's scaled by the incoming one
    xr = x.clone().requires_grad_(True)
    loss = gau_loss(xr, y, 0.3, weight=w)
    (2.0 * loss).backward()
    _, g1, s1 = abi_wloss(lib, x, y, w, 0.3, 1.0)
    assert torch.equal(bits(loss.detach().reshape(1)), bits(s1[:1])) and torch.equal(bits(xr.grad), bits(g1 * 2.0))
    # refusals that need a GPU tensor to get that far
    with pytest.raises(ValueError, match="weight lives on cpu"):
        gau_loss_with_grad(x, y, weight=w.cpu())
    with pytest.raises(ValueError, match="weight must have shape"):
        gau_loss_with_grad(x, y, weight=w[:, :-1])
    # and an unweighted call is what it was: three stats
    st3, _ = gau_loss_with_grad(x, y)
    assert tuple(st3.shape) == (3,)
