"""The depth-prior loss (csrc/egs_depthloss.hip: k_depth_sums, k_depth_grad) against the float64 form of its
definition (tests/depth_loss_ref.py) under that module's rule: 4 x what the float32 restatement loses on the case, at
least one float32 ulp.

The C ABI is called directly on buffers the test owns, with the helpers of tests/loss_abi.py: workspace, both gradient
planes and ``stats`` NaN-filled between guard bands that must be intact afterwards.  No buffer is ever smaller than the
ABI asks for: the too-small workspace is an error code returned before any launch.

Shapes (depth_loss_ref.SHAPES): 1x1, 1x2 (no float4 step at all), 5x200, 11x11 (121 = 30 float4 steps and a tail of
one), 17x65, 33x129 (5 workgroups, tail of one), 272x1024 (272 workgroups), 601x999 (587 workgroups' worth on a grid of
at most 512: the strided walk, and a tail of three).  At 1x1 and 1x2 "affine" (degenerate; an exact fit) and "pearson"
(degenerate; rho = +-1 exactly) have residuals and gradients that are rounding alone: they are checked through ``stats``,
and the gradient at those sizes through "metric".
"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import depth_loss_ref as DR
from tests import weighted_loss_ref as WR

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.loss_abi import EGS_ERR_WORKSPACE, bits, dev, guarded, guards_intact  # noqa: E402  (needs torch)

KIND_ID = {"metric": 0, "affine": 1, "pearson": 2}
sid = lambda s: "%dx%d" % s


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from easygaussiansplatting_amd import _depthlosslib
    return _depthlosslib.load()


def abi_depth(lib, D, A, q, w, kind, alpha_min=DR.ALPHA_MIN, scale=1.0, ws_short=0, need_grad=True, stream=None):
    """egs_depthloss on buffers this test owns -> (rc, dD [H,W] or None, dA, stats [6]); asserts the guards."""
    H, W = int(D.shape[0]), int(D.shape[1])
    for t in (D, A, q) + (() if w is None else (w,)):
        assert tuple(t.shape) == (H, W) and t.dtype == torch.float32 and t.is_contiguous()
    ws_bytes = int(lib.egs_depthloss_ws_bytes(H, W))
    assert ws_bytes % 8 == 0
    ws_all, ws = guarded(ws_bytes)
    d_all, gd = guarded(4 * H * W)
    a_all, ga = guarded(4 * H * W)
    s_all, s = guarded(24)
    for inner in (ws, gd, ga, s):
        inner.view(torch.float32).fill_(float("nan"))
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    st = stream if stream is not None else torch.cuda.current_stream()
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())      # the fills above
    rc = lib.egs_depthloss(H, W, p(D), p(A), p(q), p(w), KIND_ID[kind], float(alpha_min), float(scale), p(ws),
                           ws_bytes - ws_short, p(s), p(gd) if need_grad else None, p(ga) if need_grad else None,
                           C.c_void_p(st.cuda_stream))
    st.synchronize()
    torch.cuda.synchronize()
    for whole, nm in ((ws_all, "workspace"), (d_all, "dloss_ddepth"), (a_all, "dloss_dalpha"), (s_all, "stats")):
        assert guards_intact(whole), "%dx%d: the kernels wrote outside %s" % (H, W, nm)
    dD, dA = (g.view(torch.float32).reshape(H, W).clone() for g in (gd, ga))
    if not need_grad:
        assert bool(torch.isnan(dD).all()) and bool(torch.isnan(dA).all()), "a gradient was written though none was asked"
        dD = dA = None
    return rc, dD, dA, s.view(torch.float32).clone()


def as_result(stats, dD, dA):
    s = stats.tolist()
    return dict(loss=s[0], s=s[1], t=s[2], omega=s[3], rho=s[4], degenerate=s[5], dD=dD.cpu().numpy(), dA=dA.cpu().numpy())


@functools.lru_cache(maxsize=None)
def generated(H, W):
    return DR.make_case(H, W)


def check_case(lib, Dn, An, qn, wn, kind, what, alpha_min=DR.ALPHA_MIN, scale=1.0, stats_only=False):
    """the kernel against float64 under the rule; every entry of both planes and of stats written; the same bits twice"""
    D, A, q = dev(Dn), dev(An), dev(qn)
    w = None if wn is None else dev(wn)
    rc, dD, dA, stats = abi_depth(lib, D, A, q, w, kind, alpha_min, scale)
    assert rc == 0, what
    n_bad = int((~torch.isfinite(dD)).sum() + (~torch.isfinite(dA)).sum())
    assert n_bad == 0 and bool(torch.isfinite(stats).all()), "%s: %d gradient entries never written" % (what, n_bad)
    want = DR.ref(Dn, An, qn, kind, wn, alpha_min, scale)
    e_ref = DR.errors(DR.ref(Dn, An, qn, kind, wn, alpha_min, scale, dtype=np.float32), want)
    got = as_result(stats, dD, dA)
    e_hip = DR.errors(got, want)
    print("%s %s: valid %d left out %d | loss %.6g s %.6g t %.6g rho %.6g | e_ref %s | e_hip %s" % (
        what, kind, DR.compared(want)[2], DR.compared(want)[1], want["loss"], want["s"], want["t"], want["rho"],
        {k: "%.2e" % v for k, v in e_ref.items()}, {k: "%.2e" % v for k, v in e_hip.items()}))
    DR.check_against(got, want, "%s %s" % (what, kind), e_ref, stats_only=stats_only)
    invalid = torch.from_numpy(~want["valid"]).cuda()
    assert bool((dD[invalid] == 0).all()) and bool((dA[invalid] == 0).all()), "%s: a gradient at an invalid pixel" % what
    rc2, dD2, dA2, stats2 = abi_depth(lib, D, A, q, w, kind, alpha_min, scale)      # fresh NaN-filled buffers
    assert rc2 == 0 and torch.equal(bits(dD), bits(dD2)) and torch.equal(bits(dA), bits(dA2)) and \
        torch.equal(bits(stats), bits(stats2)), "%s: two calls differ" % what
    return dD, dA, stats, want


# --------------------------------------------------------------------------- generated cases against float64
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("kind", DR.KINDS)
@pytest.mark.parametrize("shape", DR.SHAPES, ids=sid)
def test_shape_by_kind(lib, shape, kind, weighted):
    H, W = shape
    Dn, An, qn = generated(H, W)
    wn = WR.make_weight("uniform", H, W) if weighted else None
    check_case(lib, Dn, An, qn, wn, kind, "generated %dx%d%s" % (H, W, " weighted" if weighted else ""),
               stats_only=kind != "metric" and H * W <= 2)


@pytest.mark.parametrize("pattern", WR.PATTERNS)
def test_weight_patterns(lib, pattern):
    H, W = 33, 129
    Dn, An, qn = generated(H, W)
    wn = WR.make_weight(pattern, H, W)
    for kind in DR.KINDS:
        # ("pixel": one weighted pixel -- the degenerate rules, on the device)
        _, _, stats, want = check_case(lib, Dn, An, qn, wn, kind, "33x129 %s" % pattern, scale=0.25)
        if pattern == "pixel":
            assert want["degenerate"] == (0 if kind == "metric" else 1) == int(stats[5])


# --------------------------------------------------------------------------- hand-built cases
@pytest.mark.parametrize("shape", [(1, 1), (33, 129), (601, 999)], ids=sid)
def test_no_valid_pixel(lib, shape):
    H, W = shape
    Dn, An, qn = generated(H, W)
    D, A = dev(Dn), dev(An)
    for kind in DR.KINDS:
        for what, q, a in (("zero prior", torch.zeros((H, W), device="cuda"), A),
                           ("NaN prior", torch.full((H, W), float("nan"), device="cuda"), A),
                           ("empty render", dev(np.abs(qn) + 1), torch.full((H, W), 0.05, device="cuda"))):
            for need_grad in (True, False):
                rc, dD, dA, stats = abi_depth(lib, D, a, q, None, kind, need_grad=need_grad)
                assert rc == 0 and stats.tolist() == [0.0, 1.0, 0.0, 0.0, 0.0, 1.0], (kind, what, stats.tolist())
                if need_grad:
                    assert bool((dD == 0).all()) and bool((dA == 0).all()), (kind, what)


def test_priors_without_data_do_not_count(lib):
    """NaN, +-inf, zero and negative priors, NaN depth and alpha: as if the pixel were not there"""
    H, W = 33, 129
    Dn, An, qn = generated(H, W)
    qn, Dn, An = qn.copy(), Dn.copy(), An.copy()
    flat = qn.reshape(-1)
    rng = np.random.default_rng(5)
    idx = rng.permutation(H * W)[:600]
    for k, bad in enumerate((np.nan, np.inf, -np.inf, -0.5, 0.0, -0.0)):
        flat[idx[100 * k:100 * k + 100]] = bad
    Dn.reshape(-1)[idx[:50]] = np.nan
    Dn.reshape(-1)[rng.permutation(H * W)[:50]] = -1.0
    An.reshape(-1)[rng.permutation(H * W)[:50]] = np.nan
    for kind in DR.KINDS:
        for wn in (None, WR.make_weight("uniform", H, W)):
            _, _, stats, want = check_case(lib, Dn, An, qn, wn, kind, "no-data priors")
            assert 0 < want["omega"] and int(want["valid"].sum()) < H * W - 600


def test_alpha_min_is_exclusive(lib):
    """A == alpha_min does not count, the next float does"""
    H, W = 17, 65
    Dn, An, qn = generated(H, W)
    qn = np.abs(qn) + np.float32(0.01)
    z = Dn / An
    for alpha_min in (0.05, 1e-3, 0.5):
        lo = np.float32(alpha_min)
        An = An.copy()
        An[:, ::2] = lo
        An[:, 1::2] = np.nextafter(lo, np.float32(2))
        for kind in DR.KINDS:
            _, _, stats, want = check_case(lib, (An * z).astype(np.float32), An, qn, None, kind,
                                           "alpha_min %g" % alpha_min, alpha_min=alpha_min)
            assert float(stats[3]) == H * (W // 2) == want["omega"]


@pytest.mark.parametrize("cut", [100, 1024, 1025, 2051, 4256])
def test_edge_of_the_valid_region(lib, cut):
    """the first ``cut`` pixels (flat order) have a prior: the edge inside a wave (100 = float4 step 25), on a workgroup
    boundary (1024 = 256 threads x 4), one past it, inside a float4 (2051), and everything but the scalar tail (4256)"""
    H, W = 33, 129
    Dn, An, qn = generated(H, W)
    qn = (np.abs(qn) + np.float32(0.01)).astype(np.float32)
    qn.reshape(-1)[cut:] = 0.0
    for kind in DR.KINDS:
        dD, dA, stats, want = check_case(lib, Dn, An, qn, None, kind, "valid below %d" % cut)
        assert float(stats[3]) == cut
        assert bool((dD.reshape(-1)[cut:] == 0).all()) and bool((dA.reshape(-1)[cut:] == 0).all())
        if kind != "pearson":
            assert int((dA.reshape(-1)[:cut] != 0).sum()) >= cut - 2


# --------------------------------------------------------------------------- the calling conventions
MID = (200, 700)      # 137 workgroups: the reductions loop over the partials


@pytest.fixture(scope="module")
def mid(lib):
    D, A, q = map(dev, DR.make_case(*MID))
    return D, A, q, dev(WR.make_weight("uniform", *MID))


@pytest.mark.parametrize("kind", DR.KINDS)
@pytest.mark.parametrize("shape", DR.SHAPES, ids=sid)
def test_unit_weights_give_the_bits_of_no_weights(lib, shape, kind):
    H, W = shape
    D, A, q = map(dev, generated(H, W))
    ones = torch.ones((H, W), device="cuda")
    for need_grad in (True, False):
        rc, dD, dA, stats = abi_depth(lib, D, A, q, ones, kind, scale=0.5, need_grad=need_grad)
        rc0, dD0, dA0, stats0 = abi_depth(lib, D, A, q, None, kind, scale=0.5, need_grad=need_grad)
        assert rc == 0 and rc0 == 0 and torch.equal(bits(stats), bits(stats0)), (stats.tolist(), stats0.tolist())
        if need_grad:
            assert torch.equal(bits(dD), bits(dD0)) and torch.equal(bits(dA), bits(dA0))


@pytest.mark.parametrize("kind", DR.KINDS)
def test_stats_do_not_depend_on_need_grad(lib, mid, kind):
    D, A, q, w = mid
    for wt in (None, w):
        _, dD, _, with_grad = abi_depth(lib, D, A, q, wt, kind)
        _, none, _, without = abi_depth(lib, D, A, q, wt, kind, need_grad=False)
        assert none is None and dD is not None
        assert torch.equal(bits(with_grad), bits(without)), (with_grad.tolist(), without.tolist())


@pytest.mark.parametrize("kind", DR.KINDS)
def test_grad_scale(lib, mid, kind):
    """powers of two scale the bits; the stats do not see the scale"""
    D, A, q, w = mid
    _, dD1, dA1, s1 = abi_depth(lib, D, A, q, w, kind)
    for scale in (0.125, 4.0, -2.0):
        _, dD, dA, s = abi_depth(lib, D, A, q, w, kind, scale=scale)
        assert torch.equal(bits(dD + 0.0), bits(dD1 * scale + 0.0)) and torch.equal(bits(dA + 0.0), bits(dA1 * scale + 0.0))
        assert torch.equal(bits(s), bits(s1)), scale
    _, dD0, dA0, _ = abi_depth(lib, D, A, q, w, kind, scale=0.0)
    assert bool((dD0 == 0).all()) and bool((dA0 == 0).all())


@pytest.mark.parametrize("kind", DR.KINDS)
def test_on_another_stream(lib, mid, kind):
    D, A, q, w = mid
    _, dD0, dA0, s0 = abi_depth(lib, D, A, q, w, kind)
    _, dD1, dA1, s1 = abi_depth(lib, D, A, q, w, kind, stream=torch.cuda.Stream())
    assert torch.equal(bits(dD0), bits(dD1)) and torch.equal(bits(dA0), bits(dA1)) and torch.equal(bits(s0), bits(s1))


def test_short_workspace_is_an_error_code_before_any_launch(lib, mid):
    D, A, q, w = mid
    rc, dD, dA, stats = abi_depth(lib, D, A, q, w, "affine", ws_short=1)
    assert rc == EGS_ERR_WORKSPACE
    assert bool(torch.isnan(dD).all()) and bool(torch.isnan(dA).all()) and bool(torch.isnan(stats).all())   # nothing ran
    assert b"workspace" in lib.egs_depthloss_last_error_string()


def test_unaligned_planes_take_the_scalar_walk(lib):
    """planes that start 4 B past a 16-B boundary: no float4 step; the result is that of the aligned call but for the
    order of the sums"""
    H, W = 33, 129
    Dn, An, qn = generated(H, W)
    pad = lambda a: dev(np.concatenate([[0.0], a.reshape(-1)]))[1:].view(H, W)
    D, A, q = pad(Dn), pad(An), pad(qn)
    assert D.data_ptr() % 16 == 4 and D.is_contiguous()
    for kind in DR.KINDS:
        rc, dD, dA, stats = abi_depth(lib, D, A, q, None, kind)
        rc0, dD0, dA0, stats0 = abi_depth(lib, dev(Dn), dev(An), dev(qn), None, kind)
        assert rc == 0 and rc0 == 0
        assert float((stats - stats0).abs().max()) <= 1e-6 * float(stats0.abs().max())
        assert float((dD - dD0).abs().max()) <= 1e-6 * float(dD0.abs().max())
        assert float((dA - dA0).abs().max()) <= 1e-6 * float(dA0.abs().max())


# --------------------------------------------------------------------------- the Python wrapper
def test_python_wrapper(lib, mid):
    from easygaussiansplatting_amd.depthloss import depth_loss, depth_loss_with_grad
    D, A, q, w = mid
    H, W = MID
    for kind in DR.KINDS:
        _, dD0, dA0, s0 = abi_depth(lib, D, A, q, w, kind, alpha_min=0.1, scale=0.5)
        stats, dd, da = depth_loss_with_grad(D[None], A[None], q, kind, weight=w, alpha_min=0.1, grad_scale=0.5)
        torch.cuda.synchronize()
        assert tuple(stats.shape) == (6,) and tuple(dd.shape) == (1, H, W) == tuple(da.shape)
        assert torch.equal(bits(stats), bits(s0)) and torch.equal(bits(dd[0]), bits(dD0)) and torch.equal(bits(da[0]), bits(dA0))
        stats2, none, none2 = depth_loss_with_grad(D, A, q, kind, weight=w, alpha_min=0.1, need_grad=False)
        assert none is None and none2 is None and torch.equal(bits(stats2), bits(s0))
    # a strided view is made contiguous
    big = torch.zeros((H + 2, W + 3), device="cuda")
    big[:H, :W] = q
    _, dD0, dA0, s0 = abi_depth(lib, D, A, q, None, "affine")
    st, dd, da = depth_loss_with_grad(D[None], A[None], big[:H, :W])
    assert torch.equal(bits(st), bits(s0)) and torch.equal(bits(dd[0]), bits(dD0))
    # the autograd form: gradients into depth and alpha scaled by the incoming one, none into the prior
    Dr, Ar = D[None].clone().requires_grad_(True), A[None].clone().requires_grad_(True)
    qr = q.clone().requires_grad_(True)
    loss = depth_loss(Dr, Ar, qr)
    (2.0 * loss).backward()
    assert torch.equal(bits(loss.detach().reshape(1)), bits(s0[:1]))
    assert torch.equal(bits(Dr.grad[0]), bits(dD0 * 2.0)) and torch.equal(bits(Ar.grad[0]), bits(dA0 * 2.0))
    assert qr.grad is None
    # refusals that need a GPU tensor to get that far
    with pytest.raises(ValueError, match="prior lives on cpu"):
        depth_loss_with_grad(D, A, q.cpu())
    with pytest.raises(ValueError, match="alpha must have shape"):
        depth_loss_with_grad(D, A[:, :-1], q)
