"""The normal loss (csrc/egs_normalloss.hip: k_normal_tile, k_normal_pairs, k_normal_grad) against the
float64 form of its definition (tests/normal_loss_ref.py) under that module's rule: 4 x what the float32 restatement
loses on the case, at least one float32 ulp (the losses: 2^-23), and the same set of pixels with a normal.

The C ABI is called directly on buffers the test owns, with the helpers of tests/loss_abi.py: workspace, both gradient
planes, ``normals_out`` and ``stats`` NaN-filled between guard bands that must be intact afterwards.  No buffer is ever
smaller than the ABI asks for: the too-small workspace is an error code returned before any launch.

Shapes: 1x1, 1x7, 7x1, 2x2 (no pixel has a normal), 3x3 (one pixel, no pair), 3x4 and 4x3 (one pair), 5x5 (the centre
is reached by all four neighbours); with TH x TW the tile: TH x TW, one and two more each way (seams at halo one and
two), (2 TH + 1) x (3 TW + 3); 601 x 999 (2432 tiles on a grid of at most 2048 workgroups, the gradient pass on
fewer: the tile walk).
"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import normal_loss_ref as NR

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.loss_abi import EGS_ERR_WORKSPACE, bits, dev, guarded, guards_intact  # noqa: E402  (needs torch)

from easygaussiansplatting_amd._normallosslib import TILE_H as TH, TILE_W as TW  # noqa: E402

SMALL = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 3), (3, 4), (4, 3), (5, 5)]
SHAPES = SMALL + [(TH, TW), (TH + 1, TW + 1), (TH + 2, TW + 2), (2 * TH + 1, 3 * TW + 3), (601, 999)]
TERMS = {"both": (True, True), "prior": (True, False), "smooth": (False, True)}
sid = lambda s: "%dx%d" % s


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from easygaussiansplatting_amd import _normallosslib
    return _normallosslib.load()


def on_device(case):
    return {k: dev(v) for k, v in case.items()}


def abi_normal(lib, c, cam, prior=True, guide=True, smooth=True, weighted=False, alpha_min=NR.ALPHA_MIN,
               gamma=NR.EDGE_GAMMA, ps=1.0, ss=1.0, ws_short=0, need_grad=True, want_normals=True, stream=None):
    """egs_normalloss on buffers this test owns -> dict(rc, dD [H,W] or None, dA, stats [6], n [3,H,W] or None);
    asserts the guards.  ``c``: device tensors D, A, q, I, w."""
    H, W = int(c["D"].shape[0]), int(c["D"].shape[1])
    for k, shp in (("D", (H, W)), ("A", (H, W)), ("q", (3, H, W)), ("I", (3, H, W)), ("w", (H, W))):
        assert tuple(c[k].shape) == shp and c[k].dtype == torch.float32 and c[k].is_contiguous()
    ws_bytes = int(lib.egs_normalloss_ws_bytes(H, W))
    assert ws_bytes % 16 == 0 and ws_bytes >= 32 * H * W
    ws_all, ws = guarded(ws_bytes)
    d_all, gd = guarded(4 * H * W)
    a_all, ga = guarded(4 * H * W)
    n_all, gn = guarded(12 * H * W)
    s_all, s = guarded(24)
    for inner in (ws, gd, ga, gn, s):
        inner.view(torch.float32).fill_(float("nan"))
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    st = stream if stream is not None else torch.cuda.current_stream()
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())      # the fills above
    rc = lib.egs_normalloss(H, W, p(c["D"]), p(c["A"]), *[float(v) for v in cam], p(c["q"]) if prior else None,
                            p(c["I"]) if guide else None, p(c["w"]) if weighted else None, 1 if smooth else 0,
                            float(alpha_min), float(gamma), float(ps), float(ss), p(ws), ws_bytes - ws_short, p(s),
                            p(gn) if want_normals else None, p(gd) if need_grad else None,
                            p(ga) if need_grad else None, C.c_void_p(st.cuda_stream))
    st.synchronize()
    torch.cuda.synchronize()
    for whole, nm in ((ws_all, "workspace"), (d_all, "dloss_ddepth"), (a_all, "dloss_dalpha"), (n_all, "normals_out"),
                      (s_all, "stats")):
        assert guards_intact(whole), "%dx%d: the kernels wrote outside %s" % (H, W, nm)
    dD, dA = (g.view(torch.float32).reshape(H, W).clone() for g in (gd, ga))
    n = gn.view(torch.float32).reshape(3, H, W).clone()
    if not need_grad:
        assert bool(torch.isnan(dD).all()) and bool(torch.isnan(dA).all()), "a gradient was written though none was asked"
        dD = dA = None
    if not want_normals:
        assert bool(torch.isnan(n).all())
        n = None
    return dict(rc=rc, dD=dD, dA=dA, stats=s.view(torch.float32).clone(), n=n)


def as_result(r):
    s = r["stats"].tolist()
    n = r["n"].cpu().numpy()
    return dict(Lp=s[0], Ls=s[1], Op=s[2], Os=s[3], count=s[4], flags=s[5], n=n, nvalid=(n != 0).any(0),
                dD=r["dD"].cpu().numpy(), dA=r["dA"].cpu().numpy())


def same_bits(r0, r1, keys=("stats", "dD", "dA", "n")):
    return all(r0[k] is None and r1[k] is None or torch.equal(bits(r0[k]), bits(r1[k])) for k in keys)


@functools.lru_cache(maxsize=None)
def generated(H, W, kind):
    return NR.make_case(H, W, kind)


def check_case(lib, case, cam, what, twice=True, **kw):
    """the kernel against float64 under the rule; every entry of both planes, of normals_out and of stats written; the
    same bits twice"""
    c = on_device(case)
    r = abi_normal(lib, c, cam, **kw)
    assert r["rc"] == 0, what
    n_bad = sum(int((~torch.isfinite(r[k])).sum()) for k in ("dD", "dA", "n", "stats"))
    assert n_bad == 0, "%s: %d entries never written (or not finite)" % (what, n_bad)
    rk = dict(prior=kw.get("prior", True), guide=kw.get("guide", True), smooth=kw.get("smooth", True),
              weighted=kw.get("weighted", False), alpha_min=kw.get("alpha_min", NR.ALPHA_MIN),
              edge_gamma=kw.get("gamma", NR.EDGE_GAMMA), prior_scale=kw.get("ps", 1.0), smooth_scale=kw.get("ss", 1.0))
    want = NR.ref(case, cam, **rk)
    f32 = NR.ref(case, cam, dtype=torch.float32, **rk)
    assert np.array_equal(f32["nvalid"], want["nvalid"]), "%s: float32 and float64 disagree on a pixel's validity" % what
    e_ref = NR.errors(f32, want)
    got = as_result(r)
    e_hip = NR.errors(got, want)
    print("%s: normals %d | Lp %.6g Ls %.6g Op %.6g Os %.6g | e_ref %s | e_hip %s" % (
        what, want["count"], want["Lp"], want["Ls"], want["Op"], want["Os"],
        {k: "%.2e" % v for k, v in e_ref.items()}, {k: "%.2e" % v for k, v in e_hip.items()}))
    NR.check_against(got, want, what, e_ref)
    invalid = torch.from_numpy(~want["dvalid"]).cuda()
    assert bool((r["dD"][invalid] == 0).all()) and bool((r["dA"][invalid] == 0).all()), \
        "%s: a gradient at a pixel that is not depth-valid" % what
    if twice:
        r2 = abi_normal(lib, c, cam, **kw)      # fresh NaN-filled buffers
        assert r2["rc"] == 0 and same_bits(r, r2), "%s: two calls differ" % what
    return r, want


# --------------------------------------------------------------------------- generated cases against float64
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("terms", list(TERMS))
@pytest.mark.parametrize("kind", NR.KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_shape_by_kind(lib, shape, kind, terms, weighted):
    H, W = shape
    case, cam = generated(H, W, kind)
    prior, smooth = TERMS[terms]
    r, want = check_case(lib, case, cam, "generated %dx%d %s %s%s" % (H, W, kind, terms, " weighted" if weighted else ""),
                         prior=prior, smooth=smooth, weighted=weighted)
    if H < 3 or W < 3:
        assert want["count"] == 0 and r["stats"].tolist() == [0, 0, 0, 0, 0, (1 if prior else 0) + (2 if smooth else 0)]
    if (H, W) == (3, 3):
        assert want["count"] <= 1 and want["Os"] == 0
    if min(H, W) >= TH:
        assert want["count"] > 0.5 * (H - 2) * (W - 2)


# --------------------------------------------------------------------------- hand-built cases
def smooth_case(H, W, seed=3):
    """a wavy surface under full opacity-ish alpha: every interior pixel has a normal"""
    case, cam = NR.make_case(H, W, "wavy", seed=seed)
    case = {k: v.copy() for k, v in case.items()}
    z = case["D"] / case["A"]
    case["A"] = np.where(case["A"] < 0.06, np.float32(0.5), case["A"]).astype(np.float32)
    case["D"] = (case["A"] * z).astype(np.float32)
    q = case["q"]
    q[:, (q == 0).all(0)] = np.float32(-1.0)       # every prior has data
    return case, cam


@pytest.mark.parametrize("hole", ["alpha", "nan_depth", "nan_alpha"])
def test_one_invalid_pixel_takes_five_normals(lib, hole):
    H = W = 7
    case, cam = smooth_case(H, W)
    if hole == "alpha":
        case["A"][3, 3] = NR.ALPHA_MIN
    elif hole == "nan_depth":
        case["D"][3, 3] = np.nan
    else:
        case["A"][3, 3] = np.nan
    c = on_device(case)
    r = abi_normal(lib, c, cam)
    assert r["rc"] == 0
    for k in ("dD", "dA", "n", "stats"):
        assert bool(torch.isfinite(r[k]).all()), k
    have = (r["n"] != 0).any(0).cpu().numpy()
    want = np.zeros((H, W), bool)
    want[1:-1, 1:-1] = True
    for y, x in ((3, 3), (2, 3), (4, 3), (3, 2), (3, 4)):
        want[y, x] = False
    assert np.array_equal(have, want) and float(r["stats"][4]) == 20
    assert float(r["dD"][3, 3]) == 0 and float(r["dA"][3, 3]) == 0
    if hole == "alpha":
        check_case(lib, case, cam, "7x7 hole")


def test_corners_get_no_gradient_and_borders_do(lib):
    H, W = 9, 11
    case, cam = smooth_case(H, W)
    r, _ = check_case(lib, case, cam, "9x11 borders")
    for name in ("dD", "dA"):
        g = r[name]
        for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
            assert float(g[y, x]) == 0, (name, y, x)
        assert bool((g[0, 1:-1] != 0).all()) and bool((g[-1, 1:-1] != 0).all())
        assert bool((g[1:-1, 0] != 0).all()) and bool((g[1:-1, -1] != 0).all())
    assert bool((r["n"][:, 0] == 0).all()) and bool((r["n"][:, :, -1] == 0).all())


def test_alpha_min_is_exclusive(lib):
    """A == alpha_min does not count, the next float does"""
    H, W = 9, 40
    case, cam = smooth_case(H, W)
    z = case["D"] / case["A"]
    for alpha_min in (0.05, 1e-3, 0.5):
        lo = np.float32(alpha_min)
        A = np.full((H, W), np.nextafter(lo, np.float32(2)), np.float32)
        A[:, 20] = lo
        cs = dict(case, A=A, D=(A * z).astype(np.float32))
        r, want = check_case(lib, cs, cam, "alpha_min %g" % alpha_min, alpha_min=alpha_min)
        # column 20 and its two neighbours have no normal
        assert float(r["stats"][4]) == (H - 2) * (W - 2 - 3) == want["count"]
        assert bool((r["dD"][:, 20] == 0).all()) and bool((r["dA"][:, 20] == 0).all())


def test_priors_without_data_leave_the_prior_term_only(lib):
    H, W = 9, 40
    case, cam = smooth_case(H, W)
    base = abi_normal(lib, on_device(case), cam)
    q = case["q"].copy()
    q[:, 2, 5] = 0.0
    q[0, 3, 6] = np.nan
    q[1, 4, 7] = np.inf
    q[2, 5, 8] = -np.inf
    cs = dict(case, q=q)
    r, want = check_case(lib, cs, cam, "no-data priors", weighted=False)
    assert float(r["stats"][2]) == float(base["stats"][2]) - 4 == want["Op"]
    assert torch.equal(bits(r["stats"][3:5]), bits(base["stats"][3:5])) and float(r["stats"][1]) == float(base["stats"][1])
    # no prior anywhere: the prior term is degenerate (bit 0), the smoothness term is what it was
    cs = dict(case, q=np.zeros_like(q))
    r0 = abi_normal(lib, on_device(cs), cam)
    only_s = abi_normal(lib, on_device(case), cam, prior=False)
    assert r0["stats"].tolist()[0] == 0 and r0["stats"].tolist()[2] == 0 and r0["stats"].tolist()[5] == 1
    assert only_s["stats"].tolist()[5] == 0
    assert torch.equal(bits(r0["dD"]), bits(only_s["dD"])) and torch.equal(bits(r0["dA"]), bits(only_s["dA"]))


def test_a_perturbed_depth_at_a_tile_corner(lib):
    """a plane but for one pixel at the corner of four tiles: its four neighbours' normals and the pairs around them"""
    H, W = 2 * TH + 3, 2 * TW + 3
    case, cam = NR.make_case(H, W, "plane")
    case = {k: v.copy() for k, v in case.items()}
    z = case["D"] / case["A"]
    case["A"][:] = 0.8
    z[TH, TW] *= 1.01
    case["D"] = (np.float32(0.8) * z).astype(np.float32)
    r, want = check_case(lib, case, cam, "tile corner")
    assert want["count"] == (H - 2) * (W - 2)
    assert want["Ls"] > 1e-6
    r_s = abi_normal(lib, on_device(case), cam, prior=False, guide=False)
    far = torch.ones((H, W), dtype=torch.bool, device="cuda")
    far[TH - 3:TH + 4, TW - 3:TW + 4] = False
    near_mag = float(r_s["dD"][TH - 2:TH + 3, TW - 2:TW + 3].abs().max())
    assert near_mag > 0 and float(r_s["dD"][far].abs().max()) < 1e-3 * near_mag


@pytest.mark.parametrize("shape", [(5, 5), (TH + 2, TW + 2), (2 * TH + 1, 3 * TW + 3)], ids=sid)
def test_unit_weights_and_a_constant_guide_change_no_bit(lib, shape):
    H, W = shape
    case, cam = generated(H, W, "wavy")
    c = on_device(case)
    c1 = dict(c, w=torch.ones((H, W), device="cuda"), I=torch.full((3, H, W), 0.37, device="cuda"))
    for need_grad in (True, False):
        a = abi_normal(lib, c1, cam, weighted=True, guide=False, need_grad=need_grad)
        b = abi_normal(lib, c, cam, weighted=False, guide=False, need_grad=need_grad)
        assert a["rc"] == 0 and b["rc"] == 0 and same_bits(a, b), "w = 1 differs from w = NULL"
        a = abi_normal(lib, c1, cam, guide=True, need_grad=need_grad)
        b = abi_normal(lib, c, cam, guide=False, need_grad=need_grad)
        assert same_bits(a, b), "a constant guide differs from no guide"


MID = (3 * TH + 5, 4 * TW + 7)


@pytest.fixture(scope="module")
def mid(lib):
    case, cam = NR.make_case(*MID, "wavy")
    return on_device(case), cam, case


def test_both_scales_give_the_sum_of_the_single_terms(lib, mid):
    c, cam, _ = mid
    both = abi_normal(lib, c, cam, weighted=True, ps=0.7, ss=1.9)
    p = abi_normal(lib, c, cam, weighted=True, ps=0.7, ss=0.0)
    s = abi_normal(lib, c, cam, weighted=True, ps=0.0, ss=1.9)
    sp = abi_normal(lib, c, cam, weighted=True, smooth=False, ps=0.7)
    ss_ = abi_normal(lib, c, cam, weighted=True, prior=False, ss=1.9)
    for k in ("dD", "dA"):
        top = max(float(t[k].abs().max()) for t in (both, p, s))
        assert float(both[k].abs().max()) > 0
        # (each call rounds its float64 gradient to float32 once: two ulps of the largest entry)
        assert float((both[k] - (p[k] + s[k])).abs().max()) <= 2 * NR.ulp32(top), k
        assert torch.equal(bits(p[k] + 0.0), bits(sp[k] + 0.0)) and torch.equal(bits(s[k] + 0.0), bits(ss_[k] + 0.0)), k
    assert torch.equal(bits(both["stats"]), bits(p["stats"]))


def test_power_of_two_scales_scale_the_bits(lib, mid):
    c, cam, _ = mid
    one = abi_normal(lib, c, cam, weighted=True)
    for scale in (0.125, 4.0, -2.0):
        r = abi_normal(lib, c, cam, weighted=True, ps=scale, ss=scale)
        for k in ("dD", "dA"):
            assert torch.equal(bits(r[k] + 0.0), bits(one[k] * scale + 0.0)), (k, scale)
        assert torch.equal(bits(r["stats"]), bits(one["stats"])) and torch.equal(bits(r["n"]), bits(one["n"]))
    zero = abi_normal(lib, c, cam, weighted=True, ps=0.0, ss=0.0)
    assert bool((zero["dD"] == 0).all()) and bool((zero["dA"] == 0).all())


@pytest.mark.parametrize("terms", list(TERMS))
def test_stats_do_not_depend_on_need_grad(lib, mid, terms):
    c, cam, _ = mid
    prior, smooth = TERMS[terms]
    a = abi_normal(lib, c, cam, prior=prior, smooth=smooth, weighted=True)
    b = abi_normal(lib, c, cam, prior=prior, smooth=smooth, weighted=True, need_grad=False)
    assert b["dD"] is None and a["dD"] is not None
    assert same_bits(a, b, ("stats", "n")), (a["stats"].tolist(), b["stats"].tolist())
    d = abi_normal(lib, c, cam, prior=prior, smooth=smooth, weighted=True, want_normals=False)
    assert same_bits(a, d, ("stats", "dD", "dA"))


def test_on_another_stream(lib, mid):
    c, cam, _ = mid
    a = abi_normal(lib, c, cam, weighted=True)
    b = abi_normal(lib, c, cam, weighted=True, stream=torch.cuda.Stream())
    assert same_bits(a, b)


def test_short_workspace_is_an_error_code_before_any_launch(lib, mid):
    c, cam, _ = mid
    r = abi_normal(lib, c, cam, ws_short=1)
    assert r["rc"] == EGS_ERR_WORKSPACE
    for k in ("dD", "dA", "n", "stats"):
        assert bool(torch.isnan(r[k]).all()), k      # nothing ran
    assert b"workspace" in lib.egs_normalloss_last_error_string()


# --------------------------------------------------------------------------- the Python wrapper
def test_python_wrapper(lib, mid):
    from easygaussiansplatting_amd.normalloss import depth_to_normals, normal_loss, normal_loss_with_grad
    c, cam, _ = mid
    H, W = MID
    D, A, q, I, w = c["D"], c["A"], c["q"], c["I"], c["w"]
    r0 = abi_normal(lib, c, cam, weighted=True, alpha_min=0.1, gamma=4.0, ps=0.5, ss=2.0)
    stats, dd, da = normal_loss_with_grad(D[None], A[None], cam, normals=q, guide=I, weight=w, alpha_min=0.1,
                                          edge_gamma=4.0, prior_scale=0.5, smooth_scale=2.0)
    torch.cuda.synchronize()
    assert tuple(stats.shape) == (6,) and tuple(dd.shape) == (1, H, W) == tuple(da.shape)
    assert torch.equal(bits(stats), bits(r0["stats"])) and torch.equal(bits(dd[0]), bits(r0["dD"])) and \
        torch.equal(bits(da[0]), bits(r0["dA"]))
    stats2, none, none2 = normal_loss_with_grad(D, A, cam, normals=q, guide=I, weight=w, alpha_min=0.1, edge_gamma=4.0,
                                                need_grad=False)
    assert none is None and none2 is None and torch.equal(bits(stats2), bits(r0["stats"]))
    # a camera object gives what the four numbers give; a strided view is made contiguous
    from easygaussiansplatting_amd.function import Camera
    camo = Camera.__new__(Camera)
    camo.fx, camo.fy, camo.cx, camo.cy = cam
    big = torch.zeros((3, H + 2, W + 3), device="cuda")
    big[:, :H, :W] = q
    r1 = abi_normal(lib, c, cam)
    st, dd, da = normal_loss_with_grad(D[None], A[None], camo, normals=big[:, :H, :W], guide=I)
    assert torch.equal(bits(st), bits(r1["stats"])) and torch.equal(bits(dd[0]), bits(r1["dD"]))
    nv = depth_to_normals(D[None], A[None], cam)
    assert tuple(nv.shape) == (3, H, W) and torch.equal(bits(nv), bits(r1["n"]))
    # the autograd form: gradients into depth and alpha scaled by the incoming one, none into the prior
    Dr, Ar = D[None].clone().requires_grad_(True), A[None].clone().requires_grad_(True)
    qr = q.clone().requires_grad_(True)
    loss = normal_loss(Dr, Ar, cam, normals=qr, guide=I)
    (2.0 * loss).backward()
    assert torch.equal(bits(loss.detach().reshape(1)), bits((r1["stats"][0] + r1["stats"][1]).reshape(1)))
    assert torch.equal(bits(Dr.grad[0]), bits(r1["dD"] * 2.0)) and torch.equal(bits(Ar.grad[0]), bits(r1["dA"] * 2.0))
    assert qr.grad is None
    # refusals that need a GPU tensor to get that far
    with pytest.raises(ValueError, match="normals lives on cpu"):
        normal_loss_with_grad(D, A, cam, normals=q.cpu())
    with pytest.raises(ValueError, match="alpha must have shape"):
        normal_loss_with_grad(D, A[:, :-1], cam)
