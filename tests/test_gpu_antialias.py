"""Anti-aliased rendering (``RenderOptions(antialiased=True)``) on the device: the fused path against the
float64 reference of tests/aa_ref.py (the oracle's own stages, drawn with the opacity alpha comp), every node and every
combination the option joins, and the one property the filter exists for -- the opacity mass of a sub-pixel Gaussian is
that of the undilated Gaussian."""
import os
import socket

import numpy as np
import pytest

from easygaussiansplatting_amd import scene as S
from oracle import gs_oracle as O
from oracle import io_oracle as IO
from tests import aa_ref
from tests.gradcheck import assert_grad_close
from tests.pose_ref import pose_vjp

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NAMES = ("pws", "shs", "alphas", "scales", "rots")
RAW = ("pws", "low_shs", "high_shs", "alphas_raw", "scales_raw", "rots_raw")


@pytest.fixture(scope="module")
def gsc():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from easygaussiansplatting_amd import gsplatcu
    gsplatcu.set_policy("gsplatcu")
    yield gsplatcu
    gsplatcu.set_policy("gsplatcu")


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def host(t):
    return t.detach().double().cpu().numpy()


def scene_256(sh=3):
    return S.small_scene(10_000, 256, 256, sh, seed=21)


def scene_250x170(sh=3):
    sc = S.small_scene(4_000, 250, 170, sh, seed=22)
    sc.cam = S.Camera(250, 170, 256.0, 256.0, 250 / 2.0 + 150.0, 85.0, np.eye(3), np.array([0.0, 0.0, 5.0]))
    return sc


SCENES = {"256": scene_256, "250x170": scene_250x170}


def leaves(sc):
    p = dict(pws=dev(sc.pws), shs=dev(sc.shs), alphas=dev(sc.alphas).reshape(-1, 1), scales=dev(sc.scales),
             rots=dev(sc.rots))
    for v in p.values():
        v.requires_grad_(True)
    return p


def raw_leaves(sc):
    a = sc.alphas.astype(np.float64)
    p = dict(pws=dev(sc.pws), low_shs=dev(sc.shs[:, :3]), high_shs=dev(sc.shs[:, 3:]),
             alphas_raw=dev(np.log(a / (1 - a))).reshape(-1, 1), scales_raw=dev(np.log(sc.scales.astype(np.float64))),
             rots_raw=dev(sc.rots))
    for v in p.values():
        v.requires_grad_(True)
    return p


def render(sc, cam, opts, p=None, raw=False):
    from easygaussiansplatting_amd.function import GSFunction, GSRawFunction
    us = torch.zeros((sc.n, 2), device="cuda", requires_grad=True)
    if raw:
        p = raw_leaves(sc) if p is None else p
        out = GSRawFunction.apply(*[p[k] for k in RAW], us, cam, opts)
    else:
        p = leaves(sc) if p is None else p
        out = GSFunction.apply(*[p[k] for k in NAMES], us, cam, opts)
    return out, p, us


def weights(sc, seed):
    H, W = sc.cam.height, sc.cam.width
    s = 1.0 / (H * W)
    return (S.normal(seed, 1, (3, H, W)) * s, S.normal(seed, 2, (H, W)) * s * 0.2, S.normal(seed, 3, (H, W)) * s)


def loss_of(out, opts, Wi, Wd=None, Wa=None):
    loss = (out[0] * dev(Wi)).sum()
    k = 2
    if opts.depth:
        loss = loss + (out[k][0] * dev(Wd)).sum(); k += 1
    if opts.alpha:
        loss = loss + (out[k][0] * dev(Wa)).sum()
    return loss


def zmax(sc):
    return float((sc.pws.astype(np.float64) @ np.asarray(sc.cam.Rcw).T + np.asarray(sc.cam.tcw))[:, 2].max())


def AA(**kw):
    from easygaussiansplatting_amd.function import RenderOptions
    return RenderOptions(antialiased=True, **kw)


# ---------------------------------------------------------------------------------------------- 1. forward parity
@pytest.mark.parametrize("name", list(SCENES))
@pytest.mark.parametrize("raw", [False, True])
@pytest.mark.parametrize("extras", [False, True])
def test_forward_parity_vs_oracle(gsc, name, raw, extras):
    from easygaussiansplatting_amd.function import Camera
    sc = SCENES[name](12 if raw else 3)
    cam = Camera.from_scene(sc.cam)
    bg = (0.2, 0.5, 0.9) if extras else None
    o = aa_ref.aa_oracle(sc, sc.cam, bg)
    assert (o["comp"][o["depths"] > 0.2] < 0.999).any()
    opts = AA(depth=True, alpha=True, background=bg) if extras else AA()
    out, _, _ = render(sc, cam, opts, raw=raw)
    assert np.abs(host(out[0]) - o["image"]).max() < 1e-4
    if extras:
        assert np.abs(host(out[3])[0] - o["alpha"]).max() < 1e-4
        assert np.abs(host(out[2])[0] - o["depth"]).max() < 1e-4 * zmax(sc)


# -------------------------------------------------------------------------------------- 2. gradients vs the oracle
@pytest.mark.parametrize("name", list(SCENES))
@pytest.mark.parametrize("extras", [False, True])
def test_gradients_vs_oracle(gsc, name, extras):
    from easygaussiansplatting_amd.function import Camera
    sc = SCENES[name]()
    sc.pws[:30, 2] = -9.0                      # some Gaussians behind the camera (near-culled: zero gradients)
    cam = Camera.from_scene(sc.cam)
    Wi, Wd, Wa = weights(sc, 7)
    bg = (0.2, 0.5, 0.9) if extras else None
    opts = AA(depth=True, alpha=True, background=bg) if extras else AA()
    o = aa_ref.aa_oracle(sc, sc.cam, bg, Wi, Wd if extras else None, Wa if extras else None)
    out, p, us = render(sc, cam, opts)
    loss_of(out, opts, Wi, Wd, Wa).backward()
    for k in NAMES:
        assert_grad_close(host(p[k].grad), o[k], "%s/%s:%s" % (name, extras, k))
    assert_grad_close(host(us.grad), o["us"], "%s/%s:us" % (name, extras))
    for k in NAMES:
        assert not host(p[k].grad)[:30].any(), k


# ------------------------------------------------------------------------------ 3. GSRawFunction == torch activations
@pytest.mark.parametrize("extras", [False, True])
def test_raw_equals_torch_activations(gsc, extras):
    from easygaussiansplatting_amd.function import Camera, GSFunction, GSRawFunction
    sc = scene_256(12)
    cam = Camera.from_scene(sc.cam)
    Wi, Wd, Wa = weights(sc, 9)
    opts = AA(depth=True, alpha=True, background=(0.3, 0.3, 0.1)) if extras else AA()
    p = raw_leaves(sc)
    u1 = torch.zeros((sc.n, 2), device="cuda", requires_grad=True)
    out1 = GSRawFunction.apply(*[p[k] for k in RAW], u1, cam, opts)
    loss_of(out1, opts, Wi, Wd, Wa).backward()
    q = {k: v.detach().requires_grad_(True) for k, v in p.items()}
    u2 = torch.zeros((sc.n, 2), device="cuda", requires_grad=True)
    act = (q["pws"], torch.cat((q["low_shs"], q["high_shs"]), 1), torch.sigmoid(q["alphas_raw"]),
           torch.exp(q["scales_raw"]), torch.nn.functional.normalize(q["rots_raw"]))
    out2 = GSFunction.apply(*act, u2, cam, opts)
    loss_of(out2, opts, Wi, Wd, Wa).backward()
    for a, b in zip(out1, out2):          # (image, mask, depth, alpha: the depth relative to its range)
        if a.dtype == torch.float32:
            assert float((a - b).detach().abs().max()) <= 1e-5 * max(1.0, float(b.detach().abs().max()))
    for k in RAW:
        assert_grad_close(host(p[k].grad), host(q[k].grad), "raw:" + k)
    assert_grad_close(host(u1.grad), host(u2.grad), "raw:us")


# ------------------------------------------------------------------------------------------------- 4. pose gradient
@pytest.mark.parametrize("extras", [False, True])
def test_pose_gradient_vs_oracle(gsc, extras):
    from tests.test_gpu_pose_grad import assert_pose_close, posed, run_pose
    sc = posed(S.small_scene(10_000, 256, 256, 12, seed=23))
    Wi, Wd, Wa = weights(sc, 3)
    bg = (0.2, 0.5, 0.9) if extras else None
    opts = AA(depth=True, alpha=True, background=bg) if extras else AA()
    _, _, (R, t) = run_pose(sc, opts, (Wi, Wd, Wa))
    o = aa_ref.aa_oracle(sc, sc.cam, bg, Wi, Wd if extras else None, Wa if extras else None)
    terms = pose_vjp(sc.pws, o["cov3ds"], sc.shs, sc.cam.Rcw, sc.cam.tcw, sc.cam, O.POLICY_G, o["us"], o["dcov2d"],
                     o["dcolour"], o["dz"], depths=o["depths"])
    assert_pose_close(host(R.grad), host(t.grad), terms, 1e-4, "aa")
    # the comp term is part of it: the pose gradient of the plain upstream would not pass
    o0 = aa_ref.aa_oracle(sc, sc.cam, bg, Wi, Wd if extras else None, Wa if extras else None, antialiased=False)
    terms0 = pose_vjp(sc.pws, o0["cov3ds"], sc.shs, sc.cam.Rcw, sc.cam.tcw, sc.cam, O.POLICY_G, o0["us"],
                      o0["dcov2d"], o0["dcolour"], o0["dz"], depths=o0["depths"])
    with pytest.raises(AssertionError):
        assert_pose_close(host(R.grad), host(t.grad), terms0, 1e-4, "plain")


# -------------------------------------------------------------------------------------------------- 5. segment path
def test_segment_path_equals_unsplit_kernels(gsc):
    from easygaussiansplatting_amd import fused
    from easygaussiansplatting_amd.function import Camera
    sc = S.skewed_scene(reset_alpha=True)
    cam = Camera.from_scene(sc.cam)
    Wi = weights(sc, 8)[0]
    prev = fused.SEGMENTS
    img, grads, used = {}, {}, {}
    try:
        for seg in ("0", "1"):
            fused.SEGMENTS = seg
            out, p, us = render(sc, cam, AA())
            used[seg] = out[0].grad_fn.state.seg is not None
            (out[0] * dev(Wi)).sum().backward()
            img[seg] = host(out[0])
            grads[seg] = {k: host(p[k].grad) for k in NAMES}
            grads[seg]["us"] = host(us.grad)
            del out, p, us
    finally:
        fused.SEGMENTS = prev
    assert used == {"0": False, "1": True}
    assert np.abs(img["1"] - img["0"]).max() <= 2e-5
    # the default rule; the two draw paths may flip a pixel or two across the skip threshold (as test_gpu_segments.py
    # allows for plain renders): a few entries of the 4.5 M may sit outside the per-entry bound
    for k in grads["0"]:
        assert_grad_close(grads["1"][k], grads["0"][k], "seg:" + k, outliers=8)


# --------------------------------------------------------------------------------------------------- 6. accumulation
def test_accumulate_two_views_equals_two_passes(gsc):
    from easygaussiansplatting_amd.function import Camera
    sc = scene_256(12)
    cams = [Camera.from_scene(sc.cam), Camera.from_scene(S.ring_cameras(sc.cam, 8, 5.0)[1])]
    Ws = [weights(sc, 4)[0], weights(sc, 5)[0]]
    sep = []
    for v in range(2):
        out, p, _ = render(sc, cams[v], AA())
        (out[0] * dev(Ws[v])).sum().backward()
        sep.append({k: host(p[k].grad) for k in NAMES})
    p = leaves(sc)
    for v in range(2):
        out, _, _ = render(sc, cams[v], AA(accumulate=True), p=p)
        (out[0] * dev(Ws[v])).sum().backward()
    for k in NAMES:
        ref = sep[0][k] + sep[1][k]
        assert np.abs(host(p[k].grad) - ref).max() <= 3e-5 * np.abs(ref).max(), k


def test_sh_sink_equals_plain_backward(gsc):
    from easygaussiansplatting_amd import dist_views as DV
    from easygaussiansplatting_amd.function import Camera
    sc = scene_256(12)
    cam = Camera.from_scene(sc.cam)
    Wi = weights(sc, 6)[0]
    out, p0, _ = render(sc, cam, AA(), raw=True)
    (out[0] * dev(Wi)).sum().backward()
    fx = DV.FactoredShGrad(1)
    p = raw_leaves(sc)
    fx.begin_step(sc.n, "cuda")
    out, _, _ = render(sc, cam, AA(accumulate=True, sh_sink=fx), p=p, raw=True)
    (out[0] * dev(Wi)).sum().backward()
    fx.finish(p["pws"], p["low_shs"], p["high_shs"])
    for k in RAW:
        ref = host(p0[k].grad)
        assert np.abs(host(p[k].grad) - ref).max() <= 3e-5 * np.abs(ref).max(), k


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_exchange_row_chunks_equal_plain_backward(gsc):
    import torch.distributed as dist
    from easygaussiansplatting_amd import dist_views as DV
    from easygaussiansplatting_amd.function import Camera
    sc = scene_256(12)
    cam = Camera.from_scene(sc.cam)
    Wi = weights(sc, 10)[0]
    out, p0, u0 = render(sc, cam, AA())
    (out[0] * dev(Wi)).sum().backward()
    started = False
    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ["MASTER_PORT"] = str(_free_port())
        try:
            dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
        except Exception:
            dist.init_process_group("gloo", rank=0, world_size=1)
        started = True
    try:
        ex = DV.ChunkedExchange(world=1, chunks=4)
        ex.begin_step()
        p = leaves(sc)
        out, _, u1 = render(sc, cam, AA(exchange=ex), p=p)
        (out[0] * dev(Wi)).sum().backward()
        assert ex.used
        assert ex.finish([p[k] for k in NAMES])
        torch.cuda.synchronize()
    finally:
        if started:
            dist.destroy_process_group()
    # (the gradient records carry the draw pass's atomic jitter: equal to the plain backward up to that)
    for k in NAMES:
        ref = host(p0[k].grad)
        assert np.abs(host(p[k].grad) - ref).max() <= 1e-5 * np.abs(ref).max(), k
    assert np.abs(host(u1.grad) - host(u0.grad)).max() <= 1e-5 * np.abs(host(u0.grad)).max()


# ---------------------------------------------------------------------------------------------- 7. the mass identity
def _isolated_subpixel_scene(sig2=(0.15, 0.25), n_side=8, alpha=0.95):
    """n_side^2 Gaussians on a grid 24 px apart, each with a 2D covariance of about sig2 px^2 (undilated)"""
    W = H = 24 * n_side
    f, z = 256.0, 5.0
    ys, xs = np.mgrid[0:n_side, 0:n_side]
    u = np.stack([xs.ravel() * 24 + 12.3, ys.ravel() * 24 + 11.6], 1)
    n = u.shape[0]
    pws = np.concatenate([(u - W / 2.0) * z / f, np.zeros((n, 1))], 1)
    s = np.sqrt(np.asarray(sig2)) * z / f
    scales = np.stack([np.full(n, s[0]), np.full(n, s[1]), np.full(n, 1e-3)], 1)
    th = np.linspace(0, np.pi, n, endpoint=False) / 2
    rots = np.stack([np.cos(th), np.zeros(n), np.zeros(n), np.sin(th)], 1)       # about the view axis
    shs = np.full((n, 3), 0.5)
    cam = S.Camera(W, H, f, f, W / 2.0, H / 2.0, np.eye(3), np.array([0.0, 0.0, z]))
    return S.Scene(pws.astype(np.float32), rots.astype(np.float32), scales.astype(np.float32),
                   np.full(n, alpha, np.float32), shs.astype(np.float32), cam)


def test_alpha_mass_of_isolated_subpixel_gaussians(gsc):
    from easygaussiansplatting_amd.function import Camera, RenderOptions
    sc = _isolated_subpixel_scene()
    cam = Camera.from_scene(sc.cam)
    o = aa_ref.aa_oracle(sc, sc.cam)
    c2 = o["c2"]
    det_sigma = (c2[:, 0] - 0.3) * (c2[:, 2] - 0.3) - c2[:, 1] ** 2
    det_dil = c2[:, 0] * c2[:, 2] - c2[:, 1] ** 2
    assert (c2[:, 0] - 0.3 < 0.5).all() and (c2[:, 2] - 0.3 < 0.5).all()     # sub-pixel
    a = sc.alphas.astype(np.float64)
    out = render(sc, cam, AA(alpha=True))[0]
    plain = render(sc, cam, RenderOptions(alpha=True))[0]
    for amap, want, tol in ((host(out[2])[0], a * 2 * np.pi * np.sqrt(det_sigma), 0.02),
                            (host(plain[2])[0], a * 2 * np.pi * np.sqrt(det_dil), 0.02)):
        cells = amap.reshape(8, 24, 8, 24).sum((1, 3)).reshape(-1)   # one Gaussian per 24 x 24 cell
        assert (np.abs(cells / want - 1) < tol).all(), (cells / want).min()
    cells_plain = host(plain[2])[0].reshape(8, 24, 8, 24).sum((1, 3)).reshape(-1)
    assert (np.abs(cells_plain / (a * 2 * np.pi * np.sqrt(det_sigma)) - 1) > 0.1).all()


# --------------------------------------------------------------------------------------------------- 8. off == plain
def test_default_is_bitwise_the_plain_call(gsc):
    from easygaussiansplatting_amd.function import Camera, GSFunction, RenderOptions
    sc = scene_256()
    cam = Camera.from_scene(sc.cam)
    Wi = weights(sc, 11)[0]
    res = []
    for opts in ("none", RenderOptions(), RenderOptions(antialiased=False)):
        p = leaves(sc)
        us = torch.zeros((sc.n, 2), device="cuda", requires_grad=True)
        args = [p[k] for k in NAMES] + [us, cam]
        out = GSFunction.apply(*args) if opts == "none" else GSFunction.apply(*args, opts)
        assert out[0].grad_fn.state.antialiased is False
        (out[0] * dev(Wi)).sum().backward()
        res.append([out[0], out[1]] + [p[k].grad for k in NAMES] + [us.grad])
    for r in res[1:]:
        assert torch.equal(r[0], res[0][0]) and torch.equal(r[1], res[0][1])     # image and mask: bitwise
        # gradients: the same kernels, up to the atomic jitter of the draw pass's gradient records
        for a, b, k in zip(r[2:], res[0][2:], NAMES + ("us",)):
            assert_grad_close(host(a), host(b), "default:" + k)
    aa = render(sc, cam, AA())[0]
    assert aa[0].grad_fn.state.antialiased is True
    assert float((aa[0] - res[0][0]).detach().abs().max()) > 1e-3


# ---------------------------------------------------------------------------------- 9. 1 M at 1080p, enqueue-ahead
def test_full_size_enqueue_ahead_against_seven_op_kernels(gsc):
    """the bench scene; the second render of the size takes the enqueue-ahead path.  Reference: the seven-op kernels
    drawing alpha comp (comp from their cov2d in float64), the comp term joined to dL/dcov2d, and their chain rule from
    dL/dcov2d on (identity in place of dcinv2d/dcov2d)"""
    from easygaussiansplatting_amd import fused
    from easygaussiansplatting_amd.function import Camera
    sc = S.big_scene()
    cam = Camera.from_scene(sc.cam)
    H, W = sc.cam.height, sc.cam.width
    Wi = weights(sc, 13)[0]
    key = (sc.n, W, H)
    render(sc, cam, AA())                          # first render of the size: synchronous
    assert fused._ctx(torch.device("cuda", 0)).capacity.get(key, 0) > 0
    out, p, us0 = render(sc, cam, AA())
    assert out[0].grad_fn.state.ticket is None     # validated (enqueue-ahead, no redo needed or redone)
    (out[0] * dev(Wi)).sum().backward()
    q = {k: v.detach() for k, v in leaves(sc).items()}
    us, pcs, depths, du = gsc.project(q["pws"], cam.Rcw, cam.tcw, cam.fx, cam.fy, cam.cx, cam.cy, True)
    cov3, dq, ds = gsc.computeCov3D(q["rots"], q["scales"], depths, True)
    cov2, d3, dpc = gsc.computeCov2D(cov3, pcs, cam.Rcw, depths, cam.fx, cam.fy, W, H, True)
    col, dsh, dpw = gsc.sh2Color(q["shs"], q["pws"], cam.twc, True)
    cinv, areas, dci = gsc.inverseCov2D(cov2, depths, True)
    c2 = host(cov2).reshape(-1, 3)
    cm = aa_ref.comp(c2)
    al = host(q["alphas"]).reshape(-1)
    ald = dev(al * cm).reshape(-1, 1)
    img, contrib, tau, ranges, gsid = gsc.splat(H, W, us, cinv, ald, depths, col, areas)
    assert float((img - out[0]).detach().abs().max()) <= 1e-4
    g_us, g_ci, g_al, g_co = gsc.splatB(H, W, us, cinv, ald, depths, col, contrib, tau, ranges, gsid, dev(Wi))
    n = sc.n
    g = host(g_al).reshape(-1)
    dcov2 = (host(g_ci).reshape(n, 1, 3) @ host(dci).reshape(n, 3, 3))[:, 0] + aa_ref.comp_vjp(c2, g * al)
    eye = torch.eye(3, device="cuda").expand(n, 3, 3).contiguous()
    dpws, dshs, dscales, drots = gsc.chain_rule(g_us, dev(dcov2), g_co, cam.Rcw, eye, d3, dq, ds, dsh, du, dpc, dpw)
    ref = dict(pws=host(dpws).reshape(n, 3), shs=host(dshs).reshape(n, -1), alphas=(g * cm)[:, None],
               scales=host(dscales).reshape(n, 3), rots=host(drots).reshape(n, 4))
    for k, v in ref.items():
        assert_grad_close(host(p[k].grad), v, "full:" + k)
    assert_grad_close(host(us0.grad), host(g_us).reshape(-1, 2), "full:us")


# -------------------------------------------------------------------------------------------------------- 10. viewer
def test_viewer_prep_antialiased(gsc):
    from easygaussiansplatting_amd.viewer import gau_prep, pack_gs_data
    from tests.test_gpu_io import _gl_matrices
    sc = S.small_scene(4000, 320, 200, 48, seed=8)
    gs = np.rec.fromarrays([sc.pws, sc.rots, sc.scales, sc.alphas, sc.shs], dtype=S.gsdata_type(48))
    g = pack_gs_data(gs)
    g[:40, 2] += 30.0                                              # some culled rows
    V, Pm, focal = _gl_matrices(320, 200)
    ref, _, culled = IO.viewer_prep(g, V, Pm, focal)
    # restated: comp from the viewer's dilated cov2d (the inverse of its covinv columns)
    ci = ref[:, 3:6]
    with np.errstate(all="ignore"):
        det_ci = ci[:, 0] * ci[:, 2] - ci[:, 1] ** 2
        c2 = np.stack([ci[:, 2] / det_ci, -ci[:, 1] / det_ci, ci[:, 0] / det_ci], 1)
    want = ref.copy()
    want[:, 11] = ref[:, 11] * aa_ref.comp(c2)
    plain, _ = gau_prep(g, V, Pm, focal)
    got, _ = gau_prep(g, V, Pm, focal, antialiased=True)
    got, plain = host(got), host(plain)
    keep = ~culled
    assert keep.sum() > 1000
    assert np.array_equal(got[:, :11], plain[:, :11])
    assert np.abs(got[keep, 11] - want[keep, 11]).max() <= 1e-4
    assert (got[keep, 11] < plain[keep, 11] - 1e-3).any()


# ------------------------------------------------------------------------------------------------------- 11. Trainer
def test_trainer_step_renders_antialiased(gsc, monkeypatch):
    from easygaussiansplatting_amd.function import Camera, GSRawFunction, RenderOptions
    from easygaussiansplatting_amd.trainer import Trainer
    sc = scene_256(12)
    gt = torch.rand((3, 256, 256), device="cuda")
    tr = Trainer(sc, [sc.cam], [gt], max_steps=10, antialiased=True, view_streams=1)
    p = {k: v.detach().clone() for k, v in tr.params.items()}
    seen = []
    orig = GSRawFunction.apply

    def spy(*args):
        seen.append(args[-1])
        out = orig(*args)
        seen.append(out[0].detach().clone())
        return out
    monkeypatch.setattr(GSRawFunction, "apply", spy)
    tr.step([0])
    monkeypatch.undo()
    assert seen[0].antialiased is True
    us = torch.zeros((sc.n, 2), device="cuda")
    want = GSRawFunction.apply(*[p[k] for k in RAW], us, Camera.from_scene(sc.cam), RenderOptions(antialiased=True))[0]
    assert torch.equal(seen[1], want)
