"""Render extras (``RenderOptions(depth=..., alpha=..., background=...)``): the depth and opacity maps and a background
colour of the fused path, against the float64 oracle and against the seven-op kernels.

The oracle needs no new math, blending being linear in the colours: with colours (z_i, 1, 0) ``O.draw`` blends
depth = sum w_i z_i into channel 0 and alpha = sum w_i into channel 1, and the image over a background is the plain image
plus (1 - alpha) bg.  The gradient of <Wi, image> + <Wd, depth> + <Wa, alpha> is ``O.draw_backward`` on the real colours
with dL/dgamma = Wi plus ``O.draw_backward`` on the colours (z, 1, 0) with dL/dgamma = (Wd, Wa - Wi . bg, 0), whose
colour gradient's first column is dL/dz; through ``O.chain_rule`` and dL/dpw += dL/dz Rcw[2, :]."""
import numpy as np
import pytest

from easygaussiansplatting_amd import scene as S
from oracle import gs_oracle as O
from tests.gradcheck import assert_grad_close

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NAMES = ("pws", "shs", "alphas", "scales", "rots")


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
    return t.detach().cpu().numpy()


def scene_256():
    return S.small_scene(10_000, 256, 256, 3, seed=21)


def scene_250x170():
    """250 x 170 (not a multiple of 16) with the principal point moved right: the left tiles stay empty"""
    sc = S.small_scene(4_000, 250, 170, 3, seed=22)
    sc.cam = S.Camera(250, 170, 256.0, 256.0, 250 / 2.0 + 150.0, 85.0, np.eye(3), np.array([0.0, 0.0, 5.0]))
    return sc


SCENES = {"256": scene_256, "250x170": scene_250x170}


def oracle(sc, cam, bg, Wi=None, Wd=None, Wa=None):
    """-> (image over bg, depth, alpha, gradients of <Wi,image> + <Wd,depth> + <Wa,alpha> or None, ranges)"""
    P = O.POLICY_G
    us, pcs, depths, du = O.project(sc.pws, cam.Rcw, cam.tcw, cam.fx, cam.fy, cam.cx, cam.cy, P, True)
    c3, dq, ds = O.compute_cov3d(sc.rots, sc.scales, depths, P, True)
    c2, d3, dpc = O.compute_cov2d(c3, pcs, cam.Rcw, depths, cam.fx, cam.fy, cam.width, cam.height, P, True)
    col, dsh, dpw = O.sh2color(sc.shs, sc.pws, cam.twc, True)
    ci, areas, dci = O.inverse_cov2d(c2, depths, P, True)
    z = depths.copy()
    img, cont, tau, ranges, gsid = O.splat(cam.height, cam.width, us, ci, sc.alphas, depths, col, areas, P)
    zc = np.stack([z, np.ones_like(z), np.zeros_like(z)], 1)
    ez = O.draw(cam.width, cam.height, ranges, gsid, us, ci, sc.alphas, zc, None, P)[0]
    depth, alpha = ez[0], ez[1]
    bgv = np.asarray(bg, np.float64)[:, None, None]
    image = img + (1.0 - alpha)[None] * bgv
    if Wi is None:
        return image, depth, alpha, None, ranges
    g1 = O.draw_backward(cam.width, cam.height, ranges, gsid, us, ci, sc.alphas, col, cont, tau, Wi, None, P)
    dl2 = np.stack([Wd, Wa - (Wi * bgv).sum(0), np.zeros_like(Wd)])
    g2 = O.draw_backward(cam.width, cam.height, ranges, gsid, us, ci, sc.alphas, zc, cont, tau, dl2, None, P)
    dus, dcinv, dal = g1[0] + g2[0], g1[1] + g2[1], g1[2] + g2[2]
    J = dict(dcinv2d_dcov2ds=dci, dcov2d_dcov3ds=d3, dcov3d_drots=dq, dcov3d_dscales=ds, dcolor_dshs=dsh,
             du_dpcs=du, dcov2d_dpcs=dpc, dcolor_dpws=dpw)
    g = O.chain_rule(dus, dcinv, dal, g1[3], cam.Rcw, J)
    dpws = g["dpws"] + g2[3][:, 0:1] * np.asarray(cam.Rcw, np.float64)[2][None, :]
    grads = dict(pws=dpws, shs=g["dshs"], alphas=g["dalphas"][:, None], scales=g["dscales"], rots=g["drots"], us=dus)
    return image, depth, alpha, grads, ranges


def zmax(sc, cam):
    """largest camera-space z of the scene (the depth tolerance is relative to it)"""
    return float((sc.pws.astype(np.float64) @ np.asarray(cam.Rcw).T + np.asarray(cam.tcw))[:, 2].max())


def leaves(sc):
    p = dict(pws=dev(sc.pws), shs=dev(sc.shs), alphas=dev(sc.alphas).reshape(-1, 1), scales=dev(sc.scales),
             rots=dev(sc.rots))
    for v in p.values():
        v.requires_grad_(True)
    return p


def render(sc, cam, opts, p=None):
    from easygaussiansplatting_amd.function import GSFunction
    p = leaves(sc) if p is None else p
    us = torch.zeros((sc.n, 2), device="cuda", requires_grad=True)
    out = GSFunction.apply(*[p[k] for k in NAMES], us, cam, opts)
    return out, p, us


def weights(sc, seed):
    H, W = sc.cam.height, sc.cam.width
    s = 1.0 / (H * W)
    return (S.normal(seed, 1, (3, H, W)) * s, S.normal(seed, 2, (H, W)) * s * 0.2, S.normal(seed, 3, (H, W)) * s)


def empty_pixels(ranges, W, H):
    gx = (W + 15) // 16
    n = ranges[:, 1] - ranges[:, 0]
    m = np.zeros((H, W), bool)
    for t in np.nonzero(n <= 0)[0]:
        ty, tx = divmod(int(t), gx)
        m[16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16] = True
    return m


# ----------------------------------------------------------------------------------------------------- forward parity
@pytest.mark.parametrize("name", list(SCENES))
@pytest.mark.parametrize("bg", [(1.0, 1.0, 1.0), (0.2, 0.5, 0.9)])
def test_forward_parity_vs_oracle(gsc, name, bg):
    from easygaussiansplatting_amd.function import Camera, RenderOptions
    sc = SCENES[name]()
    cam = Camera.from_scene(sc.cam)
    o_img, o_depth, o_alpha, _, o_ranges = oracle(sc, sc.cam, bg)
    (img, mask, depth, alpha), _, _ = render(sc, cam, RenderOptions(depth=True, alpha=True, background=bg))
    assert depth.shape == (1, sc.cam.height, sc.cam.width) and alpha.shape == depth.shape
    assert depth.dtype == torch.float32 and alpha.dtype == torch.float32
    img, depth, alpha = host(img), host(depth)[0], host(alpha)[0]
    assert np.abs(alpha - o_alpha).max() < 1e-4
    assert np.abs(img - o_img).max() < 1e-4
    assert np.abs(depth - o_depth).max() < 1e-4 * zmax(sc, sc.cam)
    empty = empty_pixels(o_ranges, sc.cam.width, sc.cam.height)
    if name == "250x170":
        assert empty.sum() > 1000
    if empty.any():
        assert (depth[empty] == 0).all() and (alpha[empty] == 0).all()
        for c in range(3):
            assert (img[c][empty] == np.float32(bg[c])).all()


# ---------------------------------------------------------------------------------------------- no-op invariance
@pytest.mark.parametrize("name", list(SCENES))
def test_extras_without_background_leave_image_and_grads(gsc, name):
    from easygaussiansplatting_amd.function import Camera, RenderOptions
    sc = SCENES[name]()
    cam = Camera.from_scene(sc.cam)
    Wi, _, _ = weights(sc, 5)
    (img0, mask0), p0, us0 = render(sc, cam, RenderOptions())
    (img1, mask1, depth, alpha), p1, us1 = render(sc, cam, RenderOptions(depth=True, alpha=True))
    assert torch.equal(img0, img1) and torch.equal(mask0, mask1)
    (img0 * dev(Wi)).sum().backward()
    (img1 * dev(Wi)).sum().backward()         # depth and alpha not in the loss: their grads are None
    for k in NAMES:
        assert_grad_close(host(p1[k].grad), host(p0[k].grad), "noop:" + k)
    assert_grad_close(host(us1.grad), host(us0.grad), "noop:us")


# ------------------------------------------------------------------------------------------ gradients vs the oracle
CASES = {"all": (1, 1, 1, (0.2, 0.5, 0.9)), "depth_only": (0, 1, 0, None), "alpha_only": (0, 0, 1, None),
         "background_only": (1, 0, 0, (1.0, 0.4, 0.7))}


@pytest.mark.parametrize("name", list(SCENES))
@pytest.mark.parametrize("case", list(CASES))
def test_gradients_vs_oracle(gsc, name, case):
    from easygaussiansplatting_amd.function import Camera, RenderOptions
    sc = SCENES[name]()
    sc.pws[:30, 2] = -9.0                      # some Gaussians behind the camera (culled)
    cam = Camera.from_scene(sc.cam)
    ui, ud, ua, bg = CASES[case]
    Wi, Wd, Wa = weights(sc, 7)
    Wi, Wd, Wa = Wi * ui, Wd * ud, Wa * ua
    _, _, _, o_g, _ = oracle(sc, sc.cam, bg if bg is not None else (0.0, 0.0, 0.0), Wi, Wd, Wa)
    (img, mask, depth, alpha), p, us = render(sc, cam, RenderOptions(depth=True, alpha=True, background=bg))
    loss = (depth[0] * dev(Wd)).sum() + (alpha[0] * dev(Wa)).sum()
    if ui:
        loss = loss + (img * dev(Wi)).sum()
    loss.backward()
    for k in NAMES:
        g = host(p[k].grad)
        if case in ("depth_only", "alpha_only") and k == "shs":
            assert not g.any()                 # the colours are not in this loss
            continue
        assert_grad_close(g, o_g[k], "%s/%s:%s" % (name, case, k))
    assert_grad_close(host(us.grad), o_g["us"], "%s/%s:us" % (name, case))
    assert not host(p["pws"].grad)[:30].any()


def test_depth_grad_only_when_image_unused(gsc):
    """only the depth map in the loss: the image's gradient is None and the backward pass still runs"""
    from easygaussiansplatting_amd.function import Camera, RenderOptions
    sc = scene_256()
    cam = Camera.from_scene(sc.cam)
    _, Wd, _ = weights(sc, 9)
    _, _, _, o_g, _ = oracle(sc, sc.cam, (0.0, 0.0, 0.0), np.zeros((3,) + Wd.shape), Wd, np.zeros_like(Wd))
    (img, mask, depth), p, us = render(sc, cam, RenderOptions(depth=True))
    (depth[0] * dev(Wd)).sum().backward()
    for k in ("pws", "alphas", "scales", "rots"):
        assert_grad_close(host(p[k].grad), o_g[k], "depth_only_output:" + k)


# ---------------------------------------------------------------------------------------------------- GSRawFunction
def test_raw_function_with_extras_equals_autograd_through_activations(gsc):
    from easygaussiansplatting_amd.function import Camera, GSFunction, GSRawFunction, RenderOptions
    sc = S.small_scene(3000, 144, 112, 12, seed=23)
    cam = Camera.from_scene(sc.cam)
    Wi, Wd, Wa = weights(sc, 11)
    bg = (0.3, 0.6, 0.1)
    opts = RenderOptions(depth=True, alpha=True, background=bg)
    raw = dict(pws=dev(sc.pws), low=dev(sc.shs[:, :3]), high=dev(sc.shs[:, 3:]),
               alphas=dev(np.log(sc.alphas / (1 - sc.alphas))).reshape(-1, 1), scales=dev(np.log(sc.scales)),
               rots=dev(sc.rots * 2.0))
    loss_of = lambda out: (out[0] * dev(Wi)).sum() + (out[2][0] * dev(Wd)).sum() + (out[3][0] * dev(Wa)).sum()
    a = {k: v.clone().requires_grad_(True) for k, v in raw.items()}
    us_a = torch.zeros((sc.n, 2), device="cuda", requires_grad=True)
    out_a = GSRawFunction.apply(a["pws"], a["low"], a["high"], a["alphas"], a["scales"], a["rots"], us_a, cam, opts)
    loss_of(out_a).backward()
    b = {k: v.clone().requires_grad_(True) for k, v in raw.items()}
    us_b = torch.zeros((sc.n, 2), device="cuda", requires_grad=True)
    out_b = GSFunction.apply(b["pws"], torch.cat((b["low"], b["high"]), 1), torch.sigmoid(b["alphas"]),
                             torch.exp(b["scales"]), torch.nn.functional.normalize(b["rots"]), us_b, cam, opts)
    loss_of(out_b).backward()
    # (the activations in torch and in the kernel round differently: alpha' differs in the last bits)
    assert (out_a[0] - out_b[0]).abs().max().item() < 1e-5 and (out_a[3] - out_b[3]).abs().max().item() < 1e-5
    assert (out_a[2] - out_b[2]).abs().max().item() < 1e-5 * zmax(sc, sc.cam)
    for k in raw:
        assert_grad_close(host(a[k].grad), host(b[k].grad), "raw:" + k)
    assert_grad_close(host(us_a.grad), host(us_b.grad), "raw:us")


# -------------------------------------------------------------------------------- full size against the seven ops
def test_full_size_against_seven_op_kernels(gsc):
    from easygaussiansplatting_amd.function import Camera, RenderOptions
    sc = S.big_scene()
    cam = Camera.from_scene(sc.cam)
    H, W = sc.cam.height, sc.cam.width
    _, Wd, Wa = weights(sc, 13)
    (img, mask, depth, alpha), p, us0 = render(sc, cam, RenderOptions(depth=True, alpha=True))
    ((depth[0] * dev(Wd)).sum() + (alpha[0] * dev(Wa)).sum()).backward()
    q = {k: v.detach() for k, v in leaves(sc).items()}
    us, pcs, depths, du = gsc.project(q["pws"], cam.Rcw, cam.tcw, cam.fx, cam.fy, cam.cx, cam.cy, True)
    z = depths.clone()
    cov3, dq, ds = gsc.computeCov3D(q["rots"], q["scales"], depths, True)
    cov2, d3, dpc = gsc.computeCov2D(cov3, pcs, cam.Rcw, depths, cam.fx, cam.fy, W, H, True)
    col, dsh, dpw = gsc.sh2Color(q["shs"], q["pws"], cam.twc, True)
    cinv, areas, dci = gsc.inverseCov2D(cov2, depths, True)
    zc = torch.stack([z, torch.ones_like(z), torch.zeros_like(z)], 1).contiguous()
    ez, contrib, tau, ranges, gsid = gsc.splat(H, W, us, cinv, q["alphas"], depths, zc, areas)
    scale = float(z[depths > 0.2].max())
    assert (depth[0] - ez[0]).abs().max().item() <= 1e-4 * scale
    assert (alpha[0] - ez[1]).abs().max().item() <= 1e-4
    dl = torch.stack([dev(Wd), dev(Wa), torch.zeros_like(dev(Wd))]).contiguous()
    g_us, g_ci, g_al, g_co = gsc.splatB(H, W, us, cinv, q["alphas"], depths, zc, contrib, tau, ranges, gsid, dl)
    dpws, dshs, dscales, drots = gsc.chain_rule(g_us, g_ci, torch.zeros_like(g_co), cam.Rcw, dci, d3, dq, ds, dsh, du,
                                                dpc, dpw)
    n = sc.n
    dpws = dpws.reshape(n, 3) + g_co.reshape(n, 3)[:, 0:1] * cam.Rcw[2][None, :]
    ref = dict(pws=dpws, alphas=g_al.reshape(n, 1), scales=dscales.reshape(n, 3), rots=drots.reshape(n, 4))
    for k, v in ref.items():
        assert_grad_close(host(p[k].grad), host(v), "full:" + k)
    assert_grad_close(host(us0.grad), host(g_us).reshape(-1, 2), "full:us")


# ------------------------------------------------------------------------------------ enqueue-ahead and the redo
def test_enqueue_ahead_and_overflow_redo(gsc):
    from easygaussiansplatting_amd import fused
    from easygaussiansplatting_amd.function import Camera, RenderOptions
    sc = S.small_scene(6000, 200, 152, 3, seed=24)
    bg = (0.1, 0.8, 0.4)
    opts = RenderOptions(depth=True, alpha=True, background=bg)
    o_img, o_depth, o_alpha, _, _ = oracle(sc, sc.cam, bg)
    cam = Camera.from_scene(sc.cam)
    key = (sc.n, sc.cam.width, sc.cam.height)
    for _ in range(2):                          # first render of the size, then the enqueue-ahead one
        (img, mask, depth, alpha), _, _ = render(sc, cam, opts)
        assert np.abs(host(img) - o_img).max() < 1e-4 and np.abs(host(alpha)[0] - o_alpha).max() < 1e-4
        assert np.abs(host(depth)[0] - o_depth).max() < 1e-4 * zmax(sc, sc.cam)
    ctx = fused._ctx(torch.device("cuda", torch.cuda.current_device()))
    cap0 = ctx.capacity[key]
    # the same problem size (N, W, H) with four times the scales: many more patches than the learnt capacity
    big = S.Scene(sc.pws, sc.rots, sc.scales * 4.0, sc.alphas, sc.shs, sc.cam)
    n_img, n_depth, n_alpha, _, n_ranges = oracle(big, big.cam, bg)
    assert int((n_ranges[:, 1] - n_ranges[:, 0]).sum()) > cap0   # the enqueue-ahead render overflows: the redo runs
    (img, mask, depth, alpha), _, _ = render(big, cam, opts)
    assert ctx.capacity[key] > cap0
    assert np.abs(host(img) - n_img).max() < 1e-4 and np.abs(host(alpha)[0] - n_alpha).max() < 1e-4
    assert np.abs(host(depth)[0] - n_depth).max() < 1e-4 * zmax(big, big.cam)


# -------------------------------------------------------------------------------------------------------- long lists
def test_long_lists_take_the_unsplit_kernels(gsc):
    from easygaussiansplatting_amd import fused
    from easygaussiansplatting_amd.function import Camera
    sc = S.skewed_scene(reset_alpha=True)
    cam = Camera.from_scene(sc.cam)
    H, W = sc.cam.height, sc.cam.width
    q = {k: v.detach() for k, v in leaves(sc).items()}
    args = (q["pws"], q["shs"], q["alphas"], q["scales"], q["rots"], cam)
    prev = fused.SEGMENTS
    fused.SEGMENTS = "1"
    try:
        img_seg, _, st_seg = fused.forward(*args)
        assert st_seg.seg is not None
        img, _, st, depth, alpha = fused.forward(*args, extras=fused.Extras(True, True, None))
    finally:
        fused.SEGMENTS = prev
    assert st.seg is None
    rg = host(st.ranges)
    lens = rg[:, 1] - rg[:, 0]
    top = np.argsort(-lens, kind="stable")[:16]
    assert lens[top[-1]] > 2048
    # the oracle's blend over the device's own (culled) lists, on the device's float32 2D Gaussians
    P = O.POLICY_G
    f32 = np.float32
    us, pcs, dz = O.project(sc.pws, sc.cam.Rcw, sc.cam.tcw, sc.cam.fx, sc.cam.fy, sc.cam.cx, sc.cam.cy, P, False, f32)
    c3 = O.compute_cov3d(sc.rots, sc.scales, dz, P, False, f32)
    c2 = O.compute_cov2d(c3, pcs, sc.cam.Rcw, dz, sc.cam.fx, sc.cam.fy, W, H, P, False, f32)
    ci, _ = O.inverse_cov2d(c2, dz.copy(), P, False, f32)
    z = host(st.depths).astype(np.float64)
    zc = np.stack([z, np.ones_like(z), np.zeros_like(z)], 1)
    ez = O.draw(W, H, rg, host(st.gaussian_ids()), np.float64(us), np.float64(ci), sc.alphas, zc, None, P,
                tiles=top)[0]
    gx = (W + 15) // 16
    for t in top:
        ty, tx = divmod(int(t), gx)
        win = (slice(16 * ty, min(16 * ty + 16, H)), slice(16 * tx, min(16 * tx + 16, W)))
        assert np.abs(host(alpha)[0][win] - ez[1][win]).max() < 1e-4, t
        assert np.abs(host(depth)[0][win] - ez[0][win]).max() < 1e-4 * z.max(), t
    d = np.abs(host(img) - host(img_seg)).max(0)
    flip = host(st.contrib) != host(st_seg.contrib)
    assert flip.sum() <= 8 and d[~flip].max() < 2e-5 and d.max() < 2e-3


# ------------------------------------------------------------------------------------------------------- composition
def test_accumulate_over_two_views_equals_separate_passes(gsc):
    from easygaussiansplatting_amd.function import Camera, GSFunction, RenderOptions
    sc = S.small_scene(4000, 160, 128, 3, seed=25)
    cams = [Camera.from_scene(sc.cam),
            Camera.from_scene(S.Camera(160, 128, 256.0, 256.0, 80.0, 64.0, np.eye(3), np.array([0.3, -0.2, 5.5])))]
    Wi, Wd, Wa = weights(sc, 17)
    bg = (0.5, 0.5, 1.0)

    def run(acc):
        p = leaves(sc)
        us = torch.zeros((sc.n, 2), device="cuda", requires_grad=True)
        for c in cams:
            o = RenderOptions(accumulate=acc, depth=True, alpha=True, background=bg)
            img, _, depth, alpha = GSFunction.apply(*[p[k] for k in NAMES], us, c, o)
            ((img * dev(Wi)).sum() + (depth[0] * dev(Wd)).sum() + (alpha[0] * dev(Wa)).sum()).backward()
        return {k: host(p[k].grad) for k in NAMES}

    ref, got = run(False), run(True)
    for k in NAMES:
        assert np.abs(got[k] - ref[k]).max() <= 3e-5 * np.abs(ref[k]).max(), k
