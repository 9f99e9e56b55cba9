"""``Trainer(normal_priors=..., normal_smooth=...)``: the per-Gaussian gradients of a step are those of a
plain-autograd torch composition of the DEFINITION (tests/normal_loss_ref.py, float64, on the maps the render produced)
under the rule of tests/gradcheck.py; a view without a normal term trains as in a trainer without the options, which
never loads the library; ``last_normal_loss`` holds the two terms; the options refuse what they cannot do and run beside
the others.

Scene, cameras and the trainers' start are those of tests/test_gpu_trainer_weights.py.  The priors are the normals of a
render of the UNPERTURBED scene, tilted smoothly across the image (the trainers start from the same geometry, and a prior
that equals the rendered normal has no gradient)."""
import numpy as np
import pytest

from easygaussiansplatting_amd import scene as S
from tests import normal_loss_ref as NR
from tests.gradcheck import assert_grad_close
from tests.test_gpu_trainer_weights import GRAD_KEYS, H, N, W, host, run, trainer

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def setup():
    """small_scene seen from three ring cameras -> (cameras, photographs, normal priors, depth priors)"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from easygaussiansplatting_amd import gsplatcu
    from easygaussiansplatting_amd.function import Camera, GSFunction, RenderOptions
    from easygaussiansplatting_amd.normalloss import depth_to_normals
    gsplatcu.set_policy("gsplatcu")
    sc = S.small_scene(N, W, H, 48)
    cams = [Camera.from_scene(c) for c in S.ring_cameras(sc.cam, 3, radius=5.0)]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    gts, normals, depths = [], [], []
    xs = torch.arange(W, device="cuda")[None, :].expand(H, W)
    ys = torch.arange(H, device="cuda")[:, None].expand(H, W)
    tilt = 0.3 * torch.stack([torch.sin(xs / 9.0), torch.cos(ys / 7.0), torch.zeros((H, W), device="cuda")])
    with torch.no_grad():
        leaves = (dev(sc.pws), dev(sc.shs), dev(sc.alphas).reshape(-1, 1), dev(sc.scales), dev(sc.rots))
        for c in cams:
            image, _, depth, alpha = GSFunction.apply(*leaves, torch.zeros((N, 2), device="cuda"), c,
                                                      RenderOptions(depth=True, alpha=True))
            gts.append(image.contiguous())
            n = depth_to_normals(depth, alpha, c)
            has = (n != 0).any(0)
            normals.append(torch.where(has, n + tilt, torch.zeros_like(n)).contiguous())      # (normalised by the loss)
            q = torch.where(alpha[0] > 0.05, alpha[0] / depth[0].clamp_min(1e-6), torch.zeros_like(alpha[0]))
            depths.append((torch.where(q > 0, (1.0 + 0.2 * torch.sin(xs / 9.0)) * (q - 0.01) / 2.5, q)).clamp_min(0)
                          .contiguous())
    assert all(float((q != 0).any(0).float().mean()) > 0.2 for q in normals)
    return cams, gts, normals, depths


def manual_step(tr_params, cams, gts, normals, views, weight, smooth, keys, depths=None, depth_weight=0.0):
    """the step's gradients by plain autograd: GSRawFunction with the maps, the fused image loss, the normal terms as a
    float64 torch composition of the definition on the maps (and the fused depth term), one backward per view"""
    from easygaussiansplatting_amd.depthloss import depth_loss_with_grad
    from easygaussiansplatting_amd.function import GSRawFunction, RenderOptions
    from easygaussiansplatting_amd.loss import gau_loss_with_grad
    leaves = [p.clone().requires_grad_(True) for p in tr_params]
    terms = []
    for v in views:
        us = torch.zeros((leaves[0].shape[0], 2), device="cuda", requires_grad=True)
        with_n = normals[v] is not None or smooth > 0
        with_d = depths is not None and depths[v] is not None
        out = GSRawFunction.apply(*leaves, us, cams[v], RenderOptions(depth=with_n or with_d, alpha=with_n or with_d))
        _, dimage = gau_loss_with_grad(out[0].detach(), gts[v], grad_scale=1.0 / len(views))
        roots, grads = [out[0]], [dimage]
        if with_d:
            _, dD, dA = depth_loss_with_grad(out[2].detach(), out[3].detach(), depths[v], "affine",
                                             grad_scale=depth_weight / len(views))
            roots += [out[2], out[3]]
            grads += [dD, dA]
        if with_n:
            cam = (cams[v].fx, cams[v].fy, cams[v].cx, cams[v].cy)
            o = NR.forward(out[2][0].double(), out[3][0].double(), cam,
                           None if normals[v] is None else normals[v].double(), gts[v].double(), None, smooth > 0)
            total = (weight * o["Lp"] + smooth * o["Ls"]) / len(views)
            terms.append((float(o["Lp"].detach()) if normals[v] is not None else None, float(o["Ls"].detach())))
            if total.requires_grad:
                roots.append(total)
                grads.append(torch.ones((), dtype=torch.float64, device="cuda"))
        torch.autograd.backward(roots, grads)
    return dict(zip(keys, (p.grad for p in leaves))), terms


CASES = {
    "one-view": dict(views=[1], priors=(0, 1, 2), weight=0.5, smooth=0.0),
    "three-views-one-without": dict(views=[0, 1, 2], priors=(1, 2), weight=0.5, smooth=0.3),
    "smoothness-only": dict(views=[2, 0], priors=None, weight=0.5, smooth=0.4),
    "with-depth-priors": dict(views=[1, 0], priors=(0, 1), weight=0.5, smooth=0.3, depth=True),
}


@pytest.mark.parametrize("case", list(CASES))
def test_step_gradients_are_those_of_the_definition(setup, case):
    cams, gts, normals, depths = setup
    c = CASES[case]
    nq = None if c["priors"] is None else [normals[v] if v in c["priors"] else None for v in range(3)]
    kw = dict(normal_priors=nq, normal_weight=c["weight"], normal_smooth=c["smooth"])
    dq = None
    if c.get("depth"):
        dq = [None, depths[1], depths[2]]
        kw.update(depth_priors=dq, depth_kind="affine", depth_weight=0.5)
    tr = trainer(cams, gts, **kw)
    before = [tr.params[k].detach().clone() for k in tr._KEYS]
    tr.step(list(c["views"]))
    nn = nq if nq is not None else [None] * 3
    want, terms = manual_step(before, cams, gts, nn, c["views"], c["weight"], c["smooth"], tr._KEYS, dq, 0.5)
    for k in GRAD_KEYS:
        assert tr.params[k].grad is not None, k
        assert_grad_close(host(tr.params[k].grad), host(want[k]), "%s %s" % (case, k), outliers=0)
    # the normal terms moved the gradients: they are not those of the step without them
    plain, _ = manual_step(before, cams, gts, [None] * 3, c["views"], 0.0, 0.0, tr._KEYS, dq, 0.5)
    assert float((plain["pws"] - want["pws"]).abs().max()) > 1e-2 * float(want["pws"].abs().max())
    lp = [t[0] for t in terms if t[0] is not None]
    got = tr.last_normal_loss.tolist()
    assert abs(got[0] - (sum(lp) / len(lp) if lp else 0.0)) <= 1e-5
    assert abs(got[1] - sum(t[1] for t in terms) / len(c["views"])) <= 1e-5
    assert (got[0] > 0) == bool(lp) and (got[1] > 0) == (c["smooth"] > 0)


def test_without_the_arguments_nothing_is_loaded_and_a_view_without_a_term_renders_as_before(setup, monkeypatch):
    """A default trainer never calls ``_normallosslib.load``; and the views without a prior of a trainer that has one
    elsewhere ask for no map, never reach the normal loss, and give the default trainer's first loss bit for bit (the
    gradients are summed with float atomics: they are held to the rule of tests/gradcheck.py)."""
    from easygaussiansplatting_amd import _normallosslib
    from easygaussiansplatting_amd import trainer as T
    cams, gts, normals, _ = setup
    steps = ([0], [2], [2, 0])
    with monkeypatch.context() as m:
        m.setattr(_normallosslib, "_lib", None)
        m.setattr(_normallosslib, "load", lambda: pytest.fail("libegs_normalloss.so was loaded"))
        tr0 = trainer(cams, gts)
        assert tr0.normal_priors is None and not tr0.normals_on and tr0.last_normal_loss is None
        plain = run(tr0, steps=steps)
        assert tr0.last_normal_loss is None and tr0._normal_sum is None and _normallosslib._lib is None
    seen = []
    real = T.GSRawFunction

    class Recording:
        @staticmethod
        def apply(*args):
            seen.append(args[-1])           # (the RenderOptions of the call)
            return real.apply(*args)

    tr = trainer(cams, gts, normal_priors=[None, normals[1], None])
    tr._normal_loss_with_grad = lambda *a, **kw: pytest.fail("the normal loss ran for a view without a term")
    monkeypatch.setattr(T, "GSRawFunction", Recording)
    got = run(tr, steps=steps)
    assert len(seen) == 4 and not any(o.has_extras() for o in seen)
    assert got[0][0] == plain[0][0] and np.abs(got[0] - plain[0]).max() <= 1e-5 * plain[0].max(), (got[0], plain[0])
    for ga, gb in zip(got[1], plain[1]):
        for k in GRAD_KEYS:
            assert_grad_close(host(ga[k]), host(gb[k]), "a view without a term: " + k, outliers=0)
    assert tr.last_normal_loss.tolist() == [0.0, 0.0]


def test_what_the_step_hands_to_the_loss(setup):
    from easygaussiansplatting_amd.normalloss import normal_loss_with_grad
    cams, gts, normals, _ = setup
    g = torch.Generator(device="cuda").manual_seed(3)
    weights = [None, 2.0 * torch.rand((H, W), device="cuda", generator=g), None]
    tr = trainer(cams, gts, normal_priors=[None, normals[1], normals[2]], pixel_weights=weights, normal_weight=0.25,
                 normal_smooth=0.5, normal_alpha_min=0.1, normal_edge_gamma=4.0)
    calls = []

    def spy(depth, alpha, cam, **kw):
        out = normal_loss_with_grad(depth, alpha, cam, **kw)
        calls.append((cam, kw, out[0].clone()))
        return out

    tr._normal_loss_with_grad = spy
    views = [0, 1]
    tr.step(views)
    assert len(calls) == 2
    for (cam, kw, stats), v in zip(calls, views):
        assert cam is tr.cams[v] and kw["guide"] is tr.gts[v] and kw["weight"] is tr.pixel_weights[v]
        assert kw["normals"] is tr.normal_priors[v] and kw["smooth"] is True
        assert (kw["alpha_min"], kw["edge_gamma"], kw["prior_scale"], kw["smooth_scale"]) == (0.1, 4.0, 0.125, 0.25)
    got = tr.last_normal_loss.tolist()
    assert got[0] == float(calls[1][2][0]) and abs(got[1] - float(calls[0][2][1] + calls[1][2][1]) / 2) <= 1e-7
    assert float(calls[0][2][2]) == 0 and float(calls[1][2][2]) > 0       # (Omega_p: view 0 has no prior)


def test_refusals(setup):
    cams, gts, normals, _ = setup
    with pytest.raises(ValueError, match=r"Trainer\(normal_priors=\.\.\.\) with absgrad=True"):
        trainer(cams, gts, normal_priors=normals, absgrad=True)
    with pytest.raises(ValueError, match=r"Trainer\(normal_priors=\.\.\.\) needs mode='fused'"):
        trainer(cams, gts, normal_priors=normals, mode="ops", fused_activations=False)
    with pytest.raises(ValueError, match="absgrad"):
        trainer(cams, gts, normal_smooth=0.1, absgrad=True)
    with pytest.raises(ValueError, match="needs mode='fused'"):
        trainer(cams, gts, normal_smooth=0.1, mode="ops", fused_activations=False)
    with pytest.raises(ValueError, match="view 2 has shape"):
        trainer(cams, gts, normal_priors=[normals[0], None, normals[2][:, :, :-1]])
    with pytest.raises(ValueError, match="view 0 has no pixel with data"):
        trainer(cams, gts, normal_priors=[torch.zeros((3, H, W), device="cuda"), None, None])


@pytest.mark.parametrize("kw", [dict(bilagrid=True, bilagrid_shape=(6, 5, 4)), dict(sparse_adam=True),
                                dict(pose_opt=True), dict(strategy="mcmc", cap_max=3000), dict(view_streams=2),
                                dict(fused_activations=False), dict(antialiased=True)],
                         ids=["bilagrid", "sparse_adam", "pose_opt", "mcmc", "two-streams", "torch-activations",
                              "antialiased"])
def test_it_works_with_the_other_options(setup, kw):
    cams, gts, normals, depths = setup
    tr = trainer(cams, gts, normal_priors=[normals[0], None, normals[2]], normal_smooth=0.2,
                 depth_priors=[None, depths[1], depths[2]], **kw)
    for views in ([0, 1], [2, 1, 0]):
        assert np.isfinite(tr.step(views)), views
        lp, ls = tr.last_normal_loss.tolist()
        assert 0.0 < lp < 2.0 and 0.0 < ls < 2.0
    for k in tr._KEYS:
        assert bool(torch.isfinite(tr.params[k]).all()), k
