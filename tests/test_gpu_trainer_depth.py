"""``Trainer(depth_priors=...)``: the gradients of a step are those of a manual composition of the render
with its depth and opacity maps, the two fused losses and one backward pass; a view without a prior trains as in a
trainer without the option; the depth term's weight follows its schedule; ``last_depth_loss`` is the kernel's value; the
option refuses what it cannot do and runs beside the others.

Scene, cameras and the trainers' start are those of tests/test_gpu_trainer_weights.py.  The priors are the disparity
alpha / depth of a render of the UNPERTURBED scene under a scale, a shift and a smooth distortion across the image (the
trainers start from brighter colours, which the depth term does not see, so without the distortion "affine" and "pearson"
would fit the prior exactly)."""
import numpy as np
import pytest

from easygaussiansplatting_amd import scene as S
from tests.gradcheck import assert_grad_close
from tests.test_gpu_trainer_weights import GRAD_KEYS, H, N, W, host, run, trainer

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def setup():
    """small_scene seen from three ring cameras -> (cameras, photographs, priors): renders of the scene itself"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from easygaussiansplatting_amd import gsplatcu
    from easygaussiansplatting_amd.function import Camera, GSFunction, RenderOptions
    gsplatcu.set_policy("gsplatcu")
    sc = S.small_scene(N, W, H, 48)
    cams = [Camera.from_scene(c) for c in S.ring_cameras(sc.cam, 3, radius=5.0)]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    gts, priors = [], []
    with torch.no_grad():
        leaves = (dev(sc.pws), dev(sc.shs), dev(sc.alphas).reshape(-1, 1), dev(sc.scales), dev(sc.rots))
        for c in cams:
            image, _, depth, alpha = GSFunction.apply(*leaves, torch.zeros((N, 2), device="cuda"), c,
                                                      RenderOptions(depth=True, alpha=True))
            gts.append(image.contiguous())
            q = torch.where(alpha[0] > 0.05, alpha[0] / depth[0].clamp_min(1e-6), torch.zeros_like(alpha[0]))
            # (a smooth distortion on top: a prior that is an affine image of the render has no "pearson" gradient)
            wave = 1.0 + 0.2 * torch.sin(torch.arange(W, device="cuda") / 9.0)[None, :]
            priors.append((torch.where(q > 0, wave * (q - 0.01) / 2.5, q)).clamp_min(0).contiguous())
    assert all(float((q > 0).float().mean()) > 0.2 for q in priors)
    return cams, gts, priors


def manual_step(tr_params, cams, gts, priors, views, kind, weight, keys):
    """the step's gradients by plain autograd: GSRawFunction with the maps, the two fused losses, one backward per view"""
    from easygaussiansplatting_amd.depthloss import depth_loss_with_grad
    from easygaussiansplatting_amd.function import GSRawFunction, RenderOptions
    from easygaussiansplatting_amd.loss import gau_loss_with_grad
    leaves = [p.clone().requires_grad_(True) for p in tr_params]
    depth_terms = []
    for v in views:
        us = torch.zeros((leaves[0].shape[0], 2), device="cuda", requires_grad=True)
        has = priors[v] is not None
        out = GSRawFunction.apply(*leaves, us, cams[v], RenderOptions(depth=has, alpha=has))
        _, dimage = gau_loss_with_grad(out[0].detach(), gts[v], grad_scale=1.0 / len(views))
        if has:
            st, dD, dA = depth_loss_with_grad(out[2].detach(), out[3].detach(), priors[v], kind,
                                              grad_scale=weight / len(views))
            depth_terms.append(st[0])
            torch.autograd.backward([out[0], out[2], out[3]], [dimage, dD, dA])
        else:
            out[0].backward(dimage)
    return dict(zip(keys, (p.grad for p in leaves))), depth_terms


@pytest.mark.parametrize("kind", ["affine", "metric", "pearson"])
@pytest.mark.parametrize("views,factored", [([1], True), ([0, 1, 2], True), ([2, 0], False)],
                         ids=["one-view", "three-views", "two-views-flat-sh"])
def test_step_gradients_are_those_of_the_manual_composition(setup, views, factored, kind):
    cams, gts, priors = setup
    priors = [None, priors[1], priors[2]]          # (view 0 has none: the accumulate path mixes both sorts of view)
    tr = trainer(cams, gts, depth_priors=priors, depth_kind=kind, depth_weight=0.5, factored_sh=factored)
    before = [tr.params[k].detach().clone() for k in tr._KEYS]
    tr.step(list(views))
    want, terms = manual_step(before, cams, gts, priors, views, kind, 0.5, tr._KEYS)
    for k in tr._KEYS if not factored else GRAD_KEYS:
        assert tr.params[k].grad is not None, k
        assert_grad_close(host(tr.params[k].grad), host(want[k]), "%s %s %s" % (kind, views, k), outliers=0)
    # the depth term moved the gradients: they are not those of the image loss alone
    plain, _ = manual_step(before, cams, gts, [None] * 3, views, kind, 0.5, tr._KEYS)
    assert float((plain["pws"] - want["pws"]).abs().max()) > 1e-2 * float(want["pws"].abs().max())
    got = float(tr.last_depth_loss)
    assert abs(got - float(sum(terms)) / len(terms)) <= 1e-6 * max(1.0, abs(got))


def test_a_view_without_a_prior_trains_as_without_the_option(setup, monkeypatch):
    """Views 0 and 2 of a trainer whose view 1 has a prior, against a trainer without the option: the renders ask for no
    map, the depth loss is never called, and the loss of the first step is the same bits.  The gradients are summed with
    float atomics and differ in their last bits between any two runs (the control pair of
    tests/test_gpu_trainer_weights.py): they are held to the relative rule of tests/gradcheck.py, the losses of the later
    steps to 1e-5 of the loss."""
    from easygaussiansplatting_amd import trainer as T
    from easygaussiansplatting_amd.depthloss import depth_loss_with_grad
    cams, gts, priors = setup
    steps = ([0], [2], [2, 0])
    plain = run(trainer(cams, gts), steps=steps)
    seen = []
    real = T.GSRawFunction

    class Recording:
        @staticmethod
        def apply(*args):
            seen.append(args[-1])           # (the RenderOptions of the call)
            return real.apply(*args)

    def refuse(*a, **kw):
        pytest.fail("the depth loss ran for a view without a prior")

    tr = trainer(cams, gts, depth_priors=[None, priors[1], None])
    tr._depth_loss_with_grad = refuse
    monkeypatch.setattr(T, "GSRawFunction", Recording)
    got = run(tr, steps=steps)
    assert len(seen) == 4 and not any(o.has_extras() for o in seen)
    # (the first step starts from the same parameters; the later ones from parameters that carry the atomics' jitter of
    # the earlier gradients through Adam's normalised step)
    assert got[0][0] == plain[0][0] and np.abs(got[0] - plain[0]).max() <= 1e-5 * plain[0].max(), (got[0], plain[0])
    for ga, gb in zip(got[1], plain[1]):
        for k in GRAD_KEYS:
            assert_grad_close(host(ga[k]), host(gb[k]), "a view without a prior: " + k, outliers=0)
    assert float(tr.last_depth_loss) == 0.0
    # and view 1 does ask for both maps
    del seen[:]
    tr._depth_loss_with_grad = depth_loss_with_grad
    tr.step([1, 0])
    assert [(o.depth, o.alpha) for o in seen] == [(True, True), (False, False)]
    assert float(tr.last_depth_loss) > 0.0


def test_default_trainer_loads_no_library(setup, monkeypatch):
    from easygaussiansplatting_amd import _depthlosslib
    cams, gts, _ = setup
    monkeypatch.setattr(_depthlosslib, "_lib", None)
    monkeypatch.setattr(_depthlosslib, "load", lambda: pytest.fail("libegs_depthloss.so was loaded"))
    tr = trainer(cams, gts)
    assert tr.depth_priors is None and tr.last_depth_loss is None
    assert np.isfinite(tr.step([1])) and np.isfinite(tr.step([0, 2]))
    assert tr.last_depth_loss is None and tr._depth_sum is None and _depthlosslib._lib is None


def test_weight_schedule_and_last_depth_loss(setup):
    from easygaussiansplatting_amd.depthloss import depth_loss_with_grad
    cams, gts, priors = setup
    g = torch.Generator(device="cuda").manual_seed(3)
    weights = [None, 2.0 * torch.rand((H, W), device="cuda", generator=g), None]
    tr = trainer(cams, gts, depth_priors=priors, pixel_weights=weights, depth_alpha_min=0.1)      # max_steps = 10
    calls = []

    def spy(depth, alpha, prior, kind, **kw):
        out = depth_loss_with_grad(depth, alpha, prior, kind, **kw)
        calls.append((depth.clone(), alpha.clone(), prior, kind, kw, out[0].clone()))
        return out

    tr._depth_loss_with_grad = spy
    for it, want in ((0, 1.0), (5, 0.1), (10, 0.01)):
        assert abs(tr.depth_weight_at(it) - want) <= 1e-12
        tr.iteration = it
        del calls[:]
        views = [1, 2]
        loss = tr.step(views, sync=False)
        assert isinstance(loss, torch.Tensor) and isinstance(tr.last_depth_loss, torch.Tensor) and tr.iteration == it + 1
        assert [c[2] is tr.depth_priors[v] for c, v in zip(calls, views)] == [True, True]
        for (depth, alpha, prior, kind, kw, stats), v in zip(calls, views):
            assert kind == "affine" and kw["alpha_min"] == 0.1 and abs(kw["grad_scale"] - want / 2) <= 1e-12
            assert kw["weight"] is tr.pixel_weights[v] and tuple(depth.shape) == (1, H, W) == tuple(alpha.shape)
            # the direct call on the maps the step rendered: the same kernel, the same bits
            again, _, _ = depth_loss_with_grad(depth, alpha, prior, kind, weight=kw["weight"], alpha_min=0.1,
                                               need_grad=False)
            assert torch.equal(again.view(torch.int32), stats.view(torch.int32))
        assert float(tr.last_depth_loss) == float((calls[0][5][0] + calls[1][5][0]) / 2)
        assert 0.0 < float(tr.last_depth_loss) < 1.0
    # a constant weight
    tr = trainer(cams, gts, depth_priors=priors, depth_weight=0.25)
    assert tr.depth_weight_at(0) == tr.depth_weight_at(7) == 0.25


def test_refusals(setup):
    cams, gts, priors = setup
    with pytest.raises(ValueError, match="absgrad"):
        trainer(cams, gts, depth_priors=priors, absgrad=True)
    with pytest.raises(ValueError, match="needs mode='fused'"):
        trainer(cams, gts, depth_priors=priors, mode="ops", fused_activations=False)
    with pytest.raises(ValueError, match="view 2 has shape"):
        trainer(cams, gts, depth_priors=[priors[0], None, priors[2][:, :-1]])
    with pytest.raises(ValueError, match="view 0 has no positive finite pixel"):
        trainer(cams, gts, depth_priors=[torch.zeros((H, W), device="cuda"), None, None])
    with pytest.raises(ValueError, match="depth_kind"):
        trainer(cams, gts, depth_priors=priors, depth_kind="huber")


@pytest.mark.parametrize("kw", [dict(bilagrid=True, bilagrid_shape=(6, 5, 4)), dict(sparse_adam=True),
                                dict(pose_opt=True), dict(strategy="mcmc", cap_max=3000), dict(view_streams=2),
                                dict(fused_activations=False), dict(antialiased=True), dict(fused_adam=False)],
                         ids=["bilagrid", "sparse_adam", "pose_opt", "mcmc", "two-streams", "torch-activations",
                              "antialiased", "torch-adam"])
def test_it_works_with_the_other_options(setup, kw):
    cams, gts, priors = setup
    tr = trainer(cams, gts, depth_priors=[priors[0], None, priors[2]], depth_kind="pearson", **kw)
    for views in ([0, 1], [2, 1, 0]):
        assert np.isfinite(tr.step(views)), views
        assert 0.0 <= float(tr.last_depth_loss) < 1.0
    for k in tr._KEYS:
        assert bool(torch.isfinite(tr.params[k]).all()), k
