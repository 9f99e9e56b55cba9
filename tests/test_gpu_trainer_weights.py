"""``Trainer(pixel_weights=...)``: the default trainer never touches libegs_wloss.so, all-ones weights
train as no weights do, a masked-out corruption of a photograph leaves no trace in the step, the gradient handed to the
render is the weighted loss kernel's, and the option runs beside every other one.

Scene and cameras are those of tests/test_gpu_trainer_bilagrid.py.  The render's backward pass sums with float atomics,
so two identical trainers need not agree to the bit: a CONTROL PAIR of unweighted trainers measures by how much they
differ, and what should be equal is held to that: to the bit where the control pair agrees to the bit, within twice its
spread otherwise.  The spread of the losses is their largest absolute difference over the three steps.  The spread of the
parameter gradients is ONE number: max|Ga - Gb| / max|Ga|, the jitter in units of the tensor's largest entry (the measure
of tests/test_gpu_determinism.py), the largest over the four gradient tensors and the three steps.  One tensor of one
step is no estimate: the differences are last-bit flips of single entries, their largest is the ulp of whichever large
entry happened to flip, and between two pairs of runs that moved by more than two (4.7e-10 against 1.9e-10 in
scales_raw, and 4.4e-8 against 2.2e-8 in its relative 2-norm, were seen with nothing but the atomics' order between
them).  Relative, because a view's gradient scales with the view and with H W / sum w."""
import numpy as np
import pytest

from easygaussiansplatting_amd import scene as S
from tests.gradcheck import assert_grad_close

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N, W, H = 2000, 128, 96
STEPS = ([0], [1], [2])
GRAD_KEYS = ("pws", "alphas_raw", "scales_raw", "rots_raw")     # (the SH gradient of a step stays factored)


@pytest.fixture(scope="module")
def setup():
    """small_scene seen from three ring cameras; the photographs are the scene's own renders"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from easygaussiansplatting_amd import gsplatcu
    from easygaussiansplatting_amd.function import Camera, render
    gsplatcu.set_policy("gsplatcu")
    sc = S.small_scene(N, W, H, 48)
    cams = [Camera.from_scene(c) for c in S.ring_cameras(sc.cam, 3, radius=5.0)]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    with torch.no_grad():
        gts = [render(dev(sc.pws), dev(sc.shs), dev(sc.alphas), dev(sc.scales), dev(sc.rots), c)[0].contiguous()
               for c in cams]
    return cams, gts


def trainer(cams, gts, **kw):
    from easygaussiansplatting_amd.trainer import Trainer
    start = S.small_scene(N, W, H, 48)
    start.shs[:, :3] += 0.2
    args = dict(max_steps=10, view_streams=1)
    args.update(kw)
    return Trainer(start, cams, gts, **args)


def host(t):
    return t.detach().cpu().numpy()


def run(tr, steps=STEPS):
    """-> (losses of the steps, parameter gradients of every step)"""
    losses, grads = [], []
    for views in steps:
        losses.append(tr.step(list(views)))
        grads.append({k: tr.params[k].grad.detach().double() for k in GRAD_KEYS})
    return np.array(losses, np.float64), grads


def spread_of(a, b):
    """how far two runs of the same steps are apart: losses absolutely, gradients in units of their largest entry
    (``grads``: the largest over tensors and steps; per tensor under its own name, for the messages)"""
    (la, ga), (lb, gb) = a, b
    rel = lambda k: max(float((x[k] - y[k]).abs().max() / x[k].abs().max()) for x, y in zip(ga, gb))
    per = {k: rel(k) for k in GRAD_KEYS}
    return dict(loss=float(np.abs(la - lb).max()), grads=max(per.values()), **per)


@pytest.fixture(scope="module")
def control(setup):
    """two unweighted trainers from the same start -> (the first one's run, how far apart the two are)"""
    cams, gts = setup
    a, b = run(trainer(cams, gts)), run(trainer(cams, gts))
    spread = spread_of(a, b)
    print("control pair: losses %s the bit; spread %s" % ("agree to" if spread["loss"] == 0 else "differ beyond", spread))
    assert np.isfinite(a[0]).all() and all(np.isfinite(v) for v in spread.values())
    return a, spread


def assert_same(got, want, spread, what):
    """the control-pair rule: equal where the control pair is equal, within twice its spread elsewhere"""
    d = spread_of(got, want)
    for k in ("loss", "grads"):
        assert d[k] <= 2.0 * spread[k], "%s: %s differs by %.3e, the control pair by %.3e (%s)" % (what, k, d[k], spread[k], d)


def test_default_trainer_loads_no_library_and_keeps_no_weight(setup, monkeypatch):
    from easygaussiansplatting_amd import _wlosslib
    cams, gts = setup
    loads = []
    monkeypatch.setattr(_wlosslib, "_lib", None)
    monkeypatch.setattr(_wlosslib, "load", lambda: loads.append(1) or pytest.fail("libegs_wloss.so was loaded"))
    tr = trainer(cams, gts)
    assert tr.pixel_weights is None
    assert np.isfinite(tr.step([1])) and np.isfinite(tr.step([0, 2]))
    assert loads == [] and _wlosslib._lib is None and tr.pixel_weights is None
    # a list of None: every view takes the unweighted kernels
    tr = trainer(cams, gts, pixel_weights=[None, None, None])
    assert np.isfinite(tr.step([1]))
    assert loads == []


def test_all_ones_weights_train_as_no_weights(setup, control):
    cams, gts = setup
    base, spread = control
    ones = [torch.ones((H, W), device="cuda") for _ in cams]
    got = run(trainer(cams, gts, pixel_weights=ones))
    print("all-ones against unweighted: %s" % spread_of(got, base))
    assert_same(got, base, spread, "all-ones weights")


def test_a_masked_corruption_leaves_no_trace(setup, control):
    """a 30 x 30 square of view 1's photograph is overwritten; the weights are zero on the square dilated by 5 px"""
    cams, gts = setup
    _, spread = control
    bad = [g.clone() for g in gts]
    bad[1][:, 30:60, 50:80] = 1.0
    assert float((bad[1] - gts[1]).abs().max()) > 0.2
    w = torch.ones((H, W), device="cuda")
    w[25:65, 45:85] = 0.0
    weights = [None, w, None]
    clean = run(trainer(cams, gts, pixel_weights=weights), steps=([1],))
    masked = run(trainer(cams, bad, pixel_weights=weights), steps=([1],))
    print("masked corruption against clean: %s" % spread_of(masked, clean))
    assert_same(masked, clean, spread, "corrupted photograph under the mask")
    unmasked = run(trainer(cams, bad), steps=([1],))
    d = spread_of(unmasked, clean)
    assert d["loss"] > 1e-3 and d["loss"] > 100 * spread["loss"], d
    for k in GRAD_KEYS:
        assert d[k] > 100 * spread["grads"], (k, d)
    # (one pixel less of dilation and the corruption is within reach of a weighted pixel's window)
    w4 = torch.ones((H, W), device="cuda")
    w4[26:64, 46:84] = 0.0
    near = [run(trainer(cams, g, pixel_weights=[None, w4, None]), steps=([1],)) for g in (gts, bad)]
    assert spread_of(*near)["loss"] > 2.0 * spread["loss"]


def test_gradient_handed_to_the_render(setup, monkeypatch):
    from easygaussiansplatting_amd import trainer as T
    from easygaussiansplatting_amd.function import GSRawFunction, RenderOptions
    from easygaussiansplatting_amd.loss import gau_loss_with_grad
    cams, gts = setup
    g = torch.Generator(device="cuda").manual_seed(3)
    weights = [3.0 * torch.rand((H, W), device="cuda", generator=g) for _ in cams]
    weights[2] = None
    tr = trainer(cams, gts, pixel_weights=weights)
    params = [tr.params[k].detach().clone() for k in tr._KEYS]
    calls = []

    def spy(image, gt, *a, **kw):
        out = gau_loss_with_grad(image, gt, *a, **kw)
        calls.append((image.detach().clone(), gt, kw, out[0].clone(), out[1].clone()))
        return out

    monkeypatch.setattr(T, "gau_loss_with_grad", spy)
    views = [1, 2]
    loss = tr.step(views)
    assert len(calls) == 2
    for v, (image, gt, kw, stats, dimage) in zip(views, calls):
        assert gt is tr.gts[v] and kw["grad_scale"] == 1.0 / len(views)
        assert kw["weight"] is tr.pixel_weights[v] and (kw["weight"] is None) == (v == 2)
        assert stats.numel() == (3 if v == 2 else 4)
    assert abs(loss - float(calls[0][3][0] + calls[1][3][0]) / 2) <= 1e-6
    # the weighted view, re-rendered from the parameters the step started with
    image, gt, kw, stats, dimage = calls[0]
    with torch.no_grad():
        us = torch.zeros((params[0].shape[0], 2), device="cuda")
        again = GSRawFunction.apply(*params, us, cams[1], RenderOptions())[0].contiguous()
    st, want = gau_loss_with_grad(again, gts[1], weight=tr.pixel_weights[1], grad_scale=0.5)
    assert_grad_close(host(dimage), host(want), "dimage of a weighted view", outliers=0)
    assert abs(float(st[0]) - float(stats[0])) <= 1e-6 and abs(float(st[3]) - float(weights[1].sum())) <= 1e-2
    # and it is not the unweighted one
    _, plain = gau_loss_with_grad(again, gts[1], grad_scale=0.5)
    assert float((plain - want).abs().max()) > 0.1 * float(plain.abs().max())


@pytest.mark.parametrize("kw", [dict(bilagrid=True, bilagrid_shape=(6, 5, 4)), dict(sparse_adam=True),
                                dict(pose_opt=True), dict(strategy="mcmc", cap_max=3000), dict(view_streams=2),
                                dict(mode="ops", fused_activations=False)],
                         ids=["bilagrid", "sparse_adam", "pose_opt", "mcmc", "two-streams", "ops"])
def test_it_works_with_the_other_options(setup, kw):
    cams, gts = setup
    w = torch.ones((H, W), device="cuda")
    w[:, :40] = 0.0
    tr = trainer(cams, gts, pixel_weights=[w, None, w > 0], **kw)      # a weighted view, a plain one, a bool mask
    assert tr.pixel_weights[1] is None and tr.pixel_weights[2].dtype == torch.float32
    for views in ([0, 1], [2, 1, 0]):
        assert np.isfinite(tr.step(views)), views
    for k in tr._KEYS:
        assert bool(torch.isfinite(tr.params[k]).all()), k
    if "bilagrid" in kw:
        assert tr.grid_table.steps.tolist() == [2, 2, 1] and bool(torch.isfinite(tr.grid_table.grids).all())
        # the weighted loss sees the corrected image: the grid of a weighted view moved
        assert bool((tr.grid_table.grids[0] != tr.grid_table.grids[1]).any())
