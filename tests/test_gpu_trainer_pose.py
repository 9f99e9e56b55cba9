"""``Trainer(pose_opt=True)``: the default trainer is untouched, the pose gradient a step hands to the
``PoseTable`` is the direct computation's, only the rendered cameras move, ``poses()`` / ``save_poses`` follow."""
import types

import numpy as np
import pytest

from easygaussiansplatting_amd import scene as S
from tests.test_gpu_pose_grad import dev, host, single_tile_scene, term_scale

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def gsc():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from easygaussiansplatting_amd import gsplatcu
    gsplatcu.set_policy("gsplatcu")
    yield gsplatcu
    gsplatcu.set_policy("gsplatcu")


def ring_setup(n=3000, w=96, h=64, sh=12, views=4):
    """small_scene seen from ``views`` ring cameras; the ground truth is the scene's own render with its SH halved
    (a loss that is not zero)"""
    from easygaussiansplatting_amd.function import Camera, GSFunction
    sc = S.small_scene(n, w, h, sh, seed=11)
    cams = [Camera.from_scene(c) for c in S.ring_cameras(sc.cam, views, radius=5.0)]
    P = [dev(sc.pws), dev(sc.shs * 0.5), dev(sc.alphas).reshape(-1, 1), dev(sc.scales), dev(sc.rots)]
    us = torch.zeros((sc.n, 2), device="cuda")
    with torch.no_grad():
        gts = [GSFunction.apply(*P, us, c)[0].clone() for c in cams]
    return sc, cams, gts


def trainer(sc, cams, gts, view_streams=1, **kw):
    from easygaussiansplatting_amd.trainer import Trainer
    return Trainer(sc, cams, gts, max_steps=10, view_streams=view_streams, **kw)


def test_default_trainer_is_untouched(gsc):
    """``pose_opt=False`` against a Trainer built without the argument: bitwise-equal parameters after two steps.
    Choice of scene: single-tile style (every Gaussian inside one tile of an identity camera, rendered by four copies
    of that camera), where the gradient records are bit-reproducible, so equal code gives equal bits"""
    from easygaussiansplatting_amd.function import Camera
    sc = single_tile_scene(n=3000, w=96, h=64, sh=12)
    cams = [Camera.from_scene(sc.cam) for _ in range(4)]
    gts = [torch.full((3, 64, 96), 0.25, device="cuda") for _ in cams]
    a, b = trainer(sc, cams, gts), trainer(sc, cams, gts, pose_opt=False)
    assert b.pose_table is None and b.pose_grad is None
    for tr in (a, b):
        tr.step([0])
        tr.step([2, 1])
    for k in a.params:
        assert torch.equal(a.params[k], b.params[k]), k
    R, t = b.poses()
    assert torch.equal(R[1], cams[1].Rcw) and torch.equal(t[1], cams[1].tcw)


def test_pose_gradient_of_a_step_and_the_rows_it_moves(gsc, tmp_path):
    """The [6] gradient the table receives for the rendered view against the direct computation (GSRawPoseFunction ->
    gau_loss_with_grad -> autograd through apply_twist).  Bound: the two differ by the draw pass's atomic jitter, 4e-6
    of the term scale per component of (dL/dRcw, dL/dtcw) (rule 2 of test_gpu_pose_only.py); the twist gradient is
    J^T (dL/dRcw, dL/dtcw) with J = d(Rcw, tcw)/dtwist, so its components are held to 4e-6 |J|^T term scale"""
    from easygaussiansplatting_amd.function import GSRawPoseFunction, RenderOptions
    from easygaussiansplatting_amd.loss import gau_loss_with_grad
    from easygaussiansplatting_amd.pose import apply_twist
    sc, cams, gts = ring_setup()
    tr = trainer(sc, cams, gts, pose_opt=True)
    v = 1
    # the direct computation, on copies of the trainer's starting parameters
    p = [tr.params[k].detach().clone().requires_grad_(True) for k in tr._KEYS]
    tw = torch.zeros(6, device="cuda", requires_grad=True)
    R, t = apply_twist(cams[v].Rcw, cams[v].tcw, tw[:3], tw[3:])
    R.retain_grad(); t.retain_grad()
    us = torch.zeros((sc.n, 2), device="cuda", requires_grad=True)
    image, _ = GSRawPoseFunction.apply(*p, us, R, t, cams[v], RenderOptions())
    _, dimage = gau_loss_with_grad(image.detach(), gts[v], grad_scale=1.0)
    image.backward(dimage)
    want = host(tw.grad)
    assert np.abs(want).max() > 0

    shim = types.SimpleNamespace(pws=host(p[0]), cam=types.SimpleNamespace(Rcw=host(cams[v].Rcw)))   # for term_scale
    scale12 = term_scale(shim, host(p[0].grad))
    J = torch.autograd.functional.jacobian(
        lambda x: torch.cat([y.reshape(-1) for y in apply_twist(cams[v].Rcw, cams[v].tcw, x[:3], x[3:])]),
        torch.zeros(6, device="cuda"))                       # [12,6]
    scale6 = np.abs(host(J)).T @ scale12
    # the step: garbage in the gradient buffer first -- a step starts from zero
    tr.pose_grad.fill_(1e6)
    tab = tr.pose_table
    before = [x.clone() for x in (tab.twist, tab.exp_avg, tab.exp_avg_sq, tab.steps)]
    tr.step([v])
    got = host(tr.pose_grad)
    gap = np.abs(got[v] - want) / scale6
    print("trainer pose gradient vs direct: max gap %.3g of |J|^T term scale" % gap.max())
    assert (gap <= 4e-6).all(), (got[v], want, scale6)
    assert not got[[0, 2, 3]].any()
    for now, was in zip((tab.twist, tab.exp_avg, tab.exp_avg_sq, tab.steps), before):
        for u in (0, 2, 3):
            assert torch.equal(now[u], was[u]), u
    assert int(tab.steps[v]) == 1 and bool((tab.twist[v] != 0).all())
    # poses() follows the table
    Rs, ts = tr.poses()
    Rv, tv = apply_twist(cams[v].Rcw, cams[v].tcw, tab.twist[v, :3], tab.twist[v, 3:])
    assert torch.equal(Rs[v], Rv) and torch.equal(ts[v], tv)
    assert not torch.equal(Rs[v], cams[v].Rcw) and torch.equal(Rs[0], cams[0].Rcw) and torch.equal(ts[3], cams[3].tcw)
    fn = str(tmp_path / "poses.npz")
    tr.save_poses(fn)
    z = np.load(fn)
    assert z["Rcw"].shape == (4, 3, 3) and z["tcw"].shape == (4, 3) and len(z["ids"]) == 4
    assert np.array_equal(z["Rcw"], Rs.cpu().numpy())
    # a redone step clears the pose gradients through this helper
    tr.pose_grad.fill_(3.0)
    tr._clear_pose_grad()
    assert not bool(tr.pose_grad.any())
    with pytest.raises(ValueError, match="twice"):
        tr.step([2, 2])


def test_pose_opt_with_activations_in_torch_and_two_views(gsc):
    """``fused_activations=False`` renders through GSPoseFunction; two views in one step (in-kernel accumulation of the
    parameter gradients) leave one gradient row each"""
    sc, cams, gts = ring_setup()
    tr = trainer(sc, cams, gts, pose_opt=True, fused_activations=False, factored_sh=False)
    loss = tr.step([0, 3])
    g = host(tr.pose_grad)
    assert np.isfinite(loss) and np.isfinite(g).all()
    assert g[0].any() and g[3].any() and not g[[1, 2]].any()
    assert tr.pose_table.steps.tolist() == [1, 0, 0, 1]


def test_view_streams_give_the_same_pose_rows(gsc):
    """two views of one step dealt to two HIP streams (the twist leaves, the renders and the row updates of the pose
    gradient run on the lanes' streams) against the same step on one stream: each view's row to the jitter bound of
    the draw pass, 4e-6 |J|^T term scale as in test_pose_gradient_of_a_step_and_the_rows_it_moves.  The term scale of a
    view comes from a one-view step of a trainer of its own (its dL/dpw), halved: a two-view step weighs each view
    with 1/2.  The other rows stay zero and both rendered rows step"""
    from easygaussiansplatting_amd.pose import apply_twist
    sc, cams, gts = ring_setup()
    rows = {}
    for lanes in (1, 2):
        tr = trainer(sc, cams, gts, view_streams=lanes, pose_opt=True, factored_sh=False)
        tr.step([1, 2])
        torch.cuda.synchronize()
        rows[lanes] = host(tr.pose_grad)
        assert tr.pose_table.steps.tolist() == [0, 1, 1, 0]
    assert not rows[2][[0, 3]].any() and rows[2][1].any() and rows[2][2].any()
    for v in (1, 2):
        one = trainer(sc, cams, gts, pose_opt=True, factored_sh=False)
        pws0 = host(one.params["pws"])
        one.step([v])
        shim = types.SimpleNamespace(pws=pws0, cam=types.SimpleNamespace(Rcw=host(cams[v].Rcw)))
        J = torch.autograd.functional.jacobian(
            lambda x: torch.cat([y.reshape(-1) for y in apply_twist(cams[v].Rcw, cams[v].tcw, x[:3], x[3:])]),
            torch.zeros(6, device="cuda"))
        scale6 = 0.5 * (np.abs(host(J)).T @ term_scale(shim, host(one.params["pws"].grad)))
        gap = np.abs(rows[2][v] - rows[1][v]) / scale6
        print("two view streams vs one, view %d: max gap %.3g of |J|^T term scale" % (v, gap.max()))
        assert (gap <= 4e-6).all(), (v, rows[2][v], rows[1][v], scale6)


def test_pose_opt_needs_the_fused_path(gsc):
    sc, cams, gts = ring_setup(n=200)
    with pytest.raises(ValueError, match="pose_opt"):
        trainer(sc, cams, gts, pose_opt=True, mode="ops", fused_activations=False)
