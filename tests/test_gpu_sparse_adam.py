"""Visibility-masked Adam on the device (csrc/egs_adam.hip, include/egs_adam.h) through
``FusedAdam.step(visible=...)`` and ``Trainer(sparse_adam=True)``.  The dense kernels are the yardstick: a visible row
gets what ``FusedAdam.step()`` gives it and an invisible row keeps what it had, so every comparison is ``torch.equal``
-- there is no tolerance anywhere in this file."""
import numpy as np
import pytest
import torch

from tests import sparse_adam_ref as R

pytestmark = pytest.mark.gpu

NAMES = ("pws", "low_shs", "high_shs", "alphas_raw", "scales_raw", "rots_raw")
KEYS = ("exp_avg", "exp_avg_sq")


def _optimizer(tensors):
    from easygaussiansplatting_amd.optim import FusedAdam
    return FusedAdam([{"params": [p], "lr": lr, "name": k} for p, lr, k in zip(tensors, R.LRS, NAMES)], lr=0.0, eps=1e-15)


def _clone(ps, opt):
    """an independent copy of the parameters and of the optimizer's state, at the same step counts"""
    qs = [p.detach().clone().requires_grad_() for p in ps]
    new = _optimizer(qs)
    for p, q in zip(ps, qs):
        if p in opt.state:
            st = opt.state[p]
            new.state[q] = {"step": st["step"], "exp_avg": st["exp_avg"].clone(), "exp_avg_sq": st["exp_avg_sq"].clone()}
    return qs, new


def _snapshot(ps, opt):
    return [(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for p in ps]


def _triples(ps, opt):
    return [(p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]) for p in ps]


def _grads(ps, gen):
    """one scale per tensor and step, spread over 1e-6 .. 1"""
    return [torch.randn(p.shape, device="cuda", generator=gen) * 10 ** float(torch.randint(-6, 1, (1,))) for p in ps]


def _start(n, seed, warm=0):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    torch.manual_seed(seed)
    ps = [torch.randn(n, w, device="cuda", generator=gen).requires_grad_() for w in R.WIDTHS]
    opt = _optimizer(ps)
    for _ in range(warm):           # dense steps: the moments are not zero when the masked step begins
        for p, g in zip(ps, _grads(ps, gen)):
            p.grad = g
        opt.step()
    return ps, opt, gen


def _bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------- 1. all visible == dense
@pytest.mark.parametrize("n", [1, 3, 63, 64, 65, 1023, 4097])
def test_all_visible_equals_the_dense_step(n):
    pa, oa, gen = _start(n, n)
    pb, ob = _clone(pa, oa)
    for step in range(3):
        gs = _grads(pa, gen)
        for a, b, g in zip(pa, pb, gs):
            a.grad, b.grad = g.clone(), g.clone()
        oa.step()
        ob.step(visible=torch.ones(n, device="cuda", dtype=torch.bool if step % 2 == 0 else torch.uint8))
        for k, (ta, tb) in enumerate(zip(_triples(pa, oa), _triples(pb, ob))):
            for x, y in zip(ta, tb):
                assert torch.equal(x, y), (step, NAMES[k], float((x - y).abs().max()))
            assert oa.state[pa[k]]["step"] == ob.state[pb[k]]["step"] == step + 1
    assert all(bool(torch.isfinite(p).all()) for p in pb)


# ---------------------------------------------------------------------------------------------------- 2. mask shapes
@pytest.mark.parametrize("n", [65, 1023])
def test_mask_shapes(n):
    """invisible rows keep their bits although their gradient rows hold NaN; visible rows get the dense step"""
    p0, o0, gen = _start(n, 100 + n, warm=2)
    gs = _grads(p0, gen)
    pa, oa = _clone(p0, o0)
    for a, g in zip(pa, gs):
        a.grad = g.clone()
    oa.step()
    dense = _triples(pa, oa)
    before = _snapshot(p0, o0)
    shapes = R.mask_shapes(n)
    assert set(shapes) == {"none", "first", "last", "alternating", "random_half", "run_aligned", "run_straddling"}
    for name, mask in shapes.items():
        vis = torch.from_numpy(mask).cuda()
        pb, ob = _clone(p0, o0)
        for b, g in zip(pb, gs):
            b.grad = g.clone()
            b.grad[~vis] = float("nan")
        ob.step(visible=vis)
        for k, (was, full, got) in enumerate(zip(before, dense, _triples(pb, ob))):
            for w, f, x in zip(was, full, got):
                assert _bits_equal(x[~vis], w[~vis]), (name, NAMES[k])
                assert _bits_equal(x[vis], f[vis]), (name, NAMES[k])
                assert bool(torch.isfinite(x).all()), (name, NAMES[k])
            assert ob.state[pb[k]]["step"] == 3                       # the tensor's count advances whatever the mask
        if mask.any():
            assert not torch.equal(pb[2].detach()[vis], before[2][0][vis]), name          # the visible rows did move


# ------------------------------------------------------------------------------------ 3. a different mask every step
def test_five_steps_with_a_different_mask_each():
    n = 1023
    ps, opt, gen = _start(n, 7, warm=1)
    emu = _snapshot(ps, opt)                       # the same sequence emulated with dense steps on clones
    rng = np.random.RandomState(3)
    for step in range(5):
        vis = torch.from_numpy(rng.rand(n) < (0.1, 0.5, 0.9, 0.5, 0.02)[step]).cuda()
        gs = _grads(ps, gen)
        # dense step on a copy at the same step count, merged back by the mask
        qs = [e[0].clone().requires_grad_() for e in emu]
        od = _optimizer(qs)
        for q, e, g in zip(qs, emu, gs):
            od.state[q] = {"step": 1 + step, "exp_avg": e[1].clone(), "exp_avg_sq": e[2].clone()}
            q.grad = g.clone()
        od.step()
        emu = [tuple(torch.where(vis[:, None], new, old) for new, old in zip(t, e))
               for t, e in zip(_triples(qs, od), emu)]
        for p, g in zip(ps, gs):
            p.grad = g.clone()
        opt.step(visible=vis)
        for k, (e, t) in enumerate(zip(emu, _triples(ps, opt))):
            for x, y in zip(e, t):
                assert _bits_equal(x, y), (step, NAMES[k])
            assert opt.state[ps[k]]["step"] == 2 + step


# -------------------------------------------------------------------------------------------------- 4. the factored form
def _factored_masks(n):
    out = dict(R.mask_shapes(n))
    out["all"] = np.ones(n, dtype=bool)
    block = np.ones(n, dtype=bool)                 # one whole 64-row block invisible, the rest visible
    first = 64 * ((n - 1) // 64 // 2)
    block[first:first + 64] = False
    out["block_invisible"] = block
    return out


@pytest.mark.parametrize("K", [3, 12, 27, 48])
@pytest.mark.parametrize("raw", [False, True])
def test_factored_form(raw, K):
    """``step(visible=m, factored_sh=...)`` == the dense ``step(factored_sh=...)`` on clones, merged by ``m``; the
    dL/dcolour rows of the invisible Gaussians hold NaN in the masked call"""
    from easygaussiansplatting_amd import dist_views as DV
    from easygaussiansplatting_amd.optim import FusedAdam
    gen = torch.Generator(device="cuda").manual_seed(1000 * K + raw)
    rn = lambda *s: torch.randn(*s, device="cuda", generator=gen)
    for n in (1, 63, 65, 200):
        stride = DV.FactoredShGrad.row_stride(n)
        pws = (rn(n, 3) * 3).contiguous()
        widths = (3, K - 3) if (raw and K > 3) else (K,)
        init = [rn(n, w) for w in widths]

        def make(values, state=None):
            ts = [x.clone().requires_grad_() for x in values]
            opt = FusedAdam([{"params": [t], "lr": lr, "name": nm}
                             for t, lr, nm in zip(ts, (1e-3, 5e-5), ("low_shs", "high_shs"))], eps=1e-15)
            for t, st in zip(ts, state or ()):
                opt.state[t] = {"step": 1, "exp_avg": st[1].clone(), "exp_avg_sq": st[2].clone()}
            return ts, opt

        def fsh(ts, rows):
            return (rows, 0.5, pws, ts[0], ts[1] if len(ts) > 1 else None)
        for V in (1, 3):
            rows = rn(V, stride) * 1e-3
            if V > 1:
                rows[1, 0:3 * n:7] = 0.0
            rows[:, 3 * n:3 * n + 3] = rn(V, 3) * 6                    # the camera centres
            warm = rn(V, stride) * 1e-3
            warm[:, 3 * n:3 * n + 3] = rows[:, 3 * n:3 * n + 3]
            ta, oa = make(init)
            oa.step(factored_sh=fsh(ta, warm))                          # moments that are not zero
            before = _snapshot(ta, oa)
            for name, mask in _factored_masks(n).items():
                vis = torch.from_numpy(mask).cuda()
                tb, ob = make([b[0] for b in before], before)
                tc, oc = make([b[0] for b in before], before)
                ob.step(factored_sh=fsh(tb, rows))                      # dense
                holes = rows.clone()
                holes[:, :3 * n].view(V, n, 3)[:, ~vis] = float("nan")
                oc.step(factored_sh=fsh(tc, holes), visible=vis)        # masked
                for k, (was, full, got) in enumerate(zip(before, _triples(tb, ob), _triples(tc, oc))):
                    for w, f, x in zip(was, full, got):
                        want = torch.where(vis[:, None], f, w)
                        assert _bits_equal(x, want), (n, V, name, k)
                        assert bool(torch.isfinite(x).all()), (n, V, name, k)
                    assert oc.state[tc[k]]["step"] == 2
                if mask.any():
                    assert not torch.equal(tc[0].detach()[vis], before[0][0][vis]), (n, V, name)


# ---------------------------------------------------------------------------------------------------------- 5. Trainer
def _two_sided_scene():
    """a small scene around the origin, seen by both cameras, plus 300 Gaussians behind camera B that camera A sees"""
    from easygaussiansplatting_amd import scene as S
    sc = S.small_scene(8000, 192, 128, 48, seed=8)
    ex = S.small_scene(300, 192, 128, 48, seed=9)
    ex.pws[:, :2] *= 0.5
    ex.pws[:, 2] = 5.5 + (ex.pws[:, 2] + 2.0) / 4.0           # z in [5.5, 6.5]: behind camera B (at z = +5, looking at -z)
    ex.scales *= 3.0
    cat = lambda a, b: np.concatenate((a, b), axis=0)
    return S.Scene(cat(sc.pws, ex.pws), cat(sc.rots, ex.rots), cat(sc.scales, ex.scales), cat(sc.alphas, ex.alphas),
                   cat(sc.shs, ex.shs), sc.cam)


@pytest.fixture(scope="module")
def two_sided():
    from easygaussiansplatting_amd import scene as S
    from easygaussiansplatting_amd.function import Camera, render
    sc = _two_sided_scene()
    cams = [Camera.from_scene(c) for c in S.ring_cameras(sc.cam, 2, radius=5.0)]        # A at z = -5, B at z = +5
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    with torch.no_grad():
        gts = [render(dev(sc.pws), dev(sc.shs), dev(sc.alphas), dev(sc.scales), dev(sc.rots), c)[0] for c in cams]
    return cams, gts


@pytest.mark.parametrize("factored", [True, False])
def test_trainer_leaves_unseen_gaussians_alone(two_sided, factored):
    from easygaussiansplatting_amd.trainer import Trainer
    cams, gts = two_sided
    A, B = 0, 1

    def run(sparse):
        start = _two_sided_scene()
        start.shs[:, :3] += 0.4
        tr = Trainer(start, cams, gts, max_steps=100, scene_size=4.0, factored_sh=factored, sparse_adam=sparse)
        loss_a = tr.step([A])
        seen_a = tr.vis_count.clone() > 0
        snap = {k: _snapshot([p], tr.opt)[0] for k, p in tr.params.items()}
        loss_b = tr.step([B])
        seen_b = (tr.vis_count - seen_a.to(torch.int32)) > 0
        only_a = seen_a & ~seen_b
        assert np.isfinite(loss_a) and np.isfinite(loss_b)
        assert int(only_a.sum()) >= 100 and int(only_a[8000:].sum()) >= 100 and int(seen_b.sum()) >= 1000
        now = {k: _triples([p], tr.opt)[0] for k, p in tr.params.items()}
        return tr, only_a, seen_b, snap, now
    tr, only_a, seen_b, snap, now = run(True)
    for k in NAMES:
        for was, got in zip(snap[k], now[k]):
            assert _bits_equal(got[only_a], was[only_a]), k              # parameter and both moments
        assert not torch.equal(now[k][0][seen_b], snap[k][0][seen_b]), k   # what B saw did move
        assert tr.opt.state[tr.params[k]]["step"] == 2
    # densification keeps working on the unchanged state layout, and the next step runs on the new shapes
    tr.densify()
    n1 = tr.params["pws"].shape[0]
    assert n1 > 0
    assert np.isfinite(tr.step([A]))
    for k in NAMES:
        st = tr.opt.state[tr.params[k]]
        assert tr.params[k].shape[0] == st["exp_avg"].shape[0] == st["exp_avg_sq"].shape[0] == n1, k
    assert tr.vis_count.shape[0] == n1
    # the dense step, the reference's, keeps moving the same Gaussians on their old momentum
    tr, only_d, _, snap, now = run(False)
    for k in NAMES:
        assert not _bits_equal(now[k][0][only_d], snap[k][0][only_d]), k
        assert not _bits_equal(now[k][1][only_d], snap[k][1][only_d]), k
