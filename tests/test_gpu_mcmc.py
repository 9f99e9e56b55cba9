"""MCMC densification on the GPU: libegs_mcmc.so through ``density.MCMCControl`` and ``Trainer(strategy=
"mcmc")`` against the float64 restatement of include/egs_mcmc.h in tests/mcmc_ref.py.

Tolerances: a quantity computed from float32 tensors is compared with the float64 reference within the larger of a
stated float32 round-off and TWICE the distance of a float32 NumPy evaluation of the same formula from the float64 one
(``R.*(dtype=np.float32)``): the bound is set by the number format, not by the kernel."""
import numpy as np
import pytest
import torch

from tests import mcmc_ref as R

pytestmark = pytest.mark.gpu

NAMES = ("pws", "low_shs", "high_shs", "alphas_raw", "scales_raw", "rots_raw")
LRS = (0.001, 0.001, 0.001 / 20, 0.05, 0.005, 0.001)
S = R.S


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _logit(o):
    return np.log(o / (1 - o))


def _raw_params(n, hw, seed, opacity):
    """raw parameter arrays (float32) with the given opacities"""
    f = lambda a: np.ascontiguousarray(a, np.float32)
    return {"pws": f(S.uniform01(seed, 1, (n, 3)) * 2 - 1), "low_shs": f(S.normal(seed, 2, (n, 3))),
            "high_shs": f(S.normal(seed, 3, (n, hw))), "alphas_raw": f(_logit(opacity)).reshape(n, 1),
            "scales_raw": f(np.log(0.05 + 0.15 * S.uniform01(seed, 4, (n, 3)))), "rots_raw": f(S.normal(seed, 5, (n, 4)))}


def _setup(raw, opt_name="fused", with_state=True, seed=9):
    from easygaussiansplatting_amd.optim import FusedAdam
    opt_cls = FusedAdam if opt_name == "fused" else torch.optim.Adam
    params = {k: _dev(raw[k]).requires_grad_() for k in NAMES}
    opt = opt_cls([{"params": [params[k]], "lr": lr, "name": k} for k, lr in zip(NAMES, LRS)], lr=0.0, eps=1e-15)
    if with_state:
        for j, k in enumerate(NAMES):
            step = 2 if opt_cls is FusedAdam else torch.tensor(2.0)
            m = S.normal(seed, 20 + j, raw[k].shape).astype(np.float32)
            v = (S.uniform01(seed, 30 + j, raw[k].shape) + 0.1).astype(np.float32)
            opt.state[params[k]] = {"step": step, "exp_avg": _dev(m), "exp_avg_sq": _dev(v)}
    return params, opt


def _moments(params, opt):
    return ({k: _np(opt.state[params[k]]["exp_avg"]) for k in NAMES},
            {k: _np(opt.state[params[k]]["exp_avg_sq"]) for k in NAMES})


# ------------------------------------------------------------------------------------------------------------ sampler
@pytest.mark.parametrize("n", [1, 1031, 300001])
def test_sampler_equals_searchsorted(n):
    """weights are multiples of 1/1024: the double prefix sum is exact in any order, so the indices must EQUAL the
    reference's.  One workgroup (1, 1031: no multiple of 256 or 1024) and a scan of 293 workgroup sums (300 001)."""
    from easygaussiansplatting_amd import _mcmclib
    lib = _mcmclib.load()
    draws, seed, rnd = 4099, 7, 5
    w = (np.floor(S.uniform01(n, 1, (n,)) * 1025) / 1024).astype(np.float32)
    if n > 1:
        w[S.uniform01(n, 2, (n,)) < 0.3] = 0          # zero rows everywhere, zero runs at both ends and inside
        w[:37] = 0
        w[-41:] = 0
        w[n // 2:n // 2 + 300] = 0
        w[37], w[n - 42] = 1 / 1024, 1.0              # the first and the last row that can be drawn
    else:
        w[:] = 0.5
    want = R.sample(w, draws, seed, rnd)
    assert (w[want] > 0).all()
    wd = _dev(w)
    ws = torch.empty(lib.egs_mcmc_sample_ws_bytes(n), dtype=torch.uint8, device="cuda")
    idx = torch.full((draws,), -7, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    _mcmclib.check(lib.egs_mcmc_sample(n, wd.data_ptr(), int((w > 0).sum()), draws, seed, rnd, idx.data_ptr(),
                                       ws.data_ptr(), ws.numel(), stream))
    got = _np(idx).astype(np.int64)
    np.testing.assert_array_equal(got, want)
    # the prefix sums themselves (first piece of the workspace) are the reference's, to the bit
    cdf = _np(ws[:8 * n].view(torch.float64))
    np.testing.assert_array_equal(cdf, R.cdf(w))
    # another round is another stream
    _mcmclib.check(lib.egs_mcmc_sample(n, wd.data_ptr(), int((w > 0).sum()), draws, seed, rnd + 1, idx.data_ptr(),
                                       ws.data_ptr(), ws.numel(), stream))
    np.testing.assert_array_equal(_np(idx).astype(np.int64), R.sample(w, draws, seed, rnd + 1))


def test_weights_and_totals():
    from easygaussiansplatting_amd.density import MCMCControl
    from easygaussiansplatting_amd import _mcmclib
    n = 1031
    o = np.where(S.uniform01(3, 1, (n,)) < 0.4, 0.001, 0.02 + 0.9 * S.uniform01(3, 2, (n,)))
    a = _logit(o).astype(np.float32)
    ctl = MCMCControl(5000)
    stream = torch.cuda.current_stream().cuda_stream
    for reloc in (True, False):
        want_w, want_dead, totals = R.weights(a, 0.005, reloc)
        w, dead, nd, nl = ctl._weights(_mcmclib.load(), [_dev(a.reshape(n, 1))] * 6, n, reloc, stream)
        assert (nd, nl) == totals and nd + nl == n
        np.testing.assert_array_equal(_np(dead).astype(bool), want_dead)
        np.testing.assert_allclose(_np(w), want_w, rtol=3e-7, atol=0)
        assert (_np(w)[want_dead] == 0).all() if reloc else (_np(w) > 0).all()


# --------------------------------------------------------------------------------------------------------- relocation
def _reloc_case(hw):
    """2000 rows, min_opacity 1e-5: 260 dead, one row with ~88 % of the weight (drawn far more than 51 times), five
    warm rows drawn a few times each, the rest almost never"""
    n = 2000
    o = 4e-5 * (0.5 + S.uniform01(21, 1, (n,)))
    dead = np.zeros(n, bool)
    dead[S.uniform01(21, 2, (n,)) < 0.13] = True
    dead[[0, n - 1]] = True
    hot, warm = 777, [5, 300, 900, 1500, 1900]
    dead[[hot] + warm] = False
    o[dead] = 1e-6
    o[hot] = 0.99
    o[warm] = 0.012
    return _raw_params(n, hw, 21, o), dead, hot


@pytest.mark.parametrize("hw", [45, 0])
@pytest.mark.parametrize("opt_name", ["fused", "torch"])
def test_relocation_matches_reference(hw, opt_name):
    from easygaussiansplatting_amd import _mcmclib
    from easygaussiansplatting_amd.density import MCMCControl
    raw, dead, hot = _reloc_case(hw)
    n = raw["pws"].shape[0]
    params, opt = _setup(raw, opt_name)
    m0, v0 = _moments(params, opt)
    ctl = MCMCControl(10 ** 6, seed=4, min_opacity=1e-5)
    lib = _mcmclib.load()
    stream = torch.cuda.current_stream().cuda_stream
    # the draws of this refinement (the sampler has its own test): same (seed, round) -> same indices
    w, dflag, nd, nl = ctl._weights(lib, [params[k] for k in NAMES], n, True, stream)
    src = _np(ctl._sample(lib, w, nl, nd, stream)).astype(np.int64)
    ctl.round = 0
    dst = np.nonzero(dead)[0]
    assert nd == dead.sum() and np.array_equal(_np(dflag).astype(bool), dead) and not dead[src].any()
    cnt = R.counts(src, n)
    others = np.setdiff1d(np.nonzero(cnt > 1)[0], [hot])
    print("draws %d, count of the hot row %d, other sources %s" % (nd, cnt[hot], sorted(cnt[others].tolist())))
    assert cnt[hot] > R.N_MAX and ((cnt[others] >= 2) & (cnt[others] <= 5)).sum() >= 3

    before = {k: t.detach().clone() for k, t in params.items()}
    rep = ctl.relocate(params, opt)
    assert rep == {"relocated": int(nd)} and ctl.round == 1
    for k, grp in zip(NAMES, opt.param_groups):          # in place: same tensors, same optimizer state objects
        assert grp["params"][0] is params[k] and params[k].shape == before[k].shape

    want = R.relocate(raw, src, dst, 1e-5)
    w32 = R.relocate(raw, src, dst, 1e-5, np.float32)
    touched = np.zeros(n, bool)
    touched[dst] = True
    touched[want["drawn"]] = True
    assert touched.sum() == nd + len(want["drawn"])
    got_o = R.sigmoid(_np(params["alphas_raw"]).reshape(-1))
    got_s = np.exp(_np(params["scales_raw"]).astype(np.float64))
    for name, got, ref, ref32 in (("opacity", got_o, want["o"], w32["o"]), ("scale", got_s, want["s"], w32["s"])):
        rel = lambda x: (np.abs(x - ref) / np.abs(ref))[touched].max()
        bound = max(1e-5, 2 * rel(ref32.astype(np.float64)))
        print("%s: max relative error %.3g (float32 evaluation %.3g, bound %.3g)"
              % (name, rel(got), rel(ref32.astype(np.float64)), bound))
        assert rel(got) <= bound, name
    # the hot row took the N = 51 branch: its copies are NOT what N = count would give
    o_hot = R.sigmoid(raw["alphas_raw"][hot])
    assert abs(got_o[hot] - (1 - (1 - o_hot) ** (1 / 51.0))) < 1e-6 * got_o[hot]
    # copied tensors: bit-equal to the source row
    for k in ("pws", "low_shs", "high_shs", "rots_raw"):
        np.testing.assert_array_equal(_np(params[k]), want[k], err_msg=k)
        np.testing.assert_array_equal(_np(params[k])[dst], raw[k][src], err_msg=k)
    # moments: zero on dst and drawn rows; every other row, and its moments, untouched to the bit
    m1, v1 = _moments(params, opt)
    for k in NAMES:
        assert not m1[k][touched].any() and not v1[k][touched].any(), k
        np.testing.assert_array_equal(m1[k][~touched], m0[k][~touched], err_msg=k)
        np.testing.assert_array_equal(v1[k][~touched], v0[k][~touched], err_msg=k)
        np.testing.assert_array_equal(_np(params[k])[~touched], raw[k][~touched], err_msg=k)
        assert float(opt.state[params[k]]["step"]) == 2.0
    # nothing is dead any more: a second refinement relocates nothing and changes nothing
    snap = {k: t.detach().clone() for k, t in params.items()}
    assert ctl.relocate(params, opt) == {"relocated": 0}
    assert all(torch.equal(snap[k], params[k].detach()) for k in NAMES)


def test_relocate_without_optimizer_state_and_with_nothing_alive():
    from easygaussiansplatting_amd.density import MCMCControl
    raw, dead, hot = _reloc_case(45)
    params, opt = _setup(raw, with_state=False)
    ctl = MCMCControl(10 ** 6, seed=4, min_opacity=1e-5)
    assert ctl.relocate(params, opt)["relocated"] == dead.sum()
    assert not opt.state and torch.isfinite(params["alphas_raw"]).all() and torch.isfinite(params["scales_raw"]).all()
    raw["alphas_raw"][:] = -20.0
    params, opt = _setup(raw, with_state=False)
    with pytest.raises(RuntimeError, match="alive"):
        ctl.relocate(params, opt)


# ------------------------------------------------------------------------------------------------------------- growth
@pytest.mark.parametrize("opt_name", ["fused", "torch"])
@pytest.mark.parametrize("cap,expect", [(5000, 1050), (1020, 1020), (1000, 1000)])
def test_growth_respects_the_cap(cap, expect, opt_name):
    from easygaussiansplatting_amd.density import MCMCControl
    n = 1000
    raw = _raw_params(n, 45, 31, 0.01 + 0.9 * S.uniform01(31, 9, (n,)))
    params, opt = _setup(raw, opt_name)
    m0, v0 = _moments(params, opt)
    old = dict(params)
    ctl = MCMCControl(cap, seed=2)
    if expect > n:      # the draws of this growth (the sampler has its own test): same (seed, round) -> same indices
        from easygaussiansplatting_amd import _mcmclib
        stream = torch.cuda.current_stream().cuda_stream
        w, _, _, _ = ctl._weights(_mcmclib.load(), [params[k] for k in NAMES], n, False, stream)
        draws = _np(ctl._sample(_mcmclib.load(), w, n, expect - n, stream)).astype(np.int64)
        want_draws = R.sample(R.weights(raw["alphas_raw"], 0.005, False)[0], expect - n, 2, 0)
        assert (draws == want_draws).mean() > 0.9      # (weights that differ in the last bit may move a boundary)
        ctl.round = 0
    rep = ctl.grow(params, opt)
    assert rep == {"added": expect - n, "total": expect} and expect == min(cap, int(1.05 * n))
    if expect == n:                       # already at the cap: the very same tensors, nothing sampled
        assert all(params[k] is old[k] for k in NAMES) and ctl.round == 0
        assert all(np.array_equal(_np(params[k]), raw[k]) for k in NAMES)
        return
    src = draws
    cnt = R.counts(src, expect)
    drawn = np.nonzero(cnt > 1)[0]
    keep = np.ones(expect, bool)
    keep[drawn] = False
    keep[n:] = False
    m1, v1 = _moments(params, opt)
    for k, grp in zip(NAMES, opt.param_groups):
        p = params[k]
        assert grp["params"][0] is p and isinstance(p, torch.nn.Parameter) and p.requires_grad
        assert p.shape == (expect,) + raw[k].shape[1:]
        st = opt.state[p]
        assert st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape and float(st["step"]) == 2.0
        np.testing.assert_array_equal(_np(p)[keep], raw[k][keep[:n]], err_msg=k)
        np.testing.assert_array_equal(m1[k][keep], m0[k][keep[:n]], err_msg=k)
        np.testing.assert_array_equal(v1[k][keep], v0[k][keep[:n]], err_msg=k)
        assert not m1[k][~keep].any() and not v1[k][~keep].any(), k
    for k in ("pws", "low_shs", "high_shs", "rots_raw"):      # appended rows are copies of the drawn rows
        np.testing.assert_array_equal(_np(params[k])[n:], raw[k][src], err_msg=k)
    # ... with the corrected opacity and scale, shared with their source
    o_new = R.sigmoid(_np(params["alphas_raw"]).reshape(-1))
    o_src, s_src = R.corrected(R.sigmoid(raw["alphas_raw"].reshape(-1))[drawn], np.exp(raw["scales_raw"].astype(np.float64))[drawn],
                               cnt[drawn], 0.005)
    np.testing.assert_allclose(o_new[drawn], o_src, rtol=1e-5)
    np.testing.assert_allclose(o_new[n:], o_new[src], rtol=0)
    np.testing.assert_allclose(np.exp(_np(params["scales_raw"]).astype(np.float64))[drawn], s_src, rtol=1e-5)
    assert torch.isfinite(params["alphas_raw"]).all() and torch.isfinite(params["scales_raw"]).all()
    # the optimizer keeps stepping on the grown tensors
    for k in NAMES:
        params[k].grad = torch.ones_like(params[k]) * 1e-3
    opt.step()
    assert all(torch.isfinite(params[k]).all() for k in NAMES)


# -------------------------------------------------------------------------------------------------------------- noise
def _noise_case(n=1531):
    o = 0.001 + 0.009 * S.uniform01(41, 1, (n,))            # w between 0.38 and 0.60 ...
    o[::7] = 0.05 + 0.9 * S.uniform01(41, 2, (n,))[::7]     # ... and opaque rows that barely move
    return _raw_params(n, 0, 41, o)


def test_noise_matches_reference():
    from easygaussiansplatting_amd.density import MCMCControl
    raw = _noise_case()
    n = raw["pws"].shape[0]
    z = S.normal(8, 77, (n, 3)).astype(np.float32)
    params, _ = _setup(raw, with_state=False)
    ctl = MCMCControl(10 ** 6, seed=6)
    lr = 1.6e-4
    ctl.inject_noise(params, lr, unit_noise=_dev(z))
    assert ctl.step == 1
    got = _np(params["pws"]).astype(np.float64) - raw["pws"]
    want = R.noise_delta(raw["alphas_raw"], raw["scales_raw"], raw["rots_raw"], z, 5e5, lr)
    with np.errstate(over="ignore"):
        w32 = R.noise_delta(raw["alphas_raw"], raw["scales_raw"], raw["rots_raw"], z, 5e5, lr, np.float32)
    big = np.abs(want).max()
    e32 = np.abs(w32 - want).max() / big
    # (the sum pws + delta is rounded to float32 once more: half an ulp of a coordinate, 1e-7 of the displacement)
    bound = max(1e-5, 2 * e32)
    err = np.abs(got - want).max() / big
    print("noise: largest displacement %.3g, max error %.3g of it (float32 evaluation %.3g, bound %.3g)"
          % (big, err, e32, bound))
    assert big > 0.1 and err <= bound
    for k in NAMES[1:]:
        np.testing.assert_array_equal(_np(params[k]), raw[k])


def test_generated_noise_is_the_documented_stream():
    from easygaussiansplatting_amd.density import MCMCControl
    raw = _noise_case()
    n = raw["pws"].shape[0]
    a, _ = _setup(raw, with_state=False)
    b, _ = _setup(raw, with_state=False)
    ca, cb = MCMCControl(10 ** 6, seed=6), MCMCControl(10 ** 6, seed=6)
    ca.step = cb.step = 12
    ca.inject_noise(a, 1.6e-4)
    cb.inject_noise(b, 1.6e-4, unit_noise=_dev(R.unit_noise(6, 12, n).astype(np.float32)))
    assert torch.equal(a["pws"].detach(), b["pws"].detach())
    assert not torch.equal(a["pws"].detach(), _dev(raw["pws"]))
    ca.inject_noise(a, 1.6e-4)                   # the next step draws from the next stream
    cb.inject_noise(b, 1.6e-4, unit_noise=_dev(R.unit_noise(6, 13, n).astype(np.float32)))
    assert torch.equal(a["pws"].detach(), b["pws"].detach())


def test_opaque_gaussians_stay_put():
    from easygaussiansplatting_amd.density import MCMCControl
    raw = _raw_params(2, 0, 43, np.array([0.9999, 0.001]))
    for k in NAMES:
        if k != "alphas_raw":
            raw[k][0] = raw[k][1]
    params, _ = _setup(raw, with_state=False)
    z = np.tile(np.array([[0.7, -1.1, 0.4]], np.float32), (2, 1))
    MCMCControl(10, seed=0).inject_noise(params, 1.6e-4, unit_noise=_dev(z))
    d = np.abs(_np(params["pws"]).astype(np.float64) - raw["pws"]).max(axis=1)
    assert d[1] > 1e-3 and d[0] < 1e-6 * d[1]


# -------------------------------------------------------------------------------------------------------- regulariser
def test_regulariser_matches_autograd():
    from easygaussiansplatting_amd.density import MCMCControl
    n = 1031
    raw = _raw_params(n, 0, 51, 0.001 + 0.998 * S.uniform01(51, 1, (n,)))
    lam_o, lam_s = 0.01, 0.02
    a64 = torch.from_numpy(raw["alphas_raw"].astype(np.float64)).requires_grad_()
    s64 = torch.from_numpy(raw["scales_raw"].astype(np.float64)).requires_grad_()
    (lam_o * torch.sigmoid(a64).mean() + lam_s * torch.exp(s64).mean()).backward()
    want = {"alphas_raw": a64.grad.numpy(), "scales_raw": s64.grad.numpy()}
    r32 = dict(zip(("alphas_raw", "scales_raw"), R.reg_grad(raw["alphas_raw"], raw["scales_raw"], lam_o, lam_s,
                                                            np.float32)))
    r64 = dict(zip(("alphas_raw", "scales_raw"), R.reg_grad(raw["alphas_raw"], raw["scales_raw"], lam_o, lam_s)))
    params, _ = _setup(raw, with_state=False)
    g0 = {}
    for j, k in enumerate(("alphas_raw", "scales_raw")):     # gradients that are already there: the call ADDS
        g0[k] = (np.abs(want[k]).max() * 0.5 * S.normal(51, 60 + j, raw[k].shape)).astype(np.float32)
        params[k].grad = _dev(g0[k])
    ctl = MCMCControl(10 ** 6, opacity_reg=lam_o, scale_reg=lam_s)
    ctl.add_regularisers(params)
    for k in ("alphas_raw", "scales_raw"):
        np.testing.assert_allclose(r64[k], want[k], rtol=1e-12)          # the restatement is the stated loss
        big = np.abs(want[k]).max()
        e32 = np.abs(r32[k].astype(np.float64) - want[k]).max() / big
        bound = max(1e-6, 2 * e32)
        err = np.abs(_np(params[k].grad).astype(np.float64) - (g0[k].astype(np.float64) + want[k])).max() / big
        print("%s: max error %.3g of the largest entry (float32 evaluation %.3g, bound %.3g)" % (k, err, e32, bound))
        assert err <= bound, k
    params["alphas_raw"].grad = None
    with pytest.raises(ValueError):
        ctl.add_regularisers(params)


# -------------------------------------------------------------------------------------------------------- determinism
def test_refinement_and_noise_are_bitwise_reproducible():
    """replicas rely on it: equal inputs and equal (seed, round, step) -> equal bits"""
    from easygaussiansplatting_amd.density import MCMCControl
    raw, _, _ = _reloc_case(45)
    runs = []
    for rep in range(2):
        params, opt = _setup(raw)
        ctl = MCMCControl(2060, seed=4, min_opacity=1e-5)
        ctl.round, ctl.step = 3, 40
        r1 = ctl.relocate(params, opt)
        r2 = ctl.grow(params, opt)
        ctl.inject_noise(params, 1.6e-4)
        assert r1["relocated"] > 0 and r2 == {"added": 60, "total": 2060} and (ctl.round, ctl.step) == (5, 41)
        m, v = _moments(params, opt)
        runs.append(({k: _np(params[k]) for k in NAMES}, m, v))
    for k in NAMES:
        for a, b in zip(runs[0], runs[1]):
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)


# ------------------------------------------------------------------------------------------------------------ trainer
def test_trainer_with_the_mcmc_strategy(monkeypatch):
    from easygaussiansplatting_amd import density
    from easygaussiansplatting_amd import gsplatcu as gsc
    from easygaussiansplatting_amd.function import Camera, render
    from easygaussiansplatting_amd.trainer import Trainer
    gsc.set_policy("gsplatcu")
    sc = S.small_scene(3000, 64, 64, 48, seed=17)
    cams = [Camera.from_scene(c) for c in S.ring_cameras(sc.cam, 2, radius=5.0)]
    with torch.no_grad():
        gts = [render(_dev(sc.pws), _dev(sc.shs), _dev(sc.alphas), _dev(sc.scales), _dev(sc.rots), c)[0] for c in cams]

    def never(*a, **k):
        raise AssertionError("reset_alpha reached with strategy='mcmc'")
    monkeypatch.setattr(density.DensityControl, "reset_alpha", never)
    start = S.small_scene(3000, 64, 64, 48, seed=17)
    start.shs[:, :3] += 0.8 * S.normal(5, 3, (3000, 3)).astype(np.float32)
    tr = Trainer(start, cams, gts, max_steps=400, scene_size=4.0, seed=3, strategy="mcmc", cap_max=3200)
    losses = [tr.step([0, 1]) for _ in range(6)]
    assert tr.mcmc.step == 6
    rep = tr.densify()
    assert rep["total"] == 3150 == tr.params["pws"].shape[0] and rep["added"] == 150
    assert tr.grad_accum.shape == (3150,) and tr.vis_count.shape == (3150,)
    losses += [tr.step([0, 1]) for _ in range(6)]
    assert tr.densify()["total"] == 3200
    losses += [tr.step([0, 1]) for _ in range(3)]
    rep = tr.densify()                    # at the cap: relocation only
    assert rep["added"] == 0 and rep["total"] == 3200 == tr.params["pws"].shape[0]
    # fit(): epochs 2..5 densify, epoch 3 would reset alpha under the default strategy
    hist = tr.fit(epochs=6, views_per_step=2, densify_every=2, reset_alpha_every=3, densify_until=5)
    losses += hist
    n = tr.params["pws"].shape[0]
    assert n == 3200 and tr.grad_accum.shape == (n,)
    for k, grp in zip(NAMES, tr.opt.param_groups):
        assert grp["params"][0] is tr.params[k] and tr.params[k].shape[0] == n
        assert tr.opt.state[tr.params[k]]["exp_avg"].shape == tr.params[k].shape
        assert torch.isfinite(tr.params[k]).all() and torch.isfinite(tr.opt.state[tr.params[k]]["exp_avg"]).all()
    print("losses", ["%.5f" % x for x in losses])
    assert all(np.isfinite(losses)) and losses[-1] <= losses[0]
