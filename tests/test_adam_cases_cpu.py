"""The case table of the Adam kernels (tests/adam_cases.py) checked on the CPU, no GPU: every regime does what its name
says in the float32 restatement alone; the float64 form is torch.optim.Adam's formula; how far the float32 restatement
is from the float64 form, per regime (printed: ``pytest -s``; tests/test_gpu_adam_rows.py records the figures); and the
table reaches every branch of the kernels it is built for, asserted from its own counts and widths."""
import numpy as np
import pytest

from tests import adam_cases as A

F = np.float32
K = 4096


def _after(name, cfg=None, k=K):
    p, g, m, v = A.regime_alone(name, k)
    cfg = A.regime_config(name) if cfg is None else cfg
    return (p, g, m, v), A.restate(p, g, m, v, cfg), cfg


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, F).view(np.int32), np.ascontiguousarray(b, F).view(np.int32))


def _constants(cfg):
    return (F(cfg["lr"] / (1.0 - cfg["betas"][0] ** cfg["step"])), F(np.sqrt(1.0 - cfg["betas"][1] ** cfg["step"])))


def test_every_regime_does_what_its_name_says():
    (p, g, m, v), (p1, m1, v1), cfg = _after("ordinary")
    assert np.isfinite(p1).all() and (1e-6 <= np.abs(g)).all() and (np.abs(g) <= 1).all()
    assert not _same_bits(p1, p) and (np.abs(g).min() < 1e-5) and (np.abs(g).max() > 0.1) and (m != 0).all()

    (p, g, m, v), (p1, m1, v1), cfg = _after("zero_all")
    assert not g.any() and not m.any() and not v.any()
    assert _same_bits(p1, p) and not m1.any() and not v1.any()
    for name in A.configs():                                   # 0 / eps, whatever eps, lr and the step are
        assert _same_bits(_after("zero_all", A.configs()[name])[1][0], p), name

    (p, g, m, v), (p1, m1, v1), cfg = _after("zero_grad_warm")
    assert not g.any() and (m != 0).all() and (v > 0).all()
    assert (p1 != p).all() and (np.abs(m1) < np.abs(m)).all() and (v1 < v).all() and (v1 > 0).all()

    (p, g, m, v), (p1, m1, v1), cfg = _after("eps_dominant")
    sqrt_bc2 = _constants(cfg)[1]
    assert cfg["eps"] == 1e-8 and (0.5e-20 <= v).all() and (v <= 1.5e-20).all()
    assert (F(cfg["eps"]) > 10 * np.sqrt(v1) / sqrt_bc2).all()
    assert np.isfinite(p1).all() and not _same_bits(p1, p)
    # ... and eps does reach the result: without it the update is ten times as large
    no_eps = A.restate(p, g, m, v, dict(cfg, eps=0.0))[0]
    assert (np.abs(no_eps - p) > 5 * np.abs(p1 - p)).sum() > 0.9 * K

    for name in ("subnormal_v_in", "subnormal_v_out"):
        for betas in A.BETAS:
            (p, g, m, v), (p1, m1, v1), cfg = _after(name, A.config(betas=betas))
            assert (v1 != 0).all() and (v1 < A.TINY).all() and (v1 > 0).all(), name
            assert np.isfinite(p1).all() and np.isfinite(m1).all(), name
    (p, g, m, v), _, _ = _after("subnormal_v_in")
    assert (v < A.TINY).all() and (v > 0).all() and not g.any()
    (p, g, m, v), _, _ = _after("subnormal_v_out")
    with np.errstate(all="ignore"):
        assert ((g * g * F(1e-3)) < A.TINY).all() and (np.abs(g) >= 0.7e-20).all() and not v.any()

    (p, g, m, v), (p1, m1, v1), cfg = _after("overflow")
    assert (np.abs(g) == F(3e19)).all() and np.isfinite(v).all()
    assert np.isposinf(v1).all() and _same_bits(p1, p) and np.isfinite(m1).all()

    (p, g, m, v), (p1, m1, v1), cfg = _after("inf_v_in")
    assert np.isposinf(v).all() and np.isposinf(v1).all() and _same_bits(p1, p) and np.isfinite(m1).all()

    (p, g, m, v), (p1, m1, v1), cfg = _after("nan_grad")
    assert np.isnan(g).all() and np.isnan(p1).all() and np.isnan(m1).all() and np.isnan(v1).all()

    (p, g, m, v), (p1, m1, v1), cfg = _after("inf_grad")
    assert np.isinf(g).all() and (g > 0).any() and (g < 0).any()
    assert np.isinf(m1).all() and np.isposinf(v1).all() and np.isnan(p1).all()          # inf / inf

    (p, g, m, v), (p1, m1, v1), cfg = _after("neg_zero_p")
    assert (p.view(np.int32) == np.int32(-2 ** 31)).all() and _same_bits(p1, p) and (v1 > 0).all()

    (p, g, m, v), (p1, m1, v1), cfg = _after("lr0")
    assert cfg["lr"] == 0.0 and _same_bits(p1, p) and not _same_bits(m1, m) and not _same_bits(v1, v)


def test_interleaved_fill_puts_four_regimes_into_every_float4_and_a_nan_only_where_it_belongs():
    count = 2049
    ids = A.interleaved_ids(count)
    quads = ids[:count // 4 * 4].reshape(-1, 4)
    assert all(len(set(q.tolist())) == 4 for q in quads)
    for r in range(A.NREG):                                    # every regime at every position of a float4
        assert set((np.flatnonzero(ids == r) % 4).tolist()) == {0, 1, 2, 3}, A.NAMES[r]
    p, g, m, v = A.fill_interleaved(count)
    again = A.fill_interleaved(count)
    assert all(A.first_difference(x, y) is None for x, y in zip((p, g, m, v), again))
    assert A.first_difference(g, A.fill_interleaved(count, seed=1)[1]) is not None
    for name in A.NAMES:                                       # an element is what its regime alone would be
        sel = ids == A.NAMES.index(name)
        alone = A.regime_alone(name, 64)
        for x, y in zip((p, g, m, v), alone):
            assert np.isnan(x[sel]).all() == np.isnan(y).all() and np.isinf(x[sel]).all() == np.isinf(y).all(), name
            assert (x[sel] == 0).all() == (y == 0).all(), name
    for cname, cfg in A.configs().items():
        p1, m1, v1 = A.restate(p, g, m, v, cfg)
        nan_grad, inf_grad = ids == A.NAMES.index("nan_grad"), ids == A.NAMES.index("inf_grad")
        assert np.array_equal(np.isnan(m1), nan_grad) and np.array_equal(np.isnan(v1), nan_grad), cname
        assert np.array_equal(np.isnan(p1), nan_grad | inf_grad), cname      # a NaN stays in its own element
    blocks = A.block_ids(130, shift=5)
    assert (blocks[:64] == 5).all() and (blocks[64:128] == 6).all() and (blocks[128:] == 7).all()
    assert A.fill_blocks(130, 48, shift=5)[0].shape == (130, 48)


def test_float64_form_is_torch_adam():
    """restate64 with its constants left in double against torch.optim.Adam in float64, twenty steps, both beta pairs,
    eps 1e-15 and 1e-8: an independent statement of the formula.  (With ``round_constants`` the two differ by the 6e-8
    of a float32 constant, which is what the kernels' host side does and torch does not.)"""
    torch = pytest.importorskip("torch")
    n, w = 61, 5
    for betas in A.BETAS:
        for eps in (1e-15, 1e-8):
            rng = np.random.RandomState(3)
            p = rng.randn(n, w)
            m, v = np.zeros_like(p), np.zeros_like(p)
            tp = torch.from_numpy(p.copy()).requires_grad_()
            lr = A.lr32(1e-3)
            opt = torch.optim.Adam([tp], lr=lr, betas=betas, eps=eps, foreach=False)
            for step in range(1, 21):
                g = A.regime_alone("ordinary", n * w, seed=step)[1].astype(np.float64).reshape(n, w)
                tp.grad = torch.from_numpy(g.copy())
                opt.step()
                p, m, v = A.restate64(p, g, m, v, A.config(step=step, betas=betas, eps=eps, lr=lr),
                                      round_constants=False)
                st = opt.state[tp]
                np.testing.assert_allclose(p, tp.detach().numpy(), rtol=1e-12, atol=0)
                np.testing.assert_allclose(m, st["exp_avg"].numpy(), rtol=1e-12, atol=0)
                np.testing.assert_allclose(v, st["exp_avg_sq"].numpy(), rtol=1e-12, atol=0)
            p0 = np.random.RandomState(3).randn(n, w)
            assert (p != p0).all() and np.abs(p - p0).max() > 1e-3                  # every parameter did move


def regime_distances():
    """name -> (dp, dm, dv): the largest |float32 restatement - float64 form| of the regime's finite elements, in float32
    ulps of the larger of the output and the terms it is summed from (p: p and p1; m: m, g (1 - b1) and m1 -- the lerp
    cancels where g is near -9 m; v: v1, a sum of positives); None where the regime has no finite element of that
    output"""
    out = {}
    for name in A.NAMES:
        p, g, m, v = A.regime_alone(name, K)
        cfg = A.regime_config(name)
        r32, r64 = A.restate(p, g, m, v, cfg), A.restate64(p, g, m, v, cfg)
        row = []
        omb1 = 1.0 - cfg["betas"][0]
        with np.errstate(all="ignore"):
            scales = (np.maximum(np.abs(p), np.abs(r64[0])), np.maximum.reduce([np.abs(m), np.abs(g * omb1), np.abs(r64[1])]),
                      np.abs(r64[2]))
        finite = np.isfinite(r32[0]) & np.isfinite(r32[1]) & np.isfinite(r32[2])      # (float64 does not overflow at 3e19)
        for a, b, scale in zip(r32, r64, scales):
            ok = finite & np.isfinite(b) & np.isfinite(scale)
            if not ok.any():
                row.append(None)
                continue
            ulp = np.spacing(np.abs(scale[ok]).astype(F)).astype(np.float64)
            row.append(float((np.abs(a[ok].astype(np.float64) - b[ok]) / ulp).max()))
        out[name] = tuple(row)
    return out


def test_float32_restatement_stays_within_its_rounding_of_the_float64_form():
    """On the elements whose three float32 outputs are finite.  m and v are three and four roundings of terms no larger
    than the scale: 2 ulp; p adds the rounding of the update's six operations, at most a few ulp of an update that is
    itself far below p: 2 ulp of p.  The figures are printed."""
    d = regime_distances()
    print()
    for name, (dp, dm, dv) in d.items():
        fmt = lambda x: "  none" if x is None else "%6.2f" % x
        print("  %-16s p %s ulp   m %s ulp   v %s ulp" % (name, fmt(dp), fmt(dm), fmt(dv)))
    for name, row in d.items():
        for x, lim in zip(row, (2.0, 2.0, 2.0)):
            assert x is None or x <= lim, (name, row)
    for name in ("nan_grad", "inf_grad", "overflow", "inf_v_in"):
        assert d[name] == (None, None, None), name


def test_table_reaches_every_branch():
    """From the table's own counts and widths: a later edit cannot silently lose a branch."""
    dense = set().union(*(A.dense_branches(c) for c in A.COUNTS))
    want_dense = {"float4", "tail1", "tail2", "tail3", "ends_on_workgroup", "one_past_workgroup", "blocks>1"}
    assert dense == want_dense
    assert any(A.dense_branches(c) == {"tail%d" % c} for c in (1, 2, 3) if c in A.COUNTS)      # a tail with no body
    assert all(c in A.COUNTS for c in (1, 2, 3))
    # the 8-record launch: a zero-count record BETWEEN two others, records that end on and one past a workgroup, every tail
    L = A.LAUNCH8
    assert len(L) == 8 and 0 in L[1:-1] and L[L.index(0) - 1] > 0 and L[L.index(0) + 1] > 0
    assert set().union(*(A.dense_branches(c) for c in L)) == want_dense - {"tail2"}
    blocks = [(c + A.PER_BLOCK - 1) // A.PER_BLOCK for c in L]
    assert sum(blocks) > len(L) and max(blocks) >= 2 and blocks.count(1) >= 4     # first_block is no identity map
    # FusedAdam: more records than one launch holds
    flat = [c for grp in A.FUSED12 for c in grp]
    assert len(A.FUSED12) == 3 and all(len(g) == 4 for g in A.FUSED12) and len(flat) == 12 > 8
    assert set().union(*(A.dense_branches(c) for c in flat)) == want_dense
    # the masked kernel: a row boundary at each of the four positions of a float4, at every width that can have one
    # there, and every other branch of the walk
    every = set()
    for w in A.WIDTHS:
        got = set().union(*(A.masked_branches(n, w) for n in A.ROWS))
        every |= got
        want = {"boundary%d" % q for q in range(4) if any((r * w) % 4 == q for r in range(1, 5))}
        assert {b for b in got if b.startswith("boundary") and len(b) == 9} == want, w
        assert {"float4", "blocks>1"} <= got, w
        if w % 4:
            assert {"tail1", "tail2", "tail3"} & got, w
        if w % 2:
            assert {"tail1", "tail2", "tail3"} <= got, w
        if w > 4 and w % 4:
            assert "wide_row_ends_mid_float4" in got, w
    assert every >= want_dense - {"ends_on_workgroup", "one_past_workgroup"} | {
        "boundary0", "boundary1", "boundary2", "boundary3", "four_rows_in_float4", "boundary_in_tail",
        "wide_row_ends_mid_float4"}
    assert {2, 5, 7} <= set(A.WIDTHS) and {3, 12, 27, 48} == set(A.SH_DIMS)
    assert set(A.LAUNCH8_MASKED_WIDTHS) <= set(A.WIDTHS) and len(A.LAUNCH8_MASKED_WIDTHS) == 8
    # the masks: the boundary between a visible and an invisible row at every position of a float4 a row can start at
    # ("mod" alone does it wherever width + 1 is odd; at widths 1, 3, 5, 7, 9 and 45 its period is even and "alternating"
    # and "random_half" supply the other positions)
    for w in A.WIDTHS:
        n, at = max(A.ROWS), {}
        for name, vis in A.masks(n, w).items():
            edges = np.flatnonzero(vis[1:] != vis[:-1]) + 1                  # rows at which visibility changes
            at[name] = set(((edges * w) % 4).tolist())
        possible = {(r * w) % 4 for r in range(1, 5)}
        assert at["mod"] | at["alternating"] | at["random_half"] == possible, w
        if (w + 1) % 2:
            assert at["mod"] == possible, w
    assert set(A.masks(65, 3)) == {"none", "first", "last", "alternating", "random_half", "run_aligned",
                                   "run_straddling", "all", "mod"}
    # the factored pair: row counts around a 64-row workgroup, a whole workgroup invisible with a visible one beside it
    assert {1, 63, 64, 65, 130} == set(A.SH_ROWS)
    for n in (65, 130):
        out = A.sh_masks(n)["workgroup_out"]
        gone = [b for b in range((n + 63) // 64) if not out[64 * b:64 * b + 64].any()]
        assert len(gone) == 1 and out.any(), n
    assert set(A.STEPS) == {1, 2, 10, 1000, 1000000} and set(A.BETAS) == {(0.9, 0.999), (0.5, 0.9)}
    cfgs = A.configs()
    assert {c["step"] for c in cfgs.values()} >= set(A.STEPS) and {c["eps"] for c in cfgs.values()} == {1e-15, 1e-8}
    assert any(c["lr"] == 0.0 for c in cfgs.values())
    assert all(c["lr"] == float(F(c["lr"])) for c in cfgs.values())      # what the ABI's float carries
