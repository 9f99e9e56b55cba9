"""The four Adam kernels -- k_adam<false> (``egs_adam_step``), k_adam<true> (``egs_sparse_adam_step``),
k_adam_sh_factored<NC, false> (``egs_adam_sh_factored``) and k_adam_sh_factored<NC, true>
(``egs_sparse_adam_sh_factored``), csrc/egs_adam_device.h -- through the raw C ABI on the hand-built cases of
tests/adam_cases.py, each held to ONE reference: ``sparse_adam_ref.masked_adam_step``, the update restated in float32
operation by operation (``adam_cases.restate``).

The rule.  After every step ``param``, ``exp_avg`` and ``exp_avg_sq`` equal the restatement BIT FOR BIT (compared as
int32; a NaN must sit in the same element, its sign and payload are the one thing the two machines may differ in:
``adam_cases.bits``).  No element is excluded and there is no tolerance.  Each of the three sits between 256-byte guard
bands that must be intact, at a 16-byte aligned address; ``grad`` and the mask are compared before and after; rows a mask
leaves out keep their bits (the restatement says so) and their gradient rows are NaN.  Multi-step cases feed the
restatement its own previous output and compare after every one of twenty steps.  The factored pair gets its gradient
rows from ``egs_sh_grad_views`` on the device (pinned to the oracle's basis in test_gpu_factored_sh.py), copied to the
host and fed to the restatement.

Why exact: the build keeps float32 subnormals, divides and takes roots correctly rounded (no fast-math flag), and
``adam1`` carries ``#pragma clang fp contract(off)``; ``lr`` crosses the ABI as a float, so the cases use float32 values
(``adam_cases.lr32``) and the references divide that value by 1 - b1^t in double, as ``adam_bias`` does.

The float32 restatement's own distance from the float64 form of the formula (``adam_cases.restate64``), measured on the CPU
by tests/test_adam_cases_cpu.py on 4096 elements per regime under the regime's own configuration, largest over the
elements whose float32 outputs are finite, in float32 ulps of the output's scale (p / m / v):
    ordinary 0.75 / 1.74 / 1.39      zero_all 0 / 0 / 0                zero_grad_warm 0.52 / 0.52 / 0.50
    eps_dominant 0.50 / 1.05 / 0.98  subnormal_v_in 0.49 / 0.52 / 0.50  subnormal_v_out 0.50 / 0.47 / 0.50
    neg_zero_p 0 / 0 / 0.50          lr0 0 / 1.48 / 1.34
    overflow, inf_v_in, nan_grad, inf_grad: no finite element (float64 does not overflow at g = 3e19; the float32 result
    there is decided by the regime's own assertions on the CPU)

Measured on MI355X: all 63 tests pass with zero elements excluded -- exact equality holds on the card for all four
kernels, so no output falls back to a tolerance and csrc is unchanged but for the alignment check of ``egs_adam_step``.
Launches compared, each on all of param / exp_avg / exp_avg_sq:
  dense    132 one-record launches (12 configurations x 11 counts, 1 .. 2049 floats), 12 regimes alone at 1027 floats, 4
           eight-record launches (1, 1024, 3, 1025, 0, 4, 2047, 5), 2 x 20 steps at 2049 floats
  masked   576 one-group launches (9 widths x 8 row counts x 7 masks up to 64 rows, 9 above; the largest 1031 x 48), 25
           eight-group launches (n 1, 65, 257; widths 1, 2, 3, 4, 5, 7, 9, 45), 20 steps at 257 x 7 with a fresh mask each
  factored 40 dense and 328 masked launches (K 3, 12, 27, 48 x raw / whole x n 1, 63, 64, 65, 130 x the masks), 4 x 20 steps
  FusedAdam  12 tensors x 3 steps (two launches each), one refused step; determinism: 2 x 3 runs
Wall time: the whole module 4.2 s; the slowest test 0.35 s (the first: it loads the libraries), test_masked_one_group[45]
0.22 s, every other below 0.15 s.

Seeded errors (csrc/egs_adam_device.h), each run ONCE on a scratch build; they change values only, every address stays
inside its tensor.  First failing test, then how many of the 63 fail:
  eps under the root      ``sqrtf(v) / sqrt_bc2 + A.eps`` -> ``sqrtf(v + A.eps) / sqrt_bc2``
                          test_dense_one_group[eps_dominant] ("count 1 param": 0x40045a3c for 0x40045a2f); 53 fail
  * sqrt_bc2              ``sqrtf(v) / sqrt_bc2`` -> ``sqrtf(v) * sqrt_bc2``
                          test_dense_one_group[eps_dominant] ("count 1 param": 0x40045621 for 0x40045a2f); 49 fail
  no contraction pragma   ``#pragma clang fp contract(off)`` removed: v * b2 + (g g (1 - b2)) becomes one fma
                          test_dense_one_group[eps_dominant] ("count 4 exp_avg_sq": 0x35827045 for 0x35827044, one ulp, 2
                          of 4 elements); 56 fail
  omb1 in float           ``(float)(1.0 - beta1)`` -> ``1.f - (float)beta1`` (0x3dccccd0 for 0x3dcccccd at beta1 = 0.9;
                          equal at 0.5): test_dense_one_group[eps_dominant] ("count 1 exp_avg": 0x39ee15a6 for
                          0x39ee15a7); 48 fail, every one under betas (0.9, 0.999) -- the (0.5, 0.9) cases pass
  first_block ``>``       ``(int)blockIdx.x >= A.g[k].first_block`` -> ``>``: a record's first workgroup takes the record
                          before it, finds ``e0 >= count`` and returns; the first 1024 floats of every record but the first
                          stay unwritten.  test_dense_eight_records_with_an_empty_one_between[t1_b0] ("record 1 (1024
                          floats) param": 170 of 1024 differ); 8 fail: the four eight-record dense launches, the three
                          eight-group masked ones and the twelve tensors of FusedAdam
  vis[q] dropped          the four ``if (vis[q])`` of k_adam's float4 body removed: test_masked_one_group[1] ("width 1 n 63
                          mask first param": NaN for -0.5023, element 1 -- the invisible rows beside row 0 took their NaN
                          gradient); 11 fail: widths 1, 2, 3, 5, 7, 9, 45, two of the eight-group launches, the masked
                          twenty steps, the determinism test.  Widths 4 and 48 pass, rightly: a float4 never spans two
                          rows there and a lane without a visible row has returned before the body.
NOT run, reasoned (they alter an index, ``row``, ``nel`` or a count and would read or write out of bounds):
  ``q + 1 < nel`` -> ``q < nel``   at the last float4 of a tensor whose last row ends on it the walk reads visible[n], one
                          byte past the mask; inside the tensor it advances ``row`` one element early only at q = 3, which
                          nothing reads -- the values would not change, the read past the mask is the defect
  ``nel`` -> 4            the ragged tail would take the float4 branch and store up to three floats behind the tensor: the
                          guard bands of every count that is no multiple of 4 (``"written outside the tensor"``)
  RowDiv.shift one less   ``row`` doubles: visible[] is read at up to 2 n; where it stays inside, every mask but "all" and
                          "none" fails at the first row boundary (test_masked_one_group, n = 2)
  ``e0 + 4 <= G.count`` -> ``<``  no address changes, the last full float4 goes through the scalar loop: no test can see it
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import adam_cases as A
from tests.loss_abi import guarded, guards_intact

pytestmark = pytest.mark.gpu

F = np.float32


# ------------------------------------------------------------------------------------------------------------- buffers
class Buf:
    """float32 values on the device between guard bands (``written``), or plainly uploaded and compared afterwards"""

    def __init__(self, a, written):
        a = np.ascontiguousarray(a, F)
        self.before, self.written = a.copy(), written
        if written:
            self.whole, inner = guarded(a.size * 4)
            self.t = inner.view(torch.float32)
        else:
            self.whole, self.t = None, torch.empty(max(a.size, 1), dtype=torch.float32, device="cuda")[:a.size]
        if a.size:
            self.t.copy_(torch.from_numpy(a.reshape(-1)))
        self.ptr = self.t.data_ptr() if a.size else None
        assert a.size == 0 or self.ptr % 16 == 0, "the test's own buffer is not 16-byte aligned"

    def get(self):
        return self.t.cpu().numpy().reshape(self.before.shape)

    def check(self, what):
        if self.written:
            assert guards_intact(self.whole), "%s: written outside the tensor" % what
        else:
            assert A.first_difference(self.get(), self.before) is None, "%s: a read-only input changed" % what


class Tensor4:
    """param, grad, exp_avg, exp_avg_sq of one record"""

    def __init__(self, p, g, m, v):
        self.p, self.m, self.v = Buf(p, True), Buf(m, True), Buf(v, True)
        self.g = Buf(g, False) if g is not None else None

    def state(self):
        return self.p.get(), self.m.get(), self.v.get()

    def check(self, what):
        for b, nm in ((self.p, "param"), (self.m, "exp_avg"), (self.v, "exp_avg_sq"), (self.g, "grad")):
            if b is not None:
                b.check("%s %s" % (what, nm))


def _mask_buf(vis):
    return torch.from_numpy(np.ascontiguousarray(vis, np.uint8)).cuda()


def _stream(stream):
    return C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)


def expect(got, want, what):
    for x, y, nm in zip(got, want, ("param", "exp_avg", "exp_avg_sq")):
        d = A.first_difference(x, y)
        assert d is None, "%s %s: %s" % (what, nm, d)


@pytest.fixture(scope="module")
def libs():
    from easygaussiansplatting_amd import _adamlib, _lib
    return _lib.load(), _adamlib.load()


# ---------------------------------------------------------------------------------------------------- the four launches
def dense_step(lib, tensors, cfgs, stream=None):
    """egs_adam_step: one record per Tensor4 (an empty one goes down with null pointers), cfgs: one per record"""
    from easygaussiansplatting_amd import _lib
    recs = [_lib.EgsAdamGroup(t.p.ptr, t.g.ptr, t.m.ptr, t.v.ptr, t.p.before.size, c["lr"], c["step"])
            for t, c in zip(tensors, cfgs)]
    c0 = cfgs[0]
    torch.cuda.synchronize()                                  # (the uploads ran on the default stream)
    rc = lib.egs_adam_step(len(recs), (_lib.EgsAdamGroup * len(recs))(*recs), c0["betas"][0], c0["betas"][1], c0["eps"],
                           _stream(stream))
    _lib.check(rc)
    torch.cuda.synchronize()


def masked_step(alib, tensors, widths, n, vis, cfgs, stream=None):
    from easygaussiansplatting_amd import _adamlib
    recs = [_adamlib.EgsSparseAdamGroup(t.p.ptr, t.g.ptr, t.m.ptr, t.v.ptr, w, c["lr"], c["step"])
            for t, w, c in zip(tensors, widths, cfgs)]
    c0 = cfgs[0]
    torch.cuda.synchronize()
    rc = alib.egs_sparse_adam_step(len(recs), (_adamlib.EgsSparseAdamGroup * len(recs))(*recs), n, vis.data_ptr(),
                                   c0["betas"][0], c0["betas"][1], c0["eps"], _stream(stream))
    _adamlib.check(rc)
    torch.cuda.synchronize()


def _group_cfgs(cfg, k):
    """the launch's eps and betas with a learning rate and a step count of its own for each of k records"""
    lrs = (cfg["lr"], 0.0, 5e-2, 1.6e-4, 1e-3)
    return [A.config(eps=cfg["eps"], betas=cfg["betas"], lr=lrs[i % len(lrs)], step=cfg["step"] + (0, 1, 7)[i % 3])
            for i in range(k)]


CONFIGS = A.configs()


# ------------------------------------------------------------------------------------------------------ the dense kernel
@pytest.mark.parametrize("cname", sorted(CONFIGS))
def test_dense_one_group(libs, cname):
    """One record, every count of the table: the float4 body, the scalar tail of 1, 2 and 3, a count that ends on and
    one past a workgroup, more than one workgroup -- under every configuration (five step counts, two beta pairs, both
    eps, lr == 0, the regimes' own)."""
    cfg = CONFIGS[cname]
    for count in A.COUNTS:
        p, g, m, v = A.fill_interleaved(count, seed=count)
        t = Tensor4(p, g, m, v)
        dense_step(libs[0], [t], [cfg])
        expect(t.state(), A.restate(p, g, m, v, cfg), "%s count %d" % (cname, count))
        t.check("%s count %d" % (cname, count))


@pytest.mark.parametrize("name", A.NAMES)
def test_dense_regime_alone_under_its_own_configuration(libs, name):
    cfg = A.regime_config(name)
    p, g, m, v = A.regime_alone(name, 1027)
    t = Tensor4(p, g, m, v)
    dense_step(libs[0], [t], [cfg])
    expect(t.state(), A.restate(p, g, m, v, cfg), name)
    t.check(name)


@pytest.mark.parametrize("cname", ["t1_b0", "t10_b1", "eps_dominant", "lr0"])
def test_dense_eight_records_with_an_empty_one_between(libs, cname):
    """(1, 1024, 3, 1025, 0, 4, 2047, 5) in one launch, each record with its own lr and step: ``first_block`` is no
    identity map, the empty record is compacted away (null pointers), and every record's neighbours keep their guards."""
    cfgs = _group_cfgs(CONFIGS[cname], 8)
    start = [A.fill_interleaved(c, seed=10 + i) for i, c in enumerate(A.LAUNCH8)]
    ts = [Tensor4(*s) for s in start]
    assert ts[4].p.ptr is None
    dense_step(libs[0], ts, cfgs)
    for i, (t, s, c) in enumerate(zip(ts, start, cfgs)):
        what = "%s record %d (%d floats)" % (cname, i, A.LAUNCH8[i])
        expect(t.state(), A.restate(*s, c), what)
        t.check(what)


def test_dense_twenty_steps(libs):
    """Twenty steps on 2049 floats with every regime in it, the restatement fed its own output; every step compared."""
    for betas, eps in zip(A.BETAS, (1e-15, 1e-8)):
        count = 2049
        p, _, m, v = A.fill_interleaved(count)
        t = Tensor4(p, np.zeros(count, F), m, v)
        for step in range(1, 21):
            cfg = A.config(step=step, betas=betas, eps=eps)
            g = A.fill_interleaved(count, seed=step)[1]
            t.g = Buf(g, False)
            dense_step(libs[0], [t], [cfg])
            p, m, v = A.restate(p, g, m, v, cfg)
            expect(t.state(), (p, m, v), "betas %s step %d" % (betas, step))
            t.check("step %d" % step)
        assert np.isfinite(p).sum() > count // 2 and np.isnan(p).any()


# ----------------------------------------------------------------------------------------------------- the masked kernel
def _masked_case(alib, n, width, vis, cfg, seed, what, stream=None):
    p, g, m, v = A.fill(A.interleaved_ids(n * width).reshape(n, width), seed)
    g = g.copy()
    g[~vis] = np.nan                                          # an invisible row's gradient is never read
    t = Tensor4(p, g, m, v)
    d_vis = _mask_buf(vis)
    masked_step(alib, [t], [width], n, d_vis, [cfg], stream)
    want = A.restate(p, g, m, v, cfg, vis)
    got = t.state()
    expect(got, want, what)
    for x, before, nm in zip(got, (p, m, v), ("param", "exp_avg", "exp_avg_sq")):      # said once more, on its own
        assert A.first_difference(x[~vis], before[~vis]) is None, "%s %s: an invisible row changed" % (what, nm)
    t.check(what)
    assert np.array_equal(d_vis.cpu().numpy() != 0, vis), "%s: the mask changed" % what
    return got


@pytest.mark.parametrize("width", A.WIDTHS)
def test_masked_one_group(libs, width):
    """Every width x row count x mask: RowDiv's magic multiply, the walk of rem / row across a float4 (a row boundary at
    each position, four rows in a float4 at width 1, wide rows ending mid-float4), ``nel`` and the ragged tail."""
    cfgs = [CONFIGS[k] for k in sorted(CONFIGS)]
    i = 0
    for n in A.ROWS:
        for mname, vis in A.masks(n, width).items():
            cfg = cfgs[i % len(cfgs)]
            i += 1
            _masked_case(libs[1], n, width, vis, cfg, seed=i, what="width %d n %d mask %s" % (width, n, mname))


@pytest.mark.parametrize("n", [1, 65, 257])
def test_masked_eight_groups(libs, n):
    """Eight groups of one row count in one launch (widths 1, 2, 3, 4, 5, 7, 9, 45), each with its own lr and step."""
    widths = A.LAUNCH8_MASKED_WIDTHS
    for mname, vis in A.masks(n, 3).items():
        cfgs = _group_cfgs(CONFIGS["t2_b1"], 8)
        start = []
        for i, w in enumerate(widths):
            p, g, m, v = A.fill(A.interleaved_ids(n * w).reshape(n, w), seed=20 + i)
            g = g.copy()
            g[~vis] = np.nan
            start.append((p, g, m, v))
        ts = [Tensor4(*s) for s in start]
        masked_step(libs[1], ts, widths, n, _mask_buf(vis), cfgs)
        for i, (t, s, c) in enumerate(zip(ts, start, cfgs)):
            what = "n %d mask %s group %d (width %d)" % (n, mname, i, widths[i])
            expect(t.state(), A.restate(*s, c, vis), what)
            t.check(what)


def test_masked_twenty_steps(libs):
    n, width = 257, 7
    ids = A.interleaved_ids(n * width).reshape(n, width)
    p, _, m, v = A.fill(ids)
    t = Tensor4(p, np.zeros((n, width), F), m, v)
    rng = np.random.RandomState(5)
    for step in range(1, 21):
        cfg = A.config(step=step, eps=1e-8)
        vis = rng.rand(n) < 0.5
        g = A.fill(ids, seed=step)[1].copy()
        g[~vis] = np.nan
        t.g = Buf(g, False)
        masked_step(libs[1], [t], [width], n, _mask_buf(vis), [cfg])
        p, m, v = A.restate(p, g, m, v, cfg, vis)
        expect(t.state(), (p, m, v), "step %d" % step)
        t.check("step %d" % step)


# ---------------------------------------------------------------------------------------------------------- determinism
def test_second_run_and_side_stream_give_the_same_bits(libs):
    cfg = CONFIGS["t10_b0"]
    side = torch.cuda.Stream()
    count = 2049
    start = A.fill_interleaved(count, seed=3)
    runs = []
    for stream in (None, None, side):
        t = Tensor4(*start)
        torch.cuda.synchronize()
        dense_step(libs[0], [t], [cfg], stream)
        runs.append(t.state())
    n, width = 257, 5
    vis = A.masks(n, width)["random_half"]
    masked = [_masked_case(libs[1], n, width, vis, cfg, 4, "run %d" % i, stream)
              for i, stream in enumerate((None, None, side))]
    for r in (runs, masked):
        for other, nm in ((r[1], "second run"), (r[2], "side stream")):
            expect(other, r[0], nm)


# ---------------------------------------------------------------------------------------------------- the factored pair
def _factored_case(libs, n, K, raw, vis, shift, steps=1):
    """-> nothing; asserts.  vis None: the dense entry point."""
    from easygaussiansplatting_amd import _adamlib, _lib
    lib, alib = libs
    V = 2
    stride = (3 * n + 6) // 4 * 4
    rng = np.random.RandomState(1000 * K + n + shift)
    pws = (rng.randn(n, 3) * 3).astype(F)
    d_pws = torch.from_numpy(pws).cuda()
    widths = (3, K - 3) if (raw and K > 3) else (K,)
    cols = (0, 3) if len(widths) == 2 else (0,)
    whole = A.fill_blocks(n, K, seed=shift, shift=shift)                     # the moments in the regime block layout
    state = [tuple(x[:, c:c + w] for x in (whole[0], whole[2], whole[3])) for c, w in zip(cols, widths)]
    ts = [Tensor4(s[0], None, s[1], s[2]) for s in state]
    what0 = "K %d n %d %s %s" % (K, n, "raw" if raw else "whole", "dense" if vis is None else "masked")
    for step in range(1, steps + 1):
        base = A.config(step=step + 2, eps=(1e-15, 1e-8)[shift % 2], betas=A.BETAS[(shift // 2) % 2])
        cfgs = [base, A.config(eps=base["eps"], betas=base["betas"], step=base["step"] + 5, lr=5e-5)]
        # dL/dcolour of two views: the first carries the regime block's own gradients (zero, 1e-20, 3e19, inf, NaN ...),
        # the second an ordinary one with every third row zero
        rows = np.full((V, stride), np.nan, F)                                # (the padding is never read)
        d0 = A.fill_blocks(n, 3, seed=100 * step + shift, shift=shift)[1]
        d1 = (rng.randn(n, 3) * 1e-3).astype(F)
        d1[::3] = 0.0
        if vis is not None:
            d0[~vis] = np.nan
            d1[~vis] = np.nan
        rows[0, :3 * n], rows[1, :3 * n] = d0.reshape(-1), d1.reshape(-1)
        rows[:, 3 * n:3 * n + 3] = (rng.randn(V, 3) * 6).astype(F)
        d_rows = torch.from_numpy(rows).cuda()
        grads = [torch.full((n, w), 7.0, device="cuda") for w in widths]
        st = _stream(None)
        _lib.check(lib.egs_sh_grad_views(n, K, V, d_pws.data_ptr(), d_rows.data_ptr(), stride, 0.5, grads[0].data_ptr(),
                                         grads[1].data_ptr() if len(grads) > 1 else None, 0, st))
        torch.cuda.synchronize()
        g_host = [g.cpu().numpy() for g in grads]
        recs = [_lib.EgsAdamGroup(t.p.ptr, None, t.m.ptr, t.v.ptr, n * w, c["lr"], c["step"])
                for t, w, c in zip(ts, widths, cfgs)]
        low = C.byref(recs[0])
        if len(recs) > 1:
            high = C.byref(recs[1])
        elif raw:                                   # K == 3 in the raw layout: high_shs is [n][0] and must be ignored
            high = C.byref(_lib.EgsAdamGroup(None, None, None, None, 0, 1.0, 1))
        else:
            high = None
        b1, b2 = base["betas"]
        if vis is None:
            _lib.check(lib.egs_adam_sh_factored(n, K, V, d_pws.data_ptr(), d_rows.data_ptr(), stride, 0.5, low, high, b1,
                                                b2, base["eps"], st))
        else:
            d_vis = _mask_buf(vis)
            _adamlib.check(alib.egs_sparse_adam_sh_factored(n, K, V, d_pws.data_ptr(), d_rows.data_ptr(), stride, 0.5, low,
                                                            high, d_vis.data_ptr(), b1, b2, base["eps"], st))
        torch.cuda.synchronize()
        for i, (t, w, c) in enumerate(zip(ts, widths, cfgs)):
            what = "%s step %d tensor %d" % (what0, step, i)
            state[i] = A.restate(state[i][0], g_host[i], state[i][1], state[i][2], c, vis)
            expect(t.state(), state[i], what)
            t.check(what)
        assert A.first_difference(d_rows.cpu().numpy(), rows) is None and A.first_difference(d_pws.cpu().numpy(), pws) is None
        if vis is not None:
            assert np.array_equal(d_vis.cpu().numpy() != 0, vis)


@pytest.mark.parametrize("K", A.SH_DIMS)
@pytest.mark.parametrize("raw", [False, True])
def test_factored_dense(libs, raw, K):
    for i, n in enumerate(A.SH_ROWS):
        _factored_case(libs, n, K, raw, None, shift=3 * i + A.SH_DIMS.index(K))


@pytest.mark.parametrize("K", A.SH_DIMS)
@pytest.mark.parametrize("raw", [False, True])
def test_factored_masked(libs, raw, K):
    i = 0
    for n in A.SH_ROWS:
        for mname, vis in A.sh_masks(n).items():
            _factored_case(libs, n, K, raw, vis, shift=i)
            i += 1


@pytest.mark.parametrize("masked", [False, True])
def test_factored_twenty_steps(libs, masked):
    n = 130
    _factored_case(libs, n, 48, True, A.sh_masks(n)["random_half"] if masked else None, shift=0, steps=20)
    _factored_case(libs, n, 27, False, A.sh_masks(n)["workgroup_out"] if masked else None, shift=4, steps=20)


# ------------------------------------------------------------------------------------------------------ through FusedAdam
def _fused12(eps, betas, lrs=(1e-3, 0.0, 5e-2)):
    from easygaussiansplatting_amd.optim import FusedAdam
    start, params, groups = [], [], []
    for gi, counts in enumerate(A.FUSED12):
        ps = []
        for ti, c in enumerate(counts):
            s = A.fill_interleaved(c, seed=40 + 4 * gi + ti)
            start.append(s)
            ps.append(torch.from_numpy(s[0].copy()).cuda().requires_grad_())
        params += ps
        groups.append({"params": ps, "lr": lrs[gi], "name": "g%d" % gi})
    opt = FusedAdam(groups, eps=eps, betas=betas)
    for k, (p, s) in enumerate(zip(params, start)):
        opt.state[p] = {"step": k, "exp_avg": torch.from_numpy(s[2].copy()).cuda(),
                        "exp_avg_sq": torch.from_numpy(s[3].copy()).cuda()}
    lr_of = [A.lr32(lrs[gi]) for gi, counts in enumerate(A.FUSED12) for _ in counts]
    return opt, params, start, lr_of


def _fused_state(opt, p):
    st = opt.state[p]
    return p.detach().cpu().numpy(), st["exp_avg"].cpu().numpy(), st["exp_avg_sq"].cpu().numpy()


def test_fused_adam_twelve_tensors_two_launches(libs):
    """3 groups x 4 tensors: 12 records, two launches; a tensor without a gradient stays out (bits and step count); a
    non-contiguous ``.grad`` is taken by value; three steps."""
    eps, betas = 1e-8, (0.5, 0.9)
    opt, params, start, lr_of = _fused12(eps, betas)
    ref = [(s[0], s[2], s[3]) for s in start]
    skipped = 6                                                # params[6]: 2047 floats, second group
    for it in range(1, 4):
        grads = []
        for k, (p, s) in enumerate(zip(params, start)):
            g = A.fill_interleaved(s[0].size, seed=50 * it + k)[1]
            grads.append(g)
            if k == skipped:
                p.grad = None
            elif k % 3 == 1:                                   # every other element of a buffer twice the size
                wide = torch.zeros(2 * g.size, device="cuda")
                wide[::2] = torch.from_numpy(g).cuda()
                p.grad = wide[::2]
                assert not p.grad.is_contiguous() or g.size == 1
            else:
                p.grad = torch.from_numpy(g).cuda()
        opt.step()
        torch.cuda.synchronize()
        for k, p in enumerate(params):
            what = "step %d tensor %d (%d floats)" % (it, k, start[k][0].size)
            if k != skipped:
                cfg = A.config(step=k + it, lr=lr_of[k], eps=eps, betas=betas)
                ref[k] = A.restate(ref[k][0], grads[k], ref[k][1], ref[k][2], cfg)
            assert opt.state[p]["step"] == (k if k == skipped else k + it), what
            expect(_fused_state(opt, p), ref[k], what)


def test_fused_adam_refused_step_leaves_every_counter(libs):
    """A step the C side refuses (an SH width the factored entry point does not have: 3 + 3) raises, moves no tensor and
    leaves every ``state[...]["step"]`` where it was -- the twelve plain tensors' as well, none of which was launched."""
    opt, params, start, _ = _fused12(1e-15, (0.9, 0.999))
    n = 16
    low, high = (torch.zeros(n, 3, device="cuda").requires_grad_() for _ in range(2))
    opt.param_groups[0]["params"].append(low)
    opt.param_groups[1]["params"].append(high)
    for p, s in zip(params, start):
        p.grad = torch.from_numpy(s[1].copy()).cuda()
    pws = torch.zeros(n, 3, device="cuda")
    rows = torch.zeros(1, 3 * n + 4, device="cuda")
    with pytest.raises(RuntimeError, match="bad argument.*sh_dim"):
        opt.step(factored_sh=(rows, 1.0, pws, low, high))
    torch.cuda.synchronize()
    for k, (p, s) in enumerate(zip(params, start)):
        assert opt.state[p]["step"] == k, k
        expect(_fused_state(opt, p), (s[0], s[2], s[3]), "tensor %d after the refused step" % k)
    for t in (low, high):
        assert opt.state[t]["step"] == 0 and not t.detach().any()
    # and the same optimizer still steps
    opt.param_groups[0]["params"].pop()
    opt.param_groups[1]["params"].pop()
    opt.step()
    torch.cuda.synchronize()
    assert [opt.state[p]["step"] for p in params] == [k + 1 for k in range(12)]
