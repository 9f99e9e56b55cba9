"""The densification kernels of csrc/egs_density.hip (k_density_accum, k_densify_classify, k_densify_scan,
k_densify_apply, k_reset_alpha) row by row, by size and class pattern, against oracle/density_oracle.py in float64.
The cases are those of tests/density_cases.py (checked without a GPU by tests/test_density_cases_cpu.py).

MATRIX
  sizes     1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513 (wave and workgroup edges); 65 535, 65 536, 65 537 (256 | 256 |
            257 workgroups: the last single-round scan of k_densify_scan and the first carry); 131 073 (513 workgroups: a
            third round with one live lane)
  A  test_abi_sizes      every size x {iid, block, all3}, hw 45, with moments
     test_abi_patterns   the other eight patterns at n = 257, 513, 65 537, hw 45, with moments
     test_abi_widths     hw {0, 9, 24, 45} x moments {yes, no} x noise {table, generator} x n {3, 257, 513} x {iid, block}
     test_abi_edges      ``density_cases.edges`` (rows ON the thresholds, zero quaternions, alphas_raw = 20) at hw 45, 0
     test_abi_is_deterministic   two runs, every output bitwise equal
  B  test_control_*      DensityControl.update_gaussian_density with FusedAdam / torch.optim.Adam at n = 257, 65 537, iid;
                         hw 0 with and without moments (``density._pset`` hands a null pointer for the empty tensor)
     test_statistics_*   update_density_info, three views, n = 1, 63, 65, 257, 513, masks as bool / uint8 / int64 / float32
     test_reset_alpha_*  egs_reset_alpha at the same sizes, with and without moments

SURFACE A is the C ABI alone (egs_densify_plan, then egs_densify_apply); every output sits in a tests/gpu_abi.Out buffer
between sentinel bands.  Asserted, no row and no case left out: ``cls`` equals the oracle's classes byte for byte, the
bytes behind row n - 1 and the bands untouched; ``totals`` == (keep, clone, split, prune); the scanned workgroup offsets
in the workspace (checked BEFORE apply runs, so that apply's writes are known to stay inside its outputs); moved rows
of all six tensors and both moments bit for bit ``x[remain]`` in order; appended ``low_shs`` / ``high_shs`` bit for bit
the parent's row, clones first, then split children by parent index; appended moments exactly zero; every word of
every output written (the outputs start as NaN sentinels, which fail every comparison); every band untouched, those of
a width-0 tensor and of n_out == 0 included.

RULE for the appended rows of pws, alphas_raw, scales_raw, rots_raw (tests/test_gpu_mcmc.py, tests/
test_gpu_pergaussian_matrix.py): the row's error against the float64 oracle, relative to max_j |ref row|, is at most
max(FLOOR, 2 x the float32 distance of THAT row); FLOOR = 1e-5 as in test_gpu_pergaussian_matrix.py.  For the one-column
alphas_raw the error is relative to max(1, |ref|): the logit's error is absolute near a = 0.  The distance is taken on
the reference alone (``density_cases.distances``): the float32 oracle, and four float32 evaluations of inputs one ulp
away, against the float64 oracle.  Rows whose float32 value is not finite (a parent with alphas_raw = 20: float32
sigmoid rounds to 1 and the child gets +inf, in the reference's own torch code as well) must equal the float32 oracle
exactly; that is the reference's behaviour, asserted as it is.  The generator runs are held to the oracle fed
``scene.normal(seed, round, (3 n,))`` by the same rule.

FLOAT32 DISTANCE, CPU, largest row over the 70 cases of A (as given | with the one-ulp moves):
  pws 2.2e-6 | 5.7e-6   alphas_raw 6.7e-5 | 6.7e-5   scales_raw 9.7e-8 | 1.8e-7   rots_raw 1.6e-7 | 2.9e-7
DEVICE ERROR, MI355X, largest row over all cases of A and B (error | error / bound; each case prints its own, and
``test_zz_report`` the maxima of the run):
  pws 2.2e-6 | 0.19   alphas_raw 6.7e-5 | 0.52   scales_raw 1.9e-7 | 0.019   rots_raw 1.6e-7 | 0.016
The device stands where the float32 oracle stands: logit(sigmoid(a)) loses its digits in 1 - sigmoid(a) on either, the
rest is the floor's.

MUTATIONS, each on a scratch build of the library, each run once against the narrowest tests.  All five only make
offsets or counts smaller, or leave writes out: no write can leave its allocation, no loop gets longer; the first
three fail on plan's outputs, before apply is launched.
  k_densify_scan      drop ``carry += tot``            caught at EVERY size, not only beyond 256 workgroups: the totals
                                                       are the carries, so they read 0.  test_abi_sizes[1-all3],
                                                       [257-iid], [511-all3]: "totals"
  k_densify_scan      ``arr[i] = carry + ex`` -> ``ex``  (the carry dropped from the offsets alone)  test_abi_sizes
                                                       [65536-iid] passes; [65537-iid] "3 workgroup offsets differ;
                                                       first: field 0 of workgroup 256 is 0, not 49170"; [131073-iid]
                                                       "771 workgroup offsets differ; first: field 0 of workgroup 256"
  k_densify_classify  ``total >> 20`` -> ``& 255``     test_abi_sizes[256-all3] and [65535-block] "totals" (a workgroup of
                                                       256 splits counts 0); [256-iid] and [65535-iid] pass: only the
                                                       whole-workgroup patterns see it
  k_densify_apply     split destination without        test_abi_sizes[513-iid]: low_shs "196 appended rows are not their
                      ``A.n_clone +``                  parent's row; first: appended row 3 (clone of parent 13)"
  k_densify_apply     appended moments not zeroed      test_abi_sizes[513-iid]: pws exp_avg "759 words of the appended
                                                       rows are not zero, first in appended row 0" (the sentinels).
                                                       test_control_matches_the_oracle_row_by_row[257-fused] failed
                                                       too, on whatever torch.empty held: surface B may see it or not
NOT run, reasoned: a split destination that is too LARGE, a lengthened scan loop, a class byte written one row late;
each could write outside an allocation.  The band checks and the offsets check in front of apply are what would
show them.

FOUND: nothing.  All 102 tests passed on the first complete run on the MI355X; no kernel, ``density.py`` or oracle line
was changed for them (the oracle gained its float64 mode, bit-identical in float32).
"""
import collections
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from easygaussiansplatting_amd import scene as S
from oracle import density_oracle as D
from tests import density_cases as DC
from tests.gpu_abi import BAND, DEV, Out, _check, _stream

pytestmark = pytest.mark.gpu

F = np.float32
NAMES = DC.NAMES
FLOOR = 1e-5
LRS = (0.001, 0.001, 0.001 / 20, 0.05, 0.005, 0.001)
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 65_535, 65_536, 65_537, 131_073)
MAIN = ("iid", "block", "all3")
OTHERS = tuple(p for p in DC.PATTERNS if p not in MAIN)
THR = (D.logit(DC.TH.alpha), math.log(DC.TH.big), DC.TH.grad, DC.TH.scale)      # as density.py hands them over

worst = collections.defaultdict(float)              # (tensor, what) -> largest figure over the tests run so far


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from easygaussiansplatting_amd import _lib
    return _lib.load()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, F).reshape(-1).view(np.int32)


# ------------------------------------------------------------------------------------------------------- expectations
class Expect:
    """what the oracle says about one case: classes, counts, the appended rows in float64 and float32, their float32
    distance row by row"""

    def __init__(self, case):
        self.case = case
        self.cls = DC.oracle_classes(case)
        remain = self.cls >= 1
        self.info = dict(remain=remain, clone=np.nonzero(self.cls == DC.CLONE)[0], split=np.nonzero(self.cls == DC.SPLIT)[0])
        self.nk, self.nc, self.ns = int(remain.sum()), len(self.info["clone"]), len(self.info["split"])
        self.n_out = self.nk + self.nc + self.ns
        self.parents = np.concatenate([self.info["clone"], self.info["split"]])
        self.ref = DC.appended_reference(case, self.info)
        self.f32 = DC.appended_reference(case, self.info, F)
        self.dist = DC.distances(case, self.info)


@functools.lru_cache(maxsize=2)
def _case(n, hw, pattern):
    case = DC.edges(hw) if pattern == "edges" else DC.build(n, hw, pattern, DC.case_seed(n, pattern))
    np.testing.assert_array_equal(DC.oracle_classes(case), case["cls"])
    return case, Expect(case)


def check_result(tag, ex, got, got_m, got_v):
    """``got`` / ``got_m`` / ``got_v``: name -> [n_out, w] float32 as the device left them (moments None: no state)"""
    case = ex.case
    nk, remain, parents = ex.nk, ex.info["remain"], ex.parents
    for j, k in enumerate(NAMES):
        w = case["params"][k].shape[1]
        assert got[k].shape == (ex.n_out, w), (tag, k, got[k].shape)
        # moved rows: the stored bits, in order
        assert np.array_equal(_bits(got[k][:nk]), _bits(case["params"][k][remain])), (tag, k, "moved rows differ")
    # appended SH rows: the parent's, clones first, then split children by parent index
    for k in ("low_shs", "high_shs"):
        a, b = got[k][nk:], case["params"][k][parents]
        w = b.shape[1]
        rows = np.nonzero((_bits(a).reshape(len(b), w) != _bits(b).reshape(len(b), w)).any(1))[0]
        assert rows.size == 0, (tag, k, "%d appended rows are not their parent's row; first: appended row %d (%s of "
                                "parent %d)" % (rows.size, rows[0], "clone" if rows[0] < ex.nc else "split child",
                                                parents[rows[0]]))
    # moments: moved with their row; exactly zero on the appended rows
    for j, k in enumerate(NAMES):
        w = case["params"][k].shape[1]
        for name, g, old in (("exp_avg", got_m, case["m"]), ("exp_avg_sq", got_v, case["v"])):
            if g is None:
                continue
            assert g[k].shape == (ex.n_out, w), (tag, k, name, g[k].shape)
            assert np.array_equal(_bits(g[k][:nk]), _bits(old[k][remain])), (tag, k, name, "moved rows differ")
            bad = np.nonzero(_bits(g[k][nk:]))[0]
            assert bad.size == 0, (tag, k, name, "%d words of the appended rows are not zero, first in appended row %d"
                                   % (bad.size, bad[0] // max(w, 1)))
    # appended rows that are computed
    for k in DC.TOLERANCED:
        a, ref, f32, d = got[k][nk:].astype(np.float64), ex.ref[k], ex.f32[k], ex.dist[k]
        if len(ref) == 0:
            continue
        exact = ~np.isfinite(f32).all(1)
        assert np.array_equal(_bits(a[exact]), _bits(f32[exact])), (tag, k, "non-finite reference rows", a[exact], f32[exact])
        assert np.isinf(d[exact]).all() and np.isfinite(d[~exact]).all()
        a, ref, d = a[~exact], ref[~exact], d[~exact]
        if len(ref) == 0:
            continue
        rel = DC.row_error(k, a, ref)
        bound = np.maximum(FLOOR, 2 * d)
        ratio = rel / bound
        at = int(np.argmax(ratio))
        worst[(k, "dist")] = max(worst[(k, "dist")], float(d.max()))
        worst[(k, "err")] = max(worst[(k, "err")], float(rel.max()))
        worst[(k, "ratio")] = max(worst[(k, "ratio")], float(ratio.max()))
        print("  %s %-11s float32 distance %.3g | device error %.3g | error / bound %.3g" % (tag, k, d.max(), rel.max(), ratio.max()))
        bad = np.nonzero(~(ratio <= 1))[0]
        assert bad.size == 0, (tag, k, "%d appended rows beyond their bound; first: appended row %d (parent %d): error "
                               "%.3g, bound %.3g; worst row %d: error %.3g, bound %.3g" %
                               (bad.size, bad[0], parents[~exact][bad[0]], rel[bad[0]], bound[bad[0]], at, rel[at], bound[at]),
                               a[bad[0]].tolist(), ref[bad[0]].tolist())


# ---------------------------------------------------------------------------------------------------------- surface A
def _pset(ptrs):
    from easygaussiansplatting_amd import _lib
    return _lib.EgsGaussianParams(*ptrs)


def _in_ptr(t):
    return t.data_ptr() if t.numel() else None


def _block_offsets(cls):
    """[3][nblocks] exclusive: survivors, clones, splits in front of each workgroup of 256 rows"""
    nb = (len(cls) + 255) // 256
    padded = np.zeros(nb * 256, np.int64)
    padded[:len(cls)] = cls
    padded = padded.reshape(nb, 256)
    sums = np.stack([(padded >= 1).sum(1), (padded == DC.CLONE).sum(1), (padded == DC.SPLIT).sum(1)])
    return (np.cumsum(sums, axis=1) - sums).astype(np.uint32)


def run_abi(lib, tag, ex, with_state, table, seed=None):
    """plan + apply through the C ABI into sentinel-banded buffers; everything about plan is asserted here, before
    apply runs.  -> (params', m', v') as numpy, name -> [n_out, w]"""
    case = ex.case
    n, hw = case["n"], case["hw"]
    p = {k: _dev(case["params"][k]) for k in NAMES}
    acc, cnt = _dev(case["grad_accum"]), _dev(case["cunt"])
    ws_bytes = lib.egs_densify_ws_bytes(n)
    assert ws_bytes % 4 == 0 and ws_bytes >= 12 * ((n + 255) // 256)
    cls, ws, totals = Out((n + 3) // 4), Out(ws_bytes // 4), Out(4)
    _check(lib, lib.egs_densify_plan(n, p["alphas_raw"].data_ptr(), p["scales_raw"].data_ptr(), acc.data_ptr(),
                                     cnt.data_ptr(), *THR, cls.ptr, ws.ptr, ws_bytes, totals.ptr, _stream()))
    got_cls = cls.read((tag, "cls")).view(np.uint8)
    bad = np.nonzero(got_cls[:n] != ex.cls)[0]
    assert bad.size == 0, (tag, "%d classes differ; first: row %d is %d, the oracle says %d%s" % (
        bad.size, bad[0], got_cls[bad[0]], ex.cls[bad[0]], ": " + case["labels"][bad[0]] if "labels" in case else ""))
    assert np.array_equal(got_cls[n:], cls.old().view(np.uint8)[n:]), (tag, "bytes behind row n - 1 written")
    assert totals.read((tag, "totals")).tolist() == [ex.nk, ex.nc, ex.ns, n - ex.nk], (tag, "totals")
    nb = (n + 255) // 256
    got_off = ws.read((tag, "ws"))[:3 * nb].view(np.uint32).reshape(3, nb)
    want_off = _block_offsets(ex.cls)
    bad = np.argwhere(got_off != want_off)
    assert bad.size == 0, (tag, "%d workgroup offsets differ; first: field %d of workgroup %d is %d, not %d" % (
        len(bad), bad[0][0], bad[0][1], got_off[tuple(bad[0])], want_off[tuple(bad[0])]))

    widths = DC.widths(hw)
    outs = [Out(ex.n_out * w) for w in widths]
    sets = [_pset([_in_ptr(p[k]) for k in NAMES]), _pset([o.ptr.value for o in outs])]
    if with_state:
        m = {k: _dev(case["m"][k]) for k in NAMES}
        v = {k: _dev(case["v"][k]) for k in NAMES}
        outs_m = [Out(ex.n_out * w) for w in widths]
        outs_v = [Out(ex.n_out * w) for w in widths]
        sets += [_pset([_in_ptr(m[k]) for k in NAMES]), _pset([_in_ptr(v[k]) for k in NAMES]),
                 _pset([o.ptr.value for o in outs_m]), _pset([o.ptr.value for o in outs_v])]
        state_ptrs = [C.byref(sets[2]), C.byref(sets[3]), C.byref(sets[1]), C.byref(sets[4]), C.byref(sets[5])]
    else:
        outs_m = outs_v = None
        state_ptrs = [None, None, C.byref(sets[1]), None, None]
    noise = _dev(case["unit_noise"]) if table else None
    # with a table the generator's key must not matter; without one it is (seed, ROUND)
    seed = (case["seed"] if seed is None else seed) + (12345 if table else 0)
    _check(lib, lib.egs_densify_apply(n, ex.nk, ex.nc, ex.ns, hw, cls.ptr, ws.ptr, C.byref(sets[0]), state_ptrs[0],
                                      state_ptrs[1], state_ptrs[2], state_ptrs[3], state_ptrs[4],
                                      noise.data_ptr() if table else None, seed, DC.ROUND, _stream()))
    torch.cuda.synchronize()
    # plan's outputs are inputs now: untouched
    assert np.array_equal(cls.read((tag, "cls after apply")).view(np.uint8)[:n], ex.cls)
    assert np.array_equal(ws.read((tag, "ws after apply"))[:3 * nb].view(np.uint32).reshape(3, nb), want_off)
    for k in NAMES:
        assert np.array_equal(_bits(_np(p[k])), _bits(case["params"][k])), (tag, k, "input changed")

    def rows(os_):
        if os_ is None:
            return None
        return {k: os_[j].read((tag, k)).view(F).reshape(ex.n_out, widths[j]) for j, k in enumerate(NAMES)}
    return rows(outs), rows(outs_m), rows(outs_v)


def abi_case(lib, n, hw, pattern, with_state=True, table=True):
    case, ex = _case(n, hw, pattern)
    tag = "%s n=%d hw=%d %s %s" % (pattern, case["n"], hw, "state" if with_state else "no state", "table" if table else "generator")
    got = run_abi(lib, tag, ex, with_state, table)
    check_result(tag, ex, *got)
    return ex, got


@pytest.mark.parametrize("pattern", MAIN)
@pytest.mark.parametrize("n", SIZES)
def test_abi_sizes(lib, n, pattern):
    ex, _ = abi_case(lib, n, 45, pattern)
    if pattern == "all3":
        assert ex.ns == n and ex.n_out == 2 * n
    if pattern == "block" and n >= 1024:
        assert min(ex.nc, ex.ns) >= 256 and n - ex.nk >= 256


@pytest.mark.parametrize("pattern", OTHERS)
@pytest.mark.parametrize("n", [257, 513, 65_537])
def test_abi_patterns(lib, n, pattern):
    ex, _ = abi_case(lib, n, 45, pattern)
    tail = n - ((n - 1) // 256) * 256
    want = {"all0": (0, 0, 0), "all1": (n, 0, 0), "all2": (n, n, 0), "first": (1, 0, 1), "last": (1, 1, 0),
            "tail_only": (tail, 0, tail), "tail_gone": (n - tail, 0, 0)}
    if pattern in want:
        assert (ex.nk, ex.nc, ex.ns) == want[pattern]


@pytest.mark.parametrize("hw", [0, 9, 24, 45])
def test_abi_widths(lib, hw):
    for n in (3, 257, 513):
        for pattern in ("iid", "block"):
            for with_state in (True, False):
                for table in (True, False):
                    abi_case(lib, n, hw, pattern, with_state, table)


@pytest.mark.parametrize("hw", [45, 0])
def test_abi_edges(lib, hw):
    """rows ON the three thresholds classify as the comparisons are written (alpha <, size >, gradient >=); a zero
    quaternion gives rots 0 and leaves the split child at its parent; alphas_raw = 20 appends +inf (float32 sigmoid
    rounds to 1; the reference's torch code does the same): asserted as the float32 oracle gives it"""
    for with_state, table in ((True, True), (False, False)):
        ex, (got, _, _) = abi_case(lib, 0, hw, "edges", with_state, table)
        labels = ex.case["labels"]
        at = lambda i: ex.nk + int(np.nonzero(ex.parents == i)[0][0])
        for i, label in enumerate(labels):
            if label.startswith("zero quaternion"):
                assert not _bits(got["rots_raw"][at(i)]).any(), label
                assert np.array_equal(_bits(got["pws"][at(i)]), _bits(ex.case["params"]["pws"][i])), label
            if label.startswith("alphas_raw 20 on"):
                assert got["alphas_raw"][at(i), 0] == np.inf, label
        assert np.isinf(got["alphas_raw"]).sum() == 2


@pytest.mark.parametrize("n,pattern,table", [(513, "iid", True), (513, "wave", False), (65_537, "iid", False)])
def test_abi_is_deterministic(lib, n, pattern, table):
    _, ex = _case(n, 45, pattern)
    runs = [run_abi(lib, "determinism %d" % rep, ex, True, table) for rep in range(2)]
    for a, b in zip(runs[0], runs[1]):
        for k in NAMES:
            assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    assert ex.nc > 0 and ex.ns > 0
    if not table:                                   # and another seed is another set of children
        other = run_abi(lib, "another seed", ex, True, False, seed=ex.case["seed"] + 1)
        assert not np.array_equal(_bits(other[0]["pws"]), _bits(runs[0][0]["pws"]))
        assert np.array_equal(_bits(other[0]["scales_raw"]), _bits(runs[0][0]["scales_raw"]))


# ---------------------------------------------------------------------------------------------------------- surface B
def _setup(case, opt_name, with_state):
    from easygaussiansplatting_amd.optim import FusedAdam
    opt_cls = FusedAdam if opt_name == "fused" else torch.optim.Adam
    params = {k: _dev(case["params"][k]).requires_grad_() for k in NAMES}
    opt = opt_cls([{"params": [params[k]], "lr": lr, "name": k} for k, lr in zip(NAMES, LRS)], lr=0.0, eps=1e-15)
    if with_state:
        for k in NAMES:
            step = 2 if opt_cls is FusedAdam else torch.tensor(2.0)
            opt.state[params[k]] = {"step": step, "exp_avg": _dev(case["m"][k]), "exp_avg_sq": _dev(case["v"][k])}
    return params, opt


def control_case(n, hw, pattern, opt_name, with_state, table):
    from easygaussiansplatting_amd.density import DensityControl
    case, ex = _case(n, hw, pattern)
    tag = "control %s n=%d hw=%d %s %s %s" % (pattern, n, hw, opt_name, "state" if with_state else "no state",
                                              "table" if table else "generator")
    params, opt = _setup(case, opt_name, with_state)
    old = dict(params)
    ctl = DensityControl(1.0, 1000, seed=case["seed"])
    ctl.round = DC.ROUND
    ctl.set_density_info(_dev(case["grad_accum"]), _dev(case["cunt"]))
    rep = ctl.update_gaussian_density(params, opt, unit_noise=_dev(case["unit_noise"]) if table else None)
    assert rep == {"pruned": n - ex.nk, "cloned": ex.nc, "splited": ex.ns, "total": ex.n_out}, (tag, rep)
    assert ctl.grad_accum is None and ctl.cunt is None and ctl.round == DC.ROUND + 1
    assert len(opt.state) == (6 if with_state else 0)
    for k, grp in zip(NAMES, opt.param_groups):
        p = params[k]
        assert grp["params"][0] is p and p is not old[k] and isinstance(p, torch.nn.Parameter) and p.requires_grad
        assert old[k] not in opt.state
        if with_state:
            st = opt.state[p]
            assert float(st["step"]) == 2.0 and st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape
    w = DC.widths(hw)
    rows = lambda get: {k: _np(get(k)).reshape(ex.n_out, w[j]) for j, k in enumerate(NAMES)}
    got = rows(lambda k: params[k])
    got_m = rows(lambda k: opt.state[params[k]]["exp_avg"]) if with_state else None
    got_v = rows(lambda k: opt.state[params[k]]["exp_avg_sq"]) if with_state else None
    check_result(tag, ex, got, got_m, got_v)
    assert params["high_shs"].shape == (ex.n_out, hw)


@pytest.mark.parametrize("opt_name", ["fused", "torch"])
@pytest.mark.parametrize("n", [257, 65_537])
def test_control_matches_the_oracle_row_by_row(lib, n, opt_name):
    control_case(n, 45, "iid", opt_name, True, True)
    if n == 257:
        control_case(n, 45, "iid", opt_name, True, False)


@pytest.mark.parametrize("with_state", [True, False])
@pytest.mark.parametrize("opt_name", ["fused", "torch"])
def test_control_without_high_shs(lib, opt_name, with_state):
    """SH degree 0: high_shs is [n, 0], its parameter, its moments and its output are empty tensors, and
    ``density._pset`` hands the kernels a null pointer for each"""
    for n in (3, 257):
        control_case(n, 0, "iid", opt_name, with_state, True)


# ---------------------------------------------------------------------------------------------------------- statistics
STAT_SIZES = (1, 63, 65, 257, 513)
MASK_TYPES = {"bool": np.bool_, "uint8": np.uint8, "int64": np.int64, "float32": np.float32}


def _views(n, seed):
    """three views: (dus [n, 2], mask [n] bool); the second view's mask is all False or all True, by the size's parity"""
    masks = [S.uniform01(seed, 10 + vw, (n,)) < 0.5 for vw in range(3)]
    masks[1][:] = n % 2 == 1
    if n > 2:
        masks[2][[0, n - 1]] = [True, False]
    return [((1e-6 * S.normal(seed, 20 + vw, (n, 2))).astype(F), masks[vw]) for vw in range(3)]


@pytest.mark.parametrize("mask_type", list(MASK_TYPES))
@pytest.mark.parametrize("first_all", [None, False, True])
def test_statistics_three_views(lib, mask_type, first_all):
    """``cunt`` exact, ``grad_accum`` within the rtol = 1e-6 of test_density_statistics_match_reference; a later view
    leaves the rows it does not see bitwise as they were.  int64 and float32 masks go through ``vis != 0``: their set
    entries are 3 and 0.25 / -2.0, not 1."""
    from easygaussiansplatting_amd.density import DensityControl
    for n in STAT_SIZES:
        views = _views(n, 300 + n)
        if first_all is not None:
            views[0][1][:] = first_all
        ctl = DensityControl(1.0, 1000)
        acc = cnt = None
        for vw, (dus, mask) in enumerate(views):
            m = mask.astype(MASK_TYPES[mask_type])
            if mask_type == "int64":
                m = m * 3
            if mask_type == "float32":
                m = np.where(np.arange(n) % 2 == 0, F(0.25), F(-2.0)) * m
            before = None if vw == 0 else (_np(ctl.grad_accum).copy(), _np(ctl.cunt).copy())
            dus_t = _dev(dus).requires_grad_(False)
            ctl.update_density_info(dus_t, _dev(m))
            acc, cnt = D.update_density_info(acc, cnt, dus, mask)
            got_acc, got_cnt = _np(ctl.grad_accum), _np(ctl.cunt)
            assert got_acc.shape == (n,) and got_cnt.shape == (n,) and got_cnt.dtype == np.int32
            np.testing.assert_array_equal(got_cnt, cnt, err_msg="n=%d view %d" % (n, vw))
            np.testing.assert_allclose(got_acc, acc, rtol=1e-6, atol=0, err_msg="n=%d view %d" % (n, vw))
            if before is not None:
                assert np.array_equal(_bits(got_acc[~mask]), _bits(before[0][~mask])), (n, vw)
                assert np.array_equal(got_cnt[~mask], before[1][~mask]), (n, vw)
                assert (got_cnt[mask] == before[1][mask] + 1).all()
        with pytest.raises(ValueError, match="rows"):
            ctl.update_density_info(torch.zeros(n + 1, 2, device=DEV), torch.ones(n + 1, dtype=torch.bool, device=DEV))
        assert np.array_equal(_np(ctl.cunt), cnt)


def test_statistics_write_nothing_else(lib):
    """egs_density_accumulate on banded buffers: first view and a later one"""
    for n in STAT_SIZES:
        (dus0, m0), (dus1, m1), _ = _views(n, 300 + n)
        acc, cnt = Out(n), Out(n)
        for first, dus, m in ((1, dus0, m0), (0, dus1, ~m0)):
            d, vis = _dev(dus), _dev(m.astype(np.uint8))
            _check(lib, lib.egs_density_accumulate(n, d.data_ptr(), vis.data_ptr(), first, acc.ptr, cnt.ptr, _stream()))
        want_acc, want_cnt = D.update_density_info(*D.update_density_info(None, None, dus0, m0), dus1, ~m0)
        np.testing.assert_array_equal(cnt.read("cunt"), want_cnt)
        np.testing.assert_allclose(acc.read("grad_accum").view(F), want_acc, rtol=1e-6, atol=0)
        assert (want_cnt == 1).all()


# --------------------------------------------------------------------------------------------------------- reset_alpha
@pytest.mark.parametrize("with_moments", [True, False])
def test_reset_alpha_rows(lib, with_moments):
    """values above logit(0.01) become exactly float32(logit(0.01)), every other value keeps its bits, the moments are
    zeroed when given, and nothing else is written"""
    r = F(D.logit(DC.TH.reset_alpha))
    for n in STAT_SIZES:
        a = (S.uniform01(400 + n, 1, (n,)) * 14 - 8).astype(F)
        a[::5] = np.nextafter(r, F(np.inf))
        a[1::7] = r
        a[2::11] = np.nextafter(r, F(-np.inf))
        a[3::13] = np.inf
        a[4::17] = -np.inf
        assert n < 3 or ((a > r).any() and (a <= r).any())
        alphas = Out(n, a)
        m = Out(n, S.normal(400 + n, 2, (n,)).astype(F)) if with_moments else None
        v = Out(n, (S.uniform01(400 + n, 3, (n,)) + 0.1).astype(F)) if with_moments else None
        _check(lib, lib.egs_reset_alpha(n, D.logit(DC.TH.reset_alpha), alphas.ptr, m.ptr if m else None,
                                        v.ptr if v else None, _stream()))
        got = alphas.read("alphas_raw").view(F)
        want = D.reset_alpha(a, DC.TH)
        assert np.array_equal(_bits(got), _bits(want)), n
        assert (got[a > r] == r).all() and np.array_equal(_bits(got[~(a > r)]), _bits(a[~(a > r)]))
        if with_moments:
            assert not m.read("exp_avg").any() and not v.read("exp_avg_sq").any()


def test_zz_report(lib):
    """the largest figures over the tests of this file that ran before (the file's docstring quotes a full run)"""
    print("\nappended rows, per tensor: largest float32 distance of a row | largest device error | largest error / bound")
    for k in DC.TOLERANCED:
        print("  %-11s %.3g | %.3g | %.3g" % (k, worst[(k, "dist")], worst[(k, "err")], worst[(k, "ratio")]))
