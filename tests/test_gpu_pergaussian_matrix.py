"""Every instance of k_preprocess_fwd (32) and k_preprocess_bwd (192) at ragged row counts, through the C ABI alone
(``egs_fused_forward``; ``egs_fused_backward`` in phase 2 with the test's own gradient records, so that the chain rule
runs without the draw pass in front: no atomics, no thresholds but the near cull), row by row against the float64
reference of tests/pergaussian_ref.py.  Benign inputs swept over instances x modes x row tails; NOT a sweep over
Gaussian regimes (near-plane straddling, fov-clamp boundary, degenerate covariances).

Row counts 1, 2, 3, 255, 256, 257, 258, 515: the last workgroup holds 1, 2, 3, 255, 256, 1, 2, 3 rows, the 45- and
9-float spans end in 1, 2, 3, 3, 0, 1, 2, 3 tail floats.  Cases are grouped by (K, raw); the loops inside cover
  forward   K x raw x dcolor_dpws x anti-aliased at n = 3 and 515, every row count for all-off / all-on;
  backward  K x raw x dcolor_dpws x extras x anti-aliased (POSE off: phase 2) at n = 3 and 515, each plain,
            EGS_BWD_ACCUMULATE over random old gradients, EGS_BWD_FACTORED_SH; every row count for all-off / all-on,
            plain and accumulate; the row windows (0, 258), (256, 259) and (0, 256) + (256, 259) at n = 515;
  pose      the POSE and the POSE_ONLY instance of the same flags through phase 0 on the 64 x 48 image.  The draw pass
            leaves its gradient records in the caller's ``grad_records``; they are read back and fed to the reference,
            so the per-Gaussian outputs of the POSE instances face a reference of the very records they consumed;
            they are compared loosely (default rule of tests/gradcheck.py, outliers=0; exact zeros, dL/dus and the
            sentinel bands as everywhere), their row errors are printed.

Tolerance (the rule of tests/test_gpu_mcmc.py), row by row: |got - ref| of a row, relative to max_j |ref row|, is at
most max(FLOOR, 2 x the float32 distance of THAT row), where the float32 distance is taken on the very inputs of the
call: the largest distance from the float64 reference of the np.float32 evaluation of the reference and of N_PERT = 4
np.float32 evaluations of the inputs moved by one ulp (``R.perturbed``).  The perturbed evaluations are what makes the
bound row-aware without looking at the kernel: a row whose inverse covariance or opacity compensation cancels loses the
same digits whichever way its inputs were rounded, a well-conditioned row gets the floor.  FLOOR = 1e-5: a float32
chain of ~100 operations at 6e-8 each; no larger than tests/gradcheck.py's default rule with outliers=0 (2e-4 of the
largest entry, 5e-3 per entry).  Rows whose reference is zero (culled rows, degree-0 dcolor/dpw) must be zero exactly.
``areas`` are compared exactly, except on the rows ``pergaussian_ref.areas_excluded`` names (at most one apart there).
Accumulate: the old gradients are 0.1 N(0, 1) and join the row's magnitude, so on rows whose own gradient is small the
accumulating call pins the ADD (and what is left alone), not the precision of the chain rule; the plain call of the
same instance pins that.  The POSE instances run plain, accumulate and factored as well, each through its own phase-0
call (own draw pass, own read-back records).

Pose-only against pose: not bitwise.  The two phase-0 calls each run the draw pass, whose float atomics leave records
that differ in their last bits, and the two instances are free to contract FMAs differently (tests/
test_gpu_pose_only.py).  Both pairs are held to ``assert_pose_close`` (1e-4 of sum |terms|) against the reference of
their OWN read-back records, and their difference to the difference of those references within 4e-6 of sum |terms|,
the bound test_gpu_pose_only.py uses between the two instances.

Measured on MI355X, largest row-normalised kernel error per tensor over all cases (each case prints its own, with the
largest float32 distance of a row and the largest error / bound ratio):
  forward   us 6.0e-7, depths 8.4e-8, cinv2ds 3.1e-6, colors 6.1e-7, dcolor_dpws 1.1e-6, record conic 3.2e-6,
            record opacity 5.6e-6
  backward  dpws 1.2e-6, dshs 4.8e-7, dalphas 5.7e-6, drots 3.3e-5, dscales 9.0e-5 (phase 2, the test's records)
  pose      POSE instances on the draw pass's records: dpws 1.1e-5, dshs 5.0e-7, dalphas 2.9e-6, dscales 8.8e-5,
            drots 9.6e-5; pose pair 5.8e-7 of sum |terms| (rule 1e-4); pose-only minus pose 2.6e-7 (rule 4e-6)
Float32 evaluation, measured on the CPU: per tensor the largest distance of any row of any input set is us 9.0e-7,
depths 8.4e-8, cinv2ds 6.3e-6, colors 1.1e-6, dcolor_dpws 1.2e-6, dpws 1.4e-6, dshs 3.8e-7, dalphas 3.2e-6,
drots 2.7e-5, dscales 1.0e-4 as given; the median row of dscales is at 2.5e-7.  The large figures belong to single
rows: for K = 27 activated the dscales distance stays below 1.5e-5 in every set but n = 258 anti-aliased, where row 187
stands at 1.6e-5 as given and 6.4e-5 with its inputs one ulp away.  (A bound of twice the per-(K, raw) maximum of
the unperturbed distance, 3.2e-5 for that group, is below the kernel's 9.0e-5 there.)
"""
import ctypes as C
import collections
import functools
import itertools

import numpy as np
import pytest
import torch

from easygaussiansplatting_amd import scene as S
from tests import pergaussian_ref as R
from tests.gpu_abi import BAND, DEV, Out, _check, _pol, _ptr, _stream
from tests.gradcheck import assert_grad_close
from tests.test_gpu_pose_grad import assert_pose_close

pytestmark = pytest.mark.gpu

W, H = R.W, R.H
FUSED_AA, FUSED_RAW = 256, 512                      # include/egs_hip.h EGS_FUSED_*
BWD_ACCUMULATE, BWD_FACTORED_SH, BWD_POSE_ONLY = 64, 128, 2048
FLOOR = 1e-5
FWD_T = ("us", "depths", "cinv2ds", "colors", "dcolor_dpws", "conic", "alpha_c")
BWD_T = ("dpws", "dshs", "dalphas", "dscales", "drots")
FLAGS3 = list(itertools.product((False, True), repeat=3))

worst = collections.defaultdict(float)              # largest kernel error per (case, tensor), printed per case


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from easygaussiansplatting_amd import _lib, gsplatcu
    gsplatcu.set_policy("gsplatcu")
    yield _lib.load()
    gsplatcu.set_policy("gsplatcu")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.int32)


# ------------------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def _inputs(n, K):
    inp = R.generate(n, K, R.seed_of(n, K))
    cam, twc = R.camera()
    d = {k: torch.from_numpy(np.array(v)).to(DEV) for k, v in inp.items() if k != "culled"}
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)
    d.update(Rcw=f(cam.Rcw), tcw=f(cam.tcw), twc=f(twc))
    return inp, d


def _params(d, raw):
    """(pws, rots, scales, shs, high_shs, alphas) as the ABI takes them"""
    if raw:
        return d["pws"], d["rots_raw"], d["scales_raw"], d["low_shs"], d["high_shs"], d["alphas_raw"]
    return d["pws"], d["rots"], d["scales"], d["shs"], None, d["alphas"]


@functools.lru_cache(maxsize=None)
def _fwd_ref(n, K, raw, aa, f32=False):
    inp, _ = _inputs(n, K)
    f = R.forward(inp, raw, aa, np.float32 if f32 else np.float64)
    f["conic"] = R.record_fields(f)[:, 2:5]
    return f


@functools.lru_cache(maxsize=None)
def _bwd_ref(n, K, raw, aa, extra, f32=False):
    inp, _ = _inputs(n, K)
    return R.backward(inp, inp["records"], raw, aa, extra, np.float32 if f32 else np.float64)


N_PERT = 4


@functools.lru_cache(maxsize=None)
def _fwd_dist(n, K, raw, aa):
    """per tensor and ROW, on the inputs of this very call: the largest distance from the float64 reference of the
    float32 evaluation and of N_PERT float32 evaluations of the inputs moved by one ulp (R.perturbed)"""
    inp, _ = _inputs(n, K)
    ref = _fwd_ref(n, K, raw, aa)
    d = {k: np.zeros(n) for k in FWD_T}
    for j in range(N_PERT + 1):
        f = R.forward(inp if j == 0 else R.perturbed(inp, j), raw, aa, np.float32)
        f["conic"] = R.record_fields(f)[:, 2:5]
        for k in FWD_T:
            d[k] = np.maximum(d[k], R.row_errors(f[k], ref[k])[0])
    return d


@functools.lru_cache(maxsize=None)
def _bwd_dist(n, K, raw, aa, extra):
    inp, _ = _inputs(n, K)
    ref = _bwd_ref(n, K, raw, aa, extra)
    d = {k: np.zeros(n) for k in BWD_T}
    for j in range(N_PERT + 1):
        p = inp if j == 0 else R.perturbed(inp, j)
        b = R.backward(p, p["records"], raw, aa, extra, np.float32)
        for k in BWD_T:
            d[k] = np.maximum(d[k], R.row_errors(b[k], ref[k])[0])
    return d


def _tol(case, name, got, ref, dist=None, rows=None, scale_with=None, loose=False):
    """the toleranced comparison of one tensor on ``rows``, row by row: a row's error, relative to the row's own
    magnitude, is at most max(FLOOR, 2 x ``dist`` of that row).  ``scale_with``: arrays that join the row's magnitude
    (the old gradient of an accumulating call; ``dist`` is rescaled to it).  ``loose``: the error is recorded but
    the assertion is the default rule of tests/gradcheck.py with outliers=0"""
    rows = slice(None) if rows is None else rows
    got = np.asarray(got).reshape(len(ref), -1)[rows]
    sw = [np.asarray(s).reshape(len(ref), -1)[rows] for s in scale_with or ()]
    ref = np.asarray(ref).reshape(len(ref), -1)[rows]
    err, inexact, at = R.row_error(got, ref, sw)
    key = name.split(":")[0]
    worst[(case, key)] = max(worst[(case, key)], err)
    assert inexact == 0, (case, name, "rows with a zero reference are not zero", inexact)
    if loose:
        if np.abs(ref).max(initial=0.0) > 0:
            assert_grad_close(got, ref, (case, name), outliers=0)
        return
    if len(ref) == 0:
        return
    rel, scale, _ = R.row_errors(got, ref, sw)
    d = np.asarray(dist[key])[rows]
    if sw:   # the float32 distance is relative to the NEW gradient's magnitude: bring it to the row's scale
        own = np.abs(np.asarray(sw[-1], np.float64)).max(1)
        d = d * own / np.where(scale == 0, 1.0, scale)
    bound = np.maximum(FLOOR, 2 * d) + (1.2e-7 if sw else 0.0)
    worst[(case, key + " f32")] = max(worst[(case, key + " f32")], float(d.max()))
    ratio = rel / bound
    worst[(case, key + " /bound")] = max(worst[(case, key + " /bound")], float(ratio.max()))
    bad = np.nonzero(ratio > 1)[0]
    assert bad.size == 0, (case, name, "%d rows beyond their bound; worst row %d: error %.3g, bound %.3g (float32 "
                           "distance of the row %.3g)" % (bad.size, int(np.argmax(ratio)), rel[np.argmax(ratio)],
                                                         bound[np.argmax(ratio)], d[np.argmax(ratio)]),
                           got[np.argmax(ratio)].tolist(), ref[np.argmax(ratio)].tolist())


def _report(case):
    keys = sorted({k for c, k in worst if c == case and not k.endswith((" f32", " /bound"))})
    print("\n%s  per tensor: largest float32 distance of a row | largest kernel error of a row | largest error / bound"
          " (loose comparisons: the kernel error alone):" % case)
    for k in keys:
        if (case, k + " /bound") in worst:
            print("  %-12s %.3g | %.3g | %.3g" % (k, worst[(case, k + " f32")], worst[(case, k)], worst[(case, k + " /bound")]))
        else:
            print("  %-18s %.3g" % (k, worst[(case, k)]))


# ----------------------------------------------------------------------------------------------------------- forward
class Fwd:
    pass


def run_forward(lib, n, K, raw, jw, aa):
    inp, d = _inputs(n, K)
    pws, rots, scales, shs, high, alphas = _params(d, raw)
    o = Fwd()
    o.us, o.depths, o.cinv, o.col, o.areas = Out(2 * n), Out(n), Out(3 * n), Out(3 * n), Out(2 * n)
    o.rec, o.dcw = Out(12 * n), (Out(9 * n) if jw else None)
    o.vis_before = np.full(n + 512, 0xA5, np.uint8)
    o.vis = torch.from_numpy(o.vis_before.copy()).to(DEV)
    ws_bin = torch.empty(lib.egs_splat_bin_ws_bytes(n), dtype=torch.uint8, device=DEV)
    o.ws_bin = ws_bin
    o.total = torch.zeros(2, dtype=torch.int32, device=DEV)
    cam, _ = R.camera()
    flags = (FUSED_RAW if raw else 0) | (FUSED_AA if aa else 0)
    _check(lib, lib.egs_fused_forward(
        n, K, _ptr(pws), _ptr(rots), _ptr(scales), _ptr(shs), _ptr(high), _ptr(alphas), _ptr(d["Rcw"]), _ptr(d["tcw"]),
        _ptr(d["twc"]), cam.fx, cam.fy, cam.cx, cam.cy, W, H, C.byref(_pol()), o.us.ptr, o.depths.ptr, o.cinv.ptr,
        o.col.ptr, o.areas.ptr, o.rec.ptr, C.c_void_p(o.vis.data_ptr() + 256), None if o.dcw is None else o.dcw.ptr,
        flags, 0, _ptr(ws_bin), ws_bin.numel(), _ptr(o.total), None, _stream()))
    torch.cuda.synchronize()
    o.flags = flags
    return o


def check_forward(case, o, n, K, raw, jw, aa):
    what = (case, n, "jw" if jw else "", "aa" if aa else "")
    inp, _ = _inputs(n, K)
    ref = _fwd_ref(n, K, raw, aa)
    live = ref["live"]
    f = lambda out, w: out.read(what + (w,)).view(np.float32)
    us, depths, cinv, col = f(o.us, "us").reshape(n, 2), f(o.depths, "depths"), f(o.cinv, "cinv2ds").reshape(n, 3), \
        f(o.col, "colors").reshape(n, 3)
    areas = o.areas.read(what + ("areas",)).reshape(n, 2)
    rec = f(o.rec, "rec").reshape(n, 12)
    vis = o.vis.cpu().numpy()
    assert np.array_equal(vis[:256], o.vis_before[:256]) and np.array_equal(vis[256 + n:], o.vis_before[256 + n:]), what
    vis = vis[256:256 + n]
    # per row against the reference
    dist = _fwd_dist(n, K, raw, aa)
    _tol(case, "us", us, ref["us"], dist)
    _tol(case, "depths", depths, ref["depths"], dist)
    _tol(case, "cinv2ds", cinv, ref["cinv2ds"], dist)
    _tol(case, "colors", col, ref["colors"], dist)
    if jw:
        _tol(case, "dcolor_dpws", f(o.dcw, "dcolor_dpws").reshape(n, 9), ref["dcolor_dpws"], dist)
    _tol(case, "conic", rec[:, 2:5], ref["conic"], dist)
    _tol(case, "alpha_c", rec[:, 5], ref["alpha_c"], dist)
    _tol(case, "us:record", rec[:, 0:2], ref["us"], dist)
    _tol(case, "colors:record", rec[:, 6:9], ref["colors"], dist)
    assert np.array_equal(vis != 0, ref["visible"]) and set(np.unique(vis)) <= {0, 1}, what
    excl = R.areas_excluded(ref)
    assert np.array_equal(areas[~excl], ref["areas"][~excl]), (what, "areas")
    assert (np.abs(areas[excl].astype(np.int64) - ref["areas"][excl]) <= 1).all(), (what, "areas near an integer radius")
    # the records agree bit for bit with the seven-op outputs of the same call
    assert np.array_equal(_bits(rec[:, 0:2]), _bits(us)) and np.array_equal(_bits(rec[:, 6:9]), _bits(col)), what
    k = R.NHL2E
    assert np.array_equal(rec[:, 2:5], np.stack([k * cinv[:, 0], (np.float32(2) * k) * cinv[:, 1], k * cinv[:, 2]], 1)), what
    if not raw and not aa:
        assert np.array_equal(_bits(rec[:, 5]), _bits(inp["alphas"])), what
    # culled rows: the documented markers, exactly
    dead = ~live
    assert np.array_equal(dead, inp["culled"])
    assert (depths[dead] == -1).all() and not us[dead].any() and not cinv[dead].any() and not areas[dead].any(), what
    assert not vis[dead].any() and not rec[dead, 0:5].any(), what
    if aa:
        assert not rec[dead, 5].any(), what
    assert (depths[live] >= 1.9).all() and vis[live].all() and (areas[live] > 0).all(), what


@pytest.mark.parametrize("raw", [False, True], ids=["act", "raw"])
@pytest.mark.parametrize("K", R.KS)
def test_forward_instances_and_row_tails(lib, K, raw):
    case = "forward K=%d %s" % (K, "raw" if raw else "act")
    runs = [(n, jw, aa) for jw in (False, True) for aa in (False, True) for n in (3, 515)]
    runs += [(n, on, on) for on in (False, True) for n in R.ROW_COUNTS if n not in (3, 515)]
    for n, jw, aa in runs:
        check_forward(case, run_forward(lib, n, K, raw, jw, aa), n, K, raw, jw, aa)
    a, b = run_forward(lib, 515, K, raw, True, True), run_forward(lib, 515, K, raw, True, True)
    for x, y in ((a.us, b.us), (a.depths, b.depths), (a.cinv, b.cinv), (a.col, b.col), (a.areas, b.areas), (a.rec, b.rec),
                 (a.dcw, b.dcw)):
        assert torch.equal(x.t, y.t), (case, "not deterministic")
    _report(case)


# ---------------------------------------------------------------------------------------------------------- backward
@functools.lru_cache(maxsize=None)
def _forward_state(lib, n, K, raw, aa):
    """the forward call whose depths, records and dcolor/dpw the backward calls read (checked by the forward test)"""
    return run_forward(lib, n, K, raw, True, aa)


def _widths(K, raw, factored):
    """name -> floats per row of the seven outputs"""
    w = dict(dpws=3, dalphas=1, dscales=3, drots=4, dus=2)
    w["dshs"] = 3 if (raw or factored) else K
    if raw and K > 3:
        w["dhigh"] = K - 3
    return w


def new_outputs(n, K, raw, mode, seed):
    """sentinel-filled (plain, factored) or holding random old gradients (accumulate); dus is never accumulated"""
    outs = {}
    for j, (name, w) in enumerate(sorted(_widths(K, raw, mode == "factored").items())):
        words = n * w + (3 if (name == "dshs" and mode == "factored") else 0)
        old = None
        if mode == "accumulate" and name != "dus":
            old = (0.1 * S.normal(seed, 50 + j, (words,))).astype(np.float32)
        outs[name] = Out(words, old)
    return outs


def run_backward(lib, fw, n, K, raw, jw, aa, extra, mode, outs, window=None, phase=2, pose=None, draw=None):
    """one egs_fused_backward call; phase 2 reads the test's own records, phase 0 (``draw``) the draw pass's"""
    inp, d = _inputs(n, K)
    pws, rots, scales, shs, high, alphas = _params(d, raw)
    cam, _ = R.camera()
    b, c = window if window is not None else (0, n)
    flags = fw.flags | {"plain": 0, "accumulate": BWD_ACCUMULATE, "factored": BWD_FACTORED_SH,
                        "pose_only": BWD_POSE_ONLY}[mode]
    from easygaussiansplatting_amd._lib import EgsExtras
    ws = torch.empty(lib.egs_fused_backward_ws_bytes(n), dtype=torch.uint8, device=DEV)
    depths = C.c_void_p(fw.depths.ptr.value)
    ex = None
    if extra:
        ex = EgsExtras(depths.value, None, None, (C.c_float * 3)(0.2, 0.5, 0.9),
                       None if draw is None else draw["dld"].data_ptr(), None if draw is None else draw["dla"].data_ptr())
    g = lambda k: None if outs is None or k not in outs else outs[k].ptr
    dr = draw or {}
    _check(lib, lib.egs_fused_backward(
        n, K, dr.get("P", 0), W, H, _ptr(pws), _ptr(rots), _ptr(scales), _ptr(shs), _ptr(high), _ptr(alphas),
        _ptr(d["Rcw"]), _ptr(d["tcw"]), _ptr(d["twc"]), cam.fx, cam.fy, cam.cx, cam.cy, C.byref(_pol()), None, None, None,
        None, fw.rec.ptr, depths, _ptr(dr.get("contrib")), _ptr(dr.get("tau")), _ptr(dr.get("ranges")),
        _ptr(dr.get("gsid")), _ptr(dr.get("dl")), _ptr(ws), ws.numel(), g("dpws"), g("dshs"), g("dhigh"), g("dalphas"),
        g("dscales"), g("drots"), g("dus"), None, _ptr(dr["gpack"] if draw else d["records"]),
        fw.dcw.ptr if jw else None, phase | flags, b, c, None, 0, _stream(), None if ex is None else C.byref(ex),
        None if pose is None else C.byref(pose)))
    torch.cuda.synchronize()


def check_backward(case, outs, n, K, raw, aa, extra, mode, windows, rec=None, ref=None, loose=False):
    """the seven outputs after the calls over ``windows`` (disjoint (begin, count) pairs) against the reference"""
    what = (case, n, "aa" if aa else "", "extra" if extra else "", mode, tuple(windows))
    inp, _ = _inputs(n, K)
    rec = inp["records"] if rec is None else rec
    dist = None if loose else _bwd_dist(n, K, raw, aa, extra)
    ref = _bwd_ref(n, K, raw, aa, extra) if ref is None else ref
    live = ref["live"]
    inwin = np.zeros(n, bool)
    for b, c in windows:
        inwin[b:b + c] = True
    factored = mode == "factored"
    got = {k: o.read(what + (k,)) for k, o in outs.items()}
    for name, w in _widths(K, raw, factored).items():
        o = outs[name]
        bits = got[name][:n * w].reshape(n, w)
        val = bits.view(np.float32)
        old_bits = o.old()[:n * w].reshape(n, w)
        # rows outside the windows: untouched, bit for bit
        assert np.array_equal(bits[~inwin], old_bits[~inwin]), (what, name, "rows outside the window were written")
        dead, alive = inwin & ~live, inwin & live
        if name == "dus":           # the record's du for every row
            assert np.array_equal(bits[inwin], _bits(rec[:, 4:6]).reshape(n, 2)[inwin]), (what, name)
            continue
        if factored and name == "dhigh":
            assert np.array_equal(got[name], o.old()), (what, "factored: dloss_dhigh_shs was written")
            continue
        if factored and name == "dshs":
            assert np.array_equal(bits[alive], _bits(rec[:, 1:4]).reshape(n, 3)[alive]), (what, "dL/dcolour")
            assert not val[dead].any(), (what, "dL/dcolour of culled rows")
            tail, tail_old = got[name][3 * n:], o.old()[3 * n:]
            if any(b == 0 for b, _ in windows):
                assert np.array_equal(tail, _bits(R.camera()[1])), (what, "twc behind the block")
            else:
                assert np.array_equal(tail, tail_old), (what, "twc written by a window that does not start at row 0")
            continue
        key = {"dhigh": "dshs_high", "dshs": "dshs_low" if raw else "dshs"}.get(name, name)
        r = np.asarray(ref[key], np.float64).reshape(n, w)
        tkey = "dshs" if name in ("dshs", "dhigh") else name
        if mode == "accumulate":
            old = old_bits.view(np.float32)
            assert np.array_equal(bits[dead], old_bits[dead]), (what, name, "culled rows must keep the old gradient")
            _tol(case, tkey + ":%s+old n=%d" % (name, n), val, r + old.astype(np.float64), dist, alive, [old, r],
                 loose)
        else:
            assert not val[dead].any(), (what, name, "culled rows must be zero")
            _tol(case, tkey + ":%s n=%d %s%s%s" % (name, n, mode, " aa" * aa, " extra" * extra), val, r, dist, alive, None,
                 loose)


@pytest.mark.parametrize("raw", [False, True], ids=["act", "raw"])
@pytest.mark.parametrize("K", R.KS)
def test_backward_instances_modes_and_row_tails(lib, K, raw):
    case = "backward K=%d %s" % (K, "raw" if raw else "act")
    runs = [(n, jw, extra, aa, mode) for jw, extra, aa in FLAGS3 for n in (3, 515)
            for mode in ("plain", "accumulate", "factored")]
    runs += [(n, on, on, on, mode) for on in (False, True) for n in R.ROW_COUNTS if n not in (3, 515)
             for mode in ("plain", "accumulate")]
    for i, (n, jw, extra, aa, mode) in enumerate(runs):
        fw = _forward_state(lib, n, K, raw, aa)
        outs = new_outputs(n, K, raw, mode, 1000 * K + n + i)
        run_backward(lib, fw, n, K, raw, jw, aa, extra, mode, outs)
        check_backward(case + (" jw" if jw else ""), outs, n, K, raw, aa, extra, mode, [(0, n)])
    # row windows at n = 515: each on its own, then two calls into the same outputs against the single call
    n = 515
    for on in (False, True):
        fw = _forward_state(lib, n, K, raw, on)
        for mode in ("plain", "accumulate", "factored"):
            for wins in ([(0, 258)], [(256, 259)], [(0, 256), (256, 259)]):
                outs = new_outputs(n, K, raw, mode, 77)
                for win in wins:
                    run_backward(lib, fw, n, K, raw, on, on, on, mode, outs, win)
                check_backward(case, outs, n, K, raw, on, on, mode, wins)
                if len(wins) == 2:
                    one = new_outputs(n, K, raw, mode, 77)
                    run_backward(lib, fw, n, K, raw, on, on, on, mode, one)
                    for k in outs:
                        assert torch.equal(outs[k].t, one[k].t), (case, mode, k, "two windows differ from the single call")
    # determinism: no atomics in phase 2
    fw = _forward_state(lib, n, K, raw, True)
    a, b = new_outputs(n, K, raw, "accumulate", 5), new_outputs(n, K, raw, "accumulate", 5)
    run_backward(lib, fw, n, K, raw, False, True, True, "accumulate", a)
    run_backward(lib, fw, n, K, raw, False, True, True, "accumulate", b)
    for k in a:
        assert torch.equal(a[k].t, b[k].t), (case, k, "not deterministic")
    _report(case)
    _report(case + " jw")


# -------------------------------------------------------------------------------------------------------------- pose
def _draw(lib, fw, n, seed):
    """the draw stage of the forward call ``fw`` and the upstream gradients of a phase-0 backward"""
    e = lambda shape, dt: torch.empty(shape, dtype=dt, device=DEV)
    cap = int(fw.total[0].item()) + 16
    T = ((W + 15) // 16) * ((H + 15) // 16)
    dr = dict(image=e((3, H, W), torch.float32), contrib=e((H, W), torch.int32), tau=e((H, W), torch.float32),
              ranges=e((T, 2), torch.int32), gsid=e((cap,), torch.int32))
    ws_draw = e((lib.egs_splat_draw_ws_bytes(n, cap, W, H),), torch.uint8)
    _check(lib, lib.egs_splat_draw_rec_seg(n, cap, _ptr(fw.total), W, H, fw.rec.ptr, C.byref(_pol()), _ptr(fw.ws_bin),
                                           _ptr(ws_draw), ws_draw.numel(), _ptr(dr["image"]), _ptr(dr["contrib"]),
                                           _ptr(dr["tau"]), _ptr(dr["ranges"]), _ptr(dr["gsid"]), None, None, None, 0, 0,
                                           None, 0, None, None, None, _stream(), None))
    torch.cuda.synchronize()
    dr["P"] = int(fw.total[0].item())
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)
    dr["dl"] = f(S.normal(seed, 1, (3, H, W)) / (3 * H * W))
    dr["dld"] = f(0.2 * S.normal(seed, 2, (H, W)) / (H * W))
    dr["dla"] = f(S.normal(seed, 3, (H, W)) / (H * W))
    return dr


def _pose_call(lib, fw, dr, n, K, raw, jw, aa, extra, mode, outs):
    from easygaussiansplatting_amd._lib import EgsPoseGrad
    dr["gpack"] = torch.zeros((n, 12), dtype=torch.float32, device=DEV)       # the records of ONE backward pass
    dR = torch.full((9,), float("nan"), dtype=torch.float32, device=DEV)
    dt = torch.full((3,), float("nan"), dtype=torch.float32, device=DEV)
    pws = torch.empty(lib.egs_pose_ws_bytes(n), dtype=torch.uint8, device=DEV)
    pg = EgsPoseGrad(dR.data_ptr(), dt.data_ptr(), pws.data_ptr(), pws.numel())
    run_backward(lib, fw, n, K, raw, jw, aa, extra, mode, outs, None, 0, pg, dr)
    return dR.double().cpu().numpy(), dt.double().cpu().numpy(), dr["gpack"].cpu().numpy()


@pytest.mark.parametrize("raw", [False, True], ids=["act", "raw"])
@pytest.mark.parametrize("K", R.KS)
def test_pose_and_pose_only_instances(lib, K, raw):
    case = "pose K=%d %s" % (K, "raw" if raw else "act")
    drawn = 0
    for (jw, extra, aa), n in itertools.product(FLAGS3, (3, 515)):
        inp, _ = _inputs(n, K)
        fw = run_forward(lib, n, K, raw, True, aa)
        dr = _draw(lib, fw, n, 300 + n)
        outs = new_outputs(n, K, raw, "plain", 0)
        gR, gt, rec = _pose_call(lib, fw, dr, n, K, raw, jw, aa, extra, "plain", outs)
        # the same POSE instance accumulating and with the factored SH gradient: each call has its own draw pass
        for mode in ("accumulate", "factored"):
            mo = new_outputs(n, K, raw, mode, 900 + n)
            mR, mt, mrec = _pose_call(lib, fw, dr, n, K, raw, jw, aa, extra, mode, mo)
            check_backward(case, mo, n, K, raw, aa, extra, mode, [(0, n)], mrec,
                           R.backward(inp, mrec, raw, aa, extra), loose=True)
            assert_pose_close(mR.reshape(3, 3), mt, R.pose_terms(inp, mrec, raw, aa, extra), 1e-4, (case, n, mode))
        oR, ot, rec_only = _pose_call(lib, fw, dr, n, K, raw, jw, aa, extra, "pose_only", None)
        drawn += int((np.abs(rec[:, :9]).max(1) > 0).sum())
        if not extra:
            assert not rec[:, 9].any() and not rec_only[:, 9].any()
        # the per-Gaussian outputs of the POSE instance, for the records its draw pass left
        ref = R.backward(inp, rec, raw, aa, extra)
        check_backward(case, outs, n, K, raw, aa, extra, "plain", [(0, n)], rec, ref, loose=True)
        # the pose pair of both instances against the reference of their own records
        terms, terms_only = R.pose_terms(inp, rec, raw, aa, extra), R.pose_terms(inp, rec_only, raw, aa, extra)
        label = (case, n, jw, extra, aa)
        gap = assert_pose_close(gR.reshape(3, 3), gt, terms, 1e-4, label + ("pose",))
        gap_only = assert_pose_close(oR.reshape(3, 3), ot, terms_only, 1e-4, label + ("pose only",))
        worst[(case, "pose gap")] = max(worst[(case, "pose gap")], gap, gap_only)
        # pose-only against pose: the two references differ by what the atomics of the two draw passes differ by
        sR, st, scale = R.pose_pair(terms)
        s2R, s2t, _ = R.pose_pair(terms_only)
        diff = np.concatenate([(oR - gR) - (s2R - sR).reshape(-1), (ot - gt) - (s2t - st)])
        rel = float((np.abs(diff) / np.maximum(scale, 1e-30)).max())
        worst[(case, "pose-only vs pose")] = max(worst[(case, "pose-only vs pose")], rel)
        assert rel <= 4e-6, (label, "pose-only differs from pose", rel)
        if n == 515:
            assert np.abs(gR).max() > 0 and np.abs(gt).max() > 0
    assert drawn > 8 * 100, (case, "the draw pass reached too few Gaussians", drawn)
    _report(case)
