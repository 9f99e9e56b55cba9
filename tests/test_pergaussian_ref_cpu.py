"""tests/pergaussian_ref.py proved on the CPU: its backward against central differences of its float64 forward, its
restated pieces against the modules they restate, and the cap on the rows its exclusion rule leaves out, for every
input set tests/test_gpu_pergaussian_matrix.py uses."""
import numpy as np
import pytest

from easygaussiansplatting_amd import scene as S
from oracle import gs_oracle as O
from tests import aa_ref
from tests import pergaussian_ref as R
from tests.test_pose_grad_cpu import rodrigues

N_FD = 12
DELTA = 1e-6
# central differences with h = 1e-6 in float64: truncation ~ h^2 = 1e-12 and round-off ~ 1e-16 |L| / h = 1e-10 |L| of
# the row's loss terms; 1e-6 of the row's gradient plus 1e-8 of its record leaves three orders of margin on both
FD_REL, FD_ABS = 1e-6, 1e-8


def _row_loss(inp, rec, raw, aa, dz, live, cam=None, twc=None):
    """L_row = <record, forward outputs> of one row: alpha_c, colour, u, cinv2d (+ z with ``dz``); culled rows: 0"""
    f = R.forward(inp, raw, aa, np.float64, cam, twc)
    cam = cam or R.camera()[0]
    pws = np.asarray(inp["pws"], np.float64)
    z = (pws @ np.asarray(cam.Rcw, np.float64).T + np.asarray(cam.tcw, np.float64))[:, 2]
    L = (rec[:, 0] * f["alpha_c"] + (rec[:, 1:4] * f["colors"]).sum(1) + (rec[:, 4:6] * f["us"]).sum(1)
         + (rec[:, 6:9] * f["cinv2ds"]).sum(1))
    if dz:
        L = L + rec[:, 9] * z
    assert np.array_equal(f["live"], live)
    return np.where(live, L, 0.0)


def _fd(inp, key, fn):
    """d L_row / d inp[key][row, j] for every j: the rows are independent, so one pair of evaluations per column"""
    base = np.asarray(inp[key], np.float64)
    base = base.reshape(len(base), -1)
    out = np.zeros_like(base)
    for j in range(base.shape[1]):
        hi, lo = base.copy(), base.copy()
        hi[:, j] += DELTA
        lo[:, j] -= DELTA
        shape = np.asarray(inp[key]).shape
        out[:, j] = (fn(dict(inp, **{key: hi.reshape(shape)})) - fn(dict(inp, **{key: lo.reshape(shape)}))) / (2 * DELTA)
    return out


def _close(num, ana, rec, what):
    num, ana = num.reshape(len(rec), -1), np.asarray(ana, np.float64).reshape(len(rec), -1)
    bound = FD_REL * np.abs(ana).max(1) + FD_ABS * np.abs(rec).max(1)
    err = np.abs(num - ana).max(1)
    assert (err <= bound).all(), (what, float((err / bound).max()), int(np.argmax(err / bound)))


@pytest.mark.parametrize("dz", [False, True])
@pytest.mark.parametrize("aa", [False, True])
@pytest.mark.parametrize("raw", [False, True])
@pytest.mark.parametrize("K", R.KS)
def test_backward_matches_central_differences(K, raw, aa, dz):
    inp = {k: np.asarray(v, np.float64) if v.dtype != bool else v for k, v in R.generate(N_FD, K, 40 + K).items()}
    rec = inp["records"]
    b = R.backward(inp, rec, raw, aa, dz)
    live = b["live"]
    assert live.sum() >= N_FD - 4 and (~live).sum() >= 1 and np.array_equal(~live, inp["culled"])
    fn = lambda d: _row_loss(d, rec, raw, aa, dz, live)
    names = dict(pws="dpws", rots_raw="drots", scales_raw="dscales", alphas_raw="dalphas", low_shs="dshs_low",
                 high_shs="dshs_high") if raw else dict(pws="dpws", rots="drots", scales="dscales", alphas="dalphas",
                                                         shs="dshs")
    for key, out in names.items():
        if inp[key].size:
            _close(_fd(inp, key, fn), b[out], rec, (key, K, raw, aa, dz))
    # culled rows: zero everywhere, the screen-space gradient is the record's for every row, the factored form is
    # the record's colour gradient on live rows
    for k in ("dpws", "dshs", "dalphas", "dscales", "drots", "dcolour"):
        assert not b[k][~live].any(), k
    assert np.array_equal(b["dus"], rec[:, 4:6]) and np.array_equal(b["dcolour"][live], rec[live, 1:4])
    # pose: Rcw moves through a twist (stays a rotation), twc = -Rcw^T tcw follows
    cam0, _ = R.camera()
    R0, t0 = np.asarray(cam0.Rcw, np.float64), np.asarray(cam0.tcw, np.float64)

    def total(x):
        Rx = rodrigues(x[:3]) @ R0
        cam = S.Camera(cam0.width, cam0.height, cam0.fx, cam0.fy, cam0.cx, cam0.cy, Rx, x[3:])
        return _row_loss(inp, rec, raw, aa, dz, live, cam, -Rx.T @ x[3:]).sum()

    x0 = np.concatenate([np.zeros(3), t0])
    num = np.zeros(6)
    for j in range(6):
        d = np.zeros(6)
        d[j] = DELTA
        num[j] = (total(x0 + d) - total(x0 - d)) / (2 * DELTA)
    terms = R.pose_terms(inp, rec, raw, aa, dz)
    dR, dt, scale = R.pose_pair(terms)
    gen = lambda k: np.cross(np.eye(3)[k], np.eye(3)).T        # [e_k]x: column j is e_k x e_j
    ana = np.array([(dR * (gen(k) @ R0)).sum() for k in range(3)] + list(dt))
    assert not terms[~live].any()
    assert (np.abs(num - ana) <= FD_REL * max(scale.max(), 1.0)).all(), (num, ana)


def test_restated_pieces_equal_their_sources():
    """comp / comp_vjp against tests/aa_ref.py, the whole backward against O.chain_rule fed the inverse's Jacobian, the
    raw chain against the activated one, all in float64"""
    inp = R.generate(40, 48, 5)
    rec = np.asarray(inp["records"], np.float64)
    st = R.stages(inp, False)
    g = rec[:, 0]
    assert np.array_equal(R.comp(st["c2"]), aa_ref.comp(st["c2"]))
    assert np.array_equal(R.comp_vjp(st["c2"], g), aa_ref.comp_vjp(st["c2"], g))
    J = dict(dcinv2d_dcov2ds=st["dci"], dcov2d_dcov3ds=st["d3"], dcov3d_drots=st["dq"], dcov3d_dscales=st["ds"],
             dcolor_dshs=st["dsh"], du_dpcs=st["du"], dcov2d_dpcs=st["dpc"], dcolor_dpws=st["dpw"])
    cam, _ = R.camera()
    want = O.chain_rule(rec[:, 4:6], rec[:, 6:9], rec[:, 0], rec[:, 1:4], cam.Rcw, J)
    got = R.backward(inp, rec, False, False, False)
    live = got["live"]
    for k in ("dpws", "dshs", "dalphas", "dscales", "drots"):
        np.testing.assert_allclose(got[k][live], want[k][live], rtol=1e-12, atol=0, err_msg=k)
    # the packed record: conic = NHL2E * (c0, 2 c1, c2)
    f = R.forward(inp, False, True)
    rf = R.record_fields(f)
    assert np.array_equal(rf[:, :2], f["us"]) and np.array_equal(rf[:, 6:], f["colors"])
    np.testing.assert_allclose(rf[:, 3], 2 * float(R.NHL2E) * f["cinv2ds"][:, 1], rtol=1e-15)
    assert (f["comp"][live] > 0).all() and (f["comp"][live] < 1).all() and not f["comp"][~live].any()
    assert not f["us"][~live].any() and (f["depths"][~live] == -1).all() and not f["areas"][~live].any()
    assert f["colors"][~live].any()                                  # colour has no depth test


def test_float32_evaluation_is_close_and_in_float32():
    inp = R.generate(64, 27, 9)
    for raw in (False, True):
        f64, f32 = R.forward(inp, raw, True), R.forward(inp, raw, True, np.float32)
        b64 = R.backward(inp, inp["records"], raw, True, True)
        b32 = R.backward(inp, inp["records"], raw, True, True, np.float32)
        for d64, d32 in ((f64, f32), (b64, b32)):
            for k, v in d32.items():
                if v.dtype.kind == "f":
                    assert v.dtype == np.float32, k
                    err, exact, _ = R.row_error(v, d64[k])
                    assert err < 1e-3 and exact == 0, (k, err, exact)


@pytest.mark.parametrize("K", R.KS)
def test_excluded_rows_stay_under_the_cap(K):
    """the share of rows left out of the toleranced ``areas`` comparison, from the float64 reference alone, for every
    input set of the GPU file -- activated and raw, since the two are different Gaussians in float32"""
    for n, k, seed in R.input_sets():
        if k != K:
            continue
        inp = R.generate(n, k, seed)
        assert (inp["culled"].sum() >= n // 20) and (~inp["culled"]).sum() >= min(n, 2) - 1
        for raw in (False, True):
            f = R.forward(inp, raw, False)
            assert np.array_equal(f["live"], ~inp["culled"])
            assert f["depths"][f["live"]].min() >= 1.9 and f["depths"][f["live"]].max() <= 8.1
            us = f["us"][f["live"]]
            assert (us >= 0).all() and (us[:, 0] <= R.W).all() and (us[:, 1] <= R.H).all()
            share = R.areas_excluded(f).mean()
            assert share <= R.EXCLUDED_CAP, (n, k, seed, raw, share)


def test_perturbed_inputs_are_one_ulp_away():
    inp = R.generate(33, 12, 3)
    a, b = R.perturbed(inp, 1), R.perturbed(inp, 2)
    for k, v in inp.items():
        if v.dtype == np.float32 and k not in ("low_shs", "high_shs"):
            up, down = np.nextafter(v, np.float32(np.inf)), np.nextafter(v, np.float32(-np.inf))
            assert ((a[k] == up) | (a[k] == down)).all() and (a[k] != v).all(), k
            assert (a[k] != b[k]).any(), k
    assert np.array_equal(np.concatenate([a["low_shs"], a["high_shs"]], 1), a["shs"])
    assert np.array_equal(a["culled"], inp["culled"])
