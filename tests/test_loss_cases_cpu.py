"""The yardsticks of tests/test_gpu_loss.py, checked without a GPU: the autograd restatement ``loss_cases.ref64`` against
the analytic float64 oracle ``gs_oracle.gau_loss`` in every regime the GPU tests lean on (the oracle's own fixtures,
g7_gau_loss.npz, are three noise images), and what the reference's float32 formulation loses there."""
import numpy as np
import pytest

from oracle import gs_oracle as O

torch = pytest.importorskip("torch")
from tests import loss_cases as LC  # noqa: E402

SHAPES = [(9, 7), (23, 70), (40, 130)]
LAMBDAS = (0.0, 0.2, 1.0)

# "Equal to float64 rounding" for two summation orders of the same window (121 products at once in ref64, 11 + 11 in
# the oracle).  A window sum of terms of size v^2, v = max(1, |x|, |y|), carries at most 121 eps v^2; the difference
# E[x^2] - mu^2 passes that on unscaled, and the SSIM map and its derivative maps divide by B2 >= C2 = 9e-4 once and
# twice: 121 * 2.2e-16 * 16 / 9e-4 = 5e-10 for the map (hdr, v = 4), 121 * 2.2e-16 / 9e-4^2 = 3e-8 for the gradient of the
# flat pairs (v = 1), each taken against the gradient's unit u.  These are worst cases (every rounding the same way);
# a factor 2 error in one term of the gradient is seven orders of magnitude beyond them.
TOL_LOSS = 1e-9
TOL_GRAD = 1e-7


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("kind", LC.KINDS)
def test_ref64_equals_analytic_oracle(kind, shape):
    x, y = LC.make_pair(kind, *shape)
    assert x.dtype == np.float32 and y.dtype == np.float32 and x.shape == y.shape == (3,) + shape
    for lam in LAMBDAS:
        lo, go, aux = O.gau_loss(x, y, lam, calc_grad=True)
        l64, g64, s64 = LC.ref64(x, y, lam)
        assert abs(l64 - lo) <= TOL_LOSS and abs(s64 - aux["ssim"]) <= TOL_LOSS, (lam, l64, lo, s64, aux["ssim"])
        e = LC.grad_error(g64.numpy(), go)
        assert e <= TOL_GRAD, (lam, e)


def test_pairs_are_what_they_claim():
    H, W = 40, 130
    P = {k: LC.make_pair(k, H, W) for k in LC.KINDS}
    for k, (x, y) in P.items():
        assert np.isfinite(x).all() and np.isfinite(y).all(), k
        x2, y2 = LC.make_pair(k, H, W)
        assert np.array_equal(x, x2) and np.array_equal(y, y2), k          # seeded: a pure function of its arguments
    x, y = P["identical"]
    assert np.array_equal(x, y) and x.std() > 0.1
    x, y = P["flat"]
    assert (x == np.float32(0.9)).all() and 5e-4 < np.abs(y - x).std() < 2e-3
    x, y = P["shifted"]
    assert np.array_equal(y[:, :, 1:], x[:, :, :-1])
    x, y = P["dark"]
    assert (x == 0).all() and 0 <= y.min() and y.max() < 0.01
    x, y = P["quantised"]
    for a in (x, y):
        assert np.array_equal(a, np.rint(a * 255).astype(np.float32) / np.float32(255))
    same = (x == y).mean()
    assert 0.45 < same < 0.75, same
    assert ((x > y).mean() > 0.1) and ((x < y).mean() > 0.1)
    x, y = P["hdr"]
    assert x.min() < -0.4 and x.max() > 3.9 and 0 <= y.min() and y.max() < 1
    x, y = P["rendered"]
    d = np.abs(x - y)
    assert y.max() > 0.3 and 0 < d.max() < 0.2 and (d > 0).mean() > 0.2      # a few per cent apart, over the drawn part
    # the smooth kinds are the cancelling regime: window variances far below the squared means
    g = O.ssim_window()
    for k in ("flat", "identical", "ramps", "shifted"):
        x = P[k][0].astype(np.float64)
        mu = O._conv_sep(x, g)[:, 5:-5, 5:-5]; var = O._conv_sep(x * x, g)[:, 5:-5, 5:-5] - mu * mu
        assert np.median(var / (mu * mu)) < 1e-3, k


def test_ref32_error_table(capsys):
    """Re-derives the table in loss_cases' docstring.  Only finiteness is asserted: the figures are the reference's, and
    the GPU rule recomputes them on every run."""
    rows = []
    for kind in LC.KINDS:
        x, y = LC.make_pair(kind, 70, 150)
        lo, go, aux = O.gau_loss(x, y, 0.2, calc_grad=True)
        e = LC.errors(LC.ref32(x, y, 0.2), (lo, go, aux["ssim"]))
        assert all(np.isfinite(v) for v in e.values()), (kind, e)
        rows.append("    %-10s  %12.1e  %19.1e" % (kind, e["d_loss"], e["e_grad"]))
    with capsys.disabled():
        print("\n    kind        |loss32 - loss64|   max|grad32 - grad64| / u\n" + "\n".join(rows))


def test_rule_takes_its_bound_from_the_reference():
    ok = dict(e_grad=3e-4, d_loss=5e-5, d_ssim=5e-5)
    LC.check_against(dict(e_grad=5.9e-4, d_loss=9e-5, d_ssim=9e-5), ok)
    LC.check_against(dict(e_grad=9e-5, d_loss=9e-6, d_ssim=9e-6), dict(e_grad=0.0, d_loss=0.0, d_ssim=0.0))
    for bad in (dict(e_grad=6.1e-4, d_loss=0, d_ssim=0), dict(e_grad=0, d_loss=1.1e-4, d_ssim=0),
                dict(e_grad=0, d_loss=0, d_ssim=1.1e-4), dict(e_grad=float("nan"), d_loss=0, d_ssim=0)):
        with pytest.raises(AssertionError):
            LC.check_against(bad, ok)
    g64 = np.zeros((3, 2, 2)); g = g64.copy(); g[0, 0, 0] = 1.0 / 12
    assert LC.grad_error(g, g64) == pytest.approx(1.0)                       # u = 1 / M when the exact gradient is 0
    g[1, 1, 1] = np.nan
    assert np.isnan(LC.grad_error(g, g64))
