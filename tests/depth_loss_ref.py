"""The depth-prior loss of include/egs_depthloss.h stated in numpy: float64 by default, and with
``dtype=np.float32`` a float32 restatement (every product, quotient and -- pairwise, numpy's -- sum in float32), which
measures what float32 arithmetic loses on a case.  Plus the case generator and the comparison rule of the GPU tests
(tests/test_gpu_depth_loss.py), which tests/test_depth_loss_cpu.py exercises without a GPU.

A GPU result is held to 4 x the error of the float32 restatement (operation order, FMA contraction), with a floor of one
float32 ulp of the quantity's largest entry (and, for the loss, the reference's own roundings: REF_ROUNDINGS).  The L1 kinds are discontinuous where the residual e changes sign: pixels
with |e_ref| < 1e-5 max|r| are left out of the gradient comparison, and may be at most 0.2 % of the valid pixels.
"""
import numpy as np

KINDS = ("metric", "affine", "pearson")
ALPHA_MIN = 0.05
FLAT = 1e-12                    # a variance at most this share of the mean square is none
NEAR_ZERO = 1e-5                # |e| below this share of max|r|: the sign of e is not compared
EXCLUDED_CAP = 0.002            # at most this share of the valid pixels may be left out
# The float64 reference is itself exact to a few roundings of its terms only.  That matters where the loss is ZERO but for
# rounding ("affine" on one pixel or on an exact fit, "pearson" on two pixels): the loss is then a sum of differences of
# terms the size of max|r| (the L1 kinds) or 1 - rho with rho = 1 (pearson), neither known below 16 float64 roundings of
# that size -- and a float32 ulp of such a loss, the floor everywhere else, is a denormal.
REF_ROUNDINGS = 16 * 2.0 ** -53
# the shapes of the GPU tests: one pixel, rows with vector tails, several workgroups, and more float4 steps than the
# largest grid has threads (2 workgroups per CU, at most 512: 524 288 pixels), with a scalar tail of three
SHAPES = [(1, 1), (1, 2), (5, 200), (11, 11), (17, 65), (33, 129), (272, 1024), (601, 999)]


def make_case(H, W, seed=0):
    """-> float32 (D, A, q): depths z ~ U(0.5, 20) seen with opacity A ~ U(0.06, 1), D = A z; the prior is the disparity
    1 / z under a scale, a shift and noise, with 10 % of it missing."""
    rng = np.random.default_rng([seed, H, W])
    z = rng.uniform(0.5, 20.0, (H, W))
    A = rng.uniform(0.06, 1.0, (H, W))
    q = (1.0 / z - 0.03) / 1.7 + rng.normal(0.0, 0.02, (H, W))
    q[rng.random((H, W)) < 0.1] = 0.0
    return (A * z).astype(np.float32), A.astype(np.float32), q.astype(np.float32)


def valid_mask(D, A, q, alpha_min=ALPHA_MIN):
    with np.errstate(invalid="ignore"):
        return (q > 0) & np.isfinite(q) & (A > np.float32(alpha_min)) & (D > 0)


def ref(D, A, q, kind, w=None, alpha_min=ALPHA_MIN, grad_scale=1.0, dtype=np.float64, fit=None):
    """-> dict(loss, s, t, omega, rho, degenerate, dD, dA [H,W], e (the residual of the L1 kinds, else None), r, valid).
    ``D``, ``A`` may be float64 (central differences); validity is decided on them as given.  ``fit`` = (s, t): evaluate
    the "affine" loss under THAT fit (the gradient holds the fit constant)."""
    assert kind in KINDS
    T = dtype
    D, A, q = np.asarray(D), np.asarray(A), np.asarray(q)
    valid = valid_mask(D, A, q, alpha_min)
    om = np.where(valid, T(1) if w is None else np.asarray(w).astype(T), T(0)).astype(T)
    Dv = np.where(valid, D, 1).astype(T)
    inv_d = np.where(valid, T(1) / Dv, T(0)).astype(T)
    r = np.where(valid, A.astype(T) / Dv, T(0)).astype(T)
    qv = np.where(valid, q, 0).astype(T)
    out = dict(loss=0.0, s=1.0, t=0.0, omega=0.0, rho=0.0, degenerate=1, dD=np.zeros(D.shape, T), dA=np.zeros(D.shape, T),
               e=None, r=r, valid=valid, kind=kind)
    Om = om.sum(dtype=T)
    if not Om > 0:
        return out
    out["omega"] = float(Om)
    out["degenerate"] = 0
    inv = T(1) / Om
    oq, orr = om * qv, om * r
    Sq, Sqq, Sr = oq.sum(dtype=T), (oq * qv).sum(dtype=T), orr.sum(dtype=T)
    Sqr, Srr = (oq * r).sum(dtype=T), (orr * r).sum(dtype=T)
    qm, rm = Sq * inv, Sr * inv
    msq, msr = Sqq * inv, Srr * inv
    vq, vr, cov = msq - qm * qm, msr - rm * rm, Sqr * inv - qm * rm
    flat_q, flat_r = not vq > T(FLAT) * msq, not vr > T(FLAT) * msr
    if kind == "pearson":
        if flat_q or flat_r:
            out.update(loss=1.0, degenerate=1)
            return out
        sq, sr = np.sqrt(vq), np.sqrt(vr)
        k1 = T(1) / (sq * sr)
        rho = cov * k1
        dr = -(om * inv) * k1 * ((qv - qm) - (rho * sq / sr) * (r - rm))
        out.update(loss=float(T(1) - rho), rho=float(rho))
    else:
        s, t = T(1), T(0)
        if kind == "affine":
            if fit is not None:
                s, t = T(fit[0]), T(fit[1])
            elif flat_q or valid.sum() < 2:
                out["degenerate"] = 1
                s = Sqr / Sqq
            else:
                s = cov / vq
                t = rm - s * qm
        e = np.where(valid, r - (s * qv + t), T(0)).astype(T)
        out.update(loss=float((om * np.abs(e)).sum(dtype=T) * inv), s=float(s), t=float(t), e=e)
        dr = om * inv * np.sign(e)
    g = T(grad_scale) * dr
    on = om > 0
    out["dD"] = np.where(on, -g * r * inv_d, T(0)).astype(T)
    out["dA"] = np.where(on, g * inv_d, T(0)).astype(T)
    return out


def compared(want):
    """-> (bool [H,W]: the pixels whose gradient is compared, how many valid pixels are left out, how many are valid)"""
    keep = np.ones(want["valid"].shape, bool)
    n_valid = int(want["valid"].sum())
    if want["e"] is None or n_valid == 0:
        return keep, 0, n_valid
    near = want["valid"] & (np.abs(want["e"]) < NEAR_ZERO * np.abs(want["r"]).max())
    return ~near, int(near.sum()), n_valid


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


STATS = ("loss", "s", "t", "omega", "rho")


def errors(got, want):
    """``got``: dict(loss, s, t, omega, rho, dD, dA) -- the float32 restatement or a kernel's result -- against the
    float64 ``want`` -> dict of absolute errors: the five stats, and dD, dA over the compared pixels."""
    keep, _, _ = compared(want)
    e = {k: abs(float(got[k]) - want[k]) for k in STATS}
    for k in ("dD", "dA"):
        d = np.abs(np.asarray(got[k], np.float64) - want[k])[keep]
        e[k] = float(d.max()) if d.size else 0.0
    return e


def bounds(e_ref, want):
    """what a kernel's errors are held to: 4 x the float32 restatement's, at least one float32 ulp of the largest entry"""
    keep, _, _ = compared(want)
    b = {k: max(4.0 * e_ref[k], ulp32(want[k])) for k in STATS}
    b["loss"] = max(b["loss"], REF_ROUNDINGS * (1.0 if want["kind"] == "pearson" else float(np.abs(want["r"]).max())))
    for k in ("dD", "dA"):
        top = float(np.abs(want[k][keep]).max()) if keep.any() else 0.0
        b[k] = max(4.0 * e_ref[k], ulp32(top))
    return b


def check_against(got, want, what, e_ref=None, stats_only=False):
    """assert the rule; -> (errors, bounds) for a report.  ``e_ref``: the float32 restatement's errors on this case.
    ``stats_only``: "affine" where the fit is exact or degenerate (every residual is rounding, no sign to compare)"""
    _, n_out, n_valid = compared(want)
    assert stats_only or n_out <= EXCLUDED_CAP * n_valid, "%s: %d of %d valid pixels left out" % (what, n_out, n_valid)
    e, b = errors(got, want), bounds(e_ref, want)
    for k in STATS if stats_only else e:
        assert np.isfinite(e[k]) and e[k] <= b[k], "%s: %s off by %.3e, bound %.3e (float32 restatement %.3e)" % (
            what, k, e[k], b[k], e_ref[k])
    assert int(got["degenerate"]) == want["degenerate"], what
    return e, b
