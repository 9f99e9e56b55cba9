"""Float64 reference of ONE Gaussian row of the fused per-Gaussian kernels (k_preprocess_fwd / k_preprocess_bwd), and
the deterministic inputs of tests/test_gpu_pergaussian_matrix.py.

Nothing here is new mathematics: the forward is the oracle's five stage functions (``O.project``, ``O.compute_cov3d``,
``O.compute_cov2d``, ``O.sh2color``, ``O.inverse_cov2d``), the backward is their ``calc_J=True`` Jacobians fed through
``O.chain_rule``, the anti-aliased opacity is tests/aa_ref.py's formula and the camera pose pair is
tests/pose_ref.py's ``pose_vjp`` / ``pose_grad``.  What this module adds is the glue the kernels have and the oracle
has not: the activations of the raw training tensors in front (and their chain behind), the packed gradient record
``{dL/dalpha, dL/dcolour[3], dL/du[2], dL/dcinv2d[3], dL/dz, -, -}`` as the input of the backward, the factored SH
gradient, the exact values of near-culled rows, and the packed 2D record of the draw kernels.

Every function takes ``dtype``: float64 is the reference, float32 is the same formulas at the precision of the
tensors -- its distance from the float64 result is what the GPU test's tolerances are made of (the rule of
tests/test_gpu_mcmc.py).  ``pose_terms`` is the one exception: tests/pose_ref.py computes in float64 whatever it is
handed, and the pose pair is judged by ``assert_pose_close`` (1e-4 of sum |terms|), which needs no float32 distance.

The kernels do NOT clamp colours at zero (kernel.cu:652,725; ``O.sh2color``), so no row is excluded for its colour; the
only rows left out of a toleranced comparison are, for ``areas`` alone, rows whose float64 radius 3 sqrt(cov2d) lies
within ``RADIUS_MARGIN`` of an integer (``ceil`` is a discrete decision a float32 evaluation may take the other way)."""
import functools

import numpy as np

from easygaussiansplatting_amd import scene as S
from oracle import gs_oracle as O
from tests import aa_ref
from tests.pose_ref import pose_grad, pose_vjp
from tests.test_pose_grad_cpu import rodrigues

POLICY = O.POLICY_G
W, H = 64, 48
NHL2E = np.float32(-0.72134752044)          # -0.5 log2(e): the conic of the packed 2D record is NHL2E * cinv2d
ROW_COUNTS = (1, 2, 3, 255, 256, 257, 258, 515)
KS = (3, 12, 27, 48)
# a radius within this of an integer (relative to the radius, at least 1) may round the other way in float32: cov2d
# carries a few float32 ulps (6e-8 each) through ~30 operations, i.e. below 2e-6 relative; ten times that
RADIUS_MARGIN = 2e-5
EXCLUDED_CAP = 0.02


def seed_of(n, K):
    """the seed of the input set (n, K): one set per row count and SH width, shared by every instance and mode"""
    return 7000 + 100 * K + n


def input_sets():
    """every (n, K, seed) the GPU file uses"""
    return [(n, K, seed_of(n, K)) for K in KS for n in ROW_COUNTS]


@functools.lru_cache(maxsize=None)
def camera():
    """64 x 48 pixels, a slightly rotated camera; Rcw / tcw / twc hold float32 values (what the device sees)"""
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    R = f32(rodrigues([0.03, -0.05, 0.02]))
    t = f32([0.05, -0.08, 0.4])
    cam = S.Camera(W, H, 58.5, 61.25, 31.5, 23.75, R, t)
    return cam, f32(-R.T @ t)


@functools.lru_cache(maxsize=None)
def generate(n, K, seed):
    """-> dict of read-only float32 arrays, a pure function of (n, K, seed) on scene.py's counter generator:
    pws; the activated rots (unit), scales, alphas, shs [n,K]; the raw rots_raw (norm 0.5 .. 2), scales_raw, alphas_raw,
    low_shs [n,3], high_shs [n,K-3]; records [n,12]; culled [n] (placed behind the near plane)."""
    cam, _ = camera()
    u = lambda stream, shape: S.uniform01(seed, stream, shape)
    culled = u(1, (n,)) < 0.1
    if n >= 3:
        culled[1] = True                        # the three-row sets see a culled row too
    z = np.where(culled, -3.0 + 3.15 * u(2, (n,)), 2.0 + 6.0 * u(2, (n,)))     # culled: z in [-3, 0.15) < 0.2
    # centres inside the image with a margin: |x/z| <= 0.85 W/(2 fx), far inside the fov clamp at 1.3 W/(2 fx)
    xz = (2 * u(3, (n,)) - 1) * 0.85 * W / (2 * cam.fx)
    yz = (2 * u(4, (n,)) - 1) * 0.85 * H / (2 * cam.fy)
    pc = np.stack([xz * z, yz * z, z], 1)
    pws = (pc - cam.tcw) @ cam.Rcw              # Rcw^T (pc - tcw)
    q = S.normal(seed, 5, (n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    qn = 0.5 * 4.0 ** u(6, (n, 1))              # 0.5 .. 2
    s = 0.02 * 15.0 ** u(7, (n, 3))             # 0.02 .. 0.3
    a = 0.05 + 0.9 * u(8, (n,))
    sh = 0.3 * S.normal(seed, 9, (n, K))
    sh[:, :3] += 0.8 * S.normal(seed, 10, (n, 3))
    rec = S.normal(seed, 11, (n, 12)) * 10.0 ** (-3.0 * u(12, (n, 1)))     # mixed magnitude, row by row
    f = lambda x: np.ascontiguousarray(x, np.float32)
    d = dict(pws=f(pws), rots=f(q), scales=f(s), alphas=f(a), shs=f(sh), rots_raw=f(q * qn), scales_raw=f(np.log(s)),
             alphas_raw=f(np.log(a / (1 - a))), low_shs=f(sh[:, :3]), high_shs=f(sh[:, 3:]), records=f(rec),
             culled=culled)
    for v in d.values():
        v.setflags(write=False)
    return d


# --------------------------------------------------------------------------------------------------------- forward
def activate(inp, raw, dtype=np.float64):
    """-> pws, rots, scales, alphas, shs as the stages see them, and |rots_raw| (1 when not raw).
    RAW: gsplat/utils.py:121-150 -- normalize (eps 1e-12), exp, sigmoid, cat."""
    c = lambda k: np.asarray(inp[k], dtype)
    if not raw:
        return c("pws"), c("rots"), c("scales"), c("alphas"), c("shs"), np.ones((inp["pws"].shape[0], 1), dtype)
    r = c("rots_raw")
    norm = np.maximum(np.sqrt((r * r).sum(1, keepdims=True)), dtype(1e-12)).astype(dtype)
    alphas = (dtype(1) / (dtype(1) + np.exp(-c("alphas_raw")))).astype(dtype)
    return (c("pws"), (r / norm).astype(dtype), np.exp(c("scales_raw")).astype(dtype), alphas,
            np.concatenate([c("low_shs"), c("high_shs")], 1), norm)


def comp(cov2ds, dtype=np.float64):
    """aa_ref.comp in ``dtype``"""
    c2 = np.asarray(cov2ds, dtype)
    a, b, c = c2[:, 0], c2[:, 1], c2[:, 2]
    h = dtype(aa_ref.H)
    with np.errstate(all="ignore"):
        det0 = (a - h) * (c - h) - b * b
        det1 = a * c - b * b
        cm = np.sqrt(det0 / det1)
    return np.where((det0 > 0) & np.isfinite(cm), cm, dtype(0)).astype(dtype)


def comp_vjp(cov2ds, g, dtype=np.float64):
    """aa_ref.comp_vjp in ``dtype``"""
    c2 = np.asarray(cov2ds, dtype)
    a, b, c = c2[:, 0], c2[:, 1], c2[:, 2]
    g = np.asarray(g, dtype)
    h = dtype(aa_ref.H)
    with np.errstate(all="ignore"):
        det0 = (a - h) * (c - h) - b * b
        det1 = a * c - b * b
        cm = np.sqrt(det0 / det1)
        ok = (det0 > 0) & np.isfinite(cm)
        d12 = det1 * det1
        dr = np.stack([((c - h) * det1 - det0 * c) / d12, 2 * b * (det0 - det1) / d12,
                       ((a - h) * det1 - det0 * a) / d12], 1)
        out = (g / (2 * cm))[:, None] * dr
    out[~ok] = 0
    return out.astype(dtype)


def stages(inp, raw, cam=None, twc=None, dtype=np.float64):
    """the five stages with their Jacobians -> dict"""
    if cam is None:
        cam, twc = camera()
    pws, rots, scales, alphas, shs, qnorm = activate(inp, raw, dtype)
    us, pcs, depths, du = O.project(pws, cam.Rcw, cam.tcw, cam.fx, cam.fy, cam.cx, cam.cy, POLICY, True, dtype)
    c3, dq, ds = O.compute_cov3d(rots, scales, depths, POLICY, True, dtype)
    c2, d3, dpc = O.compute_cov2d(c3, pcs, cam.Rcw, depths, cam.fx, cam.fy, cam.width, cam.height, POLICY, True, dtype)
    col, dsh, dpw = O.sh2color(shs, pws, twc, True, dtype)
    depths = depths.copy()
    ci, areas, dci = O.inverse_cov2d(c2, depths, POLICY, True, dtype)
    return dict(pws=pws, rots=rots, scales=scales, alphas=alphas, shs=shs, qnorm=qnorm, us=us, pcs=pcs, depths=depths,
                du=du, c3=c3, dq=dq, ds=ds, c2=c2, d3=d3, dpc=dpc, col=col, dsh=dsh, dpw=dpw, ci=ci, areas=areas, dci=dci,
                live=depths >= O.MIN_DEPTH)


def forward(inp, raw, aa, dtype=np.float64, cam=None, twc=None):
    """what k_preprocess_fwd<NC, RAW, JW, AA> writes, row by row -> dict:
    us [n,2], depths [n] (-1: culled), cinv2ds [n,3], colors [n,3] (no depth test: also for culled rows), areas [n,2]
    int32, visible [n], comp [n] (1 without AA; 0 on culled rows with it), alpha_c [n] (the opacity as drawn),
    dcolor_dpws [n,9] (no depth test either), radius [n,2] (3 sqrt|cov2d|, before ceil), live [n]."""
    st = stages(inp, raw, cam, twc, dtype)
    live = st["live"]
    cm = np.where(live, comp(st["c2"], dtype), dtype(0)).astype(dtype) if aa else np.ones(live.shape[0], dtype)
    with np.errstate(all="ignore"):
        radius = dtype(3) * np.sqrt(np.abs(st["c2"][:, [0, 2]]))
    return dict(us=st["us"], depths=st["depths"], cinv2ds=st["ci"], colors=st["col"], areas=st["areas"],
                visible=st["depths"] > dtype(0.2), comp=cm, alpha_c=(st["alphas"] * cm).astype(dtype),
                dcolor_dpws=st["dpw"].reshape(-1, 9), radius=np.where(live[:, None], radius, 0), live=live)


def record_fields(fwd):
    """the documented part of the packed 2D record [n,12] (egs_gaussian_math.h make_record): centre (0, 1), conic
    NHL2E * (c0, 2 c1, c2) (2, 3, 4), the opacity as drawn (5), colour (6, 7, 8) -> [n,9] in that order"""
    ci = fwd["cinv2ds"]
    k = ci.dtype.type(NHL2E)
    return np.concatenate([fwd["us"], np.stack([k * ci[:, 0], 2 * k * ci[:, 1], k * ci[:, 2]], 1),
                           fwd["alpha_c"][:, None], fwd["colors"]], 1)


def areas_excluded(fwd64):
    """rows (of the float64 forward) whose radius is within RADIUS_MARGIN of an integer"""
    r = fwd64["radius"]
    near = np.abs(r - np.round(r)) <= RADIUS_MARGIN * np.maximum(r, 1.0)
    return (near & fwd64["live"][:, None]).any(1)


# -------------------------------------------------------------------------------------------------------- backward
def upstream(st, rec, aa, extra, dtype=np.float64):
    """the record's slots as the chain rule sees them -> (dL/dus, dL/dcov2d, dL/dcolour, dL/dz, dL/dalpha_act):
    dL/dcov2d = dL/dcinv2d @ dcinv2d/dcov2d (+ g alpha dcomp/dcov2d, anti-aliased), dL/dalpha = g (comp)"""
    rec = np.asarray(rec, dtype)
    ga, gcol, gu, gci = rec[:, 0], rec[:, 1:4], rec[:, 4:6], rec[:, 6:9]
    dz = rec[:, 9] if extra else np.zeros_like(ga)
    dcov2 = (gci[:, None, :] @ st["dci"])[:, 0]
    dalpha = ga
    if aa:
        dcov2 = dcov2 + comp_vjp(st["c2"], ga * st["alphas"], dtype)
        dalpha = ga * comp(st["c2"], dtype)
    return gu, dcov2.astype(dtype), gcol, dz, dalpha.astype(dtype)


def backward(inp, rec, raw, aa, extra, dtype=np.float64, cam=None, twc=None):
    """what k_preprocess_bwd<NC, RAW, JW, EXTRA, *, AA, false> writes for the gradient records ``rec`` [n,12] -> dict:
    dpws [n,3], dshs [n,K] (raw: also dshs_low [n,3], dshs_high [n,K-3]), dalphas [n], dscales [n,3], drots [n,4] --
    with respect to the raw tensors when ``raw`` --, dus [n,2] (the record's du, every row), dcolour [n,3] (the factored
    SH gradient) and live [n].  Culled rows: zero everywhere but dus."""
    if cam is None:
        cam, twc = camera()
    st = stages(inp, raw, cam, twc, dtype)
    n = st["live"].shape[0]
    gu, dcov2, gcol, dz, dalpha = upstream(st, rec, aa, extra, dtype)
    eye = np.broadcast_to(np.eye(3, dtype=dtype), (n, 3, 3))
    J = dict(dcinv2d_dcov2ds=eye, dcov2d_dcov3ds=st["d3"], dcov3d_drots=st["dq"], dcov3d_dscales=st["ds"],
             dcolor_dshs=st["dsh"], du_dpcs=st["du"], dcov2d_dpcs=st["dpc"], dcolor_dpws=st["dpw"])
    g = O.chain_rule(gu, dcov2, dalpha, gcol, cam.Rcw, J)         # (dcov2 through the identity: eq (3)(4)(5)(7))
    dpws = g["dpws"] + dz[:, None] * np.asarray(cam.Rcw, dtype)[2][None, :]
    drots, dscales, dalphas, dshs = g["drots"], g["dscales"], g["dalphas"], g["dshs"]
    if raw:   # normalize: (g - q (q.g)) / |r|;  exp: g s;  sigmoid: g a (1 - a)
        q, al = st["rots"], st["alphas"]
        drots = (drots - q * (q * drots).sum(1, keepdims=True)) / st["qnorm"]
        dscales = dscales * st["scales"]
        dalphas = dalphas * al * (1 - al)
    dead = ~st["live"]
    out = dict(dpws=dpws, dshs=dshs, dalphas=dalphas, dscales=dscales, drots=drots, dcolour=gcol.copy())
    for k, v in out.items():
        v = np.array(v, dtype)
        v[dead] = 0
        out[k] = v
    out["dus"] = np.array(gu, dtype)
    out["dshs_low"], out["dshs_high"] = out["dshs"][:, :3], out["dshs"][:, 3:]
    out["live"] = st["live"]
    return out


def pose_terms(inp, rec, raw, aa, extra, dtype=np.float64, cam=None):
    """per-Gaussian terms [n,12] of (dL/dRcw, dL/dtcw) for the records ``rec`` (tests/pose_ref.pose_vjp, which
    computes in float64; the upstream gradients are formed in ``dtype``); pose_ref.pose_grad sums them"""
    if cam is None:
        cam, _ = camera()
    twc = -np.asarray(cam.Rcw, np.float64).T @ np.asarray(cam.tcw, np.float64)
    st = stages(inp, raw, cam, twc, dtype)
    gu, dcov2, gcol, dz, _ = upstream(st, rec, aa, extra, dtype)
    return pose_vjp(st["pws"], st["c3"], st["shs"], cam.Rcw, cam.tcw, cam, POLICY, gu, dcov2, gcol,
                    dz if extra else None, depths=st["depths"])


def pose_pair(terms):
    """-> (dL/dRcw [3,3], dL/dtcw [3], sum |terms| [12])"""
    return pose_grad(terms)


# ------------------------------------------------------------------------------------------------------ comparison
def perturbed(inp, j):
    """the input set with every float32 value moved to a neighbouring float32 (one ulp up or down, by the counter
    generator's stream ``j``): what the same Gaussians look like to a caller that rounded them differently.  How far
    a float32 evaluation of THESE lies from the float64 reference of the original tells, row by row and without any
    kernel, how much of a row's last digits the number format can hold at all."""
    out = {}
    for i, (k, v) in enumerate(sorted(inp.items())):
        if v.dtype != np.float32:
            out[k] = v
            continue
        up = S.uniform01(977 + j, i, v.shape) < 0.5
        out[k] = np.where(up, np.nextafter(v, np.float32(np.inf)), np.nextafter(v, np.float32(-np.inf))).astype(np.float32)
    # low_shs / high_shs and shs are the same numbers; keep them so
    if "shs" in out and out["low_shs"].shape[0]:
        out["low_shs"], out["high_shs"] = np.ascontiguousarray(out["shs"][:, :3]), np.ascontiguousarray(out["shs"][:, 3:])
    return out


def row_errors(got, ref, scale_with=None):
    """per row: max_j |got - ref| / max_j |ref| (0 where the row's scale is 0) -> (rel [n], scale [n], abs err [n])"""
    got = np.asarray(got, np.float64).reshape(len(ref), -1)
    ref = np.asarray(ref, np.float64).reshape(len(ref), -1)
    scale = np.abs(ref).max(1)
    for s in scale_with or ():
        scale = np.maximum(scale, np.abs(np.asarray(s, np.float64).reshape(len(ref), -1)).max(1))
    err = np.abs(got - ref).max(1)
    with np.errstate(all="ignore"):
        rel = np.where(scale == 0, 0.0, err / np.where(scale == 0, 1.0, scale))
    return rel, scale, err


def row_error(got, ref, scale_with=None):
    """max over rows of max_j |got - ref| / max_j |ref| of the row (``scale_with``: more arrays whose row maxima join
    the scale, e.g. the old gradient of an accumulating call).  Rows whose scale is zero must be matched exactly;
    -> (error, number of zero-scale rows that differ, index of the worst row)"""
    if len(ref) == 0 or np.asarray(ref).size == 0:
        return 0.0, 0, -1
    got = np.asarray(got, np.float64).reshape(len(ref), -1)
    ref = np.asarray(ref, np.float64).reshape(len(ref), -1)
    scale = np.abs(ref).max(1)
    for s in scale_with or ():
        scale = np.maximum(scale, np.abs(np.asarray(s, np.float64).reshape(len(ref), -1)).max(1))
    err = np.abs(got - ref).max(1)
    zero = scale == 0
    with np.errstate(all="ignore"):
        rel = np.where(zero, 0.0, err / np.where(zero, 1.0, scale))
    if not np.isfinite(got).all():
        return float("inf"), int((zero & (err != 0)).sum()), int(np.argmax(~np.isfinite(got).all(1)))
    return float(rel.max()), int((zero & (err != 0)).sum()), int(np.argmax(rel))
