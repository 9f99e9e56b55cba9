"""Float64 reference of the camera pose gradient (the VJP k_preprocess_bwd_pose + k_pose_reduce form).

Given per-Gaussian upstream gradients -- dL/dus [N,2], dL/dcov2d [N,3], dL/dcolour [N,3] and, with render extras,
dL/dz [N] -- and the scene, ``pose_vjp`` returns the contribution of every Gaussian to dL/dRcw (9, row-major) and
dL/dtcw (3) as an [N,12] array; the pose gradient is its column sum.  The stages are the oracle's
(``O.project``, ``O.compute_cov2d``, ``O.sh2color``), with the camera centre twc = -Rcw^T tcw:

* through p_c = Rcw pw + tcw (projection, the J(p_c) factor of cov2d with the oracle's own dcov2d/dpc, depth):
  dL/dtcw += gpc, dL/dRcw += gpc pw^T;
* through the W = Rcw factor of cov2d = (J W) Sigma (J W)^T, J held (clamped x/z, y/z as compute_cov2d):
  dL/dRcw += J^T dL/dM, dL/dM = [2 g0 v0 + g1 v1 ; g1 v0 + 2 g2 v1] with v = Sigma M^T;
* through the view direction of the SH colour: dL/dtwc = -gcol^T dcolor/dpw, folded back per Gaussian:
  dL/dRcw[r][k] -= tcw[r] dL/dtwc[k], dL/dtcw -= Rcw dL/dtwc.

Where the fov clamp binds, dcov2d/dpc is the reference's (it differentiates J as if x, y were not clamped), as the
per-Gaussian dL/dpw of the fused path: the p_c term then follows the reference, not the exact derivative.  Every
other term is the exact derivative."""
import numpy as np

from oracle import gs_oracle as O


def dcov2d_from_dcinv(dcinv2ds, dcinv2d_dcov2ds):
    """dL/dcov2d from dL/dcinv2d and the oracle's inverse_cov2d Jacobian"""
    return (np.asarray(dcinv2ds, np.float64)[:, None, :] @ dcinv2d_dcov2ds)[:, 0]


def pose_vjp(pws, cov3ds, shs, Rcw, tcw, cam, policy, dus, dcov2ds, dcolors, dz=None, depths=None, parts=False):
    """-> [N,12] per-Gaussian terms {dL/dRcw (9), dL/dtcw (3)} (twc fold applied); ``parts``: also a dict of the
    unfolded terms "pc" [N,12], "W" [N,9] and "twc" [N,3].  ``cam`` supplies fx, fy, cx, cy, width, height.
    ``depths`` (optional): the forward's depths after every cull (near and NaN); Gaussians below 0.2 there contribute
    nothing when the policy culls.  By default they are recomputed from the pose."""
    f64 = lambda a: np.asarray(a, np.float64)
    pws, cov3ds, R, t = f64(pws), f64(cov3ds), f64(Rcw), f64(tcw)
    n = pws.shape[0]
    twc = -R.T @ t
    us, pcs, dep, du = O.project(pws, R, t, cam.fx, cam.fy, cam.cx, cam.cy, policy, True)
    if depths is None:
        depths = dep
    _, _, dpc = O.compute_cov2d(cov3ds, pcs, R, dep, cam.fx, cam.fy, cam.width, cam.height, policy, True)
    _, _, dcol_dpw = O.sh2color(shs, pws, twc, True)
    g2 = f64(dcov2ds)
    gpc = (f64(dus)[:, None, :] @ du)[:, 0] + (g2[:, None, :] @ dpc)[:, 0]
    if dz is not None:
        gpc[:, 2] += f64(dz)
    # the W factor: J of compute_cov2d (clamped x, y), M = J R, v = Sigma M^T
    limx, limy = O.fov_limits(cam.fx, cam.fy, cam.width, cam.height, policy)
    pc = pws @ R.T + t
    z = pc[:, 2]
    with np.errstate(all="ignore"):
        x = np.clip(pc[:, 0] / z, -limx, limx) * z if np.isfinite(limx) else pc[:, 0]
        y = np.clip(pc[:, 1] / z, -limy, limy) * z if np.isfinite(limy) else pc[:, 1]
        J = np.zeros((n, 2, 3))
        J[:, 0, 0] = cam.fx / z; J[:, 0, 2] = -(cam.fx * x) / (z * z)
        J[:, 1, 1] = cam.fy / z; J[:, 1, 2] = -(cam.fy * y) / (z * z)
    M = J @ R
    a, b, c, d, e, f = (cov3ds[:, i] for i in range(6))
    Sig = np.stack([np.stack([a, b, c], 1), np.stack([b, d, e], 1), np.stack([c, e, f], 1)], 1)
    V = Sig @ M.transpose(0, 2, 1)                  # columns v0, v1
    v0, v1 = V[:, :, 0], V[:, :, 1]
    gM = np.stack([2 * g2[:, 0:1] * v0 + g2[:, 1:2] * v1, g2[:, 1:2] * v0 + 2 * g2[:, 2:3] * v1], 1)
    gW = (J.transpose(0, 2, 1) @ gM).reshape(n, 9)
    gtwc = -(f64(dcolors)[:, None, :] @ dcol_dpw)[:, 0]
    pc_terms = np.concatenate([(gpc[:, :, None] * pws[:, None, :]).reshape(n, 9), gpc], 1)
    out = pc_terms.copy()
    out[:, :9] += gW
    out[:, :9] -= (t[None, :, None] * gtwc[:, None, :]).reshape(n, 9)
    out[:, 9:] -= gtwc @ R.T
    if policy.near_cull:
        off = ~(np.asarray(depths) >= O.MIN_DEPTH)
        out[off] = 0
        pc_terms[off] = 0; gW[off] = 0; gtwc[off] = 0
    if parts:
        return out, dict(pc=pc_terms, W=gW, twc=gtwc)
    return out


def pose_grad(terms):
    """-> (dL/dRcw [3,3], dL/dtcw [3], scale [12] = sum_i |term_i| per component)"""
    s = terms.sum(0)
    return s[:9].reshape(3, 3), s[9:], np.abs(terms).sum(0)
