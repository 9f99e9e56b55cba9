"""Float64 reference of anti-aliased rendering (``RenderOptions(antialiased=True)``).

The Mip-Splatting 2D filter keeps the +0.3 px^2 dilation of every 2D covariance and scales the opacity by

    comp = sqrt(max(0, det(Sigma)) / det(Sigma + 0.3 I)),   Sigma = the 2D covariance before the +0.3,

with comp = 0 (and no gradient) when det(Sigma) <= 0 or comp is not finite.  ``comp`` / ``comp_vjp`` take the DILATED
cov2d rows (a, b, c), b the one off-diagonal entry (the convention of the oracle's inverse_cov2d / compute_cov2d
Jacobians).  ``aa_oracle`` renders and differentiates with the oracle's own stages: ``O.draw`` / ``O.draw_backward``
with the opacity alpha comp, dL/dalpha = g comp, and dL/dcov2d = dL/dcinv2d @ dcinv2d/dcov2d + g alpha dcomp/dcov2d fed
through the oracle's Jacobians (``O.chain_rule`` restated from dL/dcov2d on)."""
import numpy as np

from oracle import gs_oracle as O

H = 0.3


def comp(cov2ds):
    """[N] compensation of dilated cov2d rows [N,3]"""
    c2 = np.asarray(cov2ds, np.float64)
    a, b, c = c2[:, 0], c2[:, 1], c2[:, 2]
    with np.errstate(all="ignore"):
        det0 = (a - H) * (c - H) - b * b
        det1 = a * c - b * b
        cm = np.sqrt(det0 / det1)
    return np.where((det0 > 0) & np.isfinite(cm), cm, 0.0)


def comp_vjp(cov2ds, g):
    """[N,3] = g dcomp/d(a, b, c); zero where comp is degenerate"""
    c2 = np.asarray(cov2ds, np.float64)
    a, b, c = c2[:, 0], c2[:, 1], c2[:, 2]
    g = np.asarray(g, np.float64)
    with np.errstate(all="ignore"):
        det0 = (a - H) * (c - H) - b * b
        det1 = a * c - b * b
        cm = np.sqrt(det0 / det1)
        ok = (det0 > 0) & np.isfinite(cm)
        d12 = det1 * det1
        dr = np.stack([((c - H) * det1 - det0 * c) / d12, 2 * b * (det0 - det1) / d12,
                       ((a - H) * det1 - det0 * a) / d12], 1)
        out = (g / (2 * cm))[:, None] * dr
    out[~ok] = 0
    return out


def aa_oracle(sc, cam, bg=None, Wi=None, Wd=None, Wa=None, antialiased=True):
    """-> dict(image over bg, depth, alpha map, ranges, comp, c2, depths[, grads of <Wi,image> + <Wd,depth> +
    <Wa,alpha>: pws, shs, alphas, scales, rots, us; and the upstream dus, dcov2d, dcolour, dz, cov3ds for pose_vjp]).
    ``sc``: arrays of the ACTIVATED parameters (pws, shs, alphas [N,1], scales, rots)."""
    P = O.POLICY_G
    us, pcs, depths, du = O.project(sc.pws, cam.Rcw, cam.tcw, cam.fx, cam.fy, cam.cx, cam.cy, P, True)
    c3, dq, ds = O.compute_cov3d(sc.rots, sc.scales, depths, P, True)
    c2, d3, dpc = O.compute_cov2d(c3, pcs, cam.Rcw, depths, cam.fx, cam.fy, cam.width, cam.height, P, True)
    twc = -np.asarray(cam.Rcw, np.float64).T @ np.asarray(cam.tcw, np.float64)
    col, dsh, dpw = O.sh2color(sc.shs, sc.pws, twc, True)
    ci, areas, dci = O.inverse_cov2d(c2, depths, P, True)
    al = np.asarray(sc.alphas, np.float64).reshape(-1)
    cm = comp(c2) if antialiased else np.ones_like(al)
    ald = al * cm                                    # the opacity as drawn
    img, cont, tau, ranges, gsid = O.splat(cam.height, cam.width, us, ci, ald, depths, col, areas, P)
    z = depths.copy()
    zc = np.stack([z, np.ones_like(z), np.zeros_like(z)], 1)
    ez = O.draw(cam.width, cam.height, ranges, gsid, us, ci, ald, zc, None, P)[0]
    bgv = np.zeros(3) if bg is None else np.asarray(bg, np.float64)
    out = dict(image=img + (1.0 - ez[1])[None] * bgv[:, None, None], depth=ez[0], alpha=ez[1], ranges=ranges, comp=cm,
               c2=c2, depths=depths)
    if Wi is None:
        return out
    Hh, Ww = cam.height, cam.width
    Wd = np.zeros((Hh, Ww)) if Wd is None else Wd
    Wa = np.zeros((Hh, Ww)) if Wa is None else Wa
    g1 = O.draw_backward(cam.width, cam.height, ranges, gsid, us, ci, ald, col, cont, tau, Wi, None, P)
    dl2 = np.stack([Wd, Wa - (Wi * bgv[:, None, None]).sum(0), np.zeros_like(Wd)])
    g2 = O.draw_backward(cam.width, cam.height, ranges, gsid, us, ci, ald, zc, cont, tau, dl2, None, P)
    dus, dcinv, gdraw = g1[0] + g2[0], g1[1] + g2[1], g1[2] + g2[2]
    dcol, dz = g1[3], g2[3][:, 0]
    # dL/dcov2d: the inverse's Jacobian term plus, anti-aliased, the comp term; dL/dalpha = g comp
    dcov2 = (dcinv[:, None, :] @ dci)[:, 0]
    if antialiased:
        dcov2 = dcov2 + comp_vjp(c2, gdraw * al)
    dalpha = gdraw * cm
    # O.chain_rule restated from dL/dcov2d on
    n = dus.shape[0]
    dcov3 = dcov2[:, None, :] @ d3
    R = np.asarray(cam.Rcw, np.float64)
    dpws = (dus[:, None, :] @ du @ R + dcol[:, None, :] @ dpw + dcov2[:, None, :] @ dpc @ R)[:, 0]
    dpws = dpws + dz[:, None] * R[2][None, :]
    out.update(pws=dpws, shs=(dcol[:, :, None] * dsh).transpose(0, 2, 1).reshape(n, -1), alphas=dalpha[:, None],
               scales=(dcov3 @ ds)[:, 0], rots=(dcov3 @ dq)[:, 0], us=dus, dcov2d=dcov2, dcolour=dcol, dz=dz,
               cov3ds=c3)
    return out
