"""Render extras without a GPU: the RenderOptions rules, the new C-ABI exports, and the oracle identities the GPU tests
(tests/test_gpu_render_extras.py) build their references from, pinned against a direct per-pixel loop in float64."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from easygaussiansplatting_amd import scene as S
from oracle import gs_oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_render_options_extras_validation():
    from easygaussiansplatting_amd.function import RenderOptions
    o = RenderOptions()
    assert (o.depth, o.alpha, o.background) == (False, False, None) and o.extras() is None
    o = RenderOptions(depth=True, background=[1, 0.5, 0])
    assert o.background == (1.0, 0.5, 0.0) and o.extras() == (True, False, (1.0, 0.5, 0.0))
    for kw in (dict(depth=True), dict(alpha=True), dict(background=(0.0, 0.0, 0.0))):
        with pytest.raises(ValueError):
            RenderOptions(mode="ops", **kw)
    for bad in ((1.0, 1.0), (1.0, 1.0, 1.0, 1.0), (float("nan"), 0.0, 0.0), (0.0, float("inf"), 0.0), "rgb", 3.0,
                ("a", 0.0, 0.0), (None, 0.0, 0.0)):
        with pytest.raises(ValueError):
            RenderOptions(background=bad)


def test_extras_arguments_and_abi_version():
    from easygaussiansplatting_amd import _lib
    hdr = open(os.path.join(REPO, "include", "egs_hip.h")).read()
    assert int(re.search(r"#define EGS_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION == 12
    # ABI 11: the EgsExtras* is a nullable argument of the draw and backward entry points, not separate _ex ones
    removed = ("egs_splat_draw_rec_seg_ex", "egs_fused_backward_ex", "egs_fused_backward_raw_ex")
    for name in removed:
        assert name not in _lib.SIGNATURES and name not in hdr
    from tests.test_cabi_and_host import REMOVED_IN_ABI_12, egs_names
    for name in REMOVED_IN_ABI_12:      # (whole identifiers: egs_splat_draw_rec is a prefix of the call that stays)
        assert name not in _lib.SIGNATURES and name not in egs_names(hdr), name
    assert _lib.SIGNATURES["egs_splat_draw_rec_seg"][1][-1] is C.POINTER(_lib.EgsExtras)
    assert _lib.SIGNATURES["egs_fused_backward"][1][-2] is C.POINTER(_lib.EgsExtras)
    # the ctypes mirror has the C layout: 3 pointers, 3 floats (+4 padding), 2 pointers
    f = dict((n, getattr(_lib.EgsExtras, n).offset) for n, _ in _lib.EgsExtras._fields_)
    assert f["background"] == 24 and f["dloss_ddepth"] == 40 and C.sizeof(_lib.EgsExtras) == 56
    if os.path.exists(_lib.LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
        exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
        assert "egs_splat_draw_rec_seg" in exported and "egs_fused_backward" in exported
        for name in removed + REMOVED_IN_ABI_12:
            assert name not in exported


def _tiny():
    sc = S.small_scene(60, 40, 24, 3, seed=31)
    sc.cam = S.Camera(40, 24, 60.0, 60.0, 50.0, 12.0, np.eye(3), np.array([0.0, 0.0, 5.0]))   # empty tiles on the left
    P = O.POLICY_G
    cam = sc.cam
    us, pcs, depths = O.project(sc.pws, cam.Rcw, cam.tcw, cam.fx, cam.fy, cam.cx, cam.cy, P)
    z = depths.copy()
    c3 = O.compute_cov3d(sc.rots, sc.scales, depths, P)
    c2 = O.compute_cov2d(c3, pcs, cam.Rcw, depths, cam.fx, cam.fy, cam.width, cam.height, P)
    col = O.sh2color(sc.shs, sc.pws, cam.twc)
    ci, areas = O.inverse_cov2d(c2, depths, P)
    img, cont, tau, ranges, gsid = O.splat(cam.height, cam.width, us, ci, sc.alphas, depths, col, areas, P)
    return sc, us, ci, col, z, img, cont, tau, ranges, gsid


def _loop(sc, us, ci, col, z, ranges, gsid, bg, alphas=None):
    """direct per-pixel blend of kernel.cu:152-271 with a depth and an opacity channel and a background"""
    P = O.POLICY_G
    W, H = sc.cam.width, sc.cam.height
    gx = (W + 15) // 16
    al = sc.alphas if alphas is None else alphas
    image, depth, alpha = np.zeros((3, H, W)), np.zeros((H, W)), np.zeros((H, W))
    for py in range(H):
        for px in range(W):
            t = (py // 16) * gx + px // 16
            r0, r1 = ranges[t]
            if r1 <= r0:
                image[:, py, px] = bg
                continue
            T = 1.0
            for g in gsid[r0:r1]:
                d = us[g] - (px, py)
                maha = ci[g, 0] * d[0] ** 2 + ci[g, 2] * d[1] ** 2 + 2 * ci[g, 1] * d[0] * d[1]
                a = min(0.99, al[g] * np.exp(-0.5 * max(0.0, maha)))
                if a < P.alpha_skip:
                    continue
                w = T * a
                image[:, py, px] += w * col[g]
                depth[py, px] += w * z[g]
                alpha[py, px] += w
                T *= 1 - a
                if T < P.tau_stop:
                    break
            image[:, py, px] += T * np.asarray(bg)
    return image, depth, alpha


def test_oracle_identities_forward():
    sc, us, ci, col, z, img, cont, tau, ranges, gsid = _tiny()
    bg = (0.2, 0.5, 0.9)
    W, H = sc.cam.width, sc.cam.height
    zc = np.stack([z, np.ones_like(z), np.zeros_like(z)], 1)
    ez = O.draw(W, H, ranges, gsid, us, ci, sc.alphas, zc, None, O.POLICY_G)[0]
    l_img, l_depth, l_alpha = _loop(sc, us, ci, col, z, ranges, gsid, bg)
    assert (ranges[:, 1] <= ranges[:, 0]).any() and (ranges[:, 1] > ranges[:, 0]).any()
    assert np.abs(ez[0] - l_depth).max() < 1e-12 and np.abs(ez[1] - l_alpha).max() < 1e-12
    assert np.abs(img + (1 - ez[1])[None] * np.asarray(bg)[:, None, None] - l_img).max() < 1e-12
    # alpha = 1 - T_final where the tile has patches (final_tau keeps the reference's 0 on empty tiles)
    full = ez[1] > 0
    assert np.abs(ez[1][full] - (1 - tau[full])).max() < 1e-12


def test_oracle_identities_backward():
    """the two-pass oracle gradient of <Wi,image> + <Wd,depth> + <Wa,alpha> against central differences of the loop"""
    sc, us, ci, col, z, img, cont, tau, ranges, gsid = _tiny()
    bg = np.array([0.3, 0.7, 0.1])
    W, H = sc.cam.width, sc.cam.height
    Wi, Wd, Wa = S.normal(3, 1, (3, H, W)), S.normal(3, 2, (H, W)), S.normal(3, 3, (H, W))
    P = O.POLICY_G
    zc = np.stack([z, np.ones_like(z), np.zeros_like(z)], 1)
    g1 = O.draw_backward(W, H, ranges, gsid, us, ci, sc.alphas, col, cont, tau, Wi, None, P)
    dl2 = np.stack([Wd, Wa - (Wi * bg[:, None, None]).sum(0), np.zeros_like(Wd)])
    g2 = O.draw_backward(W, H, ranges, gsid, us, ci, sc.alphas, zc, cont, tau, dl2, None, P)
    dalpha, dz = g1[2] + g2[2], g2[3][:, 0]

    def loss(alphas=None, zz=None):
        i, d, a = _loop(sc, us, ci, col, z if zz is None else zz, ranges, gsid, bg, alphas)
        return (Wi * i).sum() + (Wd * d).sum() + (Wa * a).sum()

    rows = [g for g in np.unique(gsid) if abs(dz[g]) > 1e-3][:4]
    assert rows
    h = 1e-6
    for g in rows:
        zp, zm = z.copy(), z.copy()
        zp[g] += h; zm[g] -= h
        fd = (loss(zz=zp) - loss(zz=zm)) / (2 * h)
        assert abs(fd - dz[g]) <= 1e-5 * max(1.0, abs(fd)), (g, fd, dz[g])
        ap, am = sc.alphas.astype(np.float64).copy(), sc.alphas.astype(np.float64).copy()
        ap[g] += h; am[g] -= h
        fd = (loss(alphas=ap) - loss(alphas=am)) / (2 * h)
        assert abs(fd - dalpha[g]) <= 1e-4 * max(1.0, abs(fd)), (g, fd, dalpha[g])
