"""The splat / splatB stage through RAW C-ABI calls (include/egs_hip.h), one tensor form and one records form per stage:

1. the literal seven-op sequence a reference maintainer binds: ``egs_splat_bin`` -> read
   ``total_patches`` -> ``egs_splat_draw`` -> ``egs_splat_bwd``, all from tensors -- the draw packs its own records, which
   ``gsplatcu.splat`` (it always packs first) never does;
2. the records form with everything optional given: ``egs_splat_bin_pack`` -> ``egs_splat_draw_rec_seg`` with the count on
   the device, capacity-sized buffers, the masked and the plain list, a ``tile_order`` buffer and ``grad_records`` ->
   ``egs_splat_bwd_seg`` from the records alone;
3. the degenerate counts, n == 0 and P == 0, through both.

The forward draw has no atomics: its outputs are compared bitwise (``torch.equal``) with ``gsplatcu.splat`` on clones of
the same inputs.  The backward draw accumulates with float atomics: gradients are compared with ``gsplatcu.splatB`` by
``tests/gradcheck.assert_grad_close`` with its default parameters.  Smallest shapes with every branch: 2000 Gaussians of
``scene.small_scene`` (some behind the camera), 150 x 70 pixels = 10 x 5 tiles, partial tiles on both edges."""
import ctypes as C

import numpy as np
import pytest
import torch

from easygaussiansplatting_amd import scene as S
from tests.gradcheck import assert_grad_close

pytestmark = pytest.mark.gpu

N, W, H = 2000, 150, 70
MASKED_LISTS = 2            # include/egs_hip.h EGS_DRAW_MASKED_LISTS


@pytest.fixture()
def env():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from easygaussiansplatting_amd import _lib, fused, gsplatcu
    gsplatcu.set_policy("gsplatcu")
    gsplatcu.set_memo(False)
    keep_states = gsplatcu.set_pair_states(False)
    keep_seg, fused.SEGMENTS = fused.SEGMENTS, "0"
    yield gsplatcu, _lib.load()
    fused.SEGMENTS = keep_seg
    gsplatcu.set_pair_states(keep_states)
    gsplatcu.set_memo(False)
    gsplatcu.set_policy("gsplatcu")


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _check(lib, rc):
    assert rc == 0, (rc, lib.egs_last_error_string())


def _pol():
    from easygaussiansplatting_amd import _host
    return _host._pol()


def _inputs(gsc, n=N, behind="some"):
    """the 2D Gaussians of the five per-Gaussian ops under the current policy (+ an upstream gradient)"""
    sc = S.small_scene(max(n, 1), W, H, 3, seed=11)
    if behind == "some":
        sc.pws[:200, 2] -= 8.0          # camera-space z in [-5, -1]
    elif behind == "all":
        sc.pws[:, 2] -= 10.0
    cam = sc.cam
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)[:n]).cuda()
    pws, rots, scales, alphas, shs = map(dev, (sc.pws, sc.rots, sc.scales, sc.alphas, sc.shs))
    Rcw, tcw, twc = (torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda() for a in (cam.Rcw, cam.tcw, cam.twc))
    us, pcs, depths = gsc.project(pws, Rcw, tcw, cam.fx, cam.fy, cam.cx, cam.cy, False)
    cov3 = gsc.computeCov3D(rots, scales, depths, False)[0]
    cov2 = gsc.computeCov2D(cov3, pcs, Rcw, depths, cam.fx, cam.fy, cam.width, cam.height, False)[0]
    col = gsc.sh2Color(shs, pws, twc, False)[0]
    cinv, areas = gsc.inverseCov2D(cov2, depths, False)
    dl = torch.from_numpy(S.normal(3, 1, (3, H, W)).astype(np.float32)).cuda() / (3 * H * W)
    return dict(us=us, cinv=cinv, alphas=alphas.reshape(-1).contiguous(), depths=depths, col=col, areas=areas, dl=dl)


def _draw_outputs():
    e = lambda shape, dt: torch.empty(shape, dtype=dt, device="cuda")
    T = ((W + 15) // 16) * ((H + 15) // 16)
    return e((3, H, W), torch.float32), e((H, W), torch.int32), e((H, W), torch.float32), e((T, 2), torch.int32)


def _grad_outputs(n):
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")
    return nan(n, 2), nan(n, 3), nan(n), nan(n, 3)


def _literal(lib, d):
    """egs_splat_bin -> read total_patches -> egs_splat_draw -> egs_splat_bwd, from tensors
    -> (five forward outputs, depths, areas after the in-place cull, four gradients, P)"""
    n, pol, st = d["us"].shape[0], C.byref(_pol()), _stream()
    depths, areas = d["depths"].clone(), d["areas"].clone()
    ws_bin = torch.empty(lib.egs_splat_bin_ws_bytes(n), dtype=torch.uint8, device="cuda")
    total = torch.zeros(2, dtype=torch.int32, device="cuda")
    _check(lib, lib.egs_splat_bin(n, W, H, _ptr(d["us"]), _ptr(areas), _ptr(depths), pol, 0, _ptr(ws_bin), ws_bin.numel(),
                                  _ptr(total), st))
    P = int(total[0].item())                            # the one read-back of the op (gausplat.cu:67)
    image, contrib, tau, ranges = _draw_outputs()
    gsid = torch.empty(P, dtype=torch.int32, device="cuda")
    ws_draw = torch.empty(lib.egs_splat_draw_ws_bytes(n, P, W, H), dtype=torch.uint8, device="cuda")
    _check(lib, lib.egs_splat_draw(n, P, W, H, _ptr(d["us"]), _ptr(d["cinv"]), _ptr(d["alphas"]), _ptr(d["col"]),
                                   _ptr(areas), pol, _ptr(ws_bin), _ptr(ws_draw), ws_draw.numel(), _ptr(image),
                                   _ptr(contrib), _ptr(tau), _ptr(ranges), _ptr(gsid), st))
    ws = torch.empty(lib.egs_splat_bwd_ws_bytes(n), dtype=torch.uint8, device="cuda")
    grads = _grad_outputs(n)
    _check(lib, lib.egs_splat_bwd(n, P, W, H, _ptr(d["us"]), _ptr(d["cinv"]), _ptr(d["alphas"]), _ptr(d["col"]),
                                  _ptr(areas), pol, _ptr(contrib), _ptr(tau), _ptr(ranges), _ptr(gsid), _ptr(d["dl"]),
                                  _ptr(ws), ws.numel(), *map(_ptr, grads), st))
    torch.cuda.synchronize()
    return [image, contrib, tau, ranges, gsid], depths, areas, grads, P


def _records(lib, d, cap):
    """egs_splat_bin_pack -> egs_splat_draw_rec_seg (count on the device, buffers of ``cap`` entries, both lists, order
    buffer, gradient records) -> egs_splat_bwd_seg from the records alone
    -> (image, contrib, tau, ranges, plain list, masked list, four gradients, P)"""
    n, pol, st = d["us"].shape[0], C.byref(_pol()), _stream()
    depths, areas = d["depths"].clone(), d["areas"].clone()
    ws_bin = torch.empty(lib.egs_splat_bin_ws_bytes(n), dtype=torch.uint8, device="cuda")
    total = torch.zeros(2, dtype=torch.int32, device="cuda")
    rec = torch.empty((max(n, 1), 12), dtype=torch.float32, device="cuda")
    _check(lib, lib.egs_splat_bin_pack(n, W, H, _ptr(d["us"]), _ptr(d["cinv"]), _ptr(d["alphas"]), _ptr(d["col"]),
                                       _ptr(areas), _ptr(depths), pol, 0, _ptr(ws_bin), ws_bin.numel(), _ptr(total),
                                       None, _ptr(rec), None, None, st))
    image, contrib, tau, ranges = _draw_outputs()
    masked = torch.empty(cap, dtype=torch.int32, device="cuda")
    plain = torch.empty(cap, dtype=torch.int32, device="cuda")
    order = torch.empty(lib.egs_tile_order_len(W, H), dtype=torch.int32, device="cuda")
    gpack = torch.full((max(n, 1), 12), float("nan"), dtype=torch.float32, device="cuda")   # (the draw clears them)
    ws_draw = torch.empty(lib.egs_splat_draw_ws_bytes(n, cap, W, H), dtype=torch.uint8, device="cuda")
    _check(lib, lib.egs_splat_draw_rec_seg(n, cap, _ptr(total), W, H, _ptr(rec), pol, _ptr(ws_bin), _ptr(ws_draw),
                                           ws_draw.numel(), _ptr(image), _ptr(contrib), _ptr(tau), _ptr(ranges),
                                           _ptr(masked), _ptr(order), _ptr(gpack), None, 0, MASKED_LISTS, None, 0, None,
                                           None, _ptr(plain), st, None))
    P = int(total[0].item())
    assert P <= cap
    ws = torch.empty(lib.egs_splat_bwd_ws_bytes(n), dtype=torch.uint8, device="cuda")
    grads = _grad_outputs(n)
    _check(lib, lib.egs_splat_bwd_seg(n, P, W, H, None, None, None, None, _ptr(rec), pol, _ptr(contrib), _ptr(tau),
                                      _ptr(ranges), _ptr(masked), _ptr(d["dl"]), _ptr(ws), ws.numel(), _ptr(order),
                                      _ptr(gpack), *map(_ptr, grads), MASKED_LISTS, None, 0, 0, None, st))
    torch.cuda.synchronize()
    return image, contrib, tau, ranges, plain, masked, grads, P


def _reference(gsc, d, policy):
    """gsplatcu.splat / splatB on clones of the same inputs"""
    c = {k: v.clone() for k, v in d.items()}
    out = gsc.splat(H, W, c["us"], c["cinv"], c["alphas"], c["depths"], c["col"], c["areas"])
    g = gsc.splatB(H, W, c["us"], c["cinv"], c["alphas"], c["depths"], c["col"], out[1], out[2], out[3], out[4], c["dl"],
                   areas=c["areas"] if policy == "forward_cpu" else None)
    torch.cuda.synchronize()
    return out, c["depths"], c["areas"], g


GRAD_NAMES = ("dloss_dus", "dloss_dcinv2ds", "dloss_dalphas", "dloss_dcolors")


def _grads_close(got, ref, what):
    for a, b, name in zip(got, ref, GRAD_NAMES):
        a, b = a.cpu().numpy(), b.cpu().numpy()
        assert_grad_close(a.reshape(b.shape), b, "%s %s" % (what, name))


@pytest.mark.parametrize("policy", ["gsplatcu", "forward_cpu"])
def test_literal_tensor_sequence_equals_the_op_surface(env, policy):
    gsc, lib = env
    gsc.set_policy(policy)
    d = _inputs(gsc)
    out, depths, areas, grads, P = _literal(lib, d)
    ref_out, ref_depths, ref_areas, ref_grads = _reference(gsc, d, policy)
    assert P == ref_out[4].shape[0] and P > 100
    assert int((d["depths"] < 0.2).sum()) >= 100               # (some Gaussians are behind the camera)
    for a, b, name in zip(out, ref_out, ("image", "contrib", "final_tau", "patch_range_per_tile", "gsid_per_patch")):
        assert torch.equal(a, b), name
    assert torch.equal(depths, ref_depths) and torch.equal(areas, ref_areas)      # the in-place cull of the binning
    assert float(out[0].abs().max()) > 0 and int(out[1].max()) > 0
    _grads_close(grads, ref_grads, "literal " + policy)


def test_records_form_with_every_option_equals_the_literal_sequence(env):
    gsc, lib = env
    d = _inputs(gsc)
    out, _, _, grads, P = _literal(lib, d)
    cap = P + max(1, P * 6 // 100)                              # the device count, not the capacity, bounds every kernel
    image, contrib, tau, ranges, plain, masked, rgrads, P2 = _records(lib, d, cap)
    assert P2 == P
    for a, b, name in zip((image, contrib, tau, ranges), out, ("image", "contrib", "final_tau", "patch_range_per_tile")):
        assert torch.equal(a, b), name
    assert torch.equal(plain[:P], out[4])                       # the reference's list (gausplat.cu:108-111)
    assert torch.equal(masked[:P] & 0x0FFFFFFF, out[4])         # the list the draw kernels walked: masks above bit 28
    assert bool(((masked[:P].to(torch.int64) & 0xFFFFFFFF) >> 28).max() > 0)
    _grads_close(rgrads, grads, "records")


@pytest.mark.parametrize("case", ["n0", "p0"])
def test_degenerate_counts(env, case):
    gsc, lib = env
    d = _inputs(gsc, n=0 if case == "n0" else N, behind="all")
    n = d["us"].shape[0]
    assert n == (0 if case == "n0" else N)
    out, _, _, grads, P = _literal(lib, d)
    rec_out = _records(lib, d, 64)
    assert P == 0 and rec_out[-1] == 0
    for t in tuple(out[:4]) + tuple(rec_out[:4]):
        assert int(torch.count_nonzero(t)) == 0
    assert out[4].numel() == 0
    for g in tuple(grads) + tuple(rec_out[6]):
        assert g.shape[0] == n and int(torch.count_nonzero(g)) == 0 and bool(torch.isfinite(g).all())
