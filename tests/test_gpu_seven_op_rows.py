"""The seven-op kernels and k_chain_rule at ragged row counts, bit for bit, through the C ABI alone.

These kernels hand their rows to ``rows_out<K>`` (csrc/egs_rows.h): the workgroup's 256 rows leave through LDS as float4
pieces of one contiguous span, and when the LAST workgroup's row count times K is no multiple of four, up to three
floats leave one by one behind the pieces.  Every scene size of the other GPU tests is a multiple of four, so that tail
never runs for them.  The kernels are row-independent and have no atomics, so the test is: rows 0 .. n-1 of a call on
the first n rows equal, word for word, the same rows of the call on all 515, and nothing is written in front of or
behind an output (``gpu_abi.Out``: sentinel bands).  No tolerance anywhere; the values themselves are held to the
oracle by tests/test_gpu_parity.py.

Inputs: ONE seeded set of 515 rows per SH width (``small_scene(515, 64, 48, K)``: two full workgroups and a last one of
three rows) and seeded upstream gradients for ``egs_chain_rule``.  Row counts: 1, 2, 3 (a lone workgroup with 3, 6, 9
floats of a 3-float output: no whole piece / one and a tail / two and a tail), 255, 256, 257, 258 (around the workgroup
boundary, the last workgroup with 1 and 2 rows) and 515.  Row widths that occur: 1, 2 (direct stores), 3, 9, 27 (odd:
the span unpadded), 6, 18 (padded rows, gathered), 4, 12, 16, 24, 48 (float4 rows)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from easygaussiansplatting_amd import scene as S
from tests.gpu_abi import DEV, Out, _check, _pol, _ptr, _stream

N, W, H = 515, 64, 48
SEED = 5150
COUNTS = (1, 2, 3, 255, 256, 257, 258, 515)
OPS = ("project", "cov3d", "cov2d", "sh2color", "inv_cov2d", "chain_rule")


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from easygaussiansplatting_amd import _lib, gsplatcu
    gsplatcu.set_policy("gsplatcu")
    yield _lib.load()
    gsplatcu.set_policy("gsplatcu")


@functools.lru_cache(maxsize=None)
def inputs(K):
    """the 515 rows and their upstream gradients (float32, read-only)"""
    sc = S.small_scene(N, W, H, K, seed=SEED)
    f = lambda x: np.ascontiguousarray(x, np.float32)
    d = dict(pws=f(sc.pws), rots=f(sc.rots), scales=f(sc.scales), shs=f(sc.shs), g_us=f(S.normal(SEED, 21, (N, 2))),
             g_cinv=f(S.normal(SEED, 22, (N, 3))), g_colors=f(S.normal(SEED, 23, (N, 3))))
    for v in d.values():
        v.setflags(write=False)
    return d, sc.cam


def run(lib, K, n):
    """the five ops with their Jacobians and the chain rule on rows 0 .. n-1 -> {op: {output: int32 words [n, width]}}"""
    inp, cam = inputs(K)
    dev = lambda a: torch.from_numpy(np.array(a)).to(DEV)          # (a copy: the set itself is read-only)
    t = {k: dev(v[:n]) for k, v in inp.items()}
    Rcw, tcw, twc = (dev(np.asarray(a, np.float32)) for a in (cam.Rcw, cam.tcw, cam.twc))
    pol, s = C.byref(_pol()), _stream()
    NC = K // 3
    o = dict(project=dict(us=Out(2 * n), pcs=Out(3 * n), depths=Out(n), du_dpcs=Out(6 * n)),
             cov3d=dict(cov3ds=Out(6 * n), dcov3d_drots=Out(24 * n), dcov3d_dscales=Out(18 * n)),
             cov2d=dict(cov2ds=Out(3 * n), dcov2d_dcov3ds=Out(18 * n), dcov2d_dpcs=Out(9 * n)),
             sh2color=dict(colors=Out(3 * n), dcolor_dshs=Out(NC * n), dcolor_dpws=Out(9 * n)),
             inv_cov2d=dict(cinv2ds=Out(3 * n), areas=Out(2 * n), dcinv2d_dcov2ds=Out(9 * n)),
             chain_rule=dict(dpws=Out(3 * n), dshs=Out(K * n), dscales=Out(3 * n), drots=Out(4 * n)))
    p, c3, c2, sh, ci, cr = (o[k] for k in OPS)
    _check(lib, lib.egs_project(n, _ptr(t["pws"]), _ptr(Rcw), _ptr(tcw), cam.fx, cam.fy, cam.cx, cam.cy, pol,
                                p["us"].ptr, p["pcs"].ptr, p["depths"].ptr, p["du_dpcs"].ptr, s))
    _check(lib, lib.egs_cov3d(n, _ptr(t["rots"]), _ptr(t["scales"]), p["depths"].ptr, pol, c3["cov3ds"].ptr,
                              c3["dcov3d_drots"].ptr, c3["dcov3d_dscales"].ptr, s))
    _check(lib, lib.egs_cov2d(n, c3["cov3ds"].ptr, p["pcs"].ptr, _ptr(Rcw), p["depths"].ptr, cam.fx, cam.fy, float(W),
                              float(H), pol, c2["cov2ds"].ptr, c2["dcov2d_dcov3ds"].ptr, c2["dcov2d_dpcs"].ptr, s))
    _check(lib, lib.egs_sh2color(n, K, _ptr(t["shs"]), _ptr(t["pws"]), _ptr(twc), sh["colors"].ptr,
                                 sh["dcolor_dshs"].ptr, sh["dcolor_dpws"].ptr, s))
    # (inverse_cov2d marks a degenerate Gaussian in depths, in place: read below, after the last op, with its bands)
    _check(lib, lib.egs_inv_cov2d(n, c2["cov2ds"].ptr, p["depths"].ptr, pol, ci["cinv2ds"].ptr, ci["areas"].ptr,
                                  ci["dcinv2d_dcov2ds"].ptr, s))
    _check(lib, lib.egs_chain_rule(n, K, _ptr(t["g_us"]), _ptr(t["g_cinv"]), _ptr(t["g_colors"]), _ptr(Rcw),
                                   ci["dcinv2d_dcov2ds"].ptr, c2["dcov2d_dcov3ds"].ptr, c3["dcov3d_drots"].ptr,
                                   c3["dcov3d_dscales"].ptr, sh["dcolor_dshs"].ptr, p["du_dpcs"].ptr,
                                   c2["dcov2d_dpcs"].ptr, sh["dcolor_dpws"].ptr, cr["dpws"].ptr, cr["dshs"].ptr,
                                   cr["dscales"].ptr, cr["drots"].ptr, s))
    torch.cuda.synchronize()
    return {op: {k: out.read((K, n, op, k)).reshape(n, -1) for k, out in outs.items()} for op, outs in o.items()}


@functools.lru_cache(maxsize=None)
def all_rows(lib, K):
    """the call on all 515 rows: computed once per SH width, read-only"""
    got = run(lib, K, N)
    for outs in got.values():
        for v in outs.values():
            v.setflags(write=False)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("K", [3, 12, 27, 48])
def test_first_n_rows_equal_the_rows_of_the_full_call(lib, K):
    base = all_rows(lib, K)
    for n in COUNTS:
        got = base if n == N else run(lib, K, n)
        for op in OPS:
            assert any(v.any() for v in got[op].values()), (K, n, op, "every output is zero")
            for k, g in got[op].items():
                want = base[op][k][:n]
                bad = np.nonzero((g != want).any(1))[0]
                assert bad.size == 0, (K, n, op, k, "%d rows differ from the call on all rows; first: row %d"
                                       % (bad.size, bad[0]), g[bad[0]].tolist(), want[bad[0]].tolist())
