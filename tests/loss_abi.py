"""Helpers of the GPU tests of the fused loss (tests/test_gpu_loss.py, tests/test_gpu_weighted_loss.py) that call the C
ABI directly: device buffers the test owns, NaN-filled between guard bands that must be intact afterwards, and
``egs_gau_loss`` called on them."""
import ctypes as C

import numpy as np
import torch

GUARD = 256          # bytes on each side of a buffer the kernels write
PATTERN = 0xA5
EGS_ERR_WORKSPACE = 10002    # include/egs_hip.h


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def bits(t):
    return t.contiguous().view(torch.int32)


def nb_of(H, W):
    return ((W + 63) // 64) * ((H + 15) // 16) * 3


def guarded(nbytes):
    """A buffer of ``nbytes`` between two guard bands.  -> (whole uint8 tensor, the inner bytes as a view)."""
    whole = torch.full((nbytes + 2 * GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
    return whole, whole[GUARD:GUARD + nbytes]


def guards_intact(whole):
    return bool((whole[:GUARD] == PATTERN).all()) and bool((whole[-GUARD:] == PATTERN).all())


def abi_loss(lib, x, y, lam=0.2, scale=1.0, ws_short=0):
    """egs_gau_loss on buffers this test owns: workspace, gradient and stats NaN-filled between guard bands.
    -> (rc, grad [3,H,W], stats [3]); asserts the guards."""
    H, W = int(x.shape[1]), int(x.shape[2])
    ws_bytes = int(lib.egs_gau_loss_ws_bytes(H, W))
    assert ws_bytes % 4 == 0 and ws_bytes >= 3 * 12 * H * W + 8 * nb_of(H, W)
    ws_all, ws = guarded(ws_bytes)
    g_all, g = guarded(12 * H * W)
    s_all, s = guarded(12)
    for inner in (ws, g, s):
        inner.view(torch.float32).fill_(float("nan"))
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = lib.egs_gau_loss(H, W, p(x), p(y), float(lam), float(scale), p(ws), ws_bytes - ws_short, p(s), p(g),
                          C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    for whole, nm in ((ws_all, "workspace"), (g_all, "dloss_dimage"), (s_all, "loss_out")):
        assert guards_intact(whole), "%dx%d: the kernels wrote outside %s" % (H, W, nm)
    return rc, g.view(torch.float32).reshape(3, H, W).clone(), s.view(torch.float32).clone()
