"""Position invariance of the per-Gaussian kernels, bit for bit, through the C ABI alone (``egs_fused_forward``;
``egs_fused_backward`` in phase 2 with the test's own gradient records).

k_preprocess_fwd keeps a row's SH coefficients in flight while it computes the row's geometry and waits for them with
counted waits; both kernels send rows through one LDS stage that serves several row widths in turn (and, on some
paths, row loads as well).  What can go wrong there is a wait in the wrong place or a staging hazard: a row then picks
up a neighbour's or a stale value.  Such a fault depends on WHERE the row sits in its wave and workgroup, not on its value, so the test is: the
same row gives the same bits wherever it sits.  No tolerance anywhere; the values themselves are held to their
float64 reference by tests/test_gpu_pergaussian_matrix.py.

Inputs: ONE seeded set of 515 rows on a 256 x 192 image (16 x 12 tiles), seven classes interleaved (row i is drawn for
class i % 7, so every wave holds several of each): visible with a tile rect of at most 4 x 4 (the block bitmap of the
footprint record), between 4 x 4 and 8 x 8 (the tile bitmap), beyond 8 x 8 (counted row by row), near-culled
(0 < z < 0.2), behind the camera, off-screen (empty rect) and opacity below the skip threshold.  The CPU test below
classifies the rows with the float64 reference of tests/pergaussian_ref.py and holds every class to at least 8 rows:
a condition on the inputs, not a measurement.

Arrangements: the rows in order, the rows reversed (a row moves to the mirrored lane, wave and workgroup: rows 0 .. 2
sit in the ragged last workgroup), and windows of 1, 65 and 257 rows starting at rows 0, 64 and 258 (a lone row; one
full wave and one lane of the next; one full workgroup and one row of the next).  515 rows are two full workgroups and
a last one of three rows.

Forward: depths, visible, the 48-byte record, dcolor/dpw, us, cinv2ds, colors and areas of a row, SH degree 3 and 1,
dcolor/dpw on and off, anti-aliased on and off, footprint-culled lists on (every branch of the footprint record
runs); once more with us / cinv2ds / colors / areas not requested.  The number of patches of the two full arrangements
must agree as well (the sum of the rows' tile counts: the count records in the workspace are not an output).
Backward: dL/dpw, dL/dsh, dL/dalpha, dL/dscale, dL/drot and dL/du of a row, plain, EGS_BWD_ACCUMULATE (the old
gradients move with their rows) and EGS_BWD_FACTORED_SH, with and without the forward's dcolor/dpw rows."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from easygaussiansplatting_amd import scene as S
from oracle import gs_oracle as O
from tests import pergaussian_ref as R
from tests.gpu_abi import DEV, Out, _check, _pol, _ptr, _stream
from tests.test_pose_grad_cpu import rodrigues

N, W, H = 515, 256, 192
SEED = 4107
CLASSES = ("rect <= 4x4", "rect <= 8x8", "rect > 8x8", "near-culled", "behind", "off-screen", "low opacity")
FUSED_CULLED_LISTS, FUSED_AA = 32, 256              # include/egs_hip.h EGS_FUSED_*
BWD_ACCUMULATE, BWD_FACTORED_SH = 64, 128
ARRANGEMENTS = (("in order", np.arange(N)), ("reversed", np.arange(N)[::-1].copy()), ("window 0+1", np.arange(0, 1)),
                ("window 64+65", np.arange(64, 129)), ("window 258+257", np.arange(258, 515)))


@functools.lru_cache(maxsize=None)
def camera():
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    Rm = f32(rodrigues([0.02, -0.04, 0.03]))
    t = f32([0.04, -0.06, 0.3])
    return S.Camera(W, H, 234.0, 245.0, 127.5, 95.5, Rm, t), f32(-Rm.T @ t)


@functools.lru_cache(maxsize=None)
def generate(K):
    """the 515 rows (float32, read-only): row i is drawn for class i % 7"""
    cam, _ = camera()
    u = lambda stream, shape=(N,): S.uniform01(SEED, stream, shape)
    cls = np.arange(N) % 7
    z = 2.0 + 4.0 * u(1)
    z = np.where(cls == 3, 0.02 + 0.17 * u(2), z)                  # near-culled
    z = np.where(cls == 4, -5.0 + 4.5 * u(2), z)                   # behind the camera
    px = W * (0.2 + 0.6 * u(3))                                    # pixel centre, well inside the image
    py = H * (0.2 + 0.6 * u(4))
    px = np.where(cls == 5, np.where(u(5) < 0.5, -150.0 - 100.0 * u(6), W + 150.0 + 100.0 * u(6)), px)
    # pixel radius 3 sigma: a few pixels; 34 .. 50 (5 .. 8 tiles across); 90 .. 150 (more than 8 tiles across)
    rad = 4.0 + 6.0 * u(7)
    rad = np.where(cls == 1, 34.0 + 16.0 * u(7), rad)
    rad = np.where(cls == 2, 90.0 + 60.0 * u(7), rad)
    pc = np.stack([(px - cam.cx) / cam.fx * z, (py - cam.cy) / cam.fy * z, z], 1)
    pws = (pc - cam.tcw) @ cam.Rcw
    s = (rad * np.abs(z) / (3.0 * cam.fx))[:, None] * (0.8 + 0.2 * u(8, (N, 3)))
    q = S.normal(SEED, 9, (N, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    a = np.where(cls == 6, 1e-4 + 1.3e-3 * u(10), 0.05 + 0.9 * u(10))
    sh = 0.3 * S.normal(SEED, 11, (N, K))
    sh[:, :3] += 0.8 * S.normal(SEED, 12, (N, 3))
    rec = S.normal(SEED, 13, (N, 12)) * 10.0 ** (-3.0 * u(14, (N, 1)))
    f = lambda x: np.ascontiguousarray(x, np.float32)
    d = dict(pws=f(pws), rots=f(q), scales=f(s), alphas=f(a), shs=f(sh), records=f(rec))
    for v in d.values():
        v.setflags(write=False)
    return d


def classify(inp):
    """class index of every row from the float64 reference: depth, tile rect (oracle.get_rects), opacity"""
    cam, twc = camera()
    st = R.stages(inp, False, cam, twc, np.float64)
    z = (np.asarray(inp["pws"], np.float64) @ cam.Rcw.T + cam.tcw)[:, 2]      # (the stages zero the rows they cull)
    rects, counts = O.get_rects(st["us"], st["areas"].copy(), st["depths"].copy(), W, H, R.POLICY)
    w = rects[:, 2].astype(np.int64) - rects[:, 0]
    h = rects[:, 3].astype(np.int64) - rects[:, 1]
    cls = np.full(len(z), -1)
    seen = z >= O.MIN_DEPTH
    cls[z < 0] = 4
    cls[(z > 0) & (z < O.MIN_DEPTH)] = 3
    cls[seen & (counts == 0)] = 5
    on = seen & (counts != 0)
    low = np.asarray(inp["alphas"], np.float64) < R.POLICY.alpha_skip
    cls[on & low] = 6
    cls[on & ~low & (w <= 4) & (h <= 4)] = 0
    cls[on & ~low & ~((w <= 4) & (h <= 4)) & (w <= 8) & (h <= 8)] = 1
    cls[on & ~low & ((w > 8) | (h > 8))] = 2
    return cls


def test_every_class_has_rows():
    """the condition on the inputs: at least 8 rows of every class, several of each in every wave"""
    for K in (48, 12):
        cls = classify(generate(K))
        assert (cls >= 0).all()
        counts = np.bincount(cls, minlength=7)
        print("K = %d: " % K + ", ".join("%s %d" % (nm, c) for nm, c in zip(CLASSES, counts)))
        assert (counts >= 8).all(), dict(zip(CLASSES, counts))
        for w0 in range(0, N - 63, 64):            # every full wave of the in-order arrangement
            assert (np.bincount(cls[w0:w0 + 64], minlength=7) >= 2).all(), (K, w0)


# -------------------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from easygaussiansplatting_amd import _lib, gsplatcu
    gsplatcu.set_policy("gsplatcu")
    yield _lib.load()
    gsplatcu.set_policy("gsplatcu")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _camera_dev():
    cam, twc = camera()
    f = lambda a: _dev(np.asarray(a, np.float32))
    return f(cam.Rcw), f(cam.tcw), f(twc)


def run_forward(lib, K, idx, jw, aa, seven=True):
    """one egs_fused_forward call on rows ``idx`` of the set -> {name: int32 words [len(idx), width]}, patches"""
    inp = generate(K)
    n = len(idx)
    pws, rots, scales, shs, alphas = (_dev(inp[k][idx]) for k in ("pws", "rots", "scales", "shs", "alphas"))
    Rcw, tcw, twc = _camera_dev()
    cam, _ = camera()
    outs = dict(depths=Out(n), rec=Out(12 * n))
    if jw:
        outs["dcolor_dpws"] = Out(9 * n)
    if seven:
        outs.update(us=Out(2 * n), cinv2ds=Out(3 * n), colors=Out(3 * n), areas=Out(2 * n))
    p = lambda k: outs[k].ptr if k in outs else None
    vis = torch.full((n + 512,), 0xA5, dtype=torch.uint8, device=DEV)
    ws_bin = torch.empty(lib.egs_splat_bin_ws_bytes(n), dtype=torch.uint8, device=DEV)
    total = torch.zeros(2, dtype=torch.int32, device=DEV)
    flags = FUSED_CULLED_LISTS | (FUSED_AA if aa else 0)
    _check(lib, lib.egs_fused_forward(
        n, K, _ptr(pws), _ptr(rots), _ptr(scales), _ptr(shs), None, _ptr(alphas), _ptr(Rcw), _ptr(tcw), _ptr(twc), cam.fx,
        cam.fy, cam.cx, cam.cy, W, H, C.byref(_pol()), p("us"), p("depths"), p("cinv2ds"), p("colors"), p("areas"),
        p("rec"), C.c_void_p(vis.data_ptr() + 256), p("dcolor_dpws"), flags, 0, _ptr(ws_bin), ws_bin.numel(), _ptr(total),
        None, _stream()))
    torch.cuda.synchronize()
    what = ("forward", K, n, jw, aa)
    got = {k: o.read(what + (k,)).reshape(n, -1) for k, o in outs.items()}
    v = vis.cpu().numpy()
    assert (v[:256] == 0xA5).all() and (v[256 + n:] == 0xA5).all(), (what, "visible written outside its rows")
    got["visible"] = v[256:256 + n].astype(np.int32).reshape(n, 1)
    return got, int(total[0].item())


def _same_rows(what, base, got, idx):
    for k, g in got.items():
        want = base[k][idx]
        bad = np.nonzero((g != want).any(1))[0]
        assert bad.size == 0, (what, k, "%d rows differ from the in-order call; first: row %d of the call = row %d of "
                               "the set" % (bad.size, bad[0], idx[bad[0]]), g[bad[0]].tolist(), want[bad[0]].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("aa", [False, True], ids=["plain", "aa"])
@pytest.mark.parametrize("jw", [False, True], ids=["nojw", "jw"])
@pytest.mark.parametrize("K", [48, 12])
def test_forward_rows_do_not_depend_on_their_position(lib, K, jw, aa):
    variants = [True] + ([False] if (K == 48 and jw and not aa) else [])      # the training step requests no seven-op rows
    for seven in variants:
        base, patches = run_forward(lib, K, ARRANGEMENTS[0][1], jw, aa, seven)
        live = base["depths"].view(np.float32)[:, 0] > 0
        assert live.sum() > 3 * 8 and (~live).sum() > 3 * 8
        for name, idx in ARRANGEMENTS[1:]:
            got, p = run_forward(lib, K, idx, jw, aa, seven)
            _same_rows((K, jw, aa, seven, name), base, got, idx)
            if len(idx) == N:
                assert p == patches, (K, jw, aa, name, "patch totals differ", p, patches)


@functools.lru_cache(maxsize=None)
def _forward_state(lib, K):
    """depths, record and dcolor/dpw rows of the in-order forward call: what the backward calls read"""
    return run_forward(lib, K, ARRANGEMENTS[0][1], True, False, False)[0]


def _widths(K, factored):
    return dict(dpws=3, dalphas=1, dscales=3, drots=4, dus=2, dshs=3 if factored else K)


def run_backward(lib, K, idx, jw, mode):
    """one phase-2 egs_fused_backward call on rows ``idx`` -> {name: int32 words [len(idx), width]}"""
    inp, fw = generate(K), _forward_state(lib, K)
    n = len(idx)
    pws, rots, scales, shs, alphas, records = (_dev(inp[k][idx]) for k in ("pws", "rots", "scales", "shs", "alphas",
                                                                           "records"))
    depths, rec, dcw = (_dev(fw[k][idx]) for k in ("depths", "rec", "dcolor_dpws"))
    Rcw, tcw, twc = _camera_dev()
    cam, _ = camera()
    factored = mode == "factored"
    outs = {}
    for j, (name, w) in enumerate(sorted(_widths(K, factored).items())):
        old = None
        if mode == "accumulate" and name != "dus":      # the old gradients move with their rows
            old = (0.1 * S.normal(SEED, 50 + j, (N, w))).astype(np.float32)[idx]
        outs[name] = Out(n * w + (3 if (factored and name == "dshs") else 0), old)
    ws = torch.empty(lib.egs_fused_backward_ws_bytes(n), dtype=torch.uint8, device=DEV)
    flags = {"plain": 0, "accumulate": BWD_ACCUMULATE, "factored": BWD_FACTORED_SH}[mode]
    g = lambda k: outs[k].ptr
    _check(lib, lib.egs_fused_backward(
        n, K, 0, W, H, _ptr(pws), _ptr(rots), _ptr(scales), _ptr(shs), None, _ptr(alphas), _ptr(Rcw), _ptr(tcw), _ptr(twc),
        cam.fx, cam.fy, cam.cx, cam.cy, C.byref(_pol()), None, None, None, None, _ptr(rec), _ptr(depths), None, None, None,
        None, None, _ptr(ws), ws.numel(), g("dpws"), g("dshs"), None, g("dalphas"), g("dscales"), g("drots"), g("dus"),
        None, _ptr(records), _ptr(dcw) if jw else None, 2 | flags, 0, n, None, 0, _stream(), None, None))
    torch.cuda.synchronize()
    what = ("backward", K, n, jw, mode)
    return {k: outs[k].read(what + (k,))[:n * w].reshape(n, w) for k, w in _widths(K, factored).items()}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["plain", "accumulate", "factored"])
@pytest.mark.parametrize("K", [48, 12])
def test_backward_rows_do_not_depend_on_their_position(lib, K, mode):
    for jw in (True, False):
        base = run_backward(lib, K, ARRANGEMENTS[0][1], jw, mode)
        assert base["dshs"].view(np.float32).any() and base["drots"].view(np.float32).any()
        for name, idx in ARRANGEMENTS[1:]:
            _same_rows((K, jw, mode, name), base, run_backward(lib, K, idx, jw, mode), idx)
