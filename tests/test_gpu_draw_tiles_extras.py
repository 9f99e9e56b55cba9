"""The EXTRA instances of k_draw / k_draw_bwd (render extras: depth and opacity maps, a background;
csrc/egs_draw.hip, blend_range<.., EXTRA> of csrc/egs_draw_device.h) and the unsplit ABS instance of k_draw_bwd, on the
HAND-BUILT one-tile lists of tests/draw_tile_ref.py (``case(name, extras=True)``), through the raw C ABI: sentinel-banded
``tests/gpu_abi.Out`` buffers, ``_lib.EgsExtras``, and the backward draw pass ALONE -- ``egs_fused_backward`` with phase 1
returns behind splatB's draw pass with the packed [N][12] gradient records (0 dalpha, 1-3 dcolor, 4-5 du, 6-8 dcinv, 9 dz,
10-11 absgrad) in the caller's zeroed ``grad_records``; its 3D tensors are only null-checked there and are dummies here.

Paths (every test asserts from the profiler labels which instances ran: ``k_draw_extra`` and no ``k_draw``,
``k_draw_bwd_extra`` / ``k_draw_bwd_abs`` and no ``k_draw_bwd``):
  masked       gsplatcu; egs_splat_bin_pack (records and binning in one pass); egs_splat_draw_rec_seg with
               EGS_DRAW_MASKED_LISTS; the backward phase carries EGS_FUSED_CULLED_LISTS: non-BOX instances, block masks in
               the list values, z in the third float of sC
  plain        gsplatcu; egs_pack_records + egs_splat_bin; flags 0: the same instances with the per-entry box test
  forward_cpu  forward_cpu; egs_pack_records with ``areas`` + egs_splat_bin: the BOX instances, z in sZ in the forward

Asserted per set and path, no pixel and no row excluded:
  * ``ranges`` and the list (with the masks stripped on ``masked``) equal the intended ones, ``contrib`` the reference on
    every pixel;
  * image, final_tau, depth_out, alpha_out per pixel: |got - ref| <= max(floor, 2 x distance) (``D.pixel_floor`` /
    ``D.distances`` with extras: (a), (b) the float32 composition of the oracle on the inputs and one ulp away, z
    included, (c) the float32 blend in k_draw's own operations: polynomial exponent, cd += w z with two roundings and
    contracted, alpha = 1 - tau, fmaf(tau, bg, c));
  * empty tiles: image == float32(bg) exactly; depth, alpha, contrib, final_tau 0;
  * every output (image, contrib, final_tau, depth_out, alpha_out, ranges, lists, records) keeps the 2048 sentinel
    words in front of and behind it: the ragged right column and bottom row put lanes outside the image;
  * record slots 0-9 per Gaussian row by the rule and FLOOR of tests/test_gpu_draw_tiles.py (dz a one-column tensor)
    against the float64 reference of <Wi, image> + <Wd, depth> + <Wa, alpha>; rows with a zero reference are zero bit for
    bit; slots 10-11 are zero bit for bit; the backward fed the device's own contrib / final_tau and the backward fed the
    oracle's (rounded to float32, the oracle's lists) are held to the same bound; two runs give bitwise equal records;
  * nullable fields: depth_out / alpha_out NULL (each and both) leave image, contrib, final_tau bitwise; dloss_ddepth /
    dloss_dalpha NULL give the records of zero arrays bitwise, and without dL/ddepth slot 9 is zero bit for bit;
  * EXTRA against plain: with background 0 the EXTRA forward's image, contrib, final_tau equal the plain instances'
    from the same records as floats; with Wd = Wa = 0 and background 0 the EXTRA records' slots 0-8 meet the PLAIN
    reference's bound (not bitwise: NQ differs, so the reduction tree does);
  * nothing to draw (n > 0 with every Gaussian culled, and n == 0: the hipMemsetD32Async branch of splat_draw_impl):
    image == float32(bg) on every pixel, depth, alpha, contrib, final_tau, ranges 0;
  * refused arguments: a segment workspace with extras, and EGS_BWD_ABSGRAD with extras, return EGS_ERR_BAD_ARG and
    write nothing;
  * the unsplit ABS instance (``k_draw_bwd_abs``: phase 1 with EGS_BWD_ABSGRAD, no extras) on the three paths: slots
    10-11 against tests/absgrad_ref.draw_backward_abs (float64) by the same row rule (distance: the |t| sums of the
    float32 walks of ``D.distances``), slots 0-8 against the plain reference, slot 9 zero bit for bit.  The segment-walk
    ABS instances (k_draw_bwd_seg_abs) stay with tests/test_gpu_absgrad.py.

No tolerance here is fitted to a kernel's output: every bound is a floor counted from the roundings, or twice a distance
evaluated on the reference alone.  Nothing had to be added to the distances for the EXTRA code after the first run:
cd += w z (both roundings and contracted), 1 - tau and fmaf(tau, bg, c) are parts of ``D.blend``, fmaf(dL/ddepth, z, ..)
and the lq that starts at Wi . bg - Wa are parts of ``D.backward_hw``.  No defect was found; csrc is unchanged.

Each test prints, per tensor, the largest distance | the largest kernel error | the largest error / bound.
Measured on MI355X, largest over the five sets and three paths (58 tests pass, 0 pixels and 0 rows excluded):
                      distance   kernel error   error / bound
  image               9.0e-06    9.0e-06        0.83
  final_tau           9.3e-06    8.6e-06        0.74
  depth               0.00038    0.00034        0.74
  alpha               9.3e-06    8.6e-06        0.79
  dus                 0.00097    0.00013        0.52      backward alone  8.6e-05  0.42
  dcinv2ds            0.0001     5.4e-05        0.42      backward alone  3.4e-05  0.39
  dalphas             0.052      0.0013         0.64      backward alone  0.0014   0.44
  dcolors             0.00016    5.6e-05        0.49      backward alone  1.1e-05  0.28
  dz                  0.0092     0.0026         0.63      backward alone  0.0014   0.50
  EXTRA records with Wd = Wa = 0, background 0, against the PLAIN reference and distances:
  dus 0.52, dcinv2ds 0.46, dalphas 0.61, dcolors 0.49 of their bounds (the plain instances stand at 0.56 / 0.46 / 0.61 /
  0.49, tests/test_gpu_draw_tiles.py); the EXTRA forward over background 0 equalled the plain forward on every value.
  ABS instance, unsplit:  dus_abs  distance 0.00011, kernel error 3.5e-05, 0.38 of its bound; slots 0-8 as the plain rows.
(the large distances and errors belong to single cancelling rows, as in tests/test_gpu_draw_tiles.py.)  The largest
depth error, 3.4e-4 at z up to 100 (set values), is 0.74 of the distance of the float32 restatement.  contrib and both
lists were exact on every path; two runs of every path were bitwise equal.
Wall time on MI355X: the module 29 s (58 tests), of which the CPU reference (``D.reference`` / ``D.distances`` with and
without extras, cached per set and policy) is 15 s; the slowest test 2.7 s (lengths1 / masked, its reference included),
a test whose reference is cached takes less than 5 ms (38 of the 58).

Seeded errors (scratch builds of csrc; the three value-only ones -- no index, offset or count changes -- were each run
once against ``test_extras_one_tile_lists``, and each failed all 15 of its cases):
  blend_range   ``cd[k] += w * zj`` with the z of the PREVIOUS entry of the group of eight (``sC[jp].z`` / ``sZ[jp]``, jp =
                (j & ~7) | ((j - 1) & 7), inside the 64 staged slots).  First: [lengths0-masked] "depth", pixel (y 8, x 25)
                of tile 1 (contrib 2): error 0.634 against a bound of 1.7e-5; [stops-plain] pixel (y 0, x 48) of tile 3:
                error 59.6.
  k_draw_bwd    ``acc[e][NQ - 1] += la[k] * wgt`` (dL/dalpha for dL/ddepth in the dz partial).  First: [lengths0-masked]
                "own forward" "dz", 807 rows, worst Gaussian 783 = tile 5, entry 4 of 5: error 39.3, bound 1.06e-5;
                [stops-plain] 722 rows, worst tile 1, entry 37 of 130: error 81.4.
  k_draw_bwd    the background term dropped from the start of lq (``lq[k] = -la[k]``).  First: [lengths0-masked] "own
                forward" "dus", 807 rows, worst Gaussian 53 = tile 10, entry 57 of 65: error 7.53, bound 1.04e-5;
                [stops-plain] 440 rows, worst tile 0, entry 127 of 130: error 5.26.
NOT run, reasoned -- both decide WHERE a total lands, and a wrong slot can leave the 12-float record:
  ``qoff = 9``  lanes c16 == 3 add the dz total at gpack + 12 g + qoff.  10 or 11 stay inside the record: "dz" rows at
                error 1 (a zero where the reference is not) and "slots 10:12 are not zero bit for bit" in every case of
                ``test_extras_one_tile_lists``; 12 and above are the NEXT Gaussian's dalpha .. and, for the last
                Gaussian, memory behind the records (the sentinel band here, anything elsewhere).
  NQ = 10 tree  ``odd_lanes_tail``: s8 and s9 swapped in ``merge2<M2>(s8, s9, h2)`` trades the lanes of M2yy and dz --
                "dcinv2ds" and "dz" rows fail in every case; ``s9 += dpp_get<M4>(s9)`` dropped loses the partials of half of
                each row's lanes -- "dz" rows of every entry that hits more than a quarter of its tile.  Value-only as
                they stand, but one edit away from the lane -> slot table above, so they were left alone.
"""
import collections
import contextlib
import ctypes as C
import time

import numpy as np
import pytest
import torch

from tests import draw_tile_ref as D
from tests.gpu_abi import Out, _check, _ptr, _stream

pytestmark = pytest.mark.gpu

DEV = "cuda"
FLOOR = 1e-5                                        # tests/test_gpu_draw_tiles.py
MASKED_LISTS = 2                                    # include/egs_hip.h EGS_DRAW_MASKED_LISTS
CULLED_LISTS = 32                                   # EGS_FUSED_CULLED_LISTS
ABSGRAD = 1024                                      # EGS_BWD_ABSGRAD
BAD_ARG = 10001                                     # EGS_ERR_BAD_ARG
GSID_MASK = 0x0FFFFFFF
HW = D.H * D.W
PATHS = {"masked": dict(policy="gsplatcu", masked=True), "plain": dict(policy="gsplatcu", masked=False),
         "forward_cpu": dict(policy="forward_cpu", masked=False)}
SLOTS = dict(dalphas=slice(0, 1), dcolors=slice(1, 4), dus=slice(4, 6), dcinv2ds=slice(6, 9), dz=slice(9, 10),
             dus_abs=slice(10, 12))
ZERO_BG = (0.0, 0.0, 0.0)


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from easygaussiansplatting_amd import _lib
    return _lib.load()


def _policy(lib, name):
    from easygaussiansplatting_amd._lib import EgsPolicy
    p = EgsPolicy()
    (lib.egs_policy_gsplatcu if name == "gsplatcu" else lib.egs_policy_forward_cpu)(C.byref(p))
    return p


@contextlib.contextmanager
def labels(lib):
    """-> a set that holds, after the block, the profiler labels of the kernels launched in it"""
    got = set()
    lib.egs_prof_set_filter(None); lib.egs_prof_reset(); lib.egs_prof_enable(1)
    try:
        yield got
    finally:
        torch.cuda.synchronize()
        lib.egs_prof_enable(0)
        need = lib.egs_prof_report(None, 0)
        buf = C.create_string_buffer(need + 16)
        lib.egs_prof_report(buf, need + 16)
        got.update(ln.split()[0] for ln in buf.value.decode().splitlines() if ln.strip())
        lib.egs_prof_reset()


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)         # (a copy: the case's arrays are read-only)


class Inputs:
    """an extras case on the device (read-only: areas and depths go to every call as fresh sentinel-banded copies)"""

    def __init__(self, c):
        self.c, self.n = c, c.n
        a = c.arrays
        self.us, self.cinv, self.alphas, self.colors, self.z = (_dev(a[k]) for k in ("us", "cinv2ds", "alphas", "colors", "z"))
        self.Wi, self.Wd, self.Wa = (_dev(a[k]) for k in ("dloss_dgammas", "dloss_ddepth", "dloss_dalpha"))
        self.areas_h, self.depths_h = a["areas"], a["depths"]
        self.zeros = torch.zeros((D.H, D.W), dtype=torch.float32, device=DEV)
        # the 3D side of egs_fused_backward: null-checked only in phase 1
        self.dummy = torch.zeros(64, dtype=torch.float32, device=DEV)
        self.sink = torch.zeros(64, dtype=torch.float32, device=DEV)


_inputs = {}


def inputs(name):
    if name not in _inputs:
        _inputs[name] = Inputs(D.case(name, extras=True))
    return _inputs[name]


def _extras(inp, bg, depth_out=None, alpha_out=None, Wd=None, Wa=None):
    from easygaussiansplatting_amd._lib import EgsExtras
    ex = EgsExtras()
    ex.depths = inp.z.data_ptr() if inp.n else None
    ex.depth_out = depth_out.ptr.value if depth_out is not None else None
    ex.alpha_out = alpha_out.ptr.value if alpha_out is not None else None
    ex.background = (C.c_float * 3)(*[float(v) for v in bg])
    ex.dloss_ddepth = Wd.data_ptr() if Wd is not None else None
    ex.dloss_dalpha = Wa.data_ptr() if Wa is not None else None
    return ex


def forward(lib, inp, path, bg, depth=True, alpha=True, depths_h=None, seg_ws=None):
    """binning + draw of ``path``; ``bg`` None: the plain instances -> dict of host arrays (every band checked), the
    device buffers the backward pass takes (``dev``), P and the draw call's return code"""
    n, opt, st = inp.n, PATHS[path], _stream()
    pol = _policy(lib, opt["policy"])
    areas = Out(2 * max(n, 1), inp.areas_h if n else None)
    depths = Out(max(n, 1), (inp.depths_h if depths_h is None else depths_h) if n else None)
    total = Out(2)
    ws_bin = torch.empty(lib.egs_splat_bin_ws_bytes(n), dtype=torch.uint8, device=DEV)
    rec = torch.zeros((max(n, 1), 12), dtype=torch.float32, device=DEV)
    P = 0
    if n:
        us, cinv, alphas, colors = _ptr(inp.us), _ptr(inp.cinv), _ptr(inp.alphas), _ptr(inp.colors)
        if opt["masked"]:
            _check(lib, lib.egs_splat_bin_pack(n, D.W, D.H, us, cinv, alphas, colors, areas.ptr, depths.ptr, C.byref(pol), 0,
                                               _ptr(ws_bin), ws_bin.numel(), total.ptr, None, _ptr(rec), None, None, st))
        else:
            _check(lib, lib.egs_pack_records(n, D.W, D.H, us, cinv, alphas, colors,
                                             areas.ptr if opt["policy"] == "forward_cpu" else None, C.byref(pol), _ptr(rec),
                                             st))
            _check(lib, lib.egs_splat_bin(n, D.W, D.H, us, areas.ptr, depths.ptr, C.byref(pol), 0, _ptr(ws_bin),
                                          ws_bin.numel(), total.ptr, st))
        torch.cuda.synchronize()
        P = int(total.read("total_patches").view(np.uint32)[0])
    assert 0 <= P <= max(n, 1), P                        # (one patch per Gaussian at the most: the buffers below)
    image, contrib, tau, dout, aout = Out(3 * HW), Out(HW), Out(HW), Out(HW), Out(HW)
    ranges, walk = Out(2 * D.T), Out(max(P, 1))
    plain = Out(max(P, 1)) if opt["masked"] else None
    ws_draw = torch.empty(lib.egs_splat_draw_ws_bytes(n, P, D.W, D.H), dtype=torch.uint8, device=DEV)
    ex = None if bg is None else _extras(inp, bg, dout if depth else None, aout if alpha else None)
    rc = lib.egs_splat_draw_rec_seg(n, P, None, D.W, D.H, _ptr(rec) if n else None, C.byref(pol), _ptr(ws_bin), _ptr(ws_draw),
                                    ws_draw.numel(), image.ptr, contrib.ptr, tau.ptr, ranges.ptr, walk.ptr, None, None,
                                    None, 0, MASKED_LISTS if opt["masked"] else 0, _ptr(seg_ws),
                                    seg_ws.numel() if seg_ws is not None else 0, None, None,
                                    plain.ptr if plain is not None else None, st, C.byref(ex) if ex is not None else None)
    torch.cuda.synchronize()
    f32 = lambda o, what: o.read(what).view(np.float32).copy()
    out = dict(rc=rc, P=P, image=f32(image, "image").reshape(3, D.H, D.W), contrib=contrib.read("contrib").reshape(D.H, D.W).copy(),
               final_tau=f32(tau, "final_tau").reshape(D.H, D.W), depth=f32(dout, "depth_out").reshape(D.H, D.W),
               alpha=f32(aout, "alpha_out").reshape(D.H, D.W), ranges=ranges.read("ranges").reshape(D.T, 2).copy(),
               walk=walk.read("list").copy()[:P], plain=plain.read("plain list").copy()[:P] if plain is not None else None,
               untouched={k: np.array_equal(o.read(k), o.old()) for k, o in (("image", image), ("depth", dout), ("alpha", aout))},
               dev=dict(rec=rec, contrib=contrib, tau=tau, ranges=ranges, walk=walk, keep=(ws_bin, ws_draw)))
    return out


def backward(lib, inp, path, rec, P, contrib, tau, ranges, walk, ex=None, absgrad=False):
    """the backward draw pass alone (phase 1) -> (return code, the records [N, 12], whether they were left untouched);
    ``contrib`` .. ``walk``: pointers; ``ex``: dict(bg, Wd, Wa) for the EXTRA instance or None"""
    n, opt, st = inp.n, PATHS[path], _stream()
    pol = _policy(lib, opt["policy"])
    records = Out(12 * n, np.zeros(12 * n, np.float32))
    ws = torch.empty(lib.egs_fused_backward_ws_bytes(n), dtype=torch.uint8, device=DEV)
    x = None if ex is None else _extras(inp, ex["bg"], Wd=ex["Wd"], Wa=ex["Wa"])
    d, s = _ptr(inp.dummy), _ptr(inp.sink)
    phase = 1 | (CULLED_LISTS if opt["masked"] else 0) | (ABSGRAD if absgrad else 0)
    rc = lib.egs_fused_backward(n, 3, P, D.W, D.H, d, d, d, d, None, d, d, d, d, 1.0, 1.0, 0.0, 0.0, C.byref(pol),
                                None, None, None, None, _ptr(rec), d, contrib, tau, ranges, walk, _ptr(inp.Wi), _ptr(ws),
                                ws.numel(), s, s, None, s, s, s, s, None, records.ptr, None, phase, 0, 0, None, 0, st,
                                C.byref(x) if x is not None else None, None)
    torch.cuda.synchronize()
    got = records.read("gradient records")
    return rc, got.view(np.float32).reshape(n, 12).copy(), not got.any()


def own_backward(lib, inp, path, f, **kw):
    d = f["dev"]
    rc, rec, _ = backward(lib, inp, path, d["rec"], f["P"], d["contrib"].ptr, d["tau"].ptr, d["ranges"].ptr, d["walk"].ptr, **kw)
    _check(lib, rc)
    return rec


def _bits(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.int32)


# ------------------------------------------------------------------------------------------------------------- checks
def check_lists(name, path, pname, f):
    c = D.case(name)
    ls, rg, gs = D.lists(c, pname)
    assert f["P"] == len(gs), (name, path, "total_patches", f["P"], len(gs))
    assert np.array_equal(f["ranges"], rg), (name, path, "ranges are not the intended ones")
    if PATHS[path]["masked"]:
        assert np.array_equal(f["plain"], gs), (name, path, "the plain list is not the intended one")
        assert np.array_equal((f["walk"].view(np.uint32) & GSID_MASK).astype(np.int32), gs), (name, path, "masked & 0x0FFFFFFF")
    else:
        assert np.array_equal(f["walk"], gs), (name, path, "the list is not the intended one")
    return ls


def check_contrib(name, path, f, ref):
    wrong = np.argwhere(f["contrib"] != ref["contrib"])
    assert wrong.size == 0, (name, path, "contrib differs on %d pixels, first (y, x) %s: got %d, reference %d" % (
        len(wrong), wrong[0], f["contrib"][tuple(wrong[0])], ref["contrib"][tuple(wrong[0])]))


def check_pixels(name, path, pname, f, stats, keys=("image", "final_tau", "depth", "alpha")):
    ref, dist = D.reference(name, pname, extras=True), D.distances(name, pname, extras=True)
    floor = D.pixel_floor(name, pname, extras=True)
    for key in keys:
        got, want = f[key], ref[key]
        assert np.isfinite(got).all(), (name, path, key)
        err = np.abs(got.astype(np.float64) - want)
        err = err.max(0) if err.ndim == 3 else err
        bound = np.maximum(floor[key], 2 * dist[key])
        ratio = err / bound
        stats[key] = (float(dist[key].max()), float(err.max()), float(ratio.max()))
        y, x = np.unravel_index(np.argmax(ratio), ratio.shape)
        assert ratio.max() <= 1, (name, path, key, "pixel (y %d, x %d) of tile %d: error %.3g, bound %.3g (distance %.3g), "
                                  "contrib %d" % (y, x, (y // 16) * D.GX + x // 16, err[y, x], bound[y, x], dist[key][y, x],
                                                  f["contrib"][y, x]))


def check_empty_tiles(name, path, f, ls, bg):
    seen = 0
    for t, l in enumerate(ls):
        if len(l) == 0:
            seen += 1
            tx, ty, x0, y0, ww, hh = D.geom(t)
            win = (slice(y0, y0 + hh), slice(x0, x0 + ww))
            for ch in range(3):
                assert (f["image"][ch][win] == np.float32(bg[ch])).all(), (name, path, "empty tile %d: image is not the background" % t)
            for k in ("depth", "alpha", "contrib", "final_tau"):
                assert not _bits(f[k][win]).any() if f[k].dtype == np.float32 else not f[k][win].any(), (name, path, t, k)
    return seen


def check_rows(name, path, label, rec, ref, dist, keys, stats, c):
    """the row rule of tests/test_gpu_draw_tiles.py on the slots of ``keys``"""
    floor = FLOOR * np.maximum(1.0, ref["walked"] / 100.0)
    for key in keys:
        want = np.asarray(ref[key], np.float64).reshape(c.n, -1)
        got = rec[:, SLOTS[key]]
        assert got.shape == want.shape and np.isfinite(got).all(), (name, path, label, key)
        zero = ~want.any(1)
        nz = np.nonzero(_bits(got).reshape(c.n, -1)[zero].any(1))[0]
        assert nz.size == 0, (name, path, label, key, "%d rows with a zero reference are not zero bit for bit, first: Gaussian "
                              "%d (tile %d, entry %d)" % (nz.size, np.nonzero(zero)[0][nz[0]], c.tile_of[np.nonzero(zero)[0][nz[0]]],
                                                          c.pos_of[np.nonzero(zero)[0][nz[0]]]))
        rel = D._rows(got, want)
        bound = np.maximum(floor, 2 * dist[key])
        ratio = rel / bound
        g = int(np.argmax(ratio))
        old = stats.get(key, (0.0, 0.0, 0.0))
        stats[key] = (float(dist[key].max()), max(old[1], float(rel.max())), max(old[2], float(ratio.max())))
        assert ratio.max() <= 1, (name, path, label, key, "%d rows beyond their bound; worst: Gaussian %d = tile %d, entry %d of "
                                  "%d of the policy-G list (walked %d): error %.3g, bound %.3g (distance %.3g)" % (
                                      int((ratio > 1).sum()), g, c.tile_of[g], c.pos_of[g], len(c.lists[c.tile_of[g]]),
                                      ref["walked"][g], rel[g], bound[g], dist[key][g]), got[g].tolist(), want[g].tolist())


def zero_slots(name, path, label, rec, *slots):
    for s in slots:
        nz = np.argwhere(_bits(rec[:, s]).reshape(len(rec), -1))
        assert nz.size == 0, (name, path, label, "slots %s are not zero bit for bit: %d words, first in row %d" % (s, len(nz), nz[0][0]))


def _report(name, path, stats, t_ref, t_all):
    print("\nextras %s / %s  per tensor: largest float32 distance | largest kernel error | largest error / bound  "
          "(reference %.2f s of %.2f s)" % (name, path, t_ref, t_all))
    for k, v in stats.items():
        print("  %-22s %.3g | %.3g | %.3g" % ((k,) + v))


def _steps():
    failed = []

    def step(f, *args):     # every comparison runs and reports, the first failure is raised at the end
        try:
            return f(*args)
        except AssertionError as e:
            failed.append(e)
    return step, failed


# -------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", D.SETS)
def test_extras_one_tile_lists(lib, name, path):
    t0 = time.perf_counter()
    pname = PATHS[path]["policy"]
    c = D.case(name, extras=True)
    ref, dist = D.reference(name, pname, extras=True), D.distances(name, pname, extras=True)
    D.pixel_floor(name, pname, extras=True)
    t_ref = time.perf_counter() - t0
    inp = inputs(name)
    with labels(lib) as ran:
        f = forward(lib, inp, path, c.bg)
    _check(lib, f["rc"])
    assert "k_draw_extra" in ran and "k_draw" not in ran, (name, path, sorted(ran))
    ls = check_lists(name, path, pname, f)
    check_contrib(name, path, f, ref)
    stats = collections.OrderedDict()
    step, failed = _steps()
    step(check_pixels, name, path, pname, f, stats)
    step(check_empty_tiles, name, path, f, ls, c.bg)
    ex = dict(bg=c.bg, Wd=inp.Wd, Wa=inp.Wa)
    with labels(lib) as ranb:
        rec = own_backward(lib, inp, path, f, ex=ex)
    assert "k_draw_bwd_extra" in ranb and not {"k_draw_bwd", "k_draw_bwd_abs"} & ranb, (name, path, sorted(ranb))
    print("\nextras %s / %s ran %s and %s" % (name, path, sorted(ran), sorted(ranb)))
    again = own_backward(lib, inp, path, f, ex=ex)
    step(check_rows, name, path, "own forward", rec, ref, dist, D.GRADS_X, stats, c)
    step(zero_slots, name, path, "own forward", rec, SLOTS["dus_abs"])
    # the backward pass alone: the oracle's contrib / final_tau (rounded to float32) and lists (on ``masked`` the device's
    # own list, which IS the oracle's under its masks: check_lists)
    _, rg, gs = D.lists(c, pname)
    o_cont, o_tau, o_rg = _dev(ref["contrib"]), _dev(ref["final_tau"].astype(np.float32)), _dev(rg)
    o_gs = _dev(gs)                                   # (held until the pass has run: the call takes a raw pointer)
    o_list = f["dev"]["walk"].ptr if PATHS[path]["masked"] else _ptr(o_gs)
    rc, alone, _ = backward(lib, inp, path, f["dev"]["rec"], len(gs), _ptr(o_cont), _ptr(o_tau), _ptr(o_rg), o_list, ex=ex)
    _check(lib, rc)
    sa = collections.OrderedDict()
    step(check_rows, name, path, "backward alone", alone, ref, dist, D.GRADS_X, sa, c)
    step(zero_slots, name, path, "backward alone", alone, SLOTS["dus_abs"])
    stats.update({k + " (alone)": v for k, v in sa.items()})
    _report(name, path, stats, t_ref, time.perf_counter() - t0)
    assert np.array_equal(_bits(rec), _bits(again)), (name, path, "two runs of the backward pass differ")
    if failed:
        raise failed[0]


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", ["lengths1", "stops"])
def test_nullable_fields(lib, name, path):
    c, inp = D.case(name, extras=True), inputs(name)
    full = forward(lib, inp, path, c.bg)
    _check(lib, full["rc"])
    for depth, alpha in ((True, False), (False, True), (False, False)):
        f = forward(lib, inp, path, c.bg, depth=depth, alpha=alpha)
        _check(lib, f["rc"])
        for k in ("image", "final_tau"):
            assert np.array_equal(_bits(f[k]), _bits(full[k])), (name, path, k, "depends on depth_out / alpha_out", depth, alpha)
        assert np.array_equal(f["contrib"], full["contrib"])
        assert f["untouched"]["depth"] == (not depth) and f["untouched"]["alpha"] == (not alpha)
        for k, on in (("depth", depth), ("alpha", alpha)):
            if on:
                assert np.array_equal(_bits(f[k]), _bits(full[k])), (name, path, k)
    run = lambda Wd, Wa: own_backward(lib, inp, path, full, ex=dict(bg=c.bg, Wd=Wd, Wa=Wa))
    both = run(inp.Wd, inp.Wa)
    assert _bits(both[:, SLOTS["dz"]]).any()
    for label, a, b in (("dloss_ddepth and dloss_dalpha NULL", run(None, None), run(inp.zeros, inp.zeros)),
                        ("dloss_ddepth NULL", run(None, inp.Wa), run(inp.zeros, inp.Wa)),
                        ("dloss_dalpha NULL", run(inp.Wd, None), run(inp.Wd, inp.zeros))):
        diff = np.argwhere(_bits(a).reshape(c.n, 12) != _bits(b).reshape(c.n, 12))
        assert diff.size == 0, (name, path, label, "differs from zero arrays in %d words, first (row, slot) %s" % (len(diff), diff[0]))
        assert _bits(a[:, :9]).any()
        if "ddepth" in label:
            zero_slots(name, path, label, a, SLOTS["dz"])
            zero_slots(name, path, label + " (zero array)", b, SLOTS["dz"])
        else:
            assert np.array_equal(_bits(a[:, SLOTS["dz"]]), _bits(both[:, SLOTS["dz"]])), (name, path, label, "dz depends on dL/dalpha")


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", D.SETS)
def test_extra_instances_against_plain(lib, name, path):
    pname = PATHS[path]["policy"]
    c, inp = D.case(name, extras=True), inputs(name)
    with labels(lib) as ran:
        p = forward(lib, inp, path, None)
    assert "k_draw" in ran and "k_draw_extra" not in ran, sorted(ran)
    x = forward(lib, inp, path, ZERO_BG)
    _check(lib, p["rc"]); _check(lib, x["rc"])
    assert all(p["untouched"][k] for k in ("depth", "alpha"))
    for k in ("image", "contrib", "final_tau"):
        diff = np.argwhere(p[k] != x[k])
        assert diff.size == 0, (name, path, k, "EXTRA over background 0 differs from the plain instance on %d values, first at %s: "
                                "%r against %r" % (len(diff), diff[0], x[k][tuple(diff[0])], p[k][tuple(diff[0])]))
    rec = own_backward(lib, inp, path, x, ex=dict(bg=ZERO_BG, Wd=inp.zeros, Wa=inp.zeros))
    stats = collections.OrderedDict()
    check_rows(name, path, "EXTRA with Wd = Wa = 0, background 0", rec, D.reference(name, pname), D.distances(name, pname),
               D.GRADS, stats, c)
    zero_slots(name, path, "EXTRA with Wd = 0", rec, SLOTS["dz"], SLOTS["dus_abs"])
    _report(name, path + " (EXTRA against the plain reference)", stats, 0.0, 0.0)


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("what", ["all_culled", "n0"])
def test_nothing_to_draw(lib, what, path):
    """n > 0 with every Gaussian behind the near plane (no patches), and n == 0: the memset branch of splat_draw_impl"""
    c = D.case("reach", extras=True)
    if what == "n0":
        inp = Inputs.__new__(Inputs)
        inp.c, inp.n = c, 0
        f = forward(lib, inp, path, c.bg)
    else:
        inp = inputs("reach")
        with labels(lib) as ran:
            f = forward(lib, inp, path, c.bg, depths_h=np.full(c.n, -1.0, np.float32))
        assert not {"k_draw", "k_draw_extra"} & ran, sorted(ran)
    _check(lib, f["rc"])
    assert f["P"] == 0
    for ch in range(3):
        assert (f["image"][ch] == np.float32(c.bg[ch])).all(), (what, path, "image is not the background")
    for k in ("depth", "alpha", "final_tau"):
        assert not _bits(f[k]).any(), (what, path, k)
    assert not f["contrib"].any() and not f["ranges"].any()


def test_refused_arguments(lib):
    name, path = "reach", "masked"
    c, inp = D.case(name, extras=True), inputs(name)
    seg_ws = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    with labels(lib) as ran:
        f = forward(lib, inp, path, c.bg, seg_ws=seg_ws)
    assert f["rc"] == BAD_ARG, f["rc"]
    assert not {"k_draw", "k_draw_extra", "k_draw_seg"} & ran and all(f["untouched"].values()), sorted(ran)
    ok = forward(lib, inp, path, c.bg)
    _check(lib, ok["rc"])
    d = ok["dev"]
    with labels(lib) as ran:
        rc, _, untouched = backward(lib, inp, path, d["rec"], ok["P"], d["contrib"].ptr, d["tau"].ptr, d["ranges"].ptr,
                                    d["walk"].ptr, ex=dict(bg=c.bg, Wd=inp.Wd, Wa=inp.Wa), absgrad=True)
    assert rc == BAD_ARG and untouched and not ran, (rc, sorted(ran))


_abs_ref = {}


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", D.SETS)
def test_abs_instance_unsplit(lib, name, path):
    """``k_draw_bwd_abs``: slots 10-11 against the float64 absolute screen-space gradient of the one-tile lists, slots 0-8
    against the plain reference, slot 9 zero (the segment-walk ABS instances: tests/test_gpu_absgrad.py)"""
    t0 = time.perf_counter()
    pname = PATHS[path]["policy"]
    c, inp = D.case(name), inputs(name)
    ref, dist = D.reference(name, pname), D.distances(name, pname)
    t_ref = time.perf_counter() - t0
    f = forward(lib, inp, path, None)
    _check(lib, f["rc"])
    check_lists(name, path, pname, f)
    check_contrib(name, path, f, ref)
    with labels(lib) as ran:
        rec = own_backward(lib, inp, path, f, absgrad=True)
    assert "k_draw_bwd_abs" in ran and not {"k_draw_bwd", "k_draw_bwd_extra"} & ran, sorted(ran)
    again = own_backward(lib, inp, path, f, absgrad=True)
    stats = collections.OrderedDict()
    step, failed = _steps()
    step(check_rows, name, path, "ABS", rec, ref, dist, D.GRADS + ("dus_abs",), stats, c)
    step(zero_slots, name, path, "ABS", rec, SLOTS["dz"])
    assert (rec[:, SLOTS["dus_abs"]] >= 0).all()
    _report(name, path + " (ABS)", stats, t_ref, time.perf_counter() - t0)
    assert np.array_equal(_bits(rec), _bits(again)), (name, path, "two runs of the ABS backward pass differ")
    if failed:
        raise failed[0]
