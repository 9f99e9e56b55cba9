"""The binning chain on hand-built 2D Gaussians, by list shape and size: count (``k_bin_count`` / ``k_pack_bin``), the
depth sort with its max-key fold and record gather (``k_radix_hist`` / ``k_radix_scatter``), the offsets scan
(``k_bin_scan_partials`` / ``k_bin_scan_apply``), ``k_bin_emit``, the tile sort under a device-side count and
``k_tile_ranges`` (csrc/egs_bin.hip, csrc/egs_sort.hip), through the raw C ABI on the case sets of tests/bin_cases.py.
Everything here is an integer: there is no tolerance anywhere.

Two surfaces per case:
  tensor    ``egs_splat_bin`` -> read ``total_patches`` -> ``egs_splat_draw`` (buffers of exactly P entries)
  records   ``egs_splat_bin_pack`` -> ``egs_splat_draw_rec_seg`` with the count on the device, the masked and the plain
            list (gsplatcu cases: the entry point demands the policy), at each capacity of P, P + 1 and the next multiple
            of 2048 above P plus 1 (at least 1: the entry point refuses a capacity of 0); the ``totals`` cases also at a
            capacity of 2 621 441 + P, which puts a list of a few entries on the 16-items-per-thread tile sort.
2D Gaussians besides the three arrays of the case: isotropic conic 0.02, alpha 0.5, colour 0.5.

Asserted, all exact: total_patches == (P, largest key of a Gaussian with patches); ranges ((0, 0) for empty tiles) and the
id list == ``reference_lists``; masked & 0x0FFFFFFF == the plain list; depths / areas after the in-place cull and
``visible``; every list entry at and beyond P, and 2048 words in front of and behind every output, keep their
sentinel (no kernel of the chain writes there by design: k_bin_emit stops at its span, the scatter and k_tile_ranges at
the device count); on ``keys`` and ``totals`` a second call gives the same lists bit for bit.  The depth-key hint
(``keys`` cases, tensor surface; need = bit length of the largest key): hints 0, 32, need, need + 1 and the next two
multiples of 8 from need give the exact lists (odd and even pass counts: the copy back to the primary buffers runs); hints
need - 1 and 1 still give the exact P and the TRUE largest key in total_patches[1], which is what the host's redo
protocol reads -- no draw after those.

Decided from the reference, not from the kernel.  All three findings were defects of the ORACLE; the kernels passed
every case as they were and csrc is unchanged:
  +inf depth   kernel.cu:73 ``uint32_t depth_cm = depth * 1000`` is a float -> u32 conversion.  The GPU instruction behind it
               (cvt.rzi.u32.f32 in the reference's build, v_cvt_u32_f32 here) saturates: +inf, like 5e6 * 1000, becomes
               0xFFFFFFFF and NaN becomes 0.  The kernel's ``(uint32_t)(depth * 1000.f)`` is the reference's behaviour.
               ``O.depth_keys`` mapped every non-finite product to 0, and clamped the finite ones in float32, where
               2^32 - 1 rounds to 2^32 and wrapped to 0 as well: it saturates now.  First failing case: keys/saturate on
               the CPU ("key missed" at Gaussians 100 (5e6), 200 (+inf), 1700, 1701: 0 for 4294967295).
  NaN depth    kernel.cu:61 and :97 test ``depth < MIN_DEPTH``, which is false for NaN: the Gaussian keeps its rect, with
               key 0, and so does bin_count_one.  ``O.get_rects`` tested ``depth >= MIN_DEPTH`` and dropped it; it follows
               the reference now.  First failing case: counts/n1_all_nan on the CPU ("rect missed").  This is what lets a
               test put patch-less Gaussians anywhere in DEPTH order (tests/bin_cases.py).
  reversed     a negative radius reverses the rect; kernel.cu:112 multiplies in uint and claims ~2^32 patches.
               bin_count_one defines such a rect as empty and culls in place; ``O.get_rects`` wrapped like the reference
               (``O.bin_tiles`` would then emit 2^32 entries).  The oracle takes the project's definition now.  First
               failing case: counts/n255_only_last_mm on the CPU ("patches where none were meant", Gaussian 3).

Measured on MI355X, per set: cases; n; P; real passes of the depth sort at hint 32; passes of the tile sort:
  counts   145 cases; n 1 .. 4097;            P 0 .. 4097;   depth passes 1 and 2;    tile passes 1 (one_big_alone: 2)
  totals    28 cases; n 3 .. 5122;            P 3 .. 4097;   depth passes 2;          tile passes 1
  keys      12 cases; n 3000;                 P 3147;        depth passes 1, 2, 3, 4; tile passes 1
  grid       8 cases; n 300;                  P 282 .. 363;  depth passes 2;          tile passes 1, 1, 1, 1, 2, 2, 2, 3
  large      2 cases; n 2 621 440, 2 621 441; P 2 246 949;   depth passes 2;          tile passes 2
Wall time: the whole module 4.4 s (235 tests); test_large 0.75 s and 0.66 s, of which both surfaces with their copies and
comparisons take 0.10 s; every other test below 0.2 s.

Seeded errors (csrc), and the tests that fail.  The first two were each run once on a scratch build; the others change
an offset, a count or a tile key, can send k_bin_emit or k_tile_ranges out of bounds and were never run:
  k_radix_scatter  ``rank[r] = prev + below`` -> ``prev + (peers - 1 - below)``: the rank among the wave's equal digits
                   counted from the other end -- still a permutation of the tile, every index in range.
                   Run once: test_lists[keys-equal] ("ids", entry 0 of tile 0: 120 for 12; 2933 entries differ), every
                   other keys case, and the counts cases from test_lists[counts-n255_all_mm] on (entry 4 of tile 0: 250
                   for 200); counts-n2_all_* pass (two Gaussians, two tiles: no equal digits)
  bin_count_one    ``depth * 1000.f`` -> ``depth * 100.f``: keys only, no index or offset depends on a key.
                   Run once: test_lists[counts-n1_all_mm] first ("total_patches[1]", 20 for 200), every gsplatcu keys
                   case in test_lists and test_depth_key_hint (keys/equal: 77 for 777); the forward_cpu cases pass
                   (float-bit keys)
  k_bin_emit       ``s_off[lo + step] <= s0`` -> ``<``      NOT run, reasoned: a slot that starts a run finds the previous
                   owner and r runs past that Gaussian's rect; on the records surface (every tile, row-major) the tile row
                   y0 + r / w can leave the grid and k_tile_ranges would write ``ranges`` out of bounds.  Where it stays
                   inside, test_lists[counts-n2_all_mm]: the second slot goes to the first Gaussian again, one tile holds
                   two entries and the other none ("ranges")
  k_bin_scan_apply ``b.w = b.z + v[6]`` -> ``v[7]``         NOT run, reasoned: the eighth offset of every thread is off by
                   count[7] - count[6]: runs overlap or leave slots unwritten, which keep whatever the key buffer held --
                   k_tile_ranges uses that as an index into ``ranges``.  test_lists[counts-n256_last_of_wg_nan]: Gaussian
                   255 has no patches, 254 has one; the offset of 255 drops to 254, the workgroup's span ends one slot
                   early and slot 254 is never written
  k_radix_scatter  the ``EXTRA == 1`` gather dropped from the identity-pass branch      NOT run, reasoned: under gsplatcu
                   with hint 32 the last depth pass is an identity pass for every key below 2^24, so cr_sorted and
                   cnt_sorted stay uninitialised: P and every offset are garbage and k_bin_emit writes where they point.
                   Every case with P > 0 and a largest key below 2^24, first test_lists[counts-n1_all_mm]
  k_tile_ranges    ``if (p == P - 1)`` -> ``if (p == P)`` (never true: one store less, nothing out of range)
                   NOT run, reasoned: the last non-empty tile keeps end 0: test_lists[counts-n1_all_mm] ("ranges",
                   tile 0: (0, 0) for (0, 1)) and every case with P > 0
"""
import ctypes as C
import time

import numpy as np
import pytest
import torch

from tests import bin_cases as BC
from tests.gpu_abi import Out, _check, _ptr, _stream

pytestmark = pytest.mark.gpu

DEV = "cuda"
MASKED_LISTS = 2                                    # include/egs_hip.h EGS_DRAW_MASKED_LISTS
GSID_MASK = 0x0FFFFFFF
LONG_CAP = BC.RS_SHORT + 1                          # the first capacity on the 16-items-per-thread tile sort


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


class Inputs:
    """the case on the device: us and the benign cinv2ds / alphas / colors; areas and depths are given to every call as
    fresh sentinel-banded copies (the binning stage writes them in place)"""

    def __init__(self, case):
        self.case = case
        self.us_h, self.areas_h, self.depths_h = BC.build(case)
        n = case.n
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)
        self.us = dev(self.us_h)
        self.cinv = dev(np.tile(np.float32([0.02, 0.0, 0.02]), (n, 1)))
        self.alphas = dev(np.full(n, 0.5))
        self.colors = dev(np.full((n, 3), 0.5))

    def in_place(self):
        n = self.case.n
        return Out(2 * n, self.areas_h), Out(n, self.depths_h)


def _images(case):
    e = lambda shape, dt: torch.empty(shape, dtype=dt, device=DEV)
    return e((3, case.H, case.W), torch.float32), e((case.H, case.W), torch.int32), e((case.H, case.W), torch.float32)


def _tiles(case):
    gx, gy = BC.grid(case.W, case.H)
    return gx * gy


def run_tensor(lib, inp, hint=0, draw=True):
    """egs_splat_bin (-> total_patches read back) -> egs_splat_draw
    -> dict: P, maxkey, depths, areas after the call; with ``draw``: ranges [T, 2], ids [P]"""
    case = inp.case
    n, pol, st = case.n, _policy(lib, case.policy), _stream()
    areas, depths = inp.in_place()
    total = Out(2)
    ws_bin = torch.empty(lib.egs_splat_bin_ws_bytes(n), dtype=torch.uint8, device=DEV)
    _check(lib, lib.egs_splat_bin(n, case.W, case.H, _ptr(inp.us), areas.ptr, depths.ptr, C.byref(pol), hint, _ptr(ws_bin),
                                  ws_bin.numel(), total.ptr, st))
    torch.cuda.synchronize()
    tot = total.read("total_patches").view(np.uint32)
    out = dict(P=int(tot[0]), maxkey=int(tot[1]), depths=depths.read("depths").view(np.float32).copy(),
               areas=areas.read("areas").reshape(n, 2).copy())
    if not draw:
        return out
    P = out["P"]
    assert P == BC.reference_lists(case)["P"], (case, "total_patches[0]", P)      # (the buffers below are sized by it)
    image, contrib, tau = _images(case)
    T = _tiles(case)
    ranges, gsid = Out(2 * T), Out(P)
    ws_draw = torch.empty(lib.egs_splat_draw_ws_bytes(n, P, case.W, case.H), dtype=torch.uint8, device=DEV)
    _check(lib, lib.egs_splat_draw(n, P, case.W, case.H, _ptr(inp.us), _ptr(inp.cinv), _ptr(inp.alphas), _ptr(inp.colors),
                                   areas.ptr, C.byref(pol), _ptr(ws_bin), _ptr(ws_draw), ws_draw.numel(), _ptr(image),
                                   _ptr(contrib), _ptr(tau), ranges.ptr, gsid.ptr, st))
    torch.cuda.synchronize()
    out.update(ranges=ranges.read("ranges").reshape(T, 2).copy(), ids=gsid.read("gsid_per_patch").copy(),
               areas_after_draw=areas.read("areas").reshape(n, 2).copy())
    return out


def run_records(lib, inp, cap):
    """egs_splat_bin_pack -> egs_splat_draw_rec_seg (count on the device, lists of ``cap`` entries, masked and plain)
    -> dict: P, maxkey, depths, areas, visible, ranges, masked / plain (all ``cap`` words), and their sentinels"""
    case = inp.case
    n, pol, st = case.n, _policy(lib, case.policy), _stream()
    areas, depths = inp.in_place()
    total = Out(2)
    ws_bin = torch.empty(lib.egs_splat_bin_ws_bytes(n), dtype=torch.uint8, device=DEV)
    rec = torch.empty((n, 12), dtype=torch.float32, device=DEV)
    visible = torch.full((n,), 0xAA, dtype=torch.uint8, device=DEV)
    _check(lib, lib.egs_splat_bin_pack(n, case.W, case.H, _ptr(inp.us), _ptr(inp.cinv), _ptr(inp.alphas), _ptr(inp.colors),
                                       areas.ptr, depths.ptr, C.byref(pol), 0, _ptr(ws_bin), ws_bin.numel(), total.ptr,
                                       None, _ptr(rec), None, _ptr(visible), st))
    image, contrib, tau = _images(case)
    T = _tiles(case)
    ranges, masked, plain = Out(2 * T), Out(cap), Out(cap)
    ws_draw = torch.empty(lib.egs_splat_draw_ws_bytes(n, cap, case.W, case.H), dtype=torch.uint8, device=DEV)
    _check(lib, lib.egs_splat_draw_rec_seg(n, cap, total.ptr, case.W, case.H, _ptr(rec), C.byref(pol), _ptr(ws_bin),
                                           _ptr(ws_draw), ws_draw.numel(), _ptr(image), _ptr(contrib), _ptr(tau),
                                           ranges.ptr, masked.ptr, None, None, None, 0, MASKED_LISTS, None, 0, None, None,
                                           plain.ptr, st, None))
    torch.cuda.synchronize()
    tot = total.read("total_patches").view(np.uint32)
    return dict(P=int(tot[0]), maxkey=int(tot[1]), depths=depths.read("depths").view(np.float32).copy(),
                areas=areas.read("areas").reshape(n, 2).copy(), visible=visible.cpu().numpy(),
                ranges=ranges.read("ranges").reshape(T, 2).copy(), masked=masked.read("masked list").copy(),
                plain=plain.read("plain list").copy(), masked_old=masked.old(), plain_old=plain.old())


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


def check_counts(case, ref, got, what):
    assert got["P"] == ref["P"], (case, what, "total_patches[0]", got["P"], ref["P"])
    assert got["maxkey"] == ref["maxkey"], (case, what, "total_patches[1]", got["maxkey"], ref["maxkey"])
    assert _same_bits(got["depths"], ref["depths"]), (case, what, "depths after the in-place cull",
                                                      np.nonzero(got["depths"].view(np.int32) != ref["depths"].view(np.int32))[0][:5])
    assert np.array_equal(got["areas"], ref["areas"]), (case, what, "areas after the in-place cull")


def check_lists(case, ref, ranges, ids, what):
    if not np.array_equal(ranges, ref["ranges"]):
        t = int(np.nonzero((ranges != ref["ranges"]).any(1))[0][0])
        raise AssertionError((case, what, "ranges", "tile %d" % t, tuple(ranges[t]), "for", tuple(ref["ranges"][t])))
    assert ids.shape == ref["ids"].shape, (case, what, ids.shape)
    if not np.array_equal(ids, ref["ids"]):
        p = int(np.nonzero(ids != ref["ids"])[0][0])
        t = int(np.nonzero((ref["ranges"][:, 0] <= p) & (p < ref["ranges"][:, 1]))[0][0])
        raise AssertionError((case, what, "ids", "entry %d (tile %d, entry %d of its run)" % (p, t, p - ref["ranges"][t, 0]),
                              int(ids[p]), "for", int(ref["ids"][p]), "; %d entries differ" % int((ids != ref["ids"]).sum())))


def record_caps(P):
    return sorted({max(P, 1), P + 1, (P // 2048 + 1) * 2048 + 1})


def check_records(case, ref, got, cap, what):
    P = ref["P"]
    check_counts(case, ref, got, what)
    assert np.array_equal(got["visible"], ref["visible"]), (case, what, "visible")
    check_lists(case, ref, got["ranges"], got["plain"][:P], what + " plain")
    masked = got["masked"][:P].view(np.uint32)
    assert np.array_equal((masked & GSID_MASK).astype(np.int32), got["plain"][:P]), (case, what, "masked & 0x0FFFFFFF")
    assert np.array_equal(got["masked"][P:], got["masked_old"][P:]), (case, what, "masked list written at or beyond P")
    assert np.array_equal(got["plain"][P:], got["plain_old"][P:]), (case, what, "plain list written at or beyond P")


stats = {}


def _note(case, ref, seconds):
    s = stats.setdefault(case.cset, dict(cases=0, n=[], P=[], dp=set(), tp=set()))
    s["cases"] += 1
    s["n"].append(case.n)
    s["P"].append(ref["P"])
    s["dp"].add(BC.real_depth_passes(ref["maxkey"]))
    s["tp"].add(BC.sort_passes(BC.tile_key_bits(_tiles(case))))
    print("\nbin_lists %s/%s: n %d, P %d, depth passes %d, tile passes %d, %.2f s | set so far: %d cases, n %d..%d, "
          "P %d..%d, depth passes %s, tile passes %s" % (case.cset, case.name, case.n, ref["P"],
                                                          BC.real_depth_passes(ref["maxkey"]),
                                                          BC.sort_passes(BC.tile_key_bits(_tiles(case))), seconds, s["cases"],
                                                          min(s["n"]), max(s["n"]), min(s["P"]), max(s["P"]), sorted(s["dp"]),
                                                          sorted(s["tp"])))


def both_surfaces(lib, case, twice, caps=None):
    ref = BC.reference_lists(case)
    t0 = time.perf_counter()
    inp = Inputs(case)
    got = run_tensor(lib, inp)
    check_counts(case, ref, got, "tensor")
    check_lists(case, ref, got["ranges"], got["ids"], "tensor")
    assert np.array_equal(got["areas_after_draw"], ref["areas"]), (case, "the draw wrote areas")
    if twice:
        again = run_tensor(lib, inp)
        assert np.array_equal(again["ranges"], got["ranges"]) and np.array_equal(again["ids"], got["ids"]), (case, "tensor, second call")
    if case.policy == "gsplatcu":
        first = None
        for cap in (caps or record_caps(ref["P"])):
            rec = run_records(lib, inp, cap)
            check_records(case, ref, rec, cap, "records, capacity %d" % cap)
            first = first or rec
        if twice:
            again = run_records(lib, inp, max(ref["P"], 1))
            assert np.array_equal(again["masked"], first["masked"]) and np.array_equal(again["plain"], first["plain"]) \
                and np.array_equal(again["ranges"], first["ranges"]), (case, "records, second call")
    _note(case, ref, time.perf_counter() - t0)


SMALL = [(s, name) for s in ("counts", "totals", "keys", "grid") for name in BC.names(s)
         if not (s == "grid" and name == "T66049")]


@pytest.mark.parametrize("cset,name", SMALL, ids=["%s-%s" % sn for sn in SMALL])
def test_lists(lib, cset, name):
    both_surfaces(lib, BC.get(cset, name), twice=cset in ("keys", "totals"))


def test_three_pass_tile_sort(lib):
    """66 049 tiles: a 17-bit tile key in passes of 6, 6 and 5 bits (4100 x 4101 pixels: the one case with a large image)"""
    both_surfaces(lib, BC.get("grid", "T66049"), twice=False)


@pytest.mark.parametrize("n", BC.LARGE_N, ids=["n%d" % n for n in BC.LARGE_N])
def test_large(lib, n):
    """the last count on the 8-items-per-thread instances of the depth sort and the first on ``k_radix_hist<16>`` with the
    fold / ``k_radix_scatter<16, 1>``; the records surface at the capacity P only"""
    case = BC.large_case(n)
    both_surfaces(lib, case, twice=False, caps=[case.claims["P"]])


@pytest.mark.parametrize("name", BC.names("totals"))
def test_short_list_under_a_long_capacity(lib, name):
    """a capacity above 2 621 440 with P far below it: the tile sort takes its 16-items-per-thread instances
    (4096-item tiles, 641 workgroups of which one or two hold entries) and k_tile_ranges a grid for the capacity"""
    case = BC.get("totals", name)
    ref = BC.reference_lists(case)
    cap = LONG_CAP + ref["P"]
    check_records(case, ref, run_records(lib, Inputs(case), cap), cap, "records, capacity %d" % cap)


@pytest.mark.parametrize("name", BC.names("keys"))
def test_depth_key_hint(lib, name):
    case = BC.get("keys", name)
    ref = BC.reference_lists(case)
    inp = Inputs(case)
    need = BC.bit_length(ref["maxkey"])
    assert need >= 8
    m = 8 * ((need + 7) // 8)
    enough = sorted({0, 32, need, need + 1, m, min(m + 8, 32)})
    assert {BC.sort_passes(h if 0 < h <= 32 else 32) & 1 for h in enough} == {0, 1} or need > 24, (case, enough)
    for hint in enough:
        got = run_tensor(lib, inp, hint=hint)
        check_counts(case, ref, got, "hint %d" % hint)
        check_lists(case, ref, got["ranges"], got["ids"], "hint %d" % hint)
    for hint in sorted({need - 1, 1}):
        got = run_tensor(lib, inp, hint=hint, draw=False)
        check_counts(case, ref, got, "hint %d (too small)" % hint)
