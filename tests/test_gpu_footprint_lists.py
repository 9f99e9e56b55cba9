"""The footprint cull on hand-built Gaussians, by rect form and edge: ``foot_setup`` / ``foot_slab`` / ``foot_row`` /
``foot_mask`` / ``foot_bitmap`` / ``foot_tilemap`` / ``foot_count`` (csrc/egs_gaussian_math.h) and the four emission forms of
``k_bin_emit`` (csrc/egs_bin.hip) against the float64 reference of tests/footprint_ref.py, on its case sets.

Every case is first run through ``egs_fused_forward`` with us / cinv2ds / areas / depths / rec materialised; ``fused.forward``
on the same inputs must leave the same records bit for bit, and ALL truth is computed in float64 from those float32 2D
Gaussians of the device (the lift of the case builder only has to land near its targets).  Then, for every tile and
every entry, nothing sampled:

  fused culled lists    an ordered subsequence of the reference list; every entry whose ``must`` mask is non-zero, none
                        whose ``may`` mask is zero; must <= mask <= may bitwise; (0, 0) for tiles without entries;
                        never-blending Gaussians nowhere, uncullable ones in every tile of their rect with mask 15;
  culled | unculled     ``fused.CULL_LISTS`` off: the unculled lists ARE the reference lists; the image is bit-identical, every
                        pixel's last contributor the same Gaussian, final_tau bit-identical on every tile whose culled list
                        is not empty (a tile the cull empties is drawn as a tile without patches: final_tau 0, the
                        reference's convention for those, against exactly 1 unculled); the gradient records of the
                        backward's draw pass and the parameter gradients by the default rule of tests/gradcheck.py
                        (atomics reorder; dL/dpws, dL/dscales, dL/drots of conics of eigenvalue ratio >= 100 by the
                        bound ``chain_tolerance`` derives from the number format, which grows with that ratio);
  seven-op surface      ``gsplatcu.splat_with_records`` on the materialised tensors: ranges / gsid equal ``O.bin_tiles``,
                        the walked list carries them; its masks obey must <= mask <= may too, equal the fused path's mask
                        for every (tile, Gaussian) in both lists, and are zero for every pair the fused path dropped;
                        all outputs bit-identical with ``MASKED_LISTS`` off (the exact-threshold Gaussians of ``faint`` are
                        fed here as hand-written 2D values);
  order                 both surfaces twice, lists bitwise equal between the runs.

Measured on MI355X, per set (order: summed over its eleven cases): reference entries, entries the fused lists drop, blocks
must / device / may, and the share of (entry, block) pairs in may and not in must (the last measured on the CPU, tests/
test_footprint_ref_cpu.py; for order the largest of its cases):
  forms        2982 entries,  775 dropped, blocks  7440 /  7614 /  7649, share 0.018
  tangent      1935 entries, 1769 dropped, blocks   292 /   311 /   311, share 0.002
  faint         428 entries,  415 dropped, blocks    32 /    32 /    32, share 0.000
  needles      2039 entries, 1277 dropped, blocks  1647 /  1819 /  1868, share 0.027
  uncullable    447 entries,    3 dropped, blocks   251 /  1715 /  1717, share 0.820 (exempt from the cap)
  tall         1264 entries,   98 dropped, blocks  3859 /  4301 /  4376, share 0.102 (exempt)
  wide         1280 entries,  100 dropped, blocks  3868 /  4306 /  4380, share 0.100 (exempt)
  order        8702 entries, 2522 dropped, blocks 12890 / 13255 / 13364, share 0.018

What these tests found.  ``foot_slab`` widened the slab by eps AND the footprint's own y-extent by eps: a slab lying up to
2 eps beyond the top or bottom of the ellipse was kept and given the pixels around the centre line there.  Fourteen masks
of these sets exceeded ``may`` (forms 4, needles 1, order 9), the same entries on both surfaces; first: u = (79.5, 71.5),
conic (0.0028193, 0, 0.0028193), alpha 0.05, tile (4, 1): device mask 14, must = may = 12 -- the ellipse's top is at
y = 23.72, 0.72 px below the block's last row 23, with eps = 0.53 and e = 0.66.  Decided by hand: the derivation of e
holds (each bound widened once), the kernel over-marked; ``foot_slab`` now clamps to +-ymax (the slab's eps covers the
rounding of ymax, 1e-6 of it) and every mask of every set lies within the two bounds.

Mutations, each on a scratch build of the library:
  foot_bitmap  ``2u << br`` -> ``1u << br``       run once: caught by test_fused_culled_lists_within_the_two_bounds[tangent]
                                              ("32 contributing entries were dropped", first the tile a footprint reaches
                                              by half a pixel)
  foot_mask    ``X + 8`` -> ``X + 9``             run once: caught by test_fused_culled_lists_within_the_two_bounds[tangent]
                                              ("3 masks miss a contributing block", the tile-bitmap and row-walk forms)
  foot_tilemap ``hi - x0`` -> ``hi - x0 - 1``     NOT run, reasoned: for hi == x0 the shift count is -1 (undefined; the
                                              hardware's 2u << 31 sets bits 8..31 of the row, which spill into the bitmap
                                              rows below), so k_bin_emit can emit tile indices beyond the grid and
                                              k_tile_ranges would write ``ranges`` out of bounds.  Where it stays defined it
                                              drops the last tile of every row of a 5..8-tile rect, count and emission
                                              alike: test_fused_culled_lists_within_the_two_bounds[forms] fails with
                                              "contributing entries were dropped" (the ``over`` rects of 5 to 8 tiles fill their rows)
  wave walk    ``run +=`` dropped                 NOT run, reasoned: rows 64.. of a rect restart at offset 0 of the Gaussian's
                                              run, their own slots keep whatever the uninitialised key buffer held, and
                                              k_tile_ranges indexes ``ranges`` with those keys -- out of bounds.  With keys
                                              that happen to be valid the lists of ``tall`` lose tile rows 64..67 of its
                                              three 68-row Gaussians: test_fused_culled_lists_within_the_two_bounds[tall]
                                              (``wide`` never takes a second round: no rect has more than 64 rows)
"""
import ctypes as C

import numpy as np
import pytest
import torch

from easygaussiansplatting_amd import scene as S
from oracle import gs_oracle as O
from tests import footprint_ref as F
from tests.gpu_abi import Out, _check, _pol, _ptr, _stream
from tests.gradcheck import TOL_MAX, assert_grad_close

pytestmark = pytest.mark.gpu

DEV = "cuda"
CULLED_LISTS = 32                                   # include/egs_hip.h EGS_FUSED_CULLED_LISTS
GSID_MASK = 0x0FFFFFFF
ILL_RATIO = 100.0                                   # eigenvalue ratio of a conic from which the chain rule gets its own bound
CASES = [c.name for c in F.all_cases()]
BY_NAME = {c.name: c for c in F.all_cases()}
totals = {}                                         # set -> summed counts of the fused lists, printed per case


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from easygaussiansplatting_amd import _lib, gsplatcu
    gsplatcu.set_policy("gsplatcu")
    yield _lib.load()
    gsplatcu.set_policy("gsplatcu")


@pytest.fixture
def knobs():
    """the two A/B knobs, put back whatever the test did"""
    from easygaussiansplatting_amd import fused, gsplatcu
    before = fused.CULL_LISTS, gsplatcu.MASKED_LISTS
    yield fused, gsplatcu
    fused.CULL_LISTS, gsplatcu.MASKED_LISTS = before


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.int32)


class Run:
    pass


_runs = {}


def device_run(lib, name):
    """the case on the device, once: its inputs, the materialised 2D Gaussians and the reference lists made from them"""
    if name in _runs:
        return _runs[name]
    from easygaussiansplatting_amd.function import Camera
    case = BY_NAME[name]
    inp = F.lift(case)
    r = Run()
    r.case, r.n, r.W, r.H = case, case.n, case.width, case.height
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)
    r.P = {k: t(inp[k]) for k in ("pws", "shs", "alphas", "scales", "rots")}
    r.cam = Camera(r.W, r.H, inp["fx"], inp["fy"], inp["cx"], inp["cy"], inp["Rcw"], inp["tcw"], DEV)
    n = r.n
    us, depths, cinv, col, areas, rec = Out(2 * n), Out(n), Out(3 * n), Out(3 * n), Out(2 * n), Out(12 * n)
    vis = torch.zeros(n + 512, dtype=torch.uint8, device=DEV)
    ws_bin = torch.empty(lib.egs_splat_bin_ws_bytes(n), dtype=torch.uint8, device=DEV)
    total = torch.zeros(2, dtype=torch.int32, device=DEV)
    _check(lib, lib.egs_fused_forward(
        n, 3, _ptr(r.P["pws"]), _ptr(r.P["rots"]), _ptr(r.P["scales"]), _ptr(r.P["shs"]), None, _ptr(r.P["alphas"]),
        _ptr(r.cam.Rcw), _ptr(r.cam.tcw), _ptr(r.cam.twc), r.cam.fx, r.cam.fy, r.cam.cx, r.cam.cy, r.W, r.H, C.byref(_pol()),
        us.ptr, depths.ptr, cinv.ptr, col.ptr, areas.ptr, rec.ptr, C.c_void_p(vis.data_ptr() + 256), None, CULLED_LISTS, 0,
        _ptr(ws_bin), ws_bin.numel(), _ptr(total), None, _stream()))
    torch.cuda.synchronize()
    f = lambda o, w, shape: o.read((name, w)).view(np.float32).reshape(shape).copy()
    r.us, r.depths, r.cinv, r.col = f(us, "us", (n, 2)), f(depths, "depths", (n,)), f(cinv, "cinv2ds", (n, 3)), f(col, "colors", (n, 3))
    r.areas = areas.read((name, "areas")).reshape(n, 2).copy()
    r.rec = rec.read((name, "rec")).copy()
    r.alphas = inp["alphas"]
    r.patches = int(total[0].item())
    r.L = F.reference_lists(r.us, r.cinv, r.alphas, r.areas, r.depths, r.W, r.H)
    _runs[name] = r
    return r


def fused_forward(r, need_grad=False):
    from easygaussiansplatting_amd import fused
    P = r.P
    image, mask, st = fused.forward(P["pws"], P["shs"], P["alphas"], P["scales"], P["rots"], r.cam, need_grad=need_grad)
    torch.cuda.synchronize()
    return image, st


def fused_lists(r, st):
    return host(st.ranges), host(st.gaussian_ids()), host(st.block_masks())


def scatter_masks(L, ranges, ids, masks):
    """the device's masks in the entry space of the reference lists (-1: not listed); the lists were checked before"""
    lens = ranges[:, 1] - ranges[:, 0]
    key = np.repeat(np.arange(len(ranges)), lens).astype(np.int64) * max(len(L.alphas), 1) + ids
    ref = L.tile * max(len(L.alphas), 1) + L.gsid
    o = np.argsort(ref, kind="stable")
    where = o[np.searchsorted(ref[o], key)]
    dm = np.full(L.gsid.size, -1, np.int64)
    dm[where] = masks
    return dm


def plain_ranges(L):
    rg = L.ranges.copy()
    rg[rg[:, 1] == rg[:, 0]] = 0
    return rg


# ------------------------------------------------------------------------------------------------- fused culled lists
@pytest.mark.parametrize("name", CASES)
def test_fused_culled_lists_within_the_two_bounds(lib, knobs, name):
    fused, _ = knobs
    fused.CULL_LISTS = True
    r = device_run(lib, name)
    image, st = fused_forward(r)
    assert st.culled
    assert np.array_equal(bits(host(st.rec)), r.rec), (name, "the records of fused.forward differ from the materialised ones")
    rg, ids, masks = fused_lists(r, st)
    assert st.patch_count() == r.patches == ids.size
    got = F.check_culled(r.L, rg, ids, masks, name)
    print("\n%s: entries %d, dropped %d, blocks must %d / device %d / may %d" % (name, got["entries"], got["dropped"], got["must"],
                                                                             got["device"], got["may"]))
    key = "order" if name.startswith("order") else name
    tot = totals.setdefault(key, dict(entries=0, dropped=0, must=0, device=0, may=0))
    for k in tot:
        tot[k] += got[k]
    print("  set %s so far: %s" % (key, tot))
    if name.startswith("order"):                       # twice: the lists are bitwise the same
        image2, st2 = fused_forward(r)
        assert torch.equal(st.ranges, st2.ranges) and torch.equal(st.gsid[:ids.size], st2.gsid[:ids.size]), name
        assert torch.equal(image.view(torch.int32), image2.view(torch.int32)), name


# ------------------------------------------------------------------------------------------------ culled | unculled
def first_difference(a, b, r, st_c):
    """where two images differ, for the failure message: the pixel, its tile and that tile's culled list"""
    d = np.nonzero((bits(a) != bits(b)).reshape(a.shape).reshape(-1, r.H, r.W).any(0))
    if d[0].size == 0:
        return None
    y, x = int(d[0][0]), int(d[1][0])
    t = (y // 16) * r.L.gx + x // 16
    rg, ids, masks = fused_lists(r, st_c)
    sel = slice(rg[t, 0], rg[t, 1])
    ref = r.L.gsid[r.L.ranges[t, 0]:r.L.ranges[t, 1]]
    return dict(pixels=int(d[0].size), first=(x, y), tile=t, block=((x % 16) // 8, (y % 16) // 8), culled=list(zip(ids[sel].tolist(), masks[sel].tolist())),
                reference=[(int(g), int(mu), int(ma)) for g, mu, ma in zip(ref, r.L.must[r.L.ranges[t, 0]:r.L.ranges[t, 1]],
                                                                             r.L.may[r.L.ranges[t, 0]:r.L.ranges[t, 1]])])


def eigen_ratio(cinv):
    """largest / smallest eigenvalue of each conic (inf where it is not positive definite)"""
    c0, c1, c2 = (cinv[:, k].astype(np.float64) for k in range(3))
    mean, half = 0.5 * (c0 + c2), np.hypot(0.5 * (c0 - c2), c1)
    with np.errstate(all="ignore"):
        return np.where(mean - half > 0, (mean + half) / (mean - half), np.inf)


def chain_tolerance(kappa, pixels):
    """Bound on |culled - unculled| of a row of dL/dpws, dL/dscales, dL/drots, as a share of the tensor's largest entry,
    from the number format alone.  Both sides run the same chain-rule kernel on the draw pass's record of dL/dconic, a
    float32 sum of one term per pixel in two different orders: two such sums of P terms differ by a random walk of
    sqrt(2 P) roundings of 2^-24, taken at three sigma: 3 sqrt(2 P) 2^-24 of the record's size.  The chain rule
    dL/dSigma = -C (dL/dC) C of an elongated Gaussian is carried by the projection of dL/dC on the SHORT axis, and the
    pixels of its footprint lie along the long one: that projection is the record's size / kappa (the ratio of the
    squared extents), so its relative error, and that of the gradients made from it, is kappa times the record's.
    Never below the rule's own 2e-4; above 1 (the conics the code refuses to cull, kappa >= 1e4) it binds nothing.
    Measured on MI355X (each case prints its own), largest error of a row against its bound: needles dL/dscales 3.1e-4
    of the largest entry at kappa 1500 (bound 0.021), dL/drots 1.4e-4 (0.016), dL/dpws 5.3e-5 (0.021); forms, tall and
    wide below 3e-6 (bounds 2e-3 .. 0.1); uncullable, kappa 1.2e5: 0.2 (1.7)."""
    return np.maximum(TOL_MAX, kappa * 3 * np.sqrt(2 * pixels) * 2.0 ** -24)


@pytest.mark.parametrize("name", CASES)
def test_culled_and_unculled_lists_render_the_same(lib, knobs, name):
    fused, _ = knobs
    r = device_run(lib, name)
    P = r.P
    dl = torch.from_numpy((S.normal(41, 1, (3, r.H, r.W)) / (3 * r.H * r.W)).astype(np.float32)).to(DEV)
    out = {}
    for cull in (True, False):
        fused.CULL_LISTS = cull
        image, st = fused_forward(r, need_grad=True)
        assert st.culled == cull
        records = st.gpack                             # the draw pass of the backward leaves its gradient records here
        grads = fused.backward(P["pws"], P["shs"], P["alphas"], P["scales"], P["rots"], r.cam, st, dl)
        torch.cuda.synchronize()
        out[cull] = (host(image), host(st.final_tau), st, [host(g) for g in grads], host(records).astype(np.float64))
    img_c, tau_c, st_c, g_c, rec_c = out[True]
    img_u, tau_u, st_u, g_u, rec_u = out[False]
    # the unculled lists are the reference lists, all blocks
    assert np.array_equal(host(st_u.ranges), plain_ranges(r.L)), name
    assert np.array_equal(host(st_u.gaussian_ids()), r.L.gsid), name
    assert (host(st_u.block_masks()) == 15).all()
    assert np.array_equal(bits(img_c), bits(img_u)), (name, "the image changes with the cull", first_difference(img_c, img_u, r, st_c))
    # contrib is the 1-based position of the pixel's last contributor in its tile's list: the same Gaussian on both sides
    last = []
    for st in (st_c, st_u):
        rg, ids, cont = host(st.ranges), host(st.gaussian_ids()), host(st.contrib).astype(np.int64)
        start = np.repeat(np.repeat(rg[:, 0].reshape(r.L.gy, r.L.gx), 16, 0), 16, 1)[:r.H, :r.W]
        last.append(np.where(cont > 0, np.append(ids, -1)[np.where(cont > 0, start + cont - 1, ids.size)], -1))
    assert np.array_equal(last[0], last[1]), (name, "the last contributor of %d pixels changes with the cull" % (last[0] != last[1]).sum())
    # final_tau: bit-identical wherever the culled list of the tile is not empty.  A tile whose culled list IS empty is
    # drawn as a tile without patches, and such a tile's final_tau is 0 on every path (the reference's convention, kept:
    # csrc/egs_draw_device.h empty_tile; nothing reads it there) -- the unculled walk of entries that blend nowhere
    # leaves exactly 1 there
    rg_c = host(st_c.ranges)
    emptied = np.repeat(np.repeat(((rg_c[:, 1] == rg_c[:, 0]) & (r.L.ranges[:, 1] > r.L.ranges[:, 0])).reshape(r.L.gy, r.L.gx), 16, 0), 16, 1)
    emptied = emptied[:r.H, :r.W]
    assert np.array_equal(bits(tau_c[~emptied]), bits(tau_u[~emptied])), (name, "final_tau changes with the cull",
                                                                            first_difference(np.where(emptied, 0, tau_c), np.where(emptied, 0, tau_u), r, st_c))
    assert not tau_c[emptied].any() and (tau_u[emptied] == 1).all() and not img_u[:, emptied].any(), (name, "a tile emptied by the cull")
    # gradients.  What the cull can reach is the draw pass: its twelve-float gradient records per Gaussian obey the
    # default rule column by column, every row; so do dL/dus, dL/dshs and dL/dalphas, every row.  dL/dpws, dL/dscales and
    # dL/drots obey it on the rows whose conic has an eigenvalue ratio kappa below 100; beyond, a row's error, relative
    # to the largest entry of the tensor as in the rule's first clause, is bounded by ``chain_tolerance``.
    kappa = eigen_ratio(r.cinv)
    pixels = 64.0 * np.maximum(np.bincount(r.L.gsid, [F.popcount(m) for m in r.L.must], r.n), 1.0)
    tol = chain_tolerance(kappa, pixels)
    ill = ~(kappa < ILL_RATIO)
    for k in range(12):
        a, b = rec_c[:, k], rec_u[:, k]
        assert np.isfinite(a).all() and np.isfinite(b).all(), (name, "record column", k)
        if np.abs(b).max(initial=0.0) == 0:
            assert not a.any(), (name, "record column", k)
        else:
            assert_grad_close(a, b, (name, "record column %d" % k))
    for a, b, nm in zip(g_c, g_u, ("dpws", "dshs", "dalphas", "dscales", "drots", "dus")):
        a, b = a.reshape(r.n, -1), b.reshape(r.n, -1)
        assert np.isfinite(a).all() and np.isfinite(b).all(), (name, nm)
        chain = nm in ("dpws", "dscales", "drots")
        rows = ~ill if chain else np.ones(r.n, bool)
        if np.abs(b[rows]).max(initial=0.0) == 0:
            assert not a[rows].any(), (name, nm)
        else:
            assert_grad_close(a[rows], b[rows], (name, nm))
        if chain and ill.any():
            err = np.abs(a - b).max(1) / max(np.abs(b).max(), 1e-300)
            ratio = err[ill] / tol[ill]
            j = np.nonzero(ill)[0][int(np.argmax(ratio))]
            print("%s %s: %d rows of kappa >= %g; largest error / bound %.3g at row %d (kappa %.4g, %d pixels, error %.3g of the "
                  "largest entry, bound %.3g)" % (name, nm, ill.sum(), ILL_RATIO, ratio.max(), j, kappa[j], pixels[j], err[j], tol[j]))
            assert (ratio <= 1).all(), (name, nm, "row %d: error %.3g of the largest entry, bound %.3g, kappa %.4g" % (j, err[j], tol[j], kappa[j]))


# ------------------------------------------------------------------------------------------------- seven-op surface
def two_d(r):
    """the materialised 2D Gaussians (+ the hand-written exact-threshold ones of ``faint``) as numpy arrays"""
    d = dict(us=r.us, cinv2ds=r.cinv, alphas=r.alphas, depths=r.depths, colors=r.col, areas=r.areas)
    x = r.case.extra2d
    if x is not None:
        extra = dict(x, colors=np.full((len(x["alphas"]), 3), 0.5, np.float32))
        d = {k: np.concatenate([d[k], extra[k]]) for k in d}
    return d


def splat(gsc, r, d):
    t = lambda a, dt=np.float32: torch.from_numpy(np.ascontiguousarray(a, dt)).to(DEV)
    out, h = gsc.splat_with_records(r.H, r.W, t(d["us"]), t(d["cinv2ds"]), t(d["alphas"]), t(d["depths"]), t(d["colors"]),
                                    t(d["areas"], np.int32))
    torch.cuda.synchronize()
    return [host(o) for o in out], h


@pytest.mark.parametrize("name", CASES)
def test_seven_op_masks_agree_with_the_fused_path(lib, knobs, name):
    fused, gsc = knobs
    fused.CULL_LISTS, gsc.MASKED_LISTS = True, True
    r = device_run(lib, name)
    d = two_d(r)
    out, h = splat(gsc, r, d)
    image, contrib, tau, ranges, gsid = out
    o_ranges, o_gsid, _, _ = O.bin_tiles(d["us"], d["areas"].copy(), d["depths"].copy(), r.W, r.H, O.POLICY_G)
    assert np.array_equal(ranges, o_ranges) and np.array_equal(gsid, o_gsid), name
    assert h is not None and h.lists is not None
    walked = host(h.lists)[:gsid.size]
    assert np.array_equal(walked & GSID_MASK, gsid), name
    m7 = (walked >> 28) & 15
    # the seven-op list is the whole reference list: entry for entry against the two bounds
    L7 = r.L if r.case.extra2d is None else F.reference_lists(d["us"], d["cinv2ds"], d["alphas"], d["areas"], d["depths"], r.W, r.H)
    assert np.array_equal(L7.gsid, gsid) and np.array_equal(plain_ranges(L7), ranges), name
    bad = np.nonzero((L7.must & ~m7) != 0)[0]
    assert bad.size == 0, (name, "a seven-op mask misses a contributing block: mask %d, %s" % (m7[bad[0]] if bad.size else 0, F.describe(L7, bad[0]) if bad.size else ""))
    bad = np.nonzero((m7 & ~L7.may) != 0)[0]
    assert bad.size == 0, (name, "a seven-op mask exceeds `may`: mask %d, %s" % (m7[bad[0]] if bad.size else 0, F.describe(L7, bad[0]) if bad.size else ""))
    assert (m7[np.isin(gsid, np.nonzero(L7.kind == "all")[0])] == 15).all() and not m7[np.isin(gsid, np.nonzero(L7.kind == "never")[0])].any()
    # against the fused path's lists of the same 2D Gaussians (bitmap | tilemap + one tile's slabs | row walk there)
    _, st = fused_forward(r)
    dm = scatter_masks(r.L, *fused_lists(r, st))
    own = gsid < r.n
    assert np.array_equal(gsid[own], r.L.gsid)
    m7o = m7[own]
    both = dm >= 0
    bad = np.nonzero(both & (dm != m7o))[0]
    assert bad.size == 0, (name, "the two surfaces disagree on %d masks; first: fused %d, seven-op %d, %s"
                           % (bad.size, dm[bad[0]] if bad.size else 0, m7o[bad[0]] if bad.size else 0, F.describe(r.L, bad[0]) if bad.size else ""))
    bad = np.nonzero(~both & (m7o != 0))[0]
    assert bad.size == 0, (name, "%d entries with a seven-op mask are missing from the fused list; first: seven-op %d, %s"
                           % (bad.size, m7o[bad[0]] if bad.size else 0, F.describe(r.L, bad[0]) if bad.size else ""))
    if name.startswith("order"):
        out2, h2 = splat(gsc, r, d)
        assert np.array_equal(host(h2.lists)[:gsid.size], walked) and all(np.array_equal(bits(a), bits(b)) for a, b in zip(out, out2)), name
    # masks only skip what the draw kernel would skip itself: every output, bit for bit
    gsc.MASKED_LISTS = False
    plain, _ = splat(gsc, r, d)
    for a, b, nm in zip(out, plain, ("image", "contrib", "final_tau", "ranges", "gsid")):
        assert np.array_equal(bits(a), bits(b)), (name, nm, "changes with MASKED_LISTS",
                                                  int((bits(a) != bits(b)).sum()), int(np.nonzero(bits(a) != bits(b))[0][0]))
