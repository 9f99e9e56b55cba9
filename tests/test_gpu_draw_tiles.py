"""k_draw / k_draw_bwd (csrc/egs_draw.hip) and the segment kernels that share their bodies -- k_draw_seg walks its entries
with k_draw's own blend loop (blend_range, csrc/egs_draw_device.h), the segment backward is k_draw_bwd<SEG> -- on
HAND-BUILT one-tile lists (tests/draw_tile_ref.py): chosen list lengths (0 .. 300 around the 8-entry groups and the 64-entry chunks), chosen stop
positions per 8x8 block, chosen runs of entries that reach a block and hit nothing, clamped / floored / steepest /
500 px conics, ragged tiles -- against the float64 oracle, tightly:

  * ``patch_range_per_tile`` / ``gsid_per_patch`` equal the intended lists, ``contrib`` equals the reference on EVERY pixel
    (no flips: the builder keeps every decision of the blend clear of its threshold), empty tiles are 0 / 0 / 0;
  * image and final_tau, per pixel: |got - ref| <= max(floor, 2 x distance), ``distance`` the largest distance from the
    float64 reference of the float32 oracle, of four float32 evaluations of the inputs moved by one ulp and of the
    float32 evaluations with k_draw's polynomial exponent (``D.distances`` (a)-(c)); ``floor`` one float32 ulp per
    blended entry, 2^-23 (2 + contrib) max(1, max |colour|);
  * the four gradient tensors, per Gaussian ROW (the rule of tests/test_gpu_pergaussian_matrix.py): the row's error
    relative to max_j |ref row| is at most max(FLOOR max(1, walked / 100), 2 x distance of the row); FLOOR = 1e-5 stands
    for a chain of ~100 float32 operations, and this kernel recovers the transmittance by one division per walked
    entry (``walked``: entries between the row's own and the tile's largest contrib);
  * rows whose reference is zero (never hit, behind every stop, alpha < skip, zero dL/dgamma block) are zero bit for bit;
  * two runs of a path give bitwise equal gradients (one atomic set per Gaussian; an entry belongs to one segment);
  * the backward pass ALONE -- ``splatB`` fed the oracle's float64 contrib / final_tau (rounded to float32) and the
    oracle's lists -- is held to the same reference by the same rule and the same bound; its error against the distance
    of k_draw_bwd by itself, (a), (b), (d) below, is printed beside it.
No pixel and no row is excluded anywhere.  ``test_unsplit_tiles_see_one_loop``: on the tiles of at most 64 entries (DIRECT
items of the segment path) image, contrib and final_tau of ``seg-records-spec0`` equal those of ``records`` bit for bit.

Paths: the seven-op pair with masked lists (default) and with plain lists + the per-entry box test, the records handle,
policy forward_cpu (BOX instances, no skip, no stop), the segment path (segments of 64, every list above 64 split) with
and without speculation through the public pair (states rebuilt from contrib / states kept) and the handle.

What the distance of a gradient row is made of (``D.distances``; every part restates in float32, operation by operation,
something the kernels do, and is evaluated on the reference alone):
  (a), (b) the float32 oracle on the inputs as given and one ulp away.  By themselves they are exceeded on MI355X, up to
      2.35 x: cancelling dL/dalpha rows 120 entries in front of their tile's last contributor (192-entry list);
  (d) k_draw_bwd recovers tau by tau * v_rcp_f32(1 - alpha') and takes the Gaussian from v_exp_f32, one-ulp instructions
      where NumPy rounds correctly: one ulp per use, same sign at every use or random (``D.backward_hw``, which also
      forms the Gaussian from the pre-scaled conic with the kernel's fmaf and carries gamma_cur2last as its scalar lq);
  (e) fed its OWN forward, the backward divides its way up from a final_tau that belongs to k_draw's alpha': the
      polynomial about the tile centre on a log2(alpha) DERIVED from the record's threshold (lskip - log2f(alpha_skip /
      alpha): a difference of two numbers near 9 for alpha ~ 1, good to one ulp of 9, 1e-6), against the direct form of
      k_draw_bwd.  1 / (1 - alpha') magnifies the difference up to 100-fold: rows in front of a nearly opaque entry (the
      opacity-1 walls, the 0.995 / 1.0 clamp entries) carry up to 9e-5.  A property of the kernel pair, not of its list
      walking, and modelled, not fixed: the backward (d) fed the polynomial forward, whose derived logarithm and
      exponential are moved by their ulp, forward and backward signs opposed.  (a), (b), (d), (e) bound the pair.

Each test prints, per tensor, the largest distance | the largest kernel error | the largest error / bound.
Measured on MI355X, largest over the five sets and nine paths (45 tests pass, 0 pixels and 0 rows excluded):
                      distance   kernel error   error / bound
  image               7.4e-06    6.9e-06        0.85
  final_tau           9.3e-06    8.6e-06        0.74
  dus                 0.0057     0.0014         0.56      backward alone  0.00073  0.45   (against (a), (b), (d) only: 0.92)
  dcinv2ds            0.00027    6.7e-05        0.46      backward alone  2e-05  0.35   (against (a), (b), (d) only: 0.76)
  dalphas             0.025      0.0049         0.61      backward alone  0.0068  0.64   (against (a), (b), (d) only: 1.27)
  dcolors             0.00016    5.6e-05        0.49      backward alone  1.1e-05  0.28   (against (a), (b), (d) only: 0.71)
(the large distances and errors belong to single cancelling rows, which is what the row-aware bound is for; the median
row distance is 3e-6 .. 1.3e-5).  The largest image error, 6.8e-6 on the corner pixel of a steepest conic (set values,
tile 9, entry 2, pixel y 31, x 65), is 3.4 x the distance of the polynomial restated with NumPy's two roundings per step
(9.9e-7) and exactly the distance of the restatement with the kernel's fmaf.  Against (a), (b), (d) alone the backward
pass stands at up to 1.3 x on 1..5 cancelling dL/dalpha rows of the stops set (tile 4, entry 4, in front of the 0.95 /
0.95 / 0.99 entries): five sampled ulp patterns do not bound one particular pattern of a cancelling row within 2 x, and
the segment paths rebuild their states by a forward walk, so (e) applies to them.  contrib and both lists were exact on
every path; two runs of every path were bitwise equal.

Open gaps.  Tried on scratch builds of k_draw_bwd (lengths and stops sets; default, forward_cpu and segment paths):
``c_first = maxcont >> 6`` and ``idx > bmax[k]`` change no result, so no test can fail for them: the extra chunk holds only
entries >= bmax, which the reach mask drops, and an entry at index bmax[k] fails ``i < cont[k]`` on every pixel -- both
cuts are redundant with the per-pixel test.  ``idx >= bmax[k] - 1``, which drops each block's last contributor, fails
every one of those tests with hundreds of rows at error 1.  The empty-slot guard (``je[e] = -1``) is NOT demonstrated:
without it an empty slot addresses the gradient record of whatever id the staging buffer last held, so that build was
not run; the lists here end chunks with 1..3 empty slots (lengths 1, 2, 3, 5, 7, 9, 65, 129, 193), which pins that the
guard's presence is harmless, not that its absence is caught.
"""
import collections
import ctypes as C

import numpy as np
import pytest

from tests import draw_tile_ref as D

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FLOOR = 1e-5
PATHS = {
    "default": dict(),
    "plain-lists": dict(masked=False),
    "records": dict(handle=True),
    "forward_cpu": dict(policy="forward_cpu"),
    "seg-rebuild-spec0": dict(seg=True, spec="0", pair=False),
    "seg-rebuild-spec1": dict(seg=True, spec="1", pair=False),
    "seg-kept-spec1": dict(seg=True, spec="1", pair="content"),
    "seg-records-spec0": dict(seg=True, spec="0", handle=True),
    "seg-records-spec1": dict(seg=True, spec="1", handle=True),
}


@pytest.fixture
def gpu(monkeypatch):
    """the library with every knob this file turns put back afterwards (as tests/test_gpu_segments.py's fixture does)"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from easygaussiansplatting_amd import _lib, fused, gsplatcu
    gsplatcu.set_policy("gsplatcu")
    lib = _lib.load()
    before = (C.c_int * 2)()
    _lib.check(lib.egs_seg_config(0, 0, before))
    keep = fused.SEGMENTS, fused.SEG_SPECULATE
    pair = gsplatcu.set_pair_states("content")
    yield gsplatcu, fused, lib, monkeypatch
    fused.SEGMENTS, fused.SEG_SPECULATE = keep
    _lib.check(lib.egs_seg_config(before[0], before[1], None))
    gsplatcu.set_pair_states(pair)
    gsplatcu.set_policy("gsplatcu")
    gsplatcu.clear_memo()


def _t(a):
    return torch.from_numpy(np.array(a)).cuda()


def _host(ts):
    return [t.detach().cpu().numpy() for t in ts]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.int32)


def _configure(gpu, path):
    """the library's knobs as ``path`` wants them -> (its options, its policy name)"""
    gsc, fused, lib, monkeypatch = gpu
    from easygaussiansplatting_amd import _lib
    opt = PATHS[path]
    pname = opt.get("policy", "gsplatcu")
    gsc.set_policy(pname)
    monkeypatch.setattr(gsc, "MASKED_LISTS", opt.get("masked", True))
    fused.SEGMENTS = "1" if opt.get("seg") else "0"
    if opt.get("seg"):
        _lib.check(lib.egs_seg_config(64, 64, None))
        fused.SEG_SPECULATE = opt["spec"]
        gsc.set_pair_states(opt.get("pair", "content"))
    return opt, pname


def run_path(gpu, name, path):
    """one forward + backward of set ``name`` through ``path``, twice, and the backward alone where the path takes
    tensors -> dict(fwd: image, contrib, final_tau, ranges, gsid; grads, grads_again, alone (or None), policy)"""
    gsc = gpu[0]
    opt, pname = _configure(gpu, path)
    c = D.case(name)
    a = c.arrays
    us, cinv, alphas, colors, dl = (_t(a[k]) for k in ("us", "cinv2ds", "alphas", "colors", "dloss_dgammas"))
    out = dict(policy=pname)

    def once():
        depths, areas = _t(a["depths"]), _t(a["areas"])
        if opt.get("handle"):
            fwd, h = gsc.splat_with_records(D.H, D.W, us, cinv, alphas, depths, colors, areas)
            assert h is not None
        else:
            fwd, h = gsc.splat(D.H, D.W, us, cinv, alphas, depths, colors, areas), None
        g = gsc.splatB(D.H, D.W, us, cinv, alphas, depths, colors, fwd[1], fwd[2], fwd[3], fwd[4], dl,
                       areas=areas if pname == "forward_cpu" else None, records=h)
        info = gsc.last_splatB_info()
        torch.cuda.synchronize()
        return _host(fwd), _host(g), info

    out["fwd"], out["grads"], info = once()
    _, out["grads_again"], _ = once()
    if opt.get("seg"):
        assert info["segments"], info
        if not opt.get("handle"):
            assert info["rebuilt"] == (opt["pair"] is False) and info["kept_states"] == (opt["pair"] == "content"), info
    out["alone"] = None
    if not opt.get("handle") and opt.get("pair") != "content":
        ref = D.reference(name, pname)
        _, rg, gs = D.lists(c, pname)
        g = gsc.splatB(D.H, D.W, us, cinv, alphas, _t(a["depths"]), colors, _t(ref["contrib"]),
                       _t(ref["final_tau"].astype(np.float32)), _t(rg), _t(gs), dl,
                       areas=_t(a["areas"]) if pname == "forward_cpu" else None)
        torch.cuda.synchronize()
        out["alone"] = _host(g)
    return out


def check_forward(name, pname, fwd, stats):
    c = D.case(name)
    ref, dist = D.reference(name, pname), D.distances(name, pname)
    image, contrib, tau, ranges, gsid = fwd
    ls, rg, gs = D.lists(c, pname)
    assert np.array_equal(ranges, rg) and np.array_equal(gsid, gs), (name, "the lists are not the intended ones")
    wrong = np.argwhere(contrib != ref["contrib"])
    assert wrong.size == 0, (name, "contrib differs on %d pixels, first (y, x) %s: got %d, reference %d" % (
        len(wrong), wrong[0], contrib[tuple(wrong[0])], ref["contrib"][tuple(wrong[0])]))
    floor = D.pixel_floor(name, pname)
    for key, got, want in (("image", image, ref["image"]), ("final_tau", tau[None], ref["final_tau"][None])):
        assert np.isfinite(got).all()
        err = np.abs(got.astype(np.float64) - want).max(0)
        bound = np.maximum(floor, 2 * dist[key])
        ratio = err / bound
        stats[key] = (float(dist[key].max()), float(err.max()), float(ratio.max()))
        y, x = np.unravel_index(np.argmax(ratio), ratio.shape)
        assert ratio.max() <= 1, (name, key, "pixel (y %d, x %d) of tile %d: error %.3g, bound %.3g (distance %.3g), "
                                  "contrib %d" % (y, x, (y // 16) * D.GX + x // 16, err[y, x], bound[y, x],
                                                  dist[key][y, x], contrib[y, x]))
    for t, l in enumerate(ls):          # empty tiles: image 0, contrib 0, final_tau 0
        if len(l) == 0:
            tx, ty, x0, y0, ww, hh = D.geom(t)
            assert not image[:, y0:y0 + hh, x0:x0 + ww].any() and not contrib[y0:y0 + hh, x0:x0 + ww].any() \
                and not tau[y0:y0 + hh, x0:x0 + ww].any(), (name, t)


def check_grads(name, pname, grads, label, stats, alone=False):
    c = D.case(name)
    ref, dist = D.reference(name, pname), D.distances(name, pname)
    floor = FLOOR * np.maximum(1.0, ref["walked"] / 100.0)
    for key, got in zip(D.GRADS, grads):
        want = np.asarray(ref[key], np.float64).reshape(c.n, -1)
        got = got.reshape(c.n, -1)
        assert np.isfinite(got).all(), (name, label, key)
        zero = ~want.any(1)
        nz = np.nonzero(_bits(got).reshape(c.n, -1)[zero].any(1))[0]
        assert nz.size == 0, (name, label, key, "%d rows with a zero reference are not zero bit for bit, first: Gaussian "
                              "%d (tile %d, entry %d)" % (nz.size, np.nonzero(zero)[0][nz[0]],
                                                          c.tile_of[np.nonzero(zero)[0][nz[0]]],
                                                          c.pos_of[np.nonzero(zero)[0][nz[0]]]))
        rel = D._rows(got, want)
        dk = dist[key]
        bound = np.maximum(floor, 2 * dk)
        ratio = rel / bound
        g = int(np.argmax(ratio))
        if alone:       # printed, not asserted: against the distance of k_draw_bwd by itself, (a), (b), (d)
            stats[key + " vs (a)(b)(d)"] = (float(dist[key + "_alone"].max()), float(rel.max()),
                                            float((rel / np.maximum(floor, 2 * dist[key + "_alone"])).max()))
        old = stats.get(key, (0.0, 0.0, 0.0))
        stats[key] = (float(dk.max()), max(old[1], float(rel.max())), max(old[2], float(ratio.max())))
        assert ratio.max() <= 1, (name, label, key, "%d rows beyond their bound; worst: Gaussian %d = tile %d, entry %d of "
                                  "%d of the policy-G list (walked %d): error %.3g, bound %.3g (distance %.3g)" % (
                                      int((ratio > 1).sum()), g, c.tile_of[g], c.pos_of[g],
                                      len(c.lists[c.tile_of[g]]), ref["walked"][g], rel[g], bound[g],
                                      dk[g]), got[g].tolist(), want[g].tolist())


def _report(name, path, stats):
    print("\n%s / %s  per tensor: largest float32 distance | largest kernel error | largest error / bound" % (name, path))
    for k, v in stats.items():
        print("  %-18s %.3g | %.3g | %.3g" % ((k,) + v))


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", D.SETS)
def test_one_tile_lists(gpu, name, path):
    out = run_path(gpu, name, path)
    stats = collections.OrderedDict()
    failed = []

    def step(f, *args):     # every comparison runs and reports, the first failure is raised at the end
        try:
            f(*args)
        except AssertionError as e:
            failed.append(e)

    step(check_forward, name, out["policy"], out["fwd"], stats)
    step(check_grads, name, out["policy"], out["grads"], "own forward", stats)
    if out["alone"] is not None:
        alone = collections.OrderedDict()
        step(check_grads, name, out["policy"], out["alone"], "backward alone", alone, True)
        stats.update({k + " (alone)": v for k, v in alone.items()})
    _report(name, path, stats)
    for a, b, k in zip(out["grads"], out["grads_again"], D.GRADS):
        assert np.array_equal(_bits(a), _bits(b)), (name, path, k, "two runs differ")
    if failed:
        raise failed[0]


@pytest.mark.parametrize("name", D.SETS)
def test_unsplit_tiles_see_one_loop(gpu, name):
    """A tile of at most 64 entries is a DIRECT item of the segment path (segment length 64, split minimum 64): k_draw_seg
    walks it with the loop k_draw walks it with, so image, contrib and final_tau of ``seg-records-spec0`` equal those of
    ``records`` bit for bit on every pixel of such a tile."""
    gsc = gpu[0]
    c = D.case(name)
    a = c.arrays
    fwd = {}
    for path in ("records", "seg-records-spec0"):
        _configure(gpu, path)
        out, h = gsc.splat_with_records(D.H, D.W, *(_t(a[k]) for k in ("us", "cinv2ds", "alphas", "depths", "colors",
                                                                        "areas")))
        assert h is not None
        torch.cuda.synchronize()
        fwd[path] = _host(out[:3])
    ls = D.lists(c, "gsplatcu")[0]
    short = [t for t, l in enumerate(ls) if len(l) <= 64]
    assert any(len(ls[t]) > 0 for t in short), (name, "no unsplit tile with entries")
    for t in short:
        tx, ty, x0, y0, ww, hh = D.geom(t)
        for key, one, seg in zip(("image", "contrib", "final_tau"), fwd["records"], fwd["seg-records-spec0"]):
            one, seg = one[..., y0:y0 + hh, x0:x0 + ww], seg[..., y0:y0 + hh, x0:x0 + ww]
            diff = np.argwhere(one.view(np.int32) != seg.view(np.int32))
            assert diff.size == 0, (name, key, "tile %d (%d entries): %d words differ, first at %s: %r against %r" % (
                t, len(ls[t]), len(diff), diff[0], one[tuple(diff[0])], seg[tuple(diff[0])]))
