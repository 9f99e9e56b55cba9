"""k_blend_weights (csrc/egs_prune.hip) through ``easygaussiansplatting_amd.importance`` and the pruning
built on it, against the float64 reference of tests/blend_weights_ref.py.

1. One-tile lists (tests/draw_tile_ref.py: five sets x policies gsplatcu / forward_cpu on the 72 x 40 image, lists of
   0 .. 300 entries around the 8-entry groups and 64-entry chunks, ragged right column and bottom row, empty tiles):
   ``gsplatcu.splat``, whose ``contrib`` must equal the reference's on every pixel, then ``importance.splat_weights``:
     * ``hits`` equal the reference on EVERY row; a row whose reference is zero is zero bit for bit in all four words;
       the reserved word is zero everywhere;
     * ``sum`` and ``max`` per row: |got - ref| <= max(floor, 2 x distance) -- ``floor`` the pixel-floor rule of
       tests/draw_tile_ref.py carried over to a row, 2^-23 (2 + position of the row in its list) |ref|; ``distance`` the
       largest distance from float64 of the float32 evaluation, of four float32 evaluations of the inputs moved by one
       ulp, of the float32 evaluations with k_draw's polynomial exponent and of that evaluation with the kernel's two
       one-ulp operations (derived log2 alpha, v_exp_f32) an ulp off (``B.distance`` (a)-(d)).  No row is excluded;
     * two runs are bitwise equal (every Gaussian lies on one tile: one atomic set per row); a second call into the same
       statistics gives exactly 2 sum, 2 hits and the same max; n = 0 gives zero-row tensors and no error.
2. A fused state with culled, masked lists (20 000 Gaussians, 128 x 96): ``from_state`` against the float64 walk of the
   seven ops' 2D tensors over the state's own lists, bounded by the state's contrib; the identity
   sum_g sum[g] = sum_p (1 - final_tau[p]) on the device's own outputs; the block masks exclude no reference hit.
3. Two views accumulate into one ``BlendStats`` as the ``merge_`` of two single-view ones.
4. ``Trainer.prune_by_importance``: what no pixel sees goes, rows and Adam moments are compacted in order bit for bit,
   and the renders do not change by a bit.

Test 1 prints, per tensor, the largest distance | the largest kernel error | the largest error / bound (errors and
distances relative to the row's reference).  Measured on MI355X, largest over the five sets and two policies
(10 tests pass, 0 rows excluded):
                      distance   kernel error   error / bound   error / bound on the shared walk
  sum                 3.9e-05    2.9e-05        0.83            0.83
  max                 5.7e-05    5.7e-05        0.77            0.77
(the last column: the kernel on csrc/egs_list_walk.h, whose four words per row are those of its predecessor bit for bit
on all ten cases; the largest of both on the steepest conics of set values; the median set stands at 0.5).  ``hits`` were the reference's
on every row and two runs bitwise equal on every set.  Without part (d) of the distance two rows of lengths0 / gsplatcu
stood at 1.25 x their bound (tile 12, entry 0: 6.7 float32 ulps on a sum of 128 weights); with it that set is at 0.50.
Test 2 on MI355X: P = 11 753 after culling, 6 890 rows hit, 120 with a near pixel (1.74 %); sum 9.3e-7 of its largest
entry (median 6.0e-7), max 7.5e-6 (median 9.9e-7).
"""
import numpy as np
import pytest

from tests import blend_weights_ref as B
from tests import draw_tile_ref as D

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture
def gpu():
    """the policy, the segment switch and the splat memo put back afterwards (as tests/test_gpu_draw_tiles.py does)"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from easygaussiansplatting_amd import fused, gsplatcu, importance
    gsplatcu.set_policy("gsplatcu")
    keep = fused.SEGMENTS
    yield gsplatcu, fused, importance
    fused.SEGMENTS = keep
    gsplatcu.set_policy("gsplatcu")
    gsplatcu.clear_memo()


def _t(a):
    return torch.from_numpy(np.array(a)).cuda()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _host(t):
    return t.detach().cpu().numpy()


def _words(st):
    return _host(st.rows.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------------ 1. one-tile lists
@pytest.mark.parametrize("pname", list(D.POLICIES))
@pytest.mark.parametrize("name", D.SETS)
def test_one_tile_lists(gpu, name, pname):
    gsc, fused, imp = gpu
    c = D.case(name)
    a = c.arrays
    ref, dist, floor = B.reference(name, pname), B.distance(name, pname), B.row_floor(name, pname)
    assert dist["hits_equal"]
    gsc.set_policy(pname)
    fused.SEGMENTS = "0"
    us, cinv, alphas, colors = (_t(a[k]) for k in ("us", "cinv2ds", "alphas", "colors"))

    def once(stats=None):
        depths, areas = _t(a["depths"]), _t(a["areas"])
        image, contrib, tau, ranges, gsid = gsc.splat(D.H, D.W, us, cinv, alphas, depths, colors, areas)
        assert np.array_equal(_host(contrib), D.reference(name, pname)["contrib"]), (name, pname, "contrib")
        st = imp.splat_weights(D.H, D.W, us, cinv, alphas, depths, contrib, ranges, gsid,
                               areas=areas if pname == "forward_cpu" else None, stats=stats)
        torch.cuda.synchronize()
        return st

    st = once()
    words = _words(st)
    assert st.views == 1 and words.shape == (c.n, 4)
    hits = _host(st.hits)
    wrong = np.nonzero(hits != ref["hits"])[0]
    assert wrong.size == 0, (name, pname, "hits differ on %d rows, first: Gaussian %d (tile %d, entry %d): got %d, "
                             "reference %d" % (wrong.size, wrong[0], c.tile_of[wrong[0]], c.pos_of[wrong[0]],
                                               hits[wrong[0]], ref["hits"][wrong[0]]))
    assert not words[:, 3].any(), "the reserved word"
    zero = ref["hits"] == 0
    assert not words[zero].any(), (name, pname, "rows with a zero reference are not zero bit for bit")
    lines = []
    for key, got in (("sum", _host(st.sum)), ("max", _host(st.max))):
        assert np.isfinite(got).all()
        want = ref[key]
        err = np.abs(got.astype(np.float64) - want)
        bound = np.maximum(floor[key], 2 * dist[key])
        ratio = np.where(err == 0, 0.0, err / np.where(bound == 0, 1e-300, bound))
        nz = want > 0
        rel = lambda v: float((v[nz] / want[nz]).max()) if nz.any() else 0.0
        lines.append("%-5s %-12s %-8s distance %.2g | error %.2g | error / bound %.2f"
                     % (name, pname, key, rel(dist[key]), rel(err), float(ratio.max())))
        g = int(np.argmax(ratio))
        print(lines[-1])
        assert ratio.max() <= 1, (name, pname, key, "%d rows beyond their bound; worst: Gaussian %d = tile %d, entry %d: "
                                  "got %.9g, reference %.9g, error %.3g, bound %.3g (floor %.3g, distance %.3g)"
                                  % (int((ratio > 1).sum()), g, c.tile_of[g], c.pos_of[g], got[g], want[g], err[g],
                                     bound[g], floor[key][g], dist[key][g]))
    # two runs are bitwise equal: every Gaussian lies on one tile
    again = once()
    assert np.array_equal(_words(again), words)
    # a second call into the same statistics: exactly twice the sum and the hits, the same max
    once(again)
    twice = _words(again)
    assert again.views == 2
    assert np.array_equal(_host(again.sum), 2 * _host(st.sum)) and np.array_equal(_host(again.hits), 2 * hits)
    assert np.array_equal(twice[:, 1], words[:, 1]) and not twice[:, 3].any()


def test_no_gaussians(gpu):
    gsc, fused, imp = gpu
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device="cuda")
    st = imp.splat_weights(40, 72, z(0, 2), z(0, 3), z(0), z(0), z(40, 72, dt=torch.int32), z(15, 2, dt=torch.int32),
                           z(0, dt=torch.int32))
    torch.cuda.synchronize()
    assert tuple(st.rows.shape) == (0, 4) and tuple(st.sum.shape) == (0,) and tuple(st.hits.shape) == (0,)
    assert st.hits.dtype == torch.int32


# ------------------------------------------------------------------------------------- 2. fused state, culled masked lists
def _tensors(sc):
    return tuple(_dev(x) for x in (sc.pws, sc.shs, sc.alphas, sc.scales, sc.rots))


def test_fused_state_culled_lists(gpu):
    gsc, fused, imp = gpu
    from easygaussiansplatting_amd import scene as S
    from easygaussiansplatting_amd.function import Camera
    from oracle import gs_oracle as O
    sc = S.small_scene(20000, 128, 96, 48)
    cam = sc.cam
    W, H = cam.width, cam.height
    pws, shs, alphas, scales, rots = _tensors(sc)
    fused.SEGMENTS = "0"
    image, mask, state = fused.forward(pws, shs, alphas, scales, rots, Camera.from_scene(cam, "cuda"), need_grad=False)
    st = imp.from_state(state)
    torch.cuda.synchronize()
    assert state.culled and st.views == 1
    # the 2D tensors of the seven ops, as __graft_entry__.smoke forms them
    Rcw, tcw = _dev(cam.Rcw), _dev(cam.tcw)
    us, pcs, depths, _ = gsc.project(pws, Rcw, tcw, cam.fx, cam.fy, cam.cx, cam.cy, True)
    cov3 = gsc.computeCov3D(rots, scales, depths, True)[0]
    cov2 = gsc.computeCov2D(cov3, pcs, Rcw, depths, cam.fx, cam.fy, W, H, True)[0]
    cinv, areas = gsc.inverseCov2D(cov2, depths, True)[:2]
    torch.cuda.synchronize()
    ranges, gsid = _host(state.ranges), _host(state.gaussian_ids())
    contrib, tau = _host(state.contrib), _host(state.final_tau)
    blocks = []
    rsum, rmax, rhits, near, _ = B.image_stats(W, H, ranges, gsid, _host(us), _host(cinv), _host(alphas), None, contrib,
                                               O.POLICY_G, blocks_out=blocks)
    # a condition on the inputs, on the reference alone: few rows have a pixel next to the skip threshold
    n_hit, n_near = int((rhits > 0).sum()), int(((near > 0) & (rhits > 0)).sum())
    print("P = %d, %d rows hit, %d of them with a near pixel (%.2f %%)" % (len(gsid), n_hit, n_near, 100.0 * n_near / n_hit))
    assert n_hit > 5000 and int((near > 0).sum()) <= 0.02 * n_hit
    hits = _host(st.hits).astype(np.int64)
    bad = np.nonzero(np.abs(hits - rhits) > near)[0]
    assert bad.size == 0, ("hits beyond the near-pixel count on %d rows, first: Gaussian %d got %d, reference %d, near %d"
                           % (bad.size, bad[0], hits[bad[0]], rhits[bad[0]], near[bad[0]]))
    assert not _words(st)[:, 3].any()
    for key, got, want in (("sum", _host(st.sum), rsum), ("max", _host(st.max), rmax)):
        # the rule of tests/gradcheck.py: 2e-4 of the tensor's largest entry, median 1e-4 on entries >= 1 % of it
        top = np.abs(want).max()
        err = np.abs(got.astype(np.float64) - want)
        big = np.abs(want) >= 1e-2 * top
        med = float(np.median(err[big] / np.abs(want[big])))
        print("%-4s largest error %.3g of the largest entry, median relative error %.3g on %d rows"
              % (key, err.max() / top, med, int(big.sum())))
        assert top > 0 and err.max() <= 2e-4 * top, (key, err.max() / top)
        assert med <= 1e-4, (key, med)
    # sum_g sum[g] = sum_p (1 - final_tau[p]) over the non-empty tiles, on the device's own outputs
    gx = (W + 15) // 16
    rhs = 0.0
    for t in range(len(ranges)):
        if ranges[t, 1] > ranges[t, 0]:
            ty, tx = divmod(t, gx)
            rhs += (1.0 - tau[16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16].astype(np.float64)).sum()
    lhs = float(_host(st.sum).astype(np.float64).sum())
    assert rhs > 0 and abs(lhs - rhs) <= 2e-4 * rhs, (lhs, rhs)
    # the block masks never exclude a reference hit
    masks = _host(state.block_masks())
    want_blocks = np.zeros(len(gsid), np.int64)
    for t in range(len(ranges)):
        if ranges[t, 1] > ranges[t, 0]:
            want_blocks[ranges[t, 0]:ranges[t, 1]] = blocks[t]
    assert want_blocks.any() and not (want_blocks & ~masks.astype(np.int64)).any()


# ------------------------------------------------------------------------------------------------- 3. two views accumulate
def test_two_views_accumulate(gpu):
    gsc, fused, imp = gpu
    from easygaussiansplatting_amd import scene as S
    from easygaussiansplatting_amd.function import Camera
    sc = S.small_scene(20000, 128, 96, 48)
    cams = [Camera.from_scene(c, "cuda") for c in S.ring_cameras(sc.cam, 2, radius=5.0)]
    P = _tensors(sc)
    fused.SEGMENTS = "0"
    both = imp.BlendStats(sc.n, "cuda")
    for cam in cams:
        assert imp.render_weights(both, *P, cam) is both
    singles = [imp.render_weights(None, *P, cam) for cam in cams]
    torch.cuda.synchronize()
    assert both.views == 2 and all(s.views == 1 for s in singles)
    assert int((singles[0].hits > 0).sum()) > 1000 and int((singles[1].hits > 0).sum()) > 1000
    assert not torch.equal(singles[0].hits, singles[1].hits)
    merged = singles[0].merge_(singles[1])
    assert merged.views == 2
    assert np.array_equal(_words(both)[:, 1:], _words(merged)[:, 1:])       # max, hits, reserved: bit-equal
    top = float(merged.sum.max())
    assert top > 0 and float((both.sum - merged.sum).abs().max()) <= 2e-4 * top


# ------------------------------------------------------------------------------------------- 4. pruning keeps what is seen
def _trainer(n=5000):
    from easygaussiansplatting_amd import scene as S
    from easygaussiansplatting_amd.function import Camera
    from easygaussiansplatting_amd.trainer import Trainer
    sc = S.small_scene(n, 128, 96, 48)
    cams = [Camera.from_scene(c, "cuda") for c in S.ring_cameras(sc.cam, 2, radius=5.0)]
    gts = [_dev(S.uniform01(40 + i, 1, (3, 96, 128))) for i in range(2)]
    return Trainer(sc, cams, gts, max_steps=100, scene_size=4.0, fused_adam=True, strategy="default")


def _render(tr, fused):
    p = tr.params
    with torch.no_grad():
        out = [fused.forward(p["pws"], p["low_shs"], p["alphas_raw"], p["scales_raw"], p["rots_raw"], cam,
                             high_shs=p["high_shs"], need_grad=False, antialiased=tr.antialiased)[0].clone()
               for cam in tr.cams]
    torch.cuda.synchronize()
    return out


def _rows_of(tr):
    """every parameter tensor and both moments of every group, by name"""
    out = {}
    for g in tr.opt.param_groups:
        p = g["params"][0]
        assert p is tr.params[g["name"]]
        s = tr.opt.state[p]
        out[g["name"]] = (p.detach().clone(), s["exp_avg"].clone(), s["exp_avg_sq"].clone())
    return out


def test_pruning_keeps_what_is_seen(gpu):
    gsc, fused, imp = gpu
    fused.SEGMENTS = "0"
    tr = _trainer()
    for _ in range(2):
        assert np.isfinite(tr.step([0, 1]))
    n = tr.params["pws"].shape[0]
    st = tr.importance()
    assert st.views == 2 and st.n == n
    images = _render(tr, fused)
    old = _rows_of(tr)
    keep = st.hits >= 1
    report = tr.prune_by_importance(score="hits", threshold=1)
    assert report["pruned"] == int((st.hits < 1).sum()) > 0
    assert report["total"] == n - report["pruned"] == tr.params["pws"].shape[0]
    new = _rows_of(tr)
    assert set(new) == set(old) and len(new) == 6
    for k in old:
        for a, b, what in zip(old[k], new[k], ("parameter", "exp_avg", "exp_avg_sq")):
            assert b.shape[0] == report["total"] and b.is_contiguous()
            assert torch.equal(a[keep].view(torch.int32), b.view(torch.int32)), (k, what)
    assert new["pws"][1].abs().max() > 0 and new["pws"][2].abs().max() > 0      # the moments exist: two steps were taken
    assert tr.grad_accum.shape[0] == report["total"] and tr.vis_count.shape[0] == report["total"]
    assert not tr.grad_accum.any() and not tr.vis_count.any()
    # removing entries that hit no pixel changes no blend
    for a, b in zip(images, _render(tr, fused)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert np.isfinite(tr.step([0, 1]))
    assert int(tr.importance().hits.min()) >= 1


def test_pruning_a_fraction_by_max(gpu):
    gsc, fused, imp = gpu
    fused.SEGMENTS = "0"
    tr = _trainer()
    n = tr.params["pws"].shape[0]
    st = tr.importance()
    keep = imp.keep_mask(st, "max", fraction=0.25)
    report = tr.prune_by_importance(score="max", fraction=0.25)
    assert report["total"] == n - (n // 4) == tr.params["pws"].shape[0] and report["pruned"] == n // 4
    assert int(keep.sum()) == report["total"]
    assert float(st.max[keep].min()) >= float(st.max[~keep].max())        # no kept row below a dropped one
    with pytest.raises(ValueError):
        tr.density.prune(tr.params, tr.opt, torch.zeros(report["total"], dtype=torch.bool, device="cuda"))
    assert tr.params["pws"].shape[0] == report["total"]
