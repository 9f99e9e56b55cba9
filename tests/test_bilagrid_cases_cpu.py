"""tests/bilagrid_cases.py on the host: the hand-built cases reach every form of a wave of k_slice_bwd, the census agrees
with the library's own host functions, the float64 evaluation of the restatement is the grid_sample reference, and the T
table of the bounds is what the restatement's own evaluations ask for.  No GPU and no kernel is involved."""
import collections

import numpy as np
import pytest

from easygaussiansplatting_amd import appearance
from tests import bilagrid_cases as BC
from tests import bilagrid_ref as R


def census_of(name):
    H, W, shape = BC.shape_of(name)
    return BC.census(H, W, shape, BC.inputs(name)["image"].numpy())


def of_set(which):
    """class -> waves, summed over the cases of one set; and the cases"""
    total = collections.Counter()
    names = [n for n, c in BC.CASES.items() if c[0] == which]
    for n in names:
        total.update(census_of(n)["counts"])
    return total, names


def test_every_class_is_reached_by_its_set():
    uni, _ = of_set("uniform")
    for k in ("uniform_full_interior", "uniform_full_clamped", "uniform_dead_interior", "uniform_dead_clamped",
              "mixed_full", "mixed_dead"):
        assert uni[k] > 0, k
    mat, _ = of_set("matrix")
    for k in ("mat_flush+", "mat_flush0", "mat_dead", "wave_without_rows"):
        assert mat[k] > 0, k
    glo, _ = of_set("global")
    assert glo["global_full"] > 0 and glo["global_dead"] > 0
    # the forms the table names, case by case
    want = {"uniform-L2": "lds", "uniform-L5": "lds", "uniform-L12": "lds", "matrix-nx1": "matrix",
            "matrix-L1": "matrix", "matrix-3rows": "matrix", "matrix-box8064": "matrix", "global": "global",
            "cap-x-lds": "lds", "cap-y-matrix": "matrix", "cap-x-global": "global"}
    assert {n: census_of(n)["form"] for n in BC.CASES} == want
    assert census_of("matrix-3rows")["counts"]["wave_without_rows"] == 2
    assert census_of("matrix-L1")["counts"]["wave_without_rows"] == 4
    assert census_of("cap-y-matrix")["counts"]["mat_flush+"] == 4 * 256           # 256 blocks in y
    # a striped image has pixels on both sides of (0, 1)
    for n, c in BC.CASES.items():
        if c[4] == "striped":
            luma = BC.luma32(BC.inputs(n)["image"].numpy())
            assert (luma < 0).any() and (luma > 1).any(), n


@pytest.mark.parametrize("name,L", [("uniform-L5", 5), ("uniform-L12", 12)])
def test_interior_uniform_waves_with_many_layers(name, L):
    assert BC.shape_of(name)[2][2] == L
    c = census_of(name)["counts"]
    assert c["uniform_full_interior"] > 0 and c["uniform_dead_interior"] > 0
    # .. and they lie in more than one layer, so both adds of the uniform form land on changing nodes
    H, W, shape = BC.shape_of(name)
    z0, _ = BC.layer_of(BC.luma32(BC.inputs(name)["image"].numpy()), L)
    rows = [y for (y, bx), k in census_of(name)["rows"].items() if k == "uniform_full_interior"]
    assert len({int(z0[y, 0]) for y in rows}) >= min(L - 1, 3)


def test_census_agrees_with_the_library_host_functions():
    shapes = [BC.shape_of(n) for n in BC.CASES] + list(R.CASES)
    for H, W, shape in shapes:
        image = np.zeros((3, H, W), np.float32)
        c = BC.census(H, W, shape, image)
        assert c["form"] == appearance.dgrid_form(H, W, shape), (H, W, shape)
        assert (c["form"] == "global") == (appearance.slice_path(H, W, shape) == "global")
        assert c["box"] == appearance.largest_box(H, W, shape)
        assert BC.box_extent(H, W, shape) == appearance._box_extent(H, W, shape)


def test_the_largest_lds_request():
    H, W, shape = BC.shape_of("matrix-box8064")
    assert appearance.largest_box(H, W, shape) == 8064
    # both boxes and the matrix form's scratch of four waves x 64 lanes x (12 + 4 + 1) floats
    assert BC.lds_bytes(H, W, shape) == 4 * (2 * 8064 + 4 * 64 * 17) == 81920
    assert BC.lds_bytes(H, W, shape, dimage=False) == 4 * (8064 + 4 * 64 * 17)
    assert BC.lds_bytes(H, W, shape, dgrid=False) == 4 * 8064
    assert max(census_of(n)["lds_bytes"] for n in BC.CASES) == 81920
    assert BC.LDS_FLOATS == appearance._bilagridlib.LDS_FLOATS
    assert (BC.BW, BC.BH) == (appearance._bilagridlib.BLOCK_W, appearance._bilagridlib.BLOCK_H)


def test_the_caps():
    m = appearance._bilagridlib.MAX_COORD_PRODUCT
    for n in ("cap-x-lds", "cap-x-global"):
        H, W, (gw, gh, L) = BC.shape_of(n)
        assert (W - 1) * (gw - 1) == 4193280 < m <= (W + 1) * (gw - 1)       # two pixels below the cap
    H, W, (gw, gh, L) = BC.shape_of("cap-y-matrix")
    assert (H - 1) * (gh - 1) == 4193280 < m <= (H + 1) * (gh - 1)
    assert census_of("cap-x-global")["box"] == 9216


def test_census_of_the_ten_random_cases_is_pinned():
    """What tests/test_gpu_bilagrid.py reaches, so that a change of its inputs that loses (or gains) a class is noticed:
    its only uniform waves are the 33 of 33x129-(5,4,1), all with dead lanes and L = 1 (fz = 0: the upper four corners
    of the uniform form are zero), and its largest LDS request is the 55 296 B of 70x150-(16,16,8)."""
    got = {}
    for H, W, shape in R.CASES:
        c = BC.census(H, W, shape, R.make_inputs(H, W, shape)["image"].numpy())
        got["%dx%d-%dx%dx%d" % (H, W, *shape)] = (c["form"], c["lds_bytes"], c["counts"])
    assert got == {
        "1x1-1x1x1": ("matrix", 17504, {"mat_flush0": 1, "mat_dead": 1, "wave_without_rows": 3}),
        "5x7-1x1x1": ("matrix", 17504, {"mat_flush0": 4, "mat_dead": 4}),
        "9x1-4x4x4": ("matrix", 20480, {"mat_flush+": 4, "mat_dead": 4}),
        "20x20-1x4x3": ("matrix", 18560, {"mat_flush+": 4, "mat_dead": 4}),
        "33x129-5x4x1": ("lds", 1152, {"mixed_full": 66, "uniform_dead_clamped": 33, "wave_without_rows": 9}),
        "64x64-4x3x2": ("lds", 1536, {"mixed_full": 64}),
        "37x53-16x16x8": ("global", 0, {"global_dead": 37}),
        "70x150-16x16x8": ("lds", 55296, {"mixed_full": 140, "mixed_dead": 70}),
        "16x16-64x48x8": ("global", 0, {"global_dead": 16}),
        "70x150-2x5x8": ("matrix", 23552, {"mat_flush+": 24, "mat_dead": 12, "mat_flush0": 12}),
    }


@pytest.mark.parametrize("name", BC.ALL_NAMES)
def test_float64_restatement_is_the_grid_sample_reference(name):
    ref = BC.reference(name)
    theirs = R.ref_all(BC.inputs(name))
    for t in BC.TENSORS:
        err = np.abs(theirs[t].numpy() - ref[t]["ref"]).max()
        assert err <= 1e-12 * ref[t]["S"].max(), (t, err)
        assert (ref[t]["S"] >= np.abs(ref[t]["ref"]) * (1 - 1e-12)).all(), t


@pytest.mark.parametrize("name", list(BC.DELTA_OF))
def test_delta_reference_is_non_zero_on_the_intended_nodes_only(name):
    H, W, (gw, gh, L) = BC.shape_of(name)
    picks = BC.delta_pixels(name)
    assert all(0 <= x < W and 0 <= y < H for x, y in picks) and len(set(picks)) == len(picks)
    dout = BC.inputs(name)["dout"].numpy()
    lit = np.zeros((H, W), bool)
    for x, y in picks:
        lit[y, x] = True
    assert (dout[:, lit] != 0).all() and (dout[:, ~lit] == 0).all()
    luma = BC.luma32(BC.inputs(name)["image"].numpy())
    why = {v: k for k, v in picks.items()}
    x, y = why["luma < 0"]
    assert luma[y, x] < 0
    x, y = why["luma > 1"]
    assert luma[y, x] > 1
    x, y = why["exactly on a node of x"]
    assert x * (gw - 1) % (W - 1) == 0
    x, y = why["last live column of a ragged block, top cell of x"]
    assert x == W - 1 and W % BC.BW != 0
    hit = BC.intended_nodes(name)
    ref = BC.reference(name)["dgrid"]["ref"]
    assert 0 < hit.sum() < hit.size
    assert ((ref != 0) == hit[None]).all()
    # the grid_sample reference, which goes through normalised coordinates, agrees up to its own rounding
    theirs = R.ref_all(BC.inputs(name))["dgrid"].numpy()
    assert np.abs(theirs[:, ~hit]).max() <= 1e-12 * np.abs(theirs).max()
    dimage = BC.reference(name)["dimage"]["ref"]
    assert (dimage[:, ~lit] == 0).all() and (dimage[:, lit] != 0).all()


@pytest.mark.parametrize("name", BC.ALL_NAMES)
def test_calibration(name):
    """The T table against the reference alone: the spread of the float32 evaluations stays within half the floor
    T 2^-24 S on every entry, and no smaller power of two does that; each evaluation is within half of the whole bound
    max(floor, 2 x distance), which the kernel faces."""
    ref = BC.reference(name)
    for i, t in enumerate(BC.TENSORS):
        ratio = BC.calibration(name, t)
        print("%s %s: T = %d, spread / floor = %.2f, largest distance %.3g" % (name, t, BC.T[name][i], ratio,
                                                                                 ref[t]["distance"].max()))
        assert ratio <= 0.5, (t, ratio)
        assert BC.T[name][i] == BC.smallest_t(name, t), t
        d, bound = ref[t]["distance"], BC.bound_of(name, t)
        assert (d <= 0.5 * bound).all(), t
        assert (ref[t]["nearest"] <= d).all()


def test_orders_and_perturbations_move_the_restatement():
    """the evaluations are not nine copies of one: a shuffled order changes dgrid and nothing else, an ulp changes all"""
    inp = BC.inputs("uniform-L5")
    a, b, c = BC.slice_f32(inp), BC.slice_f32(inp, order=1), BC.slice_f32(inp, perturb=1)
    assert np.array_equal(a["out"], b["out"]) and np.array_equal(a["dimage"], b["dimage"])
    assert not np.array_equal(a["dgrid"], b["dgrid"])
    assert all(not np.array_equal(a[t], c[t]) for t in BC.TENSORS)
    assert all(a[t].dtype == np.float32 for t in BC.TENSORS)
