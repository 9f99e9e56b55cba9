"""The bilateral-grid kernels on the device (csrc/egs_bilagrid.hip) against the float64 ``grid_sample``
reference of tests/bilagrid_ref.py, on shapes that reach both kernel paths (LDS box / global), ragged pixel blocks,
lattice axes of one node and L = 1.  No pixel is excluded from any comparison: the input builder keeps every pixel away
from the luminance planes where the gradient is discontinuous.

Bounds: the forward output to 1e-4 of float64 (the project's image bound; inputs are O(1)); gradients by the rule of
tests/gradcheck.py with its defaults and ``outliers=0``; the adjoint identity and the TV value to 1e-5 relative."""
import functools

import numpy as np
import pytest

from tests import bilagrid_ref as R
from tests.gradcheck import assert_grad_close

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TV_WEIGHT = 10.0
IDS = ["%dx%d-%dx%dx%d" % (H, W, *s) for H, W, s in R.CASES]


@pytest.fixture(scope="module")
def ap():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from easygaussiansplatting_amd import appearance
    return appearance


@functools.lru_cache(maxsize=None)
def case(index):
    """inputs (float32, on the device) and the float64 reference of one case: computed once, shared, never written to"""
    H, W, shape = R.CASES[index]
    inp = R.make_inputs(H, W, shape)
    ref = R.ref_all(inp, tv_weight=TV_WEIGHT)
    return {k: v.cuda() for k, v in inp.items()}, {k: v.numpy() for k, v in ref.items()}


def host(t):
    return t.detach().cpu().numpy()


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def test_the_cases_reach_both_paths(ap):
    assert {ap.slice_path(H, W, s) for H, W, s in R.CASES} == {"lds", "global"}
    assert ap.slice_path(70, 150, (16, 16, 8)) == "lds" and ap.slice_path(16, 16, (64, 48, 8)) == "global"
    forms = {s: ap.dgrid_form(H, W, s) for H, W, s in R.CASES}
    assert set(forms.values()) == {"matrix", "lds", "global"}
    assert ap.dgrid_form(70, 150, (2, 5, 8)) == "matrix" and ap.dgrid_form(70, 150, (16, 16, 8)) == "lds"


@pytest.mark.parametrize("index", range(len(R.CASES)), ids=IDS)
def test_forward_against_float64(ap, index):
    inp, ref = case(index)
    out = ap.slice_forward(inp["image"], inp["grid"])
    again = ap.slice_forward(inp["image"], inp["grid"])
    err = np.abs(host(out).astype(np.float64) - ref["out"]).max()
    print("forward max|err| = %.3g" % err)
    assert err <= 1e-4
    assert torch.equal(bits(out), bits(again))


@pytest.mark.parametrize("index", range(len(R.CASES)), ids=IDS)
def test_backward_against_float64(ap, index):
    inp, ref = case(index)
    image, grid, dout = inp["image"], inp["grid"], inp["dout"]
    dgrid = torch.zeros_like(grid)
    dimage = ap.slice_backward(image, grid, dout, dgrid)
    assert_grad_close(host(dimage), ref["dimage"], "dimage", outliers=0)
    assert_grad_close(host(dgrid), ref["dgrid"], "dgrid", outliers=0)
    # the adjoint identity: slice is linear in G, so <dout, slice(rgb; G)> = <dgrid, G>
    out = ap.slice_forward(image, grid)
    lhs = float((host(dout).astype(np.float64) * host(out)).sum())
    rhs = float((host(dgrid).astype(np.float64) * host(grid)).sum())
    print("adjoint: %.9g against %.9g" % (lhs, rhs))
    assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), abs(rhs))
    # a second pass into the same dgrid doubles it; dimage is written, not accumulated, and reproducible to the bit
    again = ap.slice_backward(image, grid, dout, dgrid)
    assert torch.equal(bits(again), bits(dimage))
    assert_grad_close(host(dgrid), 2 * ref["dgrid"], "dgrid after two passes", outliers=0)
    # either half alone
    alone = ap.slice_backward(image, grid, dout, None)
    assert torch.equal(bits(alone), bits(dimage))
    only = torch.zeros_like(grid)
    assert ap.slice_backward(image, grid, dout, only, need_dimage=False) is None
    assert_grad_close(host(only), ref["dgrid"], "dgrid alone", outliers=0)


@pytest.mark.parametrize("index", range(len(R.CASES)), ids=IDS)
def test_tv_against_float64(ap, index):
    inp, ref = case(index)
    grid = inp["grid"]
    start = torch.randn(grid.shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    dgrid = start.clone()
    value = ap.tv(grid, TV_WEIGHT, dgrid)
    assert value.dim() == 0 and value.is_cuda
    want = float(ref["tv"])
    print("tv = %.9g against %.9g" % (float(value), want))
    assert abs(float(value) - want) <= 1e-5 * abs(want)
    added = host(dgrid).astype(np.float64) - host(start)
    if np.abs(ref["dtv"]).max() == 0:           # one node: no differences, nothing to add
        assert want == 0 and torch.equal(bits(dgrid), bits(start))
    else:
        # (the gradient is read back as a difference of float32 sums with an O(1) start: start from zero for the rule)
        fresh = torch.zeros_like(grid)
        ap.tv(grid, TV_WEIGHT, fresh)
        assert_grad_close(host(fresh), ref["dtv"], "dtv", outliers=0)
        assert np.abs(added - ref["dtv"]).max() <= 1e-6 * max(1.0, np.abs(ref["dtv"]).max())
    assert torch.equal(bits(ap.tv(grid, TV_WEIGHT)), bits(value))           # no dgrid: the value alone, same bits


@pytest.mark.parametrize("index", range(len(R.CASES)), ids=IDS)
def test_autograd_node_gives_the_direct_gradients(ap, index):
    inp, ref = case(index)
    image = inp["image"].clone().requires_grad_(True)
    grid = inp["grid"].clone().requires_grad_(True)
    out = ap.apply_grid(image, grid)
    assert torch.equal(bits(out), bits(ap.slice_forward(inp["image"], inp["grid"])))
    out.backward(inp["dout"])
    direct = ap.slice_backward(inp["image"], inp["grid"], inp["dout"], None)
    assert torch.equal(bits(image.grad), bits(direct))
    assert_grad_close(host(grid.grad), ref["dgrid"], "grid.grad", outliers=0)
    # one input alone
    g2 = inp["grid"].clone().requires_grad_(True)
    ap.apply_grid(inp["image"], g2).backward(inp["dout"])
    assert_grad_close(host(g2.grad), ref["dgrid"], "grid.grad alone", outliers=0)


def test_wrappers_refuse_what_the_library_would(ap):
    inp, _ = case(1)
    with pytest.raises(ValueError):
        ap.slice_forward(inp["image"][:2], inp["grid"])
    with pytest.raises(ValueError):
        ap.slice_forward(inp["image"].cpu(), inp["grid"])
    with pytest.raises(ValueError):
        ap.slice_backward(inp["image"], inp["grid"], inp["dout"], torch.zeros((12, 2, 2, 2), device="cuda"))
