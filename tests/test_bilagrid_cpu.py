"""Bilateral-grid appearance compensation, host side (no GPU): the C surface of libegs_bilagrid.so against
include/egs_bilagrid.h and ``_bilagridlib.SIGNATURES``, its refusals before any HIP call, the untouched libegs_hip.so,
the float64 reference's own checks (tests/bilagrid_ref.py), ``GridTable`` on CPU tensors, ``slice_path`` and the
surface of ``Trainer(bilagrid=...)`` and examples/train.py."""
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import bilagrid_ref as R

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "egs_bilagrid.h")
BAD_ARG = 10001
_FAKE = 4096                    # a pointer nobody dereferences: every call below is refused before any HIP call
NAMES = ["egs_bilagrid_abi_version", "egs_bilagrid_last_error_string", "egs_bilagrid_slice", "egs_bilagrid_slice_bwd",
         "egs_bilagrid_tv"]


@pytest.fixture(scope="module")
def lib():
    from easygaussiansplatting_amd import _bilagridlib, _lib
    if not os.path.exists(_bilagridlib.LIB_PATH):
        _lib.build()
    return _bilagridlib.load()


# -------------------------------------------------------------------------------------------------------- the C surface
def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    return sorted(ln.split()[-1] for ln in out.splitlines() if ln.strip() and ln.split()[-1].startswith("egs_"))


def test_library_exports_the_five_names(lib):
    from easygaussiansplatting_amd import _bilagridlib
    assert _exports(_bilagridlib.LIB_PATH) == NAMES
    assert sorted(_bilagridlib.SIGNATURES) == NAMES
    hdr = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(set(re.findall(r"\b(egs_[a-z0-9_]+)\s*\(", code))) == NAMES
    assert re.search(r"^#define\s+EGS_BILAGRID_ABI_VERSION\s+1\s*$", hdr, re.M)
    assert lib.egs_bilagrid_abi_version() == 1 == _bilagridlib.ABI_VERSION
    for macro, value in (("BLOCK_W", _bilagridlib.BLOCK_W), ("BLOCK_H", _bilagridlib.BLOCK_H),
                         ("LDS_FLOATS", _bilagridlib.LDS_FLOATS)):
        assert re.search(r"^#define\s+EGS_BILAGRID_%s\s+%d\s*$" % (macro, value), hdr, re.M), macro
    for macro, value in (("MAX_GRID_FLOATS", _bilagridlib.MAX_GRID_FLOATS),
                         ("MAX_COORD_PRODUCT", _bilagridlib.MAX_COORD_PRODUCT)):
        m = re.search(r"^#define\s+EGS_BILAGRID_%s\s+\(1 << (\d+)\)\s*$" % macro, hdr, re.M)
        assert m and 1 << int(m.group(1)) == value, macro


def test_libegs_hip_is_untouched():
    from easygaussiansplatting_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    assert _lib.ABI_VERSION == 12 and _lib.load().egs_abi_version() == 12
    assert not any("bilagrid" in n for n in _lib.SIGNATURES)


def _refused(lib, rc):
    assert rc == BAD_ARG, rc
    msg = lib.egs_bilagrid_last_error_string().decode()
    assert msg.startswith("egs_bilagrid error 10001: bad argument"), msg


def test_every_entry_point_refuses_bad_arguments_without_a_device(lib):
    ok = dict(H=8, W=9, Gw=4, Gh=3, L=2)
    P = _FAKE

    def fwd(image=P, grid=2 * P, out=3 * P, device=0, **kw):
        d = dict(ok, **kw)
        return lib.egs_bilagrid_slice(device, None, d["H"], d["W"], d["Gw"], d["Gh"], d["L"], image, grid, out)

    def bwd(image=P, grid=2 * P, dout=3 * P, dimage=4 * P, dgrid=5 * P, device=0, **kw):
        d = dict(ok, **kw)
        return lib.egs_bilagrid_slice_bwd(device, None, d["H"], d["W"], d["Gw"], d["Gh"], d["L"], image, grid, dout,
                                          dimage, dgrid)

    def tv(grid=P, value=2 * P, dgrid=3 * P, device=0, **kw):
        d = dict(ok, **kw)
        return lib.egs_bilagrid_tv(device, None, d["Gw"], d["Gh"], d["L"], grid, 1.0, value, dgrid)

    for size in ("H", "W", "Gw", "Gh", "L"):
        for bad in (0, -3):
            _refused(lib, fwd(**{size: bad}))
            _refused(lib, bwd(**{size: bad}))
            if size in ("Gw", "Gh", "L"):
                _refused(lib, tv(**{size: bad}))
    # oversize grids: Gw Gh L 12 floats beyond the header's limit
    big = dict(Gw=2048, Gh=1024, L=1)
    assert 12 * 2048 * 1024 > (1 << 24)
    _refused(lib, fwd(H=1, W=1, **big))
    _refused(lib, bwd(H=1, W=1, **big))
    _refused(lib, tv(**big))
    # null pointers
    for name in ("image", "grid", "out"):
        _refused(lib, fwd(**{name: None}))
    for name in ("image", "grid", "dout"):
        _refused(lib, bwd(**{name: None}))
        _refused(lib, bwd(dimage=None, dgrid=None, **{name: None}))      # (checked before the no-op return)
    for name in ("grid", "value"):
        _refused(lib, tv(**{name: None}))
    _refused(lib, fwd(device=-1))
    _refused(lib, bwd(device=-1))
    _refused(lib, tv(device=-1))
    # both halves of the backward pass skipped: nothing to do, and nothing touches a device
    assert bwd(dimage=None, dgrid=None) == 0


def test_sources_read_no_environment_variable():
    src = open(os.path.join(REPO, "easygaussiansplatting_amd", "csrc", "egs_bilagrid.hip")).read()
    assert "getenv" not in src and "WRONG" not in src


# -------------------------------------------------------------------------------------------------- the reference itself
def test_reference_identity_grid_returns_the_image():
    from easygaussiansplatting_amd import appearance
    for H, W, shape in ((5, 7, (1, 1, 1)), (9, 6, (4, 3, 5))):
        image = R.make_inputs(H, W, shape)["image"].double()
        grid = appearance.identity_grids(1, shape)[0].double()
        assert tuple(grid.shape) == (12, shape[2], shape[1], shape[0])
        assert float((R.ref_slice(image, grid) - image).abs().max()) <= 1e-12


def test_reference_single_node_grid_is_one_affine_transform():
    inp = R.make_inputs(6, 5, (1, 1, 1), seed=3)
    image, grid = inp["image"].double(), inp["grid"].double()
    A = grid.reshape(3, 4)
    want = torch.einsum("cj,jhw->chw", A[:, :3], image) + A[:, 3, None, None]
    assert float((R.ref_slice(image, grid) - want).abs().max()) <= 1e-12


def test_reference_tv_of_a_linear_ramp():
    gw, gh, L = 5, 4, 3
    a, b, c = 0.25, -0.5, 2.0
    z, y, x = torch.meshgrid(torch.arange(L), torch.arange(gh), torch.arange(gw), indexing="ij")
    grid = (a * x + b * y + c * z).double()[None].expand(12, L, gh, gw).contiguous()
    assert abs(float(R.ref_tv(grid)) - (a * a + b * b + c * c)) <= 1e-12
    assert float(R.ref_tv(grid[:, :1, :, :1])) == pytest.approx(b * b, abs=1e-12)     # axes of one node contribute 0
    assert float(R.ref_tv(grid[:, :1, :1, :1])) == 0.0


def test_reference_gradients_pass_gradcheck():
    inp = R.make_inputs(5, 7, (3, 2, 2), seed=1)
    assert bool(R.off_plane(inp["image"], 2).all())
    image = inp["image"].double().requires_grad_(True)
    grid = inp["grid"].double().requires_grad_(True)
    assert torch.autograd.gradcheck(R.ref_slice, (image, grid), eps=1e-6, atol=1e-7, rtol=1e-5)
    assert torch.autograd.gradcheck(R.ref_tv, (grid,), eps=1e-6, atol=1e-7, rtol=1e-5)


def test_input_builder_leaves_no_pixel_near_a_luminance_plane():
    for H, W, shape in R.CASES:
        inp = R.make_inputs(H, W, shape)
        L = shape[2]
        assert bool(R.off_plane(inp["image"], L).all()) or L == 1
        luma = R.luma_of(inp["image"].double())
        if H * W >= 400:          # both clamps are exercised
            assert float(luma.min()) < 0 and float(luma.max()) > 1
        assert tuple(inp["grid"].shape) == (12, L, shape[1], shape[0])


# ------------------------------------------------------------------------------------------------------------ GridTable
def test_grid_table_steps_rows_like_torch_adam_on_cpu():
    from easygaussiansplatting_amd.appearance import GridTable
    shape = (3, 2, 2)
    table = GridTable(4, shape, lr=2e-3, device="cpu")
    g = torch.Generator().manual_seed(11)
    table.grids += 0.1 * torch.randn(table.grids.shape, generator=g)
    start = table.grids.clone()
    twins = {v: table.grids[v].clone().requires_grad_(True) for v in (1, 3)}
    opts = {v: torch.optim.Adam([p], lr=2e-3, betas=(0.9, 0.999), eps=1e-15) for v, p in twins.items()}
    schedule = ([1], [3, 1], [1])                              # row 1 takes three steps, row 3 one, rows 0 and 2 none
    for views in schedule:
        rows = torch.randn((len(views), table.row_floats), generator=g) * 1e-3
        for k, v in enumerate(views):
            twins[v].grad = rows[k].reshape(twins[v].shape).clone()
            opts[v].step()
        table.step(views, rows)
    as_bits = lambda t: t.detach().contiguous().view(torch.int32)
    for v in (1, 3):
        assert torch.equal(as_bits(table.grids[v]), as_bits(twins[v])), v
        state = opts[v].state[twins[v]]
        assert torch.equal(as_bits(table.exp_avg[v]), as_bits(state["exp_avg"]))
        assert torch.equal(as_bits(table.exp_avg_sq[v]), as_bits(state["exp_avg_sq"]))
        assert not torch.equal(table.grids[v], start[v])
    for v in (0, 2):
        assert torch.equal(as_bits(table.grids[v]), as_bits(start[v]))
        assert int(table.exp_avg[v].abs().max()) == 0 and int(table.exp_avg_sq[v].abs().max()) == 0
    assert table.steps.tolist() == [0, 3, 0, 1]
    with pytest.raises(ValueError):
        table.step([1, 1], torch.zeros((2, table.row_floats)))


def test_grid_table_save_and_load_round_trip(tmp_path):
    from easygaussiansplatting_amd.appearance import GridTable
    shape = (4, 3, 2)
    table = GridTable(3, shape, device="cpu")
    table.grids += torch.randn(table.grids.shape, generator=torch.Generator().manual_seed(2))
    fn = str(tmp_path / "grids.npz")
    table.save(fn, ids=[7, 8, 9])
    with np.load(fn) as z:
        assert sorted(z.files) == ["grids", "ids", "shape"]
        assert z["ids"].tolist() == [7, 8, 9] and tuple(z["shape"]) == shape
        assert z["grids"].shape == (3, 12, 2, 3, 4) and z["grids"].dtype == np.float32
    other = GridTable(3, shape, device="cpu")
    assert other.load(fn).tolist() == [7, 8, 9]
    assert torch.equal(other.grids, table.grids)
    with pytest.raises(ValueError):
        GridTable(3, (4, 3, 3), device="cpu").load(fn)


def test_slice_path_names_both_paths():
    from easygaussiansplatting_amd import appearance
    assert appearance.slice_path(1080, 1920, (16, 16, 8)) == "lds"
    assert appearance.slice_path(16, 16, (64, 48, 8)) == "global"
    assert {appearance.slice_path(H, W, s) for H, W, s in R.CASES} == {"lds", "global"}
    # 1080p, 16 x 16 x 8: cells of 127.9 x 71.9 pixels.  A 64-wide block starts on a multiple of 64 and never straddles
    # a column of nodes (2 nodes); a 32-high block can straddle a row of nodes (3 nodes)
    assert appearance.largest_box(1080, 1920, (16, 16, 8)) == 2 * 3 * 8 * 12
    assert appearance.dgrid_form(1080, 1920, (16, 16, 8)) == "matrix"
    assert appearance.dgrid_form(64, 64, (4, 3, 2)) == "lds" and appearance.dgrid_form(16, 16, (64, 48, 8)) == "global"


# ---------------------------------------------------------------------------------------------------- the Trainer surface
def test_trainer_surface():
    from easygaussiansplatting_amd.trainer import Trainer
    params = inspect.signature(Trainer.__init__).parameters
    assert params["bilagrid"].default is False
    assert tuple(params["bilagrid_shape"].default) == (16, 16, 8)
    assert params["bilagrid_lr"].default == 2e-3 and params["bilagrid_tv"].default == 10.0
    for name in ("grids", "save_grids", "corrected"):
        assert callable(getattr(Trainer, name))
    # the constructor calls of the other host-side tests still end where they did
    with pytest.raises(ValueError, match="cap_max"):
        Trainer(None, [], [], 10, strategy="mcmc")
    with pytest.raises(ValueError, match="strategy"):
        Trainer(None, [], [], 10, strategy="adaptive")
    with pytest.raises(ValueError, match="sparse_adam=True.*fused_adam"):
        Trainer(None, [], [], max_steps=10, device="cpu", sparse_adam=True, fused_adam=False)
    with pytest.raises(ValueError, match="cap_max"):
        Trainer(None, [], [], 10, strategy="mcmc", bilagrid=True)
    with pytest.raises(ValueError, match="bilagrid_shape"):
        Trainer(None, [], [], 10, bilagrid=True, bilagrid_shape=(16, 0, 8))


def test_train_example_lists_the_flag():
    r = subprocess.run([sys.executable, os.path.join(REPO, "examples", "train.py"), "--help"], capture_output=True,
                       text=True, cwd=REPO)
    assert r.returncode == 0, r.stderr
    assert "--bilagrid" in r.stdout and "--bilagrid-shape" in r.stdout
