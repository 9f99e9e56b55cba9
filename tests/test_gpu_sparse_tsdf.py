"""The block-allocated TSDF volume (csrc/egs_sparsetsdf.hip, ``mesh.SparseTSDFVolume``) on the GPU.  Its
yardstick is the dense volume of libegs_tsdf.so, BIT FOR BIT: both call the functions of csrc/egs_tsdf_device.h, so
integration and extraction carry no tolerance at all.  Only the allocation has margins, and they are of one block each way:

  1. allocation    the allocated set holds every block with a decided sample the dense kernel updated with t < 1, and lies
                   inside the Chebyshev-2 dilation of what the float64 restatement (tests/sparse_tsdf_ref.py) flags -- the
                   float32 march at a step of one voxel and the dilation may differ from it by a block each; slots ascend
                   with the block index within a view; two runs agree.
  2. integration   a dense volume is kept beside the sparse one; after every view its planes are put back to their previous
                   bits outside the blocks allocated so far (the documented semantics: a block is updated from the view that
                   allocates it onwards), and ``to_dense()`` must equal them.  The grid capped at 1 and 3 workgroups and a
                   side stream give the same pool bits; the ABI calls run between guard bands.
  3. extraction    ``from_dense`` of volumes with all 256 corner patterns, a ragged random field and a sphere, under four
                   block masks, against ``TSDFVolume.extract`` of the same planes with the weight zeroed outside the mask.
  4. end to end    a sphere from four cameras into 40^3 (tests/test_sparse_tsdf_cpu.py shows the scene covered); errors;
                   ``Trainer.extract_mesh(sparse=...)``.

Lattices 1^3, 8^3 (one block), 9 x 8 x 8 (a second block one sample wide), 20 x 13 x 9 (ragged on every axis), 130 x 33 x 9;
views front, oblique (per-pixel weights, half the image under alpha_min) and inside (no opacity map, depth_max) at 16 x 12
and 33 x 20 pixels (tests/sparse_tsdf_ref.case_list says why 130 x 33 x 9 takes the larger image only), colour on and off.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import sparse_tsdf_ref as SR
from tests import tsdf_ref as TR

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.loss_abi import bits, dev, guarded, guards_intact  # noqa: E402  (needs torch)

CASES = SR.case_list()
CASE_IDS = ["%dx%dx%d-%dx%d" % (d + (hw[1], hw[0])) for d, hw in CASES]
BAD_ARG = 10001


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from easygaussiansplatting_amd import _sparsetsdflib
    return _sparsetsdflib.load()


class Cam:
    def __init__(self, view):
        self.fx, self.fy, self.cx, self.cy = view["K"]
        self.Rcw, self.tcw = np.asarray(view["R"], np.float64), np.asarray(view["t"], np.float64)


@functools.lru_cache(maxsize=None)
def case(dims, hw):
    """-> (lat, views, per view: the device maps, the float64 flags, the decided mask): computed once, left unchanged"""
    lat = TR.make_lattice(dims)
    views = SR.make_views(lat, hw)
    return lat, views, [SR.touch(lat, v) for v in views], [TR.decided(lat, v) for v in views]


def maps(view):
    return {k: None if view.get(k) is None else dev(view[k]) for k in ("depth", "alpha", "image", "weight")}


def fuse(vol, view, dv=None, **kw):
    dv = dv or maps(view)
    vol.integrate(dv["depth"], dv["alpha"], Cam(view), image=dv["image"] if vol.color is not None else None,
                  weight=dv["weight"], alpha_min=view["alpha_min"], near=view["near"], depth_max=view["depth_max"], **kw)


def volumes(lat, view, color, **kw):
    from easygaussiansplatting_amd.mesh import SparseTSDFVolume, TSDFVolume
    return (SparseTSDFVolume(lat["origin"], lat["voxel"], lat["dims"], trunc=view["trunc"], color=color, **kw),
            TSDFVolume(lat["origin"], lat["voxel"], lat["dims"], trunc=view["trunc"], color=color))


def same_bits(a, b):
    return (a is None and b is None) or torch.equal(bits(a), bits(b))


def pool_bits(vol):
    n = vol.n_blocks
    return [vol.directory.clone(), vol.block_coords[:n].clone(), bits(vol.tsdf[:n]).clone(), bits(vol.weight[:n]).clone(),
            None if vol.color is None else bits(vol.color[:, :n]).clone()]


def same_pools(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------------- 1. allocation
@pytest.mark.parametrize("dims,hw", CASES, ids=CASE_IDS)
def test_allocation_is_two_sided_ascending_and_reproducible(lib, dims, hw):
    lat, views, ref_flags, decided = case(dims, hw)
    runs = []
    for run in range(2):
        sp, _ = volumes(lat, views[0], True)
        upper = np.zeros(SR.block_dims(dims)[::-1], bool)
        n_prev = 0
        for k, view in enumerate(views):
            dv = maps(view)
            fuse(sp, view, dv)
            alloc = (sp.directory >= 0).cpu().numpy()
            if run == 0:
                # the dense kernel alone on a fresh volume: a sample it updated with t < 1 holds tsdf = t < 1
                _, dn = volumes(lat, view, True)
                fuse(dn, view, dv)
                band = ((dn.weight > 0) & (dn.tsdf < 1)).cpu().numpy() & decided[k]
                need = SR.blocks_of(band)
                upper |= SR.dilate(ref_flags[k], 2)
                print("%s %s view %d: %d blocks allocated of %d, %d needed, %d allowed" % (
                    dims, hw, k, int(alloc.sum()), alloc.size, int(need.sum()), int(upper.sum())))
                assert not (need & ~alloc).any(), "view %d: a block of the band is not allocated" % k
                assert not (alloc & ~upper).any(), "view %d: a block beyond two blocks of the restatement's set" % k
            fresh = sp.block_coords[n_prev:sp.n_blocks].cpu().numpy()
            assert (np.diff(fresh) > 0).all() and int(alloc.sum()) == sp.n_blocks
            n_prev = sp.n_blocks
        coords = sp.block_coords[:sp.n_blocks].long()
        assert torch.equal(sp.directory.reshape(-1)[coords], torch.arange(sp.n_blocks, dtype=torch.int32, device="cuda"))
        runs.append((sp.directory.clone(), sp.block_coords[:sp.n_blocks].clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert runs[0][1].numel() > 0


# --------------------------------------------------------------------------------------------------------- 2. integration
@pytest.mark.parametrize("color", [True, False], ids=["color", "plain"])
@pytest.mark.parametrize("dims,hw", CASES, ids=CASE_IDS)
def test_integration_gives_the_dense_kernels_bits(lib, dims, hw, color):
    lat, views, _, _ = case(dims, hw)
    sp, dn = volumes(lat, views[0], color)
    capped = [volumes(lat, views[0], color)[0] for _ in range(2)]
    side, stream = volumes(lat, views[0], color)[0], torch.cuda.Stream()
    names = ("tsdf", "weight") + (("color",) if color else ())
    for k, view in enumerate(views):
        dv = maps(view)
        prev = {n: getattr(dn, n).clone() for n in names}
        fuse(dn, view, dv)
        fuse(sp, view, dv)
        inside = torch.from_numpy(SR.samples_of((sp.directory >= 0).cpu().numpy(), dims)).cuda()
        for n in names:
            setattr(dn, n, torch.where(inside.expand_as(prev[n]), getattr(dn, n), prev[n]))
        got = sp.to_dense()
        for n in names:
            assert same_bits(getattr(got, n), getattr(dn, n)), "%s after view %d" % (n, k)
        for vol, cap in zip(capped, (1, 3)):
            fuse(vol, view, dv, grid_cap=cap)
            assert same_pools(pool_bits(vol), pool_bits(sp)), "grid capped at %d, view %d" % (cap, k)
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            fuse(side, view, dv)
        stream.synchronize()
        assert same_pools(pool_bits(side), pool_bits(sp)), "side stream, view %d" % k
    assert float(dn.weight.max()) > 0 and sp.n_blocks > 0
    if dims == (130, 33, 9):
        assert float(dn.weight.max()) > 1.0 and sp.n_blocks < sp.directory.numel()      # seen twice; truly sparse


@pytest.mark.parametrize("dims,hw", [((20, 13, 9), (12, 16)), ((130, 33, 9), (20, 33))], ids=["20x13x9", "130x33x9"])
def test_the_abi_calls_between_guard_bands_give_the_python_layers_bits(lib, dims, hw):
    """every buffer a call writes sits between guard bands that must be intact afterwards: flags, fresh, directory,
    block_coords, the pools (a capacity one slot above what the three views need), counts and the mesh buffers"""
    lat, views, _, _ = case(dims, hw)
    sp, _ = volumes(lat, views[0], True)
    for view in views:
        fuse(sp, view)
    nb = SR.block_dims(dims)
    n_dir, cap = nb[0] * nb[1] * nb[2], sp.n_blocks + 1
    geo = (*dims, *[float(v) for v in lat["origin"]], float(lat["voxel"]))
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    whole = {}

    def buf(name, nbytes, dtype, fill):
        whole[name], inner = guarded(nbytes)
        v = inner.view(dtype)
        v.fill_(fill)
        return v

    def intact(what):
        torch.cuda.synchronize()
        for name, w in whole.items():
            assert guards_intact(w), "%s wrote outside %s" % (what, name)

    directory = buf("directory", 4 * n_dir, torch.int32, -1)
    coords = buf("block_coords", 4 * cap, torch.int32, -1)
    tsdf, weight = buf("tsdf", 2048 * cap, torch.float32, 1.0), buf("weight", 2048 * cap, torch.float32, 0.0)
    color = buf("color", 3 * 2048 * cap, torch.float32, 0.0)
    n = 0
    for view in views:
        dv = maps(view)
        R, t = dev(np.asarray(view["R"]).reshape(-1)), dev(view["t"])
        tail = (*[float(v) for v in view["K"]], p(R), p(t), float(view["trunc"]), float(view["alpha_min"]),
                float(view["near"]), float("inf") if view["depth_max"] is None else float(view["depth_max"]))
        H, W = view["depth"].shape
        flags, fresh = buf("flags", 4 * n_dir, torch.int32, 0), buf("fresh", 4 * n_dir, torch.int32, -7)
        assert lib.egs_sparsetsdf_touch(*geo, H, W, p(dv["depth"]), p(dv["alpha"]), p(dv["weight"]), *tail, p(flags), st) == 0
        intact("touch")
        assert set(flags.unique().tolist()) <= {0, 1}
        assert lib.egs_sparsetsdf_mark(*dims, p(flags), p(directory), p(fresh), st) == 0
        intact("mark")
        ends = torch.cumsum(fresh, 0, dtype=torch.int64)
        offsets = (ends - fresh).contiguous()
        assert lib.egs_sparsetsdf_assign(*dims, p(fresh), p(offsets), n, cap, p(directory), p(coords), st) == 0
        intact("assign")
        n += int(ends[-1])
        assert lib.egs_sparsetsdf_integrate(*geo, n, cap, p(coords), p(tsdf), p(weight), p(color), H, W, p(dv["depth"]),
                                            p(dv["alpha"]), p(dv["image"]), p(dv["weight"]), *tail, 0, st) == 0
        intact("integrate")
    assert n == sp.n_blocks and torch.equal(directory, sp.directory.reshape(-1)) and torch.equal(coords[:n], sp.block_coords[:n])
    assert same_bits(tsdf[:512 * n], sp.tsdf[:n].reshape(-1)) and same_bits(weight[:512 * n], sp.weight[:n].reshape(-1))
    assert same_bits(color.reshape(3, cap, 512)[:, :n], sp.color[:, :n])
    assert float(tsdf[512 * n:].min()) == 1.0 and float(weight[512 * n:].max()) == 0.0      # the spare slot is untouched
    # extraction
    counts = buf("counts", 4 * 512 * n, torch.int32, -1)
    assert lib.egs_sparsetsdf_mesh_count(*dims, n, cap, p(directory), p(coords), p(tsdf), p(weight), 1.0, p(counts), st) == 0
    intact("mesh_count")
    ends = torch.cumsum(counts, 0, dtype=torch.int64)
    offsets, total = (ends - counts).contiguous(), int(ends[-1])
    assert int(counts.min()) >= 0 and int(counts.max()) <= 12 and total > 0
    verts, keys = buf("verts", 36 * total, torch.float32, float("nan")), buf("keys", 24 * total, torch.int64, -1)
    cols = buf("colors", 36 * total, torch.float32, float("nan"))
    assert lib.egs_sparsetsdf_mesh_emit(*geo, n, cap, p(directory), p(coords), p(tsdf), p(weight), p(color), 1.0,
                                        p(offsets), total, total, p(verts), p(keys), p(cols), st) == 0
    intact("mesh_emit")
    v2, k2, c2 = sp.extract_triangles()
    assert same_bits(verts, v2.reshape(-1)) and torch.equal(keys, k2.reshape(-1)) and same_bits(cols, c2.reshape(-1))
    # a short output: refused with 10003, nothing written; offsets that point past the end: nothing written there
    verts.fill_(float("nan"))
    assert lib.egs_sparsetsdf_mesh_emit(*geo, n, cap, p(directory), p(coords), p(tsdf), p(weight), p(color), 1.0,
                                        p(offsets), total, total - 1, p(verts), p(keys), p(cols), st) == 10003
    intact("a refused mesh_emit")
    assert bool(torch.isnan(verts).all())
    assert lib.egs_sparsetsdf_mesh_emit(*geo, n, cap, p(directory), p(coords), p(tsdf), p(weight), p(color), 1.0,
                                        p((offsets + total - 1).contiguous()), total, total, p(verts), p(keys), p(cols), st) == 0
    intact("mesh_emit with offsets past the end")


# ---------------------------------------------------------------------------------------------------------- 3. extraction
@functools.lru_cache(maxsize=None)
def field(name):
    if name == "patterns":
        lat, f, w = TR.pattern_volume()
        return lat, f, w, None
    if name == "smooth":
        return TR.smooth_field((20, 13, 9))
    lat, f, w = TR.sphere_volume(24)
    return lat, f, w, None


def block_masks(nb, which):
    nbx, nby, nbz = nb
    bz, by, bx = np.meshgrid(np.arange(nbz), np.arange(nby), np.arange(nbx), indexing="ij")
    if which == "all":
        return np.ones((nbz, nby, nbx), bool)
    if which == "checkerboard":
        return (bx + by + bz) % 2 == 0
    if which == "single":      # interior along every axis that has an interior, the first block along the others
        mid = lambda n: n // 2 if n >= 3 else 0
        return (bx == mid(nbx)) & (by == mid(nby)) & (bz == mid(nbz))
    return np.random.default_rng(11).random((nbz, nby, nbx)) < 0.5


def sorted_soup(verts, keys, cols):
    """the triangles in the order of their key triples"""
    k = keys.cpu().numpy()
    order = np.lexsort((k[:, 2], k[:, 1], k[:, 0]))
    take = lambda t: None if t is None else bits(t.reshape(len(k), 9)).cpu().numpy()[order]
    return k[order], take(verts), take(cols)


@pytest.mark.parametrize("which", ["all", "checkerboard", "single", "random"])
@pytest.mark.parametrize("name", ["patterns", "smooth", "sphere"])
def test_extraction_gives_the_dense_extractions_bits(lib, name, which):
    from easygaussiansplatting_amd.mesh import SparseTSDFVolume, TSDFVolume
    lat, f, w, c = field(name)
    dims = lat["dims"]
    mask = block_masks(SR.block_dims(dims), which)
    dense = TSDFVolume(lat["origin"], lat["voxel"], dims, color=c is not None)
    dense.tsdf, dense.weight = dev(f), dev(w)
    if c is not None:
        dense.color = dev(c)
    sp = SparseTSDFVolume.from_dense(dense, torch.from_numpy(mask).cuda())
    assert sp.n_blocks == int(mask.sum()) and (np.diff(sp.block_coords[:sp.n_blocks].cpu().numpy()) > 0).all()
    inside = torch.from_numpy(SR.samples_of(mask, dims)).cuda()
    dense.weight = torch.where(inside, dense.weight, torch.zeros_like(dense.weight))
    back = sp.to_dense()
    assert same_bits(back.weight, dense.weight) and same_bits(back.tsdf[inside], dense.tsdf[inside])
    # the soups: the same triangles (vertices, keys, colours, bit for bit) up to their order
    a, b = sorted_soup(*sp.extract_triangles()), sorted_soup(*dense.extract_triangles())
    print("%s / %s: %d of %d blocks, %d triangles" % (name, which, sp.n_blocks, mask.size, len(a[0])))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert (a[2] is None and b[2] is None) or np.array_equal(a[2], b[2])
    # (the one interior block of the 24^3 sphere, samples 8..15 of every axis, lies wholly inside it: no triangle either way)
    assert len(a[0]) > 0 or (name, which) == ("sphere", "single")
    # the welded meshes
    V, F, Cs = sp.extract()
    V2, F2, C2 = dense.extract()
    assert same_bits(V, V2) and same_bits(Cs, C2)
    rows = lambda F: np.unique(F.cpu().numpy(), axis=0)
    assert len(F) == len(F2) and np.array_equal(rows(F), rows(F2))
    if name == "patterns" and which == "all":
        assert sorted(set(TR.corner_patterns(f)[0, 0, ::2].tolist())) == list(range(256))
    if name == "sphere" and which == "all":
        assert TR.closed_and_consistent(F.cpu().numpy()) and TR.euler(V.cpu().numpy(), F.cpu().numpy()) == 2
    if which == "single":
        # a cell whose far corner lies in an unallocated neighbour emits nothing: both ends of every edge a vertex sits
        # on are samples of the one block
        nx, ny, _ = dims
        bz, by, bx = [int(v[0]) for v in np.nonzero(mask)]
        keys = sp.extract_triangles()[1].reshape(-1).cpu().numpy()
        lo, typ = keys // 7, keys % 7
        step = np.array([(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)])[typ]
        xyz = np.stack([lo % nx, (lo // nx) % ny, lo // (nx * ny)], 1)
        for end in (xyz, xyz + step):
            assert (end // 8 == np.array([bx, by, bz])).all()
        full = SparseTSDFVolume.from_dense(TSDFVolume(lat["origin"], lat["voxel"], dims, color=False), torch.from_numpy(mask).cuda())
        assert full.extract_triangles()[0].shape[0] == 0          # (and an unobserved block gives no triangle at all)
        assert len(a[0]) < len(sorted_soup(*SparseTSDFVolume.from_dense(
            _dense_of(lat, f, w, c), torch.ones_like(torch.from_numpy(mask)).cuda()).extract_triangles())[0])


def _dense_of(lat, f, w, c):
    from easygaussiansplatting_amd.mesh import TSDFVolume
    vol = TSDFVolume(lat["origin"], lat["voxel"], lat["dims"], color=c is not None)
    vol.tsdf, vol.weight = dev(f), dev(w)
    if c is not None:
        vol.color = dev(c)
    return vol


# ------------------------------------------------------------------------------------------------- 4. end to end, errors
def test_a_sphere_from_four_cameras_gives_the_dense_mesh_and_closes(lib):
    """tests/test_sparse_tsdf_cpu.py shows, in float64, that this scene satisfies the footprint condition, that the band
    of every view is covered and that no block is observed before the view that allocates it.  The last is asserted here
    again on the kernels' own allocation; the sparse planes then equal the dense ones on the allocated blocks, and the
    welded meshes are identical on every cell whose eight corners are allocated."""
    lat = TR.make_lattice(SR.E2E_DIMS)
    views = SR.e2e_views(lat)
    sp, dn = volumes(lat, views[0], True)
    for k, view in enumerate(views):
        dv = maps(view)
        before = (sp.directory >= 0).cpu().numpy()
        fuse(sp, view, dv)
        new = (sp.directory >= 0).cpu().numpy() & ~before
        seen = (dn.weight > 0).cpu().numpy()
        assert not (seen & SR.samples_of(new, SR.E2E_DIMS)).any(), "view %d allocates a block an earlier view observed" % k
        fuse(dn, view, dv)
    alloc = (sp.directory >= 0).cpu().numpy()
    inside = torch.from_numpy(SR.samples_of(alloc, SR.E2E_DIMS)).cuda()
    back = sp.to_dense()
    for n in ("tsdf", "weight", "color"):
        m = inside.expand_as(getattr(dn, n))
        assert same_bits(getattr(back, n)[m], getattr(dn, n)[m]), n
    dn.weight = torch.where(inside, dn.weight, torch.zeros_like(dn.weight))      # cells with all 8 corners allocated
    V, F, Cs = sp.extract()
    V2, F2, C2 = dn.extract()
    print("sphere from four cameras: %d of %d blocks, %d vertices, %d faces" % (sp.n_blocks, alloc.size, len(V), len(F)))
    assert len(F) > 5000 and same_bits(V, V2) and same_bits(Cs, C2)
    rows = lambda F: np.unique(F.cpu().numpy(), axis=0)
    assert len(F) == len(F2) and np.array_equal(rows(F), rows(F2))
    assert TR.closed_and_consistent(F.cpu().numpy())


def test_max_blocks_exceeded_raises_and_leaves_the_volume_as_it_was(lib):
    lat, views, _, _ = case((130, 33, 9), (20, 33))
    free, _ = volumes(lat, views[0], True)
    fuse(free, views[0])
    first = free.n_blocks
    fuse(free, views[1])
    assert free.n_blocks > first > 1
    sp, _ = volumes(lat, views[0], True, max_blocks=first - 1)
    before = pool_bits(sp) + [bits(sp.tsdf).clone(), bits(sp.weight).clone(), bits(sp.color).clone()]
    with pytest.raises(ValueError, match="max_blocks = %d" % (first - 1)):
        fuse(sp, views[0])
    assert sp.n_blocks == 0 and int(sp.directory.max()) == -1
    assert same_pools(before, pool_bits(sp) + [bits(sp.tsdf), bits(sp.weight), bits(sp.color)])
    sp, _ = volumes(lat, views[0], True, max_blocks=first)
    fuse(sp, views[0])
    before = pool_bits(sp) + [bits(sp.tsdf).clone(), bits(sp.weight).clone(), bits(sp.color).clone()]
    with pytest.raises(ValueError, match="new blocks"):
        fuse(sp, views[1])
    assert sp.n_blocks == first and sp.capacity == first
    assert same_pools(before, pool_bits(sp) + [bits(sp.tsdf), bits(sp.weight), bits(sp.color)])
    # the pool grows by doubling
    small, _ = volumes(lat, views[0], True)
    small.n_blocks = 0
    small._allocate_pool(2)
    for v in views[:2]:
        fuse(small, v)
    assert small.capacity >= small.n_blocks and same_pools(pool_bits(small), pool_bits(free))


def test_bad_arguments_return_10001_and_write_nothing(lib):
    dims, hw = (20, 13, 9), (12, 16)
    lat, views, _, _ = case(dims, hw)
    view = views[1]
    sp, _ = volumes(lat, view, True)
    fuse(sp, views[0])
    n, cap = sp.n_blocks, sp.capacity
    state = lambda: pool_bits(sp) + [bits(sp.tsdf).clone(), bits(sp.weight).clone(), bits(sp.color).clone()]
    before = state()
    dv = maps(view)
    R, t = dev(np.asarray(view["R"]).reshape(-1)), dev(view["t"])
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    H, W = hw

    def integrate(**over):
        a = dict(nx=dims[0], voxel=lat["voxel"], n=n, cap=cap, coords=p(sp.block_coords), tsdf=p(sp.tsdf), weight=p(sp.weight),
                 color=p(sp.color), H=H, depth=p(dv["depth"]), image=p(dv["image"]), K=view["K"], R=p(R), trunc=view["trunc"],
                 alpha_min=0.5, near=0.01, depth_max=float("inf"), max_blocks=0)
        a.update(over)
        return lib.egs_sparsetsdf_integrate(a["nx"], dims[1], dims[2], *[float(v) for v in lat["origin"]], float(a["voxel"]),
                                            a["n"], a["cap"], a["coords"], a["tsdf"], a["weight"], a["color"], a["H"], W,
                                            a["depth"], p(dv["alpha"]), a["image"], p(dv["weight"]),
                                            *[float(v) for v in a["K"]], a["R"], p(t), float(a["trunc"]), a["alpha_min"],
                                            a["near"], a["depth_max"], a["max_blocks"], st)

    for kw in (dict(nx=0), dict(voxel=0.0), dict(voxel=float("nan")), dict(n=-1), dict(n=cap + 1), dict(cap=(1 << 22) + 1),
               dict(coords=None), dict(tsdf=None), dict(weight=None), dict(color=None), dict(image=None),
               dict(tsdf=C.c_void_p(sp.tsdf.data_ptr() + 4)), dict(weight=p(sp.tsdf)), dict(color=p(sp.weight)), dict(H=0),
               dict(depth=None), dict(K=(0.0, 1.0, 1.0, 1.0)), dict(R=None), dict(trunc=0.0), dict(trunc=float("inf")),
               dict(alpha_min=-0.5), dict(near=float("nan")), dict(depth_max=0.0), dict(max_blocks=-2), dict(max_blocks=1 << 20),
               dict(depth=p(sp.tsdf)), dict(image=p(sp.color))):
        assert integrate(**kw) == BAD_ARG, kw
        assert lib.egs_sparsetsdf_last_error_string().decode().startswith("egs_sparsetsdf error 10001: bad argument"), kw
        torch.cuda.synchronize()
        assert same_pools(before, state()), "%r: refused, yet the volume was written" % (kw,)
    flags = torch.zeros(sp.directory.numel(), dtype=torch.int32, device="cuda")
    fresh = torch.full_like(flags, -7)
    geo = (*dims, *[float(v) for v in lat["origin"]])
    tail = lambda trunc: (*[float(v) for v in view["K"]], p(R), p(t), trunc, 0.5, 0.01, float("inf"))
    for vox, trunc, fl in ((0.0, view["trunc"], flags), (lat["voxel"], 0.0, flags), (lat["voxel"], view["trunc"], None),
                           (lat["voxel"], 3000.0 * lat["voxel"], flags), (lat["voxel"], view["trunc"], dv["depth"])):
        assert lib.egs_sparsetsdf_touch(*geo, float(vox), H, W, p(dv["depth"]), p(dv["alpha"]), p(dv["weight"]),
                                        *tail(float(trunc)), p(fl), st) == BAD_ARG
    assert lib.egs_sparsetsdf_mark(*dims, p(flags), p(sp.directory), None, st) == BAD_ARG
    assert lib.egs_sparsetsdf_mark(*dims, p(flags), p(sp.directory), p(flags), st) == BAD_ARG
    offsets = torch.zeros(flags.numel(), dtype=torch.int64, device="cuda")
    assert lib.egs_sparsetsdf_assign(*dims, p(fresh), p(offsets), n, n - 1, p(sp.directory), p(sp.block_coords), st) == BAD_ARG
    assert lib.egs_sparsetsdf_assign(*dims, p(fresh), p(offsets), n, cap, None, p(sp.block_coords), st) == BAD_ARG
    torch.cuda.synchronize()
    assert int(flags.max()) == 0 and int(fresh.min()) == -7 == int(fresh.max()) and same_pools(before, state())
    # an empty pool is a call that does nothing; the real call then does change the volume
    assert integrate(n=0) == 0
    torch.cuda.synchronize()
    assert same_pools(before, state())
    assert integrate() == 0
    torch.cuda.synchronize()
    assert not same_pools(before, state())


def test_trainer_extract_mesh_sparse_and_dense(lib):
    """the small trainer fixture of tests/test_gpu_trainer_mesh.py: ``sparse=True`` gives a mesh, the sparse volume's; the
    default call gives the dense manual loop's bits, as it always did"""
    from easygaussiansplatting_amd import gsplatcu
    from easygaussiansplatting_amd.function import Camera, GSFunction, GSRawFunction, RenderOptions
    from easygaussiansplatting_amd.mesh import SparseTSDFVolume, TSDFVolume
    from easygaussiansplatting_amd.trainer import Trainer
    from tests.test_gpu_trainer_mesh import BOUNDS, DIMS, N, ORIGIN, VOXEL, cameras, shell_scene
    gsplatcu.set_policy("gsplatcu")
    sc = shell_scene()
    cams = [Camera.from_scene(c) for c in cameras(sc.cam)]
    with torch.no_grad():
        leaves = (dev(sc.pws), dev(sc.shs), dev(sc.alphas).reshape(-1, 1), dev(sc.scales), dev(sc.rots))
        images = [GSFunction.apply(*leaves, torch.zeros((N, 2), device="cuda"), c, RenderOptions())[0].contiguous()
                  for c in cams]
    tr = Trainer(sc, cams, images, max_steps=10, view_streams=1)
    V, F, Cs = tr.extract_mesh(voxel_size=VOXEL, bounds=BOUNDS)
    Vs, Fs, Css = tr.extract_mesh(voxel_size=VOXEL, bounds=BOUNDS, sparse=True)
    assert len(Fs) > 1000 and Css.shape == Vs.shape and bool(torch.isfinite(Vs).all()) and int(Fs.max()) < len(Vs)
    dn, sp = TSDFVolume(ORIGIN, VOXEL, DIMS), SparseTSDFVolume(ORIGIN, VOXEL, DIMS)
    p = tr.params
    with torch.no_grad():
        for cam in cams:
            out = GSRawFunction.apply(p["pws"], p["low_shs"], p["high_shs"], p["alphas_raw"], p["scales_raw"],
                                      p["rots_raw"], torch.zeros((N, 2), device="cuda"), cam,
                                      RenderOptions(depth=True, alpha=True))
            dn.integrate(out[2], out[3], cam, image=out[0].contiguous())
            sp.integrate(out[2], out[3], cam, image=out[0].contiguous())
    V2, F2, C2 = dn.extract()
    assert len(F) > 1000 and torch.equal(F, F2) and same_bits(V, V2) and same_bits(Cs, C2)
    V3, F3, C3 = sp.extract()
    assert torch.equal(Fs, F3) and same_bits(Vs, V3) and same_bits(Css, C3)
    print("trainer: dense %d faces, sparse %d faces from %d of %d blocks" % (len(F), len(Fs), sp.n_blocks, sp.directory.numel()))
