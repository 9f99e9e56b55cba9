"""Mesh extraction (csrc/egs_tsdf.hip: k_mesh_count, k_mesh_emit) against the float64 marching tetrahedra of
tests/tsdf_ref.py, which is written from the geometry of a tetrahedron and holds no case table.  The reference is fed the
SAME float32 tsdf and weight, so every sign decision is identical and the comparison is exact where it can be.  Per cell:

  * the triangle count;
  * the set of vertex keys;
  * the sum of the triangles' area vectors (b - a) x (c - a) / 2 within 1e-5 of the voxel area: independent of how a quad
    is split, and wrong by whole triangles if an orientation is;

and per key the vertex coordinates within 1e-6 voxel and the colours within 1e-6.

WHERE THE COORDINATES ARE COMPARED.  A float32 coordinate of magnitude x is known to half an ulp, 2^-24 x at worst; that
is below 1e-6 voxel (with room for the rounding of t) only while |x| < 16 voxels.  So the 1e-6-voxel comparison is made
for the vertices all three of whose coordinates are below 16 voxels in magnitude -- every vertex of the small volumes, the
middle of the 67 x 9 x 5 one (its lattice is centred on the origin and its voxel 2^-4, so the sample positions are exact) --
and for EVERY vertex of the pattern volume, whose data are dyadic (origin 0, voxel 1, t a multiple of 1/8): there the
coordinates are exact and must be equal.  The other vertices are held by their keys and by the area vectors.

The C ABI is called directly on buffers the test owns: counts, verts, keys and colours NaN- / pattern-filled between guard
bands, the output buffers exactly ``total`` triangles long.  Every case also checks the triangle order (by cell: the
offsets are the scan of the counts and every triangle's keys belong to its cell), that a capacity one short is refused
with nothing written, and the guards.
"""
import ctypes as C

import numpy as np
import pytest

from tests import tsdf_ref as TR

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.loss_abi import PATTERN, dev, guarded, guards_intact  # noqa: E402  (needs torch)

ERR_CAPACITY = 10003
COORD_TOL, COLOR_TOL, AREA_TOL, EXACT_RANGE = 1e-6, 1e-6, 1e-5, 16.0


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from easygaussiansplatting_amd import _tsdflib
    return _tsdflib.load()


def untouched(inner):
    return bool((inner == PATTERN).all())


def abi_mesh(lib, lat, f, w, col=None, min_weight=1.0):
    """count, scan, emit on guarded buffers -> (counts [cells], verts [T,3,3], keys [T,3], colors or None) numpy; checks
    that every entry was written, that nothing else was, and the refusal of a capacity one short"""
    nx, ny, nz = lat["dims"]
    cells = max(nx - 1, 0) * max(ny - 1, 0) * max(nz - 1, 0)
    tf, tw = dev(f), dev(w)
    tc = None if col is None else dev(col)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    o = [float(v) for v in lat["origin"]]
    c_all, c_in = guarded(4 * max(cells, 1))
    assert lib.egs_tsdf_mesh_count(nx, ny, nz, p(tf), p(tw), float(min_weight), p(c_in), st) == 0
    torch.cuda.synchronize()
    assert guards_intact(c_all)
    if cells == 0:
        assert untouched(c_in), "counts written for a volume without a cell"
        counts = torch.zeros(0, dtype=torch.int32, device="cuda")
    else:
        counts = c_in.view(torch.int32).clone()
        assert int(counts.min()) >= 0 and int(counts.max()) <= 12, "a count never written, or out of range"
    ends = torch.cumsum(counts, 0, dtype=torch.int64)
    offsets = (ends - counts).contiguous()
    total = int(ends[-1]) if cells else 0
    v_all, v_in = guarded(36 * max(total, 1))
    k_all, k_in = guarded(24 * max(total, 1))
    g_all, g_in = guarded(36 * max(total, 1))
    outs = (v_in, k_in) + ((g_in,) if col is not None else ())

    def emit(capacity):
        rc = lib.egs_tsdf_mesh_emit(nx, ny, nz, *o, float(lat["voxel"]), p(tf), p(tw), p(tc), float(min_weight),
                                    p(offsets) if cells else None, total, capacity, p(v_in), p(k_in),
                                    p(g_in) if col is not None else None, st)
        torch.cuda.synchronize()
        for whole, nm in ((v_all, "verts"), (k_all, "keys"), (g_all, "colors")):
            assert guards_intact(whole), "the kernel wrote outside %s" % nm
        return rc

    if total > 0:
        assert emit(total - 1) == ERR_CAPACITY
        assert lib.egs_tsdf_last_error_string().decode().startswith("egs_tsdf error 10003")
        assert all(untouched(t) for t in outs), "a refused call wrote"
    assert emit(total) == 0
    if total == 0:
        assert all(untouched(t) for t in (v_in, k_in, g_in)), "an empty mesh wrote"
        return counts.cpu().numpy(), np.zeros((0, 3, 3), np.float32), np.zeros((0, 3), np.int64), None
    assert untouched(g_in) == (col is None)
    verts = v_in.view(torch.float32).reshape(total, 3, 3).cpu().numpy()
    keys = k_in.view(torch.int64).reshape(total, 3).cpu().numpy()
    cols = g_in.view(torch.float32).reshape(total, 3, 3).cpu().numpy() if col is not None else None
    # every byte of the outputs was written: the fill pattern is a float of about -2.9e-16 and a key of about -6.5e18
    fill32 = np.frombuffer(bytes([PATTERN] * 4), np.float32)[0]
    assert np.isfinite(verts).all() and not (verts == fill32).any() and (keys >= 0).all()
    assert cols is None or (np.isfinite(cols).all() and not (cols == fill32).any())
    return counts.cpu().numpy(), verts, keys, cols


def compare(lat, f, w, col, got, what, exact=False, min_weight=1.0):
    counts, verts, keys, cols = got
    nx, ny, nz = lat["dims"]
    ref = TR.extract(lat, f, w, col, min_weight)
    want_counts = np.zeros(len(counts), np.int64)
    for ci, tris in ref.items():
        want_counts[ci] = len(tris)
    assert np.array_equal(counts, want_counts), "%s: %d cells with another triangle count" % (
        what, int((counts != want_counts).sum()))
    off = np.concatenate([[0], np.cumsum(counts)])
    vox = lat["voxel"]
    o = np.asarray(lat["origin"], np.float64)
    e_coord = e_col = e_area = 0.0
    compared = 0
    for ci, tris in ref.items():
        sl = slice(off[ci], off[ci + 1])
        # the order is by cell: the triangles at the cell's offset are the cell's
        want_keys = {k for t in tris for k in t["keys"]}
        assert set(keys[sl].ravel().tolist()) == want_keys, "%s: cell %d has other vertex keys" % (what, ci)
        da = np.abs(TR.area_vector(verts[sl]) - TR.area_vector([t["v"] for t in tris])).max() / vox ** 2
        e_area = max(e_area, float(da))
        by_key = {t["keys"][s]: (t["v"][s], None if t["c"] is None else t["c"][s]) for t in tris for s in range(3)}
        for kk, vv, s in zip(keys[sl].ravel(), verts[sl].reshape(-1, 3), range(3 * len(tris))):
            rv, rc = by_key[int(kk)]
            if exact:
                assert np.array_equal(vv.astype(np.float64), rv), "%s: key %d is not exact" % (what, kk)
            if exact or np.abs(rv).max() < EXACT_RANGE * vox:
                e_coord = max(e_coord, float(np.abs(vv - rv).max() / vox))
                compared += 1
            if rc is not None:
                e_col = max(e_col, float(np.abs(cols[sl].reshape(-1, 3)[s] - rc).max()))
    # equal keys, equal bits
    flat_k, flat_v = keys.ravel(), verts.reshape(-1, 3)
    order = np.argsort(flat_k, kind="stable")
    same = flat_k[order][1:] == flat_k[order][:-1]
    assert np.array_equal(flat_v[order][1:][same].view(np.int32), flat_v[order][:-1][same].view(np.int32)), \
        "%s: two occurrences of a key differ" % what
    if cols is not None:
        flat_c = cols.reshape(-1, 3)
        assert np.array_equal(flat_c[order][1:][same].view(np.int32), flat_c[order][:-1][same].view(np.int32))
    print("%s: %d triangles in %d cells | coordinates %.2e voxel over %d vertices | colours %.2e | area vectors %.2e" % (
        what, len(keys), len(ref), e_coord, compared, e_col, e_area))
    assert e_area <= AREA_TOL, "%s: area vectors differ by %.3e voxel^2" % (what, e_area)
    assert e_coord <= COORD_TOL, "%s: coordinates differ by %.3e voxel" % (what, e_coord)
    assert e_col <= COLOR_TOL, "%s: colours differ by %.3e" % (what, e_col)
    return ref


@pytest.mark.parametrize("dims", [(1, 1, 1), (2, 1, 1), (2, 2, 1)], ids=lambda d: "%dx%dx%d" % d)
def test_a_volume_without_a_cell_gives_no_triangle(lib, dims):
    nx, ny, nz = dims
    lat = dict(dims=dims, origin=[0.0, 0.0, 0.0], voxel=1.0)
    f = np.where(np.arange(nx * ny * nz).reshape(nz, ny, nx) % 2 == 0, -1.0, 1.0).astype(np.float32)
    counts, verts, keys, _ = abi_mesh(lib, lat, f, np.full((nz, ny, nx), 2.0, np.float32))
    assert len(counts) == 0 and len(verts) == 0 and len(keys) == 0


@pytest.mark.parametrize("color", [False, True], ids=["plain", "color"])
@pytest.mark.parametrize("dims", [(2, 2, 2), (3, 2, 2), (5, 4, 3), (67, 9, 5)], ids=lambda d: "%dx%dx%d" % d)
def test_cells_match_the_reference(lib, dims, color):
    lat, f, w, col = TR.smooth_field(dims, seed=3, color=color)
    got = abi_mesh(lib, lat, f, w, col)
    ref = compare(lat, f, w, col, got, "%dx%dx%d" % dims)
    assert sum(len(t) for t in ref.values()) > 0
    if dims == (67, 9, 5):
        assert sum(len(t) for t in ref.values()) > 5000 and {len(t) for t in ref.values()} >= {2, 4, 6, 8}


def test_pattern_volume(lib):
    """all 256 corner sign patterns (cell 2k carries pattern k), on dyadic data: coordinates are exact"""
    lat, f, w = TR.pattern_volume()
    assert TR.corner_patterns(f)[0, 0, ::2].tolist() == list(range(256))
    got = abi_mesh(lib, lat, f, w)
    compare(lat, f, w, None, got, "pattern volume", exact=True)
    # (corner 0 alone is cut off in all six tetrahedra, corner 1 alone in the two that start along x)
    assert got[0][0] == 0 and got[0][2 * 255] == 0 and got[0][2 * 1] == 6 and got[0][2 * 2] == 2


def test_zero_counts_as_outside_and_weight_holes_emit_nothing(lib):
    lat, f, w, col = TR.smooth_field((5, 4, 3), seed=1)
    g, h = f.copy(), f.copy()
    g[1, 1, 1], h[1, 1, 1] = 0.0, 0.5
    g[0, 2, 3], h[0, 2, 3] = -0.0, 0.25           # (-0 < 0 is false too)
    got0 = abi_mesh(lib, lat, g, w, col)
    compare(lat, g, w, col, got0, "a corner at 0")
    got1 = abi_mesh(lib, lat, h, w, col)
    assert np.array_equal(got0[0], got1[0]) and np.array_equal(got0[2], got1[2])          # counts and keys
    w2 = w.copy()
    w2[1, 1, 1], w2[2, 3, 4] = 0.5, np.nan
    holes = abi_mesh(lib, lat, f, w2, col)
    full = abi_mesh(lib, lat, f, w, col)
    compare(lat, f, w2, col, holes, "weight holes")
    touched = [TR.cell_index(lat, (x, y, z)) for x in (0, 1) for y in (0, 1) for z in (0, 1)] + \
              [TR.cell_index(lat, (3, 2, 1))]
    assert (holes[0][touched] == 0).all() and full[0][touched].sum() > 0
    rest = np.setdiff1d(np.arange(len(full[0])), touched)
    assert np.array_equal(holes[0][rest], full[0][rest])
    # min_weight decides: with 0.25 the first hole is none (the NaN stays one)
    low = abi_mesh(lib, lat, f, w2, col, min_weight=0.25)
    compare(lat, f, w2, col, low, "min_weight 0.25", min_weight=0.25)
    assert low[0][touched[:8]].sum() == full[0][touched[:8]].sum() and low[0][touched[8]] == 0


def test_sphere_is_closed_outward_and_a_sphere(lib):
    """33^3 through ``mesh.TSDFVolume.extract``: the welded mesh is closed, every edge run through once each way, outward
    oriented, and V - E + F = 2"""
    from easygaussiansplatting_amd.mesh import TSDFVolume
    lat, f, w = TR.sphere_volume(33, 0.6)
    vol = TSDFVolume(lat["origin"], lat["voxel"], lat["dims"], color=False)
    vol.tsdf.copy_(dev(f))
    vol.weight.copy_(dev(w))
    V, F, Cc = vol.extract()
    assert Cc is None and V.dtype == torch.float32 and F.dtype == torch.int64
    V, F = V.cpu().numpy().astype(np.float64), F.cpu().numpy()
    assert len(F) > 3000 and int(F.max()) == len(V) - 1 and len(np.unique(F)) == len(V)
    assert TR.closed_and_consistent(F), "the welded mesh is not closed"
    assert TR.euler(V, F) == 2
    centre = np.array([0.013, -0.021, 0.008])
    tri = V[F]
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    assert (np.einsum("ij,ij->i", nrm, tri.mean(1) - centre) > 0).all(), "a face looks inwards"
    vol_mesh = TR.signed_volume(V, F)
    L = np.sqrt(3.0) * lat["voxel"]
    delta = L * L / (8.0 * (0.6 - L))                    # the bound of tests/test_tsdf_cpu.py
    assert 4 / 3 * np.pi * (0.6 - 2 * delta) ** 3 <= vol_mesh <= 4 / 3 * np.pi * 0.6 ** 3
    # the triangle soup in cell order: welding by key is all extract() adds
    verts, keys, _ = vol.extract_triangles()
    cells = keys.cpu().numpy() // 7
    assert len(verts) == len(F)
    with_color = TSDFVolume(lat["origin"], lat["voxel"], lat["dims"])
    with_color.tsdf.copy_(dev(f))
    with_color.weight.copy_(dev(w))
    with_color.color.copy_(torch.rand(with_color.color.shape, device="cuda"))
    V2, F2, C2 = with_color.extract()
    assert torch.equal(F2.cpu(), torch.from_numpy(F)) and tuple(C2.shape) == tuple(V2.shape)
    assert float(C2.min()) >= 0 and float(C2.max()) <= 1 and cells.min() >= 0
    # min_weight above every weight: an empty mesh, and it is a mesh
    V0, F0, _ = vol.extract(min_weight=5.0)
    assert tuple(V0.shape) == (0, 3) and tuple(F0.shape) == (0, 3)
