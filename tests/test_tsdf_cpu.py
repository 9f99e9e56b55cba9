"""TSDF fusion and mesh extraction without a GPU: the reference of tests/tsdf_ref.py against itself (the cap
on the samples its comparison rule leaves out, float32 against float64, the extraction on an analytic sphere, the pattern
volume), the PLY writer, the C surface of libegs_tsdf.so against include/egs_tsdf.h and its argument checks (which return
before any HIP call), the host checks of ``mesh`` and the frustum sub-box."""
import inspect
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import tsdf_ref as TR

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "egs_tsdf.h")
NAMES = sorted(["egs_tsdf_abi_version", "egs_tsdf_last_error_string", "egs_tsdf_integrate", "egs_tsdf_mesh_count",
                "egs_tsdf_mesh_emit"])
BAD_ARG, ERR_CAPACITY = 10001, 10003
_FAKE = 0x10000          # a "device pointer" no refused call dereferences
CASES = TR.case_list()


# ------------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("name", list(CASES))
def test_few_samples_are_left_out_and_float32_loses_little(name):
    """the cap of the module docstring of tests/tsdf_ref.py, from float64 alone; then the float32 restatement: the same
    updated samples where the decisions have margin, and the per-case loss the GPU bound is built from"""
    c = CASES[name]
    lat, view = TR.build_case(c)
    dec = TR.decided(lat, view)
    left_out = 1.0 - float(dec.mean())
    assert left_out <= TR.UNDECIDED_CAP, "%s: %.4f of the samples are undecided" % (name, left_out)
    s64, s32 = TR.new_state(c["dims"], c["color"]), TR.new_state(c["dims"], c["color"], np.float32)
    m64, m32 = TR.integrate(s64, lat, view), TR.integrate(s32, lat, view, np.float32)
    assert all(v is None or v.dtype == np.float32 for v in s32.values())
    assert np.array_equal(m64[dec], m32[dec]), name
    e = TR.errors(s32, s64, dec & m64)
    print("%s: updated %d of %d, left out %.4f, float32 loses %s" % (name, int(m64.sum()), m64.size, left_out, e))
    for k, v in e.items():
        assert v <= 64 * TR.ulp32(max(1.0, float(np.abs(s64[k]).max()))), (name, k, v)
    # untouched samples are what they were
    assert (s64["tsdf"][~m64] == 1).all() and (s64["weight"][~m64] == 0).all()


def test_the_cases_reach_every_rule():
    """over the cases: samples behind a camera, off the image, under alpha_min, in each of the three bands of sdf, with
    a zero weight, and every combination of the three options"""
    seen = dict(behind=0, off=0, low_alpha=0, back=0, band=0, front=0, zero_w=0)
    for name, c in CASES.items():
        lat, view = TR.build_case(c)
        p = TR.project(lat, view)
        seen["behind"] += int((~p["s1"]).sum())
        seen["off"] += int((p["s1"] & ~p["s2"]).sum())
        seen["low_alpha"] += int((p["s2"] & ~p["s3a"]).sum())
        with np.errstate(invalid="ignore"):
            seen["back"] += int((p["s3"] & (p["sdf"] < -p["trunc"])).sum())
            seen["band"] += int((p["s3"] & (np.abs(p["sdf"]) < p["trunc"])).sum())
            seen["front"] += int((p["s3"] & (p["sdf"] > p["trunc"])).sum())
            seen["zero_w"] += int((p["s3"] & (p["sdf"] >= -p["trunc"]) & ~(p["w"] > 0)).sum())
        if c["cam"] == "narrow" and c["dims"] == (130, 33, 9):
            assert (p["s1"] & ~p["s2"]).mean() > 0.5                 # most samples off the image
        if c["cam"] == "inside" and c["dims"] == (130, 33, 9):
            assert (~p["s1"]).mean() > 0.2
        if c["half_alpha"]:
            assert (view["alpha"][:, view["alpha"].shape[1] // 2:] <= TR.ALPHA_MIN).all()
    assert all(v > 0 for v in seen.values()), seen
    assert len({(c["color"], c["alpha"], c["weight"]) for c in CASES.values()}) == 8
    assert {c["hw"] for c in CASES.values()} == {(12, 16), (20, 33)}


def test_three_views_in_order_differ_from_another_order():
    lat = TR.make_lattice((9, 7, 5))
    views = [TR.make_view(lat, cam, 20, 33, weight=(k == 1), seed=k) for k, cam in enumerate(("front", "oblique", "inside"))]
    a, b = TR.new_state((9, 7, 5)), TR.new_state((9, 7, 5))
    for v in views:
        TR.integrate(a, lat, v)
    for v in views[::-1]:
        TR.integrate(b, lat, v)
    assert np.allclose(a["tsdf"], b["tsdf"], atol=1e-12) and np.array_equal(a["weight"] > 0, b["weight"] > 0)
    assert float(a["weight"].max()) > 2.0            # a sample seen by all three


def test_reference_extraction_of_a_sphere():
    """f = |p - c| - r at 17^3: closed, outward, and its volume within the lattice's discretisation of 4/3 pi r^3.

    THE BOUND.  Along a segment of length L that stays at least d from c, f is convex with f'' <= 1 / d, so the linear
    interpolant of an edge overestimates f by at most delta = L^2 / (8 d), and a mesh vertex P (a zero of the interpolant)
    has -delta <= f(P) <= 0.  A triangle's corners lie on edges of one tetrahedron, no two points of which are further
    apart than its longest edge, the cell's diagonal L = sqrt(3) h; f is convex, so f <= 0 on the triangle, and it falls
    below its corners' values by at most delta again.  With d >= r - L for every edge that crosses the surface the mesh
    lies between the spheres of radius r - 2 delta and r, and so does its volume."""
    n, r = 17, 0.6
    lat, f, w = TR.sphere_volume(n, r)
    cells = TR.extract(lat, f, w)
    V, F, C = TR.weld(cells)
    assert C is None and len(F) == sum(len(t) for t in cells.values()) > 500
    assert TR.closed_and_consistent(F) and TR.euler(V, F) == 2
    vol = TR.signed_volume(V, F)
    L = math.sqrt(3.0) * lat["voxel"]
    delta = L * L / (8.0 * (r - L))
    lo, hi = 4.0 / 3.0 * math.pi * (r - 2 * delta) ** 3, 4.0 / 3.0 * math.pi * r ** 3
    print("sphere: %d vertices, %d faces, volume %.5f in [%.5f, %.5f]" % (len(V), len(F), vol, lo, hi))
    assert lo <= vol <= hi                               # (positive: outward oriented as a whole)
    # ... and face by face: every normal points away from the centre
    tri = V[F]
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    assert (np.einsum("ij,ij->i", nrm, tri.mean(1) - np.array([0.013, -0.021, 0.008])) > 0).all()
    radius = np.linalg.norm(V - np.array([0.013, -0.021, 0.008]), axis=1)
    assert radius.max() <= r + 1e-6 and radius.min() >= r - delta - 1e-6
    assert not TR.closed_and_consistent(F[:-1]) and not TR.closed_and_consistent(np.vstack([F[:-1], F[-1:, ::-1]]))


def test_pattern_volume_holds_all_256_sign_patterns():
    lat, f, w = TR.pattern_volume()
    pat = TR.corner_patterns(f)
    assert pat.shape == (1, 1, 511)
    assert pat[0, 0, ::2].tolist() == list(range(256))
    cells = TR.extract(lat, f, w)
    for k in range(256):
        inside = bin(k).count("1")
        tris = cells.get(2 * k, [])
        assert (len(tris) == 0) == (inside in (0, 8)), k
        assert len(tris) <= 12
        for t in tris:       # dyadic data: every coordinate is exact in float32
            assert np.array_equal(t["v"].astype(np.float32).astype(np.float64), t["v"])
    # a corner at exactly 0 is outside, a hole in the weights empties the cells around it
    lat, f, w, _ = TR.smooth_field((5, 4, 3), seed=1)
    g = f.copy()
    g[1, 1, 1] = 0.0
    h = f.copy()
    h[1, 1, 1] = 0.5
    # (a cell's triangle count and the set of its vertex keys: how a quad is split is not part of the result)
    keys = lambda cells: {k: (len(v), sorted({key for t in v for key in t["keys"]})) for k, v in cells.items()}
    assert keys(TR.extract(lat, g, w)) == keys(TR.extract(lat, h, w))
    w2 = w.copy()
    w2[1, 1, 1] = 0.5
    holes = TR.extract(lat, f, w2)
    full = TR.extract(lat, f, w)
    touched = {TR.cell_index(lat, (x, y, z)) for x in (0, 1) for y in (0, 1) for z in (0, 1)}
    assert not touched & set(holes) and touched & set(full)
    assert {k: v for k, v in keys(full).items() if k not in touched} == keys(holes)


# ------------------------------------------------------------------------------------------------------------ PLY files
@pytest.mark.parametrize("with_color", [False, True])
def test_ply_round_trip(tmp_path, with_color):
    from easygaussiansplatting_amd.mesh import load_mesh_ply, save_mesh_ply
    lat, f, w = TR.sphere_volume(9, 0.55)
    V, F, _ = TR.weld(TR.extract(lat, f, w))
    V = V.astype(np.float32)
    C = np.random.default_rng(0).integers(0, 256, V.shape).astype(np.float32) / np.float32(255) if with_color else None
    path = str(tmp_path / "mesh.ply")
    save_mesh_ply(path, torch.from_numpy(V), torch.from_numpy(F), None if C is None else torch.from_numpy(C))
    head = open(path, "rb").read(400).decode("ascii", "replace")
    assert head.startswith("ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % len(V))
    assert "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % len(F) in head
    v, fc, c = load_mesh_ply(path)
    assert v.dtype == np.float32 and np.array_equal(v, V) and fc.dtype == np.int64 and np.array_equal(fc, F)
    assert (c is None) == (C is None) and (C is None or np.array_equal(c, C))
    assert os.path.getsize(path) == head.index("end_header\n") + 11 + len(V) * (15 if with_color else 12) + len(F) * 13
    save_mesh_ply(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64))       # an empty mesh is a file too
    v, fc, c = load_mesh_ply(path)
    assert v.shape == (0, 3) and fc.shape == (0, 3) and c is None
    for bad in (dict(vertices=V[:, :2], faces=F), dict(vertices=V, faces=F[:, :2]), dict(vertices=V[:5], faces=F),
                dict(vertices=V, faces=F, colors=np.zeros((3, 3), np.float32))):
        with pytest.raises(ValueError):
            save_mesh_ply(path, **bad)
    with open(path, "wb") as fh:
        fh.write(b"not a ply")
    with pytest.raises(ValueError, match="not a PLY"):
        load_mesh_ply(path)


# ------------------------------------------------------------------------------------------------------------ the library
@pytest.fixture(scope="module")
def lib():
    from easygaussiansplatting_amd import _lib, _tsdflib
    if not os.path.exists(_tsdflib.LIB_PATH):
        _lib.build()
    return _tsdflib.load()


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    return sorted(ln.split()[-1] for ln in out.splitlines() if ln.strip() and ln.split()[-1].startswith("egs_"))


def test_library_exports_what_its_header_declares(lib):
    from easygaussiansplatting_amd import _tsdflib
    assert _exports(_tsdflib.LIB_PATH) == NAMES
    assert sorted(_tsdflib.SIGNATURES) == NAMES
    hdr = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(set(re.findall(r"\b(egs_[a-z0-9_]+)\s*\(", code))) == NAMES
    assert re.search(r"^#define\s+EGS_TSDF_ABI_VERSION\s+1\s*$", hdr, re.M)
    assert lib.egs_tsdf_abi_version() == 1 == _tsdflib.ABI_VERSION
    for name, value in (("ERR_CAPACITY", _tsdflib.ERR_CAPACITY), ("MAX_BLOCKS", _tsdflib.MAX_BLOCKS),
                        ("CELL_TRIANGLES", _tsdflib.CELL_TRIANGLES)):
        assert re.search(r"^#define\s+EGS_TSDF_%s\s+%d\s*$" % (name, value), hdr, re.M), name
    for fn in ("egs_tsdf_integrate", "egs_tsdf_mesh_count", "egs_tsdf_mesh_emit"):
        decl = re.search(r"int %s\((.*?)\);" % fn, code, re.S).group(1)
        assert len(decl.split(",")) == len(_tsdflib.SIGNATURES[fn][1]), fn
    assert "NOBODY HAS TUNED" in hdr


def test_the_other_libraries_are_untouched():
    from easygaussiansplatting_amd import _lib, _normallosslib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    assert _lib.ABI_VERSION == 12 and _lib.load().egs_abi_version() == 12
    assert not any("tsdf" in n or "mesh" in n for n in _lib.SIGNATURES)
    assert _normallosslib.ABI_VERSION == 1 and not any("tsdf" in n for n in _normallosslib.SIGNATURES)


def test_source_has_no_atomic_no_allocation_and_no_inline_assembly():
    for name in ("egs_tsdf.hip", "egs_tsdf_device.h"):
        src = open(os.path.join(REPO, "easygaussiansplatting_amd", "csrc", name)).read()
        assert "getenv" not in src and re.findall(r"atomic\w*\(", src) == []
        assert "hipMalloc" not in src and "Synchronize" not in src and "asm" not in src


def test_bad_arguments_are_refused_without_a_device(lib):
    P = _FAKE
    inf = float("inf")

    def integrate(nx=9, ny=7, nz=5, o=(0.0, 0.0, 0.0), voxel=0.1, box=(0, 9, 0, 7, 0, 5), tsdf=P, weight=2 * P,
                  color=3 * P, H=12, W=16, depth=4 * P, alpha=5 * P, image=6 * P, pw=7 * P, K=(10.0, 11.0, 8.0, 6.0),
                  R=8 * P, t=9 * P, trunc=0.4, alpha_min=0.5, near=0.01, depth_max=inf, max_blocks=0):
        return lib.egs_tsdf_integrate(nx, ny, nz, *o, voxel, *box, tsdf, weight, color, H, W, depth, alpha, image, pw, *K,
                                      R, t, trunc, alpha_min, near, depth_max, max_blocks, None)

    def refused(rc):
        assert rc == BAD_ARG, rc
        msg = lib.egs_tsdf_last_error_string().decode()
        assert msg.startswith("egs_tsdf error 10001: bad argument"), msg

    for kw in (dict(nx=0), dict(ny=-1), dict(nz=0), dict(nx=1 << 16, ny=1 << 15, box=(0, 1, 0, 1, 0, 1)),
               dict(nx=1 << 11, ny=1 << 10, nz=1 << 10, box=(0, 1, 0, 1, 0, 1)),
               dict(o=(float("nan"), 0.0, 0.0)), dict(o=(0.0, inf, 0.0)), dict(voxel=0.0), dict(voxel=-1.0),
               dict(voxel=inf), dict(box=(-1, 9, 0, 7, 0, 5)), dict(box=(0, 10, 0, 7, 0, 5)), dict(box=(5, 4, 0, 7, 0, 5)),
               dict(box=(0, 9, 0, 8, 0, 5)), dict(box=(0, 9, 0, 7, 3, 2)), dict(box=(0, 9, 0, 7, 0, 6)),
               dict(tsdf=None), dict(weight=None), dict(tsdf=P + 4), dict(weight=2 * P + 8), dict(color=3 * P + 4),
               dict(weight=P), dict(color=P), dict(color=2 * P), dict(color=None), dict(image=None),
               dict(H=0), dict(W=-2), dict(H=1 << 16, W=1 << 15), dict(depth=None), dict(depth=4 * P + 2),
               dict(alpha=5 * P + 1), dict(image=6 * P + 2), dict(pw=7 * P + 3),
               dict(K=(0.0, 11.0, 8.0, 6.0)), dict(K=(10.0, -1.0, 8.0, 6.0)), dict(K=(10.0, 11.0, float("nan"), 6.0)),
               dict(K=(10.0, 11.0, 8.0, inf)), dict(R=None), dict(t=None), dict(R=8 * P + 2), dict(t=9 * P + 1),
               dict(trunc=0.0), dict(trunc=float("nan")), dict(trunc=inf), dict(alpha_min=-0.1), dict(alpha_min=inf),
               dict(near=-1.0), dict(near=float("nan")), dict(depth_max=0.0), dict(depth_max=-2.0),
               dict(depth_max=float("nan")), dict(max_blocks=-1), dict(max_blocks=8193),
               dict(tsdf=4 * P), dict(weight=5 * P), dict(color=6 * P), dict(tsdf=8 * P), dict(weight=9 * P)):
        refused(integrate(**kw))
    # an empty box is a call that does nothing: no launch, so no device is needed either
    assert integrate(box=(3, 3, 0, 7, 0, 5)) == 0 and integrate(box=(0, 9, 0, 7, 5, 5)) == 0

    def count(nx=9, ny=7, nz=5, tsdf=P, weight=2 * P, mw=1.0, counts=3 * P):
        return lib.egs_tsdf_mesh_count(nx, ny, nz, tsdf, weight, mw, counts, None)

    for kw in (dict(nx=0), dict(nz=-4), dict(tsdf=None), dict(weight=None), dict(tsdf=P + 1), dict(weight=2 * P + 2),
               dict(mw=0.0), dict(mw=-1.0), dict(mw=float("nan")), dict(mw=inf), dict(counts=None), dict(counts=3 * P + 2),
               dict(counts=P), dict(counts=2 * P)):
        refused(count(**kw))
    for dims in ((1, 1, 1), (2, 1, 1), (2, 2, 1), (1, 7, 5)):          # no cell: nothing to do, counts not looked at
        assert count(*dims, counts=None) == 0

    def emit(nx=9, ny=7, nz=5, o=(0.0, 0.0, 0.0), voxel=0.1, tsdf=P, weight=2 * P, color=3 * P, mw=1.0, offsets=4 * P,
             total=10, capacity=10, verts=5 * P, keys=6 * P, colors=7 * P):
        return lib.egs_tsdf_mesh_emit(nx, ny, nz, *o, voxel, tsdf, weight, color, mw, offsets, total, capacity, verts, keys,
                                      colors, None)

    for kw in (dict(nx=0), dict(o=(0.0, 0.0, float("nan"))), dict(voxel=0.0), dict(tsdf=None), dict(weight=None),
               dict(color=None), dict(colors=None), dict(color=3 * P + 2), dict(mw=0.0), dict(total=-1),
               dict(total=1 << 31, capacity=1 << 31), dict(capacity=-1), dict(total=8 * 6 * 4 * 12 + 1, capacity=1 << 20),
               dict(offsets=None), dict(offsets=4 * P + 4), dict(verts=None), dict(keys=None), dict(keys=6 * P + 4),
               dict(verts=5 * P + 2), dict(colors=7 * P + 1), dict(verts=6 * P), dict(colors=5 * P), dict(colors=6 * P),
               dict(verts=P), dict(keys=2 * P), dict(colors=3 * P), dict(verts=4 * P)):
        refused(emit(**kw))
    for cap in (9, 0):
        assert emit(capacity=cap) == ERR_CAPACITY
        msg = lib.egs_tsdf_last_error_string().decode()
        assert msg.startswith("egs_tsdf error 10003") and "fewer triangles" in msg, msg
    assert emit(total=0, capacity=0, verts=None, keys=None, color=None, colors=None) == 0
    assert emit(2, 2, 1, total=0, capacity=0) == 0


# ---------------------------------------------------------------------------------------------------- the Python surface
def test_signatures_and_documented_defaults():
    from easygaussiansplatting_amd import mesh
    from easygaussiansplatting_amd.trainer import Trainer
    p = inspect.signature(mesh.TSDFVolume.__init__).parameters
    assert list(p) == ["self", "origin", "voxel_size", "dims", "trunc", "color", "device"]
    assert (p["trunc"].default, p["color"].default, p["device"].default) == (None, True, "cuda")
    p = inspect.signature(mesh.TSDFVolume.integrate).parameters
    assert list(p) == ["self", "depth", "alpha", "cam", "image", "weight", "alpha_min", "near", "depth_max",
                       "clip_to_frustum"]
    assert [p[k].default for k in list(p)[4:]] == [None, None, 0.5, 0.01, None, True]
    assert inspect.signature(mesh.TSDFVolume.extract).parameters["min_weight"].default == 1.0
    assert list(inspect.signature(mesh.save_mesh_ply).parameters) == ["path", "vertices", "faces", "colors"]
    p = inspect.signature(Trainer.extract_mesh).parameters
    assert list(p)[:4] == ["self", "view_ids", "voxel_size", "bounds"] and list(p)[-1] == "integrate_kwargs"
    assert all(p[k].default is None for k in ("view_ids", "voxel_size", "bounds"))
    for doc in (mesh.__doc__, Trainer.extract_mesh.__doc__):
        assert "nobody has tuned" in doc.lower()
    assert (mesh.ALPHA_MIN, mesh.TRUNC_VOXELS, mesh.MIN_WEIGHT) == (0.5, 4.0, 1.0)


def test_host_argument_checks():
    from easygaussiansplatting_amd import scene as S
    from easygaussiansplatting_amd.mesh import TSDFVolume
    for kw, msg in ((dict(origin=(0, 0)), "origin must be three"), (dict(origin=(0, 0, float("nan"))), "origin must be"),
                    (dict(voxel_size=0.0), "voxel_size must be"), (dict(voxel_size=float("inf")), "voxel_size must be"),
                    (dict(dims=(4, 4)), "dims must be three"), (dict(dims=(4, 0, 4)), "dims must be three"),
                    (dict(dims=(2048, 1024, 1024)), "fewer than 2\\^31"), (dict(trunc=0.0), "trunc must be"),
                    (dict(trunc=float("nan")), "trunc must be"), (dict(origin="abc"), "must be three numbers")):
        args = dict(origin=(0.0, 0.0, 0.0), voxel_size=0.1, dims=(4, 5, 6), device="cpu")
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            TSDFVolume(**args)
    vol = TSDFVolume((0.0, -1.0, 2.0), 0.25, (4, 5, 6), device="cpu")
    assert vol.trunc == 1.0 and tuple(vol.tsdf.shape) == (6, 5, 4) and tuple(vol.color.shape) == (3, 6, 5, 4)
    assert float(vol.tsdf.min()) == 1.0 and float(vol.weight.max()) == 0.0 and float(vol.color.abs().max()) == 0.0
    assert TSDFVolume((0, 0, 0), 0.25, (4, 5, 6), trunc=0.3, color=False, device="cpu").color is None
    H, W = 6, 8
    d, a, img = torch.ones((1, H, W)), torch.ones((1, H, W)), torch.ones((3, H, W))
    cam = S.Camera(W, H, 10.0, 10.0, 4.0, 3.0, np.eye(3), np.array([0.0, 0.0, 2.0]))
    bad = [
        (dict(depth=torch.ones((3, H, W))), "depth must have shape"),
        (dict(depth=d.double()), "depth must be torch.float32"),
        (dict(alpha=torch.ones((1, H, W + 1))), "alpha must have shape"),
        (dict(alpha=a.half()), "alpha must be torch.float32"),
        (dict(image=torch.ones((H, W, 3))), "image must have shape"),
        (dict(image=img.double()), "image must be torch.float32"),
        (dict(image=None), "image must be given iff"),
        (dict(weight=torch.ones((H, W), dtype=torch.bool)), "weight must be torch.float32"),
        (dict(weight=torch.ones((1, H + 1, W))), "weight must have shape"),
        (dict(alpha_min=-1.0), "alpha_min must be finite"),
        (dict(near=float("nan")), "near must be finite"),
        (dict(depth_max=0.0), "depth_max must be"),
        (dict(cam=(10.0, 10.0, 4.0, 3.0)), "cam must carry its pose"),
        (dict(cam="x"), "cam must give finite intrinsics"),
    ]
    for kw, msg in bad:
        args = dict(depth=d, alpha=a, cam=cam, image=img)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            vol.integrate(**args)
    with pytest.raises(TypeError, match="depth must be a torch.Tensor"):
        vol.integrate(np.ones((H, W), np.float32), a, cam, image=img)
    with pytest.raises(ValueError, match="image must be given iff"):
        TSDFVolume((0, 0, 0), 0.25, (4, 5, 6), color=False, device="cpu").integrate(d, a, cam, image=img)
    # good arguments pass their own checks; the call is then refused for want of a GPU tensor
    for aa in (a, None):
        with pytest.raises(ValueError, match="depth must live on the GPU"):
            vol.integrate(d[0], aa, cam, image=img, weight=d[0])
    with pytest.raises(ValueError, match="min_weight must be"):
        vol.extract(min_weight=0.0)
    with pytest.raises(ValueError, match="must live on the GPU"):
        vol.extract()


FRUSTUM_CAMERAS = {      # eye, target, roll, focal multiple: inside, outside, grazing a face, looking away
    "inside": ((0.2, 0.1, -0.3), (1.0, 0.4, 0.2), 0.4, 0.7),
    "outside": ((3.1, 0.6, -0.9), (0.0, 0.1, 0.0), 0.3, 0.9),
    "grazing": ((-1.9, 1.22, 0.3), (1.5, 1.19, -0.2), 1.3, 1.5),
    "away": ((2.5, 0.3, 0.2), (5.0, 0.5, 0.1), 0.2, 1.0),
    "corner": ((1.6, 1.5, 1.7), (0.9, 1.0, 1.1), 2.0, 3.0),
}


@pytest.mark.parametrize("depth_max", [None, 1.7])
@pytest.mark.parametrize("cam", list(FRUSTUM_CAMERAS))
def test_the_frustum_box_holds_every_sample_the_view_can_update(cam, depth_max):
    """whatever the depth map says: the surface is put at every distance in turn"""
    from easygaussiansplatting_amd.mesh import frustum_box
    eye, target, roll, fmul = FRUSTUM_CAMERAS[cam]
    lat = TR.make_lattice((41, 37, 33))
    H, W = 20, 33
    R, t = TR.look_at(eye, target, roll)
    K = tuple(float(np.float32(v)) for v in (fmul * W, fmul * W, 0.5 * W - 0.4, 0.5 * H + 0.3))
    trunc = float(np.float32(4 * lat["voxel"]))
    box = frustum_box(lat["origin"], lat["voxel"], lat["dims"], K, (H, W), R, t, 0.01,
                      None if depth_max is None else depth_max + trunc)
    x0, x1, y0, y1, z0, z1 = box
    nx, ny, nz = lat["dims"]
    assert 0 <= x0 <= x1 <= nx and 0 <= y0 <= y1 <= ny and 0 <= z0 <= z1 <= nz
    inside = np.zeros((nz, ny, nx), bool)
    inside[z0:z1, y0:y1, x0:x1] = True
    reached = np.zeros_like(inside)
    for z in (0.05, 0.4, 1.0, 1.6, 2.5, 4.0, 9.0):
        view = dict(R=R, t=t, K=K, trunc=trunc, alpha_min=0.5, near=0.01, depth_max=depth_max, alpha=None, weight=None,
                    depth=np.full((H, W), z, np.float32))
        for dtype in (np.float64, np.float32):
            reached |= TR.project(lat, view, dtype)["upd"]
    print("%s: box %s holds %d samples, the view reaches %d" % (cam, box, int(inside.sum()), int(reached.sum())))
    assert not (reached & ~inside).any()
    if cam == "away":
        assert not reached.any() and not inside.any()
    else:
        assert reached.any()
    if cam == "grazing" or depth_max is not None:
        assert inside.sum() < inside.size                           # the box does cut the lattice down


def test_the_examples_list_the_flags():
    r = subprocess.run([sys.executable, os.path.join(REPO, "examples", "train.py"), "--help"], capture_output=True,
                       text=True, cwd=REPO)
    assert r.returncode == 0, r.stderr
    for flag in ("--mesh OUT.ply", "--mesh-voxel S"):
        assert flag in r.stdout, flag
    r = subprocess.run([sys.executable, os.path.join(REPO, "examples", "extract_mesh.py"), "--help"], capture_output=True,
                       text=True, cwd=REPO)
    assert r.returncode == 0, r.stderr
    for flag in ("--gs", "--path", "--out", "--voxel", "--alpha-min", "--min-weight"):
        assert flag in r.stdout, flag
