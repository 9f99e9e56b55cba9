"""The block-allocated TSDF volume without a GPU: the float64 restatement of the touch rule
(tests/sparse_tsdf_ref.py) covers the truncation band on every case the GPU tests use, which all satisfy the coverage
condition include/egs_sparse_tsdf.h documents; a host program compiled from csrc/egs_tsdf_device.h with a plain C++
compiler still reproduces the dense reference of tests/tsdf_ref.py (the addressing argument changed nothing); the C surface
of libegs_sparsetsdf.so against its header, its argument checks (which return before any HIP call), and the host checks and
plain-indexing conversions of ``mesh.SparseTSDFVolume``."""
import inspect
import os
import re
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

from tests import sparse_tsdf_ref as SR
from tests import tsdf_ref as TR

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "egs_sparse_tsdf.h")
NAMES = sorted("egs_sparsetsdf_" + n for n in ("abi_version", "last_error_string", "touch", "mark", "assign", "integrate",
                                                "mesh_count", "mesh_emit"))
BAD_ARG, ERR_CAPACITY = 10001, 10003
_FAKE = 0x10000          # a "device pointer" no refused call dereferences
CASES = SR.case_list()


# ------------------------------------------------------------------------------------------------------- the touch rule
@pytest.mark.parametrize("dims,hw", CASES, ids=lambda v: "x".join(str(k) for k in v))
def test_the_dilated_touched_set_covers_the_band(dims, hw):
    """every block that holds a decided sample updated with t < 1 is in the restatement's dilated set -- none may be
    missing -- at a march step of a quarter voxel and of a sixteenth; the case satisfies the documented footprint condition"""
    lat = TR.make_lattice(dims)
    for view in SR.make_views(lat, hw):
        fp = SR.footprint(lat, view)
        assert fp <= SR.FOOTPRINT_LIMIT, "%s %s: the coverage condition's left side is %.2f" % (dims, view["cam"], fp)
        band = SR.band_blocks(lat, view)
        for step in (0.25, 0.0625):
            flags = SR.touch(lat, view, step)
            missing = band & ~SR.dilate(flags)
            print("%s %s %s step %g: footprint %.2f, %d flagged, %d band blocks, %d missing" % (
                dims, hw, view["cam"], step, fp, int(flags.sum()), int(band.sum()), int(missing.sum())))
            assert not missing.any()
        assert band.any() or dims == (1, 1, 1)


def test_the_cases_are_the_issues():
    assert {d for d, _ in CASES} == {(1, 1, 1), (8, 8, 8), (9, 8, 8), (20, 13, 9), (130, 33, 9)}
    assert {hw for _, hw in CASES} == {(12, 16), (20, 33)}
    lat = TR.make_lattice((20, 13, 9))
    front, oblique, inside = SR.make_views(lat, (12, 16))
    assert oblique["weight"] is not None and (oblique["alpha"][:, 8:] <= TR.ALPHA_MIN).all()
    assert inside["alpha"] is None and inside["depth_max"] == 1.5 and front["weight"] is None
    assert SR.block_dims((130, 33, 9)) == (17, 5, 2) and SR.block_dims((8, 8, 8)) == (1, 1, 1)
    # the helpers against each other
    m = np.zeros((2, 5, 17), bool)
    m[1, 2, 3] = True
    assert SR.dilate(m).sum() == 2 * 3 * 3 and SR.dilate(m, 2).sum() == 2 * 5 * 5
    assert np.array_equal(SR.blocks_of(SR.samples_of(m, (130, 33, 9))), m)


def test_the_end_to_end_scene_is_covered_and_closes():
    """the four-camera sphere of the GPU end-to-end test, in float64: the footprint condition, full band coverage, no block
    observed before the view that allocates it (so the sparse volume equals the dense one on its blocks), a closed mesh"""
    lat = TR.make_lattice(SR.E2E_DIMS)
    state = TR.new_state(SR.E2E_DIMS, color=False)
    alloc = np.zeros(SR.block_dims(SR.E2E_DIMS)[::-1], bool)
    for view in SR.e2e_views(lat):
        assert SR.footprint(lat, view) <= SR.FOOTPRINT_LIMIT
        new = SR.dilate(SR.touch(lat, view)) & ~alloc
        assert not ((state["weight"] > 0) & SR.samples_of(new, SR.E2E_DIMS)).any()
        alloc |= new
        assert not (SR.band_blocks(lat, view) & ~alloc).any()
        TR.integrate(state, lat, view)
    V, F, _ = TR.weld(TR.extract(lat, state["tsdf"].astype(np.float32), state["weight"].astype(np.float32)))
    assert len(F) > 5000 and TR.closed_and_consistent(F) and TR.euler(V, F) == 2


# ---------------------------------------------------------------------------------------------- the shared device header
def _host_check(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no C++ compiler: the host program of csrc/egs_tsdf_device.h cannot be built")
    exe = str(tmp_path_factory.mktemp("tsdf_host") / "tsdf_host_check")
    r = subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-o", exe,
                        os.path.join(REPO, "tests", "tsdf_host_check.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    return _host_check(tmp_path_factory)


@pytest.mark.parametrize("cam,hw,alpha,weight,color", [("front", (20, 33), True, False, True),
                                                      ("oblique", (12, 16), True, True, True),
                                                      ("inside", (20, 33), False, False, False)])
def test_the_host_program_of_the_device_header_reproduces_the_dense_reference(host_check, tmp_path, cam, hw, alpha, weight,
                                                                              color):
    """One view into the planes of ``smooth_field((20, 13, 9))`` -- a previous state with many crossings -- and the mesh of
    the result.  Integration under THE RULE of tests/tsdf_ref.py (4 x the float32 restatement's loss, at least an ulp; the
    same updated set on the decided samples).  Extraction against the float64 extraction of the program's own float32
    planes: the same triangles per cell in number and keys; coordinates within 2 float32 ulps of the largest coordinate
    (t, t * voxel and the sum are rounded once each: three half-ulps) and colours within 2 ulps of 1."""
    dims = (20, 13, 9)
    lat, f0, w0, c0 = TR.smooth_field(dims, seed=3, color=color)
    view = TR.make_view(lat, cam, hw[0], hw[1], alpha=alpha, weight=weight, half_alpha=(cam == "oblique"), seed=7,
                        depth_max=1.5 if cam == "inside" else None)
    H, W = hw
    N = dims[0] * dims[1] * dims[2]
    f32 = lambda a: np.ascontiguousarray(a, np.float32).tobytes()
    blob = struct.pack("8i", *dims, H, W, int(alpha), int(weight), int(color))
    blob += f32(list(lat["origin"]) + [lat["voxel"]] + list(view["K"]) + list(np.asarray(view["R"]).reshape(-1))
                + list(view["t"]) + [view["trunc"], view["alpha_min"], view["near"],
                                     np.inf if view["depth_max"] is None else view["depth_max"], 1.0])
    blob += f32(view["depth"]) + (f32(view["alpha"]) if alpha else b"") + (f32(view["weight"]) if weight else b"")
    blob += (f32(view["image"]) if color else b"") + f32(f0) + f32(w0) + (f32(c0) if color else b"")
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as fh:
        fh.write(blob)
    r = subprocess.run([host_check, src, dst], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    raw = open(dst, "rb").read()
    shape = dims[::-1]
    got = dict(tsdf=np.frombuffer(raw, np.float32, N, 0).reshape(shape),
               weight=np.frombuffer(raw, np.float32, N, 4 * N).reshape(shape),
               color=np.frombuffer(raw, np.float32, 3 * N, 8 * N).reshape((3,) + shape) if color else None)
    at = 4 * N * (5 if color else 2)
    T = int(np.frombuffer(raw, np.int64, 1, at)[0])
    verts = np.frombuffer(raw, np.float32, 9 * T, at + 8).reshape(T, 3, 3)
    keys = np.frombuffer(raw, np.int64, 3 * T, at + 8 + 36 * T).reshape(T, 3)
    cols = np.frombuffer(raw, np.float32, 9 * T, at + 8 + 60 * T).reshape(T, 3, 3) if color else None
    # integration
    start = lambda dt: dict(tsdf=f0.astype(dt), weight=w0.astype(dt), color=None if c0 is None else c0.astype(dt))
    s64, s32 = start(np.float64), start(np.float32)
    dec = TR.decided(lat, view)
    upd = TR.integrate(s64, lat, view)
    TR.integrate(s32, lat, view, np.float32)
    changed = got["weight"].view(np.int32) != w0.view(np.int32)
    assert upd.any() and np.array_equal(changed[dec], upd[dec])
    e_ref, e_got = TR.errors(s32, s64, dec & upd), TR.errors(got, s64, dec & upd)
    bound = TR.bounds(e_ref, s64)
    print("%s: %d updated | e_ref %s | e_host %s" % (cam, int(upd.sum()), e_ref, e_got))
    for k in e_got:
        assert e_got[k] <= bound[k], (k, e_got[k], bound[k])
    assert np.array_equal(got["tsdf"].view(np.int32)[~changed], f0.view(np.int32)[~changed])
    # extraction
    ref = TR.extract(lat, got["tsdf"], got["weight"], got["color"], 1.0)
    assert T == sum(len(t) for t in ref.values()) > 200
    big = max(float(np.abs(verts).max()), lat["voxel"])
    at, e_coord, e_col = 0, 0.0, 0.0
    for ci in sorted(ref):
        tris = ref[ci]
        sl = slice(at, at + len(tris))
        at += len(tris)
        assert set(keys[sl].ravel().tolist()) == {k for t in tris for k in t["keys"]}, ci
        by_key = {t["keys"][s]: (t["v"][s], None if t["c"] is None else t["c"][s]) for t in tris for s in range(3)}
        for n, (kk, vv) in enumerate(zip(keys[sl].ravel(), verts[sl].reshape(-1, 3))):
            rv, rc = by_key[int(kk)]
            e_coord = max(e_coord, float(np.abs(vv - rv).max()))
            if color:
                e_col = max(e_col, float(np.abs(cols[sl].reshape(-1, 3)[n] - rc).max()))
        assert np.abs(TR.area_vector(verts[sl]) - TR.area_vector([t["v"] for t in tris])).max() <= 1e-5 * lat["voxel"] ** 2
    print("%s: %d triangles | coordinates off by %.2e (ulp %.2e) | colours %.2e" % (cam, T, e_coord, TR.ulp32(big), e_col))
    assert e_coord <= 2 * TR.ulp32(big) and e_col <= 2 * TR.ulp32(1.0)


# ------------------------------------------------------------------------------------------------------------ the library
@pytest.fixture(scope="module")
def lib():
    from easygaussiansplatting_amd import _lib, _sparsetsdflib
    if not os.path.exists(_sparsetsdflib.LIB_PATH):
        _lib.build()
    return _sparsetsdflib.load()


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    return sorted(ln.split()[-1] for ln in out.splitlines() if ln.strip() and ln.split()[-1].startswith("egs_"))


def test_library_exports_what_its_header_declares(lib):
    from easygaussiansplatting_amd import _sparsetsdflib as SL
    assert _exports(SL.LIB_PATH) == NAMES
    assert sorted(SL.SIGNATURES) == NAMES
    hdr = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(set(re.findall(r"\b(egs_[a-z0-9_]+)\s*\(", code))) == NAMES
    assert re.search(r"^#define\s+EGS_SPARSETSDF_ABI_VERSION\s+1\s*$", hdr, re.M)
    assert lib.egs_sparsetsdf_abi_version() == 1 == SL.ABI_VERSION
    for name, value in (("ERR_CAPACITY", SL.ERR_CAPACITY), ("BLOCK", SL.BLOCK), ("BLOCK_SAMPLES", SL.BLOCK_SAMPLES),
                        ("MAX_DIRECTORY", SL.MAX_DIRECTORY), ("MAX_SLOTS", SL.MAX_SLOTS), ("MAX_BLOCKS", SL.MAX_BLOCKS),
                        ("MAX_MARCH", SL.MAX_MARCH)):
        assert re.search(r"^#define\s+EGS_SPARSETSDF_%s\s+%d\s*$" % (name, value), hdr, re.M), name
    assert SL.MAX_DIRECTORY == 1 << 27 and SL.MAX_SLOTS == 1 << 22 and "2^27" in hdr and "2^22" in hdr
    for fn in (n for n in NAMES if n not in ("egs_sparsetsdf_abi_version", "egs_sparsetsdf_last_error_string")):
        decl = re.search(r"int %s\((.*?)\);" % fn, code, re.S).group(1)
        assert len(decl.split(",")) == len(SL.SIGNATURES[fn][1]), fn
    assert "THE MARCH STEP IS ONE VOXEL" in hdr and "COVERAGE" in hdr


def test_the_dense_library_keeps_its_surface():
    from easygaussiansplatting_amd import _lib, _tsdflib
    if not os.path.exists(_tsdflib.LIB_PATH):
        _lib.build()
    assert _tsdflib.ABI_VERSION == 1 and _tsdflib.load().egs_tsdf_abi_version() == 1
    assert _exports(_tsdflib.LIB_PATH) == sorted(_tsdflib.SIGNATURES)
    assert not any("sparse" in n for n in _tsdflib.SIGNATURES) and not any("tsdf" in n for n in _lib.SIGNATURES)


def test_source_has_no_atomic_no_allocation_and_no_inline_assembly():
    src = open(os.path.join(REPO, "easygaussiansplatting_amd", "csrc", "egs_sparsetsdf.hip")).read()
    assert "getenv" not in src and re.findall(r"atomic\w*\(", src) == []
    assert "hipMalloc" not in src and "Synchronize" not in src and "asm" not in src
    assert "egs_tsdf::project_sample" in src and "egs_tsdf::decide_sample" in src and "egs_tsdf::blend" in src
    assert "egs_tsdf::emit_cell" in src
    dev = open(os.path.join(REPO, "easygaussiansplatting_amd", "csrc", "egs_tsdf_device.h")).read()
    assert "#pragma clang fp contract(off)" in dev


def test_bad_arguments_are_refused_without_a_device(lib):
    P = _FAKE
    inf, nan = float("inf"), float("nan")

    def refused(rc, kw):
        assert rc == BAD_ARG, (rc, kw)
        msg = lib.egs_sparsetsdf_last_error_string().decode()
        assert msg.startswith("egs_sparsetsdf error 10001: bad argument"), msg

    def touch(nx=20, ny=13, nz=9, o=(0.0, 0.0, 0.0), voxel=0.1, H=12, W=16, depth=P, alpha=2 * P, pw=3 * P,
              K=(10.0, 11.0, 8.0, 6.0), R=4 * P, t=5 * P, trunc=0.4, alpha_min=0.5, near=0.01, depth_max=inf, flags=6 * P):
        return lib.egs_sparsetsdf_touch(nx, ny, nz, *o, voxel, H, W, depth, alpha, pw, *K, R, t, trunc, alpha_min, near,
                                        depth_max, flags, None)

    for kw in (dict(nx=0), dict(nz=-1), dict(nx=1 << 16, ny=1 << 16, nz=1 << 16), dict(o=(nan, 0.0, 0.0)), dict(voxel=0.0),
               dict(voxel=inf), dict(H=0), dict(W=-1), dict(H=1 << 16, W=1 << 15), dict(depth=None), dict(depth=P + 2),
               dict(alpha=2 * P + 1), dict(pw=3 * P + 2), dict(K=(0.0, 11.0, 8.0, 6.0)), dict(K=(10.0, 11.0, nan, 6.0)),
               dict(R=None), dict(t=None), dict(trunc=0.0), dict(trunc=nan), dict(trunc=0.1 * 2049), dict(alpha_min=-0.1),
               dict(near=nan), dict(depth_max=0.0), dict(depth_max=nan), dict(flags=None), dict(flags=6 * P + 2),
               dict(flags=P), dict(flags=2 * P), dict(flags=4 * P)):
        refused(touch(**kw), kw)

    def mark(nx=20, ny=13, nz=9, flags=P, directory=2 * P, fresh=3 * P):
        return lib.egs_sparsetsdf_mark(nx, ny, nz, flags, directory, fresh, None)

    for kw in (dict(ny=0), dict(flags=None), dict(directory=None), dict(fresh=None), dict(fresh=P), dict(fresh=2 * P),
               dict(fresh=3 * P + 1)):
        refused(mark(**kw), kw)

    def assign(nx=20, ny=13, nz=9, fresh=P, offsets=2 * P, n=3, cap=8, directory=3 * P, coords=4 * P):
        return lib.egs_sparsetsdf_assign(nx, ny, nz, fresh, offsets, n, cap, directory, coords, None)

    for kw in (dict(nx=-3), dict(n=-1), dict(n=9), dict(cap=(1 << 22) + 1), dict(fresh=None), dict(offsets=None),
               dict(offsets=2 * P + 4), dict(directory=None), dict(directory=P), dict(coords=None), dict(coords=3 * P),
               dict(coords=P)):
        refused(assign(**kw), kw)
    assert assign(n=8, cap=8, coords=None) == 0          # a full pool: nothing to write

    def integrate(nx=20, ny=13, nz=9, o=(0.0, 0.0, 0.0), voxel=0.1, n=3, cap=8, coords=P, tsdf=2 * P, weight=3 * P,
                  color=4 * P, H=12, W=16, depth=5 * P, alpha=6 * P, image=7 * P, pw=8 * P, K=(10.0, 11.0, 8.0, 6.0),
                  R=9 * P, t=10 * P, trunc=0.4, alpha_min=0.5, near=0.01, depth_max=inf, max_blocks=0):
        return lib.egs_sparsetsdf_integrate(nx, ny, nz, *o, voxel, n, cap, coords, tsdf, weight, color, H, W, depth, alpha,
                                            image, pw, *K, R, t, trunc, alpha_min, near, depth_max, max_blocks, None)

    for kw in (dict(nx=0), dict(voxel=-1.0), dict(n=-1), dict(n=9), dict(cap=(1 << 22) + 1), dict(coords=None),
               dict(coords=P + 2), dict(tsdf=None), dict(weight=None), dict(tsdf=2 * P + 4), dict(weight=2 * P),
               dict(color=2 * P), dict(color=None), dict(image=None), dict(H=0), dict(depth=None), dict(R=None),
               dict(K=(10.0, -1.0, 8.0, 6.0)), dict(trunc=inf), dict(alpha_min=inf), dict(near=-1.0), dict(depth_max=-2.0),
               dict(max_blocks=-1), dict(max_blocks=8193), dict(tsdf=5 * P), dict(weight=7 * P), dict(color=9 * P),
               dict(tsdf=P)):
        refused(integrate(**kw), kw)
    assert integrate(n=0, coords=None) == 0              # an empty pool: no launch, so no device is needed either

    def count(nx=20, ny=13, nz=9, n=3, cap=8, directory=P, coords=2 * P, tsdf=3 * P, weight=4 * P, mw=1.0, counts=5 * P):
        return lib.egs_sparsetsdf_mesh_count(nx, ny, nz, n, cap, directory, coords, tsdf, weight, mw, counts, None)

    for kw in (dict(nz=0), dict(n=9), dict(directory=None), dict(coords=None), dict(tsdf=None), dict(weight=None),
               dict(mw=0.0), dict(mw=nan), dict(mw=inf), dict(counts=None), dict(counts=5 * P + 2), dict(counts=P),
               dict(counts=3 * P)):
        refused(count(**kw), kw)
    assert count(n=0, coords=None, counts=None) == 0

    def emit(nx=20, ny=13, nz=9, o=(0.0, 0.0, 0.0), voxel=0.1, n=3, cap=8, directory=P, coords=2 * P, tsdf=3 * P,
             weight=4 * P, color=5 * P, mw=1.0, offsets=6 * P, total=10, out_cap=10, verts=7 * P, keys=8 * P, colors=9 * P):
        return lib.egs_sparsetsdf_mesh_emit(nx, ny, nz, *o, voxel, n, cap, directory, coords, tsdf, weight, color, mw,
                                            offsets, total, out_cap, verts, keys, colors, None)

    for kw in (dict(nx=0), dict(o=(0.0, inf, 0.0)), dict(voxel=0.0), dict(n=9), dict(directory=None), dict(coords=None),
               dict(tsdf=None), dict(weight=None), dict(color=None), dict(colors=None), dict(mw=0.0), dict(total=-1),
               dict(total=3 * 512 * 12 + 1, out_cap=1 << 20), dict(out_cap=-1), dict(offsets=None), dict(offsets=6 * P + 4),
               dict(verts=None), dict(keys=None), dict(keys=8 * P + 4), dict(verts=8 * P), dict(colors=7 * P),
               dict(verts=3 * P), dict(keys=P), dict(colors=5 * P), dict(verts=6 * P)):
        refused(emit(**kw), kw)
    for cap in (9, 0):
        assert emit(out_cap=cap) == ERR_CAPACITY
        msg = lib.egs_sparsetsdf_last_error_string().decode()
        assert msg.startswith("egs_sparsetsdf error 10003") and "fewer triangles" in msg, msg
    assert emit(total=0, out_cap=0, verts=None, keys=None, color=None, colors=None) == 0


# ---------------------------------------------------------------------------------------------------- the Python surface
def test_signatures_and_documented_semantics():
    from easygaussiansplatting_amd import mesh
    from easygaussiansplatting_amd.trainer import Trainer
    p = inspect.signature(mesh.SparseTSDFVolume.__init__).parameters
    assert list(p) == ["self", "origin", "voxel_size", "dims", "trunc", "color", "max_blocks", "device"]
    assert [p[k].default for k in list(p)[4:]] == [None, True, None, "cuda"]
    dense = list(inspect.signature(mesh.TSDFVolume.integrate).parameters)
    sparse = inspect.signature(mesh.SparseTSDFVolume.integrate).parameters
    assert list(sparse)[:len(dense)] == dense
    for k in dense[4:]:
        assert sparse[k].default == inspect.signature(mesh.TSDFVolume.integrate).parameters[k].default, k
    p = inspect.signature(Trainer.extract_mesh).parameters
    assert p["sparse"].default is False and list(p)[:4] == ["self", "view_ids", "voxel_size", "bounds"]
    for doc in (mesh.SparseTSDFVolume.__doc__, Trainer.extract_mesh.__doc__, open(HEADER).read()):
        flat = " ".join(doc.split()).lower()
        assert "from the view that allocates it onwards" in flat, doc[:80]
    assert "all eight" in " ".join(mesh.SparseTSDFVolume.__doc__.split())
    for script, flag in (("train.py", "--mesh-sparse"), ("extract_mesh.py", "--sparse")):
        r = subprocess.run([sys.executable, os.path.join(REPO, "examples", script), "--help"], capture_output=True,
                           text=True, cwd=REPO)
        assert r.returncode == 0 and flag in r.stdout, (script, r.stderr)


def test_host_checks_and_the_dense_round_trip():
    """on the CPU device: the constructor's checks, a lattice no dense volume can hold, and ``from_dense`` / ``to_dense``
    (plain indexing) on a ragged lattice with a random block mask"""
    from easygaussiansplatting_amd.mesh import SparseTSDFVolume, TSDFVolume
    for kw, msg in ((dict(origin=(0, 0)), "origin must be three"), (dict(voxel_size=0.0), "voxel_size must be"),
                    (dict(dims=(4, 0, 4)), "dims must be three"), (dict(dims=(1 << 13, 1 << 13, 1 << 13)), "2\\^27"),
                    (dict(trunc=0.0), "trunc must be"), (dict(trunc=0.25 * 2049), "trunc must not exceed"),
                    (dict(max_blocks=0), "max_blocks must be"), (dict(max_blocks=2.5), "max_blocks must be")):
        args = dict(origin=(0.0, 0.0, 0.0), voxel_size=0.25, dims=(20, 13, 9), device="cpu")
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            SparseTSDFVolume(**args)
    big = SparseTSDFVolume((0.0, 0.0, 0.0), 0.005, (2048, 2048, 1024), device="cpu")       # 2^32 samples, 2^23 blocks
    assert big.n_blocks == 0 and tuple(big.directory.shape) == (128, 256, 256) and int(big.directory.max()) == -1
    assert big.capacity == 1024 and tuple(big.tsdf.shape) == (1024, 512) and tuple(big.color.shape) == (3, 1024, 512)
    with pytest.raises(ValueError, match="fewer than 2\\^31"):
        big.to_dense()
    assert SparseTSDFVolume((0, 0, 0), 0.25, (20, 13, 9), max_blocks=5, device="cpu").capacity == 5

    lat, f, w, c = TR.smooth_field((20, 13, 9), seed=5)
    dense = TSDFVolume(lat["origin"], lat["voxel"], lat["dims"], device="cpu")
    dense.tsdf, dense.weight, dense.color = torch.from_numpy(f), torch.from_numpy(w), torch.from_numpy(c)
    mask = torch.from_numpy(np.random.default_rng(1).random((2, 2, 3)) < 0.6)
    sp = SparseTSDFVolume.from_dense(dense, mask)
    n = int(mask.sum())
    assert 0 < n < 12 and sp.n_blocks == n and torch.equal(sp.directory >= 0, mask)
    coords = sp.block_coords[:n]
    assert torch.equal(coords, torch.nonzero(mask.reshape(-1)).reshape(-1).int())          # ascending block index
    assert torch.equal(sp.directory.reshape(-1)[coords.long()], torch.arange(n, dtype=torch.int32))
    # sample (lx, ly, lz) of a block sits at 64 lz + 8 ly + lx of its slot
    b = int(coords[-1])
    bx, by, bz = b % 3, (b // 3) % 2, b // 6
    for lx, ly, lz in ((0, 0, 0), (3, 2, 0), (1, 4, 0)):
        if 8 * bx + lx < 20 and 8 * by + ly < 13 and 8 * bz + lz < 9:
            assert float(sp.tsdf[n - 1, 64 * lz + 8 * ly + lx]) == float(f[8 * bz + lz, 8 * by + ly, 8 * bx + lx])
    back = sp.to_dense()
    inside = torch.from_numpy(SR.samples_of(mask.numpy(), (20, 13, 9)))
    for name, fill in (("tsdf", 1.0), ("weight", 0.0), ("color", 0.0)):
        got, want = getattr(back, name), getattr(dense, name)
        m = inside.expand_as(want)
        assert torch.equal(got[m], want[m]) and bool((got[~m] == fill).all()), name
    with pytest.raises(ValueError, match="block_mask must be"):
        SparseTSDFVolume.from_dense(dense, torch.ones((2, 2, 2), dtype=torch.bool))
    with pytest.raises(ValueError, match="must live on the GPU"):
        sp.extract()
    d, a, img = torch.ones((1, 6, 8)), torch.ones((1, 6, 8)), torch.ones((3, 6, 8))
    from easygaussiansplatting_amd import scene as S
    cam = S.Camera(8, 6, 10.0, 10.0, 4.0, 3.0, np.eye(3), np.array([0.0, 0.0, 2.0]))
    with pytest.raises(ValueError, match="image must be given iff"):
        sp.integrate(d, a, cam)
    with pytest.raises(ValueError, match="depth must live on the GPU"):
        sp.integrate(d, a, cam, image=img)
