"""Vertex-clustering simplification without a GPU: the reference of tests/mesh_simplify_ref.py against itself
on every shared case (no degenerate and no duplicate face, every vertex referenced and inside its cell's closed box, kept
faces in their order, a second application with placement "mean" changes nothing where the clusters are singletons), the face
counts and radial errors of the sphere, the corner condition, the C surface of libegs_simplify.so against
include/egs_simplify.h and its argument checks (which return before any HIP call), and the host checks of ``mesh``."""
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import mesh_simplify_ref as SR

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "egs_simplify.h")
NAMES = sorted(["egs_simplify_abi_version", "egs_simplify_last_error_string", "egs_simplify_keys",
                "egs_simplify_vertex_quadrics", "egs_simplify_clusters", "egs_simplify_remap_faces",
                "egs_simplify_keep_flags"])
BAD_ARG = 10001
_FAKE = 0x10000          # a "device pointer" no refused call dereferences
CASES = list(SR.BUILDERS)


# ------------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("placement", SR.PLACEMENTS)
@pytest.mark.parametrize("name", CASES)
def test_reference_output_invariants(name, placement):
    c = SR.case(name)
    r = c[placement]
    V, F = r["V"], r["F"]
    assert V.dtype == np.float32 and F.dtype == np.int64 and r["C"].shape == V.shape
    assert (r["Vk"], r["Fk"]) == (len(V), len(F))
    # no degenerate face, no two faces with the same rotated triple, smallest index first
    assert len(F) == 0 or ((F[:, 0] != F[:, 1]) & (F[:, 1] != F[:, 2]) & (F[:, 0] != F[:, 2])).all()
    assert len(F) == 0 or ((F[:, 0] < F[:, 1]) & (F[:, 0] < F[:, 2])).all()
    assert len(np.unique(F, axis=0)) == len(F)
    # every vertex referenced, indices in range
    assert len(np.unique(F)) == len(V) and (len(F) == 0 or (F.min() == 0 and F.max() == len(V) - 1))
    # every vertex inside its cell's closed box (up to the one rounding to float32), in ascending key order
    kept = r["uniq"][r["ckeep"].astype(bool)]
    assert (np.diff(kept) > 0).all()
    cen = SR.centres(kept, c["origin"], c["cell"])
    slack = SR.ulp32(np.abs(c["V"]).max()) if len(c["V"]) else 0.0
    assert len(V) == 0 or float((np.abs(V.astype(np.float64) - cen) - 0.5 * c["cell"]).max()) <= slack
    # kept faces in their original order: each names the clusters of the original face with the smallest kept index
    fk = np.nonzero(r["fkeep"])[0]
    assert (np.diff(fk) > 0).all() and len(fk) == len(F)
    new = np.cumsum(r["ckeep"]) - 1
    if len(F):
        orig = new[r["cluster"][c["F"][fk]]]
        for k in range(3):          # the same cyclic order
            rolled = np.roll(orig, -k, axis=1)
            hit = (rolled == F).all(1)
            orig_ok = hit if k == 0 else (orig_ok | hit)
        assert orig_ok.all()
    # of equal rotated triples the first was kept: no valid dropped face precedes the kept one of its triple
    valid = r["valid"].astype(bool)
    first = {}
    for f in np.nonzero(valid)[0]:
        first.setdefault((r["hi"][f], r["lo"][f]), f)
    assert sorted(first.values()) == fk.tolist()
    assert r["degenerate"] + r["duplicate"] + len(F) == len(c["F"])
    assert sum(r["placed_counts"]) == r["clusters"] and (placement != "mean" or r["placed_counts"][0] == r["clusters"])
    assert np.isfinite(V).all() and np.isfinite(r["C"]).all()


@pytest.mark.parametrize("name", CASES)
def test_a_second_application_changes_nothing_on_singleton_clusters(name):
    c = SR.case(name)
    V, F, C = c["quadric"]["V"], c["quadric"]["F"], c["quadric"]["C"]
    # every output vertex keys back into its own cell: the clusters of the output are singletons in the same order.  (A
    # vertex clamped onto the upper wall of its cell belongs to the neighbour by the floor rule: such a mesh is left out.)
    keys = SR.cell_keys(V, c["origin"], c["cell"])
    singletons = np.array_equal(keys, c["quadric"]["uniq"][c["quadric"]["ckeep"].astype(bool)])
    if name in ("corner", "sphere-floaters@3", "fan-5000", "ties", "opposite", "same-rotation", "disjoint-1", "big-index"):
        assert singletons, name
    if not singletons:
        return
    V2, F2, C2 = SR.simplify(V, F, C, c["cell"], c["origin"], "mean")
    again = SR.simplify(V, F, C, c["cell"], c["origin"], "quadric", full=True)[3]
    assert np.array_equal(F2, F) and np.array_equal(V2.view(np.int32), V.view(np.int32))
    assert np.array_equal(C2.view(np.int32), C.view(np.int32))
    assert np.array_equal(again["F"], F)


def test_the_documented_face_counts_of_the_sphere():
    V, F = SR.sphere_largest()
    assert len(F) == 10364
    assert abs(SR.SPHERE_VOXEL - 0.075) < 1e-8
    for k, want in ((1, 1964), (2, 535), (3, 251)):
        for placement in SR.PLACEMENTS:
            got = SR.simplify(V, F, None, k * SR.SPHERE_VOXEL, SR.SPHERE_ORIGIN, placement)
            assert len(got[1]) == want, (k, placement, len(got[1]))


def test_quadric_placement_beats_the_mean_on_the_sphere():
    V, F = SR.sphere_largest()
    for k in (1, 2):
        q = SR.radial_error(SR.simplify(V, F, None, k * SR.SPHERE_VOXEL, SR.SPHERE_ORIGIN, "quadric")[0]) / SR.SPHERE_VOXEL
        m = SR.radial_error(SR.simplify(V, F, None, k * SR.SPHERE_VOXEL, SR.SPHERE_ORIGIN, "mean")[0]) / SR.SPHERE_VOXEL
        print("%d-voxel cells: mean radial error %.4f voxels (quadric), %.4f (mean)" % (k, q, m))
        assert q < m
        if k == 1:
            assert abs(q - 0.004) < 0.001 and abs(m - 0.014) < 0.001          # the figures the design quotes


def test_the_corner_condition():
    """three orthogonal, equally weighted planes through the corner: the regulariser pulls the optimum towards the cell
    mean by rho / (1 + rho) ~ 3e-3 of the mean's offset (~ 0.03), i.e. ~ 1e-4: ten times inside 0.01 x cell"""
    c = SR.case("corner")
    dist = lambda V: float(np.linalg.norm(V.astype(np.float64) - SR.CORNER, axis=1).min())
    dq, dm = dist(c["quadric"]["V"]), dist(c["mean"]["V"])
    print("corner: quadric %.2e, mean %.2e from the corner (cell %.1f)" % (dq, dm, SR.CORNER_CELL))
    assert dq <= 0.01 * SR.CORNER_CELL < dm
    assert dq < 2e-4 and dm > 0.02
    # the corner shares its cell with its neighbours, and no vertex lies on a cell boundary
    q = (c["V"].astype(np.float64) - np.array(c["origin"])) / c["cell"]
    assert float(np.abs(q - np.round(q)).min()) > 0.01
    assert int((SR.cell_keys(c["V"], c["origin"], c["cell"]) == SR.cell_keys(SR.CORNER[None], c["origin"], c["cell"])[0]).sum()) == 7


def test_special_cases():
    r = SR.case("one-cell")["quadric"]
    assert (r["Vk"], r["Fk"], r["clusters"], r["degenerate"]) == (0, 0, 1, 4) and r["V"].shape == (0, 3)
    r = SR.case("disjoint-0")["quadric"]
    assert (r["Vk"], r["Fk"], r["clusters"]) == (0, 0, 0)
    r = SR.case("opposite")["quadric"]          # faces 0 and 1 have opposite orientations: both stay; face 2 repeats face 0
    assert r["fkeep"].tolist() == [1, 1, 0] and r["F"].tolist() == [[0, 1, 2], [0, 2, 1]]
    r = SR.case("same-rotation")["quadric"]     # three rotations of one triple, its reverse, a collapsing face, the reverse again
    assert r["fkeep"].tolist() == [1, 0, 0, 1, 0, 0] and r["valid"].tolist() == [1, 1, 1, 1, 0, 1]
    assert r["rot"][:3].tolist() == [[0, 1, 2]] * 3 and r["rot"][3].tolist() == [0, 2, 1]
    # floor on boundaries: a coordinate that is an exact multiple of the cell belongs to the cell it opens
    c = SR.case("ties")
    i = SR.cell_indices(c["V"], c["origin"], c["cell"])
    assert np.array_equal(i, np.floor((c["V"].astype(np.float64) + 0.5) * 4).astype(np.int64))
    assert (c["V"][:, 0] * 4 == np.round(c["V"][:, 0] * 4)).sum() > 30
    # indices next to 2^21 - 1 on all three axes, keys beyond 2^62
    c = SR.case("big-index")
    i = SR.key_indices(c["quadric"]["keys"])
    assert i.min() >= SR.INDEX_MAX - 8 and i.max() == SR.INDEX_MAX and int(c["quadric"]["keys"].max()) > 1 << 62
    assert np.array_equal(i, SR.cell_indices(c["V"], c["origin"], c["cell"]))
    # several per cent of the field's clusters clamp; a fan's hub row has 5 000 entries and its cells many members
    r = SR.case("field-17x15x13")["quadric"]
    assert r["placed_counts"][2] >= 0.02 * r["clusters"]
    assert np.bincount(SR.case("fan-5000")["quadric"]["cluster"]).max() > 100
    assert SR.case("unreferenced")["quadric"]["placed_counts"][3] == 7          # the vertices no face names


def test_clamped_keys_and_nan():
    V = np.array([[np.nan, -5.0, 1e30], [0.25, 0.5, 0.75]], np.float32)
    i = SR.cell_indices(V, (0.0, 0.0, 0.0), 0.25)
    assert i.tolist() == [[0, 0, SR.INDEX_MAX], [1, 2, 3]]


# ------------------------------------------------------------------------------------------------------------ the library
@pytest.fixture(scope="module")
def lib():
    from easygaussiansplatting_amd import _lib, _simplifylib
    if not os.path.exists(_simplifylib.LIB_PATH):
        _lib.build()
    return _simplifylib.load()


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    return sorted(ln.split()[-1] for ln in out.splitlines() if ln.strip() and ln.split()[-1].startswith("egs_"))


def test_library_exports_what_its_header_declares(lib):
    from easygaussiansplatting_amd import _simplifylib
    assert _exports(_simplifylib.LIB_PATH) == NAMES
    assert sorted(_simplifylib.SIGNATURES) == NAMES
    hdr = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(set(re.findall(r"\b(egs_[a-z0-9_]+)\s*\(", code))) == NAMES
    assert re.search(r"^#define\s+EGS_SIMPLIFY_ABI_VERSION\s+1\s*$", hdr, re.M)
    assert lib.egs_simplify_abi_version() == 1 == _simplifylib.ABI_VERSION
    for name, value in (("ERR_BAD_ARG", _simplifylib.ERR_BAD_ARG), ("MAX_BLOCKS", _simplifylib.MAX_BLOCKS),
                        ("KEY_BITS", _simplifylib.KEY_BITS), ("PLACE_QUADRIC", _simplifylib.PLACE_QUADRIC),
                        ("PLACE_MEAN", _simplifylib.PLACE_MEAN)):
        assert re.search(r"^#define\s+EGS_SIMPLIFY_%s\s+%d\s*$" % (name, value), hdr, re.M), name
    assert _simplifylib.ERR_BAD_ARG == BAD_ARG and _simplifylib.KEY_BITS == SR.BITS
    for fn in (n for n in NAMES if n not in ("egs_simplify_abi_version", "egs_simplify_last_error_string")):
        decl = re.search(r"int %s\((.*?)\);" % fn, code, re.S).group(1)
        assert len(decl.split(",")) == len(_simplifylib.SIGNATURES[fn][1]), fn
    assert "NOBODY HAS TUNED" in hdr and "TOPOLOGY" in hdr


def test_the_mesh_cleaning_library_is_untouched():
    from easygaussiansplatting_amd import _lib, _meshopslib
    if not os.path.exists(_meshopslib.LIB_PATH):
        _lib.build()
    assert len(_exports(_meshopslib.LIB_PATH)) == 7 and _meshopslib.ABI_VERSION == 1
    assert not any("simplify" in n for n in list(_meshopslib.SIGNATURES) + list(_lib.SIGNATURES))


def test_bad_arguments_are_refused_without_a_device(lib):
    P = _FAKE
    nan, inf = float("nan"), float("inf")

    def refused(rc):
        assert rc == BAD_ARG, rc
        msg = lib.egs_simplify_last_error_string().decode()
        assert msg.startswith("egs_simplify error 10001: bad argument"), msg

    def keys(V=9, v=P, o=(0.0, 0.0, 0.0), cell=0.5, out=2 * P, mb=0):
        return lib.egs_simplify_keys(V, v, *o, cell, out, mb, None)

    for kw in (dict(V=-1), dict(v=None), dict(out=None), dict(v=P + 2), dict(out=2 * P + 4), dict(out=P), dict(cell=0.0),
               dict(cell=-1.0), dict(cell=nan), dict(cell=inf), dict(o=(nan, 0.0, 0.0)), dict(o=(0.0, inf, 0.0)),
               dict(o=(0.0, 0.0, -inf)), dict(mb=-1), dict(mb=8193)):
        refused(keys(**kw))
    assert keys(V=0, v=None, out=None) == 0

    def quadrics(V=9, F=5, v=P, f=2 * P, rs=3 * P, rows=4 * P, k=5 * P, o=(0.0, 0.0, 0.0), cell=0.5, q=6 * P, mb=0):
        return lib.egs_simplify_vertex_quadrics(V, F, v, f, rs, rows, k, *o, cell, q, mb, None)

    for kw in (dict(V=-1), dict(F=-1), dict(v=None), dict(f=None), dict(rs=None), dict(rows=None), dict(k=None), dict(q=None),
               dict(q=6 * P + 4), dict(k=5 * P + 4), dict(rs=3 * P + 2), dict(q=P), dict(q=2 * P), dict(q=5 * P), dict(cell=0.0),
               dict(cell=nan), dict(o=(0.0, nan, 0.0)), dict(mb=-1), dict(mb=8193)):
        refused(quadrics(**kw))
    assert quadrics(V=0, v=None, k=None, q=None) == 0

    def clusters(V=9, F=5, Vc=4, v=P, c=2 * P, k=3 * P, ms=4 * P, m=5 * P, q=6 * P, f=7 * P, rs=8 * P, rows=9 * P,
                 o=(0.0, 0.0, 0.0), cell=0.5, place=0, ov=10 * P, oc=11 * P, pl=12 * P, mb=0):
        return lib.egs_simplify_clusters(V, F, Vc, v, c, k, ms, m, q, f, rs, rows, *o, cell, place, ov, oc, pl, mb, None)

    for kw in (dict(V=-1), dict(F=-1), dict(Vc=-1), dict(Vc=10), dict(v=None), dict(k=None), dict(ms=None), dict(m=None),
               dict(ov=None), dict(pl=None), dict(oc=None), dict(c=None), dict(place=2), dict(place=-1), dict(cell=0.0),
               dict(cell=nan), dict(o=(inf, 0.0, 0.0)), dict(q=None, f=None), dict(q=None, rs=None), dict(q=None, rows=None),
               dict(q=6 * P + 4), dict(ov=10 * P + 2), dict(pl=12 * P + 1), dict(ms=4 * P + 4), dict(ov=P), dict(oc=2 * P),
               dict(pl=6 * P), dict(oc=10 * P), dict(pl=11 * P), dict(mb=-1), dict(mb=8193)):
        refused(clusters(**kw))
    assert clusters(Vc=0, ov=None, oc=None, pl=None) == 0
    assert clusters(V=0, F=0, Vc=0, v=None, c=None, k=None, ms=None, m=None, q=None, f=None, rs=None, rows=None, ov=None,
                    oc=None, pl=None) == 0

    def remap(V=9, F=5, Vc=4, f=P, cl=2 * P, rot=3 * P, valid=4 * P, hi=5 * P, lo=6 * P, mb=0):
        return lib.egs_simplify_remap_faces(V, F, Vc, f, cl, rot, valid, hi, lo, mb, None)

    for kw in (dict(V=-1), dict(F=-1), dict(Vc=-1), dict(Vc=10), dict(f=None), dict(cl=None), dict(rot=None), dict(valid=None),
               dict(hi=None), dict(lo=None), dict(rot=3 * P + 4), dict(valid=4 * P + 2), dict(hi=5 * P + 4), dict(rot=P),
               dict(hi=2 * P), dict(lo=5 * P), dict(valid=3 * P), dict(mb=-1), dict(mb=8193)):
        refused(remap(**kw))
    assert remap(F=0, f=None, rot=None, valid=None, hi=None, lo=None) == 0

    def flags(F=5, Vc=4, order=P, rot=2 * P, valid=3 * P, hi=4 * P, lo=5 * P, fk=6 * P, ck=7 * P, mb=0):
        return lib.egs_simplify_keep_flags(F, Vc, order, rot, valid, hi, lo, fk, ck, mb, None)

    for kw in (dict(F=-1), dict(Vc=-1), dict(order=None), dict(rot=None), dict(valid=None), dict(hi=None), dict(lo=None),
               dict(fk=None), dict(ck=None), dict(order=P + 4), dict(fk=6 * P + 2), dict(ck=7 * P + 1), dict(fk=3 * P),
               dict(ck=6 * P), dict(ck=P), dict(fk=2 * P), dict(mb=-1), dict(mb=1 << 20)):
        refused(flags(**kw))
    assert flags(F=0, Vc=0, order=None, rot=None, valid=None, hi=None, lo=None, fk=None, ck=None) == 0


# ---------------------------------------------------------------------------------------------------- the Python surface
def test_signatures_and_documented_defaults():
    from easygaussiansplatting_amd import mesh
    from easygaussiansplatting_amd.trainer import Trainer
    sig = lambda f: inspect.signature(f).parameters
    p = sig(mesh.simplify_vertex_clustering)
    assert list(p) == ["vertices", "faces", "colors", "cell_size", "origin", "placement", "check", "return_info"]
    assert [p[k].default for k in list(p)[2:]] == [None, None, None, "quadric", True, False]
    p = sig(mesh.clean_mesh)
    assert list(p)[:7] == ["vertices", "faces", "colors", "min_faces", "keep_largest", "smooth_iterations", "normals"]
    assert (p["simplify_cell"].default, p["simplify_placement"].default) == (None, "quadric")
    p = sig(Trainer.extract_mesh)
    assert p["simplify_voxels"].default is None
    for doc in (mesh.__doc__, mesh.simplify_vertex_clustering.__doc__, Trainer.extract_mesh.__doc__):
        assert "nobody has tuned" in doc.lower() or "untuned" in doc.lower()
        assert "topology" in doc.lower()
    assert "three readbacks" in mesh.simplify_vertex_clustering.__doc__


def test_host_argument_checks():
    from easygaussiansplatting_amd import mesh
    V = torch.zeros((6, 3))
    F = torch.tensor([[0, 1, 2], [3, 4, 5]], dtype=torch.int64)
    S = mesh.simplify_vertex_clustering
    bad = [
        (lambda: S(V, F), "cell_size must be a finite number > 0"),
        (lambda: S(V, F, cell_size=0), "cell_size must be a finite number > 0"),
        (lambda: S(V, F, cell_size=float("nan")), "cell_size must be a finite number > 0"),
        (lambda: S(V, F, cell_size="wide"), "cell_size must be a finite number > 0"),
        (lambda: S(V, F, cell_size=0.1, placement="median"), "placement must be 'quadric' or 'mean'"),
        (lambda: S(V, F, cell_size=0.1, origin=(0, 0)), "origin must be three finite numbers"),
        (lambda: S(V, F, cell_size=0.1, origin=(0, float("inf"), 0)), "origin must be three finite numbers"),
        (lambda: S(V.double(), F, cell_size=0.1), "vertices must be torch.float32"),
        (lambda: S(V, F.int(), cell_size=0.1), "faces must be torch.int64"),
        (lambda: S(V, F, cell_size=0.1), "faces must live on the GPU"),
        (lambda: mesh.clean_mesh(V, F, simplify_cell=-1.0), "simplify_cell must be a finite number > 0"),
        (lambda: mesh.clean_mesh(V, F, simplify_cell=0.1, simplify_placement="x"), "simplify_placement must be"),
        (lambda: mesh.clean_mesh(V, F, simplify_cell=0.1), "faces must live on the GPU"),
    ]
    for call, msg in bad:
        with pytest.raises(ValueError, match=msg):
            call()
    with pytest.raises(TypeError, match="vertices must be a torch.Tensor"):
        S(V.numpy(), F, cell_size=0.1)


def test_the_examples_list_the_flags():
    r = subprocess.run([sys.executable, os.path.join(REPO, "examples", "train.py"), "--help"], capture_output=True,
                       text=True, cwd=REPO)
    assert r.returncode == 0, r.stderr
    assert "--mesh-simplify K" in r.stdout
    r = subprocess.run([sys.executable, os.path.join(REPO, "examples", "extract_mesh.py"), "--help"], capture_output=True,
                       text=True, cwd=REPO)
    assert r.returncode == 0, r.stderr
    for flag in ("--simplify K", "--simplify-placement {quadric,mean}"):
        assert flag in r.stdout, flag
