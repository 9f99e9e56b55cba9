"""Mesh cleaning without a GPU: the reference of tests/mesh_ops_ref.py against scipy and against itself (the
invariants of the labels and counts, the removal rules on the sphere with two floaters, the cap on the vertices its normal
comparison leaves out), the C surface of libegs_meshops.so against include/egs_meshops.h and its argument checks (which
return before any HIP call), the host checks of ``mesh`` and the PLY files with normals."""
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import mesh_ops_ref as MR
from tests import tsdf_ref as TR

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "egs_meshops.h")
NAMES = sorted(["egs_meshops_abi_version", "egs_meshops_last_error_string", "egs_meshops_components",
                "egs_meshops_keep_flags", "egs_meshops_compact", "egs_meshops_vertex_normals", "egs_meshops_taubin"])
BAD_ARG = 10001
_FAKE = 0x10000          # a "device pointer" no refused call dereferences
CASES = list(MR.BUILDERS)


# ------------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("name", CASES)
def test_reference_labels_are_scipys_and_the_counts_add_up(name):
    c = MR.case(name)
    V, F = len(c["V"]), c["F"]
    label, cf, cv = c["label"], c["comp_faces"], c["comp_verts"]
    idx = np.arange(V)
    assert (label <= idx).all() and np.array_equal(label[label], label)
    assert int(cf.sum()) == len(F) and int(cv.sum()) == V
    rep = label == idx
    assert (cf[~rep] == 0).all() and (cv[~rep] == 0).all() and (cv[rep] >= 1).all()
    if len(F):
        assert np.array_equal(label[F[:, 0]], label[F[:, 1]]) and np.array_equal(label[F[:, 0]], label[F[:, 2]])
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components
    e = np.concatenate([F[:, [0, 1]], F[:, [0, 2]]])
    g = sp.coo_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(V, V))
    n, lab = connected_components(g, directed=False) if V else (0, np.zeros(0, np.int64))
    assert n == int(rep.sum())
    first = np.full(n, V, np.int64)
    np.minimum.at(first, lab, idx)          # scipy's labels renamed to the minimum index of each component
    assert np.array_equal(first[lab], label)


def test_the_documented_component_sizes():
    c = MR.case("sphere-floaters")
    assert (len(c["V"]), len(c["F"])) == (5440, 10868)
    assert sorted(c["comp_faces"][c["comp_faces"] > 0].tolist()) == [108, 396, 10364]
    c = MR.case("field-17x15x13")
    assert len(c["F"]) == 13862 and sorted(c["comp_faces"][c["comp_faces"] > 0].tolist()) == [12, 30, 13820]
    c = MR.case("tets-300")
    assert (c["comp_faces"][c["comp_faces"] > 0] == 8).all() and int((c["comp_verts"] == 7).sum()) == 150
    c = MR.case("strip-70001")
    assert int((c["label"] == 0).sum()) == 70003 and c["comp_faces"][0] == 70001
    c = MR.case("fan-5000")
    assert c["comp_faces"][0] == 5000 and int(np.diff(MR.incidence(c["F"], len(c["V"]))[0]).max()) == 5000
    c = MR.case("unreferenced")
    lone = c["comp_faces"][c["label"] == np.arange(len(c["V"]))] == 0
    assert int(lone.sum()) == 7 and c["comp_faces"][0] == 0 and c["comp_faces"][len(c["V"]) - 1] == 0


def test_removal_on_the_sphere_with_two_floaters():
    c = MR.case("sphere-floaters")
    V, F, C, _ = MR.remove(c["V"], c["F"], c["C"], keep_largest=1)
    assert len(F) == 10364 and TR.closed_and_consistent(F) and TR.euler(V, F) == 2
    V2, F2, _, _ = MR.remove(c["V"], c["F"], min_faces=200)
    lab = MR.components(F2, len(V2))
    assert len(F2) == 10364 + 396 and sorted(lab[1][lab[1] > 0].tolist()) == [396, 10364]
    assert int(lab[2].sum()) == len(V2) and (lab[2][lab[0] == np.arange(len(V2))] > 1).all()
    both = MR.remove(c["V"], c["F"], min_faces=200, keep_largest=3)
    assert np.array_equal(both[1], F2)
    assert len(MR.remove(c["V"], c["F"], min_faces=500, keep_largest=2)[1]) == 10364


@pytest.mark.parametrize("name", CASES)
def test_removal_preserves_order_and_bits(name):
    c = MR.case(name)
    for mf, kl in MR.REMOVALS:
        vkeep, fkeep = MR.keep_flags(c["F"], len(c["V"]), mf, kl)
        V, F, C, N = MR.remove(c["V"], c["F"], c["C"], c["V"][:, ::-1], mf, kl)
        sel = np.nonzero(vkeep)[0]
        assert np.array_equal(V.view(np.int32), c["V"][sel].view(np.int32))
        assert np.array_equal(C.view(np.int32), c["C"][sel].view(np.int32))
        assert np.array_equal(N.view(np.int32), c["V"][sel][:, ::-1].view(np.int32))
        # the kept faces in their order, naming the same vertices as before
        assert np.array_equal(sel[F], c["F"][fkeep.astype(bool)])
        assert len(F) == 0 or (F.min() >= 0 and F.max() < len(V))
        # every kept vertex is referenced: unreferenced ones are gone
        assert len(np.unique(F)) == len(V)
        if kl is not None:
            assert len(np.unique(c["label"][sel])) <= kl


def test_keep_largest_ties_go_to_the_smaller_label():
    c = MR.case("equal-counts")
    cf, label = c["comp_faces"], c["label"]
    reps = np.nonzero(cf)[0]
    assert sorted(cf[reps].tolist()) == [1, 1, 1, 1, 4, 4, 4, 8]
    eight, fours, ones = reps[cf[reps] == 8], reps[cf[reps] == 4], reps[cf[reps] == 1]
    assert ones[0] < eight[0] < fours[0]              # the sizes are not in label order
    for k, want in ((1, eight), (2, np.concatenate([eight, fours[:1]])), (3, np.concatenate([eight, fours[:2]])),
                    (5, np.concatenate([eight, fours, ones[:1]]))):
        vkeep, _ = MR.keep_flags(c["F"], len(c["V"]), None, k)
        assert sorted(np.unique(label[vkeep.astype(bool)]).tolist()) == sorted(want.tolist()), k


@pytest.mark.parametrize("name", CASES)
def test_few_normals_are_undecided_and_float32_loses_little(name):
    """THE CAP, from float64 alone; then what the float32 restatements lose (printed: the GPU bounds are built from it)"""
    c = MR.case(name)
    n64, decided, has_face = MR.normals(c["V"], c["F"])
    left_out = float((~decided & has_face).sum()) / max(1, int(has_face.sum()))
    assert left_out <= MR.UNDECIDED_CAP, "%s: %.4f of the vertices with a face are undecided" % (name, left_out)
    ln = np.linalg.norm(n64, axis=1)
    assert (np.abs(ln[decided & has_face & (ln > 0)] - 1) < 1e-12).all() and (n64[~has_face] == 0).all()
    n32 = MR.normals(c["V"], c["F"], np.float32)[0]
    assert n32.dtype == np.float32
    e_n = float(np.abs(n32[decided] - n64[decided]).max()) if decided.any() else 0.0
    t64, t32 = MR.taubin(c["V"], c["F"], 2), MR.taubin(c["V"], c["F"], 2, dtype=np.float32)
    assert t32.dtype == np.float32
    e_t = float(np.abs(t32 - t64).max()) if len(t64) else 0.0
    print("%s: %d of %d vertices undecided; float32 loses %.2e on normals, %.2e on two Taubin iterations" % (
        name, int((~decided & has_face).sum()), int(has_face.sum()), e_n, e_t))
    assert np.array_equal(t64[~has_face], c["V"][~has_face].astype(np.float64))
    assert e_t <= 64 * MR.ulp32(max(1.0, float(np.abs(c["V"]).max()) if len(t64) else 1.0))


def test_sphere_normals_point_outward_and_smoothing_keeps_the_sphere():
    c = MR.case("sphere-floaters")
    V, F, _, _ = MR.remove(c["V"], c["F"], keep_largest=1)
    n, decided, has_face = MR.normals(V, F)
    assert decided.all() and has_face.all()
    radial = V.astype(np.float64) - np.array([0.013, -0.021, 0.008])
    radial /= np.linalg.norm(radial, axis=1, keepdims=True)
    assert float(np.einsum("ij,ij->i", n, radial).min()) > 0.9
    sm = MR.taubin(V, F, 10)
    r0, r1 = np.linalg.norm(V - np.array([0.013, -0.021, 0.008]), axis=1), np.linalg.norm(sm - np.array([0.013, -0.021, 0.008]), axis=1)
    assert r1.std() < r0.std() and abs(r1.mean() - 0.6) < 0.01          # smoother, and not shrunk


# ------------------------------------------------------------------------------------------------------------ PLY files
def test_ply_round_trip_with_normals(tmp_path):
    from easygaussiansplatting_amd.mesh import load_mesh_ply, save_mesh_ply, save_mesh_ply_with_normals
    c = MR.case("equal-counts")
    V, F, C = c["V"], c["F"], (np.round(c["C"] * 255) / 255).astype(np.float32)
    N = MR.normals(V, F)[0].astype(np.float32)
    path = str(tmp_path / "mesh.ply")
    for colors in (None, C):
        for normals in (None, N):
            save_mesh_ply_with_normals(path, torch.from_numpy(V.copy()), torch.from_numpy(F.copy()), colors, normals)
            head = open(path, "rb").read(600).decode("ascii", "replace")
            assert ("property float z\nproperty float nx\nproperty float ny\nproperty float nz\n" in head) == (normals is not None)
            size = head.index("end_header\n") + 11 + len(V) * (12 + (12 if normals is not None else 0) + (3 if colors is not None else 0)) \
                + len(F) * 13
            assert os.path.getsize(path) == size
            v, f, col = load_mesh_ply(path)                        # an existing call: three values, whatever the file holds
            assert np.array_equal(v, V) and np.array_equal(f, F) and (col is None) == (colors is None)
            v, f, col, nrm = load_mesh_ply(path, with_normals=True)
            assert np.array_equal(v, V) and np.array_equal(f, F)
            assert (colors is None and col is None) or np.allclose(col, C, atol=1e-6)
            assert (normals is None and nrm is None) or np.array_equal(nrm.view(np.int32), N.view(np.int32))
            if normals is None:                                    # byte for byte what save_mesh_ply writes
                other = str(tmp_path / "plain.ply")
                save_mesh_ply(other, V, F, colors)
                assert open(other, "rb").read() == open(path, "rb").read()
    with pytest.raises(ValueError, match="normals must have shape"):
        save_mesh_ply_with_normals(path, V, F, None, N[:3])


def test_a_file_of_the_earlier_writer_still_loads(tmp_path):
    """written here byte by byte in the layout the writer had before normals existed"""
    from easygaussiansplatting_amd.mesh import load_mesh_ply
    V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0.5, 0.25, 2]], np.float32)
    F = np.array([[0, 1, 2], [1, 3, 2]], np.int32)
    rgb = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [51, 102, 204]], np.uint8)
    for with_color in (False, True):
        head = "ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n"
        if with_color:
            head += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
        head += "element face 2\nproperty list uchar int vertex_indices\nend_header\n"
        body = b"".join(V[i].tobytes() + (rgb[i].tobytes() if with_color else b"") for i in range(4))
        body += b"".join(b"\x03" + F[i].tobytes() for i in range(2))
        path = str(tmp_path / "old.ply")
        with open(path, "wb") as fh:
            fh.write(head.encode("ascii") + body)
        v, f, c = load_mesh_ply(path)
        assert np.array_equal(v, V) and np.array_equal(f, F) and f.dtype == np.int64
        assert (c is None) if not with_color else np.array_equal(c, rgb.astype(np.float32) / np.float32(255))
        assert load_mesh_ply(path, with_normals=True)[3] is None


# ------------------------------------------------------------------------------------------------------------ the library
@pytest.fixture(scope="module")
def lib():
    from easygaussiansplatting_amd import _lib, _meshopslib
    if not os.path.exists(_meshopslib.LIB_PATH):
        _lib.build()
    return _meshopslib.load()


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    return sorted(ln.split()[-1] for ln in out.splitlines() if ln.strip() and ln.split()[-1].startswith("egs_"))


def test_library_exports_what_its_header_declares(lib):
    from easygaussiansplatting_amd import _meshopslib
    assert _exports(_meshopslib.LIB_PATH) == NAMES
    assert sorted(_meshopslib.SIGNATURES) == NAMES
    hdr = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(set(re.findall(r"\b(egs_[a-z0-9_]+)\s*\(", code))) == NAMES
    assert re.search(r"^#define\s+EGS_MESHOPS_ABI_VERSION\s+1\s*$", hdr, re.M)
    assert lib.egs_meshops_abi_version() == 1 == _meshopslib.ABI_VERSION
    for name, value in (("ERR_BAD_ARG", _meshopslib.ERR_BAD_ARG), ("MAX_BLOCKS", _meshopslib.MAX_BLOCKS)):
        assert re.search(r"^#define\s+EGS_MESHOPS_%s\s+%d\s*$" % (name, value), hdr, re.M), name
    assert _meshopslib.ERR_BAD_ARG == BAD_ARG
    for fn in (n for n in NAMES if n not in ("egs_meshops_abi_version", "egs_meshops_last_error_string")):
        decl = re.search(r"int %s\((.*?)\);" % fn, code, re.S).group(1)
        assert len(decl.split(",")) == len(_meshopslib.SIGNATURES[fn][1]), fn
    assert "NOBODY HAS TUNED" in hdr and "VERTEX connectivity" in hdr


def test_the_tsdf_library_is_untouched():
    from easygaussiansplatting_amd import _lib, _tsdflib
    if not os.path.exists(_tsdflib.LIB_PATH):
        _lib.build()
    assert len(_exports(_tsdflib.LIB_PATH)) == 5 and _tsdflib.ABI_VERSION == 1
    assert not any("meshops" in n for n in list(_tsdflib.SIGNATURES) + list(_lib.SIGNATURES))


def test_bad_arguments_are_refused_without_a_device(lib):
    P = _FAKE
    nan, inf = float("nan"), float("inf")

    def refused(rc):
        assert rc == BAD_ARG, rc
        msg = lib.egs_meshops_last_error_string().decode()
        assert msg.startswith("egs_meshops error 10001: bad argument"), msg

    def components(V=9, F=5, faces=P, label=2 * P, cf=3 * P, cv=4 * P, mb=0):
        return lib.egs_meshops_components(V, F, faces, label, cf, cv, mb, None)

    for kw in (dict(V=-1), dict(F=-1), dict(faces=None), dict(label=None), dict(cf=None), dict(cv=None), dict(faces=P + 4),
               dict(label=2 * P + 2), dict(cf=3 * P + 1), dict(cv=4 * P + 3), dict(label=P), dict(cf=2 * P), dict(cv=3 * P),
               dict(cv=P), dict(mb=-1), dict(mb=8193)):
        refused(components(**kw))
    assert components(V=0, label=None, cf=None, cv=None) == 0 and components(V=0, F=0, faces=None) == 0

    def flags(V=9, F=5, faces=P, label=2 * P, cf=3 * P, rank=4 * P, mf=2, kl=1, vk=5 * P, fk=6 * P, mb=0):
        return lib.egs_meshops_keep_flags(V, F, faces, label, cf, rank, mf, kl, vk, fk, mb, None)

    for kw in (dict(V=-2), dict(F=-3), dict(faces=None), dict(label=None), dict(cf=None), dict(vk=None), dict(fk=None),
               dict(mf=-1), dict(kl=-1), dict(rank=None, kl=1), dict(rank=4 * P + 2), dict(faces=P + 2),
               dict(vk=2 * P), dict(fk=3 * P), dict(vk=6 * P), dict(fk=P), dict(vk=4 * P), dict(mb=-1), dict(mb=1 << 20)):
        refused(flags(**kw))
    assert flags(V=0, F=0, faces=None, label=None, cf=None, rank=None, kl=0, vk=None, fk=None) == 0
    assert flags(V=0, F=0, faces=None, label=None, cf=None, rank=None, kl=2, vk=None, fk=None) == 0

    def compact(V=9, F=5, v=P, c=2 * P, n=3 * P, faces=4 * P, vk=5 * P, fk=6 * P, vs=7 * P, fs=8 * P, Vk=4, Fk=2, ov=9 * P,
                oc=10 * P, on=11 * P, of=12 * P, mb=0):
        return lib.egs_meshops_compact(V, F, v, c, n, faces, vk, fk, vs, fs, Vk, Fk, ov, oc, on, of, mb, None)

    for kw in (dict(V=-1), dict(F=-1), dict(Vk=-1), dict(Vk=10), dict(Fk=-1), dict(Fk=6), dict(v=None), dict(faces=None),
               dict(vk=None), dict(fk=None), dict(vs=None), dict(fs=None), dict(ov=None), dict(of=None), dict(oc=None),
               dict(on=None), dict(c=None), dict(n=None), dict(vs=7 * P + 4), dict(of=12 * P + 4), dict(ov=9 * P + 2),
               dict(ov=P), dict(oc=2 * P), dict(on=3 * P), dict(of=4 * P), dict(oc=9 * P), dict(on=10 * P), dict(Vk=0, Fk=1),
               dict(mb=-1), dict(mb=8193)):
        refused(compact(**kw))
    assert compact(Vk=0, Fk=0, ov=None, oc=None, on=None, of=None) == 0
    assert compact(V=0, F=0, Vk=0, Fk=0, v=None, c=None, n=None, faces=None, vk=None, fk=None, vs=None, fs=None, ov=None,
                   oc=None, on=None, of=None) == 0

    def normals(V=9, F=5, v=P, faces=2 * P, rs=3 * P, rows=4 * P, out=5 * P, mb=0):
        return lib.egs_meshops_vertex_normals(V, F, v, faces, rs, rows, out, mb, None)

    for kw in (dict(V=-1), dict(F=-1), dict(v=None), dict(faces=None), dict(rs=None), dict(rows=None), dict(out=None),
               dict(rs=3 * P + 4), dict(rows=4 * P + 4), dict(out=5 * P + 1), dict(out=P), dict(out=2 * P), dict(mb=-1),
               dict(mb=8193)):
        refused(normals(**kw))
    assert normals(V=0, v=None, out=None) == 0

    def taubin(V=9, F=5, v=P, faces=2 * P, rs=3 * P, rows=4 * P, it=3, lam=0.5, mu=-0.53, out=5 * P, tmp=6 * P, mb=0):
        return lib.egs_meshops_taubin(V, F, v, faces, rs, rows, it, lam, mu, out, tmp, mb, None)

    for kw in (dict(V=-1), dict(F=-1), dict(v=None), dict(faces=None), dict(rs=None), dict(rows=None), dict(out=None),
               dict(tmp=None), dict(it=-1), dict(lam=nan), dict(lam=inf), dict(mu=nan), dict(mu=-inf), dict(out=P),
               dict(tmp=P), dict(tmp=5 * P), dict(out=5 * P + 2), dict(tmp=6 * P + 1), dict(mb=-1), dict(mb=8193)):
        refused(taubin(**kw))
    assert taubin(V=0, v=None, out=None, tmp=None) == 0


# ---------------------------------------------------------------------------------------------------- the Python surface
def test_signatures_and_documented_defaults():
    from easygaussiansplatting_amd import mesh
    from easygaussiansplatting_amd.trainer import Trainer
    sig = lambda f: inspect.signature(f).parameters
    assert list(sig(mesh.connected_components))[:2] == ["faces", "n_vertices"]
    assert mesh.Components._fields == ("label", "comp_faces", "comp_verts")
    p = sig(mesh.remove_small_components)
    assert list(p) == ["vertices", "faces", "colors", "min_faces", "keep_largest", "normals", "check"]
    assert [p[k].default for k in list(p)[2:]] == [None, None, None, None, True]
    p = sig(mesh.smooth_taubin)
    assert list(p)[:5] == ["vertices", "faces", "iterations", "lam", "mu"]
    assert (p["iterations"].default, p["lam"].default, p["mu"].default) == (10, 0.5, -0.53)
    p = sig(mesh.clean_mesh)
    assert list(p)[:7] == ["vertices", "faces", "colors", "min_faces", "keep_largest", "smooth_iterations", "normals"]
    assert (p["smooth_iterations"].default, p["normals"].default) == (0, False)
    assert list(sig(mesh.load_mesh_ply)) == ["path", "with_normals"] and sig(mesh.load_mesh_ply)["with_normals"].default is False
    assert list(sig(mesh.save_mesh_ply_with_normals)) == ["path", "vertices", "faces", "colors", "normals"]
    p = sig(Trainer.extract_mesh)
    assert (p["min_component_faces"].default, p["keep_largest"].default, p["smooth_iterations"].default) == (None, None, 0)
    for doc in (mesh.__doc__, mesh.smooth_taubin.__doc__, Trainer.extract_mesh.__doc__):
        assert "nobody has tuned" in doc.lower() or "untuned" in doc.lower()
    assert "not cleaned" not in open(os.path.join(REPO, "examples", "extract_mesh.py")).read()


def test_host_argument_checks():
    from easygaussiansplatting_amd import mesh
    V = torch.zeros((6, 3))
    F = torch.tensor([[0, 1, 2], [3, 4, 5]], dtype=torch.int64)
    bad = [
        (lambda: mesh.connected_components(F.int(), 6), "faces must be torch.int64"),
        (lambda: mesh.connected_components(F[:, :2], 6), "faces must have shape"),
        (lambda: mesh.connected_components(F, -1), "n_vertices must be an integer"),
        (lambda: mesh.connected_components(F, 1 << 31), "n_vertices must be an integer"),
        (lambda: mesh.connected_components(F, 6), "faces must live on the GPU"),
        (lambda: mesh.remove_small_components(V, F), "give min_faces, keep_largest or both"),
        (lambda: mesh.remove_small_components(V, F, min_faces=-1), "min_faces must be an integer"),
        (lambda: mesh.remove_small_components(V, F, keep_largest=0), "keep_largest must be an integer"),
        (lambda: mesh.remove_small_components(V.double(), F, min_faces=1), "vertices must be torch.float32"),
        (lambda: mesh.remove_small_components(V[:, :2], F, min_faces=1), "vertices must have shape"),
        (lambda: mesh.remove_small_components(V, F, min_faces=1), "faces must live on the GPU"),
        (lambda: mesh.vertex_normals(V.half(), F), "vertices must be torch.float32"),
        (lambda: mesh.vertex_normals(V, F.float()), "faces must be torch.int64"),
        (lambda: mesh.smooth_taubin(V, F, iterations=-1), "iterations must be an integer"),
        (lambda: mesh.smooth_taubin(V, F, iterations=1.5), "iterations must be an integer"),
        (lambda: mesh.smooth_taubin(V, F, lam=float("nan")), "lam and mu must be finite"),
        (lambda: mesh.smooth_taubin(V, F, mu=float("inf")), "lam and mu must be finite"),
        (lambda: mesh.clean_mesh(V, F, smooth_iterations=-2), "smooth_iterations must be an integer"),
        (lambda: mesh.clean_mesh(V, F, min_faces=3), "faces must live on the GPU"),
    ]
    for call, msg in bad:
        with pytest.raises(ValueError, match=msg):
            call()
    with pytest.raises(TypeError, match="faces must be a torch.Tensor"):
        mesh.connected_components(F.numpy(), 6)
    with pytest.raises(TypeError, match="vertices must be a torch.Tensor"):
        mesh.vertex_normals(V.numpy(), F)


def test_the_examples_list_the_flags():
    r = subprocess.run([sys.executable, os.path.join(REPO, "examples", "train.py"), "--help"], capture_output=True,
                       text=True, cwd=REPO)
    assert r.returncode == 0, r.stderr
    assert "--mesh-min-faces N" in r.stdout
    r = subprocess.run([sys.executable, os.path.join(REPO, "examples", "extract_mesh.py"), "--help"], capture_output=True,
                       text=True, cwd=REPO)
    assert r.returncode == 0, r.stderr
    for flag in ("--min-component-faces N", "--keep-largest K", "--smooth N", "--normals"):
        assert flag in r.stdout, flag
