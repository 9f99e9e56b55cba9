"""Compressed scene files without a GPU: the reference of tests/kmeans_ref.py on hand-computed cases and on
the cases the GPU tests use (the float32 restatement of the kernel's score formula obeys the derived gap bound -- which shows
that the bound, and not the kernel, is sound), the codec's error bounds, derived rather than measured, the archive, and the C
surface of libegs_kmeans.so against include/egs_kmeans.h."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests import kmeans_ref as KR

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "egs_kmeans.h")


@pytest.fixture(scope="module", autouse=True)
def reference_is_of_this_package():
    """the reference's shapes and restatement are those of THIS library: the rows per workgroup, the centroid tile and the
    chunk that ``kmeans_ref.SHAPES`` and the update cases are built around are the binding's, and its quantiser is the
    package's (so no test of the reference below stands without the package)"""
    from easygaussiansplatting_amd import _kmeanslib, compress
    assert (KR.ROWS, KR.TILE, KR.CHUNK) == (_kmeanslib.ROWS, _kmeanslib.TILE, _kmeanslib.CHUNK)
    v = np.linspace(-1.5, 2.5, 37).reshape(-1, 1)
    for bits in (8, 16):
        q, lo, hi = KR.quantise(v, bits)
        q2, lo2, hi2 = compress._quantise(v, bits)
        assert np.array_equal(q, q2) and lo == lo2 and hi == hi2
        assert np.array_equal(KR.dequantise(q, lo, hi, bits), compress._dequantise(q2, lo2, hi2, bits))


# ------------------------------------------------------------------------------------------------------- the reference
def test_assign_by_hand():
    c = np.array([[0, 0], [2, 0], [0, 0], [0, 3]], np.float32)               # 2 duplicates 0
    x = np.array([[1, 0], [0.1, 0], [1.9, 0.1], [0, 1.5], [0, 2], [np.nan, 0], [np.inf, 1]], np.float32)
    labels, dist = KR.assign(x, c)
    # (1,0): equidistant to 0 and 1 -> 0; (0,1.5): equidistant to 0 and 3 -> 0; not-finite rows -> 0
    assert labels.tolist() == [0, 0, 1, 0, 3, 0, 0] and labels.dtype == np.int32
    assert np.allclose(dist[:5], [1, 0.01, 0.02, 2.25, 1], atol=1e-6)
    assert KR.assign32(x, c).tolist() == labels.tolist()


def test_update_by_hand():
    x = np.array([[0, 0], [2, 4], [10, 10], [4, 0], [7, 7]], np.float32)
    labels = np.array([0, 0, 2, 0, 3])
    prev = np.full((4, 2), 9.5, np.float32)
    c, _, wsum, count = KR.update(x, labels, prev)
    assert np.array_equal(c, np.array([[2, 4 / 3], [9.5, 9.5], [10, 10], [7, 7]], np.float32))
    assert c[0, 1] == np.float32(4 / 3) and wsum.tolist() == [3, 0, 1, 1] and count.tolist() == [3, 0, 1, 1]
    w = np.array([1, 3, 2, 0, 0], np.float32)
    c, _, wsum, count = KR.update(x, labels, prev, w)
    assert c.tolist() == [[1.5, 3.0], [9.5, 9.5], [10, 10], [9.5, 9.5]]       # cluster 3: weight 0 keeps its bits
    assert wsum.tolist() == [4, 0, 2, 0] and count.tolist() == [3, 0, 1, 1]
    order, offsets = KR.incidence(labels, 4)
    assert order.tolist() == [0, 1, 3, 2, 4] and offsets.tolist() == [0, 3, 3, 4, 5]


def test_lloyd_on_planted_clusters():
    x, init, centres, labels = KR.planted_case()
    c, l = KR.lloyd(x, len(init), iters=1, init=init)
    assert np.array_equal(c, centres) and np.array_equal(l, labels)
    a = KR.lloyd(x, 5, iters=3, seed=4)
    b = KR.lloyd(x, 5, iters=3, seed=4)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(KR.lloyd(x, 5, iters=0, seed=4)[0], x[KR.init_rows(len(x), 5, 4)])


@pytest.mark.parametrize("shape", KR.SHAPES)
def test_lattice_cases_are_exact_and_hold_ties(shape):
    N, K, D = shape
    x, c = KR.lattice_case(N, K, D)
    d = KR.sqdist(x, c)
    labels, dist = KR.assign(x, c)
    assert np.array_equal(KR.assign32(x, c), labels)                        # exact arithmetic: the same argmin
    s = KR.scores32(x, c).astype(np.float64) + (x.astype(np.float64) ** 2).sum(1)[:, None]
    assert np.array_equal(s, d)
    at_min = d == d.min(1, keepdims=True)
    if K >= 3:
        assert at_min[:, 0][labels == 0].all() and (labels != K - 1).all()  # the duplicate never wins
        assert N < 2 or dist[1] == 0
    if K >= 2 and (K == 2 or D >= 9):
        distinct = [len({c[k].tobytes() for k in np.nonzero(row)[0]}) > 1 for row in at_min]
        assert any(distinct), "no genuine tie in the case"


@pytest.mark.parametrize("kind", ["normal", "far"])
@pytest.mark.parametrize("shape", KR.SHAPES)
def test_the_float32_restatement_obeys_the_gap_bound(shape, kind):
    x, c = KR.random_case(*shape, kind=kind)
    labels = KR.assign32(x, c)
    gap, bound = KR.gaps(x, c, labels), KR.gap_bound(x, c)
    print("%s %s: %d of %d labels differ from the float64 argmin, worst gap %.3e (bound there %.3e)" % (
        shape, kind, int((labels != KR.assign(x, c)[0]).sum()), len(x), gap.max(), bound[np.argmax(gap)]))
    assert (gap <= bound).all()


# --------------------------------------------------------------------------------------------------------------- codec
def _fake_codebook(gs, k, seed=0):
    rest = np.asarray(gs["sh"])[:, 3:]
    c, l = KR.lloyd(rest, k, iters=3, seed=seed)
    return c, l


@pytest.mark.parametrize("bits", [None, {"pw": 8, "scale": 16, "rot": 16, "alpha": 16, "sh_dc": 16}])
def test_codec_bounds(bits):
    from easygaussiansplatting_amd import compress as CP
    gs = KR.gaussians(300, 48, seed=3)
    gs["pw"][:, 1] = 0.75                                                    # a column with max == min
    gs["sh"][:, 2] = -0.125
    cb = _fake_codebook(gs, 20)
    d = CP.encode(gs, bits=bits, codebook=cb)
    b = dict(CP.DEFAULT_BITS, **(bits or {}))
    meta = json.loads(d["meta"])
    assert meta == {"version": 1, "n": 300, "sh_dim": 48, "clusters": 20, "bits": b}
    for k in ("pw", "scale", "rot", "alpha", "sh_dc"):
        assert d[k].dtype == (np.uint8 if b[k] == 8 else np.uint16)
        assert d[k + "_min"].dtype == np.float32 and d[k + "_max"].dtype == np.float32
    assert d["sh_rest_codebook"].dtype == np.float16 and d["sh_rest_index"].dtype == np.uint8
    out = CP.decode(d)
    assert out.dtype == gs.dtype and out.shape == gs.shape
    f8 = lambda a: np.asarray(a, np.float64)
    # positions, log scale, sh_dc: half a step plus one float32 ulp of the larger bound, per column
    assert (np.abs(f8(out["pw"]) - f8(gs["pw"])) <= KR.column_bound(d["pw_min"], d["pw_max"], b["pw"])).all()
    log_scale = CP._dequantise(d["scale"], d["scale_min"], d["scale_max"], b["scale"])       # the field the decoder exponentiates
    assert (np.abs(f8(log_scale) - np.log(f8(gs["scale"]))) <= KR.column_bound(d["scale_min"], d["scale_max"], b["scale"])).all()
    assert (np.abs(np.log(f8(out["scale"])) - np.log(f8(gs["scale"])))
            <= KR.column_bound(d["scale_min"], d["scale_max"], b["scale"])).all()
    assert np.array_equal(out["scale"], np.exp(f8(log_scale)).astype(np.float32))
    assert (np.abs(f8(out["sh"][:, :3]) - f8(gs["sh"][:, :3])) <= KR.column_bound(d["sh_dc_min"], d["sh_dc_max"], b["sh_dc"])).all()
    assert np.array_equal(out["pw"][:, 1], gs["pw"][:, 1]) and np.array_equal(out["sh"][:, 2], gs["sh"][:, 2])
    assert np.abs(f8(out["alpha"]) - f8(gs["alpha"])).max() <= 1.0 / (2 * (2 ** b["alpha"] - 1)) <= 1.0 / 510
    # quaternions: unit norm, w >= 0, within the angle a per-component error of one step allows
    q, q0 = f8(out["rot"]), f8(gs["rot"])
    assert np.abs(np.linalg.norm(q, axis=1) - 1).max() <= 1e-6 and (q[:, 0] >= 0).all()
    q0 = q0 / np.linalg.norm(q0, axis=1, keepdims=True)
    chord = np.minimum(np.linalg.norm(q - q0, axis=1), np.linalg.norm(q + q0, axis=1))      # (arccos of the dot is all noise here)
    angle = 4 * np.arcsin(chord / 2)
    assert angle.max() <= KR.quaternion_angle_bound(b["rot"])
    # the SH rest: the float16 rounding of the indexed codebook row, exactly
    want = cb[0].astype(np.float16).astype(np.float32)[cb[1]]
    assert np.array_equal(out["sh"][:, 3:], want)
    # the package's quantiser is the reference's
    for k, v in (("pw", gs["pw"]), ("sh_dc", gs["sh"][:, :3]), ("scale", np.log(f8(gs["scale"])))):
        qq, lo, hi = KR.quantise(v, b[k])
        assert np.array_equal(qq, d[k]) and np.array_equal(lo, d[k + "_min"]) and np.array_equal(hi, d[k + "_max"])
        assert np.array_equal(KR.dequantise(qq, lo, hi, b[k]), CP._dequantise(d[k], lo, hi, b[k]))


def test_encode_refuses_what_it_cannot_store():
    from easygaussiansplatting_amd import compress as CP
    gs = KR.gaussians(10, 3)
    for field, value in (("pw", np.nan), ("sh", np.inf), ("alpha", -np.inf), ("scale", np.nan)):
        bad = gs.copy()
        bad[field][3] = value
        with pytest.raises(ValueError, match="finite"):
            CP.encode(bad)
    bad = gs.copy()
    bad["scale"][0, 1] = 0.0
    with pytest.raises(ValueError, match="positive"):
        CP.encode(bad)
    with pytest.raises(ValueError, match="8 or 16"):
        CP.encode(gs, bits={"pw": 12})
    with pytest.raises(ValueError, match="unknown attribute"):
        CP.encode(gs, bits={"sh_rest": 8})
    assert CP.default_clusters(3) == 1 and CP.default_clusters(1000) == 250 and CP.default_clusters(10 ** 7) == 65536


# --------------------------------------------------------------------------------------------------------------- files
def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_archive_round_trip_and_dispatch(tmp_path):
    from easygaussiansplatting_amd import compress as CP
    from easygaussiansplatting_amd import gau_io
    gs = KR.gaussians(500, 27, seed=5)
    cb = _fake_codebook(gs, 300)                                             # K > 256: uint16 indices
    fn = str(tmp_path / "x.gsz")
    d = CP.save_compressed(fn, gs, codebook=cb)
    assert d["sh_rest_index"].dtype == np.uint16 and os.path.exists(fn) and not os.path.exists(fn + ".npz")
    want = CP.decode(CP.encode(gs, codebook=cb))
    assert _same(CP.load_compressed(fn), want) and _same(gau_io.load_gs(fn), want)
    np.save(str(tmp_path / "x.npy"), gs)
    assert os.path.getsize(fn) < os.path.getsize(str(tmp_path / "x.npy"))
    for other in ("x.npz", "x.gsz.bak", "x.txt"):                            # still refused
        with pytest.raises(ValueError, match="not a supported file"):
            gau_io.load_gs(str(tmp_path / other))


@pytest.mark.parametrize("n,sh_dim", [(7, 3), (1, 3), (0, 3), (1, 12)])
def test_degree_0_and_single_gaussian_round_trip(tmp_path, n, sh_dim):
    from easygaussiansplatting_amd import compress as CP
    gs = KR.gaussians(n, sh_dim, seed=6)
    kw = {} if sh_dim == 3 else {"codebook": (np.asarray(gs["sh"])[:, 3:], np.zeros(n, np.int64))}
    fn = str(tmp_path / "s.gsz")
    d = CP.save_compressed(fn, gs, **kw)                                     # degree 0: no codebook, no kernel, no GPU
    assert ("sh_rest_codebook" in d) == (sh_dim > 3)
    out = CP.load_compressed(fn)
    assert _same(out, CP.decode(d)) and out.shape == (n,)
    if n == 1:                                                               # every column has max == min: exact
        assert np.array_equal(out["pw"], gs["pw"]) and np.array_equal(out["sh"][:, :3], gs["sh"][:, :3])
        assert np.array_equal(out["sh"][:, 3:], np.asarray(gs["sh"])[:, 3:].astype(np.float16).astype(np.float32))


def test_wrong_version_and_truncated_archive_raise(tmp_path):
    from easygaussiansplatting_amd import compress as CP
    gs = KR.gaussians(50, 3)
    fn = str(tmp_path / "v.gsz")
    d = CP.save_compressed(fn, gs)
    meta = json.loads(d["meta"])
    meta["version"] = 2
    with pytest.raises(CP.GszFormatError, match="format version 2"):
        CP.decode(dict(d, meta=json.dumps(meta)))
    with open(str(tmp_path / "v2.gsz"), "wb") as f:
        np.savez_compressed(f, **dict(d, meta=json.dumps(meta)))
    with pytest.raises(ValueError, match="format version 2"):
        CP.load_compressed(str(tmp_path / "v2.gsz"))
    raw = open(fn, "rb").read()
    for keep in (len(raw) // 2, 10):
        with open(str(tmp_path / "t.gsz"), "wb") as f:
            f.write(raw[:keep])
        with pytest.raises(ValueError):
            CP.load_compressed(str(tmp_path / "t.gsz"))
    with pytest.raises(CP.GszFormatError, match="lacks the field"):
        CP.decode({k: v for k, v in d.items() if k != "alpha"})


# ------------------------------------------------------------------------------------------------------- the C surface
@pytest.fixture(scope="module")
def lib():
    from easygaussiansplatting_amd import _kmeanslib, _lib
    if not os.path.exists(_kmeanslib.LIB_PATH):
        _lib.build()
    return _kmeanslib.load()


def test_header_binding_and_library_agree(lib):
    from easygaussiansplatting_amd import _kmeanslib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(egs_kmeans_\w+)\s*\(", text)))
    assert declared == sorted(_kmeanslib.SIGNATURES)
    consts = dict(re.findall(r"#define\s+EGS_KMEANS_(\w+)\s+(\d+)", text))
    assert int(consts["ABI_VERSION"]) == _kmeanslib.ABI_VERSION and int(consts["ERR_BAD_ARG"]) == _kmeanslib.ERR_BAD_ARG
    assert (int(consts["ROWS"]), int(consts["TILE"]), int(consts["CHUNK"])) == (_kmeanslib.ROWS, _kmeanslib.TILE, _kmeanslib.CHUNK)
    assert (KR.ROWS, KR.TILE, KR.CHUNK) == (_kmeanslib.ROWS, _kmeanslib.TILE, _kmeanslib.CHUNK)
    assert (int(consts["MAX_D"]), int(consts["MAX_K"]), int(consts["MAX_BLOCKS"])) == (
        _kmeanslib.MAX_D, _kmeanslib.MAX_K, _kmeanslib.MAX_BLOCKS)
    out = subprocess.run(["nm", "-D", "--defined-only", _kmeanslib.LIB_PATH], capture_output=True, text=True).stdout
    exported = sorted(ln.split()[-1] for ln in out.splitlines() if ln.strip() and ln.split()[-1].startswith("egs_"))
    assert exported == declared
    assert lib.egs_kmeans_abi_version() == 1
    for fn in (n for n in declared if n not in ("egs_kmeans_abi_version", "egs_kmeans_last_error_string")):
        decl = re.search(r"\b%s\((.*?)\);" % fn, text, re.S).group(1)
        assert len(decl.split(",")) == len(_kmeanslib.SIGNATURES[fn][1]), fn


def test_bad_arguments_are_refused_without_a_device(lib):
    P = 0x10000          # a "device pointer" no refused call dereferences

    def refused(rc):
        assert rc == 10001, rc
        msg = lib.egs_kmeans_last_error_string().decode()
        assert msg.startswith("egs_kmeans error 10001: bad argument"), msg

    def assign(N=9, D=5, K=4, x=P, c=2 * P, cn=3 * P, lab=4 * P, dist=5 * P, mb=0):
        return lib.egs_kmeans_assign(N, D, K, x, c, cn, lab, dist, mb, None)

    for kw in (dict(N=-1), dict(D=0), dict(D=65), dict(K=0), dict(K=65537), dict(x=None), dict(c=None), dict(cn=None),
               dict(lab=None), dict(x=P + 2), dict(lab=4 * P + 1), dict(dist=5 * P + 2), dict(lab=P), dict(dist=2 * P),
               dict(cn=2 * P), dict(mb=-1), dict(mb=8193)):
        refused(assign(**kw))
    assert assign(N=0, x=None, lab=None, dist=None) == 0 and assign(N=0) == 0

    def update(N=9, D=5, K=4, x=P, w=2 * P, order=3 * P, off=4 * P, c=5 * P, ws=6 * P, cnt=7 * P, wk=8 * P, nb=None, mb=0):
        nb = lib.egs_kmeans_update_ws_bytes(N, D, K) if nb is None else nb
        return lib.egs_kmeans_update(N, D, K, x, w, order, off, c, ws, cnt, wk, nb, mb, None)

    for kw in (dict(N=-1), dict(D=0), dict(D=65), dict(K=0), dict(K=65537), dict(x=None), dict(order=None), dict(off=None),
               dict(c=None), dict(ws=None), dict(cnt=None), dict(wk=None), dict(nb=8), dict(order=3 * P + 4), dict(ws=6 * P + 4),
               dict(c=P), dict(cnt=5 * P), dict(wk=2 * P), dict(mb=-1), dict(mb=8193)):
        refused(update(**kw))
    assert update(N=0, x=None, order=None, wk=None, nb=0) == 0
    assert lib.egs_kmeans_update_ws_bytes(1000, 45, 7) == (1000 // 256 + 7) * 46 * 8
    assert lib.egs_kmeans_update_ws_bytes(9, 0, 4) == 0 and lib.egs_kmeans_update_ws_bytes(9, 5, 65537) == 0


def test_python_layer_checks_its_arguments_before_any_kernel():
    from easygaussiansplatting_amd import compress as CP
    with pytest.raises(ValueError, match="must live on the GPU"):
        CP.kmeans(torch.zeros(4, 3), 2)
    with pytest.raises(TypeError):
        CP.assign(np.zeros((4, 3), np.float32), torch.zeros(2, 3))
