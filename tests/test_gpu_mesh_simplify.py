"""libegs_simplify.so on the GPU, called through its C ABI on buffers between guard bands, against the numpy
definitions of tests/mesh_simplify_ref.py.  Exact on every case: keys, cluster ids, ``placed``, remapped faces, validity and
sort keys, keep flags, kept counts and the final faces.  Positions and colours within ONE float32 ulp of the case's largest
coordinate magnitude (colour value) of the float64 reference -- both sides do the same well-conditioned double arithmetic
and round once, so only a rounding straddle can separate them; the number of rows that are not bit-identical and the worst
difference are printed.  Every output the same bits on grids of 1 and 3 workgroups, on the default grid, on a side stream and
in the fused form of the cluster kernel.  Inputs unmodified, guard bands intact, refused and empty calls write nothing.  Then
the Python layer against the ABI's bits."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import loss_abi as LA
from tests import mesh_ops_ref as MR
from tests import mesh_simplify_ref as SR

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CASES = list(SR.BUILDERS)
BAD_ARG = 10001
PLACE = {"quadric": 0, "mean": 1}


@pytest.fixture(scope="module")
def libs():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from easygaussiansplatting_amd import _meshopslib, _simplifylib
    return _simplifylib.load(), _meshopslib.load()


class Out:
    """an output buffer between two guard bands, filled with the guards' pattern"""

    def __init__(self, shape, dtype):
        self.dtype = getattr(torch, dtype)
        self.shape = tuple(shape)
        n = int(np.prod(self.shape)) * torch.empty((), dtype=self.dtype).element_size()
        self.whole, self.inner = LA.guarded(n)

    @property
    def ptr(self):
        return C.c_void_p(self.inner.data_ptr())

    def tensor(self):
        return self.inner.view(self.dtype).reshape(self.shape)

    def numpy(self):
        assert LA.guards_intact(self.whole), "a kernel wrote outside its buffer"
        return self.tensor().cpu().numpy().copy()

    def untouched(self):
        return LA.guards_intact(self.whole) and bool((self.inner == LA.PATTERN).all())


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def to_dev(a):
    return torch.from_numpy(np.array(a, copy=True)).cuda()


@functools.lru_cache(maxsize=None)
def mesh(name):
    """the case on the device, with its incidence: built once, never written"""
    c = SR.case(name)
    row_start, rows = MR.incidence(c["F"], len(c["V"]))
    return dict(nv=len(c["V"]), nf=len(c["F"]), V=to_dev(c["V"]), F=to_dev(c["F"]), C=to_dev(c["C"]),
                row_start=to_dev(row_start), rows=to_dev(rows), cell=c["cell"], origin=c["origin"])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


class Runner:
    """the entry points on one grid cap and one stream"""

    def __init__(self, libs, max_blocks=0, side_stream=False):
        self.lib, self.mo = libs
        self.mb = max_blocks
        self.stream = torch.cuda.Stream() if side_stream else torch.cuda.current_stream()

    def _run(self, fn, *args):
        torch.cuda.synchronize()
        rc = fn(*args, self.mb, C.c_void_p(self.stream.cuda_stream))
        torch.cuda.synchronize()
        return rc

    def keys(self, m):
        out = Out((m["nv"],), "int64")
        assert self._run(self.lib.egs_simplify_keys, m["nv"], ptr(m["V"]), *m["origin"], m["cell"], out.ptr) == 0
        return out.numpy()

    def quadrics(self, m, keys):
        out = Out((m["nv"], 9), "float64")
        assert self._run(self.lib.egs_simplify_vertex_quadrics, m["nv"], m["nf"], ptr(m["V"]), ptr(m["F"]),
                         ptr(m["row_start"]), ptr(m["rows"]), ptr(keys), *m["origin"], m["cell"], out.ptr) == 0
        return out.numpy()

    def clusters(self, m, keys, member_start, members, quadrics, placement, Vc):
        pos, col, placed = Out((Vc, 3), "float32"), Out((Vc, 3), "float32"), Out((Vc,), "int32")
        assert self._run(self.lib.egs_simplify_clusters, m["nv"], m["nf"], Vc, ptr(m["V"]), ptr(m["C"]), ptr(keys),
                         ptr(member_start), ptr(members), ptr(quadrics), ptr(m["F"]), ptr(m["row_start"]), ptr(m["rows"]),
                         *m["origin"], m["cell"], PLACE[placement], pos.ptr, col.ptr, placed.ptr) == 0
        return pos.numpy(), col.numpy(), placed.numpy()

    def remap(self, m, cluster, Vc):
        rot, valid = Out((m["nf"], 3), "int64"), Out((m["nf"],), "int32")
        hi, lo = Out((m["nf"],), "int64"), Out((m["nf"],), "int64")
        assert self._run(self.lib.egs_simplify_remap_faces, m["nv"], m["nf"], Vc, ptr(m["F"]), ptr(cluster), rot.ptr,
                         valid.ptr, hi.ptr, lo.ptr) == 0
        return rot.numpy(), valid.numpy(), hi.numpy(), lo.numpy()

    def keep_flags(self, m, Vc, order, rot, valid, hi, lo):
        fk, ck = Out((m["nf"],), "int32"), Out((Vc,), "int32")
        assert self._run(self.lib.egs_simplify_keep_flags, m["nf"], Vc, ptr(order), ptr(rot), ptr(valid), ptr(hi), ptr(lo),
                         fk.ptr, ck.ptr) == 0
        return fk.numpy(), ck.numpy()

    def compact(self, m, Vc, pos, col, rot, ckeep, fkeep):
        vs, fs = torch.cumsum(ckeep, 0, dtype=torch.int64), torch.cumsum(fkeep, 0, dtype=torch.int64)
        Vk = int(vs[-1]) if Vc else 0
        Fk = int(fs[-1]) if m["nf"] else 0
        ov, oc, of = Out((Vk, 3), "float32"), Out((Vk, 3), "float32"), Out((Fk, 3), "int64")
        assert self._run(self.mo.egs_meshops_compact, Vc, m["nf"], ptr(pos), ptr(col), None, ptr(rot), ptr(ckeep), ptr(fkeep),
                         ptr(vs), ptr(fs), Vk, Fk, ov.ptr, oc.ptr, None, of.ptr) == 0
        return Vk, Fk, ov.numpy(), oc.numpy(), of.numpy()

    def pipeline(self, name, placement, fused=False):
        """every step through the ABI; sorting, unique and scans in torch as ``mesh.py`` does them -> dict of numpy arrays"""
        m = mesh(name)
        before = [t.clone() for t in (m["V"], m["F"], m["C"], m["row_start"], m["rows"])]
        r = dict(keys=self.keys(m))
        keys = to_dev(r["keys"])
        uniq, cluster = torch.unique(keys, return_inverse=True)
        cluster = cluster.contiguous()
        Vc = int(uniq.shape[0])
        srt, members = torch.sort(cluster, stable=True)
        member_start = torch.searchsorted(srt, torch.arange(Vc + 1, dtype=torch.int64, device="cuda")).contiguous()
        r.update(uniq=uniq.cpu().numpy(), cluster=cluster.cpu().numpy(), Vc=Vc)
        quadrics = None
        if placement == "quadric" and not fused:
            r["quadrics"] = self.quadrics(m, keys)
            quadrics = to_dev(r["quadrics"])
        r["pos"], r["col"], r["placed"] = self.clusters(m, keys, member_start, members.contiguous(), quadrics, placement, Vc)
        r["rot"], r["valid"], r["hi"], r["lo"] = self.remap(m, cluster, Vc)
        rot, valid, hi, lo = (to_dev(r[k]) for k in ("rot", "valid", "hi", "lo"))
        order = torch.sort(lo, stable=True).indices
        order = order[torch.sort(hi[order], stable=True).indices].contiguous()
        r["fkeep"], r["ckeep"] = self.keep_flags(m, Vc, order, rot, valid, hi, lo)
        r["Vk"], r["Fk"], r["V"], r["C"], r["F"] = self.compact(m, Vc, to_dev(r["pos"]), to_dev(r["col"]), rot,
                                                                 to_dev(r["ckeep"]), to_dev(r["fkeep"]))
        for a, b in zip(before, (m["V"], m["F"], m["C"], m["row_start"], m["rows"])):
            assert a.numel() == 0 or torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "an input was modified"
        return r


ARRAYS = ("keys", "cluster", "pos", "col", "placed", "rot", "valid", "hi", "lo", "fkeep", "ckeep", "V", "C", "F")


# ----------------------------------------------------------------------------------------------- against the reference
@pytest.mark.parametrize("placement", SR.PLACEMENTS)
@pytest.mark.parametrize("name", CASES)
def test_outputs_against_the_reference(libs, name, placement):
    c = SR.case(name)
    want = c[placement]
    got = Runner(libs).pipeline(name, placement)
    for k in ("keys", "uniq", "cluster", "placed", "rot", "valid", "hi", "lo", "fkeep", "ckeep"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    assert got["Vc"] == want["clusters"] and (got["Vk"], got["Fk"]) == (want["Vk"], want["Fk"])
    assert got["F"].dtype == np.int64 and np.array_equal(got["F"], want["F"])
    # positions of every cluster (kept or not) and of the compacted mesh; colours likewise
    ulp_v = SR.ulp32(np.abs(c["V"]).max()) if len(c["V"]) else 0.0
    ulp_c = SR.ulp32(np.abs(c["C"]).max()) if len(c["C"]) else 0.0
    for what, g, w64, w32, ulp in (("positions", got["pos"], want["pos64"], None, ulp_v),
                                   ("colours", got["col"], want["col64"], None, ulp_c),
                                   ("kept positions", got["V"], None, want["V"], ulp_v),
                                   ("kept colours", got["C"], None, want["C"], ulp_c)):
        ref = w64 if w64 is not None else w32.astype(np.float64)
        ref32 = ref.astype(np.float32)
        assert g.shape == ref.shape and np.isfinite(g).all()
        rows = int((g.view(np.int32) != ref32.view(np.int32)).any(1).sum()) if len(g) else 0
        worst = float(np.abs(g.astype(np.float64) - ref).max()) if len(g) else 0.0
        print("%s, %s: %s: %d of %d rows not bit-identical, worst difference %.3e (one ulp: %.3e)" % (
            name, placement, what, rows, len(g), worst, ulp))
        assert worst <= ulp, what
    if placement == "quadric" and len(c["V"]):
        q = got["quadrics"]
        scale = np.abs(want["quadrics"]).max(0) + 1e-300
        assert float((np.abs(q - want["quadrics"]) / scale).max()) <= 1e-12
        print("%s: %d of %d vertex quadrics not bit-identical" % (name, int((q != want["quadrics"]).any(1).sum()), len(q)))


# ------------------------------------------------------------------------------------------------------ reproducibility
@pytest.mark.parametrize("name", CASES)
def test_every_output_is_the_same_on_every_grid_stream_and_form(libs, name):
    first = Runner(libs).pipeline(name, "quadric")
    for kw in (dict(), dict(max_blocks=1), dict(max_blocks=3), dict(side_stream=True)):
        for fused in (False, True):
            again = Runner(libs, **kw).pipeline(name, "quadric", fused=fused)
            for k in ARRAYS:
                assert same_bits(first[k], again[k]), (kw, fused, k)
    mean = Runner(libs).pipeline(name, "mean")
    for kw in (dict(max_blocks=1), dict(max_blocks=3), dict(side_stream=True)):
        again = Runner(libs, **kw).pipeline(name, "mean")
        for k in ARRAYS:
            assert same_bits(mean[k], again[k]), (kw, k)


# -------------------------------------------------------------------------------------------- garbage, refused, empty
def test_values_that_would_index_outside_are_skipped(libs):
    """cluster ids, CSR entries, member lists, sort orders and face indices outside their ranges: nothing is written outside
    a buffer (the guards are checked by every ``numpy()``) and the untouched parts keep the reference's values"""
    name = "degenerate"
    c, m, run = SR.case(name), mesh(name), Runner(libs)
    want = c["quadric"]
    nv, nf, Vc = m["nv"], m["nf"], want["clusters"]
    bad_faces = m["F"].clone()
    bad_faces[1, 2] = nv
    bad_faces[2, 0] = -1
    m2 = dict(m, F=bad_faces)
    keys = to_dev(want["keys"])
    q = run.quadrics(m2, keys)
    assert np.isfinite(q).all()
    cluster = to_dev(want["cluster"])
    cluster[0] = Vc
    rot, valid, hi, lo = run.remap(m2, cluster, Vc)
    assert valid[1] == 0 and valid[2] == 0 and (rot[1] == -1).all() and hi[2] == -1
    touches0 = (c["F"] == 0).any(1)
    assert (valid[touches0] == 0).all()
    rows = m["rows"].clone()
    rows[0], rows[1] = -7, 3 * nf
    rs = m["row_start"].clone()
    rs[0], rs[-1] = -5, 3 * nf + 9
    q = run.quadrics(dict(m, rows=rows, row_start=rs), keys)
    assert np.isfinite(q).all()
    members = torch.arange(nv, device="cuda")
    members[0], members[1] = -1, nv
    ms = torch.tensor([-3] + [nv + 4] * Vc, device="cuda")
    pos, col, placed = run.clusters(m, keys, ms, members, None, "quadric", Vc)
    assert np.isfinite(pos).all() and (placed[1:] == 3).all()
    order = torch.tensor([nf, -1] + list(range(nf - 2)), device="cuda")
    fk, ck = run.keep_flags(m, Vc, order, to_dev(want["rot"]), to_dev(want["valid"]), to_dev(want["hi"]), to_dev(want["lo"]))
    assert set(np.unique(fk)) <= {0, 1} and set(np.unique(ck)) <= {0, 1}
    nan_v = m["V"].clone()
    nan_v[0, 0], nan_v[1, 1], nan_v[2, 2] = float("nan"), float("inf"), -float("inf")
    k = run.keys(dict(m, V=nan_v))
    idx = SR.key_indices(k)
    assert idx[0, 0] == 0 and idx[1, 1] == SR.INDEX_MAX and idx[2, 2] == 0
    assert np.array_equal(k, SR.cell_keys(nan_v.cpu().numpy(), c["origin"], c["cell"]))


def test_refused_and_empty_calls_write_nothing(libs):
    lib = libs[0]
    name = "unreferenced"
    c, m = SR.case(name), mesh(name)
    want = c["quadric"]
    nv, nf, Vc = m["nv"], m["nf"], want["clusters"]
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    o, cell = m["origin"], m["cell"]
    keys_o, quad_o = Out((nv,), "int64"), Out((nv, 9), "float64")
    pos_o, col_o, placed_o = Out((Vc, 3), "float32"), Out((Vc, 3), "float32"), Out((Vc,), "int32")
    rot_o, valid_o, hi_o, lo_o = Out((nf, 3), "int64"), Out((nf,), "int32"), Out((nf,), "int64"), Out((nf,), "int64")
    fk_o, ck_o = Out((nf,), "int32"), Out((Vc,), "int32")
    keys, cluster = to_dev(want["keys"]), to_dev(want["cluster"])
    _, _, member_start, members = SR.clusters(want["keys"])
    member_start, members = to_dev(member_start), to_dev(members)
    rot, valid, hi, lo = (to_dev(want[k]) for k in ("rot", "valid", "hi", "lo"))
    order = to_dev(SR.sort_order(want["hi"], want["lo"]))
    V, F, RS, R = ptr(m["V"]), ptr(m["F"]), ptr(m["row_start"]), ptr(m["rows"])
    calls = [
        lambda **k: lib.egs_simplify_keys(k.get("V", nv), V, *o, k.get("cell", cell), keys_o.ptr, k.get("mb", 0), s),
        lambda **k: lib.egs_simplify_vertex_quadrics(k.get("V", nv), nf, V, F, RS, R, ptr(keys), *o, k.get("cell", cell),
                                                     quad_o.ptr, k.get("mb", 0), s),
        lambda **k: lib.egs_simplify_clusters(k.get("V", nv), nf, Vc, V, ptr(m["C"]), ptr(keys), ptr(member_start),
                                              ptr(members), None, F, RS, R, *o, k.get("cell", cell), k.get("place", 0),
                                              pos_o.ptr, col_o.ptr, placed_o.ptr, k.get("mb", 0), s),
        lambda **k: lib.egs_simplify_remap_faces(k.get("V", nv), nf, Vc, F, ptr(cluster), rot_o.ptr, valid_o.ptr, hi_o.ptr,
                                                 lo_o.ptr, k.get("mb", 0), s),
        lambda **k: lib.egs_simplify_keep_flags(k.get("F", nf), Vc, ptr(order), ptr(rot), ptr(valid), ptr(hi), ptr(lo),
                                                fk_o.ptr, ck_o.ptr, k.get("mb", 0), s),
    ]
    outs = (keys_o, quad_o, pos_o, col_o, placed_o, rot_o, valid_o, hi_o, lo_o, fk_o, ck_o)
    for call in calls[:4]:
        for kw in (dict(V=-1), dict(mb=-1), dict(mb=8193)):
            assert call(**kw) == BAD_ARG, kw
    for call in calls[:3]:
        for kw in (dict(cell=0.0), dict(cell=float("nan"))):
            assert call(**kw) == BAD_ARG, kw
    for kw in (dict(F=-1), dict(mb=-1), dict(mb=8193)):
        assert calls[4](**kw) == BAD_ARG
    assert calls[2](place=2) == BAD_ARG
    assert calls[2](V=Vc - 1) == BAD_ARG                      # more clusters than vertices
    # aliased outputs
    assert lib.egs_simplify_keys(nv, V, *o, cell, V, 0, s) == BAD_ARG
    assert lib.egs_simplify_remap_faces(nv, nf, Vc, F, ptr(cluster), rot_o.ptr, valid_o.ptr, hi_o.ptr, hi_o.ptr, 0, s) == BAD_ARG
    assert lib.egs_simplify_keep_flags(nf, Vc, ptr(order), ptr(rot), ptr(valid), ptr(hi), ptr(lo), fk_o.ptr, fk_o.ptr, 0,
                                       s) == BAD_ARG
    assert lib.egs_simplify_clusters(nv, nf, Vc, V, ptr(m["C"]), ptr(keys), ptr(member_start), ptr(members), None, F, RS, R,
                                     *o, cell, 0, pos_o.ptr, pos_o.ptr, placed_o.ptr, 0, s) == BAD_ARG
    assert lib.egs_simplify_last_error_string().decode().startswith("egs_simplify error 10001: bad argument")
    # empty inputs: success, no launch
    assert lib.egs_simplify_keys(0, V, *o, cell, keys_o.ptr, 0, s) == 0
    assert lib.egs_simplify_vertex_quadrics(0, nf, V, F, RS, R, ptr(keys), *o, cell, quad_o.ptr, 0, s) == 0
    assert lib.egs_simplify_clusters(nv, nf, 0, V, ptr(m["C"]), ptr(keys), ptr(member_start), ptr(members), None, F, RS, R,
                                     *o, cell, 0, pos_o.ptr, col_o.ptr, placed_o.ptr, 0, s) == 0
    assert lib.egs_simplify_remap_faces(nv, 0, Vc, F, ptr(cluster), rot_o.ptr, valid_o.ptr, hi_o.ptr, lo_o.ptr, 0, s) == 0
    assert lib.egs_simplify_keep_flags(0, 0, None, None, None, None, None, fk_o.ptr, ck_o.ptr, 0, s) == 0
    torch.cuda.synchronize()
    for out in outs:
        assert out.untouched()


# ---------------------------------------------------------------------------------------------------- the Python layer
@pytest.mark.parametrize("name", ["disjoint-0", "degenerate", "one-cell", "opposite", "same-rotation", "ties", "big-index",
                                  "corner", "sphere-floaters@2", "field-17x15x13"])
def test_python_layer_gives_the_abis_bits(libs, name):
    from easygaussiansplatting_amd import mesh as M
    c, m, run = SR.case(name), mesh(name), Runner(libs)
    for placement in SR.PLACEMENTS:
        abi = run.pipeline(name, placement)
        V, F, Cc, info = M.simplify_vertex_clustering(m["V"], m["F"], m["C"], cell_size=m["cell"], origin=m["origin"],
                                                      placement=placement, return_info=True)
        assert V.is_cuda and V.dtype == torch.float32 and F.dtype == torch.int64
        assert same_bits(V.cpu().numpy(), abi["V"]) and np.array_equal(F.cpu().numpy(), abi["F"])
        assert same_bits(Cc.cpu().numpy(), abi["C"])
        want = c[placement]
        assert info == dict(clusters=want["clusters"], placed_mean=want["placed_counts"][0],
                            placed_solved=want["placed_counts"][1], placed_clamped=want["placed_counts"][2],
                            placed_no_face=want["placed_counts"][3], faces_degenerate=want["degenerate"],
                            faces_duplicate=want["duplicate"])
        bare = M.simplify_vertex_clustering(m["V"], m["F"], cell_size=m["cell"], origin=m["origin"], placement=placement)
        assert len(bare) == 3 and bare[2] is None and torch.equal(bare[1], F)
        assert torch.equal(bare[0].view(torch.int32), V.view(torch.int32))
    assert torch.equal(m["V"].cpu(), torch.from_numpy(np.array(c["V"])))           # inputs untouched
    if m["nv"]:
        lo = c["V"].astype(np.float64).min(0)
        # origin = None is the bounding box minimum
        a = M.simplify_vertex_clustering(m["V"], m["F"], m["C"], cell_size=m["cell"])
        b = M.simplify_vertex_clustering(m["V"], m["F"], m["C"], cell_size=m["cell"], origin=tuple(lo))
        assert torch.equal(a[1], b[1]) and all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in (0, 2))
        with pytest.raises(ValueError, match="must not exceed the bounding box minimum"):
            M.simplify_vertex_clustering(m["V"], m["F"], cell_size=m["cell"], origin=tuple(lo + [1e-3, 0, 0]))
        with pytest.raises(ValueError, match="cells or more from the origin"):
            M.simplify_vertex_clustering(m["V"], m["F"], cell_size=m["cell"], origin=tuple(lo - [m["cell"] * 2.0 ** 21, 0, 0]))
        with pytest.raises(ValueError, match="found an index outside"):
            M.simplify_vertex_clustering(m["V"], m["F"] + m["nv"], cell_size=m["cell"])
        bad = m["V"].clone()
        bad[0, 1] = float("nan")
        with pytest.raises(ValueError, match="vertices must be finite"):
            M.simplify_vertex_clustering(bad, m["F"], cell_size=m["cell"])


@pytest.mark.parametrize("name", ["sphere-floaters@2", "field-17x15x13"])
def test_clean_mesh_with_simplification_is_the_steps_composed(libs, name):
    from easygaussiansplatting_amd import mesh as M
    m = mesh(name)
    bits = lambda t: t.contiguous().view(torch.int32)
    V1, F1, C1, N1 = M.clean_mesh(m["V"], m["F"], m["C"], keep_largest=1, smooth_iterations=2, normals=True,
                                  simplify_cell=m["cell"])
    a = M.remove_small_components(m["V"], m["F"], m["C"], keep_largest=1)
    sv = M.smooth_taubin(a[0], a[1], 2)
    s = M.simplify_vertex_clustering(sv, a[1], a[2], cell_size=m["cell"])
    assert torch.equal(F1, s[1]) and torch.equal(bits(V1), bits(s[0])) and torch.equal(bits(C1), bits(s[2]))
    assert torch.equal(bits(N1), bits(M.vertex_normals(s[0], s[1])))
    assert 0 < F1.shape[0] < a[1].shape[0] // 3
    Vm = M.clean_mesh(m["V"], m["F"], m["C"], keep_largest=1, simplify_cell=m["cell"], simplify_placement="mean")
    sm = M.simplify_vertex_clustering(a[0], a[1], a[2], cell_size=m["cell"], placement="mean")
    assert torch.equal(Vm[1], sm[1]) and torch.equal(bits(Vm[0]), bits(sm[0])) and Vm[3] is None
    # without simplify_cell: the bits of the steps before
    plain = M.clean_mesh(m["V"], m["F"], m["C"], keep_largest=1, smooth_iterations=2)
    assert torch.equal(plain[1], a[1]) and torch.equal(bits(plain[0]), bits(sv)) and torch.equal(bits(plain[2]), bits(a[2]))
