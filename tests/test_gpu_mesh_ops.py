"""libegs_meshops.so on the GPU, called through its C ABI on buffers between guard bands, against the numpy
definitions of tests/mesh_ops_ref.py: labels, counts, keep flags, compacted faces and kept counts exactly; compacted rows
bit for bit; every output the same bits on a second run, on grids of 1 and 3 workgroups and on a side stream; normals
within 2^-23 of float64 on the decided vertices; Taubin smoothing under the rule of tests/tsdf_ref.py (4 x the float32
restatement's loss, at least one float32 ulp of the largest coordinate; both numbers printed).  Then the Python layer
against the ABI's bits."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import loss_abi as LA
from tests import mesh_ops_ref as MR

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CASES = list(MR.BUILDERS)
BAD_ARG = 10001


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from easygaussiansplatting_amd import _meshopslib
    return _meshopslib.load()


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
    c = MR.case(name)
    row_start, rows = MR.incidence(c["F"], len(c["V"]))
    return dict(nv=len(c["V"]), nf=len(c["F"]), V=to_dev(c["V"]), F=to_dev(c["F"]), C=to_dev(c["C"]),
                row_start=to_dev(row_start), rows=to_dev(rows))


class Runner:
    """the entry points on one grid cap and one stream"""

    def __init__(self, lib, max_blocks=0, side_stream=False):
        self.lib, self.mb = lib, max_blocks
        self.stream = torch.cuda.Stream() if side_stream else torch.cuda.current_stream()

    def _run(self, fn, *args):
        torch.cuda.synchronize()
        rc = fn(*args, self.mb, C.c_void_p(self.stream.cuda_stream))
        torch.cuda.synchronize()
        return rc

    def components(self, m):
        out = [Out((m["nv"],), "int32") for _ in range(3)]
        assert self._run(self.lib.egs_meshops_components, m["nv"], m["nf"], ptr(m["F"]), *[o.ptr for o in out]) == 0
        return [o.numpy() for o in out]

    def keep_flags(self, m, label, comp_faces, min_faces, keep_largest):
        rank = None if keep_largest is None else to_dev(MR.ranks(comp_faces))
        lab, cf = to_dev(label), to_dev(comp_faces)
        vk, fk = Out((m["nv"],), "int32"), Out((m["nf"],), "int32")
        assert self._run(self.lib.egs_meshops_keep_flags, m["nv"], m["nf"], ptr(m["F"]), ptr(lab), ptr(cf), ptr(rank),
                         0 if min_faces is None else min_faces, 0 if keep_largest is None else keep_largest, vk.ptr,
                         fk.ptr) == 0
        return vk.numpy(), fk.numpy()

    def compact(self, m, vkeep, fkeep, normals=None):
        vk, fk = to_dev(vkeep), to_dev(fkeep)
        vs, fs = torch.cumsum(vk, 0, dtype=torch.int64), torch.cumsum(fk, 0, dtype=torch.int64)
        Vk = int(vs[-1]) if m["nv"] else 0
        Fk = int(fs[-1]) if m["nf"] else 0
        ov, oc, of = Out((Vk, 3), "float32"), Out((Vk, 3), "float32"), Out((Fk, 3), "int64")
        on = None if normals is None else Out((Vk, 3), "float32")
        assert self._run(self.lib.egs_meshops_compact, m["nv"], m["nf"], ptr(m["V"]), ptr(m["C"]), ptr(normals),
                         ptr(m["F"]), ptr(vk), ptr(fk), ptr(vs), ptr(fs), Vk, Fk, ov.ptr, oc.ptr,
                         None if on is None else on.ptr, of.ptr) == 0
        return Vk, Fk, ov.numpy(), oc.numpy(), of.numpy(), None if on is None else on.numpy()

    def normals(self, m):
        out = Out((m["nv"], 3), "float32")
        assert self._run(self.lib.egs_meshops_vertex_normals, m["nv"], m["nf"], ptr(m["V"]), ptr(m["F"]),
                         ptr(m["row_start"]), ptr(m["rows"]), out.ptr) == 0
        return out.numpy()

    def taubin(self, m, iterations, lam=MR.LAM, mu=MR.MU):
        out, tmp = Out((m["nv"], 3), "float32"), Out((m["nv"], 3), "float32")
        before = m["V"].clone()
        assert self._run(self.lib.egs_meshops_taubin, m["nv"], m["nf"], ptr(m["V"]), ptr(m["F"]), ptr(m["row_start"]),
                         ptr(m["rows"]), iterations, lam, mu, out.ptr, tmp.ptr) == 0
        assert torch.equal(before.view(torch.int32), m["V"].view(torch.int32)), "the input was modified"
        tmp.numpy()
        return out.numpy()


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@functools.lru_cache(maxsize=None)
def taubin_refs(name, iterations):
    c = MR.case(name)
    return MR.taubin(c["V"], c["F"], iterations), MR.taubin(c["V"], c["F"], iterations, dtype=np.float32)


# ------------------------------------------------------------------------------------------------------------- integers
@pytest.mark.parametrize("name", CASES)
def test_integer_outputs_equal_the_reference(lib, name):
    c, m, run = MR.case(name), mesh(name), Runner(lib)
    label, cf, cv = run.components(m)
    assert np.array_equal(label, c["label"]) and label.dtype == np.int32
    assert np.array_equal(cf, c["comp_faces"]) and np.array_equal(cv, c["comp_verts"])
    for mf, kl in MR.REMOVALS:
        vkeep, fkeep = run.keep_flags(m, label, cf, mf, kl)
        want_v, want_f = MR.keep_flags(c["F"], m["nv"], mf, kl)
        assert np.array_equal(vkeep, want_v) and np.array_equal(fkeep, want_f), (mf, kl)
        Vk, Fk, ov, oc, of, on = run.compact(m, vkeep, fkeep, normals=m["C"].flip(1).contiguous())
        rv, rf, rc, rn = MR.remove(c["V"], c["F"], c["C"], np.ascontiguousarray(c["C"][:, ::-1]), mf, kl)
        assert (Vk, Fk) == (len(rv), len(rf)), (mf, kl)
        assert np.array_equal(of, rf) and of.dtype == np.int64
        assert same_bits(ov, rv) and same_bits(oc, rc) and same_bits(on, rn), (mf, kl)


# ------------------------------------------------------------------------------------------------------ reproducibility
@pytest.mark.parametrize("name", CASES)
def test_every_output_is_the_same_on_every_grid_and_stream(lib, name):
    m = mesh(name)

    def everything(run):
        label, cf, cv = run.components(m)
        vkeep, fkeep = run.keep_flags(m, label, cf, 2, 3)
        comp = run.compact(m, vkeep, fkeep)
        return [label, cf, cv, vkeep, fkeep, comp[2], comp[3], comp[4], run.normals(m), run.taubin(m, 3)]

    first = everything(Runner(lib))
    for kw in (dict(), dict(max_blocks=1), dict(max_blocks=3), dict(side_stream=True)):
        for a, b in zip(first, everything(Runner(lib, **kw))):
            assert same_bits(a, b), kw


# --------------------------------------------------------------------------------------------------------------- normals
@pytest.mark.parametrize("name", CASES)
def test_normals_are_the_float64_normals_rounded_once(lib, name):
    c, m = MR.case(name), mesh(name)
    got = Runner(lib).normals(m)
    want, decided, has_face = MR.normals(c["V"], c["F"])
    assert np.isfinite(got).all()
    assert (got[~has_face].view(np.int32) == 0).all()                 # exactly +0
    d = decided & has_face
    err = float(np.abs(got[d].astype(np.float64) - want[d]).max()) if d.any() else 0.0
    print("%s: normals of %d decided vertices within %.3e (2^-23 = %.3e)" % (name, int(d.sum()), err, 2.0 ** -23))
    assert err <= 2.0 ** -23
    # degenerate rows: S = 0 exactly, so is the normal
    zero = d & (np.abs(want).sum(1) == 0)
    assert (got[zero] == 0).all()
    und = got[~decided & has_face].astype(np.float64)
    ln = np.linalg.norm(und, axis=1)
    assert ((ln == 0) | (np.abs(ln - 1) <= 1e-6)).all()


# ---------------------------------------------------------------------------------------------------------------- Taubin
@pytest.mark.parametrize("iterations", [1, 10])
@pytest.mark.parametrize("name", CASES)
def test_taubin_against_float64(lib, name, iterations):
    c, m = MR.case(name), mesh(name)
    got = Runner(lib).taubin(m, iterations)
    t64, t32 = taubin_refs(name, iterations)
    if m["nv"] == 0:
        assert got.shape == (0, 3)
        return
    e_ref, e_hip = float(np.abs(t32 - t64).max()), float(np.abs(got.astype(np.float64) - t64).max())
    bound = max(4.0 * e_ref, MR.ulp32(np.abs(t64).max()))
    print("%s, %d iterations: e_ref %.3e | e_hip %.3e | bound %.3e" % (name, iterations, e_ref, e_hip, bound))
    assert np.isfinite(got).all() and e_hip <= bound
    lone = np.diff(MR.incidence(c["F"], m["nv"])[0]) == 0
    assert same_bits(got[lone], c["V"][lone])
    if m["nf"]:
        assert not same_bits(got, c["V"])


def test_zero_iterations_copy_the_input(lib):
    m = mesh("equal-counts")
    assert same_bits(Runner(lib).taubin(m, 0), MR.case("equal-counts")["V"])
    assert same_bits(Runner(lib, max_blocks=1).taubin(m, 0), MR.case("equal-counts")["V"])


# -------------------------------------------------------------------------------------------- refused and empty calls
def test_refused_and_empty_calls_write_nothing(lib):
    m = mesh("equal-counts")
    nv, nf = m["nv"], m["nf"]
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    i32 = lambda n: Out((n,), "int32")
    f32 = lambda n: Out((n, 3), "float32")
    label, cf, cv = i32(nv), i32(nv), i32(nv)
    vk, fk = i32(nv), i32(nf)
    ov, oc, on, of = f32(nv), f32(nv), f32(nv), Out((nf, 3), "int64")
    lab_in, cf_in = to_dev(MR.case("equal-counts")["label"]), to_dev(MR.case("equal-counts")["comp_faces"])
    scan_v, scan_f = torch.arange(1, nv + 1, device="cuda"), torch.arange(1, nf + 1, device="cuda")
    ones_v, ones_f = torch.ones(nv, dtype=torch.int32, device="cuda"), torch.ones(nf, dtype=torch.int32, device="cuda")
    F, V, RS, R = ptr(m["F"]), ptr(m["V"]), ptr(m["row_start"]), ptr(m["rows"])
    calls = [
        lambda **k: lib.egs_meshops_components(k.get("V", nv), nf, F, label.ptr, cf.ptr, cv.ptr, k.get("mb", 0), s),
        lambda **k: lib.egs_meshops_keep_flags(k.get("V", nv), nf, F, ptr(lab_in), ptr(cf_in), None, 2, 0, vk.ptr, fk.ptr,
                                               k.get("mb", 0), s),
        lambda **k: lib.egs_meshops_compact(k.get("V", nv), nf, V, ptr(m["C"]), k.get("n"), F, ptr(ones_v), ptr(ones_f),
                                            ptr(scan_v), ptr(scan_f), nv, nf, ov.ptr, oc.ptr, k.get("on"), of.ptr,
                                            k.get("mb", 0), s),
        lambda **k: lib.egs_meshops_vertex_normals(k.get("V", nv), nf, V, F, RS, R, on.ptr, k.get("mb", 0), s),
        lambda **k: lib.egs_meshops_taubin(k.get("V", nv), nf, V, F, RS, R, k.get("it", 2), k.get("lam", 0.5), -0.53, ov.ptr,
                                           oc.ptr, k.get("mb", 0), s),
    ]
    outs = (label, cf, cv, vk, fk, ov, oc, on, of)
    for call in calls:
        for kw in (dict(V=-1), dict(mb=-1), dict(mb=8193)):
            assert call(**kw) == BAD_ARG, kw
    # compact with colours and normals aliased (the same input twice) is refused too
    assert calls[2](n=ptr(m["C"]), on=on.ptr) == BAD_ARG
    assert calls[2](n=ptr(m["V"])) == BAD_ARG                     # normals without a place to put them
    assert calls[4](it=-1) == BAD_ARG and calls[4](lam=float("nan")) == BAD_ARG
    assert lib.egs_meshops_components(nv, nf, F, label.ptr, label.ptr, cv.ptr, 0, s) == BAD_ARG
    assert lib.egs_meshops_vertex_normals(nv, nf, V, F, RS, R, V, 0, s) == BAD_ARG
    assert lib.egs_meshops_taubin(nv, nf, V, F, RS, R, 2, 0.5, -0.53, ov.ptr, ov.ptr, 0, s) == BAD_ARG
    assert lib.egs_meshops_last_error_string().decode().startswith("egs_meshops error 10001: bad argument")
    # empty meshes: success, no launch
    assert lib.egs_meshops_components(0, nf, F, label.ptr, cf.ptr, cv.ptr, 0, s) == 0
    assert lib.egs_meshops_components(0, 0, None, None, None, None, 0, s) == 0
    assert lib.egs_meshops_keep_flags(0, 0, None, None, None, None, 2, 0, vk.ptr, fk.ptr, 0, s) == 0
    assert lib.egs_meshops_compact(nv, nf, V, ptr(m["C"]), None, F, ptr(ones_v), ptr(ones_f), ptr(scan_v), ptr(scan_f), 0, 0,
                                   ov.ptr, oc.ptr, None, of.ptr, 0, s) == 0
    assert lib.egs_meshops_vertex_normals(0, nf, V, F, RS, R, on.ptr, 0, s) == 0
    assert lib.egs_meshops_taubin(0, 0, None, None, None, None, 2, 0.5, -0.53, ov.ptr, oc.ptr, 0, s) == 0
    torch.cuda.synchronize()
    for o in outs:
        assert o.untouched()


# ---------------------------------------------------------------------------------------------------- the Python layer
@pytest.mark.parametrize("name", ["disjoint-0", "disjoint-65", "unreferenced", "degenerate", "equal-counts", "tets-300",
                                  "sphere-floaters", "field-17x15x13"])
def test_python_layer_gives_the_abis_bits(lib, name):
    from easygaussiansplatting_amd import mesh as M
    c, m, run = MR.case(name), mesh(name), Runner(lib)
    comp = M.connected_components(m["F"], m["nv"])
    label, cf, cv = run.components(m)
    assert isinstance(comp, M.Components) and all(t.is_cuda and t.dtype == torch.int32 for t in comp)
    assert np.array_equal(comp.label.cpu().numpy(), label) and np.array_equal(comp.comp_faces.cpu().numpy(), cf)
    assert np.array_equal(comp.comp_verts.cpu().numpy(), cv)
    nrm = M.vertex_normals(m["V"], m["F"])
    assert same_bits(nrm.cpu().numpy(), run.normals(m))
    assert same_bits(M.smooth_taubin(m["V"], m["F"], iterations=3).cpu().numpy(), run.taubin(m, 3))
    assert same_bits(M.smooth_taubin(m["V"], m["F"]).cpu().numpy(), run.taubin(m, 10))
    for mf, kl in MR.REMOVALS:
        got = M.remove_small_components(m["V"], m["F"], m["C"], min_faces=mf, keep_largest=kl, normals=nrm)
        vkeep, fkeep = run.keep_flags(m, label, cf, mf, kl)
        _, _, ov, oc, of, on = run.compact(m, vkeep, fkeep, normals=nrm)
        assert same_bits(got[0].cpu().numpy(), ov) and np.array_equal(got[1].cpu().numpy(), of)
        assert same_bits(got[2].cpu().numpy(), oc) and same_bits(got[3].cpu().numpy(), on)
        want = MR.remove(c["V"], c["F"], c["C"], None, mf, kl)
        assert same_bits(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1])
    bare = M.remove_small_components(m["V"], m["F"], keep_largest=1)
    assert bare[2] is None and bare[3] is None
    # clean_mesh is the three steps composed
    V1, F1, C1, N1 = M.clean_mesh(m["V"], m["F"], m["C"], min_faces=2, keep_largest=2, smooth_iterations=2, normals=True)
    a = M.remove_small_components(m["V"], m["F"], m["C"], min_faces=2, keep_largest=2)
    sv = M.smooth_taubin(a[0], a[1], 2)
    assert torch.equal(F1, a[1]) and torch.equal(C1.view(torch.int32), a[2].view(torch.int32))
    assert torch.equal(V1.view(torch.int32), sv.view(torch.int32))
    assert torch.equal(N1.view(torch.int32), M.vertex_normals(sv, a[1]).view(torch.int32))
    plain = M.clean_mesh(m["V"], m["F"])
    assert torch.equal(plain[0], m["V"]) and torch.equal(plain[1], m["F"]) and plain[2] is None and plain[3] is None
    assert torch.equal(m["V"].cpu(), torch.from_numpy(np.array(c["V"])))           # inputs untouched
    if m["nf"]:
        with pytest.raises(ValueError, match="found an index outside"):
            M.connected_components(m["F"], int(c["F"].max()))
