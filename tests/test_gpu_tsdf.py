"""TSDF integration (csrc/egs_tsdf.hip: k_tsdf_integrate) against the float64 form of its definition
(tests/tsdf_ref.py) under that module's rule: on the samples whose decisions have margin the updated set is the
reference's exactly, and tsdf, weight and colour are within 4 x what the float32 restatement loses on the case, at least
one float32 ulp of the plane's largest entry.

The C ABI is called directly on planes the test owns, between guard bands (tests/loss_abi.py) that must be intact
afterwards.  The planes are read-modify-write, so they start from the volume's initial state (1, 0, 0) or from a previous
view and are not NaN-filled; a sample the view skips must keep its previous BITS.

Cases: tests/tsdf_ref.case_list -- nx in {1, 3, 4, 5, 7, 64, 65} with ny x nz = 3 x 2 (rows that are no multiple of the
16-B quad: every alignment of a row's first and last quad), 9 x 7 x 5 and 130 x 33 x 9, each from four cameras (one with
samples behind it, one with most samples off the image, one whose opacity is under alpha_min on half the image, all with
the three bands of sdf somewhere), at 16 x 12 and 33 x 20 pixels, colour / alpha / weight on and off.  THE STRIDE WALK:
every case is launched again with ``max_blocks`` = 1 (and 3): 130 x 33 x 9 has 297 rows of 34 quads, 10098 items, 40
workgroups' worth, which one workgroup walks in 40 strides; the planes must equal the default launch's bit for bit.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import tsdf_ref as TR

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.loss_abi import bits, dev, guarded, guards_intact  # noqa: E402  (needs torch)

CASES = TR.case_list()
BAD_ARG = 10001


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from easygaussiansplatting_amd import _tsdflib
    return _tsdflib.load()


class Planes:
    """tsdf, weight and (optionally) colour of a lattice on the device, each between guard bands"""

    def __init__(self, dims, color, state=None):
        nx, ny, nz = dims
        self.dims, self.n = dims, nx * ny * nz
        self.all, self.t = {}, {}
        init = dict(tsdf=1.0, weight=0.0, color=0.0)
        for k, planes in (("tsdf", 1), ("weight", 1), ("color", 3 if color else 0)):
            if planes == 0:
                self.t[k] = None
                continue
            whole, inner = guarded(4 * planes * self.n)
            v = inner.view(torch.float32)
            if state is None:
                v.fill_(init[k])
            else:
                v.copy_(state.t[k])
            self.all[k], self.t[k] = whole, v
        assert all(t is None or t.data_ptr() % 16 == 0 for t in self.t.values())

    def host(self):
        nx, ny, nz = self.dims
        shp = {"tsdf": (nz, ny, nx), "weight": (nz, ny, nx), "color": (3, nz, ny, nx)}
        return {k: None if t is None else t.cpu().numpy().reshape(shp[k]).copy() for k, t in self.t.items()}

    def check_guards(self, what):
        for k, whole in self.all.items():
            assert guards_intact(whole), "%s: the kernel wrote outside %s" % (what, k)

    def same_bits(self, other):
        return all(t is None or torch.equal(bits(t), bits(other.t[k])) for k, t in self.t.items())


def on_device(view):
    out = {k: None if view.get(k) is None else dev(view[k]) for k in ("depth", "alpha", "image", "weight")}
    out["R"], out["t"] = dev(np.asarray(view["R"]).reshape(-1)), dev(view["t"])
    return out


def abi_integrate(lib, lat, view, dv, planes, box=None, max_blocks=0, stream=None, **over):
    """egs_tsdf_integrate of ``view`` (its device tensors ``dv``) into ``planes`` -> rc; asserts the guards"""
    nx, ny, nz = lat["dims"]
    H, W = view["depth"].shape
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    st = stream if stream is not None else torch.cuda.current_stream()
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    a = dict(nx=nx, ny=ny, nz=nz, o=lat["origin"], voxel=lat["voxel"], box=box or (0, nx, 0, ny, 0, nz),
             tsdf=p(planes.t["tsdf"]), weight=p(planes.t["weight"]), color=p(planes.t["color"]), H=H, W=W,
             depth=p(dv["depth"]), alpha=p(dv["alpha"]), image=p(dv["image"]) if planes.t["color"] is not None else None,
             pw=p(dv["weight"]), K=view["K"], R=p(dv["R"]), t=p(dv["t"]), trunc=view["trunc"], alpha_min=view["alpha_min"],
             near=view["near"], depth_max=float("inf") if view.get("depth_max") is None else view["depth_max"],
             max_blocks=max_blocks)
    a.update(over)
    rc = lib.egs_tsdf_integrate(a["nx"], a["ny"], a["nz"], *[float(v) for v in a["o"]], float(a["voxel"]), *a["box"],
                                a["tsdf"], a["weight"], a["color"], a["H"], a["W"], a["depth"], a["alpha"], a["image"],
                                a["pw"], *[float(v) for v in a["K"]], a["R"], a["t"], float(a["trunc"]),
                                float(a["alpha_min"]), float(a["near"]), float(a["depth_max"]), a["max_blocks"],
                                C.c_void_p(st.cuda_stream))
    st.synchronize()
    torch.cuda.synchronize()
    planes.check_guards("%s %s" % (lat["dims"], view.get("cam")))
    return rc


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (lat, view, decided, float64 state, updated mask, the float32 restatement's loss per plane)"""
    c = CASES[name]
    lat, view = TR.build_case(c)
    dec = TR.decided(lat, view)
    s64, s32 = TR.new_state(c["dims"], c["color"]), TR.new_state(c["dims"], c["color"], np.float32)
    m64 = TR.integrate(s64, lat, view)
    TR.integrate(s32, lat, view, np.float32)
    return lat, view, dec, s64, m64, TR.errors(s32, s64, dec & m64)


def check_against(got, want, upd, dec, e_ref, before, what):
    """THE RULE on the decided samples; a sample whose weight did not change keeps every plane's bits"""
    changed = got["weight"].view(np.int32) != before["weight"].view(np.int32)
    assert np.array_equal(changed[dec], upd[dec]), "%s: %d decided samples updated on one side only" % (
        what, int((changed != upd)[dec].sum()))
    e_hip, bound = TR.errors(got, want, dec & upd), TR.bounds(e_ref, want)
    print("%s: updated %d, left out %d | e_ref %s | e_hip %s" % (
        what, int(upd.sum()), int((~dec).sum()), {k: "%.2e" % v for k, v in e_ref.items()},
        {k: "%.2e" % v for k, v in e_hip.items()}))
    for k in e_hip:
        assert e_hip[k] <= bound[k], "%s: %s is off by %.3e, the rule allows %.3e" % (what, k, e_hip[k], bound[k])
    for k in ("tsdf", "color"):
        if got[k] is not None:
            m = np.broadcast_to(~changed, got[k].shape)
            assert np.array_equal(got[k].view(np.int32)[m], before[k].view(np.int32)[m]), \
                "%s: %s of a sample the view skipped was written" % (what, k)


@pytest.mark.parametrize("name", list(CASES))
def test_case(lib, name):
    from easygaussiansplatting_amd.mesh import frustum_box
    c = CASES[name]
    lat, view, dec, want, upd, e_ref = reference(name)
    dv = on_device(view)
    planes = Planes(c["dims"], c["color"])
    before = planes.host()
    assert abi_integrate(lib, lat, view, dv, planes) == 0, name
    got = planes.host()
    assert all(v is None or np.isfinite(v).all() for v in got.values())
    check_against(got, want, upd, dec, e_ref, before, name)
    # the same bits twice, with the grid capped (the stride walk), and on the frustum's sub-box
    again = Planes(c["dims"], c["color"])
    assert abi_integrate(lib, lat, view, dv, again) == 0 and again.same_bits(planes), "%s: two runs differ" % name
    for cap in (1, 3):
        capped = Planes(c["dims"], c["color"])
        assert abi_integrate(lib, lat, view, dv, capped, max_blocks=cap) == 0
        assert capped.same_bits(planes), "%s: max_blocks=%d differs from the default grid" % (name, cap)
    far = None if view.get("depth_max") is None else view["depth_max"] + view["trunc"]
    box = frustum_box(lat["origin"], lat["voxel"], lat["dims"], view["K"], view["depth"].shape, view["R"], view["t"],
                      view["near"], far)
    boxed = Planes(c["dims"], c["color"])
    assert abi_integrate(lib, lat, view, dv, boxed, box=box) == 0
    assert boxed.same_bits(planes), "%s: the sub-box %s differs from the full lattice" % (name, box)


@pytest.mark.parametrize("dims", [(7, 3, 2), (65, 3, 2), (9, 7, 5), (130, 33, 9)], ids=lambda d: "%dx%dx%d" % d)
def test_three_views_in_order_on_the_previous_state(lib, dims):
    """view after view into the same planes: the reference's three views in the same order; what a later view skips keeps
    the bits the earlier ones left (a non-trivial previous state); every odd sub-box of the later views gives the same"""
    lat = TR.make_lattice(dims)
    views = [TR.make_view(lat, "front", 20, 33, seed=1),
             TR.make_view(lat, "oblique", 12, 16, weight=True, half_alpha=True, seed=2),
             TR.make_view(lat, "inside", 20, 33, alpha=False, seed=3, depth_max=1.5)]
    s64, s32 = TR.new_state(dims), TR.new_state(dims, True, np.float32)
    planes = Planes(dims, True)
    dec = np.ones(dims[::-1], bool)
    for k, view in enumerate(views):
        dec &= TR.decided(lat, view)
        upd = TR.integrate(s64, lat, view)
        TR.integrate(s32, lat, view, np.float32)
        before = planes.host()
        boxed = Planes(dims, True, state=planes)
        assert abi_integrate(lib, lat, view, on_device(view), planes) == 0
        got = planes.host()
        e_ref = TR.errors(s32, s64, dec & (s64["weight"] > 0))
        # (the set of updated samples of THIS view, the values of all views so far)
        changed = got["weight"].view(np.int32) != before["weight"].view(np.int32)
        assert np.array_equal(changed[dec], upd[dec]), (dims, k)
        check_against(got, s64, upd, dec, e_ref, before, "%s view %d" % (dims, k))
        seen = dec & (s64["weight"] > 0)
        e_all, bound = TR.errors(got, s64, seen), TR.bounds(e_ref, s64)
        assert all(e_all[p] <= bound[p] for p in e_all), (dims, k, e_all, bound)
        # a sub-box: only its samples change, and they change as in the full launch
        nx, ny, nz = dims
        box = (nx // 3, nx - nx // 4, 1, ny, 0, nz - 1)
        assert abi_integrate(lib, lat, view, on_device(view), boxed, box=box) == 0
        inbox = np.zeros(dims[::-1], bool)
        inbox[box[4]:box[5], box[2]:box[3], box[0]:box[1]] = True
        part = boxed.host()
        for p in ("tsdf", "weight", "color"):
            m = np.broadcast_to(inbox, part[p].shape)
            assert np.array_equal(part[p].view(np.int32)[m], got[p].view(np.int32)[m]), (dims, k, p)
            assert np.array_equal(part[p].view(np.int32)[~m], before[p].view(np.int32)[~m]), (dims, k, p)
    assert float(s64["weight"].max()) > 1.0 and (dims != (130, 33, 9) or (s64["weight"] == 0).any())     # seen twice


def test_a_side_stream_gives_the_default_stream_bits(lib):
    name = next(n for n, c in CASES.items() if c["dims"] == (130, 33, 9) and c["cam"] == "front")
    lat, view = TR.build_case(CASES[name])
    dv = on_device(view)
    a, b = Planes(CASES[name]["dims"], True), Planes(CASES[name]["dims"], True)
    assert abi_integrate(lib, lat, view, dv, a) == 0
    assert abi_integrate(lib, lat, view, dv, b, stream=torch.cuda.Stream()) == 0
    assert a.same_bits(b) and float(a.t["weight"].max()) > 0


def test_bad_arguments_return_10001_and_write_nothing(lib):
    dims = (9, 7, 5)
    lat = TR.make_lattice(dims)
    view = TR.make_view(lat, "front", 12, 16, weight=True)
    dv = on_device(view)
    planes = Planes(dims, True)
    for k in ("tsdf", "weight", "color"):
        planes.t[k].copy_(torch.arange(planes.t[k].numel(), device="cuda", dtype=torch.float32) * 0.001 - 0.1)
    before = Planes(dims, True, state=planes)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    bad = [dict(nx=0), dict(voxel=0.0), dict(voxel=float("nan")), dict(box=(0, 10, 0, 7, 0, 5)), dict(box=(4, 3, 0, 7, 0, 5)),
           dict(box=(0, 9, 0, 7, -1, 5)), dict(tsdf=None), dict(weight=None), dict(color=None), dict(image=None),
           dict(tsdf=C.c_void_p(planes.t["tsdf"].data_ptr() + 4)), dict(weight=ptr(planes.t["tsdf"])),
           dict(color=ptr(planes.t["weight"])), dict(depth=None), dict(H=0), dict(W=-1), dict(K=(0.0, 1.0, 1.0, 1.0)),
           dict(K=(10.0, 10.0, float("inf"), 1.0)), dict(R=None), dict(t=None), dict(trunc=0.0), dict(trunc=float("inf")),
           dict(alpha_min=-0.5), dict(near=float("nan")), dict(depth_max=0.0), dict(depth_max=float("nan")),
           dict(max_blocks=-2), dict(max_blocks=1 << 20), dict(depth=ptr(planes.t["tsdf"])),
           dict(image=ptr(planes.t["color"]))]
    for kw in bad:
        assert abi_integrate(lib, lat, view, dv, planes, **kw) == BAD_ARG, kw
        assert lib.egs_tsdf_last_error_string().decode().startswith("egs_tsdf error 10001: bad argument"), kw
        assert planes.same_bits(before), "%r: refused, yet a plane was written" % (kw,)
    # an empty box: success, nothing written
    assert abi_integrate(lib, lat, view, dv, planes, box=(2, 2, 0, 7, 0, 5)) == 0 and planes.same_bits(before)
    assert abi_integrate(lib, lat, view, dv, planes) == 0 and not planes.same_bits(before)


def test_the_python_layer_clips_to_the_frustum_and_gives_the_abi_bits(lib):
    """``mesh.TSDFVolume.integrate``: the default (clipped) call, the unclipped call and the ABI call agree to the bit;
    a camera object with numpy fields and one with device tensors are taken alike"""
    from easygaussiansplatting_amd import scene as S
    from easygaussiansplatting_amd.function import Camera
    from easygaussiansplatting_amd.mesh import TSDFVolume
    dims = (65, 33, 9)
    lat = TR.make_lattice(dims)
    view = TR.make_view(lat, "narrow", 20, 33, weight=True)
    dv = on_device(view)
    planes = Planes(dims, True)
    assert abi_integrate(lib, lat, view, dv, planes) == 0
    H, W = view["depth"].shape
    cams = [S.Camera(W, H, *view["K"], view["R"], view["t"]), Camera(W, H, *view["K"], view["R"], view["t"])]
    for cam in cams:
        for clip in (True, False):
            vol = TSDFVolume(lat["origin"], lat["voxel"], dims, trunc=view["trunc"])
            vol.integrate(dv["depth"][None], dv["alpha"][None], cam, image=dv["image"], weight=dv["weight"],
                          clip_to_frustum=clip)
            torch.cuda.synchronize()
            nx, ny, nz = dims
            box = vol.last_box
            assert (box == (0, nx, 0, ny, 0, nz)) == (not clip), box
            for k in ("tsdf", "weight", "color"):
                assert torch.equal(bits(getattr(vol, k).reshape(-1)), bits(planes.t[k])), (clip, k)
    assert float(planes.t["weight"].max()) > 0
