"""Feature rendering, host side (no GPU): the float64 reference's own invariants (tests/feature_ref.py) against the
references of the draw pass and of the blend-weight statistics, the C surface of libegs_feat.so against
include/egs_feat.h and ``_featlib.SIGNATURES``, its refusals before any HIP call, the untouched surfaces of the other
three libraries, and the Python-side refusals of ``easygaussiansplatting_amd.features``."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest

from tests import blend_weights_ref as B
from tests import draw_tile_ref as D
from tests import feature_ref as F

torch = pytest.importorskip("torch")

from easygaussiansplatting_amd import _featlib, features            # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "egs_feat.h")
BAD_ARG = 10001
_FAKE = C.c_void_p(4096)        # a pointer nobody dereferences: every call below is refused before any HIP call
CASES = [(n, p) for n in D.SETS for p in D.POLICIES]
NAMES = ["egs_feat_abi_version", "egs_feat_last_error_string", "egs_feature_gather", "egs_feature_render"]


@pytest.fixture(scope="module")
def lib():
    from easygaussiansplatting_amd import _lib
    if not os.path.exists(_featlib.LIB_PATH):
        _lib.build()
    return _featlib.load()


def _nonempty(c, pname):
    m = np.zeros((D.H, D.W), bool)
    for t, l in enumerate(D.lists(c, pname)[0]):
        if len(l):
            tx, ty, x0, y0, ww, hh = D.geom(t)
            m[y0:y0 + hh, x0:x0 + ww] = True
    return m


# -------------------------------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("name,pname", CASES)
def test_colours_as_features_give_the_image(name, pname):
    c = D.case(name)
    fmap = F.case_walk(name, pname, c.arrays["colors"])[0]
    want = D.reference(name, pname)["image"]
    assert fmap.shape == want.shape == (3, D.H, D.W) and fmap.dtype == np.float64
    assert np.abs(fmap - want).max() <= 1e-12


@pytest.mark.parametrize("name,pname", CASES)
def test_an_all_ones_channel_is_the_opacity_and_gathers_the_weight_sum(name, pname):
    c = D.case(name)
    ones_f = np.ones((c.n, 1), np.float32)
    ones_g = np.ones((1, D.H, D.W), np.float32)
    fmap, gath, absg, near = F.case_walk(name, pname, ones_f, ones_g)
    tau = D.reference(name, pname)["final_tau"]
    m = _nonempty(c, pname)
    assert m.any() and np.abs(fmap[0][m] - (1.0 - tau[m])).max() <= 1e-12
    assert not fmap[0][~m].any()
    bref = B.reference(name, pname)
    assert np.abs(gath[:, 0] - bref["sum"]).max() <= 1e-12 and np.array_equal(gath, absg)
    assert np.array_equal(gath[:, 0] == 0, bref["hits"] == 0)
    # the builder lets no live alpha' come near the skip threshold on these sets
    assert near.shape == (D.H, D.W) and not near.any()


@pytest.mark.parametrize("name,pname", CASES)
def test_reference_render_and_gather_are_adjoint(name, pname):
    ref = F.reference(name, pname)
    feats, gmap = F.case_feats(name).astype(np.float64), F.case_gmap(name).astype(np.float64)
    assert feats.shape[1] == F.C_MAX == gmap.shape[0] and np.abs(feats).max() <= 1 and np.abs(gmap).max() <= 1
    # per channel, and with the magnitudes in place of the values so that nothing cancels in the comparison's scale
    lhs = (gmap * ref["map"]).sum((1, 2))
    rhs = (ref["gather"] * feats).sum(0)
    scale = (ref["absg"] * np.abs(feats)).sum(0)
    assert (scale > 0).all() and (np.abs(lhs - rhs) <= 1e-12 * scale).all()
    assert abs(lhs.sum() - rhs.sum()) <= 1e-12 * scale.sum()
    # a test of C channels reads the first C of the C_MAX computed once: the walk is channel by channel
    fmap3, gath3, _, _ = F.case_walk(name, pname, F.case_feats(name)[:, :3], F.case_gmap(name)[:3])
    assert np.array_equal(fmap3, ref["map"][:3]) and np.array_equal(gath3, ref["gather"][:, :3])


def test_floors_are_counts_of_roundings():
    name, pname = "lengths0", "gsplatcu"
    c = D.case(name)
    feats = F.case_feats(name)
    fl = F.pixel_floor(name, pname, feats)
    contrib = D.reference(name, pname)["contrib"]
    assert np.array_equal(fl, 2.0 ** -23 * (2 + contrib))                      # |feat| <= 1
    assert np.array_equal(F.pixel_floor(name, pname, 3 * feats)[contrib > 0] > fl[contrib > 0],
                          np.ones(int((contrib > 0).sum()), bool))
    rf = F.row_floor(name, pname)
    g = int(c.lists[4][7])                                                     # entry 7 of tile 4
    assert np.array_equal(rf[g], 2.0 ** -23 * 9 * F.reference(name, pname)["absg"][g])


# -------------------------------------------------------------------------------------------------------- the C surface
def declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(egs_[a-z0-9_]+)\s*\(", src)))


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip() and ln.split()[-1].startswith("egs_")}


def test_library_exports_what_the_header_declares(lib):
    names = declared_functions()
    assert names == NAMES
    assert _exports(_featlib.LIB_PATH) == set(names)
    assert set(_featlib.SIGNATURES) == set(names)
    src = open(HEADER).read()
    assert re.search(r"^#define\s+EGS_FEAT_ABI_VERSION\s+1\s*$", src, re.M)
    assert re.search(r"^#define\s+EGS_FEAT_MAX_CHANNELS\s+4096\s*$", src, re.M)
    assert lib.egs_feat_abi_version() == _featlib.ABI_VERSION == 1
    assert _featlib.DRAW_MASKED_LISTS == 2 and _featlib.MAX_CHANNELS == 4096 and _featlib.ERR_BAD_ARG == BAD_ARG


def test_the_other_three_libraries_export_nothing_of_it(lib):
    from easygaussiansplatting_amd import _lib, _mcmclib, _prunelib
    for mod in (_lib, _mcmclib, _prunelib):
        assert os.path.exists(mod.LIB_PATH)
        assert not [s for s in _exports(mod.LIB_PATH) if s.startswith("egs_feat") or s.startswith("egs_feature")]
        assert not [k for k in mod.SIGNATURES if k.startswith("egs_feat") or k.startswith("egs_feature")]


def _policy():
    from easygaussiansplatting_amd._lib import EgsPolicy
    pol = EgsPolicy()
    pol.alpha_skip, pol.tau_stop, pol.maha_floor, pol.alpha_clamp = 0.002, 1e-4, 1, 1
    return pol


@pytest.mark.parametrize("fn", ["egs_feature_render", "egs_feature_gather"])
def test_bad_arguments_are_refused_before_the_device(lib, fn):
    err = lib.egs_feat_last_error_string
    F_, N = _FAKE, None
    pol = _policy()
    f = getattr(lib, fn)
    # a: feats (render) / gmap (gather); b: fmap (render) / gfeats (gather)
    call = lambda n=10, w=64, h=48, rec=F_, p=C.byref(pol), ranges=F_, gsid=F_, contrib=F_, flags=0, ch=9, a=F_, b=F_: \
        f(n, w, h, rec, p, ranges, gsid, contrib, flags, ch, a, b, N)
    odd = lambda k: C.c_void_p(4096 + k)
    assert call(n=-1) == BAD_ARG and b"n >= 0" in err()
    assert call(w=0) == BAD_ARG and b"width > 0" in err()
    assert call(h=-3) == BAD_ARG and b"height > 0" in err()
    assert call(p=N) == BAD_ARG and b"pol" in err()
    for flags in (1, 4, 8, 2 | 16, -1):
        assert call(flags=flags) == BAD_ARG and b"flags" in err(), flags
    for ch in (0, -1, 4097, 1 << 20):
        assert call(ch=ch) == BAD_ARG and b"channels" in err(), ch
    assert call(rec=N) == BAD_ARG and b"rec" in err()
    for k in (4, 8, 12):
        assert call(rec=odd(k)) == BAD_ARG and b"rec" in err()            # 16-byte alignment
    for key in ("ranges", "gsid", "contrib"):
        assert call(**{key: N}) == BAD_ARG and key.encode() in err()
        assert call(**{key: odd(2)}) == BAD_ARG and key.encode() in err()  # 4-byte alignment
    first, second = (b"feats", b"fmap") if fn == "egs_feature_render" else (b"gmap", b"gfeats")
    assert call(a=N) == BAD_ARG and first in err()
    assert call(a=odd(1)) == BAD_ARG and first in err()
    assert call(b=N) == BAD_ARG and second in err()
    assert call(b=odd(2)) == BAD_ARG and second in err()
    assert call(n=1 << 28, flags=2) == BAD_ARG and b"EGS_GSID_BITS" in err()   # a masked list value holds 28 index bits
    # an empty call: its sizes, flags, policy and channel count are still checked
    assert call(n=0, w=0) == BAD_ARG and call(n=0, flags=4) == BAD_ARG and call(n=0, p=N) == BAD_ARG
    assert call(n=0, ch=0) == BAD_ARG and call(n=0, ch=4097) == BAD_ARG
    if fn == "egs_feature_render":
        # ... and so is the map it would zero-fill
        assert call(n=0, rec=N, ranges=N, gsid=N, contrib=N, a=N, b=N) == BAD_ARG and b"fmap" in err()
        assert call(n=0, b=odd(2)) == BAD_ARG and b"fmap" in err()
    else:
        # the gather of nothing is no error and touches nothing
        assert call(n=0, rec=N, ranges=N, gsid=N, contrib=N, a=N, b=N) == 0


def test_missing_library_raises(monkeypatch, tmp_path):
    from easygaussiansplatting_amd import _lib
    monkeypatch.setattr(_featlib, "_lib", None)
    monkeypatch.setattr(_featlib, "LIB_PATH", str(tmp_path / "libegs_feat.so"))
    with pytest.raises(_lib.EgsLibraryError):
        _featlib.load()


# ---------------------------------------------------------------------------------------------------- Python-side refusals
def _fake_state(n=5, w=32, h=16):
    return types.SimpleNamespace(patch_count=lambda: 0, depths=torch.zeros(n), culled=False, width=w, height=h)


def test_python_refuses_what_is_no_device_tensor():
    st = _fake_state()
    with pytest.raises(TypeError):
        features.render_features(st, np.zeros((5, 3), np.float32))
    with pytest.raises(TypeError):
        features.gather_features(st, [[0.0]])
    with pytest.raises(ValueError):
        features.render_features(st, torch.zeros(5, 3))                        # lives on the CPU
    with pytest.raises(ValueError):
        features.gather_features(st, torch.zeros(3, 16, 32))
    with pytest.raises(ValueError):
        features.splat_features(0, 32, *[None] * 8)
    with pytest.raises(ValueError):
        features.splat_gather(16, -1, *[None] * 8)
    with pytest.raises(TypeError):
        features.splat_features(16, 32, None, None, None, None, None, None, None, None)
    with pytest.raises(ValueError):
        features.lift([], [])
    with pytest.raises(ValueError):
        features.lift([st, st], [torch.zeros(3, 16, 32)])
    with pytest.raises(ValueError):
        features._channels(0, "x")
    with pytest.raises(ValueError):
        features._channels(4097, "x")
    assert features._channels(1, "x") == 1 and features._channels(4096, "x") == 4096


def test_trainer_has_the_convenience():
    from easygaussiansplatting_amd.trainer import Trainer
    assert callable(Trainer.render_features)
