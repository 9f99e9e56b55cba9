"""MCMC densification, host side (no GPU): the invariants of the float64 restatement (tests/mcmc_ref.py), the C surface
of libegs_mcmc.so against include/egs_mcmc.h and ``_mcmclib.SIGNATURES``, its refusals before any HIP call, and the
untouched ABI of libegs_hip.so."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import mcmc_ref as R

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "egs_mcmc.h")
BAD_ARG = 10001
_FAKE = C.c_void_p(4096)        # a pointer nobody dereferences: every call below is refused before any HIP call


@pytest.fixture(scope="module")
def lib():
    from easygaussiansplatting_amd import _lib, _mcmclib
    if not os.path.exists(_mcmclib.LIB_PATH):
        _lib.build()
    return _mcmclib.load()


def declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(egs_mcmc_[a-z0-9_]+)\s*\(", src)))


# ------------------------------------------------------------------------------------------- the reference's invariants
def test_one_copy_is_unchanged():
    o = np.array([0.004, 0.3, 0.9, 0.999])
    s = np.abs(R.S.normal(3, 1, (4, 3))) + 0.1
    o1, s1 = R.corrected(o, s, np.ones(4, int), 0.001)
    np.testing.assert_allclose(o1, o, rtol=1e-12)
    np.testing.assert_allclose(s1, s, rtol=1e-12)


def test_opacity_decreases_with_the_number_of_copies_and_scale_shrinks():
    o = np.array([0.01, 0.3, 0.9, 0.9999])
    s = np.ones((4, 3))
    prev_o, prev_s = o, s
    for N in (2, 3, 5, 20, 51):
        on, sn = R.corrected(o, s, np.full(4, N), 0.0)
        assert (on < prev_o).all() and (sn < prev_s).all() and (sn > 0).all(), N
        # N copies of opacity o' composite to the source's opacity
        np.testing.assert_allclose(1 - (1 - on) ** N, o, rtol=1e-12)
        prev_o, prev_s = on, sn
    # the correction stops at N_MAX copies
    a, b = R.corrected(o, s, np.full(4, 51), 0.0), R.corrected(o, s, np.full(4, 400), 0.0)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])


def test_the_sampler_never_returns_a_row_of_weight_zero():
    n = 5000
    w = (R.S.uniform01(11, 1, (n,)) * 1024).astype(np.int64).astype(np.float32) / 1024
    w[R.S.uniform01(11, 2, (n,)) < 0.6] = 0
    w[:40] = 0
    w[-40:] = 0
    idx = R.sample(w, 20000, seed=5, rnd=3)
    assert idx.min() >= 40 and idx.max() < n - 40 and (w[idx] > 0).all()
    # and follows the weights: the heaviest tenth of the rows gets its share of the draws
    heavy = w >= np.quantile(w[w > 0], 0.9)
    share = w[heavy].sum() / w.sum()
    assert abs(heavy[idx].mean() - share) < 0.02


def test_weights_and_dead_flags():
    a = np.array([-8.0, -5.0, 0.0, 3.0], np.float32)
    w, dead, (nd, nl) = R.weights(a, 0.005, True)
    assert dead.tolist() == [True, False, False, False] and (nd, nl) == (1, 3) and w[0] == 0 and w[1] > 0.005
    w2, _, _ = R.weights(a, 0.005, False)
    assert w2[0] > 0 and np.array_equal(w2[1:], w[1:])


def test_random_streams_do_not_collide():
    """densify round r reads the uniform streams 1000 + 2 r, 1001 + 2 r; the noise of step t 2 (2^40 + t) + 1000 / 1001;
    sampling round r 2^62 + r (include/egs_mcmc.h)"""
    from easygaussiansplatting_amd import _mcmclib
    assert (_mcmclib.STREAM_SAMPLE, _mcmclib.STREAM_NOISE) == (R.STREAM_SAMPLE, R.STREAM_NOISE) == (1 << 62, 1 << 40)
    hdr = open(HEADER).read()
    assert re.search(r"^#define\s+EGS_MCMC_STREAM_SAMPLE\s+\(1ull << 62\)\s*$", hdr, re.M)
    assert re.search(r"^#define\s+EGS_MCMC_STREAM_NOISE\s+\(1ull << 40\)\s*$", hdr, re.M)
    densify_hi = 1001 + 2 * (1 << 39)
    noise_lo, noise_hi = 2 * R.STREAM_NOISE + 1000, 2 * (R.STREAM_NOISE + (1 << 59)) + 1001
    assert densify_hi < noise_lo and noise_hi < R.STREAM_SAMPLE


# -------------------------------------------------------------------------------------------------------- the C surface
def test_library_exports_what_the_header_declares(lib):
    from easygaussiansplatting_amd import _mcmclib
    names = declared_functions()
    assert len(names) == 9 and "egs_mcmc_relocate" in names
    out = subprocess.run(["nm", "-D", "--defined-only", _mcmclib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip() and ln.split()[-1].startswith("egs_")}
    assert exported == set(names)
    assert set(_mcmclib.SIGNATURES) == set(names)
    assert re.search(r"^#define\s+EGS_MCMC_ABI_VERSION\s+1\s*$", open(HEADER).read(), re.M)
    assert lib.egs_mcmc_abi_version() == _mcmclib.ABI_VERSION == 1


def test_libegs_hip_is_untouched(lib):
    from easygaussiansplatting_amd import _lib
    main = _lib.load()
    assert main.egs_abi_version() == _lib.ABI_VERSION == 12
    assert not [k for k in _lib.SIGNATURES if "mcmc" in k]
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert "egs_mcmc" not in out


def _params(ptr=_FAKE, **over):
    from easygaussiansplatting_amd import _lib
    p = _lib.EgsGaussianParams(*[ptr.value if ptr is not None else None] * 6)
    for k, v in over.items():
        setattr(p, k, v)
    return p


def test_every_call_refuses_bad_arguments_before_the_device(lib):
    err = lib.egs_mcmc_last_error_string
    F, N = _FAKE, None
    ws = C.c_void_p(4096)
    # weights
    assert lib.egs_mcmc_weights(-1, F, 0.005, 1, F, F, F, N) == BAD_ARG and b"n >= 0" in err()
    for bad in ((N, F, F, F), (F, N, F, F), (F, F, N, F), (F, F, F, N)):
        assert lib.egs_mcmc_weights(10, bad[0], 0.005, 1, bad[1], bad[2], bad[3], N) == BAD_ARG
    assert lib.egs_mcmc_weights(10, F, 1.5, 1, F, F, F, N) == BAD_ARG
    # sample
    big = 1 << 30
    assert lib.egs_mcmc_sample(-1, F, 1, 5, 0, 0, F, ws, big, N) == BAD_ARG
    assert lib.egs_mcmc_sample(10, F, 1, -5, 0, 0, F, ws, big, N) == BAD_ARG
    assert lib.egs_mcmc_sample(10, N, 1, 5, 0, 0, F, ws, big, N) == BAD_ARG
    assert lib.egs_mcmc_sample(10, F, 1, 5, 0, 0, N, ws, big, N) == BAD_ARG
    assert lib.egs_mcmc_sample(10, F, 1, 5, 0, 0, F, N, big, N) == BAD_ARG
    assert lib.egs_mcmc_sample(10, F, 1, 5, 0, 0, F, ws, 8, N) == BAD_ARG and b"ws_bytes" in err()
    assert lib.egs_mcmc_sample(10, F, 0, 5, 0, 0, F, ws, big, N) == BAD_ARG and b"n_positive" in err()   # total == 0
    assert lib.egs_mcmc_sample(0, F, 0, 5, 0, 0, F, ws, big, N) == BAD_ARG
    assert lib.egs_mcmc_sample_ws_bytes(300001) >= 8 * 300001 + 8 * 294
    # relocate
    p = _params()
    reloc = lambda n=10, d=5, hw=45, src=F, dst=F, par=C.byref(p), m=None, v=None, mo=0.005, w=ws, wb=big: \
        lib.egs_mcmc_relocate(n, d, hw, src, dst, par, m, v, mo, w, wb, N)
    assert reloc(n=-1) == BAD_ARG and reloc(d=-1) == BAD_ARG and reloc(hw=-1) == BAD_ARG
    assert reloc(src=N) == BAD_ARG and reloc(dst=N) == BAD_ARG and reloc(par=N) == BAD_ARG and reloc(w=N) == BAD_ARG
    assert reloc(wb=8) == BAD_ARG and b"ws_bytes" in err()
    assert reloc(m=C.byref(p)) == BAD_ARG                       # one moment set without the other
    assert reloc(v=C.byref(p)) == BAD_ARG
    for k in ("pws", "low_shs", "high_shs", "alphas_raw", "scales_raw", "rots_raw"):
        q = _params(**{k: None})
        assert reloc(par=C.byref(q)) == BAD_ARG, k
        assert reloc(m=C.byref(q), v=C.byref(p)) == BAD_ARG, k
        assert reloc(m=C.byref(p), v=C.byref(q)) == BAD_ARG, k
    # regulariser
    reg = lambda n=10, a=F, s=F, ga=F, gs=F: lib.egs_mcmc_add_reg_grad(n, a, s, 0.01, 0.01, ga, gs, N)
    assert reg(n=-1) == BAD_ARG
    assert reg(a=N) == BAD_ARG and reg(s=N) == BAD_ARG and reg(ga=N) == BAD_ARG and reg(gs=N) == BAD_ARG
    # noise
    noise = lambda n=10, pw=F, a=F, s=F, r=F: lib.egs_mcmc_add_noise(n, pw, a, s, r, N, 5e5, 1e-4, 0, 0, N)
    assert noise(n=-1) == BAD_ARG
    assert noise(pw=N) == BAD_ARG and noise(a=N) == BAD_ARG and noise(s=N) == BAD_ARG and noise(r=N) == BAD_ARG
    assert noise(r=C.c_void_p(4096 + 4)) == BAD_ARG
    # empty calls are no error and touch nothing
    assert lib.egs_mcmc_sample(10, F, 1, 0, 0, 0, F, ws, big, N) == 0
    assert reloc(d=0) == 0 and reg(n=0) == 0 and noise(n=0) == 0


def test_python_surface_refuses_without_a_device():
    from easygaussiansplatting_amd.density import MCMCControl
    import inspect
    sig = inspect.signature(MCMCControl.__init__)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[2:]] == \
        [("seed", 0), ("min_opacity", 0.005), ("noise_lr", 5e5), ("opacity_reg", 0.01), ("scale_reg", 0.01),
         ("growth", 1.05)]
    with pytest.raises(ValueError):
        MCMCControl(None)
    ctl = MCMCControl(100, seed=3)
    assert (ctl.cap_max, ctl.seed, ctl.round, ctl.step) == (100, 3, 0, 0)
    for m in ("add_regularisers", "inject_noise", "relocate", "grow"):
        assert callable(getattr(ctl, m))
    from easygaussiansplatting_amd import trainer
    sig = inspect.signature(trainer.Trainer.__init__)
    assert sig.parameters["strategy"].default == "default" and sig.parameters["cap_max"].default is None
    with pytest.raises(ValueError, match="cap_max"):
        trainer.Trainer(None, [], [], 10, strategy="mcmc")
    with pytest.raises(ValueError, match="strategy"):
        trainer.Trainer(None, [], [], 10, strategy="adaptive")
