"""Visibility-masked Adam, host side (no GPU): the float32 reference's own checks (tests/sparse_adam_ref.py), the C
surface of libegs_adam.so against include/egs_adam.h and ``_adamlib.SIGNATURES``, its refusals before any HIP call, the
untouched surface of libegs_hip.so, the dense ``egs_adam_step``'s refusal of misaligned pointers (with ``FusedAdam.step``
rolling its counters back), and the refusals of ``FusedAdam.step(visible=...)`` and ``Trainer(sparse_adam=True)`` that
need no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import sparse_adam_ref as R

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "egs_adam.h")
BAD_ARG = 10001
_FAKE = 4096                    # a pointer nobody dereferences: every call below is refused before any HIP call


@pytest.fixture(scope="module")
def lib():
    from easygaussiansplatting_amd import _adamlib, _lib
    if not os.path.exists(_adamlib.LIB_PATH):
        _lib.build()
    return _adamlib.load()


# -------------------------------------------------------------------------------------------------- the reference itself
def _tensors(n, seed):
    rng = np.random.RandomState(seed)
    return [rng.randn(n, w).astype(np.float32) for w in R.WIDTHS]


def _grads(rng, n):
    """gradient scales spread over 1e-6 .. 1, one scale per tensor and step"""
    return [(rng.randn(n, w) * 10.0 ** rng.randint(-6, 1)).astype(np.float32) for w in R.WIDTHS]


def test_reference_with_every_row_visible_is_torch_adam():
    n = 37
    init = _tensors(n, 5)
    tp = [torch.from_numpy(x.copy()).requires_grad_() for x in init]
    opt = torch.optim.Adam([{"params": [p], "lr": lr} for p, lr in zip(tp, R.LRS)], lr=0.0, eps=1e-15)
    p = [x.copy() for x in init]
    m = [np.zeros_like(x) for x in init]
    v = [np.zeros_like(x) for x in init]
    rng = np.random.RandomState(6)
    vis = np.ones(n, dtype=bool)
    for step in range(1, 6):
        gs = _grads(rng, n)
        for k, g in enumerate(gs):
            tp[k].grad = torch.from_numpy(g.copy())
            p[k], m[k], v[k] = R.masked_adam_step(p[k], g, m[k], v[k], step, R.LRS[k], vis)
        opt.step()
    for k in range(len(init)):
        np.testing.assert_allclose(p[k], tp[k].detach().numpy(), rtol=2e-5, atol=1e-6)
        assert np.abs(p[k] - init[k]).max() > 0


def test_reference_keeps_invisible_rows_bit_for_bit():
    n = 130
    rng = np.random.RandomState(7)
    for name, vis in R.mask_shapes(n).items():
        for k, w in enumerate(R.WIDTHS):
            p, m = rng.randn(n, w).astype(np.float32), (rng.randn(n, w) * 1e-3).astype(np.float32)
            v = (rng.rand(n, w) * 1e-6).astype(np.float32)
            g = (rng.randn(n, w) * 1e-2).astype(np.float32)
            dense = R.masked_adam_step(p, g, m, v, 3, R.LRS[k], np.ones(n, dtype=bool))
            g[~vis] = np.nan
            got = R.masked_adam_step(p, g, m, v, 3, R.LRS[k], vis.astype(np.uint8))
            for before, after, full in zip((p, m, v), got, dense):
                assert np.array_equal(after[~vis].view(np.int32), before[~vis].view(np.int32)), (name, k)
                assert np.array_equal(after[vis].view(np.int32), full[vis].view(np.int32)), (name, k)
                assert np.isfinite(after).all()
            assert vis.sum() == 0 or not np.array_equal(got[0][vis], p[vis])


# -------------------------------------------------------------------------------------------------------- the C surface
def declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(egs_[a-z0-9_]+)\s*\(", src)))


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip() and ln.split()[-1].startswith("egs_")}


def test_library_exports_what_the_header_declares(lib):
    from easygaussiansplatting_amd import _adamlib
    names = declared_functions()
    assert names == ["egs_adam_abi_version", "egs_adam_last_error_string", "egs_sparse_adam_sh_factored",
                     "egs_sparse_adam_step"]
    assert _exports(_adamlib.LIB_PATH) == set(names)
    assert set(_adamlib.SIGNATURES) == set(names)
    hdr = open(HEADER).read()
    assert re.search(r"^#define\s+EGS_ADAM_ABI_VERSION\s+%d\s*$" % _adamlib.ABI_VERSION, hdr, re.M)
    assert lib.egs_adam_abi_version() == _adamlib.ABI_VERSION
    assert re.search(r"^#define\s+EGS_SPARSE_ADAM_MAX_GROUPS\s+%d\s*$" % _adamlib.MAX_GROUPS, hdr, re.M)
    assert _adamlib.MAX_GROUPS == 8 and _adamlib.ERR_BAD_ARG == BAD_ARG
    # the mirror of the group record: 4 pointers, width, lr, step
    assert C.sizeof(_adamlib.EgsSparseAdamGroup) == 48
    body = hdr[hdr.index("typedef struct EgsSparseAdamGroup"):hdr.index("} EgsSparseAdamGroup;")]
    assert [f[0] for f in _adamlib.EgsSparseAdamGroup._fields_] == re.findall(
        r"^\s+(?:const )?(?:float\*|int32_t|float) (\w+);", body, re.M)


def test_libegs_hip_is_untouched(lib):
    from easygaussiansplatting_amd import _lib
    main = _lib.load()
    assert main.egs_abi_version() == _lib.ABI_VERSION == 12
    assert not [k for k in _lib.SIGNATURES if "sparse" in k]
    exported = _exports(_lib.LIB_PATH)
    assert len(exported) == 64 and not [s for s in exported if "sparse" in s]
    assert "egs_adam_step" in exported and "egs_adam_sh_factored" in exported      # the dense step stays where it is


def _group(param=_FAKE, grad=_FAKE, m=_FAKE, v=_FAKE, width=3, lr=1e-3, step=1):
    from easygaussiansplatting_amd._adamlib import EgsSparseAdamGroup
    return EgsSparseAdamGroup(param, grad, m, v, width, lr, step)


def test_sparse_adam_step_refuses_bad_arguments_before_the_device(lib):
    from easygaussiansplatting_amd._adamlib import EgsSparseAdamGroup
    err = lib.egs_adam_last_error_string

    def call(groups, n=100, visible=_FAKE, n_groups=None):
        arr = (EgsSparseAdamGroup * max(len(groups), 1))(*groups)
        return lib.egs_sparse_adam_step(len(groups) if n_groups is None else n_groups, arr, n, visible, 0.9, 0.999,
                                        1e-15, None)

    def refused(rc):
        return rc == BAD_ARG and err().startswith(b"egs_adam error 10001: bad argument") and len(err()) > 40
    for field in ("param", "grad", "m", "v"):
        assert refused(call([_group(), _group(**{field: None})])), field                 # a null pointer
        assert refused(call([_group(**{field: _FAKE + 4})])), field                      # not 16-byte aligned
        assert refused(call([_group(**{field: _FAKE + 8})])), field
    assert refused(call([_group()], visible=None)) and b"visible" in err()
    assert refused(lib.egs_sparse_adam_step(1, None, 100, _FAKE, 0.9, 0.999, 1e-15, None)) and b"groups" in err()
    assert refused(call([_group(width=0)])) and b"width > 0" in err()
    assert refused(call([_group(width=-3)])) and b"width > 0" in err()
    assert refused(call([_group(step=0)])) and b"step >= 1" in err()
    assert refused(call([_group(step=-1)]))
    assert refused(call([_group()], n=-1)) and b"n >= 0" in err()
    assert refused(call([_group(width=4)], n=1 << 29))                                  # n * width == 2^31
    assert refused(call([_group(width=45)], n=47721859))                                # 45 n just above 2^31
    assert refused(call([_group()] * 9)) and b"n_groups" in err()                       # more than 8 groups
    assert refused(call([_group()], n_groups=-1))
    # nothing to do is no error and launches nothing -- but what can be checked still is
    assert call([_group()], n=0) == 0
    assert call([_group(None, None, None, None)], n=0, visible=None) == 0               # empty tensors have no storage
    assert call([], n=100) == 0
    assert lib.egs_sparse_adam_step(0, None, 100, None, 0.9, 0.999, 1e-15, None) == 0
    assert refused(call([_group(width=0)], n=0)) and refused(call([_group(step=0)], n=0))


def test_sparse_adam_sh_factored_refuses_bad_arguments_before_the_device(lib):
    from easygaussiansplatting_amd._lib import EgsAdamGroup
    err = lib.egs_adam_last_error_string
    n = 100

    def grp(width, param=_FAKE, m=_FAKE, v=_FAKE, step=1, count=None):
        return EgsAdamGroup(param, None, m, v, n * width if count is None else count, 1e-3, step)

    def call(n=n, K=48, views=1, pws=_FAKE, rows=_FAKE, stride=3 * n + 3, low=grp(3), high=grp(45), visible=_FAKE):
        return lib.egs_sparse_adam_sh_factored(n, K, views, pws, rows, stride, 1.0, C.byref(low) if low else None,
                                               C.byref(high) if high else None, visible, 0.9, 0.999, 1e-15, None)

    def refused(rc):
        return rc == BAD_ARG and err().startswith(b"egs_adam error 10001: bad argument") and len(err()) > 40
    assert refused(call(n=-1)) and refused(call(views=-1)) and refused(call(low=None))
    for K in (0, 5, 9, 45, 49):
        assert refused(call(K=K)) and b"sh_dim" in err(), K
    assert refused(call(pws=None)) and b"pws" in err()
    assert refused(call(rows=None)) and refused(call(stride=3 * n + 2))
    assert refused(call(visible=None)) and b"visible" in err()
    for bad in (dict(param=None), dict(m=None), dict(v=None), dict(step=0), dict(count=n * 3 + 1),
                dict(param=_FAKE + 4), dict(m=_FAKE + 8), dict(v=_FAKE + 4)):
        assert refused(call(low=grp(3, **bad))), bad
        hb = dict(bad, count=n * 45 + 1) if "count" in bad else bad
        assert refused(call(high=grp(45, **hb))), bad
    assert refused(call(low=grp(3), high=None))                    # whole-tensor form: low must be [n][48]
    assert refused(call(K=12, low=grp(3), high=grp(45)))           # raw form at K = 12: high must be [n][9]
    # nothing to do is no error -- but sizes are still checked
    assert call(n=0, pws=None, rows=None, visible=None) == 0
    assert refused(call(n=0, K=7)) and refused(call(n=0, low=None))


def test_dense_adam_step_refuses_misaligned_pointers_before_the_device(lib):
    """``egs_adam_step`` (libegs_hip.so) moves float4s like the masked step and refuses what the masked step refuses: each
    of the four pointers null or off a 16-byte boundary, before any HIP call.  A zero-count group is skipped, whatever it
    points to."""
    from easygaussiansplatting_amd import _lib
    main = _lib.load()
    err = main.egs_last_error_string

    def grp(param=_FAKE, grad=_FAKE, m=_FAKE, v=_FAKE, count=300, step=1):
        return _lib.EgsAdamGroup(param, grad, m, v, count, 1e-3, step)

    def call(groups):
        return main.egs_adam_step(len(groups), (_lib.EgsAdamGroup * max(len(groups), 1))(*groups), 0.9, 0.999, 1e-15, None)

    def refused(rc):
        return rc == BAD_ARG and b"bad argument" in err() and b"egs_density" in err()
    for field in ("param", "grad", "m", "v"):
        for off in (4, 8, 12):
            assert refused(call([grp(**{field: _FAKE + off})])) and b"adam_aligned16" in err(), (field, off)
            assert refused(call([grp(count=0), grp(**{field: _FAKE + off})])), (field, off)       # behind a skipped group
        assert refused(call([grp(), grp(**{field: None})])), field
    assert refused(call([grp(step=0)])) and refused(call([grp(count=-1)])) and refused(call([grp()] * 9))
    assert call([]) == 0 and call([grp(count=0)]) == 0
    assert call([grp(_FAKE + 4, _FAKE + 8, None, _FAKE + 12, count=0)]) == 0


class _DeviceLike(torch.Tensor):
    """a host tensor that calls itself a device tensor: ``FusedAdam.step`` takes it as far as the C entry point, which
    must refuse it before anything is launched"""
    is_cuda = property(lambda self: True)


@pytest.mark.parametrize("which", ["param", "grad", "exp_avg", "exp_avg_sq"])
def test_fused_adam_step_with_a_misaligned_tensor_raises_and_rolls_every_counter_back(lib, monkeypatch, which):
    """``x[1:]`` of an [n, 3] tensor is contiguous float32 and starts 12 bytes into its storage: the dense step refuses it
    (RuntimeError from the library's argument check), no tensor moves, every step counter is where it was."""
    from easygaussiansplatting_amd.optim import FusedAdam

    class _Stream:
        cuda_stream = 0
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a, **k: _Stream())
    n = 8
    like = lambda t: torch.Tensor._make_subclass(_DeviceLike, t)
    sliced = lambda value=0.5: torch.full((n + 1, 3), value)[1:]
    ps = [like(torch.full((n, 3), 0.5)).requires_grad_() for _ in range(3)]
    if which == "param":
        ps[1] = like(sliced()).requires_grad_()
    assert all(p.is_contiguous() and p.is_cuda for p in ps)
    for p in ps:
        p.grad = torch.ones(n, 3)
    if which == "grad":
        ps[1].grad = sliced()
    opt = FusedAdam([{"params": [p], "lr": 1e-3} for p in ps])
    for k, p in enumerate(ps):
        opt.state[p] = {"step": 3 + k, "exp_avg": torch.zeros(n, 3), "exp_avg_sq": torch.zeros(n, 3)}
    if which in ("exp_avg", "exp_avg_sq"):
        opt.state[ps[1]][which] = sliced(0.0)
    ptrs = dict(param=ps[1], grad=ps[1].grad, exp_avg=opt.state[ps[1]]["exp_avg"], exp_avg_sq=opt.state[ps[1]]["exp_avg_sq"])
    assert ptrs[which].data_ptr() % 16 == 12 and all(t.data_ptr() % 16 == 0 for k, t in ptrs.items() if k != which)
    with pytest.raises(RuntimeError, match="bad argument.*adam_aligned16"):
        opt.step()
    for k, p in enumerate(ps):
        st = opt.state[p]
        assert st["step"] == 3 + k and not st["exp_avg"].any() and not st["exp_avg_sq"].any(), k
        assert bool((p.detach() == 0.5).all())


def test_missing_library_raises(monkeypatch, tmp_path):
    from easygaussiansplatting_amd import _adamlib, _lib
    from easygaussiansplatting_amd.optim import FusedAdam
    monkeypatch.setattr(_adamlib, "_lib", None)
    monkeypatch.setattr(_adamlib, "LIB_PATH", str(tmp_path / "libegs_adam.so"))
    with pytest.raises(_lib.EgsLibraryError):
        _adamlib.load()
    # and the optimizer does not fall back to the dense step (or to anything else): it raises, the state stays
    p = torch.zeros(4, 3, requires_grad=True)
    p.grad = torch.ones(4, 3)
    opt = FusedAdam([{"params": [p], "lr": 1e-3}])
    opt.state[p] = {"step": 3, "exp_avg": torch.zeros(4, 3), "exp_avg_sq": torch.zeros(4, 3)}
    with pytest.raises(_lib.EgsLibraryError):
        opt.step(visible=torch.ones(4, dtype=torch.bool))
    assert opt.state[p]["step"] == 3 and not p.detach().any()


# --------------------------------------------------------------------------------------------------- Python, no device
def _cpu_optimizer(n=6):
    from easygaussiansplatting_amd.optim import FusedAdam
    ps = [torch.full((n, w), 0.5, requires_grad=True) for w in R.WIDTHS]
    for p in ps:
        p.grad = torch.ones_like(p)
    opt = FusedAdam([{"params": [p], "lr": lr} for p, lr in zip(ps, R.LRS)], eps=1e-15)
    for k, p in enumerate(ps):
        opt.state[p] = {"step": 3 + k, "exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.zeros_like(p)}
    return ps, opt


@pytest.mark.parametrize("what,mask,msg", [
    ("dtype float", lambda n: torch.ones(n), "bool or uint8"),
    ("dtype int32", lambda n: torch.ones(n, dtype=torch.int32), "bool or uint8"),
    ("not a tensor", lambda n: [True] * n, "bool or uint8"),
    ("too short", lambda n: torch.ones(n - 1, dtype=torch.bool), "rows"),
    ("too long", lambda n: torch.ones(n + 1, dtype=torch.uint8), "rows"),
    ("two-dimensional", lambda n: torch.ones(n, 1, dtype=torch.bool), "contiguous 1-D"),
    ("not contiguous", lambda n: torch.ones(2 * n, dtype=torch.bool)[::2], "contiguous 1-D"),
    ("another device", lambda n: torch.ones(n, dtype=torch.bool, device="meta"), "the mask is on"),
])
def test_fused_adam_refuses_a_bad_mask_and_leaves_the_state(lib, what, mask, msg):
    ps, opt = _cpu_optimizer()
    with pytest.raises(ValueError, match=msg):
        opt.step(visible=mask(ps[0].shape[0]))
    for k, p in enumerate(ps):
        st = opt.state[p]
        assert st["step"] == 3 + k and not st["exp_avg"].any() and not st["exp_avg_sq"].any(), what
        assert bool((p.detach() == 0.5).all())


def test_trainer_refuses_sparse_adam_without_fused_adam_and_with_mcmc():
    from easygaussiansplatting_amd.trainer import Trainer
    with pytest.raises(ValueError, match="sparse_adam=True.*fused_adam"):
        Trainer(None, [], [], max_steps=10, device="cpu", sparse_adam=True, fused_adam=False)
    with pytest.raises(ValueError, match="sparse_adam=True.*mcmc"):
        Trainer(None, [], [], max_steps=10, device="cpu", sparse_adam=True, strategy="mcmc", cap_max=1000)
    import inspect
    assert inspect.signature(Trainer.__init__).parameters["sparse_adam"].default is False
