"""Blend-weight statistics and importance pruning, host side (no GPU): the float64 reference's own invariants
(tests/blend_weights_ref.py), the C surface of libegs_prune.so against include/egs_prune.h and ``_prunelib.SIGNATURES``,
its refusals before any HIP call, the untouched surfaces of the other two libraries, ``keep_mask``, ``BlendStats.merge_``
and ``allreduce_`` over gloo."""
import ctypes as C
import os
import re
import socket
import subprocess

import numpy as np
import pytest

from tests import blend_weights_ref as B
from tests import draw_tile_ref as D

torch = pytest.importorskip("torch")
import torch.distributed as dist            # noqa: E402
import torch.multiprocessing as mp          # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "egs_prune.h")
BAD_ARG = 10001
_FAKE = C.c_void_p(4096)        # a pointer nobody dereferences: every call below is refused before any HIP call
CASES = [(n, p) for n in D.SETS for p in D.POLICIES]


@pytest.fixture(scope="module")
def lib():
    from easygaussiansplatting_amd import _lib, _prunelib
    if not os.path.exists(_prunelib.LIB_PATH):
        _lib.build()
    return _prunelib.load()


# -------------------------------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("name,pname", CASES)
def test_reference_identity_hits_and_final_tau(name, pname):
    c = D.case(name)
    ref, dref = B.reference(name, pname), D.reference(name, pname)
    # sum_g sum[g] = sum_p (1 - final_tau[p]) over the non-empty tiles
    lhs, rhs = ref["sum"].sum(), 0.0
    for t, l in enumerate(D.lists(c, pname)[0]):
        if len(l):
            tx, ty, x0, y0, ww, hh = D.geom(t)
            rhs += (1.0 - dref["final_tau"][y0:y0 + hh, x0:x0 + ww]).sum()
    assert rhs > 0 and abs(lhs - rhs) <= 1e-12 * rhs, (lhs, rhs)
    # the hits are the blend's own, the transmittance left over is the oracle's bit for bit
    assert np.array_equal(ref["hits"], dref["diag"]["hits"])
    assert ref["final_tau"].dtype == np.float64 and np.array_equal(ref["final_tau"], dref["final_tau"])
    assert (ref["max"] <= ref["sum"]).all() and ((ref["hits"] == 0) == (ref["sum"] == 0)).all()
    assert (ref["max"] >= 0).all() and (ref["max"] <= 1).all()


# -------------------------------------------------------------------------------------------------------- the C surface
def declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(egs_[a-z0-9_]+)\s*\(", src)))


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip() and ln.split()[-1].startswith("egs_")}


def test_library_exports_what_the_header_declares(lib):
    from easygaussiansplatting_amd import _prunelib
    names = declared_functions()
    assert names == ["egs_blend_weights", "egs_prune_abi_version", "egs_prune_last_error_string"]
    assert _exports(_prunelib.LIB_PATH) == set(names)
    assert set(_prunelib.SIGNATURES) == set(names)
    assert re.search(r"^#define\s+EGS_PRUNE_ABI_VERSION\s+1\s*$", open(HEADER).read(), re.M)
    assert lib.egs_prune_abi_version() == _prunelib.ABI_VERSION == 1
    assert _prunelib.DRAW_MASKED_LISTS == 2
    assert re.search(r"^#define\s+EGS_DRAW_MASKED_LISTS\s+2\s*$", open(os.path.join(REPO, "include", "egs_hip.h")).read(),
                     re.M)


def test_the_other_two_libraries_are_untouched(lib):
    from easygaussiansplatting_amd import _lib, _mcmclib
    main = _lib.load()
    assert main.egs_abi_version() == _lib.ABI_VERSION == 12
    assert not [k for k in _lib.SIGNATURES if "egs_blend" in k or "egs_prune" in k]
    assert not [s for s in _exports(_lib.LIB_PATH) if s.startswith("egs_blend") or s.startswith("egs_prune")]
    mc = _exports(_mcmclib.LIB_PATH)
    assert len(mc) == 9 and mc == set(_mcmclib.SIGNATURES)
    assert _mcmclib.load().egs_mcmc_abi_version() == 1


def test_bad_arguments_are_refused_before_the_device(lib):
    from easygaussiansplatting_amd._lib import EgsPolicy
    err = lib.egs_prune_last_error_string
    F, N = _FAKE, None
    pol = EgsPolicy()
    pol.alpha_skip, pol.tau_stop, pol.maha_floor, pol.alpha_clamp = 0.002, 1e-4, 1, 1
    call = lambda n=10, w=64, h=48, rec=F, p=C.byref(pol), ranges=F, gsid=F, contrib=F, flags=0, stats=F: \
        lib.egs_blend_weights(n, w, h, rec, p, ranges, gsid, contrib, flags, stats, N)
    assert call(n=-1) == BAD_ARG and b"n >= 0" in err()
    assert call(w=0) == BAD_ARG and b"width > 0" in err()
    assert call(h=-3) == BAD_ARG and b"height > 0" in err()
    assert call(rec=N) == BAD_ARG and b"rec" in err()
    assert call(rec=C.c_void_p(4096 + 4)) == BAD_ARG and b"rec" in err()
    assert call(p=N) == BAD_ARG and b"pol" in err()
    assert call(ranges=N) == BAD_ARG and b"ranges" in err()
    assert call(gsid=N) == BAD_ARG and b"gsid" in err()
    assert call(contrib=N) == BAD_ARG and b"contrib" in err()
    assert call(stats=N) == BAD_ARG and b"stats" in err()
    assert call(stats=C.c_void_p(4096 + 8)) == BAD_ARG and b"stats" in err()
    for flags in (1, 4, 8, 2 | 16, -1):
        assert call(flags=flags) == BAD_ARG and b"flags" in err(), flags
    assert call(n=1 << 28, flags=2) == BAD_ARG                  # a masked list value holds 28 index bits
    # an empty call is no error and touches nothing -- but its sizes and flags are still checked
    assert call(n=0, rec=N, ranges=N, gsid=N, contrib=N, stats=N) == 0
    assert call(n=0, w=0) == BAD_ARG and call(n=0, flags=4) == BAD_ARG and call(n=0, p=N) == BAD_ARG


def test_missing_library_raises(monkeypatch, tmp_path):
    from easygaussiansplatting_amd import _lib, _prunelib
    monkeypatch.setattr(_prunelib, "_lib", None)
    monkeypatch.setattr(_prunelib, "LIB_PATH", str(tmp_path / "libegs_prune.so"))
    with pytest.raises(_lib.EgsLibraryError):
        _prunelib.load()


# ------------------------------------------------------------------------------------------------------------ keep_mask
def _stats(sums, maxs, hits):
    from easygaussiansplatting_amd.importance import BlendStats
    st = BlendStats(len(sums), "cpu")
    st.sum.copy_(torch.tensor(sums, dtype=torch.float32))
    st.max.copy_(torch.tensor(maxs, dtype=torch.float32))
    st.hits.copy_(torch.tensor(hits, dtype=torch.int32))
    return st


def test_blendstats_layout():
    st = _stats([1.5, 0.0, 2.0], [0.5, 0.0, 0.25], [7, 0, 300])
    assert st.rows.dtype == torch.float32 and tuple(st.rows.shape) == (3, 4) and st.n == 3
    assert st.rows[:, 0].tolist() == [1.5, 0.0, 2.0] and st.rows[:, 1].tolist() == [0.5, 0.0, 0.25]
    assert st.rows.view(torch.int32)[:, 2].tolist() == [7, 0, 300] and st.hits.dtype == torch.int32
    assert not st.rows[:, 3].any() and not st.rows[1].any()
    st.views = 3
    st.zero_()
    assert not st.rows.view(torch.int32).any() and st.views == 0


def test_keep_mask_threshold_and_fraction():
    from easygaussiansplatting_amd.importance import keep_mask
    st = _stats([3.0, 0.0, 1.0, 1.0, 0.5, 1.0, 9.0, 0.0],
                [0.5, 0.0, 0.125, 0.25, 0.0625, 0.125, 1.0, 0.0],
                [30, 0, 1, 4, 2, 1, 90, 0])
    assert keep_mask(st, "max", threshold=0.125).tolist() == [True, False, True, True, False, True, True, False]
    assert keep_mask(st, "hits", threshold=1).tolist() == [True, False, True, True, True, True, True, False]
    assert keep_mask(st, "sum", threshold=1.0).tolist() == [True, False, True, True, False, True, True, False]
    # fraction: floor(fraction N) rows go, lowest score first; ties by index, the lower index first
    assert keep_mask(st, "sum", fraction=0.0).all()
    assert keep_mask(st, "sum", fraction=0.125).tolist() == [True, False, True, True, True, True, True, True]
    assert keep_mask(st, "sum", fraction=0.25).tolist() == [True, False, True, True, True, True, True, False]
    assert keep_mask(st, "sum", fraction=0.5).tolist() == [True, False, False, True, False, True, True, False]
    assert keep_mask(st, "sum", fraction=0.625).tolist() == [True, False, False, False, False, True, True, False]
    assert keep_mask(st, "sum", fraction=0.3).tolist() == keep_mask(st, "sum", fraction=0.25).tolist()   # floor(2.4)
    assert keep_mask(st, "hits", fraction=0.5).tolist() == [True, False, False, True, True, False, True, False]
    assert not keep_mask(st, "max", fraction=1.0).any()
    k = keep_mask(st, "max", fraction=0.25)
    assert k.dtype == torch.bool and tuple(k.shape) == (8,)
    assert keep_mask(st, "max", fraction=0.25).tolist() == k.tolist()


def test_keep_mask_refuses_what_it_cannot_mean():
    from easygaussiansplatting_amd.importance import keep_mask
    st = _stats([1.0, 2.0], [0.1, 0.2], [1, 2])
    with pytest.raises(ValueError):
        keep_mask(st, "max")
    with pytest.raises(ValueError):
        keep_mask(st, "max", threshold=0.1, fraction=0.5)
    with pytest.raises(ValueError):
        keep_mask(st, "mean", threshold=0.1)
    with pytest.raises(ValueError):
        keep_mask(st, "max", fraction=1.5)


def test_merge_adds_sums_and_hits_and_takes_the_max():
    a = _stats([1.0, 0.0, 2.5], [0.5, 0.0, 0.25], [10, 0, 1 << 24])
    b = _stats([0.25, 3.0, 0.5], [0.125, 0.75, 0.5], [3, 7, 1])
    a.views, b.views = 2, 1
    a.merge_(b)
    assert a.sum.tolist() == [1.25, 3.0, 3.0] and a.max.tolist() == [0.5, 0.75, 0.5]
    assert a.hits.tolist() == [13, 7, (1 << 24) + 1]           # integer addition, not float32
    assert not a.rows[:, 3].any() and a.views == 3
    assert b.sum.tolist() == [0.25, 3.0, 0.5]
    from easygaussiansplatting_amd.importance import BlendStats
    with pytest.raises(ValueError):
        a.merge_(BlendStats(4, "cpu"))


def test_allreduce_without_a_process_group_is_a_noop():
    a = _stats([1.0, 2.0], [0.1, 0.2], [1, 2])
    before = a.rows.clone()
    assert a.allreduce_() is a and torch.equal(a.rows, before)


def _rank_stats(rank):
    n = 257
    u = D.S.uniform01(31 + rank, 1, (3, n))
    hits = (u[2] * (1 << 25)).astype(np.int64)                 # beyond float32's integers
    hits[::5] = 0
    return _stats(np.where(hits > 0, u[0] * 40, 0).tolist(), np.where(hits > 0, u[1], 0).tolist(), hits.tolist())


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        st = _rank_stats(rank)
        st.views = rank + 1
        st.allreduce_()
        q.put((rank, st.rows.numpy().view(np.int32).copy(), st.views))
    finally:
        dist.destroy_process_group()


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def test_two_rank_allreduce_adds_sums_and_hits_and_takes_the_max():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=180) for _ in range(world)]
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    a, b = _rank_stats(0), _rank_stats(1)
    want = a.rows.clone()
    want[:, 0] = a.sum + b.sum
    want[:, 1] = torch.maximum(a.max, b.max)
    want.view(torch.int32)[:, 2] = a.hits + b.hits
    want = want.numpy().view(np.int32)
    assert np.array_equal(res[0][1], res[1][1])                 # bit-equal across the ranks
    for _, rows, views in res:
        assert np.array_equal(rows, want) and views == 3


# ---------------------------------------------------------------------------------------------------------------- prune
def test_prune_compacts_parameters_and_moments_in_order():
    from easygaussiansplatting_amd.density import DensityControl
    from easygaussiansplatting_amd.optim import NAMES
    n = 11
    widths = dict(zip(NAMES, (3, 3, 45, 1, 3, 4)))
    params = {k: torch.nn.Parameter(torch.from_numpy(D.S.normal(7, i, (n, w)).astype(np.float32)))
              for i, (k, w) in enumerate(widths.items())}
    opt = torch.optim.Adam([{"params": [p], "name": k, "lr": 1e-3} for k, p in params.items()], eps=1e-15)
    for p in params.values():
        p.grad = torch.ones_like(p) * p.detach()
    opt.step()
    old = {k: (p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone())
           for k, p in params.items()}
    ctl = DensityControl(1.0, 10)
    keep = torch.tensor([1, 0, 1, 1, 0, 0, 1, 0, 1, 1, 0], dtype=torch.bool)
    with pytest.raises(ValueError):
        ctl.prune(params, opt, torch.zeros(n, dtype=torch.bool))
    with pytest.raises(ValueError):
        ctl.prune(params, opt, keep[:-1])
    assert ctl.prune(params, opt, torch.ones(n, dtype=torch.bool)) == {"pruned": 0, "total": n}
    assert ctl.prune(params, opt, keep) == {"pruned": 5, "total": 6}
    groups = {g["name"]: g for g in opt.param_groups}
    assert len(opt.state) == 6
    for k in NAMES:
        p = params[k]
        assert groups[k]["params"][0] is p and p.requires_grad and p.is_leaf and p.shape[0] == 6
        st = opt.state[p]
        for a, b in zip(old[k], (p.detach(), st["exp_avg"], st["exp_avg_sq"])):
            assert torch.equal(a[keep], b) and b.is_contiguous()
        assert int(st["step"]) == 1
    for p in params.values():
        p.grad = torch.ones_like(p)
    opt.step()                                                     # the optimizer goes on with the compacted state
