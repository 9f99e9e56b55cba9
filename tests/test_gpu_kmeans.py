"""libegs_kmeans.so on the GPU, called through its C ABI on buffers between guard bands, against the numpy
float64 definitions of tests/kmeans_ref.py.  R = 256 rows per workgroup and T = 64 centroids per LDS tile of the assign
kernel; the shapes (``kmeans_ref.SHAPES``) take N from {1, R-1, R, R+1, 2R+3}, K from {1, 2, T-1, T, T+1, 2T+3} and D from
{1, 3, 9, 24, 45, 48, 64}.  Lattice cases: labels and distances exact, ties and duplicates to the lowest index.  Random cases:
every row's label within the derived gap bound of the float64 minimum.  Rows that are not finite: label 0, the others
unchanged.  Update: within one float32 ulp of the float64 means, counts and integer weight sums exact, empty and zero-weight
clusters keep their bits.  Every entry point: the same bits on grids of 1 and 3 workgroups, the default grid, a side stream and
twice in a row; inputs unmodified, guards intact; refused and empty calls write nothing.  Then the Python layer."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import kmeans_ref as KR
from tests import loss_abi as LA

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

R, T, CHUNK = KR.ROWS, KR.TILE, KR.CHUNK
BAD_ARG = 10001
GRIDS = (dict(), dict(max_blocks=1), dict(max_blocks=3), dict(side_stream=True), dict())


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from easygaussiansplatting_amd import _kmeanslib
    assert (_kmeanslib.ROWS, _kmeanslib.TILE, _kmeanslib.CHUNK) == (R, T, CHUNK)
    return _kmeanslib.load()


class Out:
    """an output buffer between two guard bands, filled with the guards' pattern (or with ``init``)"""

    def __init__(self, shape, dtype, init=None):
        self.dtype = getattr(torch, dtype)
        self.shape = tuple(shape)
        n = int(np.prod(self.shape)) * torch.empty((), dtype=self.dtype).element_size()
        self.whole, self.inner = LA.guarded(n)
        if init is not None:
            self.inner.copy_(torch.from_numpy(np.array(init, copy=True)).view(torch.uint8).reshape(-1).cuda())

    @property
    def ptr(self):
        return C.c_void_p(self.inner.data_ptr())

    def numpy(self):
        assert LA.guards_intact(self.whole), "a kernel wrote outside its buffer"
        return self.inner.view(self.dtype).reshape(self.shape).cpu().numpy().copy()

    def untouched(self):
        return LA.guards_intact(self.whole) and bool((self.inner == LA.PATTERN).all())


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def to_dev(a):
    return None if a is None else torch.from_numpy(np.array(a, copy=True)).cuda()


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def on_device(kind, shape):
    x, c = KR.lattice_case(*shape) if kind == "lattice" else KR.random_case(*shape, kind=kind)
    return to_dev(x), to_dev(c)


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

    def assign(self, x, c, dist=True):
        """-> (labels int32 [N], dist float32 [N] or None, cnorm float32 [K]); inputs checked unmodified"""
        N, D = x.shape
        K = c.shape[0]
        before = x.clone(), c.clone()
        lab, dst, cn = Out((N,), "int32"), Out((N,), "float32") if dist else None, Out((K,), "float32")
        assert self._run(self.lib.egs_kmeans_assign, N, D, K, ptr(x), ptr(c), cn.ptr, lab.ptr, dst.ptr if dist else None) == 0
        assert torch.equal(before[0].view(torch.int32), x.view(torch.int32)), "x was modified"
        assert torch.equal(before[1].view(torch.int32), c.view(torch.int32)), "the centroids were modified"
        return lab.numpy(), dst.numpy() if dist else None, cn.numpy()

    def update(self, x, labels, prev, weights=None):
        """-> (centroids float32 [K,D], wsum float64 [K], count int32 [K]); order and offsets by torch as ``compress`` does"""
        N, D = x.shape
        K = prev.shape[0]
        lab = to_dev(np.asarray(labels, np.int32))
        srt, order = torch.sort(lab, stable=True)
        offsets = torch.searchsorted(srt, torch.arange(K + 1, dtype=torch.int32, device="cuda")).contiguous()
        w = to_dev(None if weights is None else np.asarray(weights, np.float32))
        before = [t.clone() for t in (x, order, offsets)] + ([w.clone()] if w is not None else [])
        cen, wsum, count = Out((K, D), "float32", init=prev), Out((K,), "float64"), Out((K,), "int32")
        nb = int(self.lib.egs_kmeans_update_ws_bytes(N, D, K))
        assert nb == (N // CHUNK + K) * (D + 1) * 8
        ws = Out((nb // 8,), "float64")
        assert self._run(self.lib.egs_kmeans_update, N, D, K, ptr(x), ptr(w), ptr(order), ptr(offsets), cen.ptr, wsum.ptr,
                         count.ptr, ws.ptr, nb) == 0
        ws.numpy()                                                             # (its guards)
        for a, b in zip(before, [x, order, offsets] + ([w] if w is not None else [])):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "an input was modified"
        return cen.numpy(), wsum.numpy(), count.numpy()


# ------------------------------------------------------------------------------------------------------------- assign
@pytest.mark.parametrize("shape", KR.SHAPES)
def test_lattice_cases_exact(lib, shape):
    x, c = KR.lattice_case(*shape)
    want, d64 = KR.assign(x, c)
    labels, dist, cnorm = Runner(lib).assign(*on_device("lattice", shape))
    assert labels.dtype == np.int32 and np.array_equal(labels, want)          # ties and duplicates: the lowest index
    assert np.array_equal(dist.astype(np.float64), d64)
    assert np.array_equal(cnorm.astype(np.float64), (c.astype(np.float64) ** 2).sum(1))
    none = Runner(lib).assign(*on_device("lattice", shape), dist=False)
    assert same_bits(none[0], labels)


@pytest.mark.parametrize("kind", ["normal", "far"])
@pytest.mark.parametrize("shape", KR.SHAPES)
def test_random_cases_within_the_gap_bound(lib, shape, kind):
    x, c = KR.random_case(*shape, kind=kind)
    labels, dist, _ = Runner(lib).assign(*on_device(kind, shape))
    assert labels.min() >= 0 and labels.max() < shape[1]
    gap, bound = KR.gaps(x, c, labels), KR.gap_bound(x, c)
    i = int(np.argmax(gap - bound))
    print("%s %s: %d of %d labels differ from the float64 argmin, worst gap %.3e (bound there %.3e)" % (
        shape, kind, int((labels != KR.assign(x, c)[0]).sum()), len(x), gap.max(), bound[i]))
    assert (gap <= bound).all()                                               # every row, none left out
    d64 = KR.sqdist(x, c)[np.arange(len(x)), labels]
    # dist is the direct sum of squares: D terms, each difference rounded once
    tol = (shape[2] + 2) * KR.EPS32 * 2 * d64 + 1e-30
    assert (np.abs(dist.astype(np.float64) - d64) <= tol).all()


def test_rows_that_are_not_finite_get_label_0(lib):
    shape = (257, 65, 45)
    x, c = KR.random_case(*shape)
    x = np.array(x)
    clean = Runner(lib).assign(to_dev(x), to_dev(c))[0]
    bad_rows = {3: np.nan, 64: np.inf, 200: -np.inf, 256: np.nan}
    x2 = x.copy()
    x2[3, :] = np.nan                      # a row of NaN
    x2[64, 7] = np.inf                     # +Inf among finite values
    x2[200, 44] = -np.inf
    x2[256, 0] = np.nan                    # the last row, one NaN
    for kw in (dict(), dict(max_blocks=1)):
        labels, dist, _ = Runner(lib, **kw).assign(to_dev(x2), to_dev(c))
        assert labels.min() >= 0 and labels.max() < shape[1]
        ok = np.ones(len(x), bool)
        ok[list(bad_rows)] = False
        assert np.array_equal(labels[ok], clean[ok])                          # the finite rows are unchanged
        assert (labels[~ok] == 0).all()                                       # the documented label
        assert (KR.gaps(x[ok], c, labels[ok]) <= KR.gap_bound(x[ok], c)).all()
        assert not np.isfinite(dist[~ok]).any() and np.isfinite(dist[ok]).all()
    # centroids that are not finite never make a label leave [0, K)
    c2 = np.array(c)
    c2[5, 3], c2[64, 0] = np.nan, np.inf
    labels = Runner(lib).assign(to_dev(x2), to_dev(c2))[0]
    assert labels.min() >= 0 and labels.max() < shape[1] and not np.isin(labels, (5,)).any()


# ------------------------------------------------------------------------------------------------------------- update
def _check_update(got, x, labels, prev, weights, exact_wsum=True):
    c, wsum, count = got
    want32, want64, wsum64, count64 = KR.update(x, labels, prev, weights)
    assert count.dtype == np.int32 and np.array_equal(count, count64)
    if exact_wsum:
        assert np.array_equal(wsum, wsum64)
    keep = ~((count64 > 0) & (wsum64 > 0))
    assert same_bits(c[keep], np.asarray(prev, np.float32)[keep])             # empty and zero-weight clusters keep their bits
    ulp = np.spacing(np.abs(want64).astype(np.float32)).astype(np.float64)
    err = np.abs(c.astype(np.float64) - want64)
    print("update: %d of %d entries not the float64 mean's rounding, worst %.3e ulp" % (
        int((c != want32).sum()), c.size, float((err / ulp).max()) if c.size else 0.0))
    assert (err[~keep] <= ulp[~keep]).all()


@pytest.mark.parametrize("shape", [(515, 131, 45), (257, 63, 24), (256, 2, 64), (515, 2, 1), (1, 65, 45), (255, 131, 24)])
def test_update_against_the_reference(lib, shape):
    N, K, D = shape
    x, c = KR.random_case(*shape)
    labels = KR.assign(x, c)[0]
    prev = np.asarray(c) + np.float32(0.5)
    xd = on_device("normal", shape)[0]
    run = Runner(lib)
    plain = run.update(xd, labels, prev)
    _check_update(plain, x, labels, prev, None)
    ones = run.update(xd, labels, prev, np.ones(N, np.float32))
    assert all(same_bits(a, b) for a, b in zip(plain, ones))                  # weights=None: the bits of weights of 1.0
    r = np.random.default_rng(N + K + D)
    w = r.integers(0, 4, size=N).astype(np.float32)                           # integer weights, zeros among them
    w[labels == labels[0]] = 0                                                # a whole cluster of weight 0
    _check_update(run.update(xd, labels, prev, w), x, labels, prev, w)
    wf = r.uniform(0, 2, size=N).astype(np.float32)
    got = run.update(xd, labels, prev, wf)
    _check_update(got, x, labels, prev, wf, exact_wsum=False)
    assert np.allclose(got[1], KR.update(x, labels, prev, wf)[2], rtol=1e-12, atol=0)


def test_update_of_large_clusters_in_chunks(lib):
    N, D = 3 * CHUNK + 5, 45
    x = KR.random_case(N, 2, D)[0]
    xd = to_dev(x)
    run = Runner(lib)
    prev = np.full((1, D), 7.0, np.float32)
    _check_update(run.update(xd, np.zeros(N, np.int32), prev), x, np.zeros(N, np.int32), prev, None)      # K = 1
    labels = np.full(N, 2, np.int32)                                          # one cluster holds all but one row
    labels[N // 2] = 0
    prev = np.full((4, D), -3.0, np.float32)                                  # clusters 1 and 3 are empty
    got = run.update(xd, labels, prev)
    _check_update(got, x, labels, prev, None)
    assert got[2].tolist() == [1, 0, N - 1, 0] and same_bits(got[0][0], x[N // 2])
    for kw in GRIDS[1:4]:
        again = Runner(lib, **kw).update(xd, labels, prev)
        assert all(same_bits(a, b) for a, b in zip(got, again)), kw


# ------------------------------------------------------------------------------------------------- every entry point
@pytest.mark.parametrize("shape", [(515, 131, 45), (257, 65, 64), (256, 63, 9), (1, 1, 1)])
def test_the_same_bits_on_every_grid_and_stream(lib, shape):
    x, c = KR.random_case(*shape)
    xd, cd = on_device("normal", shape)
    w = np.random.default_rng(1).uniform(0, 1, shape[0]).astype(np.float32)
    first = None
    for kw in GRIDS:                                                          # (the last one: a second call in a row)
        run = Runner(lib, **kw)
        a = run.assign(xd, cd)
        u = run.update(xd, a[0], np.asarray(c), w)
        if first is None:
            first = a + u
        assert all(same_bits(p, q) for p, q in zip(first, a + u)), kw


def test_refused_and_empty_calls_write_nothing(lib):
    N, K, D = 300, 70, 24
    xd, cd = on_device("normal", (515, 131, 24))
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lab, dst, cn = Out((N,), "int32"), Out((N,), "float32"), Out((K,), "float32")
    cen, wsum, count = Out((K, D), "float32"), Out((K,), "float64"), Out((K,), "int32")
    nb = int(lib.egs_kmeans_update_ws_bytes(N, D, K))
    ws = Out((nb // 8,), "float64")
    order = torch.arange(N, device="cuda")
    offsets = torch.zeros(K + 1, dtype=torch.int64, device="cuda")

    def assign(N=N, D=D, K=K, x=ptr(xd), c=ptr(cd), cnorm=cn.ptr, labels=lab.ptr, dist=dst.ptr, mb=0):
        return lib.egs_kmeans_assign(N, D, K, x, c, cnorm, labels, dist, mb, s)

    def update(N=N, D=D, K=K, x=ptr(xd), order=ptr(order), off=ptr(offsets), c=cen.ptr, wsum=wsum.ptr, count=count.ptr,
               wk=ws.ptr, nb=nb, mb=0):
        return lib.egs_kmeans_update(N, D, K, x, None, order, off, c, wsum, count, wk, nb, mb, s)

    for kw in (dict(D=0), dict(D=65), dict(K=0), dict(K=65537), dict(N=-1), dict(x=None), dict(c=None), dict(cnorm=None),
               dict(labels=None), dict(mb=-1), dict(mb=8193), dict(dist=lab.ptr)):
        assert assign(**kw) == BAD_ARG, kw
        assert lib.egs_kmeans_last_error_string().decode().startswith("egs_kmeans error 10001: bad argument")
    for kw in (dict(D=0), dict(D=65), dict(K=0), dict(K=65537), dict(N=-1), dict(x=None), dict(order=None), dict(off=None),
               dict(c=None), dict(wsum=None), dict(count=None), dict(wk=None), dict(nb=nb - 8), dict(mb=-1), dict(mb=8193),
               dict(wk=wsum.ptr)):
        assert update(**kw) == BAD_ARG, kw
        assert lib.egs_kmeans_last_error_string().decode().startswith("egs_kmeans error 10001: bad argument")
    assert assign(N=0) == 0 and update(N=0) == 0                              # N = 0 succeeds and writes nothing
    torch.cuda.synchronize()
    for out in (lab, dst, cn, cen, wsum, count, ws):
        assert out.untouched()


# ---------------------------------------------------------------------------------------------------- the Python layer
def test_python_layer_gives_the_abis_bits(lib):
    from easygaussiansplatting_amd import compress as CP
    shape = (515, 131, 45)
    x, c = KR.random_case(*shape)
    xd, cd = on_device("normal", shape)
    run = Runner(lib)
    labels, dist, _ = run.assign(xd, cd)
    got = CP.assign(xd, cd)
    assert got.is_cuda and got.dtype == torch.int32 and same_bits(got.cpu().numpy(), labels)
    got = CP.assign(xd, cd, return_dist=True)
    assert same_bits(got[0].cpu().numpy(), labels) and same_bits(got[1].cpu().numpy(), dist)
    w = to_dev(np.random.default_rng(3).uniform(0, 1, shape[0]).astype(np.float32))
    for weights in (None, w):
        cur = np.array(c)
        for _ in range(2):                                                    # two iterations by hand through the ABI
            cur = run.update(xd, run.assign(xd, to_dev(cur))[0], cur, None if weights is None else weights.cpu().numpy())[0]
        want_labels = run.assign(xd, to_dev(cur))[0]
        cc, ll = CP.kmeans(xd, shape[1], iters=2, weights=weights, init=cd)
        assert same_bits(cc.cpu().numpy(), cur) and same_bits(ll.cpu().numpy(), want_labels)
    assert torch.equal(cd.cpu(), torch.from_numpy(np.array(c)))               # init is not written
    # the default init rule, and two runs with one seed
    a = CP.kmeans(xd, 40, iters=3, seed=11)
    b = CP.kmeans(xd, 40, iters=3, seed=11)
    assert same_bits(a[0].cpu().numpy(), b[0].cpu().numpy()) and same_bits(a[1].cpu().numpy(), b[1].cpu().numpy())
    assert same_bits(CP.kmeans(xd, 40, iters=0, seed=11)[0].cpu().numpy(), x[KR.init_rows(shape[0], 40, 11)])
    assert not same_bits(CP.kmeans(xd, 40, iters=3, seed=12)[0].cpu().numpy(), a[0].cpu().numpy())
    with pytest.raises(ValueError, match="exceeds the number of rows"):
        CP.kmeans(xd, shape[0] + 1)
    with pytest.raises(ValueError, match="1 to 64 columns"):
        CP.kmeans(torch.zeros((10, 65), device="cuda"), 2)


def test_planted_clusters_give_the_exact_means(lib):
    from easygaussiansplatting_amd import compress as CP
    x, init, centres, labels = KR.planted_case()
    c, l = CP.kmeans(to_dev(x), len(init), iters=1, init=to_dev(init))
    assert np.array_equal(c.cpu().numpy(), centres) and np.array_equal(l.cpu().numpy(), labels)


def test_inertia_does_not_rise(lib):
    from easygaussiansplatting_amd import compress as CP
    N, K, D = 515, 20, 45
    x = KR.random_case(N, 131, D)[0]
    xd = to_dev(x)
    inertia = []
    slack = 0.0
    for t in range(6):                                                        # the state after each of 5 iterations
        c, l = CP.kmeans(xd, K, iters=t, seed=5)
        c, l = c.cpu().numpy(), l.cpu().numpy()
        inertia.append(KR.inertia(x, c, l))
        slack = max(slack, float(KR.gap_bound(x, c).max()))
    print("inertia:", ["%.6f" % v for v in inertia], "slack per step %.3e" % (N * slack))
    for a, b in zip(inertia, inertia[1:]):
        assert b <= a + N * slack
    assert inertia[-1] < 0.9 * inertia[0]
