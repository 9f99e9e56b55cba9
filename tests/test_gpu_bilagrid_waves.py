"""The bilateral-grid kernels (csrc/egs_bilagrid.hip) through the raw C ABI on the hand-built images of
tests/bilagrid_cases.py, which reach every form a wave of k_slice_bwd takes: the matrix form with and without a flush
inside the wave's rows, the uniform wave of the LDS form with all 64 lanes live and with dead lanes, in the interior of a
layer (all eight corners non-zero, L = 2, 5 and 12) and at the clamps, the mixed wave, the global form, waves without
rows, the lattice coordinates two pixels below their cap of 2^22, and the largest LDS request the library can make.
tests/test_bilagrid_cases_cpu.py holds the cases, the census and the bounds against the reference alone.

``out``, ``dimage`` and ``dgrid`` lie between guard bands; ``out`` and ``dimage`` are pattern-filled before the call and
every pixel must have been written; ``dgrid`` starts from random values (0.5 N(0, 1) of the gradient's largest entry) and
what the call ADDED is compared.  No pixel and no entry is excluded from any comparison.

Bound, per pixel of out and dimage and per entry of dgrid: |kernel - float64| <= max(T 2^-24 S, 2 x distance), S the
entry's sum of |terms| (for dgrid of an accumulating call plus |start|), distance the largest distance from float64 of
the nine float32 evaluations of the restatement, T the per-case power of two of ``bilagrid_cases.T`` (8 .. 64, except
where float32 itself is ill-conditioned: the output at L = 128 and dgrid entries that are one pixel's term; the reasons
and the ratios are in that module).

T per case, (out, dimage, dgrid): uniform-L2 16, 16, 8; uniform-L5 32, 16, 16; uniform-L12 64, 16, 32; matrix-nx1 32, 16, 8;
matrix-L1 16, 32, 16; matrix-3rows 16, 16, 8; matrix-box8064 128, 32, 256; global 64, 16, 1024; cap-x-lds 32, 32, 16;
cap-y-matrix 32, 32, 16; cap-x-global 2048, 32, 65536; delta-uniform 32, 8, 64; delta-matrix 32, 8, 32; delta-global 64,
16, 32.  At these T the spread of the restatement's own evaluations is 0.25 .. 0.50 of the floor (the table in
tests/bilagrid_cases.py has each ratio).

Measured on MI355X, per set and tensor: largest distance | largest kernel error | largest error / bound

  uniform  out     4.66e-06 | 1.92e-06 | 0.30        uniform  dimage  3.28e-09 | 2.35e-09 | 0.27
  matrix   out     1.23e-05 | 1.21e-05 | 0.63        matrix   dimage  3.96e-08 | 3.90e-08 | 0.54
  global   out     4.67e-06 | 4.91e-06 | 0.52        global   dimage  7.00e-09 | 6.77e-09 | 0.58
  cap      out     9.59e-05 | 9.54e-05 | 0.56        cap      dimage  9.92e-07 | 9.88e-07 | 0.56
  delta    out     4.67e-06 | 4.91e-06 | 0.52        delta    dimage  1.91e-07 | 1.32e-07 | 0.50
  uniform  dgrid   7.86e-09 | 2.29e-09 | 0.14        cap      dgrid   2.18e-08 | 2.18e-08 | 0.58
  matrix   dgrid   1.62e-08 | 1.14e-08 | 0.50        delta    dgrid   7.80e-08 | 7.80e-08 | 0.50
  global   dgrid   1.59e-09 | 1.55e-09 | 0.28

Where the kernel's error equals the distance (cap, matrix-box8064, global) both are the rounding of the lattice
coordinate, which the kernel and the restatement share: gx up to 512 has an ulp of 6e-5, and that is the error of fx.
The module's 35 tests take 4.0 s together, 0.43 s the slowest (the largest image is 8191 x 3).  The largest launch asks
for 81 920 B of dynamic LDS (matrix-box8064, both halves): it ran, rc = 0, and passes the bounds like the others.

Seeded errors, each run once on a scratch build (never committed; all keep every index inside its box) -> the tests that
fail, first one first.  tests/test_gpu_bilagrid.py notices neither of the first two.

  k2 = (lane + 64) / 12 -> (lane + 60) / 12      test_backward[uniform-L2], [uniform-L5], [uniform-L12], [delta-uniform]
  the ``second`` add dropped                     test_backward[uniform-L2], [uniform-L5], [uniform-L12], [delta-uniform]
  d[..] = 0 of the dead lanes dropped            test_backward[uniform-L2] and the two other uniform cases (uniform dead),
                                                 [matrix-nx1], [matrix-L1], [matrix-3rows], [matrix-box8064],
                                                 [cap-y-matrix] (matrix dead), [delta-uniform], [delta-matrix]
  the flush on ry0 != acc_ry0 dropped            test_backward[matrix-nx1], [matrix-L1], [matrix-box8064], [cap-y-matrix],
                                                 [delta-matrix] (the cases with mat_flush+ waves; not matrix-3rows)
"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import bilagrid_cases as BC

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.loss_abi import PATTERN, guarded, guards_intact  # noqa: E402  (needs torch)

UNWRITTEN = int(np.frombuffer(bytes([PATTERN] * 4), np.int32)[0])


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from easygaussiansplatting_amd import _bilagridlib
    return _bilagridlib.load()


@functools.lru_cache(maxsize=None)
def on_device(name):
    """the inputs of a case on the device: shared, never written to"""
    return {k: v.contiguous().cuda() for k, v in BC.inputs(name).items()}


def dims(name):
    H, W, (gw, gh, L) = BC.shape_of(name)
    return H, W, gw, gh, L


class Guarded:
    """``n`` floats between guard bands: pattern-filled, or holding ``start``"""

    def __init__(self, n, start=None):
        self.whole, inner = guarded(4 * n)
        self.f = inner.view(torch.float32)
        if start is not None:
            self.f.copy_(torch.from_numpy(np.ascontiguousarray(start, np.float32).reshape(-1)))

    def ptr(self):
        return C.c_void_p(self.f.data_ptr())

    def host(self, shape):
        return self.f.cpu().numpy().reshape(shape).copy()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _error(lib):
    return lib.egs_bilagrid_last_error_string().decode("utf-8", "replace")


def forward(lib, name):
    d = on_device(name)
    H, W = dims(name)[:2]
    out = Guarded(3 * H * W)
    rc = lib.egs_bilagrid_slice(torch.cuda.current_device(), _stream(), *dims(name), _p(d["image"]), _p(d["grid"]),
                                out.ptr())
    torch.cuda.synchronize()
    assert rc == 0, (name, rc, _error(lib))
    assert guards_intact(out.whole), (name, "the forward wrote outside out")
    return out.host((3, H, W))


def backward(lib, name, dimage=True, start=None, grid=None):
    """one call of slice_bwd -> (dimage or None, dgrid after the call or None)"""
    d = on_device(name)
    H, W, gw, gh, L = dims(name)
    di = Guarded(3 * H * W) if dimage else None
    dg = Guarded(12 * L * gh * gw, start) if start is not None else None
    rc = lib.egs_bilagrid_slice_bwd(torch.cuda.current_device(), _stream(), H, W, gw, gh, L, _p(d["image"]),
                                    _p(d["grid"] if grid is None else grid), _p(d["dout"]),
                                    di.ptr() if di else None, dg.ptr() if dg else None)
    torch.cuda.synchronize()
    assert rc == 0, (name, "LDS request %d B" % BC.lds_bytes(H, W, (gw, gh, L), dimage, start is not None), rc,
                     _error(lib))
    for b, what in ((di, "dimage"), (dg, "dgrid")):
        if b is not None:
            assert guards_intact(b.whole), (name, "the backward wrote outside " + what)
    return (di.host((3, H, W)) if di else None), (dg.host((12, L, gh, gw)) if dg else None)


def start_of(name, seed):
    """the random buffer a dgrid call accumulates into: 0.5 N(0, 1) of the reference gradient's largest entry"""
    ref = BC.reference(name)["dgrid"]["ref"]
    from easygaussiansplatting_amd import scene as S
    return (0.5 * np.abs(ref).max() * S.normal(31 + seed, 3, ref.shape)).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def close(name, tensor, got, what, start=None):
    """the bound, entry by entry; prints largest distance | largest kernel error | largest error / bound"""
    r = BC.reference(name)[tensor]
    got = np.asarray(got, np.float64)
    if start is not None:
        got = got - np.asarray(start, np.float64)              # what the call added (exact in float64)
    err = np.abs(got - r["ref"])
    bound = BC.bound_of(name, tensor, start)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / bound)
    at = np.unravel_index(np.argmax(ratio), ratio.shape)
    print("MEASURED %-15s %-7s %-22s distance %.3g | error %.3g | error / bound %.3g"
          % (name, tensor, what, r["distance"].max(), err.max(), ratio.max()))
    assert np.isfinite(got).all(), (name, tensor, what)
    assert ratio.max() <= 1.0, (name, tensor, what, "entry %r: %.9g against %.9g, bound %.3g (T = %d)"
                                % (at, got[at], r["ref"][at], bound[at], BC.T[name][BC.TENSORS.index(tensor)]))


def test_the_cases_are_the_ones_the_host_tests_hold():
    assert len(BC.ALL_NAMES) == 14 and set(BC.T) == set(BC.ALL_NAMES)
    assert max(BC.lds_bytes(*BC.shape_of(n)) for n in BC.CASES) == 81920


@pytest.mark.parametrize("name", BC.ALL_NAMES)
def test_forward(lib, name):
    out = forward(lib, name)
    assert not (bits(out) == UNWRITTEN).any(), (name, "a pixel of out was not written")
    close(name, "out", out, "forward")
    assert np.array_equal(bits(forward(lib, name)), bits(out)), (name, "out is not reproducible")


@pytest.mark.parametrize("name", BC.ALL_NAMES)
def test_backward(lib, name):
    start, other = start_of(name, 0), start_of(name, 1)
    both_i, both_g = backward(lib, name, True, start)
    assert not (bits(both_i) == UNWRITTEN).any(), (name, "a pixel of dimage was not written")
    close(name, "dimage", both_i, "both halves")
    close(name, "dgrid", both_g, "both halves", start)
    alone_i, _ = backward(lib, name, True, None)
    assert np.array_equal(bits(alone_i), bits(both_i)), (name, "dimage alone differs from dimage of both halves")
    _, alone_g = backward(lib, name, False, other)
    close(name, "dgrid", alone_g, "dgrid alone", other)
    again_i, again_g = backward(lib, name, True, start)
    assert np.array_equal(bits(again_i), bits(both_i)), (name, "dimage is not reproducible")
    close(name, "dgrid", again_g, "both halves, again", start)
    if name in BC.DELTA_OF:
        hit = np.broadcast_to(BC.intended_nodes(name)[None], start.shape)
        for after, before, what in ((both_g, start, "both halves"), (alone_g, other, "dgrid alone")):
            assert np.array_equal(bits(after)[~hit], bits(before)[~hit]), \
                (name, what, "an entry outside the nodes of the lit pixels lost the start's bits")
            seen = hit & (np.abs(BC.reference(name)["dgrid"]["ref"]) >= 1e-3 * np.abs(before))
            assert seen.any() and (bits(after)[seen] != bits(before)[seen]).all(), \
                (name, what, "a node of a lit pixel was not added to")


@pytest.mark.parametrize("name", ["uniform-L5", "uniform-L12", "matrix-nx1", "matrix-box8064", "global", "cap-x-lds"])
def test_no_guidance_term_outside_01(lib, name):
    """A pixel with luma < 0 reads layer 0 alone (fz = 0, A = A_xy(0) to the bit) and has no guidance term: its dimage
    must not depend on the other layers at all.  (Above 1 the kernel forms A = A_xy(L-2) + 1 (A_xy(L-1) - A_xy(L-2)),
    which rounds: those pixels are held by the bound, whose S has no guidance term outside (0, 1).)"""
    d = on_device(name)
    L = dims(name)[4]
    luma = BC.luma32(BC.inputs(name)["image"].numpy())
    moved = d["grid"].clone()
    moved[:, 1:] = moved[:, 1:] * 1.5 + 0.25
    a, _ = backward(lib, name, True, None)
    b, _ = backward(lib, name, True, None, grid=moved)
    below, inside = luma < 0, (luma > 0) & (luma < 1)
    assert below.any() and inside.any() and L > 1
    assert np.array_equal(bits(a)[:, below], bits(b)[:, below])
    assert (bits(a)[:, inside] != bits(b)[:, inside]).any(axis=0).all()
    want = BC.reference(name)["dimage"]
    assert (np.abs(a - want["ref"])[:, below] <= BC.bound_of(name, "dimage")[:, below]).all()
