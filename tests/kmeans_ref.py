"""numpy float64 definitions of what libegs_kmeans.so and ``compress`` compute (include/egs_kmeans.h states the
rules): the nearest-centroid assignment with ties to the lowest index, the weighted centroid update, Lloyd's loop with the
package's init rule, the codec's quantiser with its derived error bounds, the float32 restatement of the kernel's score
formula, and the builders of the cases the CPU and GPU tests share."""
import functools

import numpy as np

ROWS = 256          # EGS_KMEANS_ROWS: rows per workgroup of the assign kernel (R)
TILE = 64           # EGS_KMEANS_TILE: centroids per LDS tile of the assign kernel (T)
CHUNK = 256         # EGS_KMEANS_CHUNK: members per chunk of the update
EPS32 = 2.0 ** -24

# (N, K, D): every N of {1, R-1, R, R+1, 2R+3}, every K of {1, 2, T-1, T, T+1, 2T+3} and every D of {1, 3, 9, 24, 45, 48, 64},
# each with at least two values of the other two
SHAPES = [(1, 1, 1), (1, 65, 45), (1, 64, 48), (255, 2, 3), (255, 131, 24), (255, 65, 48), (256, 63, 9), (256, 64, 48),
          (256, 2, 64), (257, 65, 64), (257, 1, 3), (257, 63, 24), (515, 131, 45), (515, 2, 1), (515, 64, 9)]


def ulp32(v):
    """one float32 ulp at magnitude v"""
    return float(np.spacing(np.float32(abs(v))))


# ---------------------------------------------------------------------------------------------------------- definitions
def sqdist(x, c):
    """[N,K] float64 squared distances, the direct sum of squares"""
    x, c = np.asarray(x, np.float64), np.asarray(c, np.float64)
    out = np.empty((len(x), len(c)))
    for i0 in range(0, len(x), 64):
        out[i0:i0 + 64] = ((x[i0:i0 + 64, None, :] - c[None, :, :]) ** 2).sum(-1)
    return out


def finite_rows(x):
    return np.isfinite(np.asarray(x)).all(1)


def assign(x, c):
    """-> (labels int32 [N], dist float64 [N]): the LOWEST index of the nearest centroid; a row that is not finite -> 0"""
    d = sqdist(x, c)
    ok = finite_rows(x)
    labels = np.zeros(len(d), np.int64)
    labels[ok] = np.argmin(d[ok], axis=1)          # (argmin returns the first of equal minima)
    with np.errstate(invalid="ignore"):
        dist = d[np.arange(len(d)), labels]
    return labels.astype(np.int32), dist


def _fma32(a, b, acc):
    """fmaf on float32 arrays: the product is exact in double; the sum is rounded to double and then to float32 (a double
    rounding that differs from fmaf in rare last-bit cases: this restates the ORDER of the kernel's arithmetic, for the
    bound, not its bits)"""
    with np.errstate(invalid="ignore", over="ignore"):
        return (a.astype(np.float64) * b.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)


def scores32(x, c):
    """The kernel's score in float32: n_k = fma chain of c_kd^2 from +0; acc = n_k; acc = fma(x_d, -2 c_kd, acc), d ascending"""
    x, c = np.asarray(x, np.float32), np.asarray(c, np.float32)
    n = np.zeros(len(c), np.float32)
    for d in range(c.shape[1]):
        n = _fma32(c[:, d], c[:, d], n)
    acc = np.broadcast_to(n, (len(x), len(c))).astype(np.float32)
    for d in range(c.shape[1]):
        acc = _fma32(x[:, d:d + 1], (np.float32(-2) * c[:, d])[None, :], acc)
    return acc


def assign32(x, c):
    """labels of the float32 restatement: strict < in ascending k from +inf, NaN never wins, not-finite rows -> 0"""
    s = scores32(x, c)
    s = np.where(np.isnan(s), np.inf, s)
    labels = np.argmin(s, axis=1)
    labels[~finite_rows(x)] = 0
    return labels.astype(np.int32)


def gap_bound(x, c):
    """[N]: what d64(x, c_label) - min_k d64(x, c_k) may be for ANY float32 summation order of either score formula:
    4 (D + 2) 2^-24 (|x| + max_k |c_k|)^2"""
    x, c = np.asarray(x, np.float64), np.asarray(c, np.float64)
    D = x.shape[1]
    return 4.0 * (D + 2) * EPS32 * (np.linalg.norm(x, axis=1) + np.linalg.norm(c, axis=1).max()) ** 2


def gaps(x, c, labels):
    """[N] float64: d64(x, c_label) - min_k d64(x, c_k)"""
    d = sqdist(x, c)
    return d[np.arange(len(d)), np.asarray(labels, np.int64)] - d.min(1)


def incidence(labels, K):
    """-> (order int64 [N], offsets int64 [K+1]): the stable sort of the labels and the exclusive scan of the counts"""
    labels = np.asarray(labels, np.int64)
    order = np.argsort(labels, kind="stable").astype(np.int64)
    offsets = np.zeros(K + 1, np.int64)
    offsets[1:] = np.cumsum(np.bincount(labels, minlength=K))
    return order, offsets


def update(x, labels, prev, weights=None):
    """-> (centroids float32 [K,D], centroids float64, wsum float64 [K], count int32 [K]): weighted means; a cluster without
    a member or with weight 0 keeps ``prev``"""
    x = np.asarray(x, np.float64)
    prev = np.asarray(prev, np.float32)
    K = len(prev)
    w = np.ones(len(x)) if weights is None else np.asarray(weights, np.float64)
    labels = np.asarray(labels, np.int64)
    wsum = np.bincount(labels, weights=w, minlength=K)
    count = np.bincount(labels, minlength=K).astype(np.int32)
    sums = np.zeros((K, x.shape[1]))
    np.add.at(sums, labels, x * w[:, None])
    keep = ~((count > 0) & (wsum > 0))
    c64 = np.where(keep[:, None], prev.astype(np.float64), sums / np.where(keep, 1.0, wsum)[:, None])
    c32 = c64.astype(np.float32)
    c32[keep] = prev[keep]
    return c32, c64, wsum, count


def init_rows(n, k, seed):
    """the package's init rule: the rows at torch.randperm(n, generator=<CPU generator seeded with seed>)[:k]"""
    import torch
    g = torch.Generator()
    g.manual_seed(int(seed))
    return torch.randperm(n, generator=g)[:k].numpy()


def lloyd(x, k, iters=10, weights=None, seed=0, init=None):
    """-> (centroids float32 [k,D], labels int32 [N]) by the definitions above"""
    x = np.asarray(x, np.float32)
    c = x[init_rows(len(x), k, seed)].copy() if init is None else np.array(init, np.float32)
    for _ in range(iters):
        c = update(x, assign(x, c)[0], c, weights)[0]
    return c, assign(x, c)[0]


def inertia(x, c, labels, weights=None):
    d = sqdist(x, c)[np.arange(len(x)), np.asarray(labels, np.int64)]
    return float(d.sum() if weights is None else (d * np.asarray(weights, np.float64)).sum())


# ---------------------------------------------------------------------------------------------------------------- codec
def quantise(v, bits, lo=None, hi=None):
    """v [N,C] float64 -> (q, lo float32 [C], hi float32 [C]): q = rint((v - lo) / (hi - lo) (2^bits - 1)), 0 where hi == lo"""
    v = np.asarray(v, np.float64)
    if lo is None:
        lo, hi = v.min(0), v.max(0)
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    L = 2 ** bits - 1
    span = hi.astype(np.float64) - lo
    q = np.where(span > 0, np.rint((v - lo) / np.where(span > 0, span, 1) * L), 0)
    return np.clip(q, 0, L).astype(np.uint8 if bits == 8 else np.uint16), lo, hi


def dequantise(q, lo, hi, bits):
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    return (lo + q.astype(np.float64) / (2 ** bits - 1) * (hi - lo)).astype(np.float32)


def column_bound(lo, hi, bits):
    """per column: half a quantisation step plus one float32 ulp of the larger bound"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    ulp = np.array([ulp32(max(abs(a), abs(b))) for a, b in zip(lo, hi)])
    return (hi - lo) / (2.0 * (2 ** bits - 1)) + ulp


def quaternion_angle_bound(bits=8):
    """the rotation angle between a unit quaternion and its decoded, renormalised form when every component errs by at
    most e = 1 / (2^bits - 1) (half a step of the [-1, 1] grid): the 4-vector moves by at most 2 e, so the angle between
    the two unit 4-vectors is at most asin(2 e / (1 - 2 e)) and the ROTATION angle is twice that"""
    e = 1.0 / (2 ** bits - 1)
    return 2.0 * np.arcsin(2 * e / (1 - 2 * e))


def gaussians(n, sh_dim, seed=0):
    """a finite record array with every attribute in a plausible range"""
    from easygaussiansplatting_amd.scene import gsdata_type
    r = np.random.default_rng(seed)
    rot = r.normal(size=(n, 4))
    rot /= np.linalg.norm(rot, axis=1, keepdims=True)
    f = np.float32
    return np.rec.fromarrays([(r.normal(size=(n, 3)) * 3).astype(f), rot.astype(f),
                              np.exp(r.normal(size=(n, 3)) - 3).astype(f), r.uniform(0, 1, n).astype(f),
                              (r.normal(size=(n, sh_dim)) * 0.3).astype(f)], dtype=gsdata_type(sh_dim))


# ---------------------------------------------------------------------------------------------------------------- cases
@functools.lru_cache(maxsize=None)
def lattice_case(N, K, D, seed=1):
    """small integers, so every float32 operation of either score formula is exact.  c[1] = c[0] + 2 e_0 and x[0] = c[0] + e_0:
    a genuine tie between distinct centroids (any other centroid is at squared distance >= 1 too); c[K-1] = c[0]: bit-identical
    duplicates; x[1] = c[0], x[2] = c[K-1]: rows bit-equal to a centroid; the other rows are random lattice points or copies
    of centroids"""
    r = np.random.default_rng(seed + 1000 * N + 10 * K + D)
    c = r.integers(-3, 4, size=(K, D)).astype(np.float32)
    x = r.integers(-4, 5, size=(N, D)).astype(np.float32)
    if K >= 2:
        c[1] = c[0]
        c[1, 0] += 2
    if K >= 3:
        c[K - 1] = c[0]
    copies = r.integers(0, K, size=N)
    take = r.uniform(size=N) < 0.25
    x[take] = c[copies[take]]
    x[0] = c[0]
    if K >= 2:
        x[0, 0] += 1
    if N >= 2:
        x[1] = c[0]
    if N >= 3:
        x[2] = c[K - 1]
    x.setflags(write=False)
    c.setflags(write=False)
    return x, c


@functools.lru_cache(maxsize=None)
def random_case(N, K, D, kind="normal", seed=2):
    """normal rows, centroids drawn from the rows plus noise; kind "far": the same around a point of norm about 1e3"""
    r = np.random.default_rng(seed + 1000 * N + 10 * K + D)
    x = r.normal(size=(N, D))
    c = x[r.integers(0, N, size=K)] + 0.1 * r.normal(size=(K, D))
    if kind == "far":
        shift = r.normal(size=D)
        shift *= 1e3 / np.linalg.norm(shift)
        x, c = x + shift, c + shift
    x, c = x.astype(np.float32), c.astype(np.float32)
    x.setflags(write=False)
    c.setflags(write=False)
    return x, c


def planted_case(k=5, per=40, D=9):
    """well-separated lattice clusters: centre j at 100 j e_0, members at integer offsets in [-2, 2] that sum to zero over
    the cluster -- so the exact mean is the centre -- and one init row per cluster -> (x, init, centres, labels)"""
    r = np.random.default_rng(7)
    centres = np.zeros((k, D), np.float32)
    centres[:, 0] = 100.0 * np.arange(k)
    off = r.integers(-2, 3, size=(k, per // 2, D)).astype(np.float32)
    off = np.concatenate([off, -off], axis=1)                          # sums to zero
    x = (centres[:, None, :] + off).reshape(k * per, D)
    labels = np.repeat(np.arange(k), per)
    perm = r.permutation(len(x))
    x, labels = x[perm], labels[perm]
    init = np.stack([x[np.nonzero(labels == j)[0][0]] for j in range(k)])
    return x, init, centres, labels.astype(np.int32)
