"""Compressed scene files: the higher-order SH coefficients of a Gaussian set vector-quantised against a
codebook that k-means builds on the GPU, every other attribute quantised to 8 or 16 bits, in one ``.gsz`` archive.

* ``assign(x, centroids)`` / ``kmeans(x, k, ...)`` -- Lloyd's iteration on device tensors through libegs_kmeans.so
  (``_kmeanslib``; include/egs_kmeans.h states every rule).  There is no fallback and no host readback inside the loop.
* ``encode(gs, ...)`` / ``decode(d)`` -- a record array (``scene.gsdata_type``) to and from the fields of format version 1.
* ``save_compressed(path, gs, ...)`` / ``load_compressed(path)`` -- one ``np.savez_compressed`` archive;
  ``gau_io.load_gs`` dispatches ``.gsz`` here.

FORMAT, version 1.  A quantised field q of b bits is stored with its float32 minimum and maximum per column and decodes,
in double, to min + q / (2^b - 1) * (max - min), rounded once to float32 (a column with max == min decodes exactly).

  pw        uint16 [N,3]  over the bounding box                  pw_min / pw_max   [3]
  scale     uint8  [N,3]  of log(scale)                          scale_min / scale_max [3]
  rot       uint8  [N,4]  of the unit quaternion with w >= 0, over [-1, 1]; the decoder renormalises
  alpha     uint8  [N]    over [0, 1]
  sh_dc     uint8  [N,3]                                         sh_dc_min / sh_dc_max [3]
  sh_rest_codebook float16 [K,D], sh_rest_index uint16 [N] (uint8 when K <= 256); absent at SH degree 0 (D = 0)
  meta      a JSON string: version, n, sh_dim, clusters, bits

At the defaults about 19 B per Gaussian plus 2 D B per centroid against 4 (14 + D) B: 19 B + 90 B per centroid against 236 B
at SH degree 3.  ``bits`` chooses 8 or 16 per attribute.  The default number of centroids, min(65536, max(1, N // 4)), is
gsplat's figure for its ``PngCompression``; NOBODY HAS TUNED it here, nor measured what a real capture loses.

Limits: the position grid spans the bounding box, so ONE distant floater coarsens every position; empty clusters are not
reseeded; there is no Morton ordering and no entropy coding beyond the archive's deflate; nothing renders the compressed
form directly.
"""
from __future__ import annotations

import json
import zipfile

import numpy as np

from .scene import gsdata_type

FORMAT_VERSION = 1
DEFAULT_BITS = {"pw": 16, "scale": 8, "rot": 8, "alpha": 8, "sh_dc": 8}
DEFAULT_MAX_CLUSTERS = 65536
_COLUMNS = {"pw": 3, "scale": 3, "rot": 4, "alpha": 1, "sh_dc": 3}


class GszFormatError(ValueError):
    pass


# ------------------------------------------------------------------------------------------------------------ k-means
def _rows(x, name="x"):
    import torch
    from . import _kmeanslib
    from ._host import _chk
    x = _chk(x, name, torch.float32, (None, None))
    if not 1 <= x.shape[1] <= _kmeanslib.MAX_D:
        raise ValueError("%s must have 1 to %d columns, got %d" % (name, _kmeanslib.MAX_D, x.shape[1]))
    if x.shape[0] >= 2 ** 31:
        raise ValueError("%s has too many rows" % name)
    return x


def _centroids(c, D):
    import torch
    from . import _kmeanslib
    from ._host import _chk
    c = _chk(c, "centroids", torch.float32, (None, D))
    if not 1 <= c.shape[0] <= _kmeanslib.MAX_K:
        raise ValueError("1 to %d centroids, got %d" % (_kmeanslib.MAX_K, c.shape[0]))
    return c


def _assign(lib, x, c, cnorm, labels, dist=None):
    from . import _kmeanslib
    from ._host import _ptr, _stream
    _kmeanslib.check(lib.egs_kmeans_assign(x.shape[0], x.shape[1], c.shape[0], _ptr(x), _ptr(c), _ptr(cnorm), _ptr(labels),
                                           _ptr(dist), 0, _stream()))


def assign(x, centroids, return_dist=False):
    """-> labels int32 [N] (and, with ``return_dist``, the squared distances float32 [N]): for every row of ``x`` [N,D] the
    index of the nearest row of ``centroids`` [K,D], ties to the lowest index; a row that is not finite gets label 0."""
    import torch
    from . import _kmeanslib
    x = _rows(x)
    c = _centroids(centroids, x.shape[1])
    lib = _kmeanslib.load()
    labels = torch.empty(x.shape[0], dtype=torch.int32, device=x.device)
    dist = torch.empty(x.shape[0], dtype=torch.float32, device=x.device) if return_dist else None
    cnorm = torch.empty(c.shape[0], dtype=torch.float32, device=x.device)
    _assign(lib, x, c, cnorm, labels, dist)
    return (labels, dist) if return_dist else labels


def kmeans(x, k, iters=10, weights=None, seed=0, init=None):
    """Lloyd's k-means of the rows of ``x`` [N,D] float32 on the device -> (centroids [k,D] float32, labels [N] int32).

    ``init`` [k,D] are the first centroids; by default the rows at ``torch.randperm(N, generator=g)[:k]`` with ``g`` a CPU
    generator seeded with ``seed``, so a run is reproducible bit for bit.  ``weights`` [N] float32 >= 0 weight the means.
    An empty cluster keeps its centroid (no reseeding).  The labels are the assignment to the returned centroids."""
    import torch
    from . import _kmeanslib
    from ._host import _chk, _ptr, _stream
    x = _rows(x)
    N, D = x.shape
    k, iters = int(k), int(iters)
    if not 1 <= k <= _kmeanslib.MAX_K:
        raise ValueError("k must be 1 to %d, got %d" % (_kmeanslib.MAX_K, k))
    if k > N:
        raise ValueError("k = %d exceeds the number of rows %d" % (k, N))
    if iters < 0:
        raise ValueError("iters must be >= 0")
    dev = x.device
    if weights is not None:
        weights = _chk(weights, "weights", torch.float32, (N,))
    if init is None:
        g = torch.Generator()
        g.manual_seed(int(seed))
        c = x[torch.randperm(N, generator=g)[:k].to(dev)].contiguous()
    else:
        c = _centroids(init, D).clone()
        if c.shape[0] != k:
            raise ValueError("init has %d rows, k = %d" % (c.shape[0], k))
    lib = _kmeanslib.load()
    S = _stream()
    labels = torch.empty(N, dtype=torch.int32, device=dev)
    cnorm = torch.empty(k, dtype=torch.float32, device=dev)
    wsum = torch.empty(k, dtype=torch.float64, device=dev)
    count = torch.empty(k, dtype=torch.int32, device=dev)
    ws_bytes = int(lib.egs_kmeans_update_ws_bytes(N, D, k))
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
    edges = torch.arange(k + 1, dtype=torch.int32, device=dev)
    for _ in range(iters):
        _assign(lib, x, c, cnorm, labels)
        srt, order = torch.sort(labels, stable=True)                  # members of a cluster in ascending row index
        offsets = torch.searchsorted(srt, edges).contiguous()         # int64 [k + 1]
        _kmeanslib.check(lib.egs_kmeans_update(N, D, k, _ptr(x), _ptr(weights), _ptr(order), _ptr(offsets), _ptr(c),
                                               _ptr(wsum), _ptr(count), _ptr(ws), ws_bytes, 0, S))
    _assign(lib, x, c, cnorm, labels)
    return c, labels


# -------------------------------------------------------------------------------------------------------------- codec
def _bits(bits):
    out = dict(DEFAULT_BITS)
    if bits is not None:
        for name, b in dict(bits).items():
            if name not in out:
                raise ValueError("bits: unknown attribute %r (expected one of %s)" % (name, sorted(out)))
            if b not in (8, 16):
                raise ValueError("bits[%r] must be 8 or 16, got %r" % (name, b))
            out[name] = int(b)
    return out


def _quantise(v, b, lo=None, hi=None):
    """v [N,C] -> (q uint8/uint16 [N,C], lo float32 [C], hi float32 [C]); the bounds are the columns' own unless given"""
    v = np.asarray(v, np.float64)
    C = v.shape[1]
    if lo is None:
        lo = v.min(0) if len(v) else np.zeros(C)
        hi = v.max(0) if len(v) else np.zeros(C)
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    levels = float(2 ** b - 1)
    span = hi.astype(np.float64) - lo.astype(np.float64)
    t = (v - lo.astype(np.float64)) / np.where(span > 0, span, 1.0) * levels
    q = np.clip(np.rint(np.where(span > 0, t, 0.0)), 0.0, levels).astype(np.uint8 if b == 8 else np.uint16)
    return q, lo, hi


def _dequantise(q, lo, hi, b):
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    return (lo + np.asarray(q, np.float64) / float(2 ** b - 1) * (hi - lo)).astype(np.float32)


def default_clusters(n):
    return min(DEFAULT_MAX_CLUSTERS, max(1, int(n) // 4))


def encode(gs, clusters=None, iters=10, weights=None, seed=0, bits=None, codebook=None):
    """Record array (``scene.gsdata_type``) -> dict of the arrays of format version 1 (module docstring).

    The SH rest is clustered on the GPU by ``kmeans(sh_rest, clusters, iters, weights, seed)`` -- ``weights`` [N] >= 0 is an
    importance score (``importance``: LightGaussian's weighting) -- unless ``codebook`` = (centroids [K,D], index [N]) brings
    one; at SH degree 0 there is none and no kernel runs.  Raises ValueError on input that is not finite."""
    bits = _bits(bits)
    gs = np.asarray(gs)
    n = int(gs.shape[0])
    pw = np.asarray(gs["pw"], np.float32).reshape(n, 3)
    rot = np.asarray(gs["rot"], np.float32).reshape(n, 4)
    scale = np.asarray(gs["scale"], np.float32).reshape(n, 3)
    alpha = np.asarray(gs["alpha"], np.float32).reshape(n, 1)
    sh_dim = int(np.prod(gs.dtype["sh"].shape, dtype=np.int64))
    sh = np.asarray(gs["sh"], np.float32).reshape(n, sh_dim)
    if sh_dim < 3 or sh_dim % 3:
        raise ValueError("sh width %d is not 3 * (degree + 1)^2" % sh_dim)
    D = sh_dim - 3
    if not all(np.isfinite(a).all() for a in (pw, rot, scale, alpha, sh)):        # the one host check
        raise ValueError("encode: the Gaussians must be finite")
    if (scale <= 0).any():
        raise ValueError("encode: scales must be positive")
    norm = np.linalg.norm(rot.astype(np.float64), axis=1, keepdims=True)
    if (norm == 0).any():
        raise ValueError("encode: a quaternion is zero")
    unit = rot.astype(np.float64) / norm
    unit = np.where(unit[:, :1] < 0, -unit, unit)
    d = {}
    d["pw"], d["pw_min"], d["pw_max"] = _quantise(pw, bits["pw"])
    d["scale"], d["scale_min"], d["scale_max"] = _quantise(np.log(scale.astype(np.float64)), bits["scale"])
    d["rot"], d["rot_min"], d["rot_max"] = _quantise(unit, bits["rot"], np.full(4, -1.0), np.full(4, 1.0))
    q, d["alpha_min"], d["alpha_max"] = _quantise(np.clip(alpha, 0.0, 1.0), bits["alpha"], np.zeros(1), np.ones(1))
    d["alpha"] = q.reshape(n)
    d["sh_dc"], d["sh_dc_min"], d["sh_dc_max"] = _quantise(sh[:, :3], bits["sh_dc"])
    K = 0
    if D > 0:
        rest = np.ascontiguousarray(sh[:, 3:])
        if codebook is not None:
            cb = np.asarray(codebook[0], np.float32)
            index = np.asarray(codebook[1]).reshape(-1).astype(np.int64)
            if cb.ndim != 2 or cb.shape[1] != D or index.shape[0] != n or not 0 < cb.shape[0] <= DEFAULT_MAX_CLUSTERS:
                raise ValueError("codebook must be ([K,%d] centroids, [%d] indices), K <= %d" % (D, n, DEFAULT_MAX_CLUSTERS))
            if n and (index.min() < 0 or index.max() >= cb.shape[0]):
                raise ValueError("codebook: an index outside [0, K)")
        elif n == 0:
            cb, index = np.zeros((0, D), np.float32), np.zeros(0, np.int64)
        else:
            import torch
            K = default_clusters(n) if clusters is None else int(clusters)
            x = torch.from_numpy(rest).cuda()
            w = None
            if weights is not None:
                w = torch.as_tensor(weights, dtype=torch.float32).reshape(n).cuda()
            c, labels = kmeans(x, K, iters=iters, weights=w, seed=seed)
            cb, index = c.cpu().numpy(), labels.cpu().numpy().astype(np.int64)
        K = int(cb.shape[0])
        with np.errstate(over="ignore"):
            cb16 = cb.astype(np.float16)
        if not np.isfinite(cb16).all():
            raise ValueError("encode: a centroid does not fit float16")
        d["sh_rest_codebook"] = cb16
        d["sh_rest_index"] = index.astype(np.uint8 if K <= 256 else np.uint16)
    d["meta"] = json.dumps({"version": FORMAT_VERSION, "n": n, "sh_dim": sh_dim, "clusters": K, "bits": bits},
                           sort_keys=True)
    return d


def decode(d):
    """The inverse of ``encode``: dict of arrays -> record array (``scene.gsdata_type``)."""
    try:
        meta = json.loads(str(np.asarray(d["meta"])[()]))
        version = meta["version"]
    except (KeyError, ValueError, TypeError) as e:
        raise GszFormatError("not a compressed scene: no readable meta (%s)" % e) from e
    if version != FORMAT_VERSION:
        raise GszFormatError("compressed scene of format version %r; this reader knows version %d" % (version, FORMAT_VERSION))
    try:
        n, sh_dim, K, bits = int(meta["n"]), int(meta["sh_dim"]), int(meta["clusters"]), _bits(meta["bits"])
        out = {}
        for name, C in _COLUMNS.items():
            q = np.asarray(d[name]).reshape(n, C)
            if q.dtype != (np.uint8 if bits[name] == 8 else np.uint16):
                raise GszFormatError("%s is %s at %d bits" % (name, q.dtype, bits[name]))
            out[name] = _dequantise(q, np.asarray(d[name + "_min"]).reshape(C), np.asarray(d[name + "_max"]).reshape(C),
                                    bits[name])
        D = sh_dim - 3
        if D < 0 or D % 3:
            raise GszFormatError("sh width %d" % sh_dim)
        sh = np.zeros((n, sh_dim), np.float32)
        sh[:, :3] = out["sh_dc"]
        if D > 0:
            cb = np.asarray(d["sh_rest_codebook"])
            index = np.asarray(d["sh_rest_index"]).reshape(n).astype(np.int64)
            if cb.dtype != np.float16 or cb.shape != (K, D):
                raise GszFormatError("codebook %s %s, expected float16 %s" % (cb.dtype, cb.shape, (K, D)))
            if n and (K == 0 or index.max() >= K):
                raise GszFormatError("a codebook index outside [0, %d)" % K)
            sh[:, 3:] = cb.astype(np.float32)[index]
    except KeyError as e:
        raise GszFormatError("compressed scene lacks the field %s" % e) from e
    rot = out["rot"].astype(np.float64)
    rot = (rot / np.linalg.norm(rot, axis=1, keepdims=True)).astype(np.float32) if n else out["rot"]
    scale = np.exp(out["scale"].astype(np.float64)).astype(np.float32)
    return np.rec.fromarrays([out["pw"], rot, scale, out["alpha"].reshape(n), sh], dtype=gsdata_type(sh_dim))


def save_compressed(path, gs, **kw):
    """``encode(gs, **kw)`` into one deflated archive at ``path`` (written through a file object, so the name stays as it
    is: ``.gsz`` by convention) -> the dict it wrote."""
    d = encode(gs, **kw)
    with open(path, "wb") as f:
        np.savez_compressed(f, **d)
    return d


def load_compressed(path):
    """-> record array: ``decode`` of the archive ``save_compressed`` wrote."""
    try:
        with np.load(path, allow_pickle=False) as z:
            d = {k: z[k] for k in z.files}
    except (zipfile.BadZipFile, EOFError, OSError, ValueError) as e:
        if isinstance(e, FileNotFoundError):
            raise
        raise GszFormatError("%s: not a readable compressed scene (%s)" % (path, e)) from e
    return decode(d)
