"""The definitions of include/egs_simplify.h in numpy float64: vertex-clustering simplification with
quadric-optimal representatives -- cell keys, clusters, the per-vertex plane quadrics in row order, the per-cluster sums in
member order, the regularised solve by the header's hand-written Cholesky, the face rules -- every operation in the order the
header states, so that agreement to the bit with the device is the normal outcome.  It also holds the cases the CPU and GPU
tests share, each with its ``(cell, origin)``.

POSITIONS AND COLOURS are compared within ONE float32 ulp of the case's largest coordinate magnitude (colour value): both
sides do the same well-conditioned double arithmetic and round once, so only a rounding straddle can separate them.
"""
import functools

import numpy as np

from tests import mesh_ops_ref as MR
from tests import tsdf_ref as TR

BITS = 21
INDEX_MAX = (1 << BITS) - 1
RHO = 1e-3
PLACED_MEAN, PLACED_SOLVED, PLACED_CLAMPED, PLACED_NO_FACE = 0, 1, 2, 3
DBL_MAX = np.finfo(np.float64).max


# ------------------------------------------------------------------------------------------------------------------ cells
def cell_indices(vertices, origin, cell):
    """-> [V,3] int64: floor(((double)p - origin) / cell), clamped to [0, 2^21 - 1], NaN to 0"""
    p = np.asarray(vertices, np.float32).astype(np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        q = np.floor((p - np.asarray(origin, np.float64)) / np.float64(cell))
    q = np.where(np.isnan(q), 0.0, q)
    return np.clip(q, 0.0, float(INDEX_MAX)).astype(np.int64)


def cell_keys(vertices, origin, cell):
    i = cell_indices(vertices, origin, cell)
    return i[:, 0] | (i[:, 1] << BITS) | (i[:, 2] << (2 * BITS))


def key_indices(keys):
    k = np.asarray(keys, np.int64)
    return np.stack([k & INDEX_MAX, (k >> BITS) & INDEX_MAX, (k >> (2 * BITS)) & INDEX_MAX], 1)


def centres(keys, origin, cell):
    """origin + (i + 1/2) cell in double, [n,3]"""
    return np.asarray(origin, np.float64) + (key_indices(keys).astype(np.float64) + 0.5) * np.float64(cell)


def clusters(keys):
    """-> (uniq ascending, cluster [V] int64, member_start [Vc+1], members [V]): members in ascending vertex index"""
    uniq, inverse = np.unique(np.asarray(keys, np.int64), return_inverse=True)
    inverse = inverse.astype(np.int64).reshape(-1)
    members = np.argsort(inverse, kind="stable").astype(np.int64)
    member_start = np.searchsorted(inverse[members], np.arange(len(uniq) + 1)).astype(np.int64)
    return uniq, inverse, member_start, members


# --------------------------------------------------------------------------------------------------------------- quadrics
def vertex_quadrics(vertices, faces, keys, origin, cell):
    """-> [V,9] float64: (a00, a01, a02, a11, a12, a22, g0, g1, g2) of every vertex, summed over its incidence row in row
    order; a face with an index outside [0, V) or with |n| zero or not finite contributes nothing"""
    V = len(vertices)
    p = np.asarray(vertices, np.float32).astype(np.float64).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    out = np.zeros((V, 9), np.float64)
    if V == 0 or len(faces) == 0:
        return out
    row_start, rows = MR.incidence(faces, V)
    rows = rows[row_start[0]:row_start[V]]                      # (entries of indices outside [0, V) lie outside)
    owner = faces.reshape(-1)[rows]
    f = faces[rows // 3]
    ok = ((f >= 0) & (f < V)).all(1)
    rows, owner, f = rows[ok], owner[ok], f[ok]
    a, b, c2 = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
    u, w = b - a, c2 - a
    with np.errstate(all="ignore"):
        nx = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1]
        ny = u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2]
        nz = u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
        L = np.sqrt((nx * nx + ny * ny) + nz * nz)
        good = (L > 0) & (L <= DBL_MAX)
        inv = 1.0 / np.where(good, L, 1.0)
        cen = centres(np.asarray(keys, np.int64)[owner], origin, cell)
        r = a - cen
        d = (nx * r[:, 0] + ny * r[:, 1]) + nz * r[:, 2]
        wx, wy, wz = inv * nx, inv * ny, inv * nz
        vals = np.stack([wx * nx, wx * ny, wx * nz, wy * ny, wy * nz, wz * nz, d * wx, d * wy, d * wz], 1)
    np.add.at(out, owner[good], vals[good])                    # one entry after another, in row order
    return out


def cholesky_solve(A6, b):
    """(A) y = b for rows of symmetric positive definite A = (a00, a01, a02, a11, a12, a22): the header's operation order"""
    a00, a01, a02, a11, a12, a22 = (A6[:, k] for k in range(6))
    with np.errstate(all="ignore"):
        l00 = np.sqrt(a00)
        l10 = a01 / l00
        l20 = a02 / l00
        l11 = np.sqrt(a11 - l10 * l10)
        l21 = (a12 - l20 * l10) / l11
        l22 = np.sqrt((a22 - l20 * l20) - l21 * l21)
        z0 = b[:, 0] / l00
        z1 = (b[:, 1] - l10 * z0) / l11
        z2 = ((b[:, 2] - l20 * z0) - l21 * z1) / l22
        y2 = z2 / l22
        y1 = (z1 - l21 * y2) / l11
        y0 = ((z0 - l10 * y1) - l20 * y2) / l00
    return np.stack([y0, y1, y2], 1)


def place(vertices, colors, keys, origin, cell, quadrics=None):
    """-> (positions [Vc,3] float64 BEFORE the rounding to float32, colours [Vc,3] float64 or None, placed [Vc] int32,
    uniq, cluster).  ``quadrics`` = None: placement "mean"."""
    p = np.asarray(vertices, np.float32).astype(np.float64).reshape(-1, 3)
    uniq, cluster, member_start, members = clusters(keys)
    Vc = len(uniq)
    cen = centres(uniq, origin, cell)
    count = np.diff(member_start).astype(np.float64)[:, None]
    s = np.zeros((Vc, 3))
    np.add.at(s, cluster, p - cen[cluster])                    # members in ascending vertex index
    with np.errstate(all="ignore"):
        ym = s / count
    col = None
    if colors is not None:
        col = np.zeros((Vc, 3))
        np.add.at(col, cluster, np.asarray(colors, np.float32).astype(np.float64))
        col = col / count
    if quadrics is None:
        return cen + ym, col, np.full(Vc, PLACED_MEAN, np.int32), uniq, cluster
    Q = np.zeros((Vc, 9))
    np.add.at(Q, cluster, quadrics)
    with np.errstate(all="ignore"):
        tr = (Q[:, 0] + Q[:, 3]) + Q[:, 5]
        solve = (tr > 0) & (tr <= DBL_MAX)
        rho = RHO * tr
        A = Q[:, :6].copy()
        A[:, 0] += rho
        A[:, 3] += rho
        A[:, 5] += rho
        b = Q[:, 6:9] + rho[:, None] * ym
        A[~solve] = [1, 0, 0, 1, 0, 1]
        y = cholesky_solve(A, b)
    y = np.where(solve[:, None], y, ym)
    h = 0.5 * np.float64(cell)
    yc = np.where(y < -h, -h, np.where(y > h, h, y))
    clamped = (yc != y).any(1) & ~np.isnan(y).any(1)
    placed = np.where(solve, np.where(clamped, PLACED_CLAMPED, PLACED_SOLVED), PLACED_NO_FACE).astype(np.int32)
    return cen + yc, col, placed, uniq, cluster


# ------------------------------------------------------------------------------------------------------------------ faces
def remap_faces(faces, cluster, n_vertices, n_clusters):
    """-> (rotated [F,3] int64, valid [F] int32, key_hi [F], key_lo [F] int64): corners through ``cluster``, the smallest
    first with the orientation kept; (-1, -1, -1), 0 and the key (-1, -1) for a face that is skipped or has two equal
    corners"""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    F = len(faces)
    rot = np.full((F, 3), -1, np.int64)
    hi, lo = np.full(F, -1, np.int64), np.full(F, -1, np.int64)
    if F == 0:
        return rot, np.zeros(0, np.int32), hi, lo
    ok = ((faces >= 0) & (faces < n_vertices)).all(1)
    m = np.where(ok[:, None], np.asarray(cluster, np.int64)[np.where(ok[:, None], faces, 0)], -1)
    ok &= ((m >= 0) & (m < n_clusters)).all(1)
    ok &= (m[:, 0] != m[:, 1]) & (m[:, 1] != m[:, 2]) & (m[:, 0] != m[:, 2])
    k = np.argmin(m, 1)
    idx = (k[:, None] + np.arange(3)) % 3
    r = np.take_along_axis(m, idx, 1)
    rot[ok] = r[ok]
    hi[ok] = r[ok, 0] * n_clusters + r[ok, 1]
    lo[ok] = r[ok, 2]
    return rot, ok.astype(np.int32), hi, lo


def sort_order(hi, lo):
    """the faces in ascending (hi, lo), ties in ascending face index: two stable sorts"""
    o = np.argsort(lo, kind="stable")
    return o[np.argsort(hi[o], kind="stable")].astype(np.int64)


def keep_flags(rot, valid, hi, lo, n_clusters):
    """-> (fkeep [F], ckeep [Vc]) int32: of the valid faces with equal rotated triples the one with the smallest index;
    the clusters a kept face names"""
    F = len(valid)
    fkeep, ckeep = np.zeros(F, np.int32), np.zeros(n_clusters, np.int32)
    if F == 0:
        return fkeep, ckeep
    o = sort_order(hi, lo)
    first = np.ones(F, bool)
    first[1:] = (hi[o][1:] != hi[o][:-1]) | (lo[o][1:] != lo[o][:-1])
    fkeep[o] = (first & (valid[o] != 0)).astype(np.int32)
    ckeep[rot[fkeep != 0].reshape(-1)] = 1
    return fkeep, ckeep


def simplify(vertices, faces, colors, cell, origin, placement="quadric", full=False):
    """-> (V' float32, F' int64, C' float32 or None); with ``full`` a dict of every intermediate as well"""
    V = np.asarray(vertices, np.float32).reshape(-1, 3)
    F = np.asarray(faces, np.int64).reshape(-1, 3)
    keys = cell_keys(V, origin, cell)
    Q = vertex_quadrics(V, F, keys, origin, cell) if placement == "quadric" else None
    pos, col, placed, uniq, cluster = place(V, colors, keys, origin, cell, Q)
    Vc = len(uniq)
    rot, valid, hi, lo = remap_faces(F, cluster, len(V), Vc)
    fkeep, ckeep = keep_flags(rot, valid, hi, lo, Vc)
    new = np.cumsum(ckeep, dtype=np.int64) - 1
    sel = ckeep.astype(bool)
    outF = new[rot[fkeep.astype(bool)]].reshape(-1, 3)
    with np.errstate(all="ignore"):
        outV = pos[sel].astype(np.float32)
        outC = None if col is None else col[sel].astype(np.float32)
    if not full:
        return outV, outF, outC
    info = dict(keys=keys, uniq=uniq, cluster=cluster, quadrics=Q, pos64=pos, col64=col, placed=placed, rot=rot, valid=valid,
                hi=hi, lo=lo, fkeep=fkeep, ckeep=ckeep, Vk=int(ckeep.sum()), Fk=int(fkeep.sum()), V=outV, F=outF, C=outC,
                clusters=Vc, placed_counts=np.bincount(placed, minlength=4)[:4].tolist(),
                degenerate=int(len(F) - valid.sum()), duplicate=int(valid.sum() - fkeep.sum()))
    return outV, outF, outC, info


# ------------------------------------------------------------------------------------------------------------------ cases
SPHERE_LATTICE = TR.make_lattice((33, 33, 33))      # the grid the sphere is simplified on: voxel 0.075
SPHERE_VOXEL = SPHERE_LATTICE["voxel"]
SPHERE_ORIGIN = tuple(o - 0.5 * SPHERE_VOXEL for o in SPHERE_LATTICE["origin"])      # lattice origin - 1/2 voxel
SPHERE_CENTRE = np.array([0.013, -0.021, 0.008])
SPHERE_RADIUS = 0.6
CORNER = np.array([0.3, 0.3, 0.3])
CORNER_CELL = 0.1


def _below(v, frac, cell):
    lo = np.asarray(v, np.float32).astype(np.float64).reshape(-1, 3).min(0) if len(v) else np.zeros(3)
    return tuple(float(x) for x in lo - frac * cell)


def corner_mesh(n=6, h=0.042):
    """three n x n-quad faces of a cube that meet at CORNER and run towards the origin, outward orientation"""
    vs, fs = [], []
    for axis in range(3):
        u, w = (axis + 1) % 3, (axis + 2) % 3
        base = len(vs)
        for i in range(n + 1):
            for j in range(n + 1):
                p = CORNER.copy()
                p[u] -= h * i
                p[w] -= h * j
                vs.append(p)
        at = lambda i, j: base + i * (n + 1) + j
        for i in range(n):
            for j in range(n):      # normal along +axis: (du x dw) points along +axis, the steps run along -u and -w
                fs += [[at(i, j), at(i + 1, j), at(i + 1, j + 1)], [at(i, j), at(i + 1, j + 1), at(i, j + 1)]]
    V = np.array(vs)
    # weld the shared edges (equal coordinates)
    uniq, inv = np.unique(np.round(V / (h / 4)).astype(np.int64), axis=0, return_inverse=True)
    first = np.full(len(uniq), -1, np.int64)
    for i, k in enumerate(inv.reshape(-1)):
        if first[k] < 0:
            first[k] = i
    order = np.argsort(first)
    rank = np.empty(len(uniq), np.int64)
    rank[order] = np.arange(len(uniq))
    return V[first[order]], rank[inv.reshape(-1)][np.array(fs, np.int64)]


def one_cell():
    v = np.array([[0.1, 0.1, 0.1], [0.3, 0.1, 0.2], [0.2, 0.4, 0.1], [0.2, 0.2, 0.45]])
    return v, np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int64)


def opposite():
    v = np.array([[0.1, 0.1, 0.1], [0.15, 0.12, 0.1], [2.1, 0.1, 0.3], [0.2, 2.2, 0.1], [2.15, 0.2, 0.35], [0.3, 2.3, 0.2]])
    return v, np.array([[0, 2, 3], [1, 5, 4], [3, 0, 2]], np.int64)


def same_rotation():
    """six vertices in three cells; the faces are the same cluster triple in its three rotations, once reversed, and one
    face that collapses"""
    v = np.array([[0.1, 0.1, 0.1], [0.2, 0.15, 0.1], [1.1, 0.1, 0.3], [1.2, 0.2, 0.2], [0.2, 1.2, 0.1], [0.3, 1.3, 0.2]])
    return v, np.array([[2, 4, 0], [1, 3, 5], [5, 0, 2], [4, 3, 1], [0, 1, 2], [3, 5, 1]], np.int64)


def ties(n=9):
    """an n x n grid of vertices at exact multiples of 0.125 (every other one ON a boundary of the 0.25 cells)"""
    g = -0.5 + 0.125 * np.arange(n)
    x, y = np.meshgrid(g, g, indexing="ij")
    v = np.stack([x.reshape(-1), y.reshape(-1), 0.25 * ((np.arange(n * n) % 3) - 1)], 1)
    at = lambda i, j: i * n + j
    f = []
    for i in range(n - 1):
        for j in range(n - 1):
            f += [[at(i, j), at(i + 1, j), at(i + 1, j + 1)], [at(i, j), at(i + 1, j + 1), at(i, j + 1)]]
    return v, np.array(f, np.int64)


def big_index(seed=7):
    """coordinates just below 2048 with a cell of 2^-10: indices near 2^21 - 1 on all three axes"""
    rng = np.random.default_rng(seed)
    steps = rng.integers(0, 5, size=(40, 3)).astype(np.float64) + rng.integers(1, 8, size=(40, 3)) / 8.0
    v = 2048.0 - steps * 2.0 ** -10
    f = np.array([rng.choice(40, 3, replace=False) for _ in range(90)], np.int64)
    return v, f


def _standard(name, cell, frac=0.25):
    def build():
        c = MR.case(name)
        return c["V"], c["F"], c["C"], cell, _below(c["V"], frac, cell)
    return build


def _sphere(k):
    def build():
        c = MR.case("sphere-floaters")
        return c["V"], c["F"], c["C"], k * SPHERE_VOXEL, SPHERE_ORIGIN
    return build


def _field():
    c = MR.case("field-17x15x13")
    lat = TR.smooth_field((17, 15, 13))[0]
    return c["V"], c["F"], c["C"], 2 * lat["voxel"], tuple(o - 0.5 * lat["voxel"] for o in lat["origin"])


def _own(builder, cell, origin):
    def build():
        v, f = builder()
        return v, f, None, cell, origin
    return build


BUILDERS = dict([
    ("disjoint-0", _standard("disjoint-0", 0.5)), ("disjoint-1", _standard("disjoint-1", 0.5)),
    ("unreferenced", _standard("unreferenced", 0.8)), ("degenerate", _standard("degenerate", 0.9)),
    ("fan-5000", _standard("fan-5000", 0.25)), ("tets-300", _standard("tets-300", 0.6)),
    ("sphere-floaters@1", _sphere(1)), ("sphere-floaters@2", _sphere(2)), ("sphere-floaters@3", _sphere(3)),
    ("field-17x15x13", _field),
    ("corner", _own(corner_mesh, CORNER_CELL, (-0.08, -0.08, -0.08))),
    ("one-cell", _own(one_cell, 1.0, (0.0, 0.0, 0.0))),
    ("opposite", _own(opposite, 0.5, (0.0, 0.0, 0.0))),
    ("same-rotation", _own(same_rotation, 0.5, (0.0, 0.0, 0.0))),
    ("ties", _own(ties, 0.25, (-0.5, -0.5, -0.5))),
    ("big-index", _own(big_index, 2.0 ** -10, (0.0, 0.0, 0.0))),
])
PLACEMENTS = ("quadric", "mean")


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(V float32, F int64, C float32, cell, origin, quadric=<simplify's full dict>, mean=<the same>): built once,
    shared, never modified (the arrays are read-only)"""
    V, F, C, cell, origin = BUILDERS[name]()
    V = np.ascontiguousarray(np.asarray(V, np.float64).reshape(-1, 3).astype(np.float32))
    F = np.ascontiguousarray(F, np.int64).reshape(-1, 3)
    if C is None:
        C = np.random.default_rng(len(V) + 1).random((len(V), 3)).astype(np.float32)
    C = np.ascontiguousarray(C, np.float32)
    out = dict(V=V, F=F, C=C, cell=float(cell), origin=tuple(float(o) for o in origin))
    for pl in PLACEMENTS:
        out[pl] = simplify(V, F, C, cell, origin, pl, full=True)[3]
    for a in [V, F, C] + [x for pl in PLACEMENTS for x in out[pl].values() if isinstance(x, np.ndarray)]:
        a.setflags(write=False)
    return out


def sphere_largest():
    """the sphere alone (keep_largest = 1): 10 364 faces"""
    c = MR.case("sphere-floaters")
    V, F, _, _ = MR.remove(c["V"], c["F"], keep_largest=1)
    return V, F


def radial_error(V):
    """mean | |p - centre| - radius | of a mesh on the sphere case"""
    return float(np.abs(np.linalg.norm(np.asarray(V, np.float64) - SPHERE_CENTRE, axis=1) - SPHERE_RADIUS).mean())


def ulp32(x):
    return TR.ulp32(x)
