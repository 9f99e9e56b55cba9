"""The definitions of include/egs_meshops.h in numpy: connected components by a plain union-find (minimum
index labels and the two count arrays), removal of small components with its ordering rules, the vertex-to-face incidence,
vertex normals and the Taubin iteration in float64 in row order -- each also restated in float32 -- and the generated cases
the CPU and GPU tests share.

NORMALS.  A vertex is DECIDED when |S| >= 1e-6 x the sum of |(b - a) x (c - a)| over its row: there the direction S / |S|
is conditioned well enough for a comparison.  At most ``UNDECIDED_CAP`` = 1 % of a case's vertices that have a face may be
undecided, which tests/test_mesh_ops_cpu.py asserts from float64 alone for every case.

THE RULE of the Taubin comparison (that of tests/tsdf_ref.py): an implementation may be off the float64 result (no
intermediate rounding) by 4 x what the float32 restatement is off on that case, and at least one float32 ulp of the largest
coordinate.
"""
import functools

import numpy as np

from tests import tsdf_ref as TR

UNDECIDED_CAP = 0.01
DECIDED_REL = 1e-6
LAM, MU = 0.5, -0.53


# ------------------------------------------------------------------------------------------------------------ components
def components(faces, n_vertices):
    """-> (label, comp_faces, comp_verts) int32 [V]: a plain union-find whose roots are minimum indices"""
    parent = list(range(n_vertices))

    def find(v):
        r = v
        while parent[r] != r:
            r = parent[r]
        while parent[v] != r:
            parent[v], v = r, parent[v]
        return r

    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    valid = ((faces >= 0) & (faces < n_vertices)).all(1) if len(faces) else np.zeros(0, bool)
    for a, b, c in faces[valid].tolist():
        for x in (b, c):
            ra, rx = find(a), find(x)
            if ra != rx:
                parent[max(ra, rx)] = min(ra, rx)
    label = np.array([find(v) for v in range(n_vertices)], np.int32).reshape(n_vertices)
    comp_verts = np.bincount(label, minlength=n_vertices).astype(np.int32)[:n_vertices]
    comp_faces = np.bincount(label[faces[valid][:, 0]], minlength=n_vertices).astype(np.int32)[:n_vertices]
    return label, comp_faces, comp_verts


def ranks(comp_faces):
    """rank[r]: the position of index r in the order "more faces first, ties to the smaller index" """
    order = np.argsort(-comp_faces.astype(np.int64), kind="stable")
    rank = np.empty(len(comp_faces), np.int32)
    rank[order] = np.arange(len(comp_faces), dtype=np.int32)
    return rank


def keep_flags(faces, n_vertices, min_faces=None, keep_largest=None):
    """-> (vkeep [V], fkeep [F]) int32"""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    label, cf, _ = components(faces, n_vertices)
    keep_comp = cf >= max(1, 0 if min_faces is None else min_faces)
    if keep_largest is not None:
        keep_comp &= ranks(cf) < keep_largest
    vkeep = keep_comp[label] if n_vertices else np.zeros(0, bool)
    valid = ((faces >= 0) & (faces < n_vertices)).all(1) if len(faces) else np.zeros(0, bool)
    fkeep = np.zeros(len(faces), bool)
    fkeep[valid] = vkeep[faces[valid][:, 0]]
    return vkeep.astype(np.int32), fkeep.astype(np.int32)


def remove(vertices, faces, colors=None, normals=None, min_faces=None, keep_largest=None):
    """-> (vertices', faces', colors', normals'): kept rows in their order, indices rewritten"""
    vkeep, fkeep = keep_flags(faces, len(vertices), min_faces, keep_largest)
    new = np.cumsum(vkeep, dtype=np.int64) - 1
    sel = vkeep.astype(bool)
    f = new[np.asarray(faces, np.int64).reshape(-1, 3)[fkeep.astype(bool)]].reshape(-1, 3)
    return (vertices[sel], f, None if colors is None else colors[sel], None if normals is None else normals[sel])


# ------------------------------------------------------------------------------------------------- normals and smoothing
def incidence(faces, n_vertices):
    """-> (row_start [V+1], rows [3F]) int64: entries 3 f + k grouped by vertex, ascending within a vertex"""
    flat = np.asarray(faces, np.int64).reshape(-1)
    rows = np.argsort(flat, kind="stable").astype(np.int64)
    row_start = np.searchsorted(flat[rows], np.arange(n_vertices + 1)).astype(np.int64)
    return row_start, rows


def _row_sum(values, owner, n_vertices):
    """per vertex the sum of its entries' ``values`` in the order given (np.add.at adds one entry after another, in the
    dtype of the values)"""
    acc = np.zeros((n_vertices, values.shape[1]), values.dtype)
    np.add.at(acc, owner, values)
    return acc


def normals(vertices, faces, dtype=np.float64):
    """-> (n [V,3] ``dtype``, decided [V] bool, has_face [V] bool)"""
    V = len(vertices)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    p = np.asarray(vertices, np.float32).astype(dtype)
    row_start, rows = incidence(faces, V)
    tri = p[faces]
    u, w = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    cr = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2],
                   u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1).astype(dtype) if len(faces) else np.zeros((0, 3), dtype)
    owner = faces.reshape(-1)[rows]
    S = _row_sum(cr[rows // 3], owner, V)
    total = _row_sum(np.linalg.norm(cr.astype(np.float64), axis=1)[rows // 3][:, None], owner, V)[:, 0]
    with np.errstate(all="ignore"):
        ln = np.sqrt((S[:, 0] * S[:, 0] + S[:, 1] * S[:, 1]) + S[:, 2] * S[:, 2])
        ok = (ln > 0) & np.isfinite(ln)
        n = np.where(ok[:, None], S / np.where(ok, ln, 1)[:, None], 0).astype(dtype)
    decided = ln.astype(np.float64) >= DECIDED_REL * total
    return n, decided, np.diff(row_start) > 0


def taubin(vertices, faces, iterations, lam=LAM, mu=MU, dtype=np.float64):
    """-> [V,3] ``dtype``: the iteration carried in ``dtype`` throughout (float64: no intermediate rounding)"""
    V = len(vertices)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    p = np.asarray(vertices, np.float32).astype(dtype)
    row_start, rows = incidence(faces, V)
    owner = faces.reshape(-1)[rows]
    f, k = rows // 3, rows % 3
    q, r = faces[f, (k + 1) % 3], faces[f, (k + 2) % 3]
    deg = np.diff(row_start)
    den = (2 * np.maximum(deg, 1)).astype(dtype)[:, None]
    for _ in range(iterations):
        for s in (dtype(lam), dtype(mu)):
            m = _row_sum(p[q] + p[r], owner, V) / den
            p = np.where((deg > 0)[:, None], p + s * (m - p), p).astype(dtype)
    return p


# ----------------------------------------------------------------------------------------------------------------- cases
def _tet(rng, centre, size):
    """four vertices and four outward faces of a random tetrahedron"""
    v = centre + size * rng.normal(size=(4, 3))
    f = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int64)
    if np.dot(np.cross(v[1] - v[0], v[2] - v[0]), v[3] - v[0]) > 0:      # vertex 3 must lie BEHIND face (0, 1, 2)
        f = f[:, ::-1]
    return v, f


def disjoint(nf, seed=0):
    rng = np.random.default_rng(seed + nf)
    v = rng.normal(size=(3 * nf, 3)) + np.repeat(np.arange(nf), 3)[:, None] * np.array([3.0, 0, 0])
    return v, np.arange(3 * nf, dtype=np.int64).reshape(nf, 3)


def strip(nf=70001, seed=1):
    """a strip of nf triangles, consistently oriented, its vertex ids randomly permuted: one component, long paths"""
    rng = np.random.default_rng(seed)
    j = np.arange(nf + 2)
    v = np.stack([0.01 * (j // 2), 0.01 * (j % 2), 0.002 * np.sin(0.37 * j)], 1)
    i = np.arange(nf)
    f = np.stack([np.where(i % 2 == 0, i, i + 1), np.where(i % 2 == 0, i + 1, i), i + 2], 1)
    perm = rng.permutation(nf + 2)
    out = np.empty_like(v)
    out[perm] = v
    return out, perm[f].astype(np.int64)


def fan(nf=5000, hub=1234):
    """nf faces around one hub vertex (a cone): every CAS lands on one root, one CSR row has nf entries"""
    th = 2 * np.pi * np.arange(nf) / nf
    rim = np.stack([np.cos(th), np.sin(th), np.zeros(nf)], 1)
    v = np.insert(rim, hub, [0.0, 0.0, 0.3], axis=0)
    ids = np.arange(nf)
    ids = ids + (ids >= hub)
    f = np.stack([np.full(nf, hub), ids, np.roll(ids, -1)], 1)
    return v, f.astype(np.int64)


def tets(n=300, seed=2):
    """n tetrahedra of which pairs share exactly one vertex (a non-manifold pinch: ONE component under vertex
    connectivity)"""
    rng = np.random.default_rng(seed)
    vs, fs, at = [], [], 0
    for i in range(n):
        v, f = _tet(rng, np.array([4.0 * (i // 2), 0.0, 0.0]) + (i % 2) * np.array([1.5, 0.3, 0.2]), 0.5 + 0.4 * rng.random())
        if i % 2 == 0:
            vs.append(v)
            fs.append(f + at)
            pinch = at + 3
            at += 4
        else:                      # its vertex 0 is the previous one's vertex 3
            ids = np.array([pinch, at, at + 1, at + 2])
            vs.append(v[1:])
            fs.append(ids[f])
            at += 3
    return np.concatenate(vs), np.concatenate(fs).astype(np.int64)


def unreferenced(seed=3):
    """tetrahedra and single triangles with vertices no face names at the start (2), in the middle (3), at the end (2)"""
    rng = np.random.default_rng(seed)
    v1, f1 = tets(6, seed)
    v2, f2 = disjoint(5, seed)
    lone = lambda k: rng.normal(size=(k, 3))
    v = np.concatenate([lone(2), v1, lone(3), v2 + 40.0, lone(2)])
    f = np.concatenate([f1 + 2, f2 + 2 + len(v1) + 3])
    return v, f.astype(np.int64)


def degenerate(seed=4):
    """a tetrahedron, faces (a, a, b) and (a, a, a) -- some on vertices of their own --, and a duplicated face"""
    rng = np.random.default_rng(seed)
    v, f = _tet(rng, np.zeros(3), 1.0)
    v = np.concatenate([v, rng.normal(size=(4, 3)) + 5.0])
    extra = np.array([[1, 1, 2], [3, 3, 3], [4, 4, 5], [6, 6, 6], [0, 1, 2], f[1]], np.int64)
    return v, np.concatenate([f, extra, f[:1]]).astype(np.int64)


def equal_counts(seed=5):
    """components with equal face counts, not in label order of size: two triangles, a pair of pinched tetrahedra (8
    faces), three tetrahedra (4 each), two more triangles"""
    rng = np.random.default_rng(seed)
    parts = [disjoint(2, seed), tets(2, seed)] + [_tet(rng, np.array([0.0, 9.0 * (k + 1), 0.0]), 0.7) for k in range(3)] \
        + [disjoint(2, seed + 1)]
    vs, fs, at = [], [], 0
    for v, f in parts:
        vs.append(v)
        fs.append(f + at)
        at += len(v)
    return np.concatenate(vs), np.concatenate(fs).astype(np.int64)


def sphere_with_floaters():
    """a sphere and two small ones at 33^3 through the reference extraction: 5 440 vertices, 10 868 faces, components of
    10 364, 396 and 108 faces"""
    lat, f0, w = TR.sphere_volume(33)
    f1 = TR.sphere_volume(33, 0.12, (0.8, 0.8, 0.8))[1]
    f2 = TR.sphere_volume(33, 0.07, (-0.8, 0.75, -0.7))[1]
    V, F, _ = TR.weld(TR.extract(lat, np.minimum(np.minimum(f0, f1), f2), w))
    return V, F


def field():
    """``smooth_field((17, 15, 13))``: 13 862 faces in components of 13 820, 30 and 12, with colours"""
    lat, f, w, c = TR.smooth_field((17, 15, 13))
    return TR.weld(TR.extract(lat, f, w, c))


BUILDERS = dict([("disjoint-%d" % n, functools.partial(disjoint, n)) for n in (0, 1, 2, 63, 64, 65, 255, 256, 257)] +
                [("strip-70001", strip), ("fan-5000", fan), ("tets-300", tets), ("unreferenced", unreferenced),
                 ("degenerate", degenerate), ("equal-counts", equal_counts), ("sphere-floaters", sphere_with_floaters),
                 ("field-17x15x13", field)])

# (min_faces, keep_largest) pairs every case is removed with
REMOVALS = [(2, None), (None, 1), (None, 2), (5, 3), (200, None)]


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(V float32 [V,3], F int64 [F,3], C float32 [V,3], label, comp_faces, comp_verts): built once, shared, never
    modified (the arrays are read-only)"""
    got = BUILDERS[name]()
    V = np.ascontiguousarray(got[0], np.float64).reshape(-1, 3).astype(np.float32)
    F = np.ascontiguousarray(got[1], np.int64).reshape(-1, 3)
    if len(got) > 2 and got[2] is not None:
        C = np.ascontiguousarray(got[2]).astype(np.float32)
    else:
        C = np.random.default_rng(len(V)).random((len(V), 3)).astype(np.float32)
    label, cf, cv = components(F, len(V))
    out = dict(V=V, F=F, C=C, label=label, comp_faces=cf, comp_verts=cv)
    for a in out.values():
        a.setflags(write=False)
    return out


def ulp32(x):
    return TR.ulp32(x)
