"""The definition of include/egs_tsdf.h in numpy: TSDF integration of one view in float64 and, with the
same operation order, in float32 (what the kernel's arithmetic is expected to lose); extraction of the zero level set by
marching tetrahedra in float64, written from the geometry of a tetrahedron and NOT from a case table; and the generated
cases the CPU and GPU tests share.

DECISIONS.  Which pixel a sample falls on and whether it is skipped are discrete: float32 and float64 may differ where a
quantity sits on its threshold.  ``decided`` marks the samples whose float64 decisions all have margin -- ``u + 0.5`` and
``v + 0.5`` at least 1e-3 px from an integer; ``p_c.z - near``, ``alpha - alpha_min``, ``z_s - depth_max`` and
``sdf + trunc`` at least 1e-5 of the larger of their operands from 0 -- a margin being asked for only where the rule it
belongs to is reached.  Value comparisons leave the other samples out; at most ``UNDECIDED_CAP`` = 2 % of a case's samples
may be left out (with u uniform the pixel margin alone takes 4e-3 of them), which tests/test_tsdf_cpu.py asserts for every
case: the cameras have generic rotations, so the lattice does not project onto pixel-boundary lines.

THE RULE of the value comparisons (that of §3.17 and §3.18): an implementation may be off the float64 result by 4 x what the
float32 restatement is off on that case, and at least one float32 ulp of the plane's largest entry.
"""
import itertools

import numpy as np

ALPHA_MIN = 0.5
UNDECIDED_CAP = 0.02
PIXEL_MARGIN = 1e-3
REL_MARGIN = 1e-5
EDGE_TYPES = {(1, 0, 0): 0, (0, 1, 0): 1, (0, 0, 1): 2, (1, 1, 0): 3, (1, 0, 1): 4, (0, 1, 1): 5, (1, 1, 1): 6}


# ------------------------------------------------------------------------------------------------------------ integration
def new_state(dims, color=True, dtype=np.float64):
    nx, ny, nz = dims
    return dict(tsdf=np.ones((nz, ny, nx), dtype), weight=np.zeros((nz, ny, nx), dtype),
                color=np.zeros((3, nz, ny, nx), dtype) if color else None)


def copy_state(s, dtype=None):
    return {k: None if v is None else v.astype(dtype or v.dtype, copy=True) for k, v in s.items()}


def project(lat, view, dtype=np.float64):
    """steps 1-5 for every sample of the lattice, in ``dtype`` with one rounding per operation -> dict(upd [nz,ny,nx] bool,
    pix (py, px) int, t, w, and the quantities the margins are taken on)"""
    f = dtype
    nx, ny, nz = lat["dims"]
    o, vx = [f(v) for v in lat["origin"]], f(lat["voxel"])
    x = (o[0] + vx * np.arange(nx, dtype=f))[None, None, :]
    y = (o[1] + vx * np.arange(ny, dtype=f))[None, :, None]
    z = (o[2] + vx * np.arange(nz, dtype=f))[:, None, None]
    R, t = np.asarray(view["R"], np.float32).astype(f), np.asarray(view["t"], np.float32).astype(f)
    fx, fy, cx, cy = [f(np.float32(v)) for v in view["K"]]
    H, W = view["depth"].shape
    trunc, alpha_min, near = f(np.float32(view["trunc"])), f(np.float32(view["alpha_min"])), f(np.float32(view["near"]))
    depth_max = f(np.inf) if view.get("depth_max") is None else f(np.float32(view["depth_max"]))
    with np.errstate(all="ignore"):
        pc = [((R[k, 0] * x + R[k, 1] * y) + R[k, 2] * z) + t[k] for k in range(3)]
        pz = pc[2]
        s1 = pz > near
        u = (fx * pc[0]) / pz + cx
        v = (fy * pc[1]) / pz + cy
        uu, vv = u + f(0.5), v + f(0.5)
        fu, fv = np.floor(uu), np.floor(vv)
        s2 = s1 & (fu >= 0) & (fu < W) & (fv >= 0) & (fv < H)
        px = np.where(s2, fu, 0).astype(np.int64)
        py = np.where(s2, fv, 0).astype(np.int64)
        d = view["depth"][py, px].astype(f)
        if view.get("alpha") is not None:
            a = view["alpha"][py, px].astype(f)
            s3a = s2 & (a > alpha_min)
            zs = d / np.where(s3a, a, f(1))
        else:
            a, s3a, zs = None, s2, d
        s3 = s3a & np.isfinite(zs) & (zs > 0) & (zs <= depth_max)
        sdf = zs - pz
        s4 = s3 & (sdf >= -trunc)
        tt = np.minimum(f(1), sdf / trunc)
        w = view["weight"][py, px].astype(f) if view.get("weight") is not None else np.ones_like(pz)
        upd = s4 & (w > 0) & np.isfinite(w)
    return dict(upd=upd, py=py, px=px, t=tt, w=w, pz=pz, uu=uu, vv=vv, a=a, zs=zs, sdf=sdf, s1=s1, s2=s2, s3a=s3a, s3=s3,
                near=near, alpha_min=alpha_min, depth_max=depth_max, trunc=trunc)


def decided(lat, view):
    """[nz,ny,nx] bool: the samples whose float64 decisions all have margin (module docstring)"""
    p = project(lat, view, np.float64)
    rel = lambda a, b: np.abs(a - b) >= REL_MARGIN * np.maximum(np.abs(a), np.abs(b))
    with np.errstate(all="ignore"):
        ok = rel(p["pz"], p["near"])
        pixel = (np.abs(p["uu"] - np.round(p["uu"])) >= PIXEL_MARGIN) & (np.abs(p["vv"] - np.round(p["vv"])) >= PIXEL_MARGIN)
        ok &= ~p["s1"] | pixel
        if p["a"] is not None:
            ok &= ~p["s2"] | rel(p["a"], p["alpha_min"])
        zs = np.where(np.isfinite(p["zs"]), p["zs"], 0.0)
        if np.isfinite(p["depth_max"]):
            ok &= ~p["s3a"] | rel(zs, p["depth_max"])
        band = np.abs(p["sdf"] + p["trunc"]) >= REL_MARGIN * np.maximum(np.maximum(np.abs(zs), np.abs(p["pz"])), p["trunc"])
        ok &= ~p["s3"] | band
    return ok


def integrate(state, lat, view, dtype=np.float64):
    """one view into ``state`` (arrays of ``dtype``), in place -> the updated samples [nz,ny,nx] bool"""
    f = dtype
    p = project(lat, view, f)
    m = p["upd"]
    W0, w, t = state["weight"][m], p["w"][m], p["t"][m]
    nw = W0 + w
    state["tsdf"][m] = (W0 * state["tsdf"][m] + w * t) / nw
    if state["color"] is not None:
        img = view["image"].astype(f)
        for c in range(3):
            state["color"][c][m] = (W0 * state["color"][c][m] + w * img[c][p["py"][m], p["px"][m]]) / nw
    state["weight"][m] = nw
    return m


def ulp32(x):
    x = np.float32(abs(float(x)))
    return float(np.spacing(x)) if x > 0 else float(np.spacing(np.float32(1.0)))


def errors(got, want, mask):
    """largest |got - want| per plane over ``mask``"""
    out = {}
    for k in ("tsdf", "weight", "color"):
        if want[k] is None:
            continue
        m = mask if k != "color" else np.broadcast_to(mask, want[k].shape)
        out[k] = float(np.abs(np.asarray(got[k], np.float64)[m] - want[k][m]).max()) if m.any() else 0.0
    return out


def bounds(e_ref, want):
    """THE RULE: 4 x the float32 restatement's loss, at least one float32 ulp of the plane's largest entry"""
    return {k: max(4.0 * e_ref[k], ulp32(np.abs(want[k]).max())) for k in e_ref}


# ------------------------------------------------------------------------------------------------------- generated cases
def look_at(eye, target, roll):
    """Rcw, tcw (float32-representable float64) of a camera at ``eye`` looking at ``target``, rolled about its axis"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    zc = (target - eye) / np.linalg.norm(target - eye)
    up = np.array([0.13, -1.0, 0.21])
    xc = np.cross(-up, zc)
    xc /= np.linalg.norm(xc)
    yc = np.cross(zc, xc)
    c, s = np.cos(roll), np.sin(roll)
    R = np.stack([c * xc + s * yc, -s * xc + c * yc, zc])
    R = R.astype(np.float32).astype(np.float64)
    t = (-R @ eye).astype(np.float32).astype(np.float64)
    return R, t


SPHERE_C, SPHERE_R = np.array([0.1, -0.05, 0.2]), 0.8
PLANE_N, PLANE_D = np.array([0.92, 0.25, -0.3]) / np.linalg.norm([0.92, 0.25, -0.3]), -0.35      # n . p = d

# name -> (eye, target, roll, focal length as a multiple of the image width, surface)
CAMERAS = {
    "front": ((2.9, 0.4, -0.7), (0.05, 0.0, 0.1), 0.3, 0.9, "sphere"),          # all three bands of sdf along its rays
    "inside": ((0.45, 0.2, 0.1), (-0.9, -0.1, 0.25), -0.7, 0.6, "plane"),        # samples behind the camera
    "narrow": ((2.2, -1.3, 1.6), (0.6, 0.5, -0.3), 1.1, 4.0, "sphere"),          # most samples off the image
    "oblique": ((-1.1, 2.4, 1.9), (0.0, 0.1, 0.0), 2.2, 0.8, "plane"),
}


def raycast(surface, R, t, K, H, W):
    """metric z per pixel (0: no hit) of the analytic surface, float64"""
    fx, fy, cx, cy = K
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    dc = np.stack([(xs - cx) / fx, (ys - cy) / fy, np.ones_like(xs)], -1)       # camera-frame ray with z = 1
    dw = dc @ R                                                                  # R^T d
    eye = -R.T @ t
    if surface == "sphere":
        oc = eye - SPHERE_C
        a = (dw * dw).sum(-1)
        b = 2.0 * (dw @ oc)
        c = oc @ oc - SPHERE_R ** 2
        disc = b * b - 4 * a * c
        with np.errstate(invalid="ignore"):
            s = (-b - np.sqrt(disc)) / (2 * a)
            s = np.where(s > 0, s, (-b + np.sqrt(disc)) / (2 * a))
        return np.where((disc > 0) & (s > 0), s, 0.0)
    den = dw @ PLANE_N
    with np.errstate(divide="ignore", invalid="ignore"):
        s = (PLANE_D - eye @ PLANE_N) / den
    return np.where(np.isfinite(s) & (s > 0) & (s < 50), s, 0.0)


def make_lattice(dims, extent=2.4):
    """a lattice centred on the world origin whose longest side is ``extent``"""
    voxel = np.float32(extent / max(max(dims) - 1, 8))
    origin = [np.float32(-0.5 * float(voxel) * (n - 1) + 0.0137 * (k + 1)) for k, n in enumerate(dims)]
    return dict(dims=tuple(int(n) for n in dims), origin=[float(v) for v in origin], voxel=float(voxel))


def make_view(lat, cam, H, W, alpha=True, weight=False, half_alpha=False, seed=0, trunc_voxels=4.0, depth_max=None):
    """a generated view of the analytic surface of camera ``cam``: depth = alpha z, alpha in (0.55, 1] (0 without a hit;
    with ``half_alpha`` 0.2 on the right half of the image), a smooth image, a weight plane in [0.5, 2] with a block of
    zeros.  Without ``alpha`` the depth map is metric with a NaN and an inf among its pixels."""
    eye, target, roll, fmul, surface = CAMERAS[cam]
    R, t = look_at(eye, target, roll)
    K = tuple(float(np.float32(v)) for v in (fmul * W, fmul * W * 1.07, 0.5 * W - 0.37, 0.5 * H + 0.21))
    z = raycast(surface, R, t, K, H, W)
    rng = np.random.default_rng(1000 + seed)
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    a = np.where(z > 0, 0.6 + 0.4 * rng.random((H, W)), 0.0)
    if half_alpha:
        a = np.where(xs >= W // 2, np.minimum(a, 0.2), a)
    view = dict(R=R, t=t, K=K, trunc=float(np.float32(trunc_voxels * lat["voxel"])), alpha_min=ALPHA_MIN,
                near=float(np.float32(0.01)), depth_max=depth_max, cam=cam)
    if alpha:
        view["alpha"] = a.astype(np.float32)
        view["depth"] = (a * z).astype(np.float32)
    else:
        d = z.astype(np.float32)
        d[0, 0], d[H - 1, W // 2] = np.nan, np.inf
        view["alpha"], view["depth"] = None, d
    view["image"] = np.stack([0.5 + 0.5 * np.sin(0.31 * xs + 0.17 * ys + k) for k in range(3)]).astype(np.float32)
    if weight:
        w = (0.5 + 1.5 * rng.random((H, W))).astype(np.float32)
        w[H // 3:H // 3 + 3, W // 4:W // 4 + 4] = 0.0
        view["weight"] = w
    else:
        view["weight"] = None
    return view


LATTICES = [(n, 3, 2) for n in (1, 3, 4, 5, 7, 64, 65)] + [(9, 7, 5), (130, 33, 9)]


def case_list():
    """name -> dict(dims, hw, cam, color, alpha, weight, half_alpha): every lattice from every camera; the three options
    run through their eight combinations, the two image sizes alternate, and the oblique camera's opacity is below
    alpha_min on the right half of its image whenever it has an opacity map"""
    out = {}
    for li, dims in enumerate(LATTICES):
        for ci, cam in enumerate(CAMERAS):
            k = li * len(CAMERAS) + ci + li // 2
            color, alpha, weight = k & 1 == 0, (k >> 1) & 1 == 0, (k >> 2) & 1 == 1
            hw = (12, 16) if (li + ci) & 1 else (20, 33)
            name = "%dx%dx%d-%s-%dx%d%s%s%s" % (dims + (cam, hw[1], hw[0], "-color" if color else "",
                                                         "-alpha" if alpha else "-metric", "-weight" if weight else ""))
            out[name] = dict(dims=dims, hw=hw, cam=cam, color=color, alpha=alpha, weight=weight,
                             half_alpha=alpha and cam == "oblique", seed=k)
    return out


def build_case(c, **kw):
    """-> (lat, view) of an entry of ``case_list``"""
    lat = make_lattice(c["dims"])
    args = dict(alpha=c["alpha"], weight=c["weight"], half_alpha=c["half_alpha"], seed=c["seed"])
    args.update(kw)
    return lat, make_view(lat, c["cam"], c["hw"][0], c["hw"][1], **args)


# ------------------------------------------------------------------------------------------------------------- extraction
def edge_key(lat, lo, hi):
    nx, ny, _ = lat["dims"]
    d = tuple(int(h - l) for l, h in zip(lo, hi))
    return 7 * ((int(lo[2]) * ny + int(lo[1])) * nx + int(lo[0])) + EDGE_TYPES[d]


def cell_index(lat, c):
    nx, ny, _ = lat["dims"]
    return (c[2] * (ny - 1) + c[1]) * (nx - 1) + c[0]


def extract(lat, tsdf, weight, color=None, min_weight=1.0):
    """marching tetrahedra of the float32 planes in float64 -> {cell index: [triangle, ...]} in cell order, a triangle
    being dict(v [3,3] world coordinates, keys (3,), c [3,3] or None).  From the geometry alone: per tetrahedron the inside
    set, the crossing points on the edges between an inside and an outside vertex, one triangle or the planar quad (its
    corners ordered around their centroid) as two, oriented so that the normal agrees with (centroid of the outside
    vertices) - (centroid of the inside ones), along which the linear interpolant grows."""
    nx, ny, nz = lat["dims"]
    f = np.asarray(tsdf, np.float64)
    wt = np.asarray(weight, np.float64)
    col = None if color is None else np.asarray(color, np.float64)
    o, vx = np.asarray(lat["origin"], np.float32).astype(np.float64), float(np.float32(lat["voxel"]))
    out = {}
    if min(nx, ny, nz) < 2:
        return out
    corner = lambda a, dz, dy, dx: a[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]
    offs = list(itertools.product((0, 1), repeat=3))
    with np.errstate(invalid="ignore"):
        valid = np.all([corner(wt, *d) >= min_weight for d in offs], 0)
        neg = np.array([corner(f, *d) < 0 for d in offs])
    mixed = valid & neg.any(0) & ~neg.all(0)
    for cz, cy, cx in zip(*np.nonzero(mixed)):
        tris = []
        for perm in itertools.permutations(range(3)):
            vs = [np.array([cx, cy, cz])]
            for ax in perm:
                e = np.zeros(3, np.int64)
                e[ax] = 1
                vs.append(vs[-1] + e)
            fv = [f[v[2], v[1], v[0]] for v in vs]
            ins = [k for k in range(4) if fv[k] < 0]
            outs = [k for k in range(4) if not fv[k] < 0]
            if not ins or not outs:
                continue
            pts = []
            for i in ins:
                for j in outs:
                    lo, hi = (vs[i], vs[j]) if i < j else (vs[j], vs[i])      # (vertex k + 1 dominates vertex k)
                    flo, fhi = f[lo[2], lo[1], lo[0]], f[hi[2], hi[1], hi[0]]
                    t = flo / (flo - fhi)
                    p = o + vx * (lo + t * (hi - lo))
                    c = None
                    if col is not None:
                        clo, chi = col[:, lo[2], lo[1], lo[0]], col[:, hi[2], hi[1], hi[0]]
                        c = clo + t * (chi - clo)
                    pts.append((p, edge_key(lat, lo, hi), c))
            grow = np.mean([vs[k] for k in outs], 0) - np.mean([vs[k] for k in ins], 0)
            if len(pts) == 4:      # order the quad's corners around their centroid, in the plane across ``grow``
                ctr = np.mean([p[0] for p in pts], 0)
                e1 = pts[0][0] - ctr
                e1 -= grow * (e1 @ grow) / (grow @ grow)
                e2 = np.cross(grow, e1)
                pts.sort(key=lambda p: np.arctan2((p[0] - ctr) @ e2, (p[0] - ctr) @ e1))
                polys = [[pts[0], pts[1], pts[2]], [pts[0], pts[2], pts[3]]]
            else:
                polys = [pts]
            for tri in polys:
                n = np.cross(tri[1][0] - tri[0][0], tri[2][0] - tri[0][0])
                if n @ grow < 0:
                    tri = [tri[0], tri[2], tri[1]]
                tris.append(dict(v=np.stack([p[0] for p in tri]), keys=tuple(p[1] for p in tri),
                                 c=None if col is None else np.stack([p[2] for p in tri])))
        out[cell_index(lat, (int(cx), int(cy), int(cz)))] = tris
    return out


def area_vector(v):
    """sum over triangles [T,3,3] of (b - a) x (c - a) / 2"""
    v = np.asarray(v, np.float64).reshape(-1, 3, 3)
    return 0.5 * np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]).sum(0)


def weld(cells):
    """the reference's triangles welded by key -> (vertices [V,3], faces [F,3], colors [V,3] or None), faces in cell order"""
    keys, where = {}, []
    verts, cols = [], []
    for ci in sorted(cells):
        for tri in cells[ci]:
            face = []
            for s in range(3):
                k = tri["keys"][s]
                if k not in keys:
                    keys[k] = len(verts)
                    verts.append(tri["v"][s])
                    cols.append(None if tri["c"] is None else tri["c"][s])
                face.append(keys[k])
            where.append(face)
    V = np.array(verts, np.float64).reshape(-1, 3)
    C = None if not cols or cols[0] is None else np.array(cols, np.float64)
    return V, np.array(where, np.int64).reshape(-1, 3), C


def closed_and_consistent(faces):
    """every undirected edge lies in exactly two triangles, which run through it in opposite directions"""
    faces = np.asarray(faces, np.int64)
    if len(faces) == 0:
        return False
    d = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    if (d[:, 0] == d[:, 1]).any():
        return False
    directed = set(map(tuple, d.tolist()))
    if len(directed) != len(d):                      # a directed edge twice
        return False
    return all((b, a) in directed for a, b in directed)


def signed_volume(verts, faces):
    v = np.asarray(verts, np.float64)[np.asarray(faces, np.int64)]
    return float(np.einsum("ij,ij->i", v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0)


def euler(verts, faces):
    faces = np.asarray(faces, np.int64)
    d = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]), 1)
    return len(verts) - len(np.unique(d, axis=0)) + len(faces)


def sphere_volume(n, radius=0.6, centre=(0.013, -0.021, 0.008)):
    """f = |p - c| - r on an n^3 lattice over [-1, 1]^3 (all weights 2) -> (lat, tsdf, weight) float32"""
    lat = dict(dims=(n, n, n), origin=[-1.0, -1.0, -1.0], voxel=float(np.float32(2.0 / (n - 1))))
    g = -1.0 + lat["voxel"] * np.arange(n)
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    f = np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - radius
    return lat, f.astype(np.float32), np.full((n, n, n), 2.0, np.float32)


def pattern_volume():
    """512 x 2 x 2: cell 2k carries corner sign pattern k (bit dx | dy << 1 | dz << 2 set: inside).  Inside corners are
    -1, outside ones 1, 3 or 7 by position, so every t = f_lo / (f_lo - f_hi) is a power of two's multiple and, with
    origin 0 and voxel 1, every vertex coordinate is exact in float32.  The odd cells between them mix two patterns."""
    lat = dict(dims=(512, 2, 2), origin=[0.0, 0.0, 0.0], voxel=1.0)
    f = np.zeros((2, 2, 512), np.float32)
    outside = (1.0, 3.0, 7.0)
    for k in range(256):
        for corner in range(8):
            dx, dy, dz = corner & 1, (corner >> 1) & 1, (corner >> 2) & 1
            f[dz, dy, 2 * k + dx] = -1.0 if (k >> corner) & 1 else outside[(k + corner) % 3]
    return lat, f, np.full((2, 2, 512), 1.0, np.float32)


def corner_patterns(tsdf):
    """the set of 8-bit inside patterns of a volume's cells"""
    f = np.asarray(tsdf)
    nz, ny, nx = f.shape
    pat = np.zeros((nz - 1, ny - 1, nx - 1), np.int64)
    for corner in range(8):
        dx, dy, dz = corner & 1, (corner >> 1) & 1, (corner >> 2) & 1
        pat |= (f[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx] < 0).astype(np.int64) << corner
    return pat


def smooth_field(dims, seed=0, color=True):
    """a random field with many crossings (a sum of waves; independent uniform values on a lattice no side of which
    exceeds 5, which waves would leave without a crossing), weights 1..3 -> (lat, tsdf, weight, color or None) float32.
    The lattice is centred on the origin with a voxel of 2^-4 and an origin that is a multiple of it: the sample
    positions are exact in float32."""
    nx, ny, nz = dims
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    if max(dims) <= 5:
        f = rng.uniform(-1, 1, (nz, ny, nx))
    else:
        f = np.zeros((nz, ny, nx))
        for _ in range(6):
            k = rng.normal(size=3) * 0.9
            f += rng.normal() * np.sin(k[0] * x + k[1] * y + k[2] * z + rng.uniform(0, 6.28))
        f = np.clip(0.4 * f, -1, 1)
    voxel = 0.0625
    lat = dict(dims=(nx, ny, nz), origin=[-voxel * ((n - 1) // 2) for n in dims], voxel=voxel)
    w = (1.0 + 2.0 * rng.random((nz, ny, nx))).astype(np.float32)
    c = rng.random((3, nz, ny, nx)).astype(np.float32) if color else None
    return lat, f.astype(np.float32), w, c
