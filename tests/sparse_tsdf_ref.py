"""The allocation rule of include/egs_sparse_tsdf.h in float64 numpy, the coverage condition it documents,
and the cases the CPU and GPU tests of the block-allocated volume share.  Integration and extraction have no restatement
of their own: the dense kernels of libegs_tsdf.so (tests/tsdf_ref.py holds their definition) are the yardstick, bit for
bit.

THE TOUCH RULE.  A pixel passes steps 3 and 5 of include/egs_tsdf.h (opacity, valid depth, depth_max, pixel weight); a
passing pixel marches its ray over p_c.z in [max(near, z_s - trunc), z_s + trunc] and flags the block of the sample
nearest to every march point; a point in the one-block rim around the block grid flags the grid block it touches, every
other point outside is ignored.  The kernel steps by one voxel in float32; ``touch`` steps by a quarter voxel (or less) in
float64, so a point of the kernel's march has a point of this one within an eighth of a voxel of p_c.z: the kernel's
flagged set lies within ONE block (Chebyshev) of this one, and its allocated set -- the dilation by one block -- within
TWO.
"""
import numpy as np

from tests import tsdf_ref as TR

BLOCK = 8
FOOTPRINT_LIMIT = 7.5          # include/egs_sparse_tsdf.h, COVERAGE


def block_dims(dims):
    return tuple((int(n) + BLOCK - 1) // BLOCK for n in dims)


def passing(view):
    """[H,W] bool and z_s [H,W] float64: the pixels that clear steps 3 and 5"""
    d = view["depth"].astype(np.float64)
    ok = np.ones(d.shape, bool)
    zs = d
    with np.errstate(all="ignore"):
        if view.get("alpha") is not None:
            a = view["alpha"].astype(np.float64)
            ok &= a > float(np.float32(view["alpha_min"]))
            zs = d / np.where(ok, a, 1.0)
        dmax = np.inf if view.get("depth_max") is None else float(np.float32(view["depth_max"]))
        ok &= np.isfinite(zs) & (zs > 0) & (zs <= dmax)
        if view.get("weight") is not None:
            w = view["weight"].astype(np.float64)
            ok &= (w > 0) & np.isfinite(w)
    return ok, np.where(ok, zs, 0.0)


def footprint(lat, view):
    """the left side of the coverage condition, its largest value over the passing pixels: (rho + voxel |d| / 2) / voxel +
    1 / 2 with rho = z sqrt(1 / fx^2 + 1 / fy^2) / 2 at z = min(z_s + trunc, z_far), z_far the largest p_c.z of the
    lattice's corners: no sample lies beyond it (0 when no pixel passes)"""
    ok, zs = passing(view)
    if not ok.any():
        return 0.0
    R, t = np.asarray(view["R"], np.float64), np.asarray(view["t"], np.float64)
    o = np.asarray(lat["origin"], np.float64)
    ext = float(lat["voxel"]) * (np.asarray(lat["dims"], np.float64) - 1.0)
    z_far = max(float(R[2] @ (o + ext * np.array([i, j, k])) + t[2]) for i in (0, 1) for j in (0, 1) for k in (0, 1))
    fx, fy, cx, cy = [float(np.float32(v)) for v in view["K"]]
    H, W = ok.shape
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    dlen = np.sqrt(((xs - cx) / fx) ** 2 + ((ys - cy) / fy) ** 2 + 1.0)
    voxel, trunc = float(np.float32(lat["voxel"])), float(np.float32(view["trunc"]))
    rho = 0.5 * np.minimum(zs + trunc, z_far) * np.sqrt(1.0 / fx ** 2 + 1.0 / fy ** 2)
    return float(((rho + 0.5 * voxel * dlen) / voxel + 0.5)[ok].max())


def touch(lat, view, step_voxels=0.25):
    """[nbz,nby,nbx] bool: the blocks the float64 march flags"""
    assert 0 < step_voxels <= 0.25
    nb = np.array(block_dims(lat["dims"]), np.int64)
    flags = np.zeros(tuple(nb[::-1]), bool)
    ok, zs = passing(view)
    if not ok.any():
        return flags
    R, t = np.asarray(view["R"], np.float32).astype(np.float64), np.asarray(view["t"], np.float32).astype(np.float64)
    fx, fy, cx, cy = [float(np.float32(v)) for v in view["K"]]
    o, voxel = np.asarray(lat["origin"], np.float32).astype(np.float64), float(np.float32(lat["voxel"]))
    trunc, near = float(np.float32(view["trunc"])), float(np.float32(view["near"]))
    py, px = np.nonzero(ok)
    zs = zs[py, px]
    z0, z1 = np.maximum(near, zs - trunc), zs + trunc
    steps = int(np.ceil(2.0 * trunc / (step_voxels * voxel))) + 1
    s = np.linspace(0.0, 1.0, steps + 1)[None, :]
    z = z0[:, None] + s * (z1 - z0)[:, None]                                   # [P, steps + 1], both ends included
    pc = np.stack([z * ((px - cx) / fx)[:, None], z * ((py - cy) / fy)[:, None], z], -1)
    pw = (pc - t) @ R                                                           # R^T (p_c - t)
    i = np.floor((pw - o) / voxel + 0.5).astype(np.int64)
    b = np.floor_divide(i, BLOCK)
    keep = ((b >= -1) & (b <= nb)).all(-1)
    b = np.clip(b, 0, nb - 1)[keep]
    flags[b[:, 2], b[:, 1], b[:, 0]] = True
    return flags


def dilate(mask, r=1):
    """the Chebyshev dilation of a [nbz,nby,nbx] bool mask by ``r`` blocks"""
    out = mask.copy()
    for _ in range(r):
        p = np.pad(out, 1)
        acc = np.zeros_like(out)
        for dz in range(3):
            for dy in range(3):
                for dx in range(3):
                    acc |= p[dz:dz + out.shape[0], dy:dy + out.shape[1], dx:dx + out.shape[2]]
        out = acc
    return out


def blocks_of(sample_mask):
    """[nz,ny,nx] bool -> [nbz,nby,nbx] bool: the blocks that hold a marked sample"""
    nz, ny, nx = sample_mask.shape
    nbx, nby, nbz = block_dims((nx, ny, nz))
    full = np.zeros((nbz * BLOCK, nby * BLOCK, nbx * BLOCK), bool)
    full[:nz, :ny, :nx] = sample_mask
    return full.reshape(nbz, BLOCK, nby, BLOCK, nbx, BLOCK).any(axis=(1, 3, 5))


def samples_of(block_mask, dims):
    """[nbz,nby,nbx] bool -> [nz,ny,nx] bool: the samples of the marked blocks"""
    nx, ny, nz = dims
    m = np.asarray(block_mask, bool)
    return np.repeat(np.repeat(np.repeat(m, BLOCK, 0), BLOCK, 1), BLOCK, 2)[:nz, :ny, :nx]


def band_blocks(lat, view):
    """the blocks that hold a decided sample the view updates with t < 1 (float64)"""
    p = TR.project(lat, view)
    with np.errstate(invalid="ignore"):
        band = p["upd"] & (p["t"] < 1) & TR.decided(lat, view)
    return blocks_of(band)


# ------------------------------------------------------------------------------------------------------------------ cases
LATTICES = [(1, 1, 1), (8, 8, 8), (9, 8, 8), (20, 13, 9), (130, 33, 9)]
SIZES = [(12, 16), (20, 33)]           # (H, W)


def make_views(lat, hw, first_seed=0):
    """the three views of the tests in their order: front; oblique with per-pixel weights and half its image under
    alpha_min; inside without an opacity map and with depth_max"""
    H, W = hw
    return [TR.make_view(lat, "front", H, W, seed=first_seed + 1),
            TR.make_view(lat, "oblique", H, W, weight=True, half_alpha=True, seed=first_seed + 2),
            TR.make_view(lat, "inside", H, W, alpha=False, seed=first_seed + 3, depth_max=1.5)]


def case_list():
    """(dims, hw) pairs: every lattice at both image sizes, except that 130 x 33 x 9 -- a voxel of 0.0186 -- takes the
    33 x 20 image only: at 16 x 12 a pixel of the front and oblique cameras is 8 to 10 voxels wide, which the documented
    coverage condition excludes (tests/test_sparse_tsdf_cpu.py asserts the condition on every case listed here)"""
    return [(dims, hw) for dims in LATTICES for hw in SIZES if not (dims == (130, 33, 9) and hw == (12, 16))]


# The end-to-end scene: tests/tsdf_ref's sphere from four cameras at the corners of a tetrahedron around it, into 40^3.
# Four cameras see every point of a sphere, but the point farthest from all of them only at 70.5 degrees from the nearest
# camera's axis: from a distance of 8 the ray meets the surface there at 76 degrees, and a sample 1.73 voxels under it (the
# diagonal of a cell) lies 1.73 / cos 76 = 7.2 voxels behind it along the ray.  A truncation of 10 voxels keeps every corner
# of every cell the surface crosses inside some view's band.  The samples just OUTSIDE the silhouette are the other half:
# a ray that passes 1.73 voxels above a sphere of 13 voxels misses it wherever it would meet the surface at more than 62
# degrees, so the pixels that miss the sphere see a backdrop at z = 20, far behind the lattice, and carry the free-space
# observations that give those samples their weight.  With both, the mesh closes.
E2E_DIMS, E2E_HW, E2E_DISTANCE, E2E_TRUNC_VOXELS, E2E_FOCAL = (40, 40, 40), (48, 64), 8.0, 10.0, 2.4
E2E_BACKDROP = 20.0
E2E_EYES = [tuple(TR.SPHERE_C + E2E_DISTANCE * np.array(d) / np.sqrt(3.0))
            for d in ((1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1))]


def e2e_views(lat):
    """four renders (depth = alpha z, alpha in (0.6, 1]) of the analytic sphere, in fusion order"""
    H, W = E2E_HW
    views = []
    for k, eye in enumerate(E2E_EYES):
        R, t = TR.look_at(eye, TR.SPHERE_C, 0.3 + 0.5 * k)
        K = tuple(float(np.float32(v)) for v in (E2E_FOCAL * W, E2E_FOCAL * W * 1.07, 0.5 * W - 0.37, 0.5 * H + 0.21))
        z = TR.raycast("sphere", R, t, K, H, W)
        rng = np.random.default_rng(2000 + k)
        z = np.where(z > 0, z, E2E_BACKDROP)
        a = 0.6 + 0.4 * rng.random((H, W))
        xs, ys = np.meshgrid(np.arange(W), np.arange(H))
        img = np.stack([0.5 + 0.5 * np.sin(0.31 * xs + 0.17 * ys + c) for c in range(3)]).astype(np.float32)
        views.append(dict(R=R, t=t, K=K, trunc=float(np.float32(E2E_TRUNC_VOXELS * lat["voxel"])), alpha_min=TR.ALPHA_MIN,
                          near=float(np.float32(0.01)), depth_max=None, cam="e2e%d" % k, alpha=a.astype(np.float32),
                          depth=(a * z).astype(np.float32), weight=None, image=img))
    return views
