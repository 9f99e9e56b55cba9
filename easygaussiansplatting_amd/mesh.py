"""From a trained scene to a triangle mesh: the depth maps rendered at the training cameras
(``RenderOptions(depth=True, alpha=True)``: depth = sum w z, alpha = sum w) are fused into a truncated signed distance
volume, and its zero level set is extracted by marching tetrahedra -- the route 2DGS, PGSR and DN-Splatter take to their
meshes.  Three HIP kernels (csrc/egs_tsdf.hip, libegs_tsdf.so; include/egs_tsdf.h has every rule); integration reads
nothing back, extraction reads one number (the triangle count).

    from easygaussiansplatting_amd.mesh import TSDFVolume, save_mesh_ply
    vol = TSDFVolume(origin=(-1, -1, -1), voxel_size=2 / 255, dims=(256, 256, 256))
    for cam in cams:
        image, _, depth, alpha = GSFunction.apply(..., cam, RenderOptions(depth=True, alpha=True))
        vol.integrate(depth, alpha, cam, image=image)
    save_mesh_ply("mesh.ply", *vol.extract())

``Trainer.extract_mesh`` does the loop over a trainer's cameras.  ``alpha_min`` = 0.5, ``trunc`` = 4 voxels and
``min_weight`` = 1 are defaults NOBODY HAS TUNED.  The expected depth sum w z / sum w bleeds at silhouettes (a pixel that
sees two surfaces reports a depth between them); ``alpha_min`` is the only guard against it here.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _tsdflib
from ._host import _lib_on, _ptr, _stream
from .depthloss import _plane
from .normalloss import _intrinsics, _planes3

ALPHA_MIN = 0.5           # a pixel counts when the render's opacity exceeds it; untuned
TRUNC_VOXELS = 4.0        # the truncation distance in voxels; untuned
MIN_WEIGHT = 1.0          # a cell is meshed when every corner was seen with this total weight; untuned


def _host_pose(cam):
    """(Rcw [3,3], tcw [3]) float64 numpy of a camera: of its numpy fields, or one copy of its device tensors kept on it"""
    if isinstance(cam.Rcw, torch.Tensor):
        got = getattr(cam, "_host_pose", None)
        if got is None or got[0] is not cam.Rcw or got[1] is not cam.tcw:
            got = (cam.Rcw, cam.tcw, cam.Rcw.detach().double().cpu().numpy(), cam.tcw.detach().double().cpu().numpy())
            try:
                cam._host_pose = got
            except AttributeError:
                pass
        return got[2].reshape(3, 3), got[3].reshape(3)
    return np.asarray(cam.Rcw, np.float64).reshape(3, 3), np.asarray(cam.tcw, np.float64).reshape(3)


def frustum_box(origin, voxel, dims, K, hw, Rcw, tcw, near, far):
    """The lattice sub-box (x0, x1, y0, y1, z0, z1), upper ends exclusive, that holds every sample a view can update:
    the samples inside the view frustum between ``near`` and ``far`` (``None``: the volume's farthest corner), computed
    in float64 from the host-side pose, widened by one pixel on the image and by one sample on the lattice so that the
    kernel's float32 arithmetic cannot reach a sample outside it.  Empty (x0 == x1) when the frustum misses the volume."""
    fx, fy, cx, cy = K
    H, W = hw
    R, t = np.asarray(Rcw, np.float64), np.asarray(tcw, np.float64)
    o, n = np.asarray(origin, np.float64), np.asarray(dims, np.int64)
    corners = o + voxel * np.array([[i, j, k] for i in (0, n[0] - 1) for j in (0, n[1] - 1) for k in (0, n[2] - 1)], np.float64)
    zmax = float((corners @ R[2] + t[2]).max())
    slack = 1e-4 * (abs(zmax) + float(np.abs(t).max()) + voxel)      # float32 against float64 on p_c.z
    far = zmax if far is None else min(float(far), zmax)
    far += slack
    lo_z = max(float(near) - slack, 0.0)
    if not far > lo_z:
        return (0, 0, 0, 0, 0, 0)
    pts = []
    for z in (lo_z, far):
        for u in (-1.5, W + 0.5):
            for v in (-1.5, H + 0.5):
                pc = np.array([(u - cx) / fx * z, (v - cy) / fy * z, z])
                pts.append(R.T @ (pc - t))
    pts = np.array(pts)
    lo = np.floor((pts.min(0) - o) / voxel).astype(np.int64) - 1
    hi = np.ceil((pts.max(0) - o) / voxel).astype(np.int64) + 2
    lo, hi = np.clip(lo, 0, n), np.clip(hi, 0, n)
    if (hi <= lo).any():
        return (0, 0, 0, 0, 0, 0)
    return (int(lo[0]), int(hi[0]), int(lo[1]), int(hi[1]), int(lo[2]), int(hi[2]))


class TSDFVolume:
    """A dense truncated signed distance volume on the GPU: ``dims`` = (nx, ny, nz) samples at ``origin`` +
    ``voxel_size`` (ix, iy, iz) in the world frame.  ``tsdf`` [nz,ny,nx] (1), ``weight`` [nz,ny,nx] (0) and, with
    ``color``, ``color`` [3,nz,ny,nx] (0) are plain torch tensors.  ``trunc`` defaults to 4 voxels (untuned)."""

    def __init__(self, origin, voxel_size, dims, trunc=None, color=True, device="cuda"):
        try:
            self.origin = tuple(float(v) for v in origin)
            self.dims = tuple(int(v) for v in dims)
            self.voxel_size = float(voxel_size)
        except (TypeError, ValueError):
            raise ValueError("origin, voxel_size, dims must be three numbers, a number and three integers") from None
        if len(self.origin) != 3 or not all(math.isfinite(v) for v in self.origin):
            raise ValueError("origin must be three finite numbers, got %r" % (origin,))
        if not (math.isfinite(self.voxel_size) and self.voxel_size > 0):
            raise ValueError("voxel_size must be finite and > 0, got %r" % (voxel_size,))
        if len(self.dims) != 3 or min(self.dims) < 1:
            raise ValueError("dims must be three positive integers (nx, ny, nz), got %r" % (dims,))
        if self.dims[0] * self.dims[1] * self.dims[2] > _tsdflib.MAX_SAMPLES:
            raise ValueError("dims %r: the volume takes fewer than 2^31 samples" % (self.dims,))
        self.trunc = TRUNC_VOXELS * self.voxel_size if trunc is None else float(trunc)
        if not (math.isfinite(self.trunc) and self.trunc > 0):
            raise ValueError("trunc must be finite and > 0, got %r" % (trunc,))
        nx, ny, nz = self.dims
        self.device = torch.device(device)
        self.tsdf = torch.ones((nz, ny, nx), dtype=torch.float32, device=self.device)
        self.weight = torch.zeros((nz, ny, nx), dtype=torch.float32, device=self.device)
        self.color = torch.zeros((3, nz, ny, nx), dtype=torch.float32, device=self.device) if color else None
        self.last_box = None

    def integrate(self, depth, alpha, cam, image=None, weight=None, alpha_min=ALPHA_MIN, near=0.01, depth_max=None,
                  clip_to_frustum=True):
        """Fuse one view.  ``depth`` [1,H,W] or [H,W] float32 and ``alpha`` likewise are the render's maps; ``alpha`` =
        None: ``depth`` is metric z (a sensor, a prior).  ``cam``: a camera with fx, fy, cx, cy, Rcw, tcw
        (``function.Camera`` or ``scene.Camera``).  ``image`` [3,H,W]: the colours, needed iff the volume has a colour
        plane; ``weight`` [H,W] >= 0 or None.  ``clip_to_frustum``: launch on the lattice sub-box the view can reach
        (``frustum_box``; the same bits as the full launch).  Shapes, dtypes and devices are checked (ValueError), values
        are not.  Nothing is read back."""
        d = _plane(depth, "depth")
        H, W = int(d.shape[0]), int(d.shape[1])
        a = None if alpha is None else _plane(alpha, "alpha", (H, W), d)
        w = None if weight is None else _plane(weight, "weight", (H, W), d)
        if (image is None) != (self.color is None):
            raise ValueError("image must be given iff the volume has a colour plane (color=%s)" % (self.color is not None))
        img = None if image is None else _planes3(image, "image", (H, W), d)
        K = _intrinsics(cam)
        alpha_min, near = float(alpha_min), float(near)
        if not 0.0 <= alpha_min < float("inf"):
            raise ValueError("alpha_min must be finite and >= 0, got %r" % (alpha_min,))
        if not 0.0 <= near < float("inf"):
            raise ValueError("near must be finite and >= 0, got %r" % (near,))
        if depth_max is not None and not float(depth_max) > 0:
            raise ValueError("depth_max must be > 0 or None, got %r" % (depth_max,))
        if not (hasattr(cam, "Rcw") and hasattr(cam, "tcw")):
            raise ValueError("cam must carry its pose Rcw, tcw, got %r" % (cam,))
        if d.device != self.tsdf.device:
            raise ValueError("depth lives on %s, the volume on %s" % (d.device, self.tsdf.device))
        if not d.is_cuda:
            raise ValueError("depth must live on the GPU (got device %s)" % (d.device,))
        _lib_on(d)
        lib = _tsdflib.load()
        as_dev = lambda p: (p if isinstance(p, torch.Tensor) else torch.as_tensor(np.asarray(p, np.float32))) \
            .detach().to(device=d.device, dtype=torch.float32).contiguous()
        Rcw, tcw = as_dev(cam.Rcw).reshape(-1), as_dev(cam.tcw).reshape(-1)
        if Rcw.numel() != 9 or tcw.numel() != 3:
            raise ValueError("cam.Rcw must have 9 entries and cam.tcw 3")
        nx, ny, nz = self.dims
        box = (0, nx, 0, ny, 0, nz)
        if clip_to_frustum:
            hR, ht = _host_pose(cam)
            far = None if depth_max is None or not math.isfinite(float(depth_max)) else float(depth_max) + self.trunc
            box = frustum_box(self.origin, self.voxel_size, self.dims, K, (H, W), hR, ht, near, far)
        self.last_box = box
        d, a, w, img = (None if t is None else t.contiguous() for t in (d, a, w, img))
        _tsdflib.check(lib.egs_tsdf_integrate(
            nx, ny, nz, *self.origin, self.voxel_size, *box, _ptr(self.tsdf), _ptr(self.weight), _ptr(self.color), H, W,
            _ptr(d), _ptr(a), _ptr(img), _ptr(w), *K, _ptr(Rcw), _ptr(tcw), self.trunc, alpha_min, near,
            float("inf") if depth_max is None else float(depth_max), 0, _stream()))
        return self

    def extract_triangles(self, min_weight=MIN_WEIGHT):
        """-> (verts [T,3,3] float32, keys [T,3] int64, colors [T,3,3] float32 or None): the triangle soup of the zero
        level set, in cell order, every vertex with the key of its lattice edge"""
        min_weight = float(min_weight)
        if not (math.isfinite(min_weight) and min_weight > 0):
            raise ValueError("min_weight must be finite and > 0, got %r" % (min_weight,))
        dev = self.tsdf.device
        if not self.tsdf.is_cuda:
            raise ValueError("the volume must live on the GPU (got device %s)" % (dev,))
        _lib_on(self.tsdf)
        lib = _tsdflib.load()
        nx, ny, nz = self.dims
        cells = (nx - 1) * (ny - 1) * (nz - 1)
        total = 0
        if cells > 0:
            counts = torch.empty(cells, dtype=torch.int32, device=dev)
            _tsdflib.check(lib.egs_tsdf_mesh_count(nx, ny, nz, _ptr(self.tsdf), _ptr(self.weight), min_weight,
                                                   _ptr(counts), _stream()))
            ends = torch.cumsum(counts, 0, dtype=torch.int64)
            offsets = (ends - counts).contiguous()
            total = int(ends[-1])          # the one readback of an extraction
            if total > _tsdflib.MAX_SAMPLES:
                raise ValueError("the mesh has %d triangles, more than 2^31 - 1" % total)
        verts = torch.empty((total, 3, 3), dtype=torch.float32, device=dev)
        keys = torch.empty((total, 3), dtype=torch.int64, device=dev)
        colors = torch.empty((total, 3, 3), dtype=torch.float32, device=dev) if self.color is not None else None
        if total > 0:
            _tsdflib.check(lib.egs_tsdf_mesh_emit(nx, ny, nz, *self.origin, self.voxel_size, _ptr(self.tsdf),
                                                  _ptr(self.weight), _ptr(self.color), min_weight, _ptr(offsets), total,
                                                  total, _ptr(verts), _ptr(keys), _ptr(colors), _stream()))
        return verts, keys, colors

    def extract(self, min_weight=MIN_WEIGHT):
        """-> (vertices [V,3] float32, faces [F,3] int64, colors [V,3] float32 or None): the zero level set as an indexed
        mesh.  A cell is meshed when all its corners have weight >= ``min_weight`` (1 by default, untuned).  Vertices on
        the same lattice edge are welded by their key; their coordinates are identical, any occurrence gives them.
        Outward orientation: a face's normal points from negative to positive tsdf, towards the cameras."""
        verts, keys, colors = self.extract_triangles(min_weight)
        uniq, inverse = torch.unique(keys.reshape(-1), return_inverse=True)
        faces = inverse.reshape(-1, 3)
        V = torch.empty((uniq.shape[0], 3), dtype=torch.float32, device=verts.device)
        V[inverse] = verts.reshape(-1, 3)          # (duplicates hold the same bits: whichever lands is right)
        C = None
        if colors is not None:
            C = torch.empty((uniq.shape[0], 3), dtype=torch.float32, device=verts.device)
            C[inverse] = colors.reshape(-1, 3)
        return V, faces, C


# ------------------------------------------------------------------------------------------------------------ PLY files
def _np(t, dtype):
    return np.ascontiguousarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, dtype)


def save_mesh_ply(path, vertices, faces, colors=None):
    """Binary little-endian PLY of an indexed triangle mesh: vertices [V,3] float32, faces [F,3] integers, optional
    colors [V,3] in [0, 1] written as uchar red green blue.  numpy alone, no ``plyfile``."""
    v, f = _np(vertices, np.float32), _np(faces, np.int64)
    if v.ndim != 2 or v.shape[1] != 3:
        raise ValueError("vertices must have shape [V, 3], got %s" % (list(v.shape),))
    if f.ndim != 2 or f.shape[1] != 3:
        raise ValueError("faces must have shape [F, 3], got %s" % (list(f.shape),))
    if f.size and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError("faces index %d vertices, found an index outside" % len(v))
    if len(v) >= 1 << 31:
        raise ValueError("a PLY face list holds int32 indices")
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    head = ["ply", "format binary_little_endian 1.0", "element vertex %d" % len(v), "property float x",
            "property float y", "property float z"]
    if colors is not None:
        c = _np(colors, np.float32)
        if c.shape != v.shape:
            raise ValueError("colors must have shape %s, got %s" % (list(v.shape), list(c.shape)))
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        head += ["property uchar red", "property uchar green", "property uchar blue"]
    head += ["element face %d" % len(f), "property list uchar int vertex_indices", "end_header"]
    vrec = np.empty(len(v), dtype=fields)
    vrec["x"], vrec["y"], vrec["z"] = v[:, 0], v[:, 1], v[:, 2]
    if colors is not None:
        c8 = np.clip(np.rint(np.nan_to_num(c) * 255.0), 0, 255).astype(np.uint8)
        vrec["red"], vrec["green"], vrec["blue"] = c8[:, 0], c8[:, 1], c8[:, 2]
    frec = np.empty(len(f), dtype=[("n", "u1"), ("i", "<i4", (3,))])
    frec["n"] = 3
    frec["i"] = f
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode("ascii"))
        fh.write(vrec.tobytes())
        fh.write(frec.tobytes())


def load_mesh_ply(path):
    """-> (vertices [V,3] float32, faces [F,3] int64, colors [V,3] float32 in [0, 1] or None) numpy arrays of a file
    ``save_mesh_ply`` wrote (binary little-endian, float x y z, optional uchar red green blue, triangles as
    ``uchar int`` lists)."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.find(b"end_header\n")
    if not data.startswith(b"ply\n") or end < 0:
        raise ValueError("%s is not a PLY file" % path)
    lines = data[:end].decode("ascii").split("\n")
    if "format binary_little_endian 1.0" not in lines:
        raise ValueError("%s: only binary little-endian PLY is read" % path)
    nv = nf = None
    props = {"vertex": [], "face": []}
    element = None
    for ln in lines:
        p = ln.split()
        if p[:1] == ["element"]:
            element = p[1]
            if element == "vertex":
                nv = int(p[2])
            elif element == "face":
                nf = int(p[2])
        elif p[:1] == ["property"] and element in props:
            props[element].append(p[1:])
    names = [p[-1] for p in props["vertex"]]
    has_color = names == ["x", "y", "z", "red", "green", "blue"]
    if nv is None or nf is None or not (names == ["x", "y", "z"] or has_color) or \
            props["face"] != [["list", "uchar", "int", "vertex_indices"]]:
        raise ValueError("%s: not the layout save_mesh_ply writes" % path)
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")] + ([("red", "u1"), ("green", "u1"), ("blue", "u1")] if has_color else [])
    body = end + len(b"end_header\n")
    vrec = np.frombuffer(data, dtype=fields, count=nv, offset=body)
    frec = np.frombuffer(data, dtype=[("n", "u1"), ("i", "<i4", (3,))], count=nf, offset=body + vrec.nbytes)
    if nf and not (frec["n"] == 3).all():
        raise ValueError("%s: a face that is not a triangle" % path)
    v = np.stack([vrec["x"], vrec["y"], vrec["z"]], 1).astype(np.float32)
    c = np.stack([vrec["red"], vrec["green"], vrec["blue"]], 1).astype(np.float32) / np.float32(255) if has_color else None
    return v, frec["i"].astype(np.int64), c
