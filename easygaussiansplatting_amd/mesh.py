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

A TSDF of splat depth maps carries floaters.  The mesh is cleaned where it already lives, on the GPU (DESIGN §3.20,
csrc/egs_meshops.hip, libegs_meshops.so; include/egs_meshops.h has every rule): ``connected_components`` (a lock-free
union-find over vertex connectivity), ``remove_small_components`` (by face count and/or the k largest, with compaction),
``vertex_normals`` (area weighted, outward), ``smooth_taubin`` and ``clean_mesh``, which chains them.  All of it is
deterministic bit for bit.  ``lam`` = 0.5, ``mu`` = -0.53 and 10 iterations of the smoothing are Taubin's and Open3D's
defaults, which nobody has tuned here either.

    V, F, C, N = clean_mesh(*vol.extract(), min_faces=200, normals=True)
    save_mesh_ply_with_normals("mesh.ply", V, F, C, N)

Marching tetrahedra on a 256^3 lattice leave about 0.9 M triangles for one object.  ``simplify_vertex_clustering`` (DESIGN
§3.21, csrc/egs_simplify.hip, libegs_simplify.so; include/egs_simplify.h has every rule) decimates the mesh on the GPU:
every cell of a uniform grid becomes one vertex, placed where it minimises the squared distance to the planes of the faces
that touched the cell (Lindstrom's scheme, Open3D's ``simplify_vertex_clustering`` with ``Quadric`` contraction); collapsed
and duplicate faces are dropped.  Deterministic bit for bit like the rest.  The regulariser of the placement, 1e-3, is
untuned: nobody has tuned it here.  Vertex clustering does NOT preserve topology: a closed manifold may come out with a few
opposite face pairs and another Euler characteristic.  ``clean_mesh(..., simplify_cell=...)`` runs it between the smoothing
and the normals.

A dense volume costs what its bounding box costs.  ``SparseTSDFVolume`` (csrc/egs_sparsetsdf.hip,
libegs_sparsetsdf.so; include/egs_sparse_tsdf.h has every rule) stores and updates only the 8^3-sample blocks within the
truncation band of an observed surface: the same arithmetic on the same lattice (both volumes call csrc/egs_tsdf_device.h),
the same vertex keys, so everything after ``extract()`` is unchanged.  A block is updated only from the view that allocates
it onwards, and a cell is meshed only when all eight corners are allocated.

    vol = SparseTSDFVolume(origin=(-1, -1, -1), voxel_size=2 / 1023, dims=(1024, 1024, 1024))
"""
from __future__ import annotations

import collections
import math

import numpy as np
import torch

from . import _meshopslib, _simplifylib, _sparsetsdflib, _tsdflib
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


def _weld(verts, keys, colors):
    """a triangle soup with vertex keys -> (vertices [V,3], faces [F,3] int64, colors [V,3] or None), welded by key"""
    uniq, inverse = torch.unique(keys.reshape(-1), return_inverse=True)
    faces = inverse.reshape(-1, 3)
    V = torch.empty((uniq.shape[0], 3), dtype=torch.float32, device=verts.device)
    V[inverse] = verts.reshape(-1, 3)          # (duplicates hold the same bits: whichever lands is right)
    C = None
    if colors is not None:
        C = torch.empty((uniq.shape[0], 3), dtype=torch.float32, device=verts.device)
        C[inverse] = colors.reshape(-1, 3)
    return V, faces, C


def _view_args(has_color, device, depth, alpha, cam, image, weight, alpha_min, near, depth_max):
    """The checks ``TSDFVolume.integrate`` and ``SparseTSDFVolume.integrate`` share -> (d, a, w, img, K, alpha_min, near,
    Rcw, tcw): the maps as planes, the intrinsics, the pose as device tensors"""
    d = _plane(depth, "depth")
    H, W = int(d.shape[0]), int(d.shape[1])
    a = None if alpha is None else _plane(alpha, "alpha", (H, W), d)
    w = None if weight is None else _plane(weight, "weight", (H, W), d)
    if (image is None) != (not has_color):
        raise ValueError("image must be given iff the volume has a colour plane (color=%s)" % (has_color))
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
    if d.device != device:
        raise ValueError("depth lives on %s, the volume on %s" % (d.device, device))
    if not d.is_cuda:
        raise ValueError("depth must live on the GPU (got device %s)" % (d.device,))
    _lib_on(d)
    as_dev = lambda p: (p if isinstance(p, torch.Tensor) else torch.as_tensor(np.asarray(p, np.float32))) \
        .detach().to(device=d.device, dtype=torch.float32).contiguous()
    Rcw, tcw = as_dev(cam.Rcw).reshape(-1), as_dev(cam.tcw).reshape(-1)
    if Rcw.numel() != 9 or tcw.numel() != 3:
        raise ValueError("cam.Rcw must have 9 entries and cam.tcw 3")
    return d, a, w, img, K, alpha_min, near, Rcw, tcw


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
        d, a, w, img, K, alpha_min, near, Rcw, tcw = _view_args(self.color is not None, self.tsdf.device, depth, alpha, cam,
                                                                image, weight, alpha_min, near, depth_max)
        H, W = int(d.shape[0]), int(d.shape[1])
        lib = _tsdflib.load()
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
        return _weld(*self.extract_triangles(min_weight))


# ------------------------------------------------------------------------------------------------------ the sparse volume
SPARSE_FIRST_CAPACITY = 1024      # pool slots before the first doubling


class SparseTSDFVolume:
    """A block-allocated truncated signed distance volume on the GPU (csrc/egs_sparsetsdf.hip,
    libegs_sparsetsdf.so; include/egs_sparse_tsdf.h has every rule): the lattice of ``TSDFVolume`` -- ``dims`` = (nx, ny,
    nz) samples at ``origin`` + ``voxel_size`` (ix, iy, iz) -- of which only the 8 x 8 x 8-sample blocks within the
    truncation band of an observed surface are stored, so the cost follows the surface and not the bounding box, and the
    lattice may have 2^31 samples and more (at most 2^27 blocks; at most 2^22 of them allocated).

    ``directory`` [nbz,nby,nbx] int32 holds -1 or a block's pool slot, ``block_coords`` [capacity] int32 the linear block
    index of each slot, ``tsdf`` and ``weight`` [capacity,512] and ``color`` [3,capacity,512] the pools (x fastest within
    a block); slots 0 .. ``n_blocks`` - 1 are in use.  The pool grows by doubling; ``max_blocks`` caps it.

    SEMANTICS.  Every sample of an allocated block takes the bits ``TSDFVolume`` gives it from the same previous bits
    (both call the functions of csrc/egs_tsdf_device.h), but a block is updated only FROM THE VIEW THAT ALLOCATES IT
    onwards: free-space observations (t = 1) that earlier views made of its samples are not recorded.  A cell is meshed
    only when all eight of its corners lie in allocated blocks (and have weight >= ``min_weight``); its triangles, vertex
    keys and colours are then the dense volume's."""

    def __init__(self, origin, voxel_size, dims, trunc=None, color=True, max_blocks=None, device="cuda"):
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
        if len(self.dims) != 3 or min(self.dims) < 1 or max(self.dims) > _tsdflib.MAX_SAMPLES:
            raise ValueError("dims must be three positive integers (nx, ny, nz), got %r" % (dims,))
        B = _sparsetsdflib.BLOCK
        self.block_dims = tuple((n + B - 1) // B for n in self.dims)
        total = self.block_dims[0] * self.block_dims[1] * self.block_dims[2]
        if total > _sparsetsdflib.MAX_DIRECTORY:
            raise ValueError("dims %r: %d blocks, the directory takes at most 2^27" % (self.dims, total))
        self.trunc = TRUNC_VOXELS * self.voxel_size if trunc is None else float(trunc)
        if not (math.isfinite(self.trunc) and self.trunc > 0):
            raise ValueError("trunc must be finite and > 0, got %r" % (trunc,))
        if 2.0 * self.trunc > _sparsetsdflib.MAX_MARCH * self.voxel_size:
            raise ValueError("trunc must not exceed %d voxels, got %r" % (_sparsetsdflib.MAX_MARCH // 2, trunc))
        self.limit = min(total, _sparsetsdflib.MAX_SLOTS)
        if max_blocks is not None:
            if int(max_blocks) != max_blocks or int(max_blocks) < 1:
                raise ValueError("max_blocks must be a positive integer or None, got %r" % (max_blocks,))
            self.limit = min(self.limit, int(max_blocks))
        self.max_blocks = None if max_blocks is None else int(max_blocks)
        self.device = torch.device(device)
        self.has_color = bool(color)
        nbx, nby, nbz = self.block_dims
        self.directory = torch.full((nbz, nby, nbx), -1, dtype=torch.int32, device=self.device)
        self.n_blocks = 0
        self._allocate_pool(min(self.limit, SPARSE_FIRST_CAPACITY))

    # ---- the pool
    def _allocate_pool(self, capacity):
        """new pools of ``capacity`` slots holding 1 / 0 / 0, the slots in use copied over"""
        S, dev, n = _sparsetsdflib.BLOCK_SAMPLES, self.device, self.n_blocks
        coords = torch.full((capacity,), -1, dtype=torch.int32, device=dev)
        tsdf = torch.ones((capacity, S), dtype=torch.float32, device=dev)
        weight = torch.zeros((capacity, S), dtype=torch.float32, device=dev)
        color = torch.zeros((3, capacity, S), dtype=torch.float32, device=dev) if self.has_color else None
        if n > 0:
            coords[:n] = self.block_coords[:n]
            tsdf[:n] = self.tsdf[:n]
            weight[:n] = self.weight[:n]
            if color is not None:
                color[:, :n] = self.color[:, :n]
        self.block_coords, self.tsdf, self.weight, self.color, self.capacity = coords, tsdf, weight, color, capacity

    def _geometry(self):
        return (*self.dims, *self.origin, self.voxel_size)

    def integrate(self, depth, alpha, cam, image=None, weight=None, alpha_min=ALPHA_MIN, near=0.01, depth_max=None,
                  clip_to_frustum=True, grid_cap=0):
        """Fuse one view: the arguments of ``TSDFVolume.integrate`` (``clip_to_frustum`` is accepted and has nothing to
        do: only allocated blocks are walked).  First the blocks the view's truncation band meets, dilated by one block,
        are allocated -- ONE integer, the number of new blocks, is read back -- then the view is fused into every
        allocated block.  ``max_blocks`` exceeded: ValueError, and the volume is left as it was.  ``grid_cap``: a cap on
        the workgroups of the fusion (the ABI's ``max_blocks``; the same bits)."""
        d, a, w, img, K, alpha_min, near, Rcw, tcw = _view_args(self.has_color, self.tsdf.device, depth, alpha, cam, image,
                                                                weight, alpha_min, near, depth_max)
        H, W = int(d.shape[0]), int(d.shape[1])
        lib = _sparsetsdflib.load()
        chk = _sparsetsdflib.check
        d, a, w, img = (None if t is None else t.contiguous() for t in (d, a, w, img))
        dmax = float("inf") if depth_max is None else float(depth_max)
        nx, ny, nz = self.dims
        dev = self.tsdf.device
        flags = torch.zeros(self.directory.shape, dtype=torch.int32, device=dev)
        chk(lib.egs_sparsetsdf_touch(*self._geometry(), H, W, _ptr(d), _ptr(a), _ptr(w), *K, _ptr(Rcw), _ptr(tcw),
                                     self.trunc, alpha_min, near, dmax, _ptr(flags), _stream()))
        fresh = torch.empty(self.directory.shape, dtype=torch.int32, device=dev)
        chk(lib.egs_sparsetsdf_mark(nx, ny, nz, _ptr(flags), _ptr(self.directory), _ptr(fresh), _stream()))
        fresh = fresh.reshape(-1)
        ends = torch.cumsum(fresh, 0, dtype=torch.int64)
        new = int(ends[-1])                # the one readback of a view
        if self.n_blocks + new > self.limit:
            raise ValueError("the view needs %d new blocks beside the %d allocated: more than %s"
                             % (new, self.n_blocks, "max_blocks = %d" % self.max_blocks if self.limit == self.max_blocks
                                else "the volume's limit of %d" % self.limit))
        if new > 0:
            if self.n_blocks + new > self.capacity:
                self._allocate_pool(min(self.limit, max(2 * self.capacity, self.n_blocks + new)))
            offsets = (ends - fresh).contiguous()
            chk(lib.egs_sparsetsdf_assign(nx, ny, nz, _ptr(fresh), _ptr(offsets), self.n_blocks, self.capacity,
                                          _ptr(self.directory), _ptr(self.block_coords), _stream()))
            self.n_blocks += new
        chk(lib.egs_sparsetsdf_integrate(*self._geometry(), self.n_blocks, self.capacity, _ptr(self.block_coords),
                                         _ptr(self.tsdf), _ptr(self.weight), _ptr(self.color), H, W, _ptr(d), _ptr(a),
                                         _ptr(img), _ptr(w), *K, _ptr(Rcw), _ptr(tcw), self.trunc, alpha_min, near, dmax,
                                         int(grid_cap), _stream()))
        return self

    def extract_triangles(self, min_weight=MIN_WEIGHT):
        """-> (verts [T,3,3] float32, keys [T,3] int64, colors [T,3,3] float32 or None): the triangle soup of the zero
        level set by slot, then by the cell within the block; the keys are the dense volume's"""
        min_weight = float(min_weight)
        if not (math.isfinite(min_weight) and min_weight > 0):
            raise ValueError("min_weight must be finite and > 0, got %r" % (min_weight,))
        dev = self.tsdf.device
        if not self.tsdf.is_cuda:
            raise ValueError("the volume must live on the GPU (got device %s)" % (dev,))
        _lib_on(self.tsdf)
        lib = _sparsetsdflib.load()
        nx, ny, nz = self.dims
        n, total = self.n_blocks, 0
        if n > 0:
            counts = torch.empty(n * _sparsetsdflib.BLOCK_SAMPLES, dtype=torch.int32, device=dev)
            _sparsetsdflib.check(lib.egs_sparsetsdf_mesh_count(nx, ny, nz, n, self.capacity, _ptr(self.directory),
                                                               _ptr(self.block_coords), _ptr(self.tsdf),
                                                               _ptr(self.weight), min_weight, _ptr(counts), _stream()))
            ends = torch.cumsum(counts, 0, dtype=torch.int64)
            offsets = (ends - counts).contiguous()
            total = int(ends[-1])          # the one readback of an extraction
            if total > _tsdflib.MAX_SAMPLES:
                raise ValueError("the mesh has %d triangles, more than 2^31 - 1" % total)
        verts = torch.empty((total, 3, 3), dtype=torch.float32, device=dev)
        keys = torch.empty((total, 3), dtype=torch.int64, device=dev)
        colors = torch.empty((total, 3, 3), dtype=torch.float32, device=dev) if self.color is not None else None
        if total > 0:
            _sparsetsdflib.check(lib.egs_sparsetsdf_mesh_emit(*self._geometry(), n, self.capacity, _ptr(self.directory),
                                                              _ptr(self.block_coords), _ptr(self.tsdf), _ptr(self.weight),
                                                              _ptr(self.color), min_weight, _ptr(offsets), total, total,
                                                              _ptr(verts), _ptr(keys), _ptr(colors), _stream()))
        return verts, keys, colors

    def extract(self, min_weight=MIN_WEIGHT):
        """-> (vertices [V,3] float32, faces [F,3] int64, colors [V,3] float32 or None), welded by key as
        ``TSDFVolume.extract`` does.  A cell is meshed when all eight corners lie in allocated blocks with weight >=
        ``min_weight``: the surface ends where the allocation ends."""
        return _weld(*self.extract_triangles(min_weight))

    # ---- to and from a dense volume (plain indexing)
    def to_dense(self):
        """-> a ``TSDFVolume`` with the allocated blocks' samples and 1 / 0 / 0 elsewhere; it takes fewer than 2^31
        samples like every dense volume"""
        vol = TSDFVolume(self.origin, self.voxel_size, self.dims, trunc=self.trunc, color=self.has_color,
                         device=self.device)
        B = _sparsetsdflib.BLOCK
        nx, ny, nz = self.dims
        nbx, nby, nbz = self.block_dims
        n = self.n_blocks
        b = self.block_coords[:n].long()

        def scatter(pool, fill):
            blocks = torch.full((nbz * nby * nbx, B, B, B), fill, dtype=torch.float32, device=self.device)
            blocks[b] = pool[:n].reshape(n, B, B, B)
            full = blocks.reshape(nbz, nby, nbx, B, B, B).permute(0, 3, 1, 4, 2, 5).reshape(nbz * B, nby * B, nbx * B)
            return full[:nz, :ny, :nx].contiguous()

        vol.tsdf, vol.weight = scatter(self.tsdf, 1.0), scatter(self.weight, 0.0)
        if self.has_color:
            vol.color = torch.stack([scatter(self.color[c], 0.0) for c in range(3)])
        return vol

    @classmethod
    def from_dense(cls, volume, block_mask):
        """A sparse volume holding the blocks of the dense ``volume`` that ``block_mask`` [nbz,nby,nbx] (bool) selects,
        slots in ascending block index"""
        B = _sparsetsdflib.BLOCK
        self = cls(volume.origin, volume.voxel_size, volume.dims, trunc=volume.trunc, color=volume.color is not None,
                   device=volume.tsdf.device)
        nbx, nby, nbz = self.block_dims
        mask = torch.as_tensor(block_mask, device=self.device)
        if mask.dtype != torch.bool or tuple(mask.shape) != (nbz, nby, nbx):
            raise ValueError("block_mask must be a bool tensor of shape %s, got %s %s"
                             % ([nbz, nby, nbx], mask.dtype, list(mask.shape)))
        b = torch.nonzero(mask.reshape(-1)).reshape(-1)
        n = int(b.shape[0])
        if n > self.limit:
            raise ValueError("block_mask selects %d blocks, the volume's limit is %d" % (n, self.limit))
        nx, ny, nz = self.dims

        def gather(plane, fill):
            full = torch.full((nbz * B, nby * B, nbx * B), fill, dtype=torch.float32, device=self.device)
            full[:nz, :ny, :nx] = plane
            blocks = full.reshape(nbz, B, nby, B, nbx, B).permute(0, 2, 4, 1, 3, 5).reshape(nbz * nby * nbx, B * B * B)
            return blocks[b]

        self.n_blocks = 0
        self._allocate_pool(max(n, 1))
        self.n_blocks = n
        if n > 0:
            self.block_coords[:n] = b.to(torch.int32)
            self.directory.reshape(-1)[b] = torch.arange(n, dtype=torch.int32, device=self.device)
            self.tsdf[:n], self.weight[:n] = gather(volume.tsdf, 1.0), gather(volume.weight, 0.0)
            if self.has_color:
                for c in range(3):
                    self.color[c, :n] = gather(volume.color[c], 0.0)
        return self


# -------------------------------------------------------------------------------------------------------- mesh cleaning
TAUBIN_LAMBDA = 0.5       # Taubin's pair, Open3D's defaults; untuned here
TAUBIN_MU = -0.53
TAUBIN_ITERATIONS = 10

Components = collections.namedtuple("Components", ["label", "comp_faces", "comp_verts"])


def _count(value, name, minimum=0):
    try:
        ok = int(value) == value and int(value) >= minimum
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok or int(value) > _meshopslib.MAX_COUNT:
        raise ValueError("%s must be an integer in [%d, 2^31), got %r" % (name, minimum, value))
    return int(value)


def _faces(faces, n_vertices, check):
    """``faces`` as a contiguous [F,3] int64 tensor on the GPU; with ``check`` one ``aminmax`` (a readback) makes sure every
    index lies in [0, n_vertices)"""
    if not isinstance(faces, torch.Tensor):
        raise TypeError("faces must be a torch.Tensor, got %s" % type(faces).__name__)
    if faces.dtype != torch.int64:
        raise ValueError("faces must be torch.int64, got %s" % (faces.dtype,))
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError("faces must have shape [F, 3], got %s" % (list(faces.shape),))
    if faces.shape[0] > _meshopslib.MAX_COUNT:
        raise ValueError("a mesh takes fewer than 2^31 faces, got %d" % faces.shape[0])
    if not faces.is_cuda:
        raise ValueError("faces must live on the GPU (got device %s)" % (faces.device,))
    f = faces.detach().contiguous()
    if check and f.shape[0] > 0:
        lo, hi = torch.stack(torch.aminmax(f)).tolist()
        if lo < 0 or hi >= n_vertices:
            raise ValueError("faces index %d vertices, found an index outside (min %d, max %d)" % (n_vertices, lo, hi))
    return f


def _rows3(t, name, like=None):
    """``t`` as a contiguous [V,3] float32 tensor, with the shape and device of ``like`` if given"""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor, got %s" % (name, type(t).__name__))
    if t.dtype != torch.float32:
        raise ValueError("%s must be torch.float32, got %s" % (name, t.dtype))
    if t.dim() != 2 or t.shape[1] != 3 or (like is not None and t.shape[0] != like.shape[0]):
        raise ValueError("%s must have shape [%s, 3], got %s" % (name, "V" if like is None else like.shape[0],
                                                                 list(t.shape)))
    if t.shape[0] > _meshopslib.MAX_COUNT:
        raise ValueError("a mesh takes fewer than 2^31 vertices, got %d" % t.shape[0])
    if like is not None and t.device != like.device:
        raise ValueError("%s lives on %s, vertices on %s" % (name, t.device, like.device))
    return t.detach().contiguous()


def _mesh_args(vertices, faces, check):
    v = _rows3(vertices, "vertices")
    f = _faces(faces, v.shape[0], check)
    if f.device != v.device:
        raise ValueError("faces live on %s, vertices on %s" % (f.device, v.device))
    _lib_on(v)
    return v, f


def _incidence(f, n_vertices):
    """the vertex-to-face incidence in CSR form (include/egs_meshops.h): -> (row_start [V+1] int64, rows [3F] int64), the
    entries 3 f + k of a vertex in ascending order: a stable sort of the flattened faces"""
    flat = f.reshape(-1)
    keys, rows = torch.sort(flat, stable=True)
    row_start = torch.searchsorted(keys, torch.arange(n_vertices + 1, dtype=torch.int64, device=f.device))
    return row_start.contiguous(), rows.contiguous()


def connected_components(faces, n_vertices, check=True):
    """-> Components(label, comp_faces, comp_verts), three [n_vertices] int32 tensors on the device.  Two vertices are
    connected when a face holds both (vertex connectivity).  ``label[v]`` is the smallest vertex index of v's component;
    ``comp_faces[r]`` and ``comp_verts[r]`` are the numbers of faces and vertices of the component whose representative
    (``label[r] == r``) is r, and 0 at every other index.  A face belongs to the component of its first vertex; a vertex
    no face names is a component without a face.  A lock-free union-find and integer sums: the same bits on every run.
    ``check`` = False skips the index-range test (one ``aminmax`` readback); the kernels skip a face with an index
    outside [0, n_vertices) either way."""
    n = _count(n_vertices, "n_vertices")
    f = _faces(faces, n, check)
    _lib_on(f)
    lib = _meshopslib.load()
    out = [torch.empty(n, dtype=torch.int32, device=f.device) for _ in range(3)]
    _meshopslib.check(lib.egs_meshops_components(n, f.shape[0], _ptr(f), _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), 0,
                                                 _stream()))
    return Components(*out)


def remove_small_components(vertices, faces, colors=None, min_faces=None, keep_largest=None, normals=None, check=True):
    """-> (vertices', faces', colors' or None, normals' or None) without the small components.  A component is kept when it
    has at least ``min_faces`` faces (if given) and is among the ``keep_largest`` components with the most faces (if
    given; ties go to the smaller label, i.e. the smaller first vertex index); at least one of the two must be given.
    Components without a face are always dropped, which removes unreferenced vertices.  Kept vertices and faces keep
    their relative order, face indices are rewritten, colours and normals travel with their vertices bit for bit,
    degenerate faces are left as they are.  One readback: the two kept counts, in a single copy (and the ``aminmax`` of
    ``check``)."""
    if min_faces is None and keep_largest is None:
        raise ValueError("give min_faces, keep_largest or both")
    min_faces = 0 if min_faces is None else _count(min_faces, "min_faces")
    k = None if keep_largest is None else _count(keep_largest, "keep_largest", 1)
    v, f = _mesh_args(vertices, faces, check)
    c = None if colors is None else _rows3(colors, "colors", v)
    nrm = None if normals is None else _rows3(normals, "normals", v)
    lib = _meshopslib.load()
    dev = v.device
    V, F = v.shape[0], f.shape[0]
    comp = connected_components(f, V, check=False)
    rank = None
    if k is not None:
        order = torch.sort(comp.comp_faces, descending=True, stable=True).indices      # more faces first, then label
        rank = torch.empty(V, dtype=torch.int32, device=dev)
        rank[order] = torch.arange(V, dtype=torch.int32, device=dev)
    vkeep = torch.empty(V, dtype=torch.int32, device=dev)
    fkeep = torch.empty(F, dtype=torch.int32, device=dev)
    _meshopslib.check(lib.egs_meshops_keep_flags(V, F, _ptr(f), _ptr(comp.label), _ptr(comp.comp_faces), _ptr(rank),
                                                 min_faces, 0 if k is None else k, _ptr(vkeep), _ptr(fkeep), 0, _stream()))
    vscan = torch.cumsum(vkeep, 0, dtype=torch.int64)
    fscan = torch.cumsum(fkeep, 0, dtype=torch.int64)
    zero = torch.zeros(1, dtype=torch.int64, device=dev)
    Vk, Fk = torch.cat([vscan[-1:] if V else zero, fscan[-1:] if F else zero]).tolist()      # the one readback
    ov = torch.empty((Vk, 3), dtype=torch.float32, device=dev)
    of = torch.empty((Fk, 3), dtype=torch.int64, device=dev)
    oc = None if c is None else torch.empty((Vk, 3), dtype=torch.float32, device=dev)
    on = None if nrm is None else torch.empty((Vk, 3), dtype=torch.float32, device=dev)
    _meshopslib.check(lib.egs_meshops_compact(V, F, _ptr(v), _ptr(c), _ptr(nrm), _ptr(f), _ptr(vkeep), _ptr(fkeep),
                                              _ptr(vscan), _ptr(fscan), Vk, Fk, _ptr(ov), _ptr(oc), _ptr(on), _ptr(of), 0,
                                              _stream()))
    return ov, of, oc, on


def vertex_normals(vertices, faces, check=True):
    """-> [V,3] float32: the area-weighted vertex normals, S / |S| with S the sum of (b - a) x (c - a) over a vertex's
    faces -- outward for a mesh of ``TSDFVolume.extract``.  Summed in double in (face, corner) order by one thread per
    vertex and rounded once: bitwise reproducible.  (0, 0, 0) where |S| is 0 or not finite or the vertex has no face."""
    v, f = _mesh_args(vertices, faces, check)
    lib = _meshopslib.load()
    row_start, rows = _incidence(f, v.shape[0])
    out = torch.empty_like(v)
    _meshopslib.check(lib.egs_meshops_vertex_normals(v.shape[0], f.shape[0], _ptr(v), _ptr(f), _ptr(row_start), _ptr(rows),
                                                     _ptr(out), 0, _stream()))
    return out


def smooth_taubin(vertices, faces, iterations=TAUBIN_ITERATIONS, lam=TAUBIN_LAMBDA, mu=TAUBIN_MU, check=True):
    """-> the smoothed vertices [V,3] float32; the input is not modified.  Each iteration is a ``lam`` step and a ``mu``
    step of p' = p + s (m - p), m being the face umbrella of p: the mean of q + r over the other two vertices of every
    incident face, halved (the uniform umbrella on a closed manifold; at a boundary interior neighbours weigh double).
    Double sums in (face, corner) order, one rounding per step; a vertex without a face does not move.  ``lam`` = 0.5,
    ``mu`` = -0.53 and 10 iterations are Taubin's and Open3D's defaults, which nobody has tuned here."""
    iterations = _count(iterations, "iterations")
    lam, mu = float(lam), float(mu)
    if not (math.isfinite(lam) and math.isfinite(mu)):
        raise ValueError("lam and mu must be finite, got %r, %r" % (lam, mu))
    v, f = _mesh_args(vertices, faces, check)
    lib = _meshopslib.load()
    row_start, rows = _incidence(f, v.shape[0])
    out = torch.empty_like(v)
    tmp = torch.empty_like(v) if iterations > 0 else None
    _meshopslib.check(lib.egs_meshops_taubin(v.shape[0], f.shape[0], _ptr(v), _ptr(f), _ptr(row_start), _ptr(rows),
                                             iterations, lam, mu, _ptr(out), _ptr(tmp), 0, _stream()))
    return out


PLACEMENTS = {"quadric": _simplifylib.PLACE_QUADRIC, "mean": _simplifylib.PLACE_MEAN}


def _cell_size(value, name="cell_size"):
    try:
        cell = float(value)
    except (TypeError, ValueError):
        cell = float("nan")
    if not (math.isfinite(cell) and cell > 0):
        raise ValueError("%s must be a finite number > 0, got %r" % (name, value))
    return cell


def _placement(value, name="placement"):
    if value not in PLACEMENTS:
        raise ValueError("%s must be 'quadric' or 'mean', got %r" % (name, value))
    return PLACEMENTS[value]


def _origin(value):
    try:
        origin = tuple(float(x) for x in value)
    except (TypeError, ValueError):
        origin = ()
    if len(origin) != 3 or not all(math.isfinite(x) for x in origin):
        raise ValueError("origin must be three finite numbers or None, got %r" % (value,))
    return origin


def simplify_vertex_clustering(vertices, faces, colors=None, cell_size=None, origin=None, placement="quadric", check=True,
                               return_info=False):
    """-> (vertices', faces', colors' or None): vertex-clustering simplification (include/egs_simplify.h has every rule).
    The vertices that fall into one cell of the uniform grid (``origin`` + ``cell_size`` x integers; ``origin`` = None: the
    bounding box minimum) become one vertex.  ``placement`` = "quadric" puts it where it minimises the summed squared
    distance to the planes of the faces that touched the cell (area weighted, regularised towards the cell mean with the
    weight 1e-3 of the quadric's trace -- a value nobody has tuned here -- and clamped to the cell); "mean" takes the mean
    of the cell's vertices.  The colour is the mean.  A face two of whose corners fall into one cell is dropped; of faces on
    the same three cells in the same orientation the first stays (opposite orientations are different faces: both stay);
    cells no kept face names are dropped.  Kept faces keep their order, vertices come in ascending cell key (x fastest).
    Topology is NOT preserved.  Sums in double in a fixed order, no float atomic: the same bits on every run.

    ``check`` makes sure every face index lies in [0, V) (the kernels skip such a face either way).  Vertices must be
    finite, ``origin`` <= the bounding box minimum and the extent below 2^21 cells per axis: ValueError otherwise.
    At most three readbacks: the bounding box (with it the finite check, the 2^21 check and the index check, in one copy),
    the cluster count (``torch.unique``) and the two kept counts in one copy.  ``return_info`` adds a dict -- ``clusters``,
    ``placed_mean``, ``placed_solved``, ``placed_clamped``, ``placed_no_face``, ``faces_degenerate``, ``faces_duplicate`` -- at
    the cost of one more readback."""
    if cell_size is None:
        raise ValueError("cell_size must be a finite number > 0, got None")
    cell = _cell_size(cell_size)
    place = _placement(placement)
    org = None if origin is None else _origin(origin)
    v, f = _mesh_args(vertices, faces, False)
    c = None if colors is None else _rows3(colors, "colors", v)
    dev = v.device
    V, F = v.shape[0], f.shape[0]
    empty = (torch.empty((0, 3), dtype=torch.float32, device=dev), torch.empty((0, 3), dtype=torch.int64, device=dev),
             None if c is None else torch.empty((0, 3), dtype=torch.float32, device=dev))
    info = dict(clusters=0, placed_mean=0, placed_solved=0, placed_clamped=0, placed_no_face=0, faces_degenerate=F,
                faces_duplicate=0)
    if V == 0:
        return empty + (info,) if return_info else empty
    # readback 1: the bounding box, and with check the range of the face indices (exact in double: |index| < 2^53 or refused)
    lo, hi = torch.aminmax(v.double(), dim=0)
    parts = [lo, hi]
    if check and F > 0:
        parts.append(torch.stack(torch.aminmax(f)).clamp(-(1 << 52), 1 << 52).double())
    box = torch.cat(parts).tolist()
    if not all(math.isfinite(x) for x in box[:6]):
        raise ValueError("vertices must be finite (bounding box %r .. %r)" % (box[:3], box[3:6]))
    if len(box) > 6 and (box[6] < 0 or box[7] >= V):
        raise ValueError("faces index %d vertices, found an index outside (min %d, max %d)" % (V, box[6], box[7]))
    if org is None:
        org = tuple(box[:3])
    if any(o > m for o, m in zip(org, box[:3])):
        raise ValueError("origin %r must not exceed the bounding box minimum %r" % (org, tuple(box[:3])))
    if any(math.floor((m - o) / cell) >= (1 << _simplifylib.KEY_BITS) for o, m in zip(org, box[3:6])):
        raise ValueError("cell_size %r: the mesh spans 2^%d cells or more from the origin" % (cell_size, _simplifylib.KEY_BITS))
    lib = _simplifylib.load()
    S = _stream()
    keys = torch.empty(V, dtype=torch.int64, device=dev)
    _simplifylib.check(lib.egs_simplify_keys(V, _ptr(v), *org, cell, _ptr(keys), 0, S))
    uniq, cluster = torch.unique(keys, return_inverse=True)          # readback 2 (torch's): the cluster count
    cluster = cluster.contiguous()
    Vc = uniq.shape[0]
    srt, members = torch.sort(cluster, stable=True)                    # members in ascending vertex index
    member_start = torch.searchsorted(srt, torch.arange(Vc + 1, dtype=torch.int64, device=dev)).contiguous()
    members = members.contiguous()
    quadrics = None
    if place == _simplifylib.PLACE_QUADRIC:                            # the two-pass form: per-vertex partials first
        row_start, rows = _incidence(f, V) if F > 0 else (None, None)
        quadrics = torch.empty((V, 9), dtype=torch.float64, device=dev)
        _simplifylib.check(lib.egs_simplify_vertex_quadrics(V, F, _ptr(v), _ptr(f), _ptr(row_start), _ptr(rows), _ptr(keys),
                                                            *org, cell, _ptr(quadrics), 0, S))
    pos = torch.empty((Vc, 3), dtype=torch.float32, device=dev)
    col = None if c is None else torch.empty((Vc, 3), dtype=torch.float32, device=dev)
    placed = torch.empty(Vc, dtype=torch.int32, device=dev)
    _simplifylib.check(lib.egs_simplify_clusters(V, F, Vc, _ptr(v), _ptr(c), _ptr(keys), _ptr(member_start), _ptr(members),
                                                 _ptr(quadrics), None, None, None, *org, cell, place, _ptr(pos), _ptr(col),
                                                 _ptr(placed), 0, S))
    rot = torch.empty((F, 3), dtype=torch.int64, device=dev)
    valid = torch.empty(F, dtype=torch.int32, device=dev)
    key_hi = torch.empty(F, dtype=torch.int64, device=dev)
    key_lo = torch.empty(F, dtype=torch.int64, device=dev)
    _simplifylib.check(lib.egs_simplify_remap_faces(V, F, Vc, _ptr(f), _ptr(cluster), _ptr(rot), _ptr(valid), _ptr(key_hi),
                                                    _ptr(key_lo), 0, S))
    order = torch.sort(key_lo, stable=True).indices                    # (key_hi, key_lo) ascending, ties by face index
    order = order[torch.sort(key_hi[order], stable=True).indices].contiguous()
    fkeep = torch.empty(F, dtype=torch.int32, device=dev)
    ckeep = torch.empty(Vc, dtype=torch.int32, device=dev)
    _simplifylib.check(lib.egs_simplify_keep_flags(F, Vc, _ptr(order), _ptr(rot), _ptr(valid), _ptr(key_hi), _ptr(key_lo),
                                                   _ptr(fkeep), _ptr(ckeep), 0, S))
    vscan = torch.cumsum(ckeep, 0, dtype=torch.int64)
    fscan = torch.cumsum(fkeep, 0, dtype=torch.int64)
    zero = torch.zeros(1, dtype=torch.int64, device=dev)
    Vk, Fk = torch.cat([vscan[-1:], fscan[-1:] if F else zero]).tolist()      # readback 3: the two kept counts
    ov = torch.empty((Vk, 3), dtype=torch.float32, device=dev)
    of = torch.empty((Fk, 3), dtype=torch.int64, device=dev)
    oc = None if c is None else torch.empty((Vk, 3), dtype=torch.float32, device=dev)
    _meshopslib.check(_meshopslib.load().egs_meshops_compact(Vc, F, _ptr(pos), _ptr(col), None, _ptr(rot), _ptr(ckeep),
                                                             _ptr(fkeep), _ptr(vscan), _ptr(fscan), Vk, Fk, _ptr(ov),
                                                             _ptr(oc), None, _ptr(of), 0, S))
    if not return_info:
        return ov, of, oc
    counts = torch.cat([torch.bincount(placed.clamp(0, 3), minlength=4), valid.sum(dtype=torch.int64).reshape(1)]).tolist()
    info = dict(clusters=Vc, placed_mean=counts[0], placed_solved=counts[1], placed_clamped=counts[2],
                placed_no_face=counts[3], faces_degenerate=F - counts[4], faces_duplicate=counts[4] - Fk)
    return ov, of, oc, info


def clean_mesh(vertices, faces, colors=None, min_faces=None, keep_largest=None, smooth_iterations=0, normals=False,
               lam=TAUBIN_LAMBDA, mu=TAUBIN_MU, check=True, simplify_cell=None, simplify_placement="quadric"):
    """-> (vertices, faces, colors or None, normals or None): ``remove_small_components`` (if ``min_faces`` or
    ``keep_largest`` is given), then ``smooth_taubin`` (if ``smooth_iterations`` > 0), then
    ``simplify_vertex_clustering`` with cells of ``simplify_cell`` from the bounding box minimum (if given), then -- with
    ``normals`` -- the ``vertex_normals`` of the result."""
    smooth_iterations = _count(smooth_iterations, "smooth_iterations")
    if simplify_cell is not None:
        _cell_size(simplify_cell, "simplify_cell")
        _placement(simplify_placement, "simplify_placement")
    v, f = _mesh_args(vertices, faces, check)
    c = None if colors is None else _rows3(colors, "colors", v)
    if min_faces is not None or keep_largest is not None:
        v, f, c, _ = remove_small_components(v, f, c, min_faces=min_faces, keep_largest=keep_largest, check=False)
    if smooth_iterations > 0:
        v = smooth_taubin(v, f, smooth_iterations, lam, mu, check=False)
    if simplify_cell is not None:
        v, f, c = simplify_vertex_clustering(v, f, c, cell_size=simplify_cell, placement=simplify_placement, check=False)
    n = vertex_normals(v, f, check=False) if normals else None
    return v, f, c, n


# ------------------------------------------------------------------------------------------------------------ PLY files
def _np(t, dtype):
    return np.ascontiguousarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, dtype)


def save_mesh_ply(path, vertices, faces, colors=None):
    """Binary little-endian PLY of an indexed triangle mesh: vertices [V,3] float32, faces [F,3] integers, optional
    colors [V,3] in [0, 1] written as uchar red green blue.  numpy alone, no ``plyfile``.
    ``save_mesh_ply_with_normals`` writes vertex normals as well."""
    save_mesh_ply_with_normals(path, vertices, faces, colors, None)


def save_mesh_ply_with_normals(path, vertices, faces, colors=None, normals=None):
    """``save_mesh_ply`` with optional normals [V,3] float32, written as float nx ny nz after x y z (the order MeshLab and
    Open3D write); without ``normals`` the file is ``save_mesh_ply``'s byte for byte."""
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
    if normals is not None:
        n = _np(normals, np.float32)
        if n.shape != v.shape:
            raise ValueError("normals must have shape %s, got %s" % (list(v.shape), list(n.shape)))
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
        head += ["property float nx", "property float ny", "property float nz"]
    if colors is not None:
        c = _np(colors, np.float32)
        if c.shape != v.shape:
            raise ValueError("colors must have shape %s, got %s" % (list(v.shape), list(c.shape)))
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        head += ["property uchar red", "property uchar green", "property uchar blue"]
    head += ["element face %d" % len(f), "property list uchar int vertex_indices", "end_header"]
    vrec = np.empty(len(v), dtype=fields)
    vrec["x"], vrec["y"], vrec["z"] = v[:, 0], v[:, 1], v[:, 2]
    if normals is not None:
        vrec["nx"], vrec["ny"], vrec["nz"] = n[:, 0], n[:, 1], n[:, 2]
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


def load_mesh_ply(path, with_normals=False):
    """-> (vertices [V,3] float32, faces [F,3] int64, colors [V,3] float32 in [0, 1] or None) numpy arrays of a file
    ``save_mesh_ply`` or ``save_mesh_ply_with_normals`` wrote (binary little-endian, float x y z, optional float nx ny
    nz, optional uchar red green blue, triangles as ``uchar int`` lists).  With ``with_normals`` a fourth value: the
    normals [V,3] float32, or None if the file has none."""
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
    xyz, nrm, rgb = ["x", "y", "z"], ["nx", "ny", "nz"], ["red", "green", "blue"]
    has_normals = names[3:6] == nrm
    has_color = names[-3:] == rgb
    if nv is None or nf is None or names != xyz + (nrm if has_normals else []) + (rgb if has_color else []) or \
            props["face"] != [["list", "uchar", "int", "vertex_indices"]]:
        raise ValueError("%s: not the layout save_mesh_ply writes" % path)
    fields = [(k, "<f4") for k in xyz + (nrm if has_normals else [])] + ([(k, "u1") for k in rgb] if has_color else [])
    body = end + len(b"end_header\n")
    vrec = np.frombuffer(data, dtype=fields, count=nv, offset=body)
    frec = np.frombuffer(data, dtype=[("n", "u1"), ("i", "<i4", (3,))], count=nf, offset=body + vrec.nbytes)
    if nf and not (frec["n"] == 3).all():
        raise ValueError("%s: a face that is not a triangle" % path)
    v = np.stack([vrec["x"], vrec["y"], vrec["z"]], 1).astype(np.float32)
    c = np.stack([vrec["red"], vrec["green"], vrec["blue"]], 1).astype(np.float32) / np.float32(255) if has_color else None
    if not with_normals:
        return v, frec["i"].astype(np.int64), c
    n = np.stack([vrec["nx"], vrec["ny"], vrec["nz"]], 1).astype(np.float32) if has_normals else None
    return v, frec["i"].astype(np.int64), c, n
