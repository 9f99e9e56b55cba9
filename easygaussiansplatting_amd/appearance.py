"""Bilateral-grid appearance compensation (include/egs_bilagrid.h): a per-image lattice of 3 x 4 affine
colour transforms, indexed by pixel position and by the pixel's own luminance, that absorbs the frame-to-frame changes
of exposure, white balance and vignetting of a real capture (Wang et al. 2024, "Bilateral Guided Radiance Field
Processing"; gsplat's ``use_bilateral_grid``).  A 1 x 1 x 1 grid is plain per-image exposure / white balance.

A grid is float32 ``[12, L, Gh, Gw]``: channel ``4c + j`` is entry (c, j) of the transform.  ``shape`` arguments are
``(Gw, Gh, L)``.  An image is planar float32 ``[3, H, W]``.  Pixel (x, y) with colour rgb reads the grid trilinearly at

    gx = x / max(W-1, 1) (Gw-1)    gy = y / max(H-1, 1) (Gh-1)    gz = clamp(0.299 r + 0.587 g + 0.114 b, 0, 1) (L-1)

(``grid_sample``: bilinear, border padding, align_corners) and leaves ``out_c = sum_j A[c, j] rgb_j + A[c, 3]``.

    grids = identity_grids(V)                               # [V, 12, L, Gh, Gw], every node [I | 0]
    out = slice_forward(image, grids[v])                    # HIP (libegs_bilagrid.so)
    dimage = slice_backward(image, grids[v], dout, dgrid)   # dimage is returned, dgrid ACCUMULATED INTO
    value = tv(grids[v], weight, dgrid)                     # weight TV as a 0-dim tensor; dgrid += weight dTV/dG
    out = apply_grid(image, grid)                           # the same under torch.autograd (BilagridSlice)
    table = GridTable(V, shape)                             # the rows, their Adam moments and step counts

``out``, ``dimage`` and everything of ``tv`` are bitwise reproducible.  ``dgrid`` of ``slice_backward`` is a sum of
float atomics: it differs in the last bits from run to run.

The gradient with respect to the image has two terms: ``A^T[:, :3] dout`` and the guidance term through the luminance,
which is zero when ``L == 1`` or the luminance lies outside (0, 1).  It is discontinuous where ``luma (L-1)`` is an
integer.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _bilagridlib
from ._host import _chk, _ptr, _stream

DEFAULT_SHAPE = (16, 16, 8)


def _shape3(shape):
    gw, gh, l = (int(s) for s in shape)
    if min(gw, gh, l) < 1:
        raise ValueError("a grid shape is (Gw, Gh, L) with every size >= 1, got %r" % (tuple(shape),))
    if 12 * gw * gh * l > _bilagridlib.MAX_GRID_FLOATS:
        raise ValueError("a grid of shape %r holds more than %d floats" % ((gw, gh, l), _bilagridlib.MAX_GRID_FLOATS))
    return gw, gh, l


def identity_grids(V, shape=DEFAULT_SHAPE, device="cpu") -> torch.Tensor:
    """-> float32 ``[V, 12, L, Gh, Gw]``: every node of every grid is the identity transform ``[I | 0]``."""
    gw, gh, l = _shape3(shape)
    g = torch.zeros((int(V), 12, l, gh, gw), dtype=torch.float32, device=device)
    g[:, (0, 5, 10)] = 1.0
    return g


def _span(p0, p1, scale, den, g):
    """the box of nodes of the pixels [p0, p1] of one axis -> node count (span_of in csrc/egs_bilagrid.hip)"""
    top = max(g - 2, 0)
    c0 = min(p0 * scale // den, top)
    c1 = min(min(p1 * scale // den, top) + 1, g - 1)
    return c1 - c0 + 1


def _box_extent(H, W, shape):
    gw, gh, l = _shape3(shape)
    bw, bh = _bilagridlib.BLOCK_W, _bilagridlib.BLOCK_H
    nx = max(_span(p, min(p + bw, W) - 1, gw - 1, max(W - 1, 1), gw) for p in range(0, W, bw))
    ny = max(_span(p, min(p + bh, H) - 1, gh - 1, max(H - 1, 1), gh) for p in range(0, H, bh))
    return nx, ny, l


def largest_box(H, W, shape) -> int:
    """floats of the largest box of lattice nodes that one workgroup's pixel block touches (largest_box in
    csrc/egs_bilagrid.hip: integer arithmetic, the same on both sides)"""
    nx, ny, l = _box_extent(H, W, shape)
    return nx * ny * l * 12


def slice_path(H, W, shape) -> str:
    """Which kernels the library picks for an ``H x W`` image and a grid of ``shape``: "lds" (the box of lattice nodes of
    every pixel block fits the LDS budget: staged / accumulated there) or "global" (cells smaller than pixels: global
    reads and per-pixel global atomics).  A pure host function that mirrors the library's decision."""
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError("slice_path: the image is %d x %d" % (H, W))
    return "lds" if largest_box(H, W, shape) <= _bilagridlib.LDS_FLOATS else "global"


def dgrid_form(H, W, shape) -> str:
    """How the backward pass sums ``dgrid`` inside a pixel block: "matrix" (LDS path, every box at most 2 columns wide,
    at most 8 layers: MFMAs keep a wave's sums in registers), "lds" (LDS path otherwise: wave reduction or LDS atomics)
    or "global" (per-pixel global atomics).  Mirrors the library's choice, as ``slice_path`` does."""
    if slice_path(H, W, shape) == "global":
        return "global"
    nx, _, l = _box_extent(int(H), int(W), shape)
    return "matrix" if nx <= 2 and l <= 8 else "lds"


def _check_pair(image, grid, what):
    image = _chk(image, "image", torch.float32, (3, None, None))
    grid = _chk(grid, "grid", torch.float32, (12, None, None, None))
    if grid.device != image.device:
        raise ValueError("%s: the grid lives on %s, the image on %s" % (what, grid.device, image.device))
    H, W = image.shape[1:]
    l, gh, gw = grid.shape[1:]
    _shape3((gw, gh, l))
    m = _bilagridlib.MAX_COORD_PRODUCT
    if (W - 1) * (gw - 1) >= m or (H - 1) * (gh - 1) >= m:
        raise ValueError("%s: (W-1)(Gw-1) and (H-1)(Gh-1) must stay below %d" % (what, m))
    return image, grid, (int(H), int(W), int(gw), int(gh), int(l))


def _dev(t):
    return t.device.index if t.device.index is not None else torch.cuda.current_device()


def slice_forward(image, grid) -> torch.Tensor:
    """-> float32 [3,H,W]: ``image`` under ``grid`` ([12,L,Gh,Gw]), on the current stream.  Bitwise reproducible."""
    image, grid, dims = _check_pair(image, grid, "slice_forward")
    out = torch.empty_like(image)                       # the kernel writes every pixel
    lib = _bilagridlib.load()
    with torch.cuda.device(image.device):
        _bilagridlib.check(lib.egs_bilagrid_slice(_dev(image), _stream(), *dims, _ptr(image.detach()),
                                                  _ptr(grid.detach()), _ptr(out)))
    return out


def slice_backward(image, grid, dout, dgrid=None, need_dimage=True):
    """The backward pass of ``slice_forward`` for the upstream gradient ``dout`` [3,H,W].  -> ``dimage`` [3,H,W] (written,
    bitwise reproducible; None with ``need_dimage=False``).  With ``dgrid`` ([12,L,Gh,Gw] float32, contiguous) the grid's
    gradient is ACCUMULATED INTO it (float atomics: not reproducible to the bit); None skips that half."""
    image, grid, dims = _check_pair(image, grid, "slice_backward")
    dout = _chk(dout, "dout", torch.float32, tuple(image.shape))
    if dout.device != image.device:
        raise ValueError("slice_backward: dout lives on %s, the image on %s" % (dout.device, image.device))
    if dgrid is not None:
        if isinstance(dgrid, torch.Tensor) and not dgrid.is_contiguous():
            raise ValueError("dgrid must be contiguous: the gradient is accumulated into the caller's own buffer")
        dgrid = _chk(dgrid, "dgrid", torch.float32, tuple(grid.shape))
        if dgrid.device != image.device:
            raise ValueError("slice_backward: dgrid lives on %s, the image on %s" % (dgrid.device, image.device))
    dimage = torch.empty_like(image) if need_dimage else None
    lib = _bilagridlib.load()
    with torch.cuda.device(image.device):
        _bilagridlib.check(lib.egs_bilagrid_slice_bwd(_dev(image), _stream(), *dims, _ptr(image.detach()),
                                                      _ptr(grid.detach()), _ptr(dout.detach()), _ptr(dimage),
                                                      _ptr(dgrid)))
    return dimage


def tv(grid, weight, dgrid=None) -> torch.Tensor:
    """-> ``weight * TV(grid)`` as a 0-dim device tensor, TV = the sum over the axes x, y, z of the mean squared forward
    difference along the axis (an axis of one node contributes 0); with ``dgrid`` ([12,L,Gh,Gw], contiguous) adds
    ``weight * dTV/dgrid`` to it.  One launch, no atomics: bitwise reproducible."""
    grid = _chk(grid, "grid", torch.float32, (12, None, None, None))
    l, gh, gw = (int(s) for s in grid.shape[1:])
    _shape3((gw, gh, l))
    if dgrid is not None:
        if isinstance(dgrid, torch.Tensor) and not dgrid.is_contiguous():
            raise ValueError("dgrid must be contiguous: the gradient is accumulated into the caller's own buffer")
        dgrid = _chk(dgrid, "dgrid", torch.float32, tuple(grid.shape))
        if dgrid.device != grid.device:
            raise ValueError("tv: dgrid lives on %s, the grid on %s" % (dgrid.device, grid.device))
    value = torch.empty((), dtype=torch.float32, device=grid.device)
    lib = _bilagridlib.load()
    with torch.cuda.device(grid.device):
        _bilagridlib.check(lib.egs_bilagrid_tv(_dev(grid), _stream(), gw, gh, l, _ptr(grid.detach()), float(weight),
                                               _ptr(value), _ptr(dgrid)))
    return value


class BilagridSlice(torch.autograd.Function):
    """``BilagridSlice.apply(image, grid)`` -> the corrected image, differentiable with respect to both."""

    @staticmethod
    def forward(ctx, image, grid):
        ctx.save_for_backward(image, grid)
        return slice_forward(image, grid)

    @staticmethod
    def backward(ctx, dout):
        image, grid = ctx.saved_tensors
        need_image, need_grid = ctx.needs_input_grad
        if not (need_image or need_grid):
            return None, None
        dgrid = torch.zeros_like(grid, memory_format=torch.contiguous_format) if need_grid else None
        dimage = slice_backward(image, grid, dout.contiguous(), dgrid, need_dimage=need_image)
        return dimage, dgrid


def apply_grid(image, grid) -> torch.Tensor:
    """``slice_forward`` as an autograd node (``BilagridSlice``)"""
    return BilagridSlice.apply(image, grid)


class GridTable:
    """One grid per training image, all identity at the start, and an Adam that steps ROWS (as ``pose.PoseTable``): a
    view's grid, both moments and its step count move only in the steps that rendered it.  A stepped row is
    ``torch.optim.Adam`` on that row alone -- the same torch ops in the same order.

    ``grids``, ``exp_avg``, ``exp_avg_sq`` [V,12,L,Gh,Gw] live on ``device``; ``steps`` [V] int64 on the host (the bias
    corrections are host scalars: no device read-back in a step).  ``step`` is pure torch and runs on CPU tensors too."""

    def __init__(self, V, shape=DEFAULT_SHAPE, lr=2e-3, betas=(0.9, 0.999), eps=1e-15, device="cuda"):
        self.shape = _shape3(shape)
        self.device = device
        self.grids = identity_grids(V, self.shape, device)
        self.exp_avg = torch.zeros_like(self.grids)
        self.exp_avg_sq = torch.zeros_like(self.grids)
        self.steps = torch.zeros(int(V), dtype=torch.int64)
        self.lr = float(lr)
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)

    def __len__(self):
        return self.grids.shape[0]

    @property
    def row_floats(self):
        gw, gh, l = self.shape
        return 12 * l * gh * gw

    @torch.no_grad()
    def step(self, view_ids, grad_rows):
        """One Adam step of the rows ``view_ids`` on ``grad_rows``: row k of ``grad_rows`` ([len(view_ids), ...], any
        trailing shape of 12 L Gh Gw floats) is the gradient of grid ``view_ids[k]``.  A view may appear once."""
        ids = [int(i) for i in view_ids]
        if len(set(ids)) != len(ids):
            raise ValueError("GridTable.step: a view appears twice in %r" % (ids,))
        if grad_rows.shape[0] != len(ids):
            raise ValueError("GridTable.step: %d gradient rows for %d views" % (grad_rows.shape[0], len(ids)))
        b1, b2 = self.betas
        for k, v in enumerate(ids):
            self.steps[v] += 1
            n = int(self.steps[v])
            bc1, bc2 = 1 - b1 ** n, 1 - b2 ** n
            g = grad_rows[k].reshape(self.grids.shape[1:])
            p, m, s = self.grids[v], self.exp_avg[v], self.exp_avg_sq[v]
            m.lerp_(g, 1 - b1)                                   # torch/optim/adam.py _single_tensor_adam, op for op
            s.mul_(b2).addcmul_(g, g, value=1 - b2)
            denom = (s.sqrt() / bc2 ** 0.5).add_(self.eps)
            p.addcdiv_(m, denom, value=-(self.lr / bc1))

    def save(self, fn, ids=None):
        """The grids as an ``.npz``: ``ids`` [V], ``grids`` [V,12,L,Gh,Gw], ``shape`` = (Gw, Gh, L)."""
        ids = np.arange(len(self)) if ids is None else np.asarray(ids)
        np.savez(fn, ids=ids, grids=self.grids.detach().cpu().numpy(), shape=np.asarray(self.shape, np.int64))

    def load(self, fn):
        """Read the grids of ``save`` back (moments and step counts start afresh).  -> ``ids``"""
        with np.load(fn) as z:
            shape = tuple(int(s) for s in z["shape"])
            grids = torch.from_numpy(np.ascontiguousarray(z["grids"], np.float32))
            ids = np.asarray(z["ids"])
        if shape != self.shape or tuple(grids.shape) != tuple(self.grids.shape):
            raise ValueError("GridTable.load: %s holds %d grids of shape %r, the table %d of shape %r"
                             % (fn, grids.shape[0], shape, len(self), self.shape))
        self.grids.copy_(grids)
        self.exp_avg.zero_()
        self.exp_avg_sq.zero_()
        self.steps.zero_()
        return ids
