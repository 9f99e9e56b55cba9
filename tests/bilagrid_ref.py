"""float64 reference of the bilateral-grid slice and of the grid's total variation, written with
``torch.nn.functional.grid_sample`` so that autograd gives the reference gradients, and the deterministic inputs of the
bilagrid tests.

The gradient through the luminance is discontinuous where ``luma (L-1)`` is an integer (the pixel changes its z cell;
at 0 and L-1 it enters the clamp).  ``make_inputs`` moves every pixel that lies within 0.01 of such a plane to the
middle of a cell, so float32 and float64 evaluate every pixel in the same cell and NO pixel is excluded from any
comparison.
"""
import torch
import torch.nn.functional as F

LUMA = (0.299, 0.587, 0.114)

# (H, W, (Gw, Gh, L)) of the GPU tests
CASES = [
    (1, 1, (1, 1, 1)),          # degenerate
    (5, 7, (1, 1, 1)),          # global affine
    (9, 1, (4, 4, 4)),          # one column
    (20, 20, (1, 4, 3)),        # size-1 lattice axis (Gw = 1)
    (33, 129, (5, 4, 1)),       # L = 1: no guidance term
    (64, 64, (4, 3, 2)),
    (37, 53, (16, 16, 8)),
    (70, 150, (16, 16, 8)),     # ragged block edges
    (16, 16, (64, 48, 8)),      # global path
    # beyond the issue's list: the matrix form of the dgrid sum (boxes at most two columns wide) on several blocks with
    # ragged edges, waves that cross rows of cells, every layer of an 8-layer grid
    (70, 150, (2, 5, 8)),
]


def luma_of(image):
    return LUMA[0] * image[0] + LUMA[1] * image[1] + LUMA[2] * image[2]


def ref_slice(image, grid):
    """image [3,H,W], grid [12,L,Gh,Gw] (any float dtype, differentiable) -> the corrected image [3,H,W]"""
    H, W = image.shape[1:]
    ys = torch.arange(H, dtype=image.dtype, device=image.device)
    xs = torch.arange(W, dtype=image.dtype, device=image.device)
    ny = (2 * ys / max(H - 1, 1) - 1)[:, None].expand(H, W)
    nx = (2 * xs / max(W - 1, 1) - 1)[None, :].expand(H, W)
    nz = 2 * luma_of(image) - 1
    coords = torch.stack((nx, ny, nz), -1)[None, None]                    # [1,1,H,W,3]: x -> Gw, y -> Gh, z -> L
    A = F.grid_sample(grid[None], coords, mode="bilinear", padding_mode="border", align_corners=True)
    A = A[0, :, 0].reshape(3, 4, H, W)
    return (A[:, :3] * image[None]).sum(1) + A[:, 3]


def ref_tv(grid):
    """sum over the axes x, y, z of the mean squared forward difference (an axis of one node contributes 0)"""
    total = grid.new_zeros(())
    for axis in (3, 2, 1):
        if grid.shape[axis] > 1:
            d = grid.narrow(axis, 1, grid.shape[axis] - 1) - grid.narrow(axis, 0, grid.shape[axis] - 1)
            total = total + (d * d).mean()
    return total


def off_plane(image, L, margin=0.01):
    """bool [H,W]: the pixel's luma (L-1) lies further than ``margin`` from every integer (float64)"""
    t = luma_of(image.double()) * (L - 1)
    return (t - torch.round(t)).abs() >= margin


def make_inputs(H, W, shape, seed=0):
    """-> dict of float32 CPU tensors: image [3,H,W] uniform in [-0.25, 1.25] (both clamps are exercised) with the pixels
    near a luminance plane moved to the middle of a cell, grid [12,L,Gh,Gw] = identity + 0.5 normal, dout [3,H,W] =
    normal / (H W)."""
    gw, gh, L = shape
    g = torch.Generator().manual_seed(1000 * seed + 7 * H + 13 * W + gw + 3 * gh + 5 * L)
    image = torch.rand((3, H, W), generator=g, dtype=torch.float64) * 1.5 - 0.25
    if L > 1:
        for _ in range(3):       # (the float32 rounding of a moved pixel cannot bring it back: 0.5 >> 1e-7)
            t = luma_of(image) * (L - 1)
            k = torch.round(t)
            near = (t - k).abs() < 0.01 + 1e-6
            image = image + torch.where(near, (k + 0.5 - t) / (L - 1), torch.zeros_like(t))[None]
            image = image.float().double()
            if bool(off_plane(image, L).all()):
                break
        assert bool(off_plane(image, L).all()), "a pixel is still within 0.01 of a luminance plane"
    grid = torch.zeros((12, L, gh, gw), dtype=torch.float64)
    grid[(0, 5, 10),] = 1.0
    grid = grid + 0.5 * torch.randn(grid.shape, generator=g, dtype=torch.float64)
    dout = torch.randn((3, H, W), generator=g, dtype=torch.float64) / (H * W)
    return dict(image=image.float(), grid=grid.float(), dout=dout.float())


def ref_all(inp, tv_weight=None):
    """float64 reference of one input set: -> dict(out, dimage, dgrid) for the upstream gradient ``dout`` (and tv, dtv
    with ``tv_weight``)"""
    image = inp["image"].double().requires_grad_(True)
    grid = inp["grid"].double().requires_grad_(True)
    out = ref_slice(image, grid)
    dimage, dgrid = torch.autograd.grad(out, (image, grid), inp["dout"].double())
    r = dict(out=out.detach(), dimage=dimage, dgrid=dgrid)
    if tv_weight is not None:
        g2 = inp["grid"].double().requires_grad_(True)
        value = tv_weight * ref_tv(g2)
        if value.requires_grad and value.grad_fn is not None:
            r["dtv"] = torch.autograd.grad(value, g2)[0]
        else:                                     # a 1 x 1 x 1 grid has no differences
            r["dtv"] = torch.zeros_like(g2)
        r["tv"] = value.detach()
    return r
