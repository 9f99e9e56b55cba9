"""Hand-built inputs of the bilateral-grid kernels by the form a wave of the backward pass takes, a census of those forms
on the CPU, and a float32 restatement of the slice that says how far float32 itself lies from float64.  Host only (numpy
and torch on the CPU); tests/test_bilagrid_cases_cpu.py checks all of it, tests/test_gpu_bilagrid_waves.py runs the cases.

The census is written from include/egs_bilagrid.h and DESIGN §3.15 and from the integer rules of ``appearance._span``: a
workgroup owns 64 x 32 pixels, wave w of its four takes the rows w, w + 4, .. of the block, lane l the column l of the
block, clamped into the image (a lane outside the image stays active, reads the last column and carries dout = 0).  A
pixel's cell on an axis of g nodes is ``min(p (g-1) // max(n-1, 1), max(g-2, 0))``.

The classes, counted per (block, wave, row) unless said otherwise:

  lds form     uniform (the 64 lanes share the x cell and the layer) / mixed, each full / dead (lanes outside the image);
               a uniform wave is interior (every live lane has 0 < fz < 1) or clamped
  matrix form  per (block, wave) with rows: mat_flush+ (the wave's rows cross a row of cells, so its accumulators are
               flushed before the end) / mat_flush0; mat_dead counts those of them in a block with dead lanes
  global form  global_full / global_dead
  any form     wave_without_rows, per (block, wave): the block has fewer rows than the wave's index + 1

Bounds: an entry of a tensor may differ from float64 by max(T 2^-24 S, 2 x distance).  S is the entry's sum of |terms|,
distance the largest distance from float64 of the float32 restatement over EVALUATIONS (as given, four with every input
one ulp away, four with the dgrid sum in a shuffled pixel order).  The two branches cover two things.  What every float32
evaluation shares -- the one rounding of the lattice coordinate x (Gw-1) / (W-1), whose ulp grows with the coordinate:
1e-4 of the output at 513 nodes -- is in ``distance``.  What they disagree by is the floor's: T is, per case and tensor,
the smallest power of two at which the spread of the evaluations (largest minus smallest distance) stays within half of
T 2^-24 S on every entry.  It is set by the reference alone.  T is 8 .. 32 where the chain of roundings is all there
is; it grows with L on the output (gz = luma (L-1) has an ulp of (L-1) 2^-24, which moves fz and with it every weight),
and on dgrid where cells are smaller than pixels: an entry is then one pixel's term, and the relative error of one
small weight fz or 1 - fz has no bound.
"""
import collections
import functools

import numpy as np
import torch

from easygaussiansplatting_amd import scene as S
from tests import bilagrid_ref as R

F = np.float32
BW, BH, WAVES = 64, 32, 4                     # EGS_BILAGRID_BLOCK_W / _H; 256 threads
LDS_FLOATS = 8192                             # EGS_BILAGRID_LDS_FLOATS
MAT_NX, MAT_L = 2, 8                          # the matrix form: boxes at most 2 columns wide, at most 8 layers
MAT_SCRATCH_BYTES = WAVES * 64 * (12 + 4 + 1) * 4      # per wave and lane: a V row, four weights, four packed nodes
N_PERTURBED, N_ORDERS = 4, 4
EVALUATIONS = [(None, None)] + [(j, None) for j in range(N_PERTURBED)] + [(None, j) for j in range(N_ORDERS)]
TENSORS = ("out", "dimage", "dgrid")


# ---- the integer rules -------------------------------------------------------------------------------------------

def cell(p, scale, den, g):
    """lower node of the cell of pixel(s) ``p`` on an axis of ``g`` nodes"""
    return np.minimum(np.asarray(p) * scale // den, max(g - 2, 0))


def span(p0, p1, scale, den, g):
    """first node and node count of the box of the pixels [p0, p1]"""
    c0 = int(cell(p0, scale, den, g))
    return c0, min(int(cell(p1, scale, den, g)) + 1, g - 1) - c0 + 1


def box_extent(H, W, shape):
    gw, gh, L = shape
    nx = max(span(p, min(p + BW, W) - 1, gw - 1, max(W - 1, 1), gw)[1] for p in range(0, W, BW))
    ny = max(span(p, min(p + BH, H) - 1, gh - 1, max(H - 1, 1), gh)[1] for p in range(0, H, BH))
    return nx, ny, L


def form_of(H, W, shape):
    nx, ny, L = box_extent(H, W, shape)
    if nx * ny * L * 12 > LDS_FLOATS:
        return "global"
    return "matrix" if nx <= MAT_NX and L <= MAT_L else "lds"


def lds_bytes(H, W, shape, dimage=True, dgrid=True):
    """dynamic LDS of the backward launch: one box per half it is asked for, and the matrix form's scratch"""
    form = form_of(H, W, shape)
    if form == "global":
        return 0
    nx, ny, L = box_extent(H, W, shape)
    return 4 * nx * ny * L * 12 * (int(dimage) + int(dgrid)) + (MAT_SCRATCH_BYTES if form == "matrix" and dgrid else 0)


def luma32(image):
    """float32 luminance, one rounding per operation"""
    image = np.asarray(image, F)
    return F(0.299) * image[0] + F(0.587) * image[1] + F(0.114) * image[2]


def layer_of(luma, L):
    """-> (z0, fz) of float32 luminances"""
    gz = np.clip(luma, F(0), F(1)) * F(L - 1)
    z0 = np.minimum(gz.astype(np.int64), max(L - 2, 0))
    return z0, gz - z0.astype(F)


def census(H, W, shape, image):
    """-> dict(form, box (floats of the largest box), lds_bytes (both halves), counts (class -> waves),
    rows ({(y, block column): class} of the lds and global forms, for picking pixels))"""
    gw, gh, L = shape
    form = form_of(H, W, shape)
    nx, ny, _ = box_extent(H, W, shape)
    counts = collections.Counter()
    rows = {}
    nbx, nby = -(-W // BW), -(-H // BH)
    z0, fz = layer_of(luma32(np.asarray(image)), L)
    ycell = cell(np.arange(H), gh - 1, max(H - 1, 1), gh)
    for by in range(nby):
        nrows = min(BH, H - by * BH)
        for bx in range(nbx):
            live = min(BW, W - bx * BW)
            x = np.minimum(bx * BW + np.arange(BW), W - 1)
            xc = cell(x, gw - 1, max(W - 1, 1), gw)
            dead = live < BW
            for w in range(WAVES):
                mine = list(range(by * BH + w, by * BH + nrows, WAVES))
                if not mine:
                    counts["wave_without_rows"] += 1
                    continue
                if form == "matrix":
                    crossed = len(set(int(ycell[y]) for y in mine)) > 1
                    counts["mat_flush+" if crossed else "mat_flush0"] += 1
                    if dead:
                        counts["mat_dead"] += 1
                    continue
                for y in mine:
                    if form == "global":
                        name = "global_dead" if dead else "global_full"
                    else:
                        zs = z0[y, x]
                        uniform = bool((xc == xc[0]).all() and (zs == zs[0]).all())
                        name = ("uniform_" if uniform else "mixed_") + ("dead" if dead else "full")
                        if uniform:
                            f = fz[y, x[:live]]
                            name += "_interior" if bool(((f > 0) & (f < 1)).all()) else "_clamped"
                    counts[name] += 1
                    rows[(y, bx)] = name
    return dict(form=form, box=nx * ny * L * 12, lds_bytes=lds_bytes(H, W, shape), counts=dict(counts), rows=rows)


# ---- the inputs --------------------------------------------------------------------------------------------------

def random(H, W, shape):
    return R.make_inputs(H, W, shape)


def clamp_rows(H):
    """the rows of ``striped`` that hold the pixels outside (0, 1): -> (low, high); with H == 2 both share row 1 (left
    half low, right half high)"""
    if H >= 3:
        return max(y for y in range(H) if y % 3 == 1), max(y for y in range(H) if y % 3 == 2)
    return H - 1, H - 1


def striped(H, W, shape):
    """``make_inputs`` with every third row moved, pixel by pixel, into one layer: the luma of row 3 i lands at
    (k + u) / (L-1), u in [0.15, 0.85], k = i mod (L-1); one row lands below 0 and one above 1.  The move is one
    constant per pixel added to all three channels (the luminance weights sum to 1)."""
    gw, gh, L = shape
    assert L >= 2 and H >= 2
    inp = R.make_inputs(H, W, shape)
    image = inp["image"].double().numpy()
    luma = R.LUMA[0] * image[0] + R.LUMA[1] * image[1] + R.LUMA[2] * image[2]
    u = S.uniform01(4242 + 7 * H + 13 * W + gw + 3 * gh + 5 * L, 0, (H, W))
    target = luma.copy()
    for i, y in enumerate(range(0, H, 3)):
        target[y] = (i % (L - 1) + 0.15 + 0.7 * u[y]) / (L - 1)
    low, high = clamp_rows(H)
    below, above = -(0.3 + 0.4 * u) / (L - 1), 1 + (0.3 + 0.4 * u) / (L - 1)
    if low != high:
        target[low], target[high] = below[low], above[high]
    else:
        target[low, :W // 2], target[low, W // 2:] = below[low, :W // 2], above[low, W // 2:]
    image = torch.from_numpy((image + (target - luma)[None]).astype(F))
    assert bool(R.off_plane(image, L).all()), "a pixel lies within 0.01 of a luminance plane"
    return dict(inp, image=image)


BUILDERS = {"random": random, "striped": striped}

# name -> (set, H, W, (Gw, Gh, L), builder)
CASES = collections.OrderedDict([
    ("uniform-L2", ("uniform", 40, 200, (3, 3, 2), "random")),
    ("uniform-L5", ("uniform", 40, 200, (3, 3, 5), "striped")),
    ("uniform-L12", ("uniform", 37, 100, (2, 3, 12), "striped")),      # L > 8 keeps boxes 2 wide out of the matrix form
    ("matrix-nx1", ("matrix", 70, 150, (1, 9, 3), "striped")),
    ("matrix-L1", ("matrix", 130, 70, (2, 40, 1), "random")),
    ("matrix-3rows", ("matrix", 3, 70, (2, 2, 4), "striped")),
    ("matrix-box8064", ("matrix", 64, 70, (2, 84, 8), "striped")),     # the largest LDS request of the library
    ("global", ("global", 40, 130, (40, 30, 4), "striped")),
    ("cap-x-lds", ("cap", 2, 8191, (513, 1, 2), "striped")),           # (W-1)(Gw-1) = 4 193 280 < 2^22
    ("cap-y-matrix", ("cap", 8191, 3, (1, 513, 2), "striped")),        # (H-1)(Gh-1) likewise; 256 blocks in y
    ("cap-x-global", ("cap", 2, 8191, (513, 1, 128), "random")),       # box 9216
])
DELTA_OF = collections.OrderedDict([("delta-uniform", "uniform-L5"), ("delta-matrix", "matrix-nx1"),
                                    ("delta-global", "global")])
ALL_NAMES = list(CASES) + list(DELTA_OF)

# per case: T of (out, dimage, dgrid), the smallest powers of two at which ``calibration`` stays at or below 0.5; behind
# each the ratios it then gives.  test_bilagrid_cases_cpu.test_calibration holds the table against the reference.
T = {
    "uniform-L2": (16, 16, 8),              # 0.33, 0.33, 0.34
    "uniform-L5": (32, 16, 16),             # 0.49, 0.33, 0.27
    "uniform-L12": (64, 16, 32),            # 0.48, 0.35, 0.29
    "matrix-nx1": (32, 16, 8),              # 0.40, 0.39, 0.42
    "matrix-L1": (16, 32, 16),              # 0.46, 0.27, 0.25
    "matrix-3rows": (16, 16, 8),            # 0.32, 0.27, 0.38
    "matrix-box8064": (128, 32, 256),       # 0.28, 0.28, 0.41
    "global": (64, 16, 1024),               # 0.29, 0.47, 0.25
    "cap-x-lds": (32, 32, 16),              # 0.29, 0.30, 0.49
    "cap-y-matrix": (32, 32, 16),           # 0.34, 0.28, 0.37
    "cap-x-global": (2048, 32, 65536),      # 0.48, 0.46, 0.32
    "delta-uniform": (32, 8, 64),           # 0.49, 0.50, 0.46
    "delta-matrix": (32, 8, 32),            # 0.40, 0.32, 0.39
    "delta-global": (64, 16, 32),           # 0.29, 0.26, 0.49
}


def shape_of(name):
    """-> (H, W, (Gw, Gh, L))"""
    return CASES[DELTA_OF.get(name, name)][1:4]


def on_node(n, g):
    """the pixels of an axis of n pixels that lie exactly on one of its g nodes"""
    den = max(n - 1, 1)
    return [p for p in range(n) if p * (g - 1) % den == 0]


def delta_pixels(name):
    """the hand-picked pixels of a delta case: -> {(x, y): why}"""
    H, W, shape = shape_of(name)
    gw, gh, L = shape
    base = inputs(DELTA_OF[name])
    cen = census(H, W, shape, base["image"].numpy())
    low, high = clamp_rows(H)
    inner = [x for x in on_node(W, gw) if 0 < x < W - 1]
    picks = collections.OrderedDict()
    picks[(BW, 4)] = "first column of a block"
    picks[(W - 1, 9)] = "last live column of a ragged block, top cell of x"
    picks[(inner[0] if inner else 0, 13)] = "exactly on a node of x"
    picks[(17, H - 1)] = "last row, top cell of y"
    picks[(W - 1, H - 1)] = "last pixel of both axes"
    picks[(100, low)] = "luma < 0"
    picks[(101, high)] = "luma > 1"
    if cen["form"] == "lds":
        uni = sorted(k for k, v in cen["rows"].items() if v == "uniform_full_interior")
        mix = sorted(k for k, v in cen["rows"].items() if v == "mixed_full")
        (y, bx) = uni[len(uni) // 2]
        picks[(bx * BW + 21, y)] = "a uniform wave"
        (y, bx) = mix[len(mix) // 2]
        picks[(bx * BW + 40, y)] = "a mixed wave"
    return picks


@functools.lru_cache(maxsize=None)
def inputs(name):
    """-> dict of float32 CPU tensors image, grid, dout (shared: never written to)"""
    if name in DELTA_OF:
        base = inputs(DELTA_OF[name])
        H, W, _ = shape_of(name)
        dout = torch.zeros_like(base["dout"])
        for (x, y) in delta_pixels(name):
            dout[:, y, x] = base["dout"][:, y, x] * (H * W / 16.0)
        return dict(base, dout=dout)
    _, H, W, shape, builder = CASES[name]
    return BUILDERS[builder](H, W, shape)


def intended_nodes(name):
    """bool [L, Gh, Gw]: the nodes that the pixels of a delta case reach with a non-zero weight, by integer rules"""
    H, W, (gw, gh, L) = shape_of(name)
    image = inputs(name)["image"].numpy()
    luma = luma32(image)

    def axis(p, n, g):
        num, den = p * (g - 1), max(n - 1, 1)
        c = int(cell(p, g - 1, den, g))
        nodes = []
        if num != (c + 1) * den:
            nodes.append(c)
        if num != c * den:
            nodes.append(min(c + 1, g - 1))
        return nodes

    hit = np.zeros((L, gh, gw), bool)
    for (x, y) in delta_pixels(name):
        lu = float(luma[y, x])
        if lu <= 0 or L == 1:
            zs = [0]
        elif lu >= 1:
            zs = [L - 1]
        else:
            z0 = min(int(lu * (L - 1)), L - 2)
            zs = [z0, z0 + 1]
        for z in zs:
            for yy in axis(y, H, gh):
                for xx in axis(x, W, gw):
                    hit[z, yy, xx] = True
    return hit


# ---- the restatement ---------------------------------------------------------------------------------------------

def perturbed(inp, j):
    """every float32 input one ulp up or down by the counter generator's stream ``j`` (tests/pergaussian_ref.perturbed);
    zeros stay zeros (the dout of a delta case is structure, not a rounding)"""
    out = {}
    for i, k in enumerate(sorted(inp)):
        v = np.asarray(inp[k], F)
        up = S.uniform01(977 + j, i, v.shape) < 0.5
        moved = np.where(up, np.nextafter(v, F(np.inf)), np.nextafter(v, F(-np.inf))).astype(F)
        out[k] = np.where(v == 0, v, moved)
    return out


def _axis(n, g, dt):
    """cells and positions of the n pixels of an axis of g nodes: the quotient is formed in ``dt``, as the header says"""
    p = np.arange(n, dtype=np.int64)
    q = (p * (g - 1)).astype(dt) / dt(max(n - 1, 1))
    c = np.minimum(np.floor(q).astype(np.int64), max(g - 2, 0))
    return c, np.minimum(c + 1, g - 1), q - c.astype(dt)


def slice_np(inp, perturb=None, order=None, dtype=F):
    """The slice, its dimage and its dgrid in ``dtype`` arithmetic, one rounding per operation, from the formulas of
    include/egs_bilagrid.h.  ``perturb``: stream of ``perturbed``; ``order``: seed of the pixel order of the dgrid sum.
    -> dict(out, dimage, dgrid) and, under "S", the float64 sum of |terms| of every entry of the three."""
    dt = dtype
    arrays = {k: np.asarray(v, F) for k, v in inp.items() if k in ("image", "grid", "dout")}
    if perturb is not None:
        arrays = perturbed(arrays, perturb)
    image, grid, dout = (arrays[k].astype(dt) for k in ("image", "grid", "dout"))
    _, H, W = image.shape
    _, L, gh, gw = grid.shape
    x0, x1, fx = _axis(W, gw, dt)
    y0, y1, fy = _axis(H, gh, dt)
    luma = dt(0.299) * image[0] + dt(0.587) * image[1] + dt(0.114) * image[2]
    gz = np.clip(luma, dt(0), dt(1)) * dt(L - 1)
    z0 = np.minimum(gz.astype(np.int64), max(L - 2, 0))
    z1 = np.minimum(z0 + 1, L - 1)
    fz = gz - z0.astype(dt)
    one = dt(1)
    wx, wy, wz = (one - fx, fx), (one - fy, fy), (one - fz, fz)
    xs, ys, zs = (x0, x1), (y0, y1), (z0, z1)
    rgb1 = np.concatenate([image, np.ones((1, H, W), dt)], 0)
    # corner k = 4 kz + 2 ky + kx: weight, node and the node's twelve floats, per pixel
    weight, node, G = [], [], []
    for k in range(8):
        kz, ky, kx = k >> 2, (k >> 1) & 1, k & 1
        weight.append(wz[kz] * wy[ky][:, None] * wx[kx][None, :])
        yy = np.broadcast_to(ys[ky][:, None], (H, W))
        xx = np.broadcast_to(xs[kx][None, :], (H, W))
        node.append((zs[kz] * gh + yy) * gw + xx)
        G.append(grid[:, zs[kz], yy, xx])                         # [12, H, W]
    A = np.zeros((12, H, W), dt)
    dA = np.zeros((12, H, W), dt)                                  # A_xy(z1) - A_xy(z0)
    SA = np.zeros((12, H, W), np.float64)
    SdA = np.zeros((12, H, W), np.float64)
    for k in range(8):
        A = A + weight[k][None] * G[k]
        wxy = wy[(k >> 1) & 1][:, None] * wx[k & 1][None, :]
        dA = dA + (wxy if k >= 4 else -wxy)[None] * G[k]
        SA += np.abs(weight[k][None].astype(np.float64) * G[k])
        SdA += np.abs(wxy[None].astype(np.float64) * G[k])
    if L == 1:
        dA[:] = 0
        SdA[:] = 0
    A, dA, SA, SdA = (a.reshape(3, 4, H, W) for a in (A, dA, SA, SdA))
    out = A[:, 0] * rgb1[0] + A[:, 1] * rgb1[1] + A[:, 2] * rgb1[2] + A[:, 3]
    S_out = (SA * np.abs(rgb1.astype(np.float64))[None]).sum(1)
    # dimage_j = sum_c A[c, j] dout_c + luma weight_j (L-1) sum_c dout_c (dA[c] . rgb1) inside (0, 1)
    dimage = A[0, :3] * dout[0][None] + A[1, :3] * dout[1][None] + A[2, :3] * dout[2][None]
    S_dimage = (SA[:, :3] * np.abs(dout.astype(np.float64))[:, None]).sum(0)
    inside = (luma > 0) & (luma < 1) & (L > 1)
    through = np.zeros((H, W), dt)
    S_through = np.zeros((H, W), np.float64)
    for c in range(3):
        through = through + dout[c] * (dA[c, 0] * rgb1[0] + dA[c, 1] * rgb1[1] + dA[c, 2] * rgb1[2] + dA[c, 3])
        S_through += np.abs(dout[c].astype(np.float64)) * (SdA[c] * np.abs(rgb1.astype(np.float64))).sum(0)
    through = through * dt(L - 1)
    coef = np.array([0.299, 0.587, 0.114], dt)
    dimage = dimage + np.where(inside, through, dt(0))[None] * coef[:, None, None]
    S_dimage += np.where(inside, S_through * (L - 1), 0.0)[None] * coef.astype(np.float64)[:, None, None]
    # dgrid[4c + j, node] = sum over pixels and corners of w dout_c rgb1_j, added one term at a time in pixel order
    v = (dout[:, None] * rgb1[None]).reshape(12, H * W)           # [12, pixels]
    pix = np.arange(H * W)
    if order is not None:
        pix = np.argsort(S.uniform01(555 + order, 0, (H * W,)), kind="stable")
    nodes = L * gh * gw
    dgrid = np.zeros(12 * nodes, dt)
    S_dgrid = np.zeros(12 * nodes, np.float64)
    ch = (np.arange(12) * nodes)[:, None]
    for k in range(8):
        term = weight[k].reshape(-1)[pix][None] * v[:, pix]
        at = (ch + node[k].reshape(-1)[pix][None]).T.reshape(-1)   # pixel-major: a pixel's twelve, then the next pixel
        np.add.at(dgrid, at, term.T.reshape(-1))
        np.add.at(S_dgrid, at, np.abs(term.astype(np.float64)).T.reshape(-1))
    return dict(out=out, dimage=dimage, dgrid=dgrid.reshape(12, L, gh, gw),
                S=dict(out=S_out, dimage=S_dimage, dgrid=S_dgrid.reshape(12, L, gh, gw)))


def slice_f32(inp, perturb=None, order=None):
    """``slice_np`` in float32.  (Not float32 grid_sample: that goes through normalised coordinates.)"""
    return slice_np(inp, perturb, order, F)


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> dict per tensor of float64 arrays: ref (the float64 evaluation of the restatement, which
    test_bilagrid_cases_cpu holds against the grid_sample reference), S, distance and nearest (largest and smallest
    over EVALUATIONS of |float32 restatement - ref|, per entry).  Computed once per case, shared, never written to."""
    inp = inputs(name)
    r64 = slice_np(inp, dtype=np.float64)
    out = {t: dict(ref=r64[t], S=r64["S"][t], distance=np.zeros(r64[t].shape), nearest=np.full(r64[t].shape, np.inf))
           for t in TENSORS}
    for perturb, order in EVALUATIONS:
        r32 = slice_f32(inp, perturb, order)
        for t in TENSORS:
            d = np.abs(r32[t].astype(np.float64) - r64[t])
            o = out[t]
            o["nearest"] = np.minimum(o["nearest"], d)
            o["distance"] = np.maximum(o["distance"], d)
    return out


def floor_of(name, tensor, extra=None):
    """T 2^-24 S per entry; ``extra`` (the start of an accumulating call) joins the magnitude"""
    s = reference(name)[tensor]["S"]
    if extra is not None:
        s = s + np.abs(np.asarray(extra, np.float64))
    return T[name][TENSORS.index(tensor)] * 2.0 ** -24 * s


def bound_of(name, tensor, extra=None):
    """what a float32 evaluation may differ from float64 by, per entry: max(floor, 2 x distance)"""
    return np.maximum(floor_of(name, tensor, extra), 2 * reference(name)[tensor]["distance"])


def calibration(name, tensor, t=None):
    """The floor held against the restatement itself: the spread of its evaluations -- largest minus smallest distance
    from float64, what float32 evaluations of one entry disagree by -- over the floor T 2^-24 S.  (The other branch of
    the bound, 2 x distance, holds for the restatement by construction: it covers what all evaluations share, the
    rounding of the lattice coordinate.)  -> the largest ratio over the entries (0 where the spread is 0); ``t``
    replaces the case's T."""
    r = reference(name)[tensor]
    floor = float(T[name][TENSORS.index(tensor)] if t is None else t) * 2.0 ** -24 * r["S"]
    spread = r["distance"] - r["nearest"]
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(spread == 0, 0.0, spread / floor)
    return float(ratio.max())


def smallest_t(name, tensor):
    """the smallest power of two at which ``calibration`` stays at or below 0.5"""
    t = 1
    while calibration(name, tensor, t) > 0.5:
        t *= 2
    return t
