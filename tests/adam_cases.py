"""Hand-built cases of the four Adam kernels (csrc/egs_adam_device.h: k_adam<false / true>, k_adam_sh_factored<NC, false /
true>) and the two references they are held to.  NumPy only; tests/test_adam_cases_cpu.py checks this table on the CPU,
tests/test_gpu_adam_rows.py runs it through the C ABI.

References
  restate     ``sparse_adam_ref.masked_adam_step``: the update in float32, operation by operation, as ``adam1`` states it.
              The kernels are held to it bit for bit.
  restate64   the same formula in float64.  With ``round_constants`` (the default) 1 - beta, beta2, eps, lr / (1 - b1^t)
              and sqrt(1 - b2^t) are the float32 values the kernels get (``adam_fill_betas`` / ``adam_bias``: derived in
              double, rounded once), so that its distance from ``restate`` is the rounding of the five float32 operations
              alone; without, every constant stays a double and the function is torch.optim.Adam's formula.

``lr`` travels through the C ABI as a float (EgsAdamGroup.lr): the double that ``adam_bias`` divides by 1 - b1^t is the
float32 value.  Every learning rate here is therefore float32-representable (``lr32``), and the references get that
value -- their arithmetic is untouched.

Element regimes.  A regime fixes (p, g, m, v) of an element and, where its name needs one, the configuration (eps, lr,
step, betas) under which it does what its name says.  ``interleaved`` deals the regimes out element by element, rotated
by one every 12 elements: a float4 holds four different regimes and every regime visits every position of a float4;
``blocks`` gives one regime to each run of 64 rows (a workgroup of the factored kernels).
"""
import numpy as np

from tests import sparse_adam_ref as R

F = np.float32
TINY = np.finfo(np.float32).tiny
CANONICAL_NAN = np.int32(0x7FC00000)


def lr32(lr):
    """The double the kernels' host side works with: ``lr`` after its trip through the ABI's float."""
    return float(F(lr))


# ------------------------------------------------------------------------------------------------------- configurations
DEFAULT = dict(eps=1e-15, lr=lr32(1e-3), step=3, betas=(0.9, 0.999))
STEPS = (1, 2, 10, 1000, 1000000)
BETAS = ((0.9, 0.999), (0.5, 0.9))


def config(**over):
    c = dict(DEFAULT)
    c.update(over)
    c["lr"] = lr32(c["lr"])
    return c


def configs():
    """name -> configuration: every step count with both beta pairs (eps alternating between the trainer's 1e-15 and
    torch's default 1e-8), and the configurations the regimes name."""
    out = {}
    for i, step in enumerate(STEPS):
        for j, betas in enumerate(BETAS):
            out["t%d_b%d" % (step, j)] = config(step=step, betas=betas, eps=(1e-15, 1e-8)[(i + j) % 2],
                                                lr=(1e-3, 5e-2, 1.6e-4)[(i + j) % 3])
    for name, (_, over) in REGIMES.items():
        if over:
            out[name] = config(**over)
    return out


# -------------------------------------------------------------------------------------------------------------- regimes
def _ordinary(rng, k):
    g = (np.where(rng.rand(k) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-6, 0, k)).astype(F)     # 1e-6 .. 1, both signs
    return rng.randn(k).astype(F), g, (rng.randn(k) * 1e-3).astype(F), (rng.rand(k) * 1e-6 + 1e-12).astype(F)


def _with(rng, k, **fixed):
    p, g, m, v = _ordinary(rng, k)
    d = dict(p=p, g=g, m=m, v=v)
    for key, val in fixed.items():
        d[key] = (val(rng, k) if callable(val) else np.full(k, val)).astype(F)
    return d["p"], d["g"], d["m"], d["v"]


_sign = lambda rng, k: np.where(rng.rand(k) < 0.5, -1.0, 1.0)

# name -> (fill(rng, k) -> (p, g, m, v) float32 [k], the configuration the regime needs beyond DEFAULT)
REGIMES = {
    "ordinary": (_ordinary, {}),
    "zero_all": (lambda r, k: _with(r, k, g=0.0, m=0.0, v=0.0), {}),
    "zero_grad_warm": (lambda r, k: _with(r, k, g=0.0), {}),
    # sqrt(v) / sqrt_bc2 is a tenth of eps at most: the update is m / eps (step 1000: sqrt_bc2 = 0.795)
    "eps_dominant": (lambda r, k: _with(r, k, g=lambda r, k: _sign(r, k) * r.uniform(0.5, 2, k) * 1e-11,
                                        m=lambda r, k: r.randn(k) * 1e-10,
                                        v=lambda r, k: r.uniform(0.5, 1.5, k) * 1e-20), dict(eps=1e-8, step=1000)),
    "subnormal_v_in": (lambda r, k: _with(r, k, g=0.0, m=lambda r, k: r.randn(k) * 1e-22,
                                          v=lambda r, k: r.uniform(0.5, 2, k) * 1e-40), {}),
    "subnormal_v_out": (lambda r, k: _with(r, k, g=lambda r, k: _sign(r, k) * r.uniform(0.7, 2, k) * 1e-20, m=0.0,
                                           v=0.0), {}),
    "overflow": (lambda r, k: _with(r, k, g=lambda r, k: _sign(r, k) * 3e19), {}),
    "inf_v_in": (lambda r, k: _with(r, k, v=np.inf), {}),
    "nan_grad": (lambda r, k: _with(r, k, g=np.nan), {}),
    "inf_grad": (lambda r, k: _with(r, k, g=lambda r, k: _sign(r, k) * np.inf), {}),
    "neg_zero_p": (lambda r, k: _with(r, k, p=-0.0, g=0.0, m=0.0), {}),
    "lr0": (_ordinary, dict(lr=0.0)),
}
NAMES = tuple(REGIMES)
NREG = len(NAMES)
assert NREG % 4 == 0          # a float4 starts at a multiple of 4: (e + e // NREG) % NREG is four different regimes in it


def regime_config(name):
    return config(**REGIMES[name][1])


def regime_alone(name, k, seed=0):
    """-> (p, g, m, v) float32 [k], every element of the one regime"""
    return REGIMES[name][0](np.random.RandomState(7919 * seed + NAMES.index(name)), k)


def interleaved_ids(count):
    e = np.arange(count)
    return (e + e // NREG) % NREG


def block_ids(n, shift=0):
    return (np.arange(n) // 64 + shift) % NREG


def fill(ids, seed=0):
    """ids: int [...] regime numbers -> (p, g, m, v) float32 of ids' shape.  The same ids and seed give the same values; a
    different seed keeps every element in its regime with fresh magnitudes (the gradients of a later step)."""
    ids = np.asarray(ids)
    out = [np.empty(ids.shape, F) for _ in range(4)]
    for r, name in enumerate(NAMES):
        sel = ids == r
        k = int(sel.sum())
        if k:
            for dst, src in zip(out, REGIMES[name][0](np.random.RandomState(104729 * seed + 31 * r + ids.size % 97), k)):
                dst[sel] = src
    return tuple(out)


def fill_interleaved(count, seed=0):
    return fill(interleaved_ids(count), seed)


def fill_blocks(n, width, seed=0, shift=0):
    """[n, width]: one regime per run of 64 rows, starting with regime number ``shift``"""
    return fill(np.repeat(block_ids(n, shift)[:, None], width, 1), seed)


# ----------------------------------------------------------------------------------------------------------- references
def restate(p, g, m, v, cfg, visible=None):
    """The float32 restatement under a configuration -> (p, m, v); visible None: every row."""
    rows = p.shape[0] if p.ndim else 1
    p2 = p.reshape(rows, p.size // rows if rows else 0)              # (an empty record stays empty)
    vis = np.ones(p2.shape[0], bool) if visible is None else visible
    out = R.masked_adam_step(p2, g.reshape(p2.shape), m.reshape(p2.shape), v.reshape(p2.shape), cfg["step"], cfg["lr"],
                             vis, cfg["betas"][0], cfg["betas"][1], cfg["eps"])
    return tuple(x.reshape(p.shape) for x in out)


def restate64(p, g, m, v, cfg, visible=None, round_constants=True):
    """The same formula in float64 -> (p, m, v) float64."""
    beta1, beta2 = cfg["betas"]
    step, lr, eps = cfg["step"], float(cfg["lr"]), float(cfg["eps"])
    omb1, omb2, b2 = 1.0 - beta1, 1.0 - beta2, float(beta2)
    step_size, sqrt_bc2 = lr / (1.0 - beta1 ** step), float(np.sqrt(1.0 - beta2 ** step))
    if round_constants:
        omb1, omb2, b2, eps, step_size, sqrt_bc2 = (float(F(x)) for x in (omb1, omb2, b2, eps, step_size, sqrt_bc2))
    p, g, m, v = (np.asarray(x, np.float64) for x in (p, g, m, v))
    with np.errstate(all="ignore"):
        m1 = m + (g - m) * omb1
        v1 = v * b2 + g * g * omb2
        p1 = p - step_size * (m1 / (np.sqrt(v1) / sqrt_bc2 + eps))
    if visible is not None:
        keep = (np.asarray(visible).reshape(-1) != 0).reshape((-1,) + (1,) * (p.ndim - 1))
        p1, m1, v1 = np.where(keep, p1, p), np.where(keep, m1, m), np.where(keep, v1, v)
    return p1, m1, v1


def bits(a):
    """float32 array -> int32 bit patterns, every NaN as the one canonical quiet NaN: hardware differs in the sign and
    payload of the NaN an invalid operation yields (x86 gives 0xFFC00000, the GPU 0x7FC00000), in nothing else.  A NaN
    still has to sit in the same ELEMENT on both sides."""
    a = np.ascontiguousarray(a, F)
    return np.where(np.isnan(a), CANONICAL_NAN, a.view(np.int32))


def first_difference(got, want):
    """None if bit-equal (``bits``), else a description of the first differing element"""
    a, b = bits(got).reshape(-1), bits(want).reshape(-1)
    if a.shape != b.shape:
        return "shapes %s / %s" % (np.shape(got), np.shape(want))
    bad = np.flatnonzero(a != b)
    if bad.size == 0:
        return None
    i = int(bad[0])
    return "%d of %d elements differ, first at flat index %d: got 0x%08x (%r), want 0x%08x (%r)" % (
        bad.size, a.size, i, int(a[i]) & 0xFFFFFFFF, float(np.reshape(got, -1)[i]), int(b[i]) & 0xFFFFFFFF,
        float(np.reshape(want, -1)[i]))


# -------------------------------------------------------------------------------------------------------------- layouts
PER_BLOCK = 1024                                                # floats per workgroup of k_adam (ADAM_PER_BLOCK)
COUNTS = (1, 2, 3, 4, 5, 7, 8, 1023, 1024, 1025, 2049)         # one-group launches of the dense kernel, in floats
LAUNCH8 = (1, 1024, 3, 1025, 0, 4, 2047, 5)                    # one launch, 8 records; the 0 for the dense entry point only
LAUNCH8_MASKED_WIDTHS = (1, 2, 3, 4, 5, 7, 9, 45)              # the masked entry point: 8 groups at one row count
FUSED12 = ((1, 1024, 3, 1025), (5, 4, 2047, 7), (8, 2, 1023, 2049))     # FusedAdam: 3 groups x 4 tensors, two launches
WIDTHS = (1, 2, 3, 4, 5, 7, 9, 45, 48)
ROWS = (1, 2, 63, 64, 65, 255, 257, 1031)
SH_DIMS = (3, 12, 27, 48)
SH_ROWS = (1, 63, 64, 65, 130)


def masks(n, width):
    """name -> bool [n]: the seven shapes of ``sparse_adam_ref.mask_shapes`` (the two runs need n > 64), every row, and
    every row whose index is 1 mod width + 1 -- the boundary between a visible and an invisible row then moves through
    every position of a float4."""
    out = dict(R.mask_shapes(n))
    out["all"] = np.ones(n, bool)
    out["mod"] = np.arange(n) % (width + 1) == 1
    return out


def sh_masks(n):
    """the masks of the factored pair: ``masks`` at width 3 and, from 65 rows on, one whole 64-row workgroup invisible"""
    out = masks(n, 3)
    if n > 64:
        out["workgroup_out"] = np.ones(n, bool)
        out["workgroup_out"][64 * ((n - 1) // 64 - 1):][:64] = False        # the last FULL workgroup before the ragged one
    return out


def dense_branches(count):
    """the branches of k_adam<false> a group of ``count`` floats takes"""
    out = set()
    if count >= 4:
        out.add("float4")
    if count % 4:
        out.add("tail%d" % (count % 4))
    if count and count % PER_BLOCK == 0:
        out.add("ends_on_workgroup")
    if count % PER_BLOCK == 1 and count > 1:
        out.add("one_past_workgroup")
    if count > PER_BLOCK:
        out.add("blocks>1")
    return out


def masked_branches(n, width):
    """the branches of k_adam<true> on an [n][width] tensor: ``dense_branches`` of its n width floats, the positions in a
    float4 at which a row starts (``boundary0`` .. ``boundary3``: the walk's ``++rem == width`` at q = 3, 0, 1, 2), a
    float4 with more than two rows, and a row boundary inside the ragged tail"""
    count = n * width
    out = dense_branches(count)
    starts = np.arange(1, n) * width
    for q in sorted(set((starts % 4).tolist())):
        out.add("boundary%d" % q)
    if width == 1 and n >= 4:
        out.add("four_rows_in_float4")
    if count % 4 and np.any(starts > count - count % 4):
        out.add("boundary_in_tail")
    if width > 4 and np.any((starts % 4 != 0) & (starts < count - count % 4)):
        out.add("wide_row_ends_mid_float4")
    return out
