"""Float32 reference of the visibility-masked Adam step (include/egs_adam.h).  CPU only, numpy.

The element update is torch.optim.Adam's (no weight decay, no amsgrad) as the device code states it
(csrc/egs_adam_device.h), every product rounded to float32:
    m <- m + (g - m) (1 - b1)          v <- v b2 + g g (1 - b2)
    p <- p - lr / (1 - b1^t) * (m / (sqrt(v) / sqrt(1 - b2^t) + eps))
with 1 - b and the bias corrections derived in double and rounded once.  Rows whose mask entry is zero keep p, m and v
bit for bit, whatever their gradient row holds; ``t`` is the tensor's own step count, advanced on every call.
"""
import numpy as np

WIDTHS = (3, 3, 45, 1, 3, 4)                                  # the trainer's six groups at degree 3
LRS = (0.001, 0.001, 0.001 / 20, 0.05, 0.005, 0.001)


def masked_adam_step(p, g, m, v, step, lr, visible, beta1=0.9, beta2=0.999, eps=1e-15):
    """-> (p, m, v) after step number ``step`` (1-based); p, g, m, v: float32 [n, width], visible: [n] bool / uint8."""
    f = np.float32
    assert all(a.dtype == np.float32 for a in (p, g, m, v)) and step >= 1
    omb1, omb2, b2 = f(1.0 - beta1), f(1.0 - beta2), f(beta2)
    step_size = f(float(lr) / (1.0 - beta1 ** step))
    sqrt_bc2 = f(np.sqrt(1.0 - beta2 ** step))
    with np.errstate(all="ignore"):                            # (an invisible row's gradient may hold anything)
        m1 = m + (g - m) * omb1
        v1 = v * b2 + g * g * omb2
        denom = np.sqrt(v1) / sqrt_bc2 + f(eps)
        p1 = p - step_size * (m1 / denom)
    assert p1.dtype == m1.dtype == v1.dtype == np.float32
    keep = (np.asarray(visible).reshape(-1) != 0).reshape((-1,) + (1,) * (p.ndim - 1))
    return np.where(keep, p1, p), np.where(keep, m1, m), np.where(keep, v1, v)


def mask_shapes(n, seed=0):
    """name -> bool [n]: the mask shapes the kernels are tested on (a run needs n > 64: those are left out below it)."""
    rng = np.random.RandomState(1000 * seed + n)
    z = lambda: np.zeros(n, dtype=bool)
    out = {"none": z(), "first": z(), "last": z(), "alternating": z(), "random_half": rng.rand(n) < 0.5}
    out["first"][0] = True
    out["last"][-1] = True
    out["alternating"][::2] = True
    if n > 64:
        out["run_aligned"] = z()
        out["run_aligned"][64 * ((n // 64) // 2):][:64] = True      # one whole 64-row block (the last one may be ragged)
        out["run_straddling"] = z()
        out["run_straddling"][40:104] = True                        # 64 rows over two blocks
    return out
