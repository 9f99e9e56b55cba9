"""NumPy restatement of MCMC densification (include/egs_mcmc.h sections 1-5), written from the formulas, for the tests
of libegs_mcmc.so.  Everything is evaluated in ``dtype`` (float64: the reference; float32: the same formulas at the
precision of the tensors, whose distance from the float64 result sets the tests' tolerances).  The random streams are
``scene.uniform01`` / ``scene.normal``."""
import math

import numpy as np

from easygaussiansplatting_amd import scene as S

STREAM_SAMPLE = 1 << 62
STREAM_NOISE = 1 << 40
N_MAX = 51


def sigmoid(x, dtype=np.float64):
    x = np.asarray(x, dtype)
    return (1 / (1 + np.exp(-x))).astype(dtype)


def weights(alphas_raw, min_opacity, relocation):
    """-> weight (float32, as the kernel stores it), dead (bool), (n_dead, n_live).  The opacity is the float32 sigmoid
    of the kernel: a row within an ulp of ``min_opacity`` may be classified either way, tests keep away from it."""
    o = sigmoid(np.asarray(alphas_raw).reshape(-1), np.float32)
    dead = o <= np.float32(min_opacity)
    w = np.where(dead, np.float32(0), o) if relocation else o
    return w.astype(np.float32), dead, (int(dead.sum()), int((~dead).sum()))


def cdf(weight):
    """inclusive prefix sum in float64 (sequential order; exact -- and so order-independent -- for the tests' weights)"""
    return np.cumsum(np.asarray(weight, np.float64))


def sample(weight, n_draws, seed, rnd):
    c = cdf(weight)
    u = S.uniform01(seed, STREAM_SAMPLE + rnd, (n_draws,))
    return np.searchsorted(c, u * c[-1], side="right").astype(np.int64)


def corrected(o, s, count, min_opacity, dtype=np.float64):
    """(o [M], s [M,3], count [M]) -> activated (o', s') of every copy; count = 1 + the number of draws of the row"""
    o = np.asarray(o, dtype).reshape(-1)
    s = np.asarray(s, dtype).reshape(-1, 3)
    N = np.minimum(np.asarray(count).reshape(-1), N_MAX).astype(np.int64)
    one = dtype(1)
    on = (one - (one - o) ** (one / N.astype(dtype))).astype(dtype)
    D = np.zeros_like(o)
    for i in range(1, N_MAX + 1):
        use = N >= i
        if not use.any():
            break
        for k in range(i):
            term = (dtype(math.comb(i - 1, k)) * dtype((-1) ** k) / np.sqrt(dtype(k + 1)) * on ** dtype(k + 1)).astype(dtype)
            D = np.where(use, D + term, D).astype(dtype)
    s_new = (s * (o / D)[:, None]).astype(dtype)
    o_new = np.clip(on, dtype(min_opacity), dtype(1 - 1e-6)).astype(dtype)
    return o_new, s_new


def counts(src, n_rows):
    return 1 + np.bincount(np.asarray(src, np.int64), minlength=n_rows)


def relocate(params, src, dst, min_opacity, dtype=np.float64):
    """params: dict of raw arrays.  -> dict with the ACTIVATED opacity ``o`` [n] and scale ``s`` [n,3] after the move
    (rows neither drawn nor written keep their activated values) and the copied tensors."""
    n = params["pws"].shape[0]
    cnt = counts(src, n)
    o = sigmoid(params["alphas_raw"].reshape(-1), dtype)
    s = np.exp(np.asarray(params["scales_raw"], dtype)).astype(dtype)
    drawn = np.nonzero(cnt > 1)[0]
    o_c, s_c = corrected(o[drawn], s[drawn], cnt[drawn], min_opacity, dtype)
    o_out, s_out = o.copy(), s.copy()
    o_out[drawn], s_out[drawn] = o_c, s_c
    o_out[dst], s_out[dst] = o_out[src], s_out[src]
    out = {"o": o_out, "s": s_out, "drawn": drawn}
    for k in ("pws", "low_shs", "high_shs", "rots_raw"):
        a = params[k].copy()
        a[dst] = a[src]
        out[k] = a
    return out


def reg_grad(alphas_raw, scales_raw, lam_o, lam_s, dtype=np.float64):
    n = alphas_raw.shape[0]
    o = sigmoid(alphas_raw, dtype)
    s = np.exp(np.asarray(scales_raw, dtype)).astype(dtype)
    return (dtype(lam_o) / dtype(n) * o * (dtype(1) - o)).astype(dtype), (dtype(lam_s) / dtype(3 * n) * s).astype(dtype)


def rotation(q, dtype=np.float64):
    q = np.asarray(q, dtype)
    q = q / np.linalg.norm(q, axis=1, keepdims=True).astype(dtype)
    w, x, y, z = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                  2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                  2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1)
    return R.reshape(-1, 3, 3).astype(dtype)


def noise_delta(alphas_raw, scales_raw, rots_raw, z, noise_lr, lr_pws, dtype=np.float64):
    """displacement of pws [n,3]"""
    o = sigmoid(alphas_raw.reshape(-1), dtype)
    w = (dtype(1) / (dtype(1) + np.exp(-dtype(100) * ((dtype(1) - o) - dtype(0.995))))).astype(dtype)
    s = np.exp(np.asarray(scales_raw, dtype)).astype(dtype)
    R = rotation(rots_raw, dtype)
    cov = np.einsum("nij,nj,nkj->nik", R, s * s, R).astype(dtype)
    v = (np.asarray(z, dtype) * w[:, None] * dtype(noise_lr) * dtype(lr_pws)).astype(dtype)
    return np.einsum("nik,nk->ni", cov, v).astype(dtype)


def unit_noise(seed, step, n):
    return S.normal(seed, STREAM_NOISE + step, (n, 3))
