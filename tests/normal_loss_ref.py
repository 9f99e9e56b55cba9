"""The normal loss of include/egs_normalloss.h stated in torch: float64 by default, with its gradient from
autograd, and with ``dtype=torch.float32`` the same code as a float32 restatement, which measures what float32 arithmetic
loses on a case.  Plus the case generator and the comparison rule of the GPU tests (tests/test_gpu_normal_loss.py),
which tests/test_normal_loss_cpu.py exercises without a GPU.

The rule is the project's own (tests/depth_loss_ref.py): a GPU result is held to 4 x the error of the float32 restatement
on that case, with a floor of one float32 ulp of the quantity's largest entry; for the two losses the floor is 2^-23 (each
term is a difference from 1, so a loss that is zero but for rounding -- "plane", L_s -- is not known any finer).  The set
of pixels with a normal must EQUAL the reference's, and stats[4], Omega_p and Omega_s agree accordingly: no pixel is
left out.
"""
import numpy as np
import torch

KINDS = ("noise", "plane", "wavy")
ALPHA_MIN = 0.05
EDGE_GAMMA = 10.0
LOSS_FLOOR = 2.0 ** -23
STATS = ("Lp", "Ls", "Op", "Os", "count")


def intrinsics(H, W):
    """an off-centre principal point, a focal length of the order of the image"""
    f = 1.2 * max(H, W, 4)
    return (f, 1.1 * f, 0.5 * W + 0.7, 0.5 * H - 1.3)


def make_case(H, W, kind, seed=0):
    """-> float32 dict(D, A, q [3,H,W], I [3,H,W], w [H,W]) and cam = (fx, fy, cx, cy).  Depths of the three kinds seen
    with opacity A ~ U(0.06, 1), 3 % of the pixels at 0.01 (below alpha_min); D = A z; random unit priors of which 10 %
    are missing (zeros); a uniform-noise guide; uniform weights."""
    assert kind in KINDS
    rng = np.random.default_rng([seed, H, W, KINDS.index(kind)])
    cam = intrinsics(H, W)
    fx, fy, cx, cy = cam
    X = (np.arange(W)[None, :] - cx) / fx + np.zeros((H, 1))
    Y = (np.arange(H)[:, None] - cy) / fy + np.zeros((1, W))
    if kind == "noise":
        z = rng.uniform(0.5, 20.0, (H, W))
    elif kind == "plane":
        z = 4.0 / (1.0 + 0.4 * X - 0.25 * Y)
    else:
        z = 6.0 + 1.5 * np.sin(7 * X) * np.cos(5 * Y) + rng.normal(0.0, 0.01, (H, W))
    A = rng.uniform(0.06, 1.0, (H, W))
    A[rng.random((H, W)) < 0.03] = 0.01
    q = rng.normal(0.0, 1.0, (3, H, W))
    q[2] = -np.abs(q[2]) - 0.2
    q /= np.sqrt((q * q).sum(0, keepdims=True))
    q[:, rng.random((H, W)) < 0.1] = 0.0
    I = rng.uniform(0.0, 1.0, (3, H, W))
    w = rng.uniform(0.0, 2.0, (H, W))
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    return dict(D=f32(A * z), A=f32(A), q=f32(q), I=f32(I), w=f32(w)), cam


def _t(a, dtype):
    return None if a is None else torch.as_tensor(np.asarray(a)).to(dtype)


def forward(D, A, cam, q=None, I=None, w=None, smooth=True, alpha_min=ALPHA_MIN, edge_gamma=EDGE_GAMMA,
            dtype=torch.float64):
    """The definition on torch tensors ``D``, ``A`` of ``dtype`` (leaves with requires_grad for a gradient), on their
    device.
    -> dict(Lp, Ls, Op, Os, count, flags, n [3,H,W], nvalid [H,W] bool, dvalid [H,W] bool); Lp, Ls are tensors."""
    T, dev = dtype, D.device
    H, W = D.shape
    fx, fy, cx, cy = (torch.tensor(float(v), dtype=T, device=dev) for v in cam)
    dvalid = (A > torch.tensor(np.float32(alpha_min).item(), dtype=A.dtype, device=dev)) & (D > 0)
    z = torch.where(dvalid, D / torch.where(dvalid, A, torch.ones_like(A)), torch.ones_like(D))
    xs = torch.arange(W, dtype=T, device=dev)[None, :].expand(H, W)
    ys = torch.arange(H, dtype=T, device=dev)[:, None].expand(H, W)
    p = torch.stack([z * ((xs - cx) / fx), z * ((ys - cy) / fy), z])
    zero = torch.zeros((), dtype=T, device=dev)
    out = dict(Lp=zero, Ls=zero, Op=0.0, Os=0.0, count=0, flags=0, n=torch.zeros((3, H, W), dtype=T, device=dev),
               nvalid=torch.zeros((H, W), dtype=torch.bool, device=dev), dvalid=dvalid)
    if H >= 3 and W >= 3:
        dx = p[:, 1:-1, 2:] - p[:, 1:-1, :-2]
        dy = p[:, 2:, 1:-1] - p[:, :-2, 1:-1]
        c = torch.cross(dy, dx, dim=0)
        c2 = (c * c).sum(0)
        five = dvalid[1:-1, 1:-1] & dvalid[1:-1, 2:] & dvalid[1:-1, :-2] & dvalid[2:, 1:-1] & dvalid[:-2, 1:-1]
        nv = five & (c2 > 0) & torch.isfinite(c2)
        n_in = torch.where(nv, c / torch.sqrt(torch.where(nv, c2, torch.ones_like(c2))), torch.zeros_like(c))
        n = torch.nn.functional.pad(n_in, (1, 1, 1, 1))
        nvalid = torch.nn.functional.pad(nv, (1, 1, 1, 1))
        out.update(n=n, nvalid=nvalid, count=int(nvalid.sum()))
    n, nvalid = out["n"], out["nvalid"]
    om = torch.where(nvalid, torch.ones((H, W), dtype=T, device=dev) if w is None else w.to(T),
                     torch.zeros((H, W), dtype=T, device=dev))
    if q is not None:
        q = q.to(T)
        q2 = (q * q).sum(0)
        data = torch.isfinite(q).all(0) & (q2 > 0) & torch.isfinite(q2)
        qh = torch.where(data, q / torch.sqrt(torch.where(data, q2, torch.ones_like(q2))), torch.zeros_like(q))
        omp = torch.where(data, om, torch.zeros_like(om))
        Op = omp.sum()
        if float(Op) > 0:
            out.update(Lp=(omp * (1 - (n * qh).sum(0))).sum() / Op, Op=float(Op))
        else:
            out["flags"] |= 1
    if smooth:
        num, Os = zero, zero
        for sl_a, sl_b in (((slice(None), slice(0, -1)), (slice(None), slice(1, None))),
                           ((slice(0, -1), slice(None)), (slice(1, None), slice(None)))):
            oo = om[sl_a] * om[sl_b]
            g = 1.0
            if I is not None:
                Ia, Ib = I.to(T)[(slice(None),) + sl_a], I.to(T)[(slice(None),) + sl_b]
                g = torch.exp(-torch.tensor(np.float32(edge_gamma).item(), dtype=T, device=dev) * (Ia - Ib).abs().mean(0))
            dot = (n[(slice(None),) + sl_a] * n[(slice(None),) + sl_b]).sum(0)
            num = num + (oo * g * (1 - dot)).sum()
            Os = Os + oo.sum()
        if float(Os) > 0:
            out.update(Ls=num / Os, Os=float(Os))
        else:
            out["flags"] |= 2
    return out


def ref(case, cam, prior=True, guide=True, smooth=True, weighted=False, alpha_min=ALPHA_MIN, edge_gamma=EDGE_GAMMA,
        prior_scale=1.0, smooth_scale=1.0, dtype=torch.float64):
    """-> dict(Lp, Ls, Op, Os, count, flags (floats / ints), n [3,H,W], nvalid, dvalid, dD, dA [H,W]) as numpy: the loss
    prior_scale L_p + smooth_scale L_s and its gradient by autograd, exactly 0 at pixels that are not depth-valid."""
    D = _t(case["D"], dtype).requires_grad_(True)
    A = _t(case["A"], dtype).requires_grad_(True)
    o = forward(D, A, cam, _t(case["q"], dtype) if prior else None, _t(case["I"], dtype) if guide else None,
                _t(case["w"], dtype) if weighted else None, smooth, alpha_min, edge_gamma, dtype)
    total = prior_scale * o["Lp"] + smooth_scale * o["Ls"]
    if total.requires_grad:
        dD, dA = torch.autograd.grad(total, [D, A], allow_unused=True)
    else:
        dD = dA = None
    res = dict(o)
    dv = o["dvalid"]
    for k, g in (("dD", dD), ("dA", dA)):
        g = torch.zeros_like(D) if g is None else g.detach()
        res[k] = torch.where(dv, g, torch.zeros_like(g)).numpy()
    res.update(Lp=float(o["Lp"].detach()), Ls=float(o["Ls"].detach()), n=o["n"].detach().numpy(), nvalid=o["nvalid"].numpy(),
               dvalid=dv.numpy())
    return res


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def errors(got, want):
    """``got``: dict(Lp, Ls, Op, Os, count, n, dD, dA) -- the float32 restatement or a kernel's result -- against the
    float64 ``want`` -> dict of absolute errors (arrays: the largest)."""
    e = {k: abs(float(got[k]) - float(want[k])) for k in STATS}
    for k in ("n", "dD", "dA"):
        if got.get(k) is not None:
            e[k] = float(np.abs(np.asarray(got[k], np.float64) - want[k]).max())
    return e


def bounds(e_ref, want):
    """what a kernel's errors are held to: 4 x the float32 restatement's, at least one float32 ulp of the largest entry
    (the two losses: at least 2^-23)"""
    b = {k: max(4.0 * e_ref[k], ulp32(want[k])) for k in ("Op", "Os")}
    b["count"] = 0.0
    for k in ("Lp", "Ls"):
        b[k] = max(4.0 * e_ref[k], LOSS_FLOOR)
    for k in ("n", "dD", "dA"):
        b[k] = max(4.0 * e_ref[k], ulp32(float(np.abs(want[k]).max())))
    return b


def check_against(got, want, what, e_ref):
    """assert the rule; -> (errors, bounds) for a report.  ``e_ref``: the float32 restatement's errors on this case."""
    if got.get("nvalid") is not None:
        assert np.array_equal(np.asarray(got["nvalid"], bool), want["nvalid"]), "%s: the set of pixels with a normal differs" % what
    e, b = errors(got, want), bounds(e_ref, want)
    for k in e:
        assert np.isfinite(e[k]) and e[k] <= b[k], "%s: %s off by %.3e, bound %.3e (float32 restatement %.3e)" % (
            what, k, e[k], b[k], e_ref[k])
    assert int(got["flags"]) == want["flags"], what
    return e, b
