"""Per-Gaussian blend-weight statistics and importance-based pruning (include/egs_prune.h).

The forward draw pass forms the blending weight ``w = tau alpha'`` of every (pixel, list entry) pair and keeps only the
image.  ``egs_blend_weights`` (libegs_prune.so) walks the tile lists of a finished forward pass again, bounded by its
``contrib``, and accumulates per Gaussian the sum of ``w`` (Mini-Splatting's score), its maximum (RadSplat's) and the
number of pixels hit (LightGaussian's):

    st = BlendStats(n, device)
    for cam in cameras:
        render_weights(st, pws, shs, alphas, scales, rots, cam)       # one fused forward + one walk per view
    keep = keep_mask(st, score="max", threshold=0.01)
    density_control.prune(params, optimizer, keep)

``max`` and ``hits`` are bitwise reproducible; ``sum`` is a float atomic add per (tile, Gaussian) and reproducible only
when every Gaussian lies on one tile of one view.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _prunelib
from ._host import _pol, _ptr, _splat_lists, _state_lists, _stream

SCORES = ("max", "sum", "hits")


class BlendStats:
    """``rows`` float32 [N,4], zeroed: sum | max | hits (int32 bits) | reserved (stays 0).  ``sum`` / ``max`` / ``hits``
    are views of it; ``views`` counts the renders accumulated (host side)."""

    def __init__(self, n: int, device="cuda"):
        self.rows = torch.zeros((int(n), 4), dtype=torch.float32, device=device)
        self.views = 0

    @property
    def n(self):
        return self.rows.shape[0]

    @property
    def sum(self):
        return self.rows[:, 0]

    @property
    def max(self):
        return self.rows[:, 1]

    @property
    def hits(self):
        return self.rows.view(torch.int32)[:, 2]

    def zero_(self):
        self.rows.zero_()
        self.views = 0
        return self

    def merge_(self, other: "BlendStats"):
        """add the sums and hits of ``other``, take the larger max"""
        if other.rows.shape != self.rows.shape:
            raise ValueError("BlendStats.merge_: %d rows against %d" % (self.n, other.n))
        o = other.rows.to(self.rows.device)
        self.sum.add_(o[:, 0])
        torch.maximum(self.max, o[:, 1], out=self.max)
        self.hits.add_(o.view(torch.int32)[:, 2])
        self.views += other.views
        return self

    def allreduce_(self, group=None):
        """sum and hits added, max taken over the ranks of ``group``: every rank ends with the same bits.  A no-op when
        ``torch.distributed`` is not initialised.  Works on CPU tensors over gloo."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            return self
        s, m, h = self.sum.contiguous(), self.max.contiguous(), self.hits.contiguous()
        v = torch.tensor([self.views], dtype=torch.int64, device=self.rows.device)
        dist.all_reduce(s, op=dist.ReduceOp.SUM, group=group)
        dist.all_reduce(m, op=dist.ReduceOp.MAX, group=group)
        dist.all_reduce(h, op=dist.ReduceOp.SUM, group=group)
        dist.all_reduce(v, op=dist.ReduceOp.SUM, group=group)
        self.sum.copy_(s); self.max.copy_(m); self.hits.copy_(h)
        self.views = int(v.item())
        return self


def _stats_for(stats, n, device):
    if stats is None:
        return BlendStats(n, device)
    if not isinstance(stats, BlendStats):
        raise TypeError("stats must be a BlendStats, got %s" % type(stats).__name__)
    r = stats.rows
    if not (r.is_cuda and r.device == device and r.dtype == torch.float32 and r.is_contiguous() and
            tuple(r.shape) == (n, 4)):
        raise ValueError("stats.rows must be a contiguous float32 [%d, 4] tensor on %s" % (n, device))
    return stats


def _accumulate(n, W, H, rec, ranges, gsid, contrib, flags, stats):
    lib = _prunelib.load()
    _prunelib.check(lib.egs_blend_weights(n, W, H, _ptr(rec), C.byref(_pol()), _ptr(ranges), _ptr(gsid), _ptr(contrib),
                                          flags, _ptr(stats.rows), _stream()))
    stats.views += 1
    return stats


def from_state(state, stats: BlendStats = None) -> BlendStats:
    """Accumulate the statistics of one fused render: ``state`` is the ``fused.FusedState`` of
    ``fused.forward(..., need_grad=False)`` under the current raster policy.  Settles the render's ticket, then walks
    its own records and lists on the current stream.  Anti-aliased and raw states work unchanged (the kernel reads
    the packed records)."""
    lists = _state_lists(state)
    return _accumulate(*lists, _stats_for(stats, lists[0], state.depths.device))


@torch.no_grad()
def render_weights(stats, pws, shs, alphas, scales, rots, cam, high_shs=None, antialiased=False) -> BlendStats:
    """One ``fused.forward`` of ``cam`` plus ``from_state``: the statistics of that view are added to ``stats`` (None: a
    fresh ``BlendStats``).  Arguments as ``fused.forward`` (with ``high_shs``: the raw training tensors)."""
    from . import fused
    out = fused.forward(pws, shs, alphas, scales, rots, cam, high_shs=high_shs, need_grad=False,
                        antialiased=antialiased)
    return from_state(out[2], stats)


@torch.no_grad()
def splat_weights(H, W, us, cinv2ds, alphas, depths, contrib, ranges, gsid, areas=None, stats=None) -> BlendStats:
    """The statistics of one ``gsplatcu.splat`` under the current policy, from its inputs and its outputs ``contrib``,
    ``patch_range_per_tile`` and ``gsid_per_patch`` (plain lists).  ``areas`` ([N,2] int32, as ``splat`` left them) is
    needed under the pixel-box policy, as for ``splatB``."""
    lists = _splat_lists(H, W, us, cinv2ds, alphas, depths, contrib, ranges, gsid, areas, "splat_weights")
    return _accumulate(*lists, _stats_for(stats, lists[0], us.device))


def keep_mask(stats: BlendStats, score: str = "max", threshold=None, fraction=None) -> torch.Tensor:
    """-> bool [N].  ``threshold``: keep the rows with ``score >= threshold``.  ``fraction``: drop that share of the
    rows, floor(fraction N) of them, with the lowest score; ties go by index (the lower index is dropped first).
    Exactly one of the two must be given."""
    if score not in SCORES:
        raise ValueError("keep_mask: unknown score %r (expected one of %s)" % (score, ", ".join(SCORES)))
    if (threshold is None) == (fraction is None):
        raise ValueError("keep_mask: give exactly one of threshold / fraction")
    s = getattr(stats, score)
    if threshold is not None:
        return s >= threshold
    fraction = float(fraction)
    if not 0.0 <= fraction <= 1.0:
        raise ValueError("keep_mask: fraction must lie in [0, 1], got %r" % (fraction,))
    n = s.shape[0]
    drop = int(fraction * n)
    keep = torch.ones(n, dtype=torch.bool, device=s.device)
    if drop > 0:
        order = torch.sort(s, stable=True).indices
        keep[order[:drop]] = False
    return keep
