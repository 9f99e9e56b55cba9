"""Per-device render scheduling shared by ``fused.forward`` and the seven-op ``splat``: the page-locked mailbox, what
was learnt about each problem size (patch-list capacity, significant depth-key bits, how far tile lists are walked),
the renders awaiting validation -- and the enqueue-ahead protocol on that state, ``render``.

The A/B knobs that steer it (``fused.SEGMENTS``, ``fused.SEG_SPECULATE``, ``fused.ENQUEUE_AHEAD``,
``fused.MAILBOX_COPY``) stay module attributes of ``fused``; their values arrive here as arguments."""
from __future__ import annotations

import collections
import ctypes as C
import threading

import torch

from . import _lib
from ._host import _ptr

MAILBOX_SLOTS = 64
HINT_SLOTS = 16           # problem sizes that keep a hint slot (longest list / longest walk of their recent renders)
SIZE_TABLE_MAX = 1024     # problem sizes (N, W, H) a process remembers a patch capacity / depth-key hint for


class _Ticket:
    """One enqueue-ahead render whose {P, max depth key} read-back is still in flight."""
    __slots__ = ("ctx", "slot", "key", "cap", "hint", "state", "status", "patches", "need", "collected")
    PENDING, OK, FAILED = 0, 1, 2


class _DeviceCtx:
    """Per-device host state of the render paths: the mailbox, what was learnt about each problem size
    (patch-list capacity, significant depth-key bits) and the renders awaiting validation.  Nothing here
    is shared between devices; access is serialised by ``lock`` (autograd runs backward on its own thread)."""

    def __init__(self, lib, index):
        self.index = index
        self.lib = lib
        self.mb = lib.egs_mailbox_create(MAILBOX_SLOTS)
        if not self.mb:
            raise RuntimeError("egs_mailbox_create failed (page-locked host memory)")
        self.free = list(range(MAILBOX_SLOTS))
        self.pending = collections.deque()
        self.failed = []
        self.capacity = {}      # (N, W, H) -> patch-list allocation size learnt from earlier renders
        # (camera, stream) -> (weakref, its [order | work] buffer, renders so far, problem size): the dispatch order
        # of the tiles is kept between the renders of a camera (a trainer meets every view again each epoch)
        self.tile_work = {}
        self.seg_hint = {}      # (N, W, H) -> mailbox slot kept as the landing zone of "longest list of the last render"
        # ((N, W, H), stream) -> one persistent int32 device word (-1 = nothing gathered): the draw items of a render
        # gather its longest walk there, the next render on that stream publishes it into the hint slot (egs_hip.h)
        self.walk_word = {}
        self.long_walks_expected = 0   # renders for which a caller announced long walks (expect_long_walks)
        self.lock = threading.RLock()


_contexts = {}
_tls = threading.local()     # .deferred: inside a ``deferred()`` block (a real per-thread context)


def _ctx(dev) -> _DeviceCtx:
    c = _contexts.get(dev.index)
    if c is None:
        c = _contexts.setdefault(dev.index, _DeviceCtx(_lib.load(), dev.index))
    return c


def _grow(p):
    return p + p // 16 + 4096


def _learn_capacity(ctx, key, patches):
    """Raise the enqueue-ahead patch capacity of a problem size (ctx.lock held by the caller or not needed: one dict
    store); the table is bounded -- a process that meets ever new sizes (a densifying trainer: one per densification; a
    server rendering many scenes) forgets the sizes it met first."""
    cap = ctx.capacity
    val = max(cap.pop(key, 0), _grow(min(patches, 2**31 - 1)))
    cap[key] = val                                      # (re-inserted: most recently learnt)
    while len(cap) > SIZE_TABLE_MAX:
        cap.pop(next(iter(cap)), None)


_key_bits = {}   # (device index, problem key) -> significant depth-key bits learnt from the previous call
_key_low = {}    # (device index, problem key) -> [renders in a row that needed fewer bits, the most they needed]
KEY_BITS_DECAY = 32   # renders in a row with a smaller need before the hint is lowered


def _get_key_bits(dev_index, key=None) -> int:
    return _key_bits.get((dev_index, key), 32)


def _set_key_bits(dev_index, key, bits) -> None:
    _key_bits[(dev_index, key)] = int(bits)
    _key_low.pop((dev_index, key), None)


def _learn_key_bits(dev_index, key, need, missed=False) -> None:
    """Update the depth-key bit hint of a problem size from one render's largest key (``need`` bits).
    The hint is shared by all cameras that render this problem size, so it follows a slowly decaying MAXIMUM:
    raised at once, lowered only after KEY_BITS_DECAY renders in a row needed less (to the most they needed) --
    cameras whose depth ranges differ by a bit or two then never miss, where "need + 1 after every success"
    made them alternate between a miss (a redone step under deferred validation) and a reset.  A miss sets
    the hint to 32 for the redo; the first success after that adopts need + 1."""
    k = (dev_index, key)
    target = min(32, int(need) + 1)
    while len(_key_bits) > 1024:          # (bounded like the capacity table: SIZE_TABLE_MAX)
        old = next(iter(_key_bits))
        _key_bits.pop(old, None)
        _key_low.pop(old, None)
    if missed:
        _key_bits[k] = 32
        _key_low.pop(k, None)
        return
    hint = _key_bits.get(k, 32)
    if hint >= 32 or target >= hint:
        _key_bits[k] = target
        _key_low.pop(k, None)
        return
    low = _key_low.setdefault(k, [0, 0])
    low[0] += 1
    low[1] = max(low[1], target)
    if low[0] >= KEY_BITS_DECAY:
        _key_bits[k] = low[1]
        _key_low.pop(k, None)


def _bin_stage(enqueue, device, key=None):
    """Run the binning stage with the depth-key bit-count hint protocol of egs_splat_bin:
    ``enqueue(hint, total, None)`` enqueues the stage; returns the patch count P.  The single
    8-byte read-back (reference: gausplat.cu:67) also brings the largest depth key, which
    sizes the next call's sort (depth keys rarely need more than 16 of their 32 bits; the hint is kept
    per device and problem ``key``); a too-small hint triggers one full-width re-run."""
    total = torch.empty(2, dtype=torch.int32, device=device)
    hint = _get_key_bits(device.index, key)
    enqueue(hint, total, None)
    p, mk = (int(v) & 0xFFFFFFFF for v in total.tolist())
    need = mk.bit_length()
    if hint < 32 and need > hint:
        enqueue(32, total, None)
        p, mk = (int(v) & 0xFFFFFFFF for v in total.tolist())
    _learn_key_bits(device.index, key, need)
    if p >= 2**31:
        raise RuntimeError("splat: %d tile patches overflow int32 indexing" % p)
    return p


def _settle(t: _Ticket, blocking: bool) -> bool:
    """Look at the read-back of one render: True once it has been validated (either way)."""
    ctx = t.ctx
    with ctx.lock:
        if t.status != _Ticket.PENDING:
            return True
        out = (C.c_uint32 * 2)()
    rc = ctx.lib.egs_mailbox_fetch(ctx.mb, t.slot, 1 if blocking else 0, out)   # (the wait holds no lock, no GIL)
    if rc == 0:
        return False
    if rc < 0:
        # the slot never received its values (a HIP error behind the binning stage): the ticket is settled as
        # FAILED and its slot handed back, so that later commit() calls do not trip over it again
        with ctx.lock:
            if t.status == _Ticket.PENDING:
                t.status, t.patches, t.need = _Ticket.FAILED, 0, 0
                ctx.free.append(t.slot)
                try:
                    ctx.pending.remove(t)
                except ValueError:
                    pass
                if t.state is not None:
                    t.state.ticket = None
                    t.state._patches = 0
        _lib.check(-rc)
    with ctx.lock:
        if t.status != _Ticket.PENDING:
            return True
        t.patches, mk = int(out[0]), int(out[1])
        t.need = mk.bit_length()
        ctx.free.append(t.slot)
        try:
            ctx.pending.remove(t)
        except ValueError:
            pass
        ok = t.patches <= t.cap and not (t.hint < 32 and t.need > t.hint) and t.patches < 2**31
        # what the next render of this size starts from
        _learn_key_bits(ctx.index, t.key, t.need, missed=(t.hint < 32 and t.need > t.hint))
        _learn_capacity(ctx, t.key, t.patches)
        t.status = _Ticket.OK if ok else _Ticket.FAILED
        S = t.state
        if S is not None:
            S._patches = t.patches
            S.ticket = None
            if ok:
                S.gsid = S.gsid[:t.patches]
        if not ok and not t.collected:
            ctx.failed.append(t)
    return True


class deferred:
    """``with fused.deferred() as d: ...; bad = d.commit()`` -- renders inside the block are NOT validated
    when ``forward`` returns: the host never waits for the 8-byte read-back of the patch count inside a
    step and can run a whole step ahead of the GPU.  ``commit()`` validates everything rendered so far
    (it waits for the binning stage of the last render, not for its draw or backward kernels) and returns the
    ``FusedState`` objects whose patch list outgrew the enqueue-ahead capacity or whose depth keys outgrew the
    sort's bit hint: their images and gradients are INCOMPLETE and must be recomputed before anything
    consumes them (the learnt capacity / hint are already raised, so recomputing succeeds).  Leaving the
    block with such a failure uncollected raises."""

    def __enter__(self):
        self._prev = getattr(_tls, "deferred", False)
        _tls.deferred = True
        return self

    def commit(self):
        return commit()

    def __exit__(self, et, ev, tb):
        _tls.deferred = self._prev
        if et is None and not self._prev:
            bad = commit()
            if bad:
                raise RuntimeError("%d enqueue-ahead render(s) were incomplete (patch capacity or depth-key hint "
                                   "exceeded) and nobody collected them with commit(): their results must not be used"
                                   % len(bad))
        return False


def commit(device=None):
    """Validate every render of ``device`` (default: the current one) that is still awaiting its read-back;
    -> list of the FusedState objects that turned out incomplete since the last commit."""
    index = torch.cuda.current_device() if device is None else torch.device(device).index
    ctx = _contexts.get(index)
    if ctx is None:
        return []
    while True:
        with ctx.lock:
            t = ctx.pending[0] if ctx.pending else None
        if t is None:
            break
        _settle(t, True)
    with ctx.lock:
        bad, ctx.failed = ctx.failed, []
    for t in bad:
        t.collected = True
    return [t.state for t in bad]


def expect_long_walks(device=None, renders=4):
    """A caller that KNOWS the next renders will walk their tile lists far (this package's ``DensityControl.reset_alpha``:
    every opacity drops to 0.01, nothing saturates any more, gsmodel.py:320-324) says so: the next ``renders`` renders on
    ``device`` take the segment path and speculate whole lists at once, instead of learning it from the hint words two
    renders late (the draw stage publishes a render's longest walk at the start of the NEXT draw stage on its stream;
    13 + 10 ms instead of 3.3 per training step on scene.skewed_scene's ring views).  An unmodified reference caller never
    calls this and pays those two steps."""
    index = torch.cuda.current_device() if device is None else torch.device(device).index
    if index is None:
        return
    ctx = _contexts.get(index)
    if ctx is None:
        ctx = _ctx(torch.device("cuda", index))
    with ctx.lock:
        ctx.long_walks_expected = max(ctx.long_walks_expected, int(renders))


def _seg_decision(ctx, lib, key, pol_, segments, speculate):
    """-> (use the segment path for this render, device-visible address of the hint slot or None, speculate whole
    lists); ``segments`` / ``speculate``: the callers' ``fused.SEGMENTS`` / ``fused.SEG_SPECULATE``.  The draw stage
    leaves two numbers in a page-locked slot kept per problem size -- the longest list, and the longest WALK (largest
    contributor index of a tile) of a recent render -- and a later render looks at them WITHOUT waiting (they may be a
    render or two old; they only select between two exact paths): a scene whose tiles are all walked for less than the
    split threshold takes the unsplit kernels (three launches less), at first sight and from then on long walks take
    the segment path."""
    if segments == "0" or pol_.footprint != 0 or not (pol_.alpha_skip > 0) or not (pol_.tau_stop > 0):
        return False, None, speculate == "1"
    with ctx.lock:
        slot = ctx.seg_hint.pop(key, None)
        if slot is None:
            # at most HINT_SLOTS problem sizes keep a slot; the least recently used one hands its slot on (a kernel of
            # that size still in flight may write into it once more: a stale hint, never a wrong result)
            if len(ctx.seg_hint) >= HINT_SLOTS:
                slot = ctx.seg_hint.pop(next(iter(ctx.seg_hint)))
            elif len(ctx.free) > MAILBOX_SLOTS // 2:     # (never starve the renders of their read-back slots)
                slot = ctx.free.pop()
            else:
                return segments == "1", None, speculate == "1"
            _lib.check(lib.egs_mailbox_clear(ctx.mb, slot))
        ctx.seg_hint[key] = slot                         # (re-inserted: most recently used)
    out = (C.c_uint32 * 4)()
    _lib.check(lib.egs_mailbox_peek(ctx.mb, slot, out))
    cfg = (C.c_int * 2)()
    _lib.check(lib.egs_seg_config(0, 0, cfg))
    longest, walk = int(out[0]), int(out[1])
    known = walk != 0xFFFFFFFF and longest != 0xFFFFFFFF
    # no walk on record yet: the longest LIST bounds it (a scene whose lists all stay below the split threshold never
    # pays for the segment workspace, ~6 KB per 256 entries of a split tile); nothing known at all: the segment path
    unknown = walk == 0xFFFFFFFF and (longest == 0xFFFFFFFF or longest > cfg[1])
    use = segments == "1" or unknown or (walk != 0xFFFFFFFF and walk > cfg[1])
    with ctx.lock:
        announced = ctx.long_walks_expected > 0
        if announced:
            ctx.long_walks_expected -= 1
    hint = C.c_void_p(lib.egs_mailbox_slot(ctx.mb, slot))
    if announced and segments != "0":
        return True, hint, speculate != "0"
    return use, hint, speculate == "1" or (speculate == "auto" and known and 2 * walk >= longest)


def _walk_word(ctx, key, dev, st, have_hint):
    """The persistent device word of (problem size, stream) for the draw stage's longest-walk report, or None."""
    if not have_hint:
        return None
    k = (key, int(st.value or 0))
    with ctx.lock:
        w = ctx.walk_word.get(k)
        if w is None:
            while len(ctx.walk_word) >= 4 * HINT_SLOTS:          # (bounded: streams and sizes that are gone)
                ctx.walk_word.pop(next(iter(ctx.walk_word)))
            w = ctx.walk_word[k] = torch.full((16,), -1, dtype=torch.int32, device=dev)
    return w


def seg_hint(device=None, key=None):
    """(longest list, longest walk) the draw stage last reported for problem size ``key`` = (N, W, H) on ``device``
    (None: nothing yet / no slot) -- what ``_seg_decision`` steers by; for bench lines and tests."""
    index = torch.cuda.current_device() if device is None else torch.device(device).index
    ctx = _contexts.get(index)
    if ctx is None:
        return None
    with ctx.lock:
        slot = ctx.seg_hint.get(key)
    if slot is None:
        return None
    out = (C.c_uint32 * 4)()
    _lib.check(ctx.lib.egs_mailbox_peek(ctx.mb, slot, out))
    f = lambda v: None if v == 0xFFFFFFFF else int(v)
    return f(out[0]), f(out[1])


# ---- the enqueue-ahead render protocol ----------------------------------------------------------------------------
# The two callers hand ``render`` what is theirs as callables:
#   enqueue_bin(hint, total, host_slot)  enqueue the binning stage with this depth-key bit hint; {P, max key} go to the
#                                        device words ``total`` and, when ``host_slot`` is given, to that mailbox slot
#   draw(rows, total, redo)              enqueue the draw stage: for exactly ``rows`` patches (``total`` None), or with
#                                        buffers of ``rows`` patches and the count taken from the device words ``total``.
#                                        ``redo``: the draw stage of this render ran once already on truncated lists (more
#                                        patches than the enqueue-ahead buffers held).  Its range kernel has published the
#                                        PREVIOUS render's hint words; what that truncated draw raised in the walk word is
#                                        nobody's longest walk: the second range kernel clears it without publishing (the
#                                        callee withholds the hint address) -- otherwise a later render steers by
#                                        (1189, 696) where the render walked (2063, 696)
def try_slot(ctx):
    """A free mailbox slot, or None: the render then takes the synchronous form."""
    with ctx.lock:
        return ctx.free.pop() if ctx.free else None


def wait_slot(ctx):
    """A free mailbox slot; while every slot is in flight, waits for the oldest render."""
    while True:
        with ctx.lock:
            if ctx.free:
                return ctx.free.pop()
            oldest = ctx.pending[0] if ctx.pending else None
        if oldest is None:
            raise RuntimeError("fused.forward: no mailbox slot free and no render in flight (slots leaked)")
        _settle(oldest, True)


def _render_sync(ctx, dev, key, enqueue_bin, draw, redo=False):
    """Synchronous form: read P back (8 bytes, as the reference does at gausplat.cu:67), then draw -- the GPU idles
    around the read."""
    patches = _bin_stage(enqueue_bin, dev, key)
    draw(patches, None, redo)
    if key[0] > 0:
        with ctx.lock:
            _learn_capacity(ctx, key, patches)
    return patches


def render(ctx, dev, key, st, cap, slot_of, enqueue_bin, draw, state=None, defer=False, post_copy=False):
    """One render of problem size ``key`` = (N, W, H) on stream ``st`` -> its patch count P, or None while it awaits
    validation (``defer``).  ``cap`` == 0 (first render of this size, or enqueue-ahead switched off) or no slot from
    ``slot_of(ctx)`` (``try_slot`` / ``wait_slot``): the synchronous form.  Else the draw stage is enqueued AHEAD of the
    read-back: buffers sized by the largest patch count seen so far (``cap``), the kernels take the real count from
    device memory, and {P, max depth key} travel to a page-locked mailbox slot -- stored by the binning kernels, or
    (``post_copy``) by a copy enqueued between the two stages (egs_mailbox_post).  The GPU never waits for the host
    (the reference idles around cudaMemcpy(&P), gausplat.cu:67).  An overflow of the capacity or of the depth-key hint
    is detected after the fact -- here (one C-side wait on the slot's event) or, with ``defer``, at ``commit()``, which
    reports ``state`` -- and the render is redone.  ``state`` (a ``FusedState`` or None) carries the ticket meanwhile."""
    slot = None
    if cap > 0:
        hint = _get_key_bits(dev.index, key)
        slot = slot_of(ctx)
    if slot is None:
        return _render_sync(ctx, dev, key, enqueue_bin, draw)
    t = _Ticket()
    t.ctx, t.key, t.cap, t.hint, t.slot, t.state, t.status = ctx, key, cap, hint, slot, state, _Ticket.PENDING
    t.collected = state is None                       # (nothing commit() could report)
    lib = ctx.lib
    try:
        total = torch.empty(2, dtype=torch.int32, device=dev)
        if post_copy:             # {P, max key} by an 8-byte device-to-host copy behind the binning stage
            enqueue_bin(hint, total, None)
            _lib.check(lib.egs_mailbox_post(ctx.mb, slot, _ptr(total), st))
        else:                     # the binning kernels store them into the page-locked slot themselves
            _lib.check(lib.egs_mailbox_arm(ctx.mb, slot, st))
            enqueue_bin(hint, total, C.c_void_p(lib.egs_mailbox_slot(ctx.mb, slot)))
        draw(cap, total, False)
    except BaseException:
        # Whatever was enqueued before the failure (the arm, the binning chain) still stores {P, max key} into the
        # slot: it goes back on the free list only once those kernels have run -- otherwise a render on another
        # ViewStreams lane could pick it up and settle on THEIR values.  Rare path: a stream wait is fine.
        try:
            torch.cuda.current_stream(dev).synchronize()
        except Exception:
            pass
        with ctx.lock:
            t.status = _Ticket.FAILED
            ctx.free.append(slot)
        raise
    if state is not None:
        state.ticket = t
    with ctx.lock:
        ctx.pending.append(t)
    if defer:
        with ctx.lock:                                # look at whatever has landed meanwhile (no waiting)
            waiting = list(ctx.pending)
        for old in waiting:
            if old is not t and not _settle(old, False):
                break
        return None
    t.collected = True                                # validated right here: never reported by commit()
    _settle(t, True)                                  # one C-side wait on the slot; learns capacity and depth-key bits
    if t.status == _Ticket.FAILED:
        if t.patches >= 2**31:
            raise RuntimeError("splat: %d tile patches overflow int32 indexing" % t.patches)
        if t.hint < 32 and t.need > t.hint:           # stale depth-key hint: everything again (the stage is idempotent)
            return _render_sync(ctx, dev, key, enqueue_bin, draw, redo=True)
        draw(t.patches, None, True)                   # more patches than ever before: redo the draw stage
    return t.patches
