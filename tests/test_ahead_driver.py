"""The enqueue-ahead render protocol (``_ahead.render``) driven on the CPU: a stub library whose ``egs_mailbox_*`` calls
are scripted, recording callables for the binning and the draw stage, CPU tensors.  Both callers' ways of using the
driver are exercised: ``fused.forward``'s (``wait_slot``, a state that carries the ticket, optional deferral and
``post_copy``) and the seven-op ``splat``'s (``try_slot``, no state, settled at once).  Nothing here touches a GPU."""
import collections
import ctypes as C

import pytest
import torch

from easygaussiansplatting_amd import _ahead as A

DEV = torch.device("cpu", 0)
SLOT_BASE, SLOT_BYTES = 0x10000, 16


class StubLib:
    """The mailbox of include/egs_hip.h in host memory: ``land`` is what the binning kernels (or the posted copy) do."""

    def __init__(self):
        self.calls = []
        self.landed = {}
        self.lag = False          # True: nothing has landed yet for a fetch that does not wait

    def egs_mailbox_create(self, slots):
        return 1

    def egs_mailbox_slot(self, mb, slot):
        return SLOT_BASE + SLOT_BYTES * slot

    def egs_mailbox_arm(self, mb, slot, st):
        self.calls.append(("arm", slot))
        self.landed.pop(slot, None)
        return 0

    def egs_mailbox_post(self, mb, slot, total, st):
        self.calls.append(("post", slot))
        words = (C.c_uint32 * 2).from_address(total.value)
        self.landed[slot] = (int(words[0]), int(words[1]))
        return 0

    def land(self, address, patches, max_key):
        self.landed[(address - SLOT_BASE) // SLOT_BYTES] = (patches, max_key)

    def egs_mailbox_fetch(self, mb, slot, blocking, out):
        self.calls.append(("fetch", slot, blocking))
        if self.lag and not blocking:
            return 0
        out[0], out[1] = self.landed[slot]
        return 1


class State:
    """What the driver and ``_settle`` touch of a ``fused.FusedState``."""

    def __init__(self):
        self.ticket, self._patches, self.gsid = None, None, None


class Boom(BaseException):
    pass


class Rig:
    def __init__(self, way, key, monkeypatch):
        self.way, self.key = way, key
        self.lib = StubLib()
        self.ctx = A._DeviceCtx(self.lib, DEV.index)
        monkeypatch.setattr(A, "_contexts", {DEV.index: self.ctx})
        monkeypatch.setattr(A, "_key_bits", {})
        monkeypatch.setattr(A, "_key_low", {})
        self.tickets = tickets = []

        class Ticket(A._Ticket):
            __slots__ = ()

            def __init__(self):
                tickets.append(self)
        monkeypatch.setattr(A, "_Ticket", Ticket)
        self.script = collections.deque()      # (P, max depth key) the next binning stages report
        self.bins, self.draws, self.totals = [], [], []
        self.draw_raises = None
        self.state = None

    def enqueue_bin(self, hint, total, host_slot):
        patches, max_key = self.script.popleft()
        self.bins.append((hint, None if host_slot is None else host_slot.value))
        self.totals.append(total)
        total[:] = torch.tensor([patches, max_key], dtype=torch.int64).to(torch.int32)      # (wraps, as the words do)
        if host_slot is not None:
            self.lib.land(host_slot.value, patches, max_key)

    def draw(self, rows, total, redo):
        if self.draw_raises is not None:
            raise self.draw_raises
        self.draws.append((rows, total, redo))
        if self.state is not None:
            self.state.gsid = range(rows)                  # (sliceable, as the tensor is)

    def render(self, report, defer=False, post_copy=False):
        """One render the way ``self.way`` does it; ``report``: what its binning stages will report, in order."""
        self.script.extend(report)
        self.bins.clear(), self.draws.clear(), self.totals.clear(), self.lib.calls.clear()
        cap = self.ctx.capacity.get(self.key, 0)
        if self.way == "fused":
            self.state = State()
            return A.render(self.ctx, DEV, self.key, None, cap, A.wait_slot, self.enqueue_bin, self.draw, self.state,
                            defer, post_copy)
        return A.render(self.ctx, DEV, self.key, None, cap, A.try_slot, self.enqueue_bin, self.draw)

    def slots_all_free(self):
        return sorted(self.ctx.free) == list(range(A.MAILBOX_SLOTS))


@pytest.fixture(params=["fused", "splat"])
def rig(request, monkeypatch):
    return Rig(request.param, (1000, 64, 48), monkeypatch)


@pytest.fixture
def fused_rig(monkeypatch):
    """for what only ``fused.forward`` asks of the driver: ``post_copy`` (fused.MAILBOX_COPY) and deferred validation"""
    return Rig("fused", (1000, 64, 48), monkeypatch)


def test_first_render_is_synchronous_and_learns_the_capacity(rig):
    assert rig.render([(5000, 0xFFF)]) == 5000
    assert rig.bins == [(32, None)]                              # nothing known: full-width keys, no mailbox slot
    assert rig.draws == [(5000, None, False)]
    assert not any(c[0] in ("arm", "post", "fetch") for c in rig.lib.calls)
    assert rig.ctx.capacity[rig.key] == A._grow(5000)
    assert A._get_key_bits(DEV.index, rig.key) == 13
    assert rig.slots_all_free() and not rig.ctx.pending


def test_second_render_is_enqueued_ahead(rig):
    rig.render([(5000, 0xFFF)])
    cap = A._grow(5000)
    assert rig.render([(5100, 0xFFF)]) == 5100
    slot = rig.tickets[-1].slot
    assert rig.lib.calls[0] == ("arm", slot) and ("fetch", slot, 1) in rig.lib.calls
    assert rig.bins == [(13, rig.lib.egs_mailbox_slot(1, slot))]
    assert len(rig.draws) == 1 and rig.draws[0][0] == cap and rig.draws[0][2] is False
    assert rig.draws[0][1] is rig.totals[0]                      # the count comes from the binning stage's device words
    assert rig.tickets[-1].status == A._Ticket.OK
    assert rig.slots_all_free() and not rig.ctx.pending and not rig.ctx.failed
    if rig.state is not None:
        assert rig.state.ticket is None and rig.state._patches == 5100 and len(rig.state.gsid) == 5100


def test_more_patches_than_the_capacity_redoes_the_draw_only(rig):
    rig.render([(5000, 0xFFF)])
    cap = A._grow(5000)
    big = cap + 1
    assert rig.render([(big, 0xFFF)]) == big
    assert len(rig.bins) == 1                                    # no second binning stage
    assert [(d[0], d[2]) for d in rig.draws] == [(cap, False), (big, True)] and rig.draws[1][1] is None
    assert rig.tickets[-1].status == A._Ticket.FAILED
    assert rig.ctx.capacity[rig.key] == A._grow(big)
    assert rig.slots_all_free() and not rig.ctx.pending and not rig.ctx.failed


def test_stale_key_hint_redoes_everything_at_full_width(rig):
    rig.render([(5000, 0xFFF)])
    cap = A._grow(5000)
    assert rig.render([(5000, 0xFFFFF), (5000, 0xFFFFF)]) == 5000
    assert [b[0] for b in rig.bins] == [13, 32] and rig.bins[1][1] is None     # (no slot: it was handed back)
    assert [(d[0], d[2]) for d in rig.draws] == [(cap, False), (5000, True)] and rig.draws[1][1] is None
    assert A._get_key_bits(DEV.index, rig.key) == 21             # what _learn_key_bits makes of a miss, then 20 bits
    assert rig.slots_all_free() and not rig.ctx.pending and not rig.ctx.failed


def test_patch_count_beyond_int32_raises(rig):
    rig.render([(5000, 0xFFF)])
    with pytest.raises(RuntimeError, match=r"^splat: 2147483648 tile patches overflow int32 indexing$"):
        rig.render([(2**31, 0xFFF)])
    assert len(rig.draws) == 1 and len(rig.bins) == 1
    assert rig.slots_all_free() and not rig.ctx.pending


def test_a_failing_draw_hands_the_slot_back_once(rig):
    rig.render([(5000, 0xFFF)])
    rig.draw_raises = Boom()
    with pytest.raises(Boom):
        rig.render([(5000, 0xFFF)])
    t = rig.tickets[-1]
    assert t.status == A._Ticket.FAILED
    assert rig.ctx.free.count(t.slot) == 1 and rig.slots_all_free()
    assert not rig.ctx.pending and not rig.ctx.failed
    assert not any(c[0] == "fetch" for c in rig.lib.calls)


def test_no_free_slot(rig):
    rig.render([(5000, 0xFFF)])
    cap = A._grow(5000)
    rig.ctx.free.clear()
    if rig.way == "splat":                                       # the synchronous form for this call
        assert rig.render([(5050, 0xFFF)]) == 5050
        assert rig.bins == [(13, None)] and rig.draws == [(5050, None, False)]
        assert not rig.tickets and not rig.ctx.free
        return
    with pytest.raises(RuntimeError, match="no mailbox slot free and no render in flight"):
        rig.render([])                                           # (raises before any stage is enqueued)
    assert not rig.bins and not rig.draws
    # every slot in flight: the oldest pending render is settled first, its slot serves this one
    rig.ctx.free.append(7)
    rig.lib.lag = True
    assert rig.render([(5001, 0xFFF)], defer=True) is None
    oldest = rig.tickets[-1]
    assert oldest.status == A._Ticket.PENDING and not rig.ctx.free
    assert rig.render([(5002, 0xFFF)]) == 5002
    assert oldest.status == A._Ticket.OK and oldest.patches == 5001
    assert rig.lib.calls[0] == ("fetch", 7, 1) and rig.lib.calls[1] == ("arm", 7)
    assert len(rig.draws) == 1 and rig.draws[0][0] == cap and rig.draws[0][1] is rig.totals[0]
    assert rig.ctx.free == [7] and not rig.ctx.pending


def test_posted_copy_instead_of_kernel_stores(fused_rig):
    rig = fused_rig
    rig.render([(5000, 0xFFF)])
    assert rig.render([(5100, 0xFFF)], post_copy=True) == 5100
    slot = rig.tickets[-1].slot
    assert rig.bins == [(13, None)]
    assert [c[0] for c in rig.lib.calls] == ["post", "fetch"] and rig.lib.calls[0] == ("post", slot)
    assert rig.slots_all_free() and not rig.ctx.pending


def test_deferred_renders_stay_pending_until_commit(fused_rig):
    rig = fused_rig
    rig.render([(5000, 0xFFF)])
    cap = A._grow(5000)
    rig.lib.lag = True
    states = []
    for report in ((5010, 0xFFF), (cap + 1, 0xFFF), (5020, 0xFFFFF), (5030, 0xFFF)):
        assert rig.render([report], defer=True) is None
        assert len(rig.bins) == 1 and len(rig.draws) == 1 and rig.draws[0][0] == cap
        assert not any(c[0] == "fetch" and c[2] for c in rig.lib.calls)       # older renders polled, never waited for
        states.append(rig.state)
    assert [t.status for t in rig.tickets] == [A._Ticket.PENDING] * 4
    assert list(rig.ctx.pending) == rig.tickets and len(rig.ctx.free) == A.MAILBOX_SLOTS - 4
    assert all(s.ticket is t and s._patches is None for s, t in zip(states, rig.tickets))
    bad = A.commit(DEV)
    assert len(bad) == 2 and bad[0] is states[1] and bad[1] is states[2]
    assert [s._patches for s in states] == [5010, cap + 1, 5020, 5030] and all(s.ticket is None for s in states)
    assert len(states[0].gsid) == 5010 and len(states[1].gsid) == cap          # (an incomplete render keeps its buffers)
    assert rig.slots_all_free() and not rig.ctx.pending and A.commit(DEV) == []
    # with the read-backs landing in time, the next deferred render settles its predecessor without waiting
    rig.lib.lag = False
    rig.render([(5040, 0xFFF)], defer=True)
    first = rig.tickets[-1]
    rig.render([(5050, 0xFFF)], defer=True)
    assert first.status == A._Ticket.OK and list(rig.ctx.pending) == [rig.tickets[-1]]
    assert ("fetch", first.slot, 0) in rig.lib.calls
    assert A.commit(DEV) == []
