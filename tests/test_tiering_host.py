"""Bounded local tiers, host side (no GPU): the free list of the arenas, the group LRU and its budgets
(lmcache_amd/storage_backend/tiering.py), the unbounded arena against its recorded behaviour, and the three C-ABI
symbols of the demotion / promotion legs."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch

from lmcache_amd import native
from lmcache_amd.storage_backend.serde.cachegen_device import ArenaFull, PinnedArena
from lmcache_amd.storage_backend.tiering import FreeList, GroupLRU, Tiers, parse_bytes


# ---- free list ------------------------------------------------------------------------------------------------------
def _overlaps(regions):
    by_slab = {}
    for sid, off, size in regions:
        by_slab.setdefault(sid, []).append((off, off + size))
    for spans in by_slab.values():
        spans.sort()
        if any(a[1] > b[0] for a, b in zip(spans, spans[1:])):
            return True
    return False


def test_free_list_random_sequence_never_overlaps_and_holds_its_budget():
    rng = random.Random(1234)
    budget, slab = 64 << 10, 16 << 10
    fl = FreeList(budget)
    live, nslabs, refused = [], 0, 0
    for step in range(4000):
        if live and (rng.random() < 0.45 or fl.live > budget * 0.9):
            sid, off, size = live.pop(rng.randrange(len(live)))
            fl.free(sid, off, size)
        else:
            need = 16 * rng.randint(1, 200)
            got = fl.alloc(need)
            if got is None and fl.fits_budget(need):
                size = min(max(slab, need), fl.room_for_slab()) & ~15
                if size >= need:
                    fl.add_slab(nslabs, size)
                    nslabs += 1
                    got = fl.alloc(need)
            if got is None:
                refused += 1
                continue
            live.append((got[0], got[1], need))
        assert fl.reserved <= budget and fl.live <= budget
        assert fl.live == sum(r[2] for r in live)
        assert not _overlaps(live)
        for sid, off, size in live:
            assert off + size <= fl.slabs[sid]
            assert all(h[0] + h[1] <= off or off + size <= h[0] for h in fl.holes[sid]), "a live region lies in a hole"
    assert refused > 0 and nslabs >= 2, "the sequence must reach the budget and more than one slab"
    for sid, off, size in live:
        fl.free(sid, off, size)
    assert fl.live == 0
    for sid, size in fl.slabs.items():  # a full free: one hole per slab
        assert fl.holes[sid] == [[0, size, []]] and fl.is_empty(sid)


def test_free_list_hands_a_freed_regions_events_to_whoever_overlaps_it():
    fl = FreeList()
    fl.add_slab("s", 1024)
    a = fl.alloc(256)
    b = fl.alloc(256)
    c = fl.alloc(512)
    assert (a[1], b[1], c[1]) == (0, 256, 512) and a[2] == b[2] == c[2] == []
    ev_a, ev_b = object(), object()
    fl.free("s", 0, 256, [ev_a])
    fl.free("s", 512, 512)             # no neighbour to merge with, no event
    assert fl.holes["s"] == [[0, 256, [ev_a]], [512, 512, []]]
    fl.free("s", 256, 256, [ev_b])     # merges with both neighbours: one hole, both events, each once
    assert len(fl.holes["s"]) == 1 and fl.holes["s"][0][:2] == [0, 1024]
    assert set(map(id, fl.holes["s"][0][2])) == {id(ev_a), id(ev_b)}
    x = fl.alloc(128)                  # overlaps the region ev_a guards (conservatively: the merged hole's events)
    assert x[1] == 0 and {id(e) for e in x[2]} == {id(ev_a), id(ev_b)}
    y = fl.alloc(128)                  # the rest of the hole keeps them for the next owner
    assert y[1] == 128 and {id(e) for e in y[2]} == {id(ev_a), id(ev_b)}
    # events that have fired are forgotten when holes merge
    fired = set()
    fl2 = FreeList(done=lambda e: id(e) in fired)
    fl2.add_slab(0, 64)
    p, q = fl2.alloc(32), fl2.alloc(32)
    fl2.free(0, 0, 32, [ev_a])
    fired.add(id(ev_a))
    fl2.free(0, 32, 32, [ev_b])
    assert fl2.holes[0] == [[0, 64, [ev_b]]]


def test_free_list_refuses_over_budget_and_a_double_free():
    fl = FreeList(budget=96)
    fl.add_slab(0, 96)
    assert fl.room_for_slab() == 0
    a = fl.alloc(64)
    assert fl.alloc(48) is None and fl.alloc(32) is not None and fl.alloc(16) is None
    fl.free(0, a[1], 64)
    with pytest.raises(AssertionError):
        fl.free(0, a[1], 64)


class _FakeBuffer:
    made = 0

    def __init__(self, nbytes):
        _FakeBuffer.made += 1
        self.nbytes, self.ptr, self.id, self.freed = nbytes, 1 << 40, _FakeBuffer.made, False

    def free(self):
        self.freed = True


# (tag, slab number, offset, nbytes, total_allocated, slab sizes) of the bump allocator as it was before it learnt to
# free: recorded from that implementation with 4096-byte slabs.
RECORDED = [("a100", 1, 0, 100, 112, [4096]),
            ("a1000", 1, 112, 1000, 1120, [4096]),
            ("s300", 1, 112, 300, 416, [4096]),
            ("a3000", 1, 416, 3000, 3424, [4096]),
            ("s-notlast", 1, 0, 10, 3424, [4096]),
            ("a2000", 2, 0, 2000, 5424, [4096, 10000]),
            ("reserve", None, None, None, 5424, [4096, 10000]),
            ("a9000", 4, 0, 9000, 14432, [4096, 10000, 9008]),
            ("a5000", 3, 0, 5000, 19440, [4096, 10000, 9008, 6000]),
            ("a1", 3, 5008, 1, 19456, [4096, 10000, 9008, 6000]),
            ("s0", 3, 5008, 0, 19456, [4096, 10000, 9008, 6000]),
            ("reset", None, None, None, 0, [6000]),
            ("a64", 3, 0, 64, 64, [6000])]


def test_unbounded_pinned_arena_behaves_as_recorded():
    _FakeBuffer.made = 0
    a = PinnedArena(slab_bytes=4096, buffer_factory=_FakeBuffer)
    out = []

    def rec(tag, hb=None):
        out.append((tag, hb.slab.id if hb else None, hb.offset if hb else None, hb.nbytes if hb else None,
                    a.total_allocated, [s.nbytes for s in a._slabs]))
    h1 = a.alloc(100); rec("a100", h1)
    h2 = a.alloc(1000, slab_hint=8192); rec("a1000", h2)
    h2 = a.shrink(h2, 300); rec("s300", h2)
    h3 = a.alloc(3000); rec("a3000", h3)
    rec("s-notlast", a.shrink(h1, 10))
    rec("a2000", a.alloc(2000, slab_hint=10000))
    a.reserve(5000, 6000); rec("reserve")
    rec("a9000", a.alloc(9000))
    rec("a5000", a.alloc(5000))
    h7 = a.alloc(1); rec("a1", h7)
    rec("s0", a.shrink(h7, 0))
    a.reset(); rec("reset")
    rec("a64", a.alloc(64))
    assert out == RECORDED
    assert a.budget is None


# (operation, where the region landed -- (index in _slabs, offset), "full" for ArenaFull --, live_bytes, slab sizes) of both
# arenas through unbounded, bounded, over budget, unlimited again and bounded again: recorded with 4096-byte slabs from the
# two separate implementations that were there before arena.SlabArena.  One row differs: over its budget the pinned arena
# gives empty slabs back oldest first, the HBM arena newest first.
_S4 = [4096, 4096, 6000, 5008]
_S3 = [4096, 4096, 2304]
RECORDED_BOTH = [(("alloc", "a", 3000), (0, 0), 3008, [4096]),
                 (("alloc", "b", 2000), (1, 0), 5008, [4096, 4096]),
                 (("alloc", "c", 6000), (2, 0), 11008, [4096, 4096, 6000]),
                 (("alloc", "d", 5000), (3, 0), 16016, _S4),
                 (("free", "b"), None, 14016, _S4),
                 (("budget", 30000), None, 14016, _S4),
                 (("alloc", "e", 1500), (1, 0), 15520, _S4),
                 (("free", "c"), None, 9520, _S4),
                 (("free", "d"), None, 4512, _S4),
                 (("free", "e"), None, 3008, _S4),
                 (("budget", 10500), None, 3008, {"pinned": [4096, 5008], "device": [4096, 4096]}),
                 (("alloc", "f", 7000), "full", 3008, [4096]),   # (refused, and the empty slab has gone back all the same)
                 (("alloc", "g", 4000), (1, 0), 7008, [4096, 4096]),
                 (("alloc", "h", 2000), (2, 0), 9008, _S3),      # (a slab cut to the 2304 bytes the budget leaves)
                 (("free", "a"), None, 6000, _S3),
                 (("alloc", "i", 4500), "full", 6000, _S3),
                 (("alloc", "j", 6000), "full", 6000, _S3),
                 (("budget", None), None, 6000, _S3),            # (still a free list; later slabs get the unbounded size)
                 (("alloc", "k", 9000), (3, 0), 15008, _S3 + [9008]),
                 (("free", "g"), None, 11008, _S3 + [9008]),
                 (("budget", 12000), None, 11008, [2304, 9008])]


def _host_arena(kind, **kw):
    """-> (arena, where(region) -> (index in _slabs, offset)); plain host tensors stand in for HBM."""
    from lmcache_amd.storage_backend.serde.cachegen_device import DeviceArena
    if kind == "pinned":
        a = PinnedArena(slab_bytes=4096, buffer_factory=_FakeBuffer, **kw)
        return a, lambda r: (next(k for k, s in enumerate(a._slabs) if s is r.slab), r.offset)
    a = DeviceArena(torch.device("cpu"), slab_bytes=4096, **kw)
    return a, lambda r: next((k, r.data_ptr() - s.data_ptr()) for k, s in enumerate(a._slabs)
                             if s.data_ptr() <= r.data_ptr() < s.data_ptr() + s.numel())


@pytest.mark.parametrize("kind", ["pinned", "device"])
def test_both_arenas_behave_as_recorded_through_every_mode(kind):
    a, where = _host_arena(kind)
    held, out = {}, []
    for op, _, _, _ in RECORDED_BOTH:
        at = None
        if op[0] == "alloc":
            try:
                held[op[1]] = a.alloc(op[2])
                at = where(held[op[1]])
            except ArenaFull:
                at = "full"
        elif op[0] == "free":
            a.free(held.pop(op[1]))
        else:
            a.set_budget(op[1])
        out.append((op, at, a.live_bytes, [s.nbytes for s in a._slabs]))
    assert out == [(op, at, live, sizes[kind] if isinstance(sizes, dict) else sizes) for op, at, live, sizes in RECORDED_BOTH]
    assert a.reserved_bytes == 2304 + 9008 and a.budget == 12000
    if kind == "pinned":
        assert a.total_allocated == a.live_bytes


class _WaitLog:
    def __init__(self):
        self.waited = []

    def wait_event(self, e):
        self.waited.append(e)


@pytest.mark.parametrize("kind", ["pinned", "device"])
def test_a_fence_given_back_while_unbounded_is_waited_for_once_the_arena_is_bounded(kind):
    """Freed with an event while the arena only counts, allocated after a budget was set: the stream named at alloc() waits
    for exactly that event, and for nothing when it takes bytes nobody gave back."""
    a, where = _host_arena(kind)
    alloc = (lambda n, st: a.alloc(n, streams=[st])) if kind == "pinned" else (lambda n, st: a.alloc(n, stream=st))
    x, y = a.alloc(1000), a.alloc(1000)
    ev = object()
    a.free(x, [ev])
    a.set_budget(8192)
    st = _WaitLog()
    assert where(alloc(1000, st)) == (0, 0) and st.waited == [ev]
    st2 = _WaitLog()
    assert where(alloc(1000, st2)) == (0, 2016) and st2.waited == []   # (behind the bump pointer: never handed out)
    a.free(y)
    assert where(a.alloc(1000)) == (0, 1008)   # no stream named, no event: the HBM arena does not ask for the current stream


def test_every_stream_named_at_alloc_waits_for_a_fence_given_back_while_unbounded():
    a, where = _host_arena("pinned")
    x = a.alloc(1000)
    ev = object()
    a.free(x, [ev])
    a.set_budget(4096)
    s1, s2 = _WaitLog(), _WaitLog()
    assert where(a.alloc(1000, streams=[s1, s2])) == (0, 0)
    assert s1.waited == [ev] and s2.waited == [ev]


def test_bounded_pinned_arena_reserves_no_more_than_its_budget_and_reuses_what_is_freed():
    _FakeBuffer.made = 0
    a = PinnedArena(slab_bytes=4096, budget=6000, buffer_factory=_FakeBuffer)
    ev = object()

    class Stream:
        def __init__(self):
            self.waited = []

        def wait_event(self, e):
            self.waited.append(e)
    st = Stream()
    h1 = a.alloc(3000, streams=[st])
    h2 = a.alloc(1000)
    assert (h1.offset, h2.offset) == (0, 3008) and a.reserved_bytes == 4096 and st.waited == []
    h3 = a.alloc(1500)                       # a second slab, cut to what the budget leaves
    assert h3.slab is not h1.slab and a.reserved_bytes == 4096 + 1904 <= 6000
    with pytest.raises(ArenaFull):
        a.alloc(1000)                        # 5520 live + 1008 > 6000
    a.free(h1, [ev])
    h4 = a.alloc(2000, streams=[st])         # first fit: h1's region, behind its reader's event
    assert h4.slab is h1.slab and h4.offset == 0 and st.waited == [ev]
    # allocated at a bound, cut to size: the budget was tested against the bound and is corrected by the cut
    live = a.live_bytes
    h5 = a.alloc(900)
    h5 = a.shrink(h5, 100)
    assert a.live_bytes == live + 112 and h5.nbytes == 100
    a.shrink(h5, 0)
    assert a.live_bytes == live
    assert a.reserved_bytes <= 6000


def test_an_arena_bounded_later_keeps_what_it_handed_out():
    _FakeBuffer.made = 0
    a = PinnedArena(slab_bytes=4096, buffer_factory=_FakeBuffer)
    h1, h2 = a.alloc(1000), a.alloc(3200)    # two slabs
    a.free(h2)                               # unbounded: only counted
    assert a.live_bytes == 1008
    h3 = a.alloc(500)
    assert h3.slab is h2.slab and h3.offset == 3200  # ... the bump allocator reuses nothing
    a.set_budget(1530)
    # what the bump pointers cover and nobody has given back counts as live; what was given back is a hole again (it
    # used to stay counted for good: a tier bounded after a key was stored twice lost that much of its budget)
    assert a.live_bytes == 1008 + 512
    with pytest.raises(ArenaFull):
        a.alloc(16)
    slab2 = h3.slab
    a.free(h3)
    assert slab2.freed and a.reserved_bytes == 4096  # over budget: the empty slab went back to the system
    assert a.alloc(500).offset == 1008


def test_a_bounded_arena_whose_groups_have_gone_takes_a_region_larger_than_any_slab():
    """Slabs that are one hole are traded for a slab of the needed size: an arena that is empty takes whatever its
    budget allows, however its earlier allocations cut it up."""
    _FakeBuffer.made = 0
    a = PinnedArena(slab_bytes=4096, budget=10000, buffer_factory=_FakeBuffer)
    h1, h2 = a.alloc(5000), a.alloc(4900)
    assert h1.slab is not h2.slab and a.reserved_bytes <= 10000
    a.free(h1)
    a.free(h2)
    big = a.alloc(6000)
    assert big.nbytes == 6000 and a.live_bytes == 6000 and a.reserved_bytes <= 10000
    assert h1.slab.freed or h2.slab.freed
    with pytest.raises(ArenaFull):
        a.alloc(5000)                        # the byte count itself says no
    a.free(big)
    assert a.alloc(9984).nbytes == 9984 and a.reserved_bytes <= 10000


@pytest.mark.parametrize("kind", ["pinned", "device"])
def test_a_bounded_arena_that_loses_its_limit_keeps_allocating(kind):
    from lmcache_amd.storage_backend.serde.cachegen_device import DeviceArena
    if kind == "pinned":
        _FakeBuffer.made = 0
        a = PinnedArena(slab_bytes=4096, budget=8192, buffer_factory=_FakeBuffer)
        size = lambda x: x.nbytes
    else:
        a = DeviceArena(torch.device("cpu"), slab_bytes=4096, budget=8192)   # (plain host tensors stand in for HBM)
        size = lambda x: x.numel()
    first = a.alloc(3000)
    with pytest.raises(ArenaFull):
        a.alloc(8000)
    a.set_budget(None)
    assert a.budget is None
    got = [a.alloc(3000) for _ in range(6)]  # no hole fits after the first: new slabs, of the unbounded size
    assert all(size(x) == 3000 for x in got) and a.live_bytes == 7 * 3008
    a.free(got[0])
    a.free(first)
    assert a.live_bytes == 5 * 3008
    assert size(a.alloc(9000)) == 9000
    a.set_budget(1 << 20)
    assert size(a.alloc(100)) == 100 and a.reserved_bytes <= 1 << 20


def test_demotion_room_is_sized_by_what_the_group_takes_in_the_pinned_tier():
    lru = GroupLRU()
    log = []

    def demote(gid):
        log.append(("demote", gid))
        lru.add("pinned", gid, 120)          # a pack is a little larger than its blobs
        return True
    t = Tiers(lru, demote, lambda gid: log.append(("drop", gid)), pinned_size=lambda gid: 120)
    t.budget["hbm"], t.budget["pinned"] = 100, 230
    lru.add("pinned", 0, 120)
    lru.add("hbm", 1, 100)
    lru.add("hbm", 2, 100)
    t.enforce()                              # 120 + 120 > 230: group 0 has to go first, though 120 + 100 would fit
    assert log == [("drop", 0), ("demote", 1)] and lru.live("pinned") == 120


# ---- group LRU --------------------------------------------------------------------------------------------------------
def test_touch_order_eats_a_chain_from_its_tail():
    lru = GroupLRU()
    for g in range(5):
        lru.add("hbm", g, 100)
    assert lru.groups("hbm") == [0, 1, 2, 3, 4]
    lru.touch_chain([1, 1, 2, 2, 2, 3])      # a hit over the chain 1 -> 2 -> 3 (several chunks per group)
    # untouched groups go first, then the chain from its tail: 3 before 2 before its head 1
    assert lru.groups("hbm") == [0, 4, 3, 2, 1]
    assert lru.victims("hbm", budget=300) == [0, 4]
    assert lru.victims("hbm", budget=250) == [0, 4, 3]
    assert lru.victims("hbm", budget=300, need=100) == [0, 4, 3]
    assert lru.victims("hbm", budget=300, keep=[0]) == [4, 3]
    assert lru.victims("hbm", budget=500) == []
    lru.remove(4)
    assert lru.live("hbm") == 400 and lru.tier_of(4) is None and lru.count("hbm") == 4


def _tiers(budget_hbm, budget_pinned, demote_ok=True):
    lru = GroupLRU()
    log = []

    def demote(gid):
        log.append(("demote", gid))
        if not demote_ok:
            return False
        lru.add("pinned", gid, lru.nbytes(gid))
        return True

    def drop(gid):
        log.append(("drop", gid))
    t = Tiers(lru, demote, drop)
    t.budget["hbm"], t.budget["pinned"] = budget_hbm, budget_pinned
    return t, lru, log


def test_demote_then_drop_cascade_across_two_tiers():
    t, lru, log = _tiers(300, 200)
    for g in range(3):
        lru.add("hbm", g, 100)
    assert t.make_room("hbm", 100) and log == [("demote", 0)]
    lru.add("hbm", 3, 100)
    assert t.make_room("hbm", 200)
    # pinned holds 200: group 0 was its LRU and had to go before group 2 could come down
    assert log == [("demote", 0), ("demote", 1), ("drop", 0), ("demote", 2)]
    assert lru.groups("pinned") == [1, 2] and lru.groups("hbm") == [3]
    assert (t.demotions, t.evictions) == (3, 1)
    assert lru.live("hbm") <= 300 and lru.live("pinned") <= 200


def test_hbm_budget_alone_drops_and_a_failed_demotion_drops_too():
    t, lru, log = _tiers(200, None)
    for g in range(3):
        lru.add("hbm", g, 100)
    t.enforce()
    assert log == [("drop", 0)] and lru.groups("hbm") == [1, 2] and t.evictions == 1
    t, lru, log = _tiers(100, 1000, demote_ok=False)
    lru.add("hbm", 7, 100)
    lru.add("hbm", 8, 100)
    t.enforce()
    assert log == [("demote", 7), ("drop", 7)] and lru.groups("hbm") == [8] and (t.demotions, t.evictions) == (0, 1)


def test_an_oversize_group_disturbs_nobody():
    t, lru, log = _tiers(300, 1000)
    for g in range(3):
        lru.add("hbm", g, 100)
    assert t.place(301) == "pinned" and t.place(300) == "hbm" and t.place(1001) is None
    assert log == [] and lru.groups("hbm") == [0, 1, 2]
    t2, _, _ = _tiers(300, None)
    assert t2.place(301) is None  # no pinned tier to fall to
    # a group in a tier that is larger than the pinned budget is dropped, not demoted
    t3, lru3, log3 = _tiers(100, 50)
    lru3.add("hbm", 0, 100)
    lru3.add("hbm", 1, 100)
    t3.enforce()
    assert log3 == [("drop", 0)]


def test_parse_bytes():
    assert parse_bytes(None) is None and parse_bytes("") is None
    assert (parse_bytes("1536"), parse_bytes("64K"), parse_bytes("2m"), parse_bytes("3G"), parse_bytes("1GB")) == \
        (1536, 64 << 10, 2 << 20, 3 << 30, 1 << 30)
    with pytest.raises(ValueError):
        parse_bytes("lots")


# ---- the three symbols --------------------------------------------------------------------------------------------------
def test_pack_chunk_bytes_matches_the_oracle_and_refuses_a_truncated_pack(oracle):
    L = native.lib()
    for name in ("lmc_pack_blobs", "lmc_unpack_blobs", "lmc_pack_chunk_bytes"):
        assert name in native.SYMBOLS and getattr(L, name).argtypes == native.SYMBOLS[name][1]
    Ln, H, D, cs, T = 2, 1, 72, 32, 71     # two full chunks and a ragged one of 7 tokens
    g = torch.Generator().manual_seed(5)
    x = torch.randn(Ln, 2, T, H * D, generator=g).to(torch.bfloat16)
    bins = np.array([32, 16, 32, 16], np.int32)
    blobs = []
    for t0 in range(0, T, cs):
        bits, code = oracle.torch_to_bits(x[:, :, t0:t0 + cs].contiguous())
        blobs.append(oracle.encode_blob(bits, code, H, D, bins))
    pack = oracle.pack_from_blobs(blobs, cs)
    buf = (ctypes.c_uint8 * (len(pack) + 16))()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    ctypes.memmove(base, pack, len(pack))
    for i, b in enumerate(blobs):
        assert native.pack_chunk_bytes(base, len(pack), i) == len(b)
        assert native.pack_extract(base, len(pack), i) == b
    for bad in (len(blobs), -1):
        with pytest.raises(native.NativeError):
            native.pack_chunk_bytes(base, len(pack), bad)
    with pytest.raises(native.NativeError):
        native.pack_chunk_bytes(base, len(pack) - 16, 0)
