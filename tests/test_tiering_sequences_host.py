"""Tiers over GroupLRU (lmcache_amd/storage_backend/tiering.py) under random operation sequences, against a brute-force
model (no GPU).

The model is a plain list of [gid, tier, nbytes] rows in use order, least recently used first, scanned linearly for every
decision; it never calls victims, make_room or touch_chain.  The movers are fakes that do what LMCLocalBackend's do to the
LRU: `demote` re-files the group in the pinned tier at its pinned size (a pack is a little larger than its blobs), fails
every FAIL_EVERY-th call, and on every FULL_EVERY-th call finds the pinned arena "too fragmented" first and makes room there
itself by take_lru("pinned", keep=[gid]), as _demote_group does on ArenaFull; `drop` only records.  The operations
(tests/tier_sequences.py, host_ops): add, a store (place, make_room, add, enforce), touch, touch_chain of 1 to 4 groups
with repeats, resize, remove, budgets of None / 0 / a few group sizes, make_room, take_lru, enforce, and a promotion as
_promote_group files one.  Every fourth sequence runs without a demote mover (a backend that only drops).

Behind every operation: per tier the order, the sizes and the live bytes equal the model's; demotions, promotions and
evictions equal the model's counts; the movers were called for the same groups in the same order; every group taken out
was, at that moment, the least recently used group of its tier outside the `keep` of the call that took it (so: never a
kept one, and LRU first); make_room -> True means live + need <= budget, False means no group outside `keep` is left in
that tier; a chain that touch_chain touched lies at the recent end of each tier from its tail to its head.

240 sequences of 300 operations (8 cases of 30): 1.3 s for the whole file on one CPU core, 5 ms per sequence.
"""
import pytest

from lmcache_amd.storage_backend.tiering import GroupLRU, Tiers
from tests.tier_sequences import host_ops

TIERS = ("hbm", "pinned")
FAIL_EVERY, FULL_EVERY = 5, 4


def _pinned_size(gid: int, nbytes: int) -> int:
    return nbytes + 16 * (gid % 3)


class Model:
    """What Tiers and GroupLRU should do, the slow way."""

    def __init__(self, demotes: bool):
        self.rows = []               # [gid, tier, nbytes], least recently used first
        self.budget = {"hbm": None, "pinned": None}
        self.demotes = demotes
        self.demotions = self.promotions = self.evictions = 0
        self.calls = 0               # of the demote mover
        self.log = []                # ("demote", gid, ok) / ("drop", gid)

    # ---- the list
    def row(self, gid):
        for r in self.rows:
            if r[0] == gid:
                return r
        return None

    def tier_of(self, gid):
        r = self.row(gid)
        return r[1] if r else None

    def order(self, tier):
        return [(r[0], r[2]) for r in self.rows if r[1] == tier]

    def live(self, tier):
        return sum(r[2] for r in self.rows if r[1] == tier)

    def remove(self, gid):
        self.rows = [r for r in self.rows if r[0] != gid]

    def add(self, tier, gid, nbytes):
        self.remove(gid)
        self.rows.append([gid, tier, nbytes])

    def touch(self, gid):
        r = self.row(gid)
        if r is not None:
            self.rows.remove(r)
            self.rows.append(r)

    def touch_chain(self, gids):
        chain = []
        for g in gids:
            if g not in chain:
                chain.append(g)
        for g in chain[::-1]:        # the head of the chain ends up the most recent
            self.touch(g)

    def resize(self, gid, nbytes):
        self.row(gid)[2] = nbytes

    # ---- the budgets
    def tiered(self):
        return self.demotes and self.budget["hbm"] is not None and self.budget["pinned"] is not None

    def place(self, nbytes, pinned_bytes):
        b = self.budget["hbm"]
        if b is None or nbytes <= b:
            return "hbm"
        if self.tiered() and pinned_bytes <= self.budget["pinned"]:
            return "pinned"
        return None

    def lru_outside(self, tier, keep):
        for r in self.rows:
            if r[1] == tier and r[0] not in keep:
                return r[0]
        return None

    def make_room(self, tier, need, keep):
        b = self.budget[tier]
        if b is None:
            return True
        while self.live(tier) + need > b:
            gid = self.lru_outside(tier, keep)
            if gid is None:
                break
            self.take_out(tier, gid, keep)
        return self.live(tier) + need <= b

    def take_out(self, tier, gid, keep):
        if tier == "hbm" and self.tiered():
            nb = _pinned_size(gid, self.row(gid)[2])
            if nb <= self.budget["pinned"] and self.make_room("pinned", nb, keep) and self.demote(gid):
                self.demotions += 1
                return
        if self.tier_of(gid) == tier:
            self.log.append(("drop", gid))
            self.remove(gid)
            self.evictions += 1

    def demote(self, gid):
        self.calls += 1
        ok = self.calls % FAIL_EVERY != 0
        if ok and self.calls % FULL_EVERY == 0:
            ok = self.take_lru("pinned", [gid])   # "ArenaFull": the pinned tier's LRU group goes, or the demotion fails
        if ok:
            self.add("pinned", gid, _pinned_size(gid, self.row(gid)[2]))
        self.log.append(("demote", gid, ok))
        return ok

    def take_lru(self, tier, keep):
        gid = self.lru_outside(tier, keep)
        if gid is None:
            return False
        self.take_out(tier, gid, keep)
        return True

    def enforce(self, keep):
        self.make_room("hbm", 0, keep)
        self.make_room("pinned", 0, keep)


class Real:
    """Tiers over GroupLRU with the fake movers; every take-out is checked where it happens."""

    def __init__(self, demotes: bool):
        self.lru = GroupLRU()
        self.tiers = Tiers(self.lru, self.demote if demotes else None, self.drop,
                           pinned_size=lambda gid: _pinned_size(gid, self.lru.nbytes(gid)))
        self.calls, self.log, self.keeps, self.wrong = 0, [], [()], []

    def taken(self, gid):
        """`gid` is being taken out of its tier by the call whose keep is on top of the stack."""
        keep, tier = self.keeps[-1], self.lru.tier_of(gid)
        first = next((g for g in self.lru.groups(tier) if g not in keep), None)
        if gid in keep:
            self.wrong.append(f"group {gid} was taken out of {tier} though it is in keep {list(keep)}")
        elif gid != first:
            self.wrong.append(f"group {gid} was taken out of {tier}, the LRU group outside keep {list(keep)} is {first}")

    def drop(self, gid):
        self.taken(gid)
        self.log.append(("drop", gid))

    def demote(self, gid):
        self.taken(gid)
        self.calls += 1
        ok = self.calls % FAIL_EVERY != 0
        if ok and self.calls % FULL_EVERY == 0:
            self.keeps.append((gid,))
            try:
                ok = self.tiers.take_lru("pinned", keep=[gid])
            finally:
                self.keeps.pop()
        if ok:
            self.lru.add("pinned", gid, _pinned_size(gid, self.lru.nbytes(gid)))
        self.log.append(("demote", gid, ok))
        return ok

    def call(self, keep, fn, *args):
        self.keeps.append(tuple(keep))
        try:
            return fn(*args)
        finally:
            self.keeps.pop()


def _run(seed: int, nops: int = 300) -> dict:
    demotes = seed % 4 != 3
    ops = host_ops(seed, nops)
    real, model = Real(demotes), Model(demotes)
    lru, tiers = real.lru, real.tiers
    seen = {"demotions": 0, "evictions": 0, "promotions": 0, "failed demotions": 0, "refused": 0, "could not fit": 0}
    for i, op in enumerate(ops):
        where = f"seed {seed}, operation {i} {op!r} of host_ops({seed}, {nops})[:{i + 1}]"
        kind = op[0]
        if kind == "add":
            _, gid, nb = op
            tier = tiers.place(nb, _pinned_size(gid, nb))
            assert tier == model.place(nb, _pinned_size(gid, nb)), where
            if tier is None:
                seen["refused"] += 1
            else:
                size = nb if tier == "hbm" else _pinned_size(gid, nb)
                lru.add(tier, gid, size)
                model.add(tier, gid, size)
        elif kind == "store":        # LMCLocalBackend._store: place, make room, file, enforce
            _, gid, nb = op
            tier = tiers.place(nb, _pinned_size(gid, nb))
            assert tier == model.place(nb, _pinned_size(gid, nb)), where
            if tier is None:
                seen["refused"] += 1
            else:
                size = nb if tier == "hbm" else _pinned_size(gid, nb)
                ok = real.call((), tiers.make_room, tier, size)
                assert ok == model.make_room(tier, size, ()), where
                if ok:
                    lru.add(tier, gid, size)
                    model.add(tier, gid, size)
                    real.call((), tiers.enforce)
                    model.enforce(())
        elif kind == "touch":
            lru.touch(op[1])
            model.touch(op[1])
        elif kind == "touch_chain":
            lru.touch_chain(op[1])
            model.touch_chain(op[1])
            chain = [g for k, g in enumerate(op[1]) if g not in op[1][:k]]
            for t in TIERS:          # eaten from its tail: at the recent end of each tier, the tail first, the head last
                part = [g for g in reversed(chain) if lru.tier_of(g) == t]
                assert lru.groups(t)[len(lru.groups(t)) - len(part):] == part, f"{where}: {t} is {lru.groups(t)}"
        elif kind == "resize":
            if lru.tier_of(op[1]) is not None:
                lru.resize(op[1], op[2])
                model.resize(op[1], op[2])
        elif kind == "remove":
            lru.remove(op[1])
            model.remove(op[1])
        elif kind == "budget":
            tiers.budget[op[1]] = model.budget[op[1]] = op[2]
        elif kind == "make_room":
            _, tier, need, keep = op
            ok = real.call(keep, tiers.make_room, tier, need, keep)
            assert ok == model.make_room(tier, need, keep), where
            b = tiers.budget[tier]
            if ok:
                assert b is None or lru.live(tier) + need <= b, where
            else:
                seen["could not fit"] += 1
                assert all(g in keep for g in lru.groups(tier)), f"{where}: refused with {lru.groups(tier)} still in {tier}"
        elif kind == "take_lru":
            _, tier, keep = op
            assert real.call(keep, tiers.take_lru, tier, keep) == model.take_lru(tier, keep), where
        elif kind == "enforce":
            real.call(op[1], tiers.enforce, op[1])
            model.enforce(op[1])
            for t in TIERS:
                b = tiers.budget[t]
                assert b is None or lru.live(t) <= b or all(g in op[1] for g in lru.groups(t)), where
        else:                        # LMCLocalBackend._promote_group's bookkeeping
            gid = op[1]
            if lru.tier_of(gid) != "pinned" and lru.count("pinned"):
                gid = lru.groups("pinned")[gid % lru.count("pinned")]  # (the operation names a group that is not there: another)
            if lru.tier_of(gid) == "pinned" and tiers.tiered():
                nb = max(16, lru.nbytes(gid) - 16 * (gid % 3))
                ok = nb <= tiers.budget["hbm"] and real.call([gid], tiers.make_room, "hbm", nb, [gid])
                assert ok == (nb <= model.budget["hbm"] and model.make_room("hbm", nb, [gid])), where
                if ok and lru.tier_of(gid) == "pinned":
                    lru.add("hbm", gid, nb)
                    model.add("hbm", gid, nb)
                    tiers.promotions += 1
                    model.promotions += 1
                    real.call([gid], tiers.enforce, [gid])
                    model.enforce([gid])
        assert not real.wrong, f"{where}: {real.wrong[0]}"
        assert real.log == model.log, f"{where}: movers called {real.log[-6:]}, the model says {model.log[-6:]}"
        for t in TIERS:
            got = [(g, lru.nbytes(g)) for g in lru.groups(t)]
            assert got == model.order(t), f"{where}: {t} holds {got}, the model {model.order(t)}"
            assert lru.live(t) == model.live(t) and lru.count(t) == len(got), where
            assert all(lru.tier_of(g) == t for g, _ in got), where
        assert (tiers.demotions, tiers.promotions, tiers.evictions) == (model.demotions, model.promotions, model.evictions), where
    seen.update(demotions=tiers.demotions, evictions=tiers.evictions, promotions=tiers.promotions,
                **{"failed demotions": sum(1 for e in real.log if e[0] == "demote" and not e[2])})
    return seen


@pytest.mark.parametrize("block", range(8))
def test_tiers_and_lru_follow_the_brute_force_model_through_random_sequences(block):
    total = {}
    for seed in range(30 * block, 30 * block + 30):
        for k, v in _run(seed).items():
            total[k] = total.get(k, 0) + v
    # the sequences reach what they were written for (30 sequences of 300 operations each block)
    assert total["demotions"] > 30 and total["evictions"] > 30 and total["promotions"] > 5, total
    assert total["failed demotions"] > 5 and total["refused"] > 5 and total["could not fit"] > 5, total


def test_a_demotion_that_makes_its_own_room_in_the_pinned_tier():
    """The shortest case of the mover that calls take_lru("pinned", keep=[gid]) itself: the fourth demotion finds the
    pinned arena full, the pinned tier's LRU group (the first one demoted) goes, and the group lands."""
    real = Real(True)
    real.tiers.budget["hbm"], real.tiers.budget["pinned"] = 0, 10000
    for gid in (0, 3, 6, 9):         # (multiples of 3: the same size in both tiers)
        real.lru.add("hbm", gid, 160)
    real.call((), real.tiers.enforce)
    assert not real.wrong
    assert real.log == [("demote", 0, True), ("demote", 3, True), ("demote", 6, True), ("drop", 0), ("demote", 9, True)]
    assert real.lru.groups("pinned") == [3, 6, 9] and real.lru.groups("hbm") == []
    assert (real.tiers.demotions, real.tiers.evictions) == (4, 1)


# ---- the arenas: what the engine-level sequences found (tests/test_gpu_tier_sequences.py), at the level of the arena ----
class _Buffer:
    def __init__(self, nbytes):
        self.nbytes, self.ptr, self.freed = nbytes, 1 << 40, False

    def free(self):
        self.freed = True


class _Stream:
    def __init__(self):
        self.waited = []

    def wait_event(self, e):
        self.waited.append(e)


class _Event:
    def query(self):
        return False


def _arena(kind, **kw):
    import torch
    from lmcache_amd.storage_backend.serde.cachegen_device import DeviceArena, PinnedArena
    if kind == "pinned":
        return PinnedArena(slab_bytes=4096, buffer_factory=_Buffer, **kw), (lambda x: x.offset)
    a = DeviceArena(torch.device("cpu"), slab_bytes=4096, **kw)   # (plain host tensors stand in for HBM)
    return a, (lambda x: x.data_ptr() - a._slabs[0].data_ptr())


def _one_hole_each(a):
    return all(a._fl.is_empty(sid) for sid in a._fl.slabs)


@pytest.mark.parametrize("kind", ["pinned", "device"])
def test_what_an_unbounded_arena_was_given_back_is_free_once_it_is_bounded(kind):
    """A key stored again while no budget is set gives its old bytes back to a bump allocator, which only counts them.  When
    a budget is set later those bytes must be holes -- with the events of whoever may still read them -- and not live bytes
    that nothing will ever free: the tier would cache that much less than its budget, down to nothing."""
    a, offset = _arena(kind)
    x, y, z = a.alloc(1000), a.alloc(1000), a.alloc(1000)
    ev, st = _Event(), _Stream()
    a.free(y, [ev])
    assert a.live_bytes == 2016
    a.set_budget(3100)
    assert a.live_bytes == 2016 and a.reserved_bytes == 4096
    w = a.alloc(1000, streams=[st]) if kind == "pinned" else a.alloc(1000, stream=st)
    assert offset(w) == 1008 and st.waited == [ev], "the hole of the freed region, behind its reader's event"
    from lmcache_amd.storage_backend.serde.cachegen_device import ArenaFull
    with pytest.raises(ArenaFull):
        a.alloc(100)                             # 3024 live + 112 > 3100
    for r in (x, w, z):
        a.free(r)
    assert a.live_bytes == 0 and _one_hole_each(a)


def test_a_pack_tail_an_unbounded_pinned_arena_could_not_cut_is_named_and_comes_back():
    """Two stores that overlap: the first pack is cut to size when the second one's region lies behind it already.  The
    bump allocator cannot take the tail back: it stays counted (cut_bytes says how much) and is a hole once a budget is set."""
    a, _ = _arena("pinned")
    first, second = a.alloc(2000), a.alloc(1000)
    first = a.shrink(first, 500)
    assert (a.live_bytes, a.cut_bytes) == (2000 + 1008, 2000 - 512)
    a.set_budget(4096)
    assert (a.live_bytes, a.cut_bytes) == (512 + 1008, 0)
    assert a.alloc(1488).offset == 512           # exactly the tail
    a.free(first)
    a.free(second)
    assert a.live_bytes == 1488


@pytest.mark.parametrize("kind", ["pinned", "device"])
def test_a_budget_that_shrinks_sends_empty_slabs_back_at_once(kind):
    a, _ = _arena(kind, budget=12000)
    x, y = a.alloc(4000), a.alloc(4000)          # two slabs
    a.free(y)                                    # within the budget: the empty slab is kept for the next allocation
    assert a.reserved_bytes == 8192
    a.set_budget(5000)                           # no free() follows that would notice: set_budget itself must
    assert a.reserved_bytes == 4096 and a.live_bytes == 4000
    a.free(x)
    assert a.live_bytes == 0
