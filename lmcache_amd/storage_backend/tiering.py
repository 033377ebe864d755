"""Bookkeeping of the bounded local tiers: what is free in an arena, and which store group goes next.

Nothing here touches torch.cuda or the HIP library: regions are abstract (slab id, offset, size) records, events are
whatever objects the caller hands in, and the movers of `Tiers` are callbacks -- the arenas (storage_backend/arena.py)
and LMCLocalBackend put memory and kernels behind them.

  FreeList   first-fit over the slabs of one arena with coalescing, and an optional byte budget.  A freed region
             carries the events of whoever may still read or write it (a decode launched from it, a DMA out of it);
             they are handed to the next allocation that overlaps it, whose stream waits for them.
  GroupLRU   the store groups of every tier in LRU order.  A group is the chunks of ONE put call (what a pack holds:
             consecutive links of one hash chain).
  Tiers      budgets over a GroupLRU: who is demoted, who is dropped, in which order.
"""
from collections import OrderedDict
from typing import Callable, Dict, Iterable, List, Optional, Sequence, Tuple

GRANULE = 16


def r16(x: int) -> int:
    return (x + 15) & ~15


def parse_bytes(text: Optional[str]) -> Optional[int]:
    """"1536", "64K", "512M", "4G" (binary multiples) -> bytes; None / "" -> None (unbounded)."""
    if text is None or not str(text).strip():
        return None
    t = str(text).strip().upper()
    if t.endswith("B") and len(t) > 1 and t[-2] in "KMG":
        t = t[:-1]
    mult = {"K": 1 << 10, "M": 1 << 20, "G": 1 << 30}.get(t[-1], 1)
    if mult != 1:
        t = t[:-1]
    n = int(t) * mult
    if n < 0:
        raise ValueError(f"a byte budget cannot be negative: {text!r}")
    return n


class FreeList:
    """Free regions of an arena's slabs.  Sizes and offsets are multiples of 16 (the caller rounds).

    budget: live bytes never exceed it (alloc returns None instead), and room_for_slab() says how large a slab may
    still be taken from the system so that the RESERVED bytes -- the sum of the slab sizes -- do not exceed it either.
    done(event) -> True lets a completed event be forgotten when holes are merged (None: events are kept)."""

    def __init__(self, budget: Optional[int] = None, done: Optional[Callable] = None):
        self.budget = budget
        self.slabs: "OrderedDict[object, int]" = OrderedDict()   # slab id -> bytes
        self.holes: Dict[object, List[list]] = {}                 # slab id -> [[offset, size, [events]], ...] by offset
        self.live = 0
        self._done = done

    @property
    def reserved(self) -> int:
        return sum(self.slabs.values())

    def add_slab(self, sid, size: int, used: int = 0) -> None:
        """A slab of `size` bytes whose first `used` bytes are live (an arena that turns bounded hands over its bump
        pointer this way)."""
        assert sid not in self.slabs and 0 <= used <= size
        self.slabs[sid] = size
        self.holes[sid] = [[used, size - used, []]] if used < size else []
        self.live += used

    def drop_slab(self, sid) -> None:
        """Forget a slab that is one hole (the caller returns its memory to the system)."""
        assert self.is_empty(sid)
        del self.slabs[sid], self.holes[sid]

    def is_empty(self, sid) -> bool:
        h = self.holes[sid]
        return len(h) == 1 and h[0][0] == 0 and h[0][1] == self.slabs[sid]

    def room_for_slab(self) -> Optional[int]:
        """Bytes a new slab may have (None: no budget)."""
        return None if self.budget is None else max(0, self.budget - self.reserved)

    def fits_budget(self, need: int) -> bool:
        return self.budget is None or self.live + need <= self.budget

    def alloc(self, need: int) -> Optional[Tuple[object, int, list]]:
        """First fit -> (slab id, offset, events the new owner must wait for), or None: over budget, or no hole is
        large enough (the caller adds a slab if room_for_slab() allows, or evicts)."""
        assert need > 0 and need % GRANULE == 0
        if not self.fits_budget(need):
            return None
        for sid, holes in self.holes.items():
            for k, (off, size, events) in enumerate(holes):
                if size >= need:
                    if size == need:
                        holes.pop(k)
                    else:
                        holes[k] = [off + need, size - need, events]  # the rest may have been read by the same jobs
                    self.live += need
                    return sid, off, list(events)
        return None

    def free(self, sid, off: int, size: int, events: Iterable = ()) -> None:
        """[off, off + size) of slab `sid` is free once `events` have fired; merged with its free neighbours."""
        assert size > 0 and off % GRANULE == 0 and size % GRANULE == 0 and off + size <= self.slabs[sid]
        holes = self.holes[sid]
        k = 0
        while k < len(holes) and holes[k][0] < off:
            k += 1
        assert (k == 0 or holes[k - 1][0] + holes[k - 1][1] <= off) and (k == len(holes) or off + size <= holes[k][0]), \
            "freed region overlaps a free one"
        cur = [off, size, list(events)]
        if k < len(holes) and holes[k][0] == off + size:
            nxt = holes.pop(k)
            cur = [off, size + nxt[1], self._merge(cur[2], nxt[2])]
        if k > 0 and holes[k - 1][0] + holes[k - 1][1] == off:
            prv = holes.pop(k - 1)
            k -= 1
            cur = [prv[0], prv[1] + cur[1], self._merge(prv[2], cur[2])]
        holes.insert(k, cur)
        self.live -= size

    def _merge(self, a: list, b: list) -> list:
        out = list(a)
        out += [e for e in b if not any(e is x for x in out)]
        if self._done is not None:
            out = [e for e in out if not self._done(e)]
        return out


class GroupLRU:
    """Store groups per tier, least recently used first."""

    def __init__(self, tiers: Sequence[str] = ("hbm", "pinned")):
        self._order: Dict[str, "OrderedDict[int, int]"] = {t: OrderedDict() for t in tiers}
        self._tier: Dict[int, str] = {}

    def add(self, tier: str, gid: int, nbytes: int) -> None:
        """A new group, or a group that has moved: most recently used of `tier`."""
        self.remove(gid)
        self._order[tier][gid] = nbytes
        self._tier[gid] = tier

    def remove(self, gid: int) -> None:
        t = self._tier.pop(gid, None)
        if t is not None:
            del self._order[t][gid]

    def touch(self, gid: int) -> None:
        t = self._tier.get(gid)
        if t is not None:
            self._order[t].move_to_end(gid)

    def touch_chain(self, gids: Iterable[int]) -> None:
        """A hit that read these groups, in chain order: touched from the last to the first, so that the head of the
        chain ends up the most recent and a chain is eaten from its tail (the prefix probe stops at the first miss:
        a tail without its head would be dead weight)."""
        seen, chain = set(), []
        for g in gids:
            if g not in seen:
                seen.add(g)
                chain.append(g)
        for g in reversed(chain):
            self.touch(g)

    def tier_of(self, gid: int) -> Optional[str]:
        return self._tier.get(gid)

    def nbytes(self, gid: int) -> int:
        return self._order[self._tier[gid]][gid]

    def resize(self, gid: int, nbytes: int) -> None:
        """The group counts for `nbytes` from now on (part of its memory has been released); its place in the order stays."""
        self._order[self._tier[gid]][gid] = nbytes

    def live(self, tier: str) -> int:
        return sum(self._order[tier].values())

    def count(self, tier: str) -> int:
        return len(self._order[tier])

    def groups(self, tier: str) -> List[int]:
        """LRU first."""
        return list(self._order[tier])

    def victims(self, tier: str, budget: int, need: int = 0, keep: Iterable[int] = ()) -> List[int]:
        """The groups to take out of `tier`, LRU first, so that its live bytes + need fit the budget (`keep` are never
        chosen).  Fewer than needed if the tier cannot be made to fit."""
        keep = set(keep)
        live, out = self.live(tier), []
        for gid, nb in self._order[tier].items():
            if live + need <= budget:
                break
            if gid in keep:
                continue
            out.append(gid)
            live -= nb
        return out


class Tiers:
    """Budgets over a GroupLRU.  `demote(gid) -> bool` moves a group from "hbm" to "pinned" (False: it could not, the
    group is dropped instead), `drop(gid)` forgets a group; both are called with the group still filed where it was and
    re-file it themselves (add / remove), so the bytes this class counts are the caller's."""

    def __init__(self, lru: GroupLRU, demote: Optional[Callable[[int], bool]], drop: Callable[[int], None],
                 pinned_size: Optional[Callable[[int], int]] = None):
        """pinned_size(gid): the bytes an HBM group takes once demoted (a pack is a little larger than its blobs: table,
        padded static slots); None: the same as in HBM."""
        self.lru, self._demote, self._drop = lru, demote, drop
        self._pinned_size = pinned_size or lru.nbytes
        self.budget: Dict[str, Optional[int]] = {"hbm": None, "pinned": None}
        self.demotions = self.promotions = self.evictions = 0

    def tiered(self) -> bool:
        return self._demote is not None and self.budget["hbm"] is not None and self.budget["pinned"] is not None

    def place(self, nbytes: int, pinned_bytes: Optional[int] = None) -> Optional[str]:
        """Where a new group of `nbytes` (pinned_bytes: its size as a pack, if that differs) goes: "hbm", "pinned"
        (tiered: larger than the whole HBM budget) or None -- it fits nowhere, and nothing is evicted for it."""
        b = self.budget["hbm"]
        if b is None or nbytes <= b:
            return "hbm"
        if self.tiered() and (nbytes if pinned_bytes is None else pinned_bytes) <= self.budget["pinned"]:
            return "pinned"
        return None

    def _evict(self, gid: int) -> None:
        self._drop(gid)
        self.lru.remove(gid)
        self.evictions += 1

    def make_room(self, tier: str, need: int = 0, keep: Iterable[int] = ()) -> bool:
        """Take LRU groups out of `tier` until live + need <= its budget: demoted if this is the HBM tier of a tiered
        pair (dropping the pinned tier's LRU groups first when that is full), else dropped.  -> whether it fits now."""
        b = self.budget[tier]
        if b is None:
            return True
        keep = list(keep)
        for gid in self.lru.victims(tier, b, need, keep):
            self._take_out(tier, gid, keep)
        return self.lru.live(tier) + need <= b

    def _take_out(self, tier: str, gid: int, keep: list) -> None:
        if tier == "hbm" and self.tiered():
            nb = self._pinned_size(gid)
            if nb <= self.budget["pinned"] and self.make_room("pinned", nb, keep) and self._demote(gid):
                self.demotions += 1
                return
        if self.lru.tier_of(gid) == tier:
            self._evict(gid)

    def take_lru(self, tier: str, keep: Iterable[int] = ()) -> bool:
        """Take the LRU group out of `tier` whatever the budget says (an arena too fragmented for an allocation that
        the byte count allows) -> False: there is none."""
        keep = list(keep)
        for gid in self.lru.groups(tier):
            if gid not in keep:
                self._take_out(tier, gid, keep)
                return True
        return False

    def enforce(self, keep: Iterable[int] = ()) -> None:
        """Both tiers back under their budgets (after a store, a promotion, a budget that shrank)."""
        self.make_room("hbm", 0, keep)
        self.make_room("pinned", 0, keep)
