"""The slab arenas of the local tiers: SlabArena, and what it is over pinned host DRAM (PinnedArena) and HBM (DeviceArena).

An arena hands out 16-byte-granular regions of slabs it takes from the system.  Without a budget it is a bump allocator
that returns memory at close() (the reference never evicts, hybrid_backend.py:24): free() only counts.  With a byte budget
(constructor, or set_budget() later) regions come from a first-fit free list with coalescing (tiering.FreeList), free()
gives them back, and the bytes reserved from the system -- the sum of the slab sizes -- never exceed the budget (an arena
that was unbounded before keeps the slabs it has that still hold live bytes; it takes no new one while it is over, and
what it was given back while unbounded becomes holes).  A freed region carries the events of whoever may still read it;
alloc() makes the streams of the next owner wait for them.

The free list knows a slab by id(slab): the slabs are buffers or tensors (`==` of a tensor is elementwise), and every one
the free list knows is in `_slabs`, so its id is its own for as long.
"""
import ctypes
import threading
from dataclasses import dataclass
from typing import List, Optional, Sequence

import torch

from lmcache_amd import native
from lmcache_amd.storage_backend.tiering import FreeList, r16


class ArenaFull(MemoryError):
    """A bounded arena cannot take the allocation: over its budget, or no hole is large enough."""


def _event_done(ev) -> bool:
    try:
        return bool(ev.query())
    except Exception:
        return False


def _stream_waits(stream, events) -> None:
    """`stream` runs behind `events` (torch events or native.NativeEvent): a stream-side wait, never a host wait."""
    for ev in events:
        if isinstance(ev, native.NativeEvent):
            ev.wait(stream.cuda_stream)
        else:
            stream.wait_event(ev)


class SlabArena:
    """What both arenas do.  A subclass says how a slab is made (_new_slab(size) -> an object with .nbytes) and given
    back (_release_slab), what the caller gets for (slab, offset, nbytes) and how that maps back (_handle, _locate), and
    who waits for a region's previous owner when the caller names no stream (_default_streams)."""

    name = "arena"                  # in ArenaFull's message
    release_newest_first = False    # over budget: which of the slabs that are one hole goes back to the system first

    def __init__(self, slab_bytes: int, budget: Optional[int] = None):
        self.slab_bytes = slab_bytes
        self._slabs: list = []
        self._tops: List[int] = []      # unbounded: the bump pointer each earlier slab was left at
        self._used = 0                  # ... and that of the newest slab
        self._live = 0                  # ... and the bytes handed out and not given back
        # unbounded: the regions given back so far, (slab, offset, size, events) -- only counted while the arena is a bump
        # allocator, holes of the free list once it turns bounded
        self._freed: List[tuple] = []
        self._fl: Optional[FreeList] = None
        self._lock = threading.Lock()
        if budget is not None:
            self.set_budget(budget)

    def _release_slab(self, slab) -> None:
        pass

    def _default_streams(self) -> Sequence:
        return ()

    def _grow(self, need: int, hint: int):
        """Unbounded: the slab the bump pointer moves to."""
        return self._new_slab(max(self.slab_bytes, need, hint))

    @property
    def budget(self) -> Optional[int]:
        return self._fl.budget if self._fl is not None else None

    @property
    def live_bytes(self) -> int:
        return self._fl.live if self._fl is not None else self._live

    @property
    def reserved_bytes(self) -> int:
        return sum(s.nbytes for s in self._slabs)

    def set_budget(self, budget: Optional[int]) -> None:
        """Bound the arena from now on (None on an unbounded arena: nothing changes; a bounded arena stays a free list
        and only loses its limit).  What the bump allocator has handed out so far and not been given back counts as
        live; what was given back meanwhile becomes holes.  Slabs that are one hole go back to the system while the
        arena is over the new budget."""
        with self._lock:
            if self._fl is not None:
                self._fl.budget = budget
            elif budget is not None:
                self._fl = self._to_free_list(budget)
            else:
                return
            self._release_empty_locked()

    def _to_free_list(self, budget: int) -> FreeList:
        fl = FreeList(budget, _event_done)
        for slab, top in zip(self._slabs, self._tops + [self._used]):
            fl.add_slab(id(slab), slab.nbytes, top)
        for slab, off, size, events in self._freed:
            fl.free(id(slab), off, size, events)
        self._freed = []
        return fl

    def _release_empty_locked(self, until: int = 0) -> None:
        """Slabs that are one hole go back to the system while the arena is over its budget (an arena bounded after the
        fact), or -- until > 0 -- until the budget leaves room for a new slab of `until` bytes.  A slab whose last
        readers have not finished is waited for: the one host wait of the arena, on the rare path where memory has to
        change hands with the system."""
        fl = self._fl
        if fl.budget is None:
            return
        for slab in self._slabs[::-1] if self.release_newest_first else self._slabs[:]:
            if fl.reserved <= fl.budget and (until <= 0 or fl.budget - fl.reserved >= until):
                break
            if fl.is_empty(id(slab)):
                for e in fl.holes[id(slab)][0][2]:
                    if not _event_done(e) and hasattr(e, "synchronize"):
                        e.synchronize()
                fl.drop_slab(id(slab))
                self._slabs = [s for s in self._slabs if s is not slab]
                self._release_slab(slab)

    def _alloc_bounded(self, need: int, hint: int, streams: Sequence) -> tuple:
        fl = self._fl
        got = fl.alloc(need)
        if got is None and fl.fits_budget(need):
            room = fl.room_for_slab()
            if room is not None and room < need:
                # no hole takes it and the budget leaves no slab of its size: slabs that are one hole go back to the
                # system first (an arena whose groups have all gone must take a region larger than any slab it has)
                self._release_empty_locked(until=need)
                room = fl.room_for_slab()
            size = max(self.slab_bytes, need, hint)
            if room is not None:  # (None: a bounded arena whose limit has been taken away again)
                size = min(size, room) & ~15
            if size >= need:
                slab = self._new_slab(size)
                self._slabs.append(slab)
                fl.add_slab(id(slab), size)
                got = fl.alloc(need)
        if got is None:
            raise ArenaFull(f"{self.name}: {need} bytes do not fit ({fl.live} live of a budget of {fl.budget})")
        sid, off, events = got
        if events:
            for st in streams or self._default_streams():
                _stream_waits(st, events)
        return next(s for s in self._slabs if id(s) == sid), off

    def _alloc(self, nbytes: int, hint: int = 0, streams: Sequence = ()):
        """hint: size of the slab to take if a new one is needed.  streams: who will write the region (bounded arena:
        they wait for the events of its previous owner).  Bounded and full: ArenaFull."""
        need = r16(max(nbytes, 16))
        with self._lock:
            if self._fl is not None:
                slab, off = self._alloc_bounded(need, hint, streams)
            else:
                if not self._slabs or self._used + need > self._slabs[-1].nbytes:
                    if self._slabs:
                        self._tops.append(self._used)
                    self._slabs.append(self._grow(need, hint))
                    self._used = 0
                slab, off = self._slabs[-1], self._used
                self._used += need
                self._live += need
            return self._handle(slab, off, nbytes)

    def free(self, handle, events: Sequence = ()) -> None:
        """Give back what alloc() returned; `events`: what may still read or write it.  An unbounded arena reuses
        nothing: it only counts."""
        with self._lock:
            slab, off, nbytes = self._locate(handle)
            size = r16(max(nbytes, 16))
            if self._fl is None:
                self._live -= size
                self._freed.append((slab, off, size, list(events)))
                return
            self._fl.free(id(slab), off, size, events)
            self._release_empty_locked()  # over budget (bounded after the fact): empty slabs go back

    def close(self):
        with self._lock:
            for s in self._slabs:
                self._release_slab(s)
            self._slabs, self._tops, self._used, self._live, self._freed = [], [], 0, 0, []
            if self._fl is not None:
                self._fl = FreeList(self._fl.budget, _event_done)


@dataclass
class HostBlob:
    """One encoded chunk resident in pinned host DRAM."""
    slab: native.PinnedBuffer
    offset: int
    nbytes: int

    @property
    def ptr(self) -> int:
        return self.slab.ptr + self.offset

    def tobytes(self) -> bytes:
        return ctypes.string_at(self.ptr, self.nbytes)


class PinnedArena(SlabArena):
    """The arena over hipHostMalloc'ed slabs; a region is a HostBlob.  Unbounded it can also take slabs ahead of need
    (reserve), cut a region to its size (shrink) and start over (reset)."""

    name = "pinned arena"

    def __init__(self, slab_bytes: int = 256 << 20, budget: Optional[int] = None, buffer_factory=None):
        self._new_slab = buffer_factory or native.PinnedBuffer
        self._spare: List[native.PinnedBuffer] = []   # slabs allocated ahead of need (reserve)
        # unbounded: how many of the bytes given back are tails that shrink() could not return to the bump pointer
        # (live_bytes still counts those)
        self.cut_bytes = 0
        super().__init__(slab_bytes, budget)

    def _release_slab(self, slab) -> None:
        slab.free()

    def _handle(self, slab, off: int, nbytes: int) -> HostBlob:
        return HostBlob(slab, off, nbytes)

    def _locate(self, hb: HostBlob) -> tuple:
        return hb.slab, hb.offset, hb.nbytes

    def _grow(self, need: int, hint: int):
        k = next((i for i, b in enumerate(self._spare) if b.nbytes >= need), None)
        return self._spare.pop(k) if k is not None else super()._grow(need, hint)

    def _to_free_list(self, budget: int) -> FreeList:
        for b in self._spare:  # (slabs the bump pointer has not reached: each one hole)
            if self._slabs:
                self._tops.append(self._used)
            self._slabs.append(b)
            self._used = 0
        self._spare, self.cut_bytes = [], 0
        return super()._to_free_list(budget)

    @property
    def total_allocated(self) -> int:
        return self.live_bytes

    @property
    def reserved_bytes(self) -> int:
        return sum(b.nbytes for b in self._slabs + self._spare)

    def alloc(self, nbytes: int, slab_hint: int = 0, streams: Sequence = ()) -> HostBlob:
        """slab_hint: size of the slab to allocate if a new one is needed (a pack is allocated at its bound and cut
        to its size afterwards: a slab of a few bounds keeps the cut-off tails usable).  streams: who will write the
        region (bounded arena: they wait for the events of its previous owner).  Bounded and full: ArenaFull."""
        return self._alloc(nbytes, slab_hint, streams)

    def shrink(self, hb: HostBlob, nbytes: int) -> HostBlob:
        """Give back the tail of `hb`.  Unbounded: only if it is still the arena's last allocation (a pack is allocated
        at its bound and cut to its size once the GPU has written it); otherwise the tail stays unused.  Bounded: the
        tail is freed like any region -- the budget was tested against the bound at alloc() and is corrected here
        (nbytes 0: the whole region goes back)."""
        keep, old = r16(max(nbytes, 16)), r16(max(hb.nbytes, 16))
        with self._lock:
            if self._fl is not None:
                if nbytes <= 0:
                    keep = 0
                if old > keep:
                    self._fl.free(id(hb.slab), hb.offset + keep, old - keep)
            elif self._slabs and hb.slab is self._slabs[-1] and hb.offset + old == self._used:
                self._live -= self._used - (hb.offset + keep)
                self._used = hb.offset + keep
            elif old > keep:
                # (another allocation lies behind it: the tail stays unused and counted; a hole once the arena is bounded)
                self._freed.append((hb.slab, hb.offset + keep, old - keep, []))
                self.cut_bytes += old - keep
        return HostBlob(hb.slab, hb.offset, nbytes)

    def reserve(self, nbytes: int, slab_bytes: int = 0) -> None:
        """Allocate slabs for `nbytes` more bytes now (hipHostMalloc of hundreds of MB takes tens of ms and stalls
        the device: a backend sized for its working set pays that at start-up, not inside a store).  A bounded arena
        takes its slabs as it needs them."""
        slab = max(self.slab_bytes, slab_bytes)
        with self._lock:
            if self._fl is not None:
                return
            have = sum(b.nbytes for b in self._spare)
            while have < nbytes:
                self._spare.append(self._new_slab(slab))
                have += slab

    def reset(self):
        """Recycle the newest slab (callers that own every blob handed out so far)."""
        with self._lock:
            for s in self._slabs[:-1]:
                s.free()
            self._slabs = self._slabs[-1:]
            self._tops, self._used, self._live = [], 0, 0
            self._freed, self.cut_bytes = [], 0
            if self._fl is not None:
                self._fl = self._to_free_list(self._fl.budget)

    def close(self):
        with self._lock:
            self._slabs, self._spare, self.cut_bytes = self._slabs + self._spare, [], 0
        super().close()


class DeviceArena(SlabArena):
    """The arena over HBM slabs, for encoded chunks that stay on the GPU (LMCLocalBackend, local_device="cuda" +
    local_serde="cachegen": 4.2x more warm context in the 288 GB than raw chunks).  A region is a uint8 view of its
    slab; free() takes the events of the decodes and copies that may still read it."""

    name = "HBM arena"
    release_newest_first = True

    def __init__(self, device, slab_bytes: int = 512 << 20, budget: Optional[int] = None):
        self.device = device
        super().__init__(slab_bytes, budget)

    def _new_slab(self, size: int) -> torch.Tensor:
        return torch.empty(size, dtype=torch.uint8, device=self.device)

    def _handle(self, slab: torch.Tensor, off: int, nbytes: int) -> torch.Tensor:
        return slab[off:off + nbytes]

    def _locate(self, t: torch.Tensor) -> tuple:
        p = t.data_ptr()
        for slab in self._slabs:
            base = slab.data_ptr()
            if base <= p < base + slab.nbytes:
                return slab, p - base, t.numel()
        raise ValueError("DeviceArena.free: not a region of this arena")

    def _default_streams(self) -> Sequence:
        return (torch.cuda.current_stream(self.device),)

    def alloc(self, nbytes: int, stream=None) -> torch.Tensor:
        """stream: who writes the region (bounded arena: it waits for the events of the previous owner; None: the
        current stream).  Bounded and full: ArenaFull."""
        return self._alloc(nbytes, streams=() if stream is None else (stream,))
