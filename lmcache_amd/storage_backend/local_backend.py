"""LMCLocalBackend -- the local (HBM / host-DRAM) leg of the hot path.

Mirror of the reference's LMCLocalBackend (lmcache/storage_backend/
local_backend.py:22-153): a dict keyed by CacheEngineKey, `put` (blocking or
queued to a worker thread, :72-80, :102-125), `get` returning a tensor on the
GPU (:128-144), `contains`, `close`.

Three storage modes, chosen by the config:
  local_device="cuda"                      chunks stay in HBM (reference :95-100 with device "cuda")
  local_device="cpu"                       raw chunks in PINNED host DRAM: hipMemcpyAsync on a side
                                           stream + events (the reference's pin-memory path is stubbed
                                           off and device-synchronises, :50, :82-90)
  local_device="cpu", local_serde="cachegen"
                                           CacheGen-ENCODED chunks in pinned host DRAM -- the
                                           BASELINE.json north-star path: fused HIP encode, blobs DMA'd
                                           to host on the side stream, ~3x less PCIe and DRAM
  local_device="cuda", local_serde="cachegen"
                                           CacheGen-ENCODED chunks kept in HBM: 4.2x more warm context in the
                                           288 GB than raw chunks, and the one tier whose retrieve (a decode,
                                           no PCIe) can hide behind the model layer by layer
                                           (get_kv_range(..., layers_per_launch=...))
  local_device="cuda", local_serde="cachegen-fixed"
                                           the same tier (mode "hbm-cachegen", model "fixed") with FIXED-WIDTH blobs
                                           (LMC_MODEL_FIXED: 3.8x instead of 4.6x, no entropy coder on either leg).
                                           No layer-wise store.  With both budgets its LRU groups are dropped, as
                                           they always were -- or, with LMCACHE_AMD_FIXED_DEMOTE=1, demoted like the
                                           coded tier's, as entropy-coded packs (below), and with
                                           LMCACHE_AMD_FIXED_PROMOTE=1 as well a demoted group that is hit is
                                           promoted back.  ValueError with any other device.

Bounded tiers.  LMCACHE_AMD_HBM_BYTES / LMCACHE_AMD_PINNED_BYTES (integers, optional K / M / G suffix; read at
construction, unset = unbounded) or set_capacity() give the HBM and the pinned tier a byte budget.  The unit of
eviction is the GROUP -- the chunks of one put / put_kv_range call: what a pack holds, consecutive links of one hash
chain -- in LRU order (a hit touches the groups it read from the last to the first: chains are eaten from the tail).
Over budget, the LRU groups are dropped; an "hbm-cachegen" backend with BOTH budgets is tiered instead: its LRU group
is demoted -- two or more chunks repacked on the GPU into one pinned pack (lmc_pack_blobs, then DMA), a single chunk
copied as it is -- and a group that is hit in the pinned tier is served where it lies and afterwards promoted on the
worker thread (lmc_unpack_blobs), demoting colder groups to make room.
The fixed-width tier ("cachegen-fixed") is tiered only where LMCACHE_AMD_FIXED_DEMOTE=1 was set when the backend was
built (backend.fixed_demotes; the default keeps what the tier did before it could demote: with both budgets its LRU groups
are dropped).  It demotes by TRANSCODING: its blobs hold the symbols and scales the entropy-coded
blobs of the same KV hold, so lmc_transcode_fixed turns a group -- one chunk or many -- into those blobs in the codec's
transient HBM staging (outside both budgets), and from there the leg is the coded tier's: lmc_pack_blobs, DMA, the check
of the landed pack.  Each tier keeps the format it wants: fixed width where the bytes stay in HBM, entropy-coded where
they cross PCIe.  The pack's size is known only after the transcode: room in the pinned tier is made for the pack's
BOUND and the group is filed at the size that landed.  A demoted group is served where it lies, by the rANS decoder
(every retrieve goes by what an entry IS, never by the backend's model: a prefix half in HBM and half demoted is a
fixed-width run and a pack run).  PROMOTION of such a group is the reverse transcode and has a switch of its own,
LMCACHE_AMD_FIXED_PROMOTE=1 (read at construction, backend.fixed_promotes; it takes effect only where fixed_demotes
holds).  Without it a hit does not queue a promotion (logged once) and the group stays in the pinned tier until it is
evicted.  With it a hit queues one as the coded tier does: on the worker thread the pack -- of one chunk or many -- is
unpacked into the codec's transient HBM staging (lmc_unpack_blobs), room is made in the HBM tier for the group's
fixed-width size (native.fixed_blob_bytes per chunk: a function of geometry, bins and chunk lengths, known beforehand),
and lmc_transcode_to_fixed -- the rANS decoder with a fixed-width sink, one launch, no KV and no symbol workspace --
writes the blobs lmc_encode_chunks_fixed would have written into the arena's regions.  What holds:
  1. A key is in exactly one tier, and `contains` never reads False during a demotion or promotion: the new entry is
     published before the old memory is released.  Every change of `dict` bumps `_gen`, so neither the kept prefix
     answer nor the codec's table of a kept entry list can be served stale.
  2. A retrieve that took its entries before an eviction completes bit-exact: a released region carries the events of
     the jobs that read it, and its next owner's stream waits for them.
  3. After a blocking put has returned, and after drain() behind a non-blocking one, each tier's live bytes are within
     its budget.
  4. A group larger than a tier's whole budget is not kept there: tiered, it goes straight to the pinned tier; if it
     fits nowhere it is not cached (logged once) and nothing else is evicted for it.
  5. A demotion or promotion that fails (its status word, the check of the landed pack, an exception) leaves the group
     where it was or drops it; bytes that were not checked are never published.
tier_of(), tier_stats() and drain() show what happened.
One lock (`_tier_lock`) covers every change of a tier and every launch that reads one.  Without a budget a store holds it
only to file its group.  WITH budgets it is held across the host waits of a bounded store, a demotion and a promotion (the
DMA of a whole pack: about 10 ms for a 16 k context), so a retrieve that arrives while the worker thread moves a group waits
that long before its first launch; "promotion adds no work in front of the hit" holds for the hit that queued it, not for
one that arrives during the move.  Narrowing the lock to the publish-and-release step is left for later.

All three implement the optional put_kv_range / get_kv_range protocol
(abstract_backend.py) so the engine never materialises the [L,2,T,H,D] blob
(cache_engine.py:98-161) nor the final torch.cat (:362-368): KV is gathered
from / scattered to the caller's tensors by the HIP kernels.
"""
import ctypes
import os
import queue
import time
import threading
from dataclasses import dataclass, field
from typing import Dict, Iterable, List, Optional, Sequence, Tuple, Union

import torch

from lmcache_amd import native
from lmcache_amd.config import LMCacheEngineConfig, LMCacheEngineMetadata, check_local_serde
from lmcache_amd.logging import init_logger
from lmcache_amd.storage_backend.abstract_backend import LMCBackendInterface
from lmcache_amd.storage_backend.serde.cachegen_basics import CacheGenConfig
from lmcache_amd.storage_backend.serde.cachegen_decoder import output_spec, retrieve_spec
from lmcache_amd.storage_backend.serde.cachegen_device import (ArenaFull, DeviceArena, HostBlob, HostPack, PinnedArena,
                                                               get_codec)
from lmcache_amd.storage_backend.tiering import GroupLRU, Tiers, parse_bytes, r16
from lmcache_amd.utils import CacheEngineKey, _lmcache_nvtx_annotate

logger = init_logger(__name__)


class LocalBackendEndSignal:
    pass


@dataclass
class _DevChunk:
    blob: torch.Tensor                 # uint8 view of the backend's HBM arena: one encoded chunk
    shape: Tuple[int, ...]
    dtype: torch.dtype
    model: Optional[str] = None        # the blob's coder model as the codec names it: None (entropy-coded) or "fixed"


@dataclass
class _HostChunk:
    blob: HostBlob
    ready: Optional[torch.cuda.Event]  # D2H finished
    shape: Tuple[int, ...]             # chunk tensor shape in the engine's fmt
    dtype: torch.dtype
    encoded: bool


@dataclass
class _PackChunk:
    """Chunk `index` of a pack: the blobs of one put_kv_range() call, stored plane-major (pack v3) in pinned host DRAM."""
    pack: HostPack
    index: int
    shape: Tuple[int, ...]
    dtype: torch.dtype
    blob: Optional[HostBlob] = None    # the chunk as a blob of its own, reassembled on first single-chunk use
    encoded: bool = True
    ready: Optional[torch.cuda.Event] = None


@dataclass
class _Group:
    """The chunks of one put call: the unit of the LRU, of eviction, demotion and promotion."""
    gid: int
    keys: List[CacheEngineKey]
    nbytes: int                        # what it counts for in its tier
    geometry: Optional[Tuple[int, int, int]]  # (L, H, D) of an encoded group
    chunk_tokens: int
    ntokens: int
    readers: list                      # events of the jobs that wrote or read its memory: a release is fenced by them
    orphans: list = field(default_factory=list)  # pack chunks whose key a later store took: the pack goes back with the group

    def live_readers(self) -> list:
        out = []
        for ev in self.readers:
            try:
                if ev.query():
                    continue
            except Exception:
                pass
            out.append(ev)
        return out


def _chunk_shape(fmt: str, L: int, T: int, H: int, D: int) -> Tuple[int, ...]:
    if fmt == "vllm":
        return (L, 2, T, H, D)
    if fmt == "huggingface":
        return (L, 2, H, T, D)
    raise ValueError(f"Invalid format: {fmt}")


def _token_axis(fmt: str) -> int:
    """The token dimension of a chunk shape (_chunk_shape)."""
    return 2 if fmt == "vllm" else 3


def _coded_dtype(fmt: str, kv_dtype: torch.dtype) -> torch.dtype:
    """The dtype a cachegen-tier chunk is retrieved as: the reference's rule for 16-bit KV (output_spec: bf16 for vllm,
    fp16 for huggingface), the stored dtype for fp8 KV."""
    if kv_dtype in (torch.float8_e4m3fn, torch.float8_e5m2):
        return kv_dtype
    return output_spec(fmt, 1, 1, 1, 8)[1]


def _fmt_of_chunk(t: torch.Tensor, fmt_hint: Optional[str]) -> str:
    return fmt_hint or "vllm"


class LayerwisePut:
    """One begin_put_kv_layers() in flight."""

    def __init__(self, backend: "LMCLocalBackend", keys, job, shapes, dtype):
        self.backend, self.keys, self.job, self.shapes, self.dtype = backend, keys, job, shapes, dtype

    def encode_layer(self, layer: int) -> None:
        self.job.encode_layer(layer)

    def layer_event(self, layer: int):
        """Behind it layer `layer`'s KV has been read (torch.cuda.Event)."""
        return self.job.layer_events[layer]

    def finish(self, blocking: bool = True) -> int:
        """The last launch behind the last layer, then the tier's copies and the publishing: here, or -- blocking=False --
        on the backend's worker thread (drain() waits for it).  -> chunks stored."""
        b, job = self.backend, self.job
        with torch.cuda.device(job.arena.device):
            job.finish()
        if blocking:
            b._finish_layers(self.keys, job, self.shapes, self.dtype)
        else:
            b.put_queue.put(lambda: b._finish_layers(self.keys, job, self.shapes, self.dtype))
        return len(self.keys)

    def abort(self) -> None:
        self.job.abort()
        self.backend._codec().release_layer_stream(self.job)


class LMCLocalBackend(LMCBackendInterface):
    supports_kv_layout = True

    def __init__(self, config: LMCacheEngineConfig, metadata: Optional[LMCacheEngineMetadata] = None):
        super().__init__()
        native.lib()  # no CPU fallback: fail at construction if the HIP library is missing
        self.chunk_size = config.chunk_size
        self.config = config
        self.metadata = metadata
        self.fmt = metadata.fmt if metadata is not None else None
        self.device = config.local_device
        self.dst_device = "cuda"
        # the coder model of an encoded tier: "rans" (the entropy-coded blobs) or "fixed" (local_serde="cachegen-fixed":
        # LMC_MODEL_FIXED, fixed-width symbols -- HBM-resident only); None on the raw tiers
        self.model: Optional[str] = None
        if config.local_serde not in (None, "cachegen", "cachegen-fixed"):
            raise ValueError(f"Invalid local_serde: {config.local_serde}")
        if self.device == "cuda":
            self.mode = "hbm-cachegen" if config.local_serde in ("cachegen", "cachegen-fixed") else "hbm"
        elif self.device == "cpu":
            check_local_serde(self.device, config.local_serde)  # "cachegen-fixed": ValueError, the pinned tier is PCIe-bound
            self.mode = "cachegen" if config.local_serde == "cachegen" else "raw"
        else:
            raise ValueError(f"LMCLocalBackend: unsupported local_device {self.device!r}")
        if self.mode in ("cachegen", "hbm-cachegen"):
            self.model = "fixed" if config.local_serde == "cachegen-fixed" else "rans"
        # get_kv_range(heads=...): a window of heads out of chunks stored under another tensor-parallel degree -- the
        # decoders' business, so the two CacheGen tiers only (the raw tiers copy whole chunks)
        self.supports_head_window = self.mode in ("cachegen", "hbm-cachegen")
        self.cachegen_config = None
        if self.mode in ("cachegen", "hbm-cachegen"):
            if metadata is None:
                raise ValueError("local_serde='cachegen' needs the engine metadata (model name, fmt)")
            self.cachegen_config = CacheGenConfig.from_model_name(metadata.model_name)
        self.dict: Dict[CacheEngineKey, Union[torch.Tensor, _HostChunk]] = {}
        self.update_lock = threading.Lock()
        self.host_arena = PinnedArena() if self.mode in ("raw", "cachegen") else None
        # pinned CacheGen tier: a put_kv_range() of several chunks is stored as ONE plane-major pack (lmc_store_pack_parts), so
        # that a retrieve of the same prefix moves a range of layers as one transfer (LMCACHE_AMD_PINNED_PACKS=0: one
        # blob per chunk, as the reference stores them)
        self.pack_stores = self.mode == "cachegen" and os.environ.get("LMCACHE_AMD_PINNED_PACKS", "1") != "0"
        self.dev_arena: Optional[DeviceArena] = None   # hbm-cachegen: created on first use, on the KV's device
        self._stage: Optional[torch.Tensor] = None   # device staging for raw gathers / scatters
        self._stage_free: Optional[torch.cuda.Event] = None
        self._cuda_device = torch.cuda.current_device()
        self.last_publish_time = 0.0
        self._gen = 0               # bumped by every change of `dict`: what _prefix_entries' kept answer is valid for
        self._prefix_memo = None
        # bounded tiers (module docstring): groups in LRU order, budgets, and one lock around every change of a tier and
        # every launch that reads one
        self._tier_lock = threading.RLock()
        self._lru = GroupLRU()
        self._groups: Dict[int, "_Group"] = {}
        self._key_gid: Dict[CacheEngineKey, int] = {}
        self._next_gid = 0
        self._promoting: set = set()
        self._oversize_logged = False
        self._promotion_off_logged = False
        # both coder models can demote, the fixed-width one by transcoding its blobs (_demote_group) -- but only where it is
        # asked to: a fixed-width backend with both budgets has always DROPPED its LRU groups, and keeps doing so unless
        # LMCACHE_AMD_FIXED_DEMOTE=1 says otherwise (read here, once)
        self.fixed_demotes = self.model == "fixed" and os.environ.get("LMCACHE_AMD_FIXED_DEMOTE", "0") == "1"
        # ... and a demoted fixed-width group is promoted back -- the pack's coded blobs transcoded into fixed-width ones
        # (_promote_group) -- only where LMCACHE_AMD_FIXED_PROMOTE=1 is set as well: without it a hit serves such a group
        # where it lies and leaves it there, as before the reverse transcode existed
        self.fixed_promotes = self.fixed_demotes and os.environ.get("LMCACHE_AMD_FIXED_PROMOTE", "0") == "1"
        # the fixed-width tier stores layer by layer (begin_put_kv_layers: lmc_encode_layers_begin_fixed) only where
        # LMCACHE_AMD_FIXED_LAYERWISE=1 is set (read here, once): the default keeps what the tier has always done with a
        # layer-wise store -- one encode of the whole context behind the last layer
        self.fixed_layerwise = self.model == "fixed" and os.environ.get("LMCACHE_AMD_FIXED_LAYERWISE", "0") == "1"
        self._tiers = Tiers(self._lru, self._demote_group if self._demotes() else None, self._drop_group, self._demoted_size)
        self.put_queue: "queue.Queue" = queue.Queue()
        self.put_thread = threading.Thread(target=self.put_worker, daemon=True)
        self.put_thread.start()
        self.set_capacity(parse_bytes(os.environ.get("LMCACHE_AMD_HBM_BYTES")),
                          parse_bytes(os.environ.get("LMCACHE_AMD_PINNED_BYTES")), _keep_unset=True)

    # ------------------------------------------------------------------ basics
    def contains(self, key: CacheEngineKey) -> bool:
        return key in self.dict

    def _prefix_entries(self, keys: Sequence[CacheEngineKey]) -> list:
        """The entries of the leading keys that are present (stop at the first miss).  The last answer is kept for the SAME
        key list object while nothing has been published since (the engine keeps the key lists of its last hash chains:
        the lookup -> retrieve of a warm prefix probes the same 64 keys twice, every call of a serving engine)."""
        # the generation is read BEFORE the scan: a publish that lands while the dict is being scanned leaves the answer
        # filed under the older generation, so the next call scans again instead of repeating a short answer
        gen = self._gen
        m = self._prefix_memo
        if m is not None and m[0] is keys and m[1] == gen:
            return m[2]
        d, entries = self.dict, []
        for k in keys:
            e = d.get(k)
            if e is None:
                break
            entries.append(e)
        self._prefix_memo = (keys, gen, entries)
        return entries

    def contains_prefix(self, keys: Sequence[CacheEngineKey]) -> int:
        """How many leading keys are present: the engine's prefix probe (cache_engine.py:323-345: stop at the first
        miss) as one call."""
        return len(self._prefix_entries(keys))

    def _publish(self, key: CacheEngineKey, entry) -> None:
        with self.update_lock:
            self.dict[key] = entry
            self._gen += 1
            self.last_publish_time = time.perf_counter()  # (when a non-blocking store became visible: bench.py store_hidden)

    def _unpublish(self, key: CacheEngineKey) -> None:
        with self.update_lock:
            if self.dict.pop(key, None) is not None:
                self._gen += 1

    # ------------------------------------------------------------------ bounded tiers
    def _tier_name(self) -> str:
        """The tier a store of this backend's mode lands in."""
        return "hbm" if self.mode in ("hbm", "hbm-cachegen") else "pinned"

    def set_capacity(self, hbm_bytes: Optional[int] = None, pinned_bytes: Optional[int] = None, _keep_unset: bool = False) -> None:
        """Byte budgets of the HBM and the pinned tier (None: unbounded).  A budget that shrinks evicts -- or, tiered,
        demotes -- at once."""
        with self._tier_lock:
            self._tiers.budget["hbm"], self._tiers.budget["pinned"] = hbm_bytes, pinned_bytes
            if _keep_unset and hbm_bytes is None and pinned_bytes is None:
                return
            if self._demotes() and pinned_bytes is not None and self.host_arena is None:
                self.host_arena = PinnedArena()
            if self.host_arena is not None:
                self.host_arena.set_budget(pinned_bytes)
            if self.dev_arena is not None:
                self.dev_arena.set_budget(hbm_bytes)
            self._tiers.enforce()

    def _demotes(self) -> bool:
        """Whether this backend's HBM tier has a pinned tier under it: the coded HBM tier, and the fixed-width one where
        fixed_demotes is set."""
        return self.mode == "hbm-cachegen" and (self.model != "fixed" or self.fixed_demotes)

    def tier_of(self, key: CacheEngineKey) -> Optional[str]:
        e = self.dict.get(key)
        if e is None:
            return None
        return "hbm" if isinstance(e, (_DevChunk, torch.Tensor)) else "pinned"

    def tier_stats(self) -> dict:
        with self._tier_lock:
            out = {"demotions": self._tiers.demotions, "promotions": self._tiers.promotions, "evictions": self._tiers.evictions}
            for tier, arena in (("hbm", self.dev_arena), ("pinned", self.host_arena)):
                live = self._lru.live(tier)
                out[tier] = {"live_bytes": live, "reserved_bytes": arena.reserved_bytes if arena is not None else live,
                             "groups": self._lru.count(tier), "budget": self._tiers.budget[tier]}
            return out

    def drain(self) -> None:
        """Wait until the worker thread has done everything queued so far (non-blocking puts, promotions)."""
        while True:
            done = threading.Event()
            self.put_queue.put(done.set)
            done.wait()
            with self._tier_lock:
                if not self._promoting and self.put_queue.empty():
                    return

    def _new_group(self, tier: str, keys: Sequence[CacheEngineKey], entries: Sequence, nbytes: int, geometry=None,
                   chunk_tokens: int = 0, ntokens: int = 0, ready=None) -> None:
        """File the chunks of one put call as a group and publish them (caller holds _tier_lock)."""
        gid, self._next_gid = self._next_gid, self._next_gid + 1
        self._groups[gid] = _Group(gid, list(keys), nbytes, geometry, chunk_tokens, ntokens, [ready] if ready is not None else [])
        self._lru.add(tier, gid, nbytes)
        for key, e in zip(keys, entries):
            old_gid, old_e = self._key_gid.get(key), self.dict.get(key)
            self._key_gid[key] = gid
            self._publish(key, e)
            if old_gid is not None and old_e is not None:
                self._release_replaced(old_gid, old_e)

    def _release_replaced(self, old_gid: int, old_e) -> None:
        """A key was stored again: the entry it had leaves its older group.  A chunk with memory of its own gives it back
        now (fenced by that group's readers) and the group counts for less; a chunk of a pack waits for its pack, which
        goes back with the group; a group that has lost its last key goes altogether."""
        g = self._groups.get(old_gid)
        if g is None:
            return
        if isinstance(old_e, _PackChunk):
            g.orphans.append(old_e)
        else:
            self._release([old_e], g.live_readers())
            if isinstance(old_e, _DevChunk):
                nb = r16(old_e.blob.numel())
            elif isinstance(old_e, _HostChunk):
                nb = r16(old_e.blob.nbytes)
            else:
                nb = old_e.numel() * old_e.element_size()
            g.nbytes = max(0, g.nbytes - nb)
            if self._lru.tier_of(old_gid) is not None:
                self._lru.resize(old_gid, g.nbytes)
        if not self._own_keys(g):
            self._drop_group(old_gid)
            self._lru.remove(old_gid)

    def _demoted_size(self, gid: int) -> int:
        """Bytes group `gid` of the HBM tier takes in the pinned tier: its pack's exact size, or its one blob's.  A
        fixed-width group's pack is known only once it has been transcoded: its BOUND (_demote_group files the group at
        the size that landed)."""
        g = self._groups[gid]
        devs = [self.dict[k] for k in self._own_keys(g) if isinstance(self.dict.get(k), _DevChunk)]
        if devs and g.geometry is not None and any(e.model == "fixed" for e in devs):
            return r16(native.pack_bound(len(devs), g.geometry[0], g.chunk_tokens, g.geometry[1], g.geometry[2]))
        sizes = [e.blob.numel() for e in devs]
        if len(sizes) >= 2 and len(sizes) == len(g.keys) and g.geometry is not None:
            return r16(self._codec().demoted_bytes(sizes, g.geometry, g.chunk_tokens, g.ntokens))
        return sum(r16(n) for n in sizes) or g.nbytes

    def _own_keys(self, g: "_Group") -> list:
        return [k for k in g.keys if self._key_gid.get(k) == g.gid]

    def _release(self, entries: Sequence, events: Sequence) -> None:
        """Give the memory of a group's entries back to its arena, fenced by `events` (who may still read it)."""
        packs = []
        for e in entries:
            if isinstance(e, _DevChunk):
                if self.dev_arena is not None:
                    self.dev_arena.free(e.blob, events)
            elif isinstance(e, _PackChunk):
                if not any(e.pack is p for p in packs):
                    packs.append(e.pack)
                if e.blob is not None and self.host_arena is not None:
                    self.host_arena.free(e.blob, events)
            elif isinstance(e, _HostChunk) and self.host_arena is not None:
                self.host_arena.free(e.blob, events)
        for p in packs:
            if self.host_arena is not None:
                self.host_arena.free(p.blob, events)

    def _drop_group(self, gid: int) -> None:
        """Forget a group: its keys leave the dict, then its memory goes back (Tiers removes it from the LRU)."""
        g = self._groups.pop(gid)
        entries = []
        for k in self._own_keys(g):
            e = self.dict.get(k)
            if e is not None:
                entries.append(e)
            self._unpublish(k)
            del self._key_gid[k]
        self._release(entries + g.orphans, g.live_readers())

    def _demote_group(self, gid: int) -> bool:
        """HBM blobs of a group -> the pinned tier (Tiers has made room there): republished first, released after.
        False: nothing changed, the caller drops the group."""
        g = self._groups[gid]
        keys = self._own_keys(g)
        old = [self.dict[k] for k in keys]
        if len(keys) != len(g.keys) or not all(isinstance(e, _DevChunk) for e in old):
            return False  # (a group that lost a key to a later store is no whole chain link any more)
        codec = self._codec()
        fixed = any(e.model == "fixed" for e in old)
        if fixed and (g.geometry is None or not all(e.model == "fixed" for e in old)):
            return False

        def move():
            if fixed:
                # fixed-width blobs cross PCIe entropy-coded: transcoded, then the same pack leg -- a single chunk too (its
                # blob as it is would be a fixed-width blob in the tier the rANS decoder serves)
                pack = codec.demote_blobs([e.blob for e in old], g.geometry, g.chunk_tokens, g.ntokens, self.host_arena,
                                          ready=g.readers[:1], model="fixed", bins=self.cachegen_config.plane_bins(g.geometry[0]))
                return [_PackChunk(pack, i, e.shape, e.dtype) for i, e in enumerate(old)], r16(pack.blob.nbytes)
            if len(old) >= 2:
                pack = codec.demote_blobs([e.blob for e in old], g.geometry, g.chunk_tokens, g.ntokens, self.host_arena,
                                          ready=g.readers[:1])
                return [_PackChunk(pack, i, e.shape, e.dtype) for i, e in enumerate(old)], r16(pack.blob.nbytes)
            e = old[0]
            hb = self.host_arena.alloc(e.blob.numel(), streams=[codec.copy_stream])
            for ev in g.readers[:1]:
                codec.copy_stream.wait_event(ev)
            native.memcpy_async(hb.ptr, e.blob.data_ptr(), e.blob.numel(), "d2h", codec.copy_stream.cuda_stream)
            codec.copy_stream.synchronize()
            return [_HostChunk(hb, None, e.shape, e.dtype, True)], r16(hb.nbytes)

        new = None
        try:
            with torch.cuda.device(self._cuda_device):
                while new is None:
                    try:
                        new, nbytes = move()
                    except ArenaFull:
                        # the byte count allowed it, the holes did not: the pinned tier's LRU group goes, and again
                        if not self._tiers.take_lru("pinned", keep=[gid]):
                            raise
        except Exception as exc:
            logger.warning("demotion failed (%s: %s): the group is dropped", type(exc).__name__, exc)
            return False
        for k, e in zip(keys, new):
            self._publish(k, e)
        self._release(old, g.live_readers())
        g.readers, g.nbytes = [], nbytes
        self._lru.add("pinned", gid, nbytes)
        return True

    def _promote_group(self, gid: int) -> None:
        """Worker thread: a pinned group that was hit goes back to HBM, colder groups making room."""
        with self._tier_lock:
            self._promoting.discard(gid)
            g = self._groups.get(gid)
            if g is None or self._lru.tier_of(gid) != "pinned" or not self._tiers.tiered():
                return
            keys = self._own_keys(g)
            old = [self.dict[k] for k in keys]
            # a fixed-width backend's pinned groups are packs of entropy-coded blobs whatever their length (_demote_group
            # makes a pack of a single chunk too) and go back as fixed-width blobs: the reverse transcode
            fixed = self.model == "fixed"
            if fixed and (not self.fixed_promotes or g.geometry is None):
                return
            packed = len(old) >= (1 if fixed else 2) and all(isinstance(e, _PackChunk) and e.pack is old[0].pack and e.index == i
                                                             for i, e in enumerate(old)) and old[0].pack.nchunks == len(old)
            single = not fixed and len(old) == 1 and isinstance(old[0], _HostChunk) and old[0].encoded
            if len(keys) != len(g.keys) or not (packed or single):
                return
            codec = self._codec()
            bins = self.cachegen_config.plane_bins(g.geometry[0]) if fixed else None
            try:
                if fixed:
                    pack = old[0].pack
                    L, H, D = g.geometry
                    lens = [g.chunk_tokens] * (len(old) - 1) + [g.ntokens - (len(old) - 1) * g.chunk_tokens]
                    sizes = [native.fixed_blob_bytes(L, T, H, D, bins) for T in lens]
                elif packed:
                    pack = old[0].pack
                    sizes = [native.pack_chunk_bytes(pack.blob.ptr, pack.blob.nbytes, i) for i in range(len(old))]
                else:
                    sizes = [old[0].blob.nbytes]
                nbytes = sum(r16(n) for n in sizes)
                if nbytes > self._tiers.budget["hbm"] or not self._tiers.make_room("hbm", nbytes, keep=[gid]):
                    return
                if self._lru.tier_of(gid) != "pinned":
                    return
                if self.dev_arena is None:
                    self.dev_arena = DeviceArena(torch.device("cuda", self._cuda_device), budget=self._tiers.budget["hbm"])

                def move():
                    if fixed:
                        return codec.promote_pack(pack, self.dev_arena, model="fixed", bins=bins)
                    if packed:
                        return codec.promote_pack(pack, self.dev_arena)
                    cur = torch.cuda.current_stream()
                    t = self.dev_arena.alloc(sizes[0], stream=cur)
                    native.memcpy_async(t.data_ptr(), old[0].blob.ptr, sizes[0], "h2d", cur.cuda_stream)
                    cur.synchronize()
                    return [t]

                blobs = None
                with torch.cuda.device(self._cuda_device):
                    while blobs is None:
                        try:
                            blobs = move()
                        except ArenaFull:
                            # the byte count allowed it, the holes did not: the HBM tier's LRU group goes down, and again
                            # (its demotion may have pushed THIS group out of a fragmented pinned tier: then nothing is left
                            # to promote)
                            if not self._tiers.take_lru("hbm", keep=[gid]) or self._lru.tier_of(gid) != "pinned":
                                return
            except Exception:
                logger.exception("promotion failed: the group stays in the pinned tier")
                return
            for k, e, t in zip(keys, old, blobs):
                self._publish(k, _DevChunk(t, e.shape, e.dtype, model="fixed" if fixed else None))
            self._release(old, g.live_readers())
            g.readers, g.nbytes = [], nbytes
            self._lru.add("hbm", gid, nbytes)
            self._tiers.promotions += 1
            self._tiers.enforce(keep=[gid])

    def _touch(self, keys: Sequence[CacheEngineKey], events: Sequence = ()) -> None:
        """A hit read these keys (caller holds _tier_lock): their groups move up the LRU, remember `events` (the jobs
        that read them: a later release is fenced by those), and -- tiered -- pinned ones are queued for promotion."""
        gids = []
        for k in keys:
            gid = self._key_gid.get(k)
            if gid is not None and (not gids or gids[-1] != gid):
                gids.append(gid)
        self._lru.touch_chain(gids)
        for gid in set(gids):
            g = self._groups.get(gid)
            if g is None:
                continue
            if events:
                g.readers = g.live_readers() + list(events)
            if self._lru.tier_of(gid) == "pinned" and self._tiers.tiered() and gid not in self._promoting:
                if self.model == "fixed" and not self.fixed_promotes:
                    # promotion turns the pack's coded blobs back into fixed-width ones (the reverse transcode); without
                    # LMCACHE_AMD_FIXED_PROMOTE=1 the group is served where it lies and stays there
                    if not self._promotion_off_logged:
                        self._promotion_off_logged = True
                        logger.info("fixed-width tier: a demoted group that is hit stays in the pinned tier (no promotion; logged once)")
                    continue
                self._promoting.add(gid)
                self.put_queue.put(lambda gid=gid: self._promote_group(gid))

    def _not_cached(self, nbytes: int) -> None:
        if not self._oversize_logged:
            self._oversize_logged = True
            logger.warning("a group of %d bytes fits no tier's budget: not cached (logged once)", nbytes)

    def _store(self, tier: str, need: int, make, keys: Sequence[CacheEngineKey], **group) -> bool:
        """File a new group in `tier`.  make() -> (entries, bytes, ready event or None) allocates and fills its memory.
        Unbounded tier: make() runs outside the tier lock (a store in flight never holds up a retrieve).  Bounded: room for
        `need` bytes is made first; an arena that is still full (fragmented) has its LRU group taken out and make() runs
        again.  -> False: the group fits nowhere and was not cached."""
        b = self._tiers.budget[tier]
        if b is None:
            got = make()
            with self._tier_lock:
                if self._tiers.budget[tier] is not None and tier == "hbm" and self.dev_arena is not None:
                    self.dev_arena.set_budget(self._tiers.budget[tier])  # (bounded in the meantime)
                self._new_group(tier, keys, got[0], got[1], ready=got[2], **group)
                self._tiers.enforce()
            return True
        with self._tier_lock:
            got = None
            if need <= b and self._tiers.make_room(tier, need):
                while got is None:
                    try:
                        got = make()
                    except ArenaFull:
                        if not self._tiers.take_lru(tier):
                            break
            if got is None:
                self._not_cached(need)
                return False
            self._new_group(tier, keys, got[0], got[1], ready=got[2], **group)
            self._tiers.enforce()
            return True

    @_lmcache_nvtx_annotate
    def put_worker(self):
        torch.cuda.set_device(self._cuda_device)
        while True:
            item = self.put_queue.get()
            if isinstance(item, LocalBackendEndSignal):
                break
            try:
                item()
            except Exception:  # keep the worker alive; the chunk simply is not cached
                logger.exception("asynchronous put failed")

    def close(self):
        if self.put_thread is not None and self.put_thread.is_alive():
            self.put_queue.put(LocalBackendEndSignal())
            self.put_thread.join()
        if self.host_arena is not None:
            # entries may still be read by a caller holding tensors made from them: drop our refs first
            self.dict.clear()
            self.host_arena.close()
            self.host_arena = None
        if self.dev_arena is not None:
            self.dict.clear()
            self.dev_arena.close()
            self.dev_arena = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------ single chunk
    def _codec(self):
        return get_codec(self._cuda_device)

    def _coder(self) -> dict:
        """The codec's `model` argument for this tier's encode / decode_device calls."""
        return {"model": "fixed"} if self.model == "fixed" else {}

    @staticmethod
    def _run_model(entries: Sequence) -> Optional[str]:
        """The coder model of a run of HBM entries, read off the entries (one decode job is one model)."""
        models = {e.model for e in entries}
        if len(models) != 1:
            raise ValueError("one decode job over HBM blobs of two coder models")
        return models.pop()

    def _group_of(self, geometry: tuple, chunk_tokens: int, shapes) -> dict:
        """What _store keeps about a CacheGen group beside its entries (the repack legs of demotion and promotion need it)."""
        tok = _token_axis(self.fmt or "vllm")
        return dict(geometry=tuple(geometry), chunk_tokens=chunk_tokens, ntokens=sum(shp[tok] for shp in shapes))

    def _finish_encoded(self, keys: Sequence[CacheEngineKey], job, shapes, dtype) -> None:
        codec = self._codec()
        group = self._group_of(job.geometry[:3], job.geometry[3], shapes)
        if self.mode == "hbm-cachegen":
            def keep():
                if self.dev_arena is None:
                    self.dev_arena = DeviceArena(torch.device("cuda", self._cuda_device), budget=self._tiers.budget["hbm"])
                blobs = codec.keep_on_device(job, self.dev_arena)
                ready = torch.cuda.Event()
                ready.record(torch.cuda.current_stream(self._cuda_device))
                return ([_DevChunk(t, shp, dtype, self._coder().get("model")) for t, shp in zip(blobs, shapes)],
                        sum(r16(t.numel()) for t in blobs), ready)
            if self._tiers.budget["hbm"] is None:
                self._store("hbm", 0, keep, keys, **group)
                return
            sizes = codec.sizes_of(job)
            nbytes = sum(r16(n) for n in sizes)
            fixed = self.model == "fixed"
            L, H, D = group["geometry"]
            bound = r16(native.pack_bound(len(sizes), L, group["chunk_tokens"], H, D)) if fixed else None
            where = self._tiers.place(nbytes, bound)
            if where == "hbm":
                ok = self._store("hbm", nbytes, keep, keys, **group)
            elif where == "pinned" and fixed:
                # larger than the whole HBM budget: straight to the pinned tier, transcoded from the encode arena into one
                # entropy-coded pack (room is made for its bound, the group is filed at the size that landed)
                def to_pack():
                    views = [job.arena[i * job.stride:i * job.stride + nb] for i, nb in enumerate(sizes)]
                    pack = codec.demote_blobs(views, group["geometry"], group["chunk_tokens"], group["ntokens"], self.host_arena,
                                              ready=[job.done], model="fixed", bins=self.cachegen_config.plane_bins(L))
                    job.offload_issued = True
                    return [_PackChunk(pack, i, shp, dtype) for i, shp in enumerate(shapes)], r16(pack.blob.nbytes), None
                ok = self._store("pinned", bound, to_pack, keys, **group)
            elif where == "pinned":  # larger than the whole HBM budget: straight to the pinned tier, a blob per chunk
                ok = self._store("pinned", nbytes, lambda: self._offload_entries(job, sizes, shapes, dtype), keys, **group)
            else:
                self._not_cached(nbytes)
                ok = False
            if not ok:
                job.offload_issued = True  # (nothing reads the encode arena any more)
            return
        if self._tiers.budget["pinned"] is None:
            # range by range, overlapping the rest of the encode
            self._store("pinned", 0, lambda: self._offload_entries(job, None, shapes, dtype), keys, **group)
            return
        sizes = codec.sizes_of(job)
        nbytes = sum(r16(n) for n in sizes)
        if not self._store("pinned", nbytes, lambda: self._offload_entries(job, sizes, shapes, dtype), keys, **group):
            job.offload_issued = True

    def _offload_entries(self, job, sizes, shapes, dtype):
        """The job's blobs in pinned host DRAM -> (entries, bytes, None)."""
        blobs, done = self._codec().offload(job, sizes, self.host_arena)
        done.synchronize()
        return [_HostChunk(hb, None, shp, dtype, True) for hb, shp in zip(blobs, shapes)], sum(r16(hb.nbytes) for hb in blobs), None

    def _finish_pack(self, keys: Sequence[CacheEngineKey], job, shapes, dtype) -> None:
        def finish():
            pack = self._codec().finish_pack(job, self.host_arena)
            return [_PackChunk(pack, i, shp, dtype) for i, shp in enumerate(shapes)], r16(pack.blob.nbytes), None

        # bounded: the region is taken at the pack's bound and cut to size while the tier has room for the bound (the parts
        # then leave while the later planes are coded, as in an unbounded tier); a tier that would have to evict for the
        # bound waits for the last part instead and makes room for the pack's exact size
        b = self._tiers.budget["pinned"]
        need = 0
        if b is not None:
            need = r16(job.cap)
            if self._lru.live("pinned") + need > b:
                need = r16(max(self._codec().pack_bytes(job), 16))
        if not self._store("pinned", need, finish, keys, **self._group_of(job.geometry, job.chunk_tokens, shapes)):
            if not job.d2h_issued:  # never taken by finish_pack: its kernels finish, its words and the staging go back
                job.done.synchronize()
                with self._codec()._lock:
                    job.retire()
                    job.d2h_issued = True

    def _own_blob(self, e: _PackChunk) -> HostBlob:
        """A pack's chunk as a blob of its own in the pinned arena (the single-chunk paths: get(), a retrieve that mixes
        chunks of different stores)."""
        if e.blob is None:
            data = e.pack.extract(e.index)
            hb = self.host_arena.alloc(len(data))
            ctypes.memmove(hb.ptr, data, len(data))
            e.blob = hb
        return e.blob

    def _put_chunk_now(self, key: CacheEngineKey, kv_chunk: torch.Tensor, fmt: str) -> None:
        if not kv_chunk.is_cuda:
            kv_chunk = kv_chunk.to(self.dst_device)
        if self.mode == "hbm":
            self._keep_tensors([key], [kv_chunk if kv_chunk.is_contiguous() else kv_chunk.contiguous()])
            return
        lay = native.KVLayout.from_chunk(kv_chunk, fmt)
        shape = _chunk_shape(fmt, lay.L, lay.ntokens, lay.H, lay.D)
        if self.mode in ("cachegen", "hbm-cachegen"):
            out_dt = _coded_dtype(fmt, kv_chunk.dtype)
            with torch.cuda.device(kv_chunk.device):
                job = self._codec().encode(lay, 0, lay.ntokens, lay.ntokens, self.cachegen_config.plane_bins(lay.L), **self._coder())
            self._finish_encoded([key], job, [shape], out_dt)
            return
        # raw: contiguous chunk -> pinned host
        src = kv_chunk if kv_chunk.is_contiguous() else kv_chunk.contiguous()
        nbytes = src.numel() * src.element_size()
        codec = self._codec()

        def copy_out():
            hb = self.host_arena.alloc(nbytes, streams=[codec.copy_stream])
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(src.device))
            codec.copy_stream.wait_event(ev)
            native.memcpy_async(hb.ptr, src.data_ptr(), nbytes, "d2h", codec.copy_stream.cuda_stream)
            done = torch.cuda.Event()
            done.record(codec.copy_stream)
            done.synchronize()  # `src` may be freed by the caller after we return
            return [_HostChunk(hb, None, tuple(src.shape), src.dtype, False)], r16(nbytes), None

        self._store("pinned", r16(nbytes), copy_out, [key])

    def _keep_tensors(self, keys: Sequence[CacheEngineKey], chunks: Sequence[torch.Tensor]) -> None:
        """Raw chunks that stay in HBM as the tensors they are ("hbm" mode): one group."""
        nbytes = sum(c.numel() * c.element_size() for c in chunks)
        self._store("hbm", nbytes, lambda: (list(chunks), nbytes, None), keys)

    def put(self, key: CacheEngineKey, kv_chunk: torch.Tensor, blocking: bool = True) -> None:
        fmt = _fmt_of_chunk(kv_chunk, self.fmt)
        if blocking:
            self._put_chunk_now(key, kv_chunk, fmt)
        else:
            # the worker thread queues its work on ITS current stream: order it behind the stream that produced the chunk
            ready = None
            if kv_chunk.is_cuda:
                ready = torch.cuda.Event()
                ready.record(torch.cuda.current_stream(kv_chunk.device))

            def queued():
                if ready is not None:
                    torch.cuda.current_stream(kv_chunk.device).wait_event(ready)
                self._put_chunk_now(key, kv_chunk, fmt)
            self.put_queue.put(queued)

    @_lmcache_nvtx_annotate
    def get(self, key: CacheEngineKey) -> Optional[torch.Tensor]:
        # (the tier lock is held to the end: every path below has finished reading the entry when it returns, but for the
        # raw copy, whose event fences a later release)
        with self._tier_lock:
            out = self._get_locked(key)
            if out is not None:
                ev = None
                if self.mode == "raw":
                    ev = torch.cuda.Event()
                    ev.record(torch.cuda.current_stream(out.device))
                self._touch([key], [ev] if ev is not None else ())
            return out

    def _get_locked(self, key: CacheEngineKey) -> Optional[torch.Tensor]:
        entry = self.dict.get(key, None)
        if entry is None:
            return None
        if isinstance(entry, torch.Tensor):
            return entry.to(self.dst_device)
        dev = torch.device("cuda", self._cuda_device)
        out = torch.empty(entry.shape, dtype=entry.dtype, device=dev)
        fmt = self.fmt or "vllm"
        if isinstance(entry, _DevChunk):
            T = entry.shape[2] if fmt == "vllm" else entry.shape[3]
            codec = self._codec()
            try:
                codec.finish_decode(codec.decode_device([entry.blob], native.KVLayout.from_chunk(out, fmt), 0, T, model=entry.model))
            except native.NativeError:
                logger.exception("stored chunk does not decode: treated as a miss")
                return None
            return out
        if entry.encoded:
            T = entry.shape[2] if fmt == "vllm" else entry.shape[3]
            codec = self._codec()
            try:
                lay = native.KVLayout.from_chunk(out, fmt)
                if isinstance(entry, _PackChunk) and entry.pack.chunk_tokens >= T:
                    # a chunk of a pack is read where it lies (lmc_load_pack over one chunk): nothing is reassembled on
                    # the host, no pinned memory is taken
                    with torch.cuda.device(dev):
                        codec.finish_decode(codec.load_pack(entry.pack, entry.index, 1, lay, 0, None))
                else:
                    blob = self._own_blob(entry) if isinstance(entry, _PackChunk) else entry.blob
                    codec.finish_decode(codec.decode([blob], lay, 0, T))
            except native.NativeError:
                logger.exception("stored chunk does not decode: treated as a miss")
                return None
        else:
            cur = torch.cuda.current_stream(dev)
            native.memcpy_async(out.data_ptr(), entry.blob.ptr, entry.blob.nbytes, "h2d", cur.cuda_stream)
        return out

    def chunk_meta(self, key: CacheEngineKey) -> Tuple[Tuple[int, ...], torch.dtype]:
        """(shape, dtype) of the chunk tensor get(key) would return."""
        e = self.dict[key]
        return (tuple(e.shape), e.dtype)

    # ------------------------------------------------------------- range protocol
    def _stage_tensor(self, nbytes: int, dev) -> torch.Tensor:
        if self._stage is None or self._stage.numel() < nbytes:
            self._stage = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        return self._stage

    def put_kv_range(self, keys: Sequence[CacheEngineKey], src: native.KVLayout, fmt: str, tok_begin: int,
                     tok_end: int, chunk_tokens: int, blocking: bool = True, direct: bool = False) -> int:
        """Store chunks [tok_begin + i*chunk_tokens, ...) of `src` under keys[i], reading KV where it lies.
        direct (store_paged(direct=True)): the CacheGen tiers hand an "NHDB" cache to the encoder instead of staging it;
        the raw tiers gather every chunk themselves either way."""
        n = (tok_end - tok_begin + chunk_tokens - 1) // chunk_tokens
        assert n == len(keys), "one key per chunk"
        if n == 0:
            return 0
        L, H, D, tok = src.L, src.H, src.D, _token_axis(fmt)
        dt = native.torch_dtype(src.dtype)
        shapes = [_chunk_shape(fmt, L, min(chunk_tokens, tok_end - (tok_begin + i * chunk_tokens)), H, D)
                  for i in range(n)]
        ctx = native.get_context(self._cuda_device)
        dev = src.device
        if self.mode in ("cachegen", "hbm-cachegen"):
            out_dt = _coded_dtype(fmt, dt)
            if self.pack_stores and n >= 2:
                with torch.cuda.device(dev):
                    pjob = self._codec().store_pack(src, tok_begin, tok_end, chunk_tokens, self.cachegen_config.plane_bins(L),
                                                    self.host_arena, direct=direct)
                if blocking:
                    self._finish_pack(keys, pjob, shapes, out_dt)
                else:
                    self.put_queue.put(lambda: self._finish_pack(list(keys), pjob, shapes, out_dt))
                return n
            with torch.cuda.device(dev):
                job = self._codec().encode(src, tok_begin, tok_end, chunk_tokens, self.cachegen_config.plane_bins(L), direct=direct,
                                           **self._coder())
            if blocking:
                self._finish_encoded(keys, job, shapes, out_dt)
            else:
                self.put_queue.put(lambda: self._finish_encoded(list(keys), job, shapes, out_dt))
            return n
        if self.mode == "hbm":
            b, raw = self._tiers.budget["hbm"], sum(L * 2 * shp[tok] * H * D for shp in shapes) * dt.itemsize
            if b is not None and raw > b:
                self._not_cached(raw)  # (not even gathered: it fits nowhere)
                return n
            chunks = []
            for shp, i in zip(shapes, range(n)):
                chunk = torch.empty(shp, dtype=dt, device=dev)
                T = shp[tok]
                ctx.copy_kv(src, tok_begin + i * chunk_tokens, T, native.KVLayout.from_chunk(chunk, fmt), 0)
                chunks.append(chunk)
            self._keep_tensors(list(keys), chunks)
            return n
        # raw: gather every chunk into a device staging arena with the copy kernel, then D2H on the side stream
        codec = self._codec()
        cur = torch.cuda.current_stream(dev)
        eb = native.elem_bytes(src.dtype)
        chunk_bytes = L * 2 * chunk_tokens * H * D * eb
        stage = self._stage_tensor(n * chunk_bytes, dev)
        if self._stage_free is not None:
            cur.wait_event(self._stage_free)
        views = []
        for i, shp in enumerate(shapes):
            numel = 1
            for s in shp:
                numel *= s
            v = stage[i * chunk_bytes:i * chunk_bytes + numel * eb].view(dt).view(shp)
            T = shp[tok]
            ctx.copy_kv(src, tok_begin + i * chunk_tokens, T, native.KVLayout.from_chunk(v, fmt), 0)
            views.append(v)
        gathered = torch.cuda.Event()
        gathered.record(cur)
        codec.copy_stream.wait_event(gathered)
        total = sum(r16(v.numel() * eb) for v in views)

        def copy_out():
            entries = []
            try:
                for v in views:
                    nb = v.numel() * eb
                    hb = self.host_arena.alloc(nb, streams=[codec.copy_stream])
                    native.memcpy_async(hb.ptr, v.data_ptr(), nb, "d2h", codec.copy_stream.cuda_stream)
                    entries.append(_HostChunk(hb, None, tuple(v.shape), dt, False))
            except ArenaFull:
                evf = torch.cuda.Event()
                evf.record(codec.copy_stream)
                for e in entries:
                    self.host_arena.free(e.blob, [evf])
                raise
            return entries, total, None

        # (the group is visible once its copies have landed: blocking here, on the worker thread otherwise)
        box = {}

        def copy_and_wait():
            entries, nb, _ = copy_out()
            box["done"] = torch.cuda.Event()
            box["done"].record(codec.copy_stream)
            self._stage_free = box["done"]
            if blocking or self._tiers.budget["pinned"] is not None:
                box["done"].synchronize()
            return entries, nb, None

        if blocking or self._tiers.budget["pinned"] is not None:
            self._store("pinned", total, copy_and_wait, list(keys))
            return n
        entries, _, _ = copy_and_wait()
        done = box["done"]

        def finish():
            done.synchronize()
            with self._tier_lock:
                self._new_group("pinned", list(keys), entries, total)
                self._tiers.enforce()

        self.put_queue.put(finish)
        return n

    def begin_put_kv_layers(self, keys: Sequence[CacheEngineKey], src: native.KVLayout, fmt: str, tok_begin: int,
                            tok_end: int, chunk_tokens: int) -> Optional["LayerwisePut"]:
        """put_kv_range whose encode is issued layer by layer, while the forward pass that writes `src` is still running:
        -> a LayerwisePut (encode_layer(l) for l = 0 .. L-1, layer_event(l), finish(blocking)), or None -- the caller
        then stores in one piece with put_kv_range once every layer is there.  None is returned by the raw tiers (their
        gather IS the store), for a job the layer-wise encoder does not take (CacheGenDeviceCodec.encode_layers: a
        layout it cannot read in place, chunks outside 2 .. 256 tokens, planes of more than 1024 channels) and by the
        fixed-width tier unless LMCACHE_AMD_FIXED_LAYERWISE=1 was set when the backend was built (fixed_layerwise; then
        CacheGenDeviceCodec.encode_layers_fixed: any chunk length, the same layouts and planes).
        Replaces the store of the reference behind the forward pass (cache_engine.py:268-282) and the connector's gather
        of every layer in front of it (docs/source/developer_tutorial/LLM_Engine.rst:91-122).
        After finish() the backend holds what put_kv_range leaves for the same arguments -- the same keys, the same blob
        bytes; on the pinned tier the same pack (built from the finished blobs by the repack leg demotion uses,
        lmc_pack_blobs + DMA, so a later layer-wise retrieve is still cut by layers); budgets, LRU groups and publishing
        are put_kv_range's.  Nothing is published before finish()."""
        n = (tok_end - tok_begin + chunk_tokens - 1) // chunk_tokens
        assert n == len(keys), "one key per chunk"
        if n == 0 or self.mode not in ("cachegen", "hbm-cachegen") or (self.model == "fixed" and not self.fixed_layerwise):
            return None
        L, H, D = src.L, src.H, src.D
        codec = self._codec()
        encode_layers = codec.encode_layers_fixed if self.model == "fixed" else codec.encode_layers
        with torch.cuda.device(src.device):
            job = encode_layers(src, tok_begin, tok_end, chunk_tokens, self.cachegen_config.plane_bins(L))
        if job is None:
            return None
        shapes = [_chunk_shape(fmt, L, min(chunk_tokens, tok_end - (tok_begin + i * chunk_tokens)), H, D) for i in range(n)]
        return LayerwisePut(self, list(keys), job, shapes, _coded_dtype(fmt, native.torch_dtype(src.dtype)))

    def _finish_layers(self, keys: Sequence[CacheEngineKey], job, shapes, dtype) -> None:
        """A finished layer-wise encode job -> the tier, as put_kv_range files its own."""
        codec = self._codec()
        try:
            if not (self.pack_stores and job.nchunks >= 2):
                self._finish_encoded(keys, job, shapes, dtype)
                return
            # the pinned tier's pack, from the finished blobs
            L, H, D, cs = job.geometry
            group = self._group_of((L, H, D), cs, shapes)
            ntokens = group["ntokens"]
            sizes = codec.sizes_of(job)
            blobs = [job.arena[i * job.stride:i * job.stride + sizes[i]] for i in range(job.nchunks)]

            def finish():
                with torch.cuda.device(self._cuda_device):
                    pack = codec.demote_blobs(blobs, (L, H, D), cs, ntokens, self.host_arena, ready=[job.done])
                return [_PackChunk(pack, i, shp, dtype) for i, shp in enumerate(shapes)], r16(pack.blob.nbytes), None

            need = 0 if self._tiers.budget["pinned"] is None else r16(codec.demoted_bytes(sizes, (L, H, D), cs, ntokens))
            self._store("pinned", need, finish, keys, **group)
            job.offload_issued = True
        finally:
            codec.release_layer_stream(job)

    def get_kv_range(self, keys: Sequence[CacheEngineKey], dst: native.KVLayout, fmt: str, dst_tok0: int,
                     chunk_tokens: int, layers_per_launch: Optional[int] = None, jobs_out: Optional[list] = None,
                     post: Optional[native.RangePost] = None, heads: Optional[native.HeadWindow] = None) -> int:
        """Write chunk i (stored under keys[i]) to dst tokens dst_tok0 + i*chunk_tokens ...; tokens that land
        below 0 are dropped (retrieve()'s first-chunk trim, cache_engine.py:360-365).  Returns the number of
        leading chunks written (a key that has gone since `contains` ends the run, like the reference's break on
        the first None chunk, cache_engine.py:339-345); raises NativeError if a stored blob does not decode.
        post (CacheGen tiers, with jobs_out): a native.RangePost -- re-rotate the keys, scatter a staged chunk into an
        "NHDB" cache -- done to every layer range of every decode job before the range's event, by the C call that
        launches the range (HBM blobs: lmc_decode_chunks_schedule_post, packs: lmc_load_pack_post).  One lmc_range_post
        per job: a retrieve that spans several stores is several jobs, each with its own token window.  A run of pinned
        blobs that are no pack (a store of one chunk, LMCACHE_AMD_PINNED_PACKS=0) crosses PCIe whole before its first
        range is decoded (CacheGenDeviceCodec.decode_host_post): its events mean what the others' mean, but layer 0 waits
        for the run's whole transfer.
        heads (CacheGen tiers; ValueError on the raw ones and together with `post`, before anything is queued): a
        native.HeadWindow -- the chunks were stored under another tensor-parallel degree and have heads.src_heads heads,
        of which a window goes to heads of `dst`, which has a head count of its own.  HBM blobs, coded or fixed-width, are
        decoded where they lie and only the window's streams are read.  A pack chunk gives its blob (_own_blob) and the
        WHOLE blob crosses PCIe before the window is decoded from it (CacheGenDeviceCodec.decode): moving only the
        window's byte range of a pack is not built.  The decoders hold every blob's header against heads.src_heads."""
        if heads is not None:
            if not self.supports_head_window:
                raise ValueError(f"get_kv_range(heads=...): the {self.mode!r} tier stores raw chunks; a window of heads is "
                                 "decoded out of CacheGen blobs only (local_serde='cachegen' / 'cachegen-fixed')")
            if post is not None:
                raise ValueError("get_kv_range(heads=...) takes no post-op: it acts on every head of the destination; "
                                 "apply it once behind the last window")
        # the tier lock is held from taking the entries to the last launch: an eviction either happens before (the keys
        # are gone: a shorter run) or after (the jobs launched here are among the events its release is fenced by)
        with self._tier_lock:
            return self._get_kv_range_locked(keys, dst, fmt, dst_tok0, chunk_tokens, layers_per_launch, jobs_out, post, heads)

    def _get_kv_range_locked(self, keys, dst, fmt, dst_tok0, chunk_tokens, layers_per_launch, jobs_out, post=None,
                             heads=None) -> int:
        assert post is None or (jobs_out is not None and layers_per_launch and self.mode in ("cachegen", "hbm-cachegen")), \
            "a post-op rides on the layer ranges of the CacheGen tiers' decode jobs: it needs layers_per_launch and jobs_out"
        entries = self._prefix_entries(keys)
        if not entries:
            return 0
        ctx = native.get_context(self._cuda_device)
        dev = dst.device
        if self.mode == "hbm-cachegen" and all(isinstance(e, _DevChunk) for e in entries) and len({e.model for e in entries}) == 1:
            # blobs in HBM: one decode launch per range of layers, an event after each; with jobs_out the call
            # returns at once and the caller finishes the job (engine.retrieve_layerwise)
            codec = self._codec()
            with torch.cuda.device(dev):
                # (`entries` is the SAME list object for a repeated lookup of one prefix -- _prefix_entries -- and the codec
                # keeps the uploaded address table of the last few lists it has seen)
                job = codec.decode_device([e.blob for e in entries], dst, dst_tok0, chunk_tokens, layers_per_launch,
                                          same_blobs_as=entries, post=post, model=self._run_model(entries), heads=heads)
            self._touch(keys[:len(entries)], [job.done])
            if jobs_out is not None:
                jobs_out.append((codec, job))
            else:
                codec.finish_decode(job)
            return len(entries)
        if self.mode in ("cachegen", "hbm-cachegen"):
            # The entries split into maximal RUNS: consecutive chunks of one pack (what one put_kv_range stored) are one
            # lmc_load_pack -- a transfer and a decode per range of layers, straight from the pack --, a run of chunks
            # with blobs of their own is one decode over those blobs.  A retrieve that spans several stores (every turn
            # of a conversation, every prompt behind a shared prefix adds a pack) is a few such jobs on the same
            # streams, one behind the other; nothing is reassembled on the host and no pinned memory is allocated.
            # (A tiered hbm-cachegen backend whose prefix lies partly in HBM, partly demoted: its HBM blobs are runs of
            # a third kind, decoded where they lie.)
            codec = self._codec()
            runs, i = [], 0

            def kind_of(e):
                if isinstance(e, _DevChunk):
                    return "dev-fixed" if e.model == "fixed" else "dev"
                # (a window of heads: a pack chunk gives its own blob, which crosses PCIe whole -- see get_kv_range)
                return "pack" if isinstance(e, _PackChunk) and e.pack.chunk_tokens == chunk_tokens and heads is None else "blobs"
            while i < len(entries):
                e = entries[i]
                j = i + 1
                kind = kind_of(e)
                if kind == "pack":
                    while (j < len(entries) and isinstance(entries[j], _PackChunk) and entries[j].pack is e.pack
                           and entries[j].index == e.index + (j - i)):
                        j += 1
                else:
                    while j < len(entries) and kind_of(entries[j]) == kind:
                        j += 1
                runs.append((kind, i, j))
                i = j
            # (the HBM tier hands its jobs out whenever the caller takes them, as above; the pinned tier only cut by layers)
            layerwise = bool(layers_per_launch) and jobs_out is not None
            events = []
            for kind, i, j in runs:
                tok0 = dst_tok0 + i * chunk_tokens
                with torch.cuda.device(dev):
                    if kind in ("dev", "dev-fixed"):
                        job = codec.decode_device([e.blob for e in entries[i:j]], dst, tok0, chunk_tokens, layers_per_launch,
                                                  post=post, model=self._run_model(entries[i:j]), heads=heads)
                    elif kind == "pack":
                        job = codec.load_pack(entries[i].pack, entries[i].index, j - i, dst, tok0, layers_per_launch, post=post)
                    else:
                        # (a pack chunk of another chunk length -- never stored by this engine -- takes its blob from the pack)
                        blobs = [self._own_blob(e) if isinstance(e, _PackChunk) else e.blob for e in entries[i:j]]
                        if heads is not None:
                            job = codec.decode(blobs, dst, tok0, chunk_tokens, heads=heads)
                        elif post is not None:
                            # (whole blobs over PCIe, then the ranges' decodes with the post-op in front of every event)
                            job = codec.decode_host_post(blobs, dst, tok0, chunk_tokens, layers_per_launch, post)
                        elif layerwise:
                            # pinned tier cut by layers (engine.retrieve_layerwise): one lmc_load_chunks call gathers and
                            # decodes range after range; the caller's layers wait for their range's event only
                            job = codec.decode_host_layerwise(blobs, dst, tok0, chunk_tokens, layers_per_launch)
                        else:
                            job = codec.decode(blobs, dst, tok0, chunk_tokens)
                events.append(job.done)
                if (layerwise and not (heads is not None and kind == "blobs")) or (kind in ("dev", "dev-fixed") and jobs_out is not None):
                    jobs_out.append((codec, job))
                else:
                    codec.finish_decode(job)  # this decode's event, then its own status word
            self._touch(keys[:len(entries)], events)
            return len(entries)
        cur = torch.cuda.current_stream(dev)
        stage = None
        if self.mode == "raw":
            tot = sum(native.r16(e.blob.nbytes) for e in entries)
            stage = self._stage_tensor(tot, dev)
            if self._stage_free is not None:
                cur.wait_event(self._stage_free)
        off = 0
        for i, e in enumerate(entries):
            if isinstance(e, torch.Tensor):
                chunk = e
            else:
                numel = e.blob.nbytes // e.dtype.itemsize
                chunk = stage[off:off + e.blob.nbytes].view(e.dtype)[:numel].view(e.shape)
                native.memcpy_async(chunk.data_ptr(), e.blob.ptr, e.blob.nbytes, "h2d", cur.cuda_stream)
                off += native.r16(e.blob.nbytes)
            T = chunk.shape[2] if fmt == "vllm" else chunk.shape[3]
            t0 = dst_tok0 + i * chunk_tokens
            skip = max(0, -t0)
            if skip < T:
                ctx.copy_kv(native.KVLayout.from_chunk(chunk, fmt), skip, T - skip, dst, t0 + skip)
        ev = None
        if stage is not None:
            ev = torch.cuda.Event()
            ev.record(cur)
            self._stage_free = ev
        self._touch(keys[:len(entries)], [ev] if ev is not None else ())
        return len(entries)


class LMCLocalDiskBackend(LMCBackendInterface):
    """The local-disk tier (mirror of the reference's LMCLocalDiskBackend, lmcache/storage_backend/local_backend.py:
    163-310: `config.local_device` is a directory, one file per chunk named after the key, a set of the keys written
    by this process, `put` blocking or queued to a worker thread, `get` returning a tensor on the GPU).

    Two file formats, chosen like the host tier's by `config.local_serde`:
      None        the reference's own: a safetensors file holding the raw chunk under "kv_chunk" (:246, :300-303) --
                  files written by either implementation are read by the other;
      "cachegen"  the flat v6 blob (include/lmc_format.h) exactly as the GPU wrote it: put = fused HIP encode, DMA into
                  pinned memory, ONE write() from that buffer; get = ONE readinto() a pinned buffer, H2D on the copy
                  stream, decode straight into the returned tensor -- 4.6x less file I/O than the raw chunk, no
                  pickle, no intermediate host copy ("on-disk backend reuse").
    """

    def __init__(self, config: LMCacheEngineConfig, metadata: Optional[LMCacheEngineMetadata] = None):
        super().__init__()
        self.chunk_size = config.chunk_size
        self.config = config
        self.metadata = metadata
        self.path = config.local_device
        assert self.path is not None, "Need to specify local path if when using LMCLocalDiskBackend"
        if config.local_serde not in (None, "cachegen"):
            raise ValueError(f"Invalid local_serde: {config.local_serde}")
        self.encoded = config.local_serde == "cachegen"
        self.cachegen_config = None
        self.fmt = metadata.fmt if metadata is not None else None
        if self.encoded:
            native.lib()  # no CPU fallback: fail at construction if the HIP library is missing
            if metadata is None:
                raise ValueError("local_serde='cachegen' needs the engine metadata (model name, fmt)")
            self.cachegen_config = CacheGenConfig.from_model_name(metadata.model_name)
        if not os.path.exists(self.path):
            os.makedirs(self.path)
        self.existing_keys = set()
        self.update_lock = threading.Lock()
        self._io_lock = threading.Lock()       # one staging buffer per direction
        self._staging = None                   # PinnedArena, created on first encoded put
        self._read_buf: Optional[native.PinnedBuffer] = None
        self.dst_device = "cuda"
        self._cuda_device = torch.cuda.current_device() if torch.cuda.is_available() else None
        self.put_queue: "queue.Queue" = queue.Queue()
        self.put_thread: Optional[threading.Thread] = threading.Thread(target=self.put_worker, daemon=True)
        self.put_thread.start()

    def contains(self, key: CacheEngineKey) -> bool:
        return key in self.existing_keys

    def _key_to_path(self, key: CacheEngineKey) -> str:
        # the reference's naming (:222-236), the extension telling the two formats apart
        return self.path + key.to_string().replace("/", "-") + (".lmc" if self.encoded else ".pt")

    def put_worker(self):
        # the worker's own stream on the ENGINE's device (a thread starts on device 0), ordered behind whatever produced
        # each chunk: put() records an event on the caller's stream -- the engine fills the chunk with copy_kv on that
        # stream and returns at once -- and the queued put waits for it before it reads the tensor
        stream = None
        if self._cuda_device is not None:
            torch.cuda.set_device(self._cuda_device)
            stream = torch.cuda.Stream()
        while True:
            item = self.put_queue.get()
            if isinstance(item, LocalBackendEndSignal):
                break
            key, value, ready = item
            try:
                if stream is not None:
                    with torch.cuda.stream(stream):
                        if ready is not None:
                            stream.wait_event(ready)
                        self.put_blocking(key, value)
                else:
                    self.put_blocking(key, value)
            except Exception:
                logger.exception("queued disk put failed")

    @_lmcache_nvtx_annotate
    def put_blocking(self, key: CacheEngineKey, kv_chunk: torch.Tensor) -> None:
        path = self._key_to_path(key)
        tmp = f"{path}.{os.getpid()}.{threading.get_ident()}.tmp"
        if self.encoded:
            self._write_encoded(kv_chunk, tmp)
        else:
            from safetensors.torch import save_file
            save_file({"kv_chunk": kv_chunk.contiguous()}, tmp)
        os.replace(tmp, path)  # a reader never sees a half-written file
        # the order of "file complete" and "key visible" matters (:247-252)
        with self.update_lock:
            self.existing_keys.add(key)

    def _write_encoded(self, kv_chunk: torch.Tensor, path: str) -> None:
        fmt = _fmt_of_chunk(kv_chunk, self.fmt)
        if not kv_chunk.is_cuda:
            kv_chunk = kv_chunk.to(self.dst_device)
        with self._io_lock, torch.cuda.device(kv_chunk.device):
            if self._staging is None:
                self._staging = PinnedArena(slab_bytes=64 << 20)
            codec = get_codec(kv_chunk.device.index)
            lay = native.KVLayout.from_chunk(kv_chunk, fmt)
            job = codec.encode(lay, 0, lay.ntokens, lay.ntokens, self.cachegen_config.plane_bins(lay.L))
            sizes = codec.sizes_of(job)
            blobs, done = codec.offload(job, sizes, self._staging)
            done.synchronize()
            hb = blobs[0]
            view = (ctypes.c_uint8 * hb.nbytes).from_address(hb.ptr)
            fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
            try:
                mv, off = memoryview(view).cast("B"), 0
                while off < hb.nbytes:
                    off += os.write(fd, mv[off:])
            finally:
                os.close(fd)
            self._staging.reset()  # single in-flight blob: recycle the slab

    def put(self, key: CacheEngineKey, kv_chunk: torch.Tensor, blocking: bool = True) -> None:
        if blocking:
            self.put_blocking(key, kv_chunk)
        else:
            ready = None
            if kv_chunk.is_cuda:
                ready = torch.cuda.Event()
                ready.record(torch.cuda.current_stream(kv_chunk.device))
            self.put_queue.put((key, kv_chunk, ready))

    @_lmcache_nvtx_annotate
    def get(self, key: CacheEngineKey) -> Optional[torch.Tensor]:
        if key not in self.existing_keys:
            return None
        path = self._key_to_path(key)
        if not self.encoded:
            from safetensors import safe_open
            with safe_open(path, framework="pt", device=self.dst_device) as f:
                return f.get_tensor("kv_chunk")
        fmt = self.fmt or "vllm"
        dev = torch.device("cuda", torch.cuda.current_device())
        with self._io_lock, torch.cuda.device(dev):
            nbytes = os.path.getsize(path)
            if self._read_buf is None or self._read_buf.nbytes < nbytes:
                if self._read_buf is not None:
                    self._read_buf.free()
                self._read_buf = native.PinnedBuffer(max(native.r16(nbytes), 16 << 20))
            view = (ctypes.c_uint8 * nbytes).from_address(self._read_buf.ptr)
            with open(path, "rb", buffering=0) as f:
                mv, off = memoryview(view).cast("B"), 0
                while off < nbytes:
                    n = f.readinto(mv[off:])
                    if not n:
                        break
                    off += n
            try:
                if off != nbytes:
                    raise native.NativeError(f"short read: {off} of {nbytes} bytes")
                h = native.blob_info(bytes(mv[:native.HEADER_BYTES]), nbytes)
                shape, dtype = retrieve_spec(fmt, h)
                out = torch.empty(shape, dtype=dtype, device=dev)
                codec = get_codec(dev.index)
                hb = HostBlob(self._read_buf, 0, nbytes)
                # finish_decode waits for this decode: the read buffer is free again when the lock is released
                codec.finish_decode(codec.decode([hb], native.KVLayout.from_chunk(out, fmt), 0, h.ntokens))
            except native.NativeError:
                logger.exception("stored chunk does not decode: treated as a miss")
                return None
            return out

    def close(self):
        if self.put_thread is not None and self.put_thread.is_alive():
            self.put_queue.put(LocalBackendEndSignal())
            self.put_thread.join()
            logger.info("Closed the put worker in local disk backend")
        self.put_thread = None
        with self._io_lock:
            if self._staging is not None:
                self._staging.close()
                self._staging = None
            if self._read_buf is not None:
                self._read_buf.free()
                self._read_buf = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
