"""Device-side plumbing shared by the CacheGen serializer, deserializer and the
pinned-host backend: the jobs in flight, side copy stream, stream/event ordering.
The pinned host arena and the HBM blob arena the blobs live in are in
storage_backend/arena.py and re-exported here.  All compute goes through the
C ABI (lmcache_amd.native); this file only sequences it.

What it replaces in the reference: the implicit, synchronous data movement of
`pickle.dump` of CUDA tensors (cachegen_basics.py:131-136), `.cuda()` after
`pickle.load` (cachegen_decoder.py:144-147) and the pageable `.to("cpu")` /
`.to("cuda")` copies of LMCLocalBackend (local_backend.py:82-100, 128-144) --
with pinned `hipMemcpyAsync` on a side stream ordered by events (no device-wide
synchronisation: the reference itself flags torch.cuda.synchronize() as harmful
here, local_backend.py:83-85).
"""
import contextlib
import ctypes
import os
import threading
import weakref
from dataclasses import dataclass
from typing import List, Optional, Sequence

import torch

from lmcache_amd import native
from lmcache_amd.logging import init_logger
from lmcache_amd.storage_backend.arena import ArenaFull, DeviceArena, HostBlob, PinnedArena, _stream_waits  # noqa: F401

logger = init_logger(__name__)


class PinnedWords:
    """Pool of small pinned buffers the jobs in flight borrow (size words, pointer / size arrays, part words): hipHostMalloc
    stalls the device, so a buffer is allocated once and lent again and again."""

    def __init__(self):
        self._bufs: List[native.PinnedBuffer] = []

    def __len__(self) -> int:
        return len(self._bufs)

    def take(self, min_bytes: int, alloc_bytes: int) -> native.PinnedBuffer:
        """The first buffer of at least min_bytes, else a new one of alloc_bytes."""
        for k, b in enumerate(self._bufs):
            if b.nbytes >= min_bytes:
                return self._bufs.pop(k)
        return native.PinnedBuffer(alloc_bytes)

    def give(self, buf: native.PinnedBuffer) -> None:
        self._bufs.append(buf)

    def close(self) -> None:
        for b in self._bufs:
            b.free()
        self._bufs = []


def _borrow(loans: list, words: PinnedWords, min_bytes: int, alloc_bytes: int) -> native.PinnedBuffer:
    """A buffer of `words`, entered in the launch's `loans` (whoever holds the list gives it back)."""
    buf = words.take(min_bytes, alloc_bytes)
    loans.append((buf, words))
    return buf


def _raise_on(st: int, what: str) -> None:
    if st:
        raise native.NativeError(f"{what}: " + native.describe_status(st))


class Job:
    """What every job in flight owns: the event behind its last kernel, its own status word, and its loans -- pinned
    buffers its kernels read or write, each with the PinnedWords it goes back to."""

    def __init__(self, done, status_idx: int, pool: native.StatusWords, loans=()):
        self.done = done                # recorded after the job's last kernel
        self.status_idx = status_idx    # this job's status word (native.StatusWords); -1 once read
        self.pool = pool                # where status_idx goes back to
        self._loans = list(loans)       # [(PinnedBuffer, PinnedWords)]

    def retire(self) -> int:
        """`done` has fired: the status word is read and returned, every loan goes back to its pool -> the status
        (0 for a job that has been retired before)."""
        st = 0
        if self.status_idx >= 0:
            st, self.status_idx = self.pool.read_release(self.status_idx), -1
        for buf, words in self._loans:
            words.give(buf)
        self._loans = []
        return st

    def __del__(self):  # a job dropped unread (an exception between launch and completion): its words return once its
        if getattr(self, "status_idx", -1) < 0:  # kernels can no longer write them
            return
        try:
            self.done.synchronize()
        except Exception:
            pass
        try:
            self.retire()
        except Exception:
            pass


class EncodeJob(Job):
    def __init__(self, nchunks: int, stride: int, arena: torch.Tensor, sizes: native.PinnedBuffer, geometry: tuple,
                 parts: list, **base):
        super().__init__(parts[-1][2], **base)
        self.nchunks, self.stride = nchunks, stride
        self.arena = arena          # device uint8, blob i at i*stride
        self.sizes = sizes          # this job's own uint32 [nchunks], written by the GPU; back in the pool once read
        self.geometry = geometry    # (L, H, D, chunk_tokens)
        self.size_list: Optional[List[int]] = None  # filled by sizes_of / offload
        # a long job is launched as a few consecutive ranges of chunks, each with its own event, so that the
        # host-DRAM offload of range r can start while range r+1 is still being encoded: (chunk0, chunk1, event)
        self.parts = parts
        self.offload_issued = False  # its device -> host copies are on the copy streams (the arena may be reused after them)

    def retire(self) -> int:
        self.sizes = None
        return super().retire()


class LayerwiseEncodeJob(EncodeJob):
    """An encode issued layer by layer (CacheGenDeviceCodec.encode_layers / encode_layers_fixed; lmc_encode_layers_*,
    csrc/k_layers.h, and for the fixed-width model csrc/k_fixed.h):
    encode_layer(l) for l = 0 .. L-1 in order, then finish().  After finish() it IS an EncodeJob -- arena at blob_bound
    stride, pinned size words, its own status word, `done` behind its last kernel -- whose blobs are byte for byte those
    of CacheGenDeviceCodec.encode() for the same source, range, chunk length and bins: sizes_of, offload and
    keep_on_device take it unchanged.  The coder never runs on the caller's stream: every launch goes to the job's side
    stream, behind an event recorded on the caller's current stream in encode_layer.
    layer_events[l] (after encode_layer(l)): behind it layer l's KV has been read -- the cache may be overwritten."""

    def __init__(self, handle: native.LayerEncodeHandle, stream, nlayers: int, **kw):
        super().__init__(**kw)
        self.handle, self.stream, self.nlayers = handle, stream, nlayers
        self.layer_events: List[torch.cuda.Event] = []
        self.finished = False

    def encode_layer(self, layer: int) -> None:
        """Layer `layer`'s KV, as the caller's current stream has written it, is quantised and coded on the side stream."""
        dev = self.arena.device
        with torch.cuda.device(dev):
            ready = torch.cuda.Event()
            ready.record(torch.cuda.current_stream(dev))
            self.stream.wait_event(ready)
            self.handle.encode_layer(layer, self.stream.cuda_stream)  # (raises, with nothing queued, out of order)
            ev = torch.cuda.Event()
            ev.record(self.stream)
            self.layer_events.append(ev)

    def finish(self) -> "LayerwiseEncodeJob":
        """The finish kernel (k_layers_finish, k_fixed_layers_finish) behind the last layer; `done` is recorded behind it.
        No host wait."""
        with torch.cuda.device(self.arena.device):
            self.handle.finish(self.stream.cuda_stream)
            self.done.record(self.stream)
        self.finished = True
        return self

    def abort(self) -> None:
        """Give the job up: the C side's buffers go back behind what was queued; the job's words once that has run."""
        if not self.finished:
            self.handle.abort()
            self.done.record(self.stream)
            self.finished = True

    def __del__(self):
        try:
            if not getattr(self, "finished", True):
                self.abort()
        except Exception:
            pass
        super().__del__()


@dataclass
class HostPack:
    """The blobs of one store call in pinned host DRAM, laid out plane-major (include/lmc_format.h, "pack" v3)."""
    blob: HostBlob
    nchunks: int
    chunk_tokens: int

    def extract(self, chunk: int) -> bytes:
        """Chunk `chunk` as the blob lmc_encode_chunks wrote (host-side reassembly)."""
        return native.pack_extract(self.blob.ptr, self.blob.nbytes, chunk)


class PackJob(Job):
    """One store_pack() in flight."""

    def __init__(self, nchunks: int, chunk_tokens: int, geometry: tuple, dev: torch.Tensor, cap: int,
                 sizes: native.PinnedBuffer, part_info: native.PinnedBuffer, part_events: list, **base):
        super().__init__(**base)
        self.nchunks, self.chunk_tokens = nchunks, chunk_tokens
        self.geometry = geometry    # (L, H, D)
        self.dev, self.cap = dev, cap   # the HBM region the pack is written to first (allocated at an upper bound)
        self.d2h_issued = False     # ... and whether its copies to pinned memory have been queued
        self.sizes = sizes
        # the encode went out in plane ranges (lmc_store_pack_parts); part r's bytes may leave once part_events[r]
        # has fired: part_info (pinned uint64 [2 nparts]) says where they lie
        self.part_events, self.part_info = part_events, part_info

    def retire(self) -> int:
        self.sizes = self.part_info = None
        return super().retire()


def pack_cap(n: int, L: int, T: int, H: int, D: int, bins: Sequence[int]) -> int:
    """Bytes a pack of n T-token chunks can need: the static sections plus, per group stream, its largest head (every
    symbol of the plane at the widest count) and the coder's bound -- a lane emits at most T * log2(symbols) + 48 bits
    (DESIGN.md "stream bound"; chunks below 256 tokens: + 1.44 bit per symbol kind for the rounding of the scaled model
    counts, lmc_format.h) -- with 3 % on top."""
    import math
    G = (H * D + native.LANES - 1) // native.LANES
    static = native.r16(native.blob_static_bytes(L, T, H, D))
    width = (255 if T == 256 else T).bit_length()
    streams = 0
    for b in bins:
        lane_bytes = math.ceil((T * math.log2(max(2, b - 1)) * 1.03 + 128) / 8) + 4
        head = native.r16(((b - 1 + 7) & ~7) + 8 * (b - 1) * width)
        streams += G * (head + native.r16(native.LANES * lane_bytes))
    return min(native.pack_bound(n, L, T, H, D), native.r16(256 + 8 * (2 * L * n + 1)) + n * (static + streams))


def layer_ranges(L: int, layers_per_launch) -> list:
    """[(first layer, end layer), ...] covering 0..L: one range when layers_per_launch is None / 0, ranges of a
    fixed size for an int, and for a sequence of sizes the ranges it lists, its last size repeating."""
    if not layers_per_launch:
        return [(0, L)]
    sizes = [layers_per_launch] if isinstance(layers_per_launch, int) else list(layers_per_launch)
    out, l0, i = [], 0, 0
    while l0 < L:
        step = max(1, min(L - l0, int(sizes[min(i, len(sizes) - 1)])))
        out.append((l0, l0 + step))
        l0 += step
        i += 1
    return out


def range_step(L: int, layers_per_range) -> int:
    """Layers per range of the loads that take ONE range size (lmc_load_chunks, lmc_load_pack): None / 0 is a single
    range of all L layers, an int is held to 1..L, and of a schedule of sizes the first entry is used."""
    if layers_per_range and not isinstance(layers_per_range, int):
        layers_per_range = list(layers_per_range)[0]
    return max(1, min(L, int(layers_per_range or L)))


class DecodeJob(Job):
    """One decode() call in flight: `done` fires after its last kernel, `status_idx` is its own status word.
    layer_events (decode_device with layers_per_launch): (first layer after the range, event) per launch, in layer
    order -- the KV of layers below `first layer after` is complete once the event has fired."""

    def __init__(self, done, layer_events: Optional[list] = None, table: Optional[torch.Tensor] = None, **base):
        super().__init__(done, **base)
        self.layer_events = layer_events
        self._table = table  # decode_device: the address table the kernels read, alive as long as the job


class CacheGenDeviceCodec:
    """Per-device encode/decode sequencer."""

    def __init__(self, device: Optional[int] = None):
        self.device_index = torch.cuda.current_device() if device is None else int(device)
        self.device = torch.device("cuda", self.device_index)
        self.ctx = native.get_context(self.device_index)
        self.copy_stream = torch.cuda.Stream(device=self.device)
        # a second DMA queue for the device -> host leg: two hipMemcpyAsync streams keep two SDMA engines busy
        self.copy_stream2 = torch.cuda.Stream(device=self.device)
        self.d2h_streams = 2
        self.encode_parts = 4                                # ranges a long encode job is launched in
        self._lock = threading.RLock()
        self._enc_arena: Optional[torch.Tensor] = None
        self._dec_arena: Optional[torch.Tensor] = None
        self._size_pool = PinnedWords()                      # pinned size words, one buffer per job in flight
        self._meta_pool = PinnedWords()                      # pinned pointer / size arrays of decode_host_layerwise jobs
        self._part_info_pool = PinnedWords()                 # pinned part words of store_pack jobs
        self._status = native.StatusWords()                  # one status word per job in flight
        self._arena_free: Optional[torch.cuda.Event] = None  # D2H of the last job that used the shared arena done
        self._dec_free: Optional[torch.cuda.Event] = None    # previous decode kernel done
        self._stage: Optional[native.PinnedBuffer] = None    # staging for pageable `bytes` inputs
        self._shared_job: Optional[EncodeJob] = None         # last job that encoded into the shared arena
        self.decode_batch_chunks = 8                         # chunks per H2D/decode pipeline stage
        self._pack_dev: Optional[torch.Tensor] = None        # HBM staging of a pack on its way to pinned memory (store_pack)
        self._pack_dev_free: Optional[torch.cuda.Event] = None
        self._xcode_dev: Optional[torch.Tensor] = None       # HBM staging of a fixed-width group's coded blobs (transcode_fixed)
        self._pack_prev = None                               # weak reference to the last PackJob that took _pack_dev
        # plane ranges a pack's encode is launched in (store_pack): LMCACHE_AMD_PACK_PARTS=1 is the round-5 behaviour
        # (the whole encode, then the pack, then its copies), for A/B
        self.pack_parts = max(1, min(16, int(os.environ.get("LMCACHE_AMD_PACK_PARTS", "8"))))
        self._layer_streams: List[torch.cuda.Stream] = []    # side streams of finished layer-wise encode jobs, for the next ones
        self._warned_wide_split = False                      # direct store of an NHDB cache with planes the split quantiser does not read
        self._same_blobs: dict = {}                          # id(caller's list) -> (the list, its blobs' address tuple, largest blob)
        self._table_cache: dict = {}                         # blob-address tuple -> (device table, upload stream)

    # ---- encode ------------------------------------------------------------------
    def _readable(self, src: native.KVLayout, tok_begin: int, tok_end: int, direct: bool = False):
        """The encoders read 16-byte vectors (native.KVLayout.vector_readable).  The reference's serde takes any shape
        (torch_quant_vectorized, cachegen_encoder.py:40-61), so a range of a layout that is not -- a head_size that is no
        multiple of 8 under a huggingface / NHBD layout, rows off a 16-byte boundary, or by default the "NHDB" cache of
        vLLM's ROCm paged-attention kernels, which has no rows at all -- is first brought into a contiguous vllm chunk on
        the device (lmc_copy_kv: element-wise for the former, k_copy_split.h's gather for the latter) and encoded from
        there.  direct: an "NHDB" cache with planes of at most 1024 channels goes to the encoder as it is
        (lmc_encode_chunks_split, lmc_encode_chunks_fixed_split and the stores read the split blocks: k_quantize.h); wider
        planes are staged all the same, whichever coder model."""
        if src.vector_readable():
            return src, tok_begin, tok_end
        if direct and src.struct.paged_kind == native.PAGED_SPLIT:
            if src.H * src.D <= 1024:
                return src, tok_begin, tok_end
            if not self._warned_wide_split:
                self._warned_wide_split = True
                logger.warning("direct store from an NHDB cache: planes of %d channels are wider than the 1024 the split "
                               "encoders (coded and fixed-width) read; staging through lmc_copy_kv", src.H * src.D)
        n = tok_end - tok_begin
        with torch.cuda.device(self.device):
            chunk = torch.empty((src.L, 2, n, src.H, src.D), dtype=native.torch_dtype(src.dtype), device=src.device)
            self.ctx.copy_kv(src, tok_begin, n, native.KVLayout.from_chunk(chunk, "vllm"), 0)
        return native.KVLayout.from_chunk(chunk, "vllm"), 0, n

    # (coder model, split layout) -> the context's method; the coded schedules take a split destination themselves
    _ENCODERS = {(None, False): "encode_chunks", (None, True): "encode_chunks_split",
                 ("fixed", False): "encode_chunks_fixed", ("fixed", True): "encode_chunks_fixed_split"}
    _SCHEDULES = {("fixed", False): "decode_chunks_fixed_schedule", ("fixed", True): "decode_chunks_fixed_split_schedule"}
    # ... with a window of heads (native.HeadWindow): one export per model, which takes either layout
    _HEAD_SCHEDULES = {("fixed", False): "decode_chunks_fixed_heads_schedule", ("fixed", True): "decode_chunks_fixed_heads_schedule"}

    # coder model of a group's HBM blobs -> the codec's method that turns them into entropy-coded blobs in front of the pack
    # leg of a demotion (None: they are coded already)
    _DEMOTERS = {None: None, "fixed": "transcode_fixed"}
    # ... and the way back: the codec's method that turns a pack's entropy-coded blobs into the model's HBM blobs behind
    # the unpack leg of a promotion (None: the HBM tier keeps them coded)
    _PROMOTERS = {None: None, "fixed": "transcode_to_fixed"}

    def _entry(self, names: dict, model: Optional[str], layout: native.KVLayout, default: Optional[str] = None):
        """self.ctx's method, looked up at call time, for an encode from / a decode into `layout` in coder `model`: the one
        place that knows the models -- None, the entropy-coded blobs, and "fixed", LMC_MODEL_FIXED, 16-bit KV only."""
        if model not in (None, "fixed"):
            raise ValueError(f"unknown coder model {model!r} (None or 'fixed')")
        if model == "fixed" and native.elem_bytes(layout.dtype) != 2:
            raise ValueError("the fixed-width model stores bf16 / fp16 KV only")
        return getattr(self.ctx, names.get((model, layout.struct.paged_kind == native.PAGED_SPLIT), default))

    @staticmethod
    def _job_size(src: native.KVLayout, tok_begin: int, tok_end: int, chunk_tokens: int) -> tuple:
        """(chunks, arena stride of a blob) of an encode job."""
        return -(-(tok_end - tok_begin) // chunk_tokens), native.r16(native.blob_bound(src.L, chunk_tokens, src.H, src.D))

    def encode(self, src: native.KVLayout, tok_begin: int, tok_end: int, chunk_tokens: int,
               bins: Sequence[int], direct: bool = False, model: Optional[str] = None) -> EncodeJob:
        """Launch the fused encode of every chunk of [tok_begin, tok_end) on the CURRENT stream
        (so it is ordered after whatever produced the KV).  Asynchronous.  direct: see _readable.
        model: None -- the entropy-coded blobs; "fixed" -- LMC_MODEL_FIXED (lmc_encode_chunks_fixed, for a split source
        lmc_encode_chunks_fixed_split: fixed-width symbols, for blobs that stay in HBM; 16-bit KV only)."""
        self._entry(self._ENCODERS, model, src)  # (what is refused is refused before anything is staged)
        src, tok_begin, tok_end = self._readable(src, tok_begin, tok_end, direct)
        encode_chunks = self._entry(self._ENCODERS, model, src)
        L, H, D = src.L, src.H, src.D
        n, stride = self._job_size(src, tok_begin, tok_end, chunk_tokens)
        with self._lock:
            with torch.cuda.device(self.device):
                # The shared arena may be rewritten only after the copies of the last job that used it have been
                # ISSUED (then `_arena_free` orders us behind them).  A non-blocking store defers its offload to the
                # backend's worker thread: while that has not happened, a new job gets an arena of its own.
                prev = self._shared_job
                if prev is None or prev.offload_issued:
                    if self._enc_arena is None or self._enc_arena.numel() < n * stride:
                        self._enc_arena = torch.empty(n * stride, dtype=torch.uint8, device=self.device)
                    arena = self._enc_arena
                else:
                    arena = torch.empty(n * stride, dtype=torch.uint8, device=self.device)
                # every job owns its size words and its status word: a second store never waits for the first
                # one's sizes to be read (the reference's own note on this path: "synchronize is harmful",
                # local_backend.py:83-90), and never sees its failures
                cur = torch.cuda.current_stream(self.device)
                loans = []
                with self._launch(cur, loans) as (st, st_ptr):
                    sizes = _borrow(loans, self._size_pool, 4 * n, 4 * max(n, 256))
                    if arena is self._enc_arena and self._arena_free is not None:
                        cur.wait_event(self._arena_free)  # previous job's D2H has read the arena
                    nparts = self.encode_parts if n >= 4 * self.encode_parts else 1
                    per = (n + nparts - 1) // nparts
                    parts = []
                    for c0 in range(0, n, per):
                        c1 = min(n, c0 + per)
                        encode_chunks(src, tok_begin + c0 * chunk_tokens, min(tok_end, tok_begin + c1 * chunk_tokens),
                                      chunk_tokens, bins, arena.data_ptr() + c0 * stride, stride,
                                      sizes.ptr + 4 * c0, stream=cur.cuda_stream, status_ptr=st_ptr)
                        ev = torch.cuda.Event()
                        ev.record(cur)
                        parts.append((c0, c1, ev))
            job = EncodeJob(n, stride, arena, sizes, (L, H, D, chunk_tokens), parts, status_idx=st, pool=self._status, loans=loans)
            if arena is self._enc_arena:
                self._shared_job = job
            return job

    def encode_layers(self, src: native.KVLayout, tok_begin: int, tok_end: int, chunk_tokens: int,
                      bins: Sequence[int]) -> Optional[LayerwiseEncodeJob]:
        """encode() issued layer by layer -> a LayerwiseEncodeJob (encode_layer(l), finish()), or None when the job is
        not eligible and the caller encodes in one piece: a source the encoders do not read in place (_readable would
        stage it -- there is nothing to stage before the layers exist), a chunk, the ragged last one included, outside
        2 .. 256 tokens, planes of more than 1024 channels (lmc_encode_layers_begin).  Nothing is queued here.
        The job has an arena of its own and a side stream: it spans a forward pass and must not hold the shared encode
        arena, nor the model's stream."""
        return self._encode_layers(src, tok_begin, tok_end, chunk_tokens, bins, None)

    def encode_layers_fixed(self, src: native.KVLayout, tok_begin: int, tok_end: int, chunk_tokens: int,
                            bins: Sequence[int]) -> Optional[LayerwiseEncodeJob]:
        """encode(model="fixed") issued layer by layer (lmc_encode_layers_begin_fixed, csrc/k_fixed.h): the same job
        object as encode_layers', and after finish() an EncodeJob of the fixed-width model -- sizes_of and keep_on_device
        take it as they take encode(model="fixed")'s.  None: a source the encoders do not read in place, or planes of
        more than 1024 channels; every chunk length is eligible.  fp8 KV raises, as in encode()."""
        return self._encode_layers(src, tok_begin, tok_end, chunk_tokens, bins, "fixed")

    # coder model -> the context's begin of a layer-wise job
    _LAYER_BEGINS = {None: "encode_layers_begin", "fixed": "encode_layers_begin_fixed"}

    def _encode_layers(self, src: native.KVLayout, tok_begin: int, tok_end: int, chunk_tokens: int,
                       bins: Sequence[int], model: Optional[str]) -> Optional[LayerwiseEncodeJob]:
        """The one body of encode_layers / encode_layers_fixed."""
        begin = self._entry({}, model, src, self._LAYER_BEGINS.get(model))  # (one entry per model: it takes either layout)
        split = src.struct.paged_kind == native.PAGED_SPLIT
        if not (src.vector_readable() or (split and src.H * src.D <= 1024)):
            return None
        L, H, D = src.L, src.H, src.D
        n, stride = self._job_size(src, tok_begin, tok_end, chunk_tokens)
        with self._lock, torch.cuda.device(self.device):
            side = self._layer_streams.pop() if self._layer_streams else torch.cuda.Stream(device=self.device)
            arena = torch.empty(n * stride, dtype=torch.uint8, device=self.device)
            arena.record_stream(side)
            loans = []
            with self._launch(side, loans) as (st, st_ptr):
                sizes = _borrow(loans, self._size_pool, 4 * n, 4 * max(n, 256))
                handle = begin(src, tok_begin, tok_end, chunk_tokens, bins, arena.data_ptr(), stride, sizes.ptr, status_ptr=st_ptr)
            if handle is None:  # not eligible: nothing was queued, the words go back as they came
                self._status.read_release(st)
                for buf, words in loans:
                    words.give(buf)
                self._layer_streams.append(side)
                return None
            done = torch.cuda.Event()
            return LayerwiseEncodeJob(handle, side, L, nchunks=n, stride=stride, arena=arena, sizes=sizes,
                                      geometry=(L, H, D, chunk_tokens), parts=[(0, n, done)], status_idx=st,
                                      pool=self._status, loans=loans)

    def release_layer_stream(self, job: LayerwiseEncodeJob) -> None:
        """A finished job's side stream goes back for the next job (whose work queues behind what is left on it)."""
        with self._lock:
            if job.stream is not None and len(self._layer_streams) < 8:
                self._layer_streams.append(job.stream)
            job.stream = None

    @contextlib.contextmanager
    def _launch(self, stream, loans=()):
        """The guard around every launch sequence: acquires the job's status word and yields (its index, its address).
        A sequence that fails half way may have queued kernels that still write the word and the `loans` taken so far
        (_borrow), so they go back to their pools only after the stream has drained (an error path: the host wait does
        not matter)."""
        st = self._status.acquire()
        try:
            yield st, self._status.ptr(st)
        except BaseException:
            try:
                stream.synchronize()
            except Exception:
                pass
            self._status.read_release(st)
            for buf, words in loans:
                words.give(buf)
            raise

    def sizes_of(self, job: EncodeJob) -> List[int]:
        """Wait for THIS job only (event, not device) and read the blob sizes the GPU wrote to pinned memory."""
        with self._lock:
            if job.size_list is None:
                job.done.synchronize()
                job.size_list = job.sizes.tensor[:4 * job.nchunks].view(torch.int32).tolist()  # before the words go back
                _raise_on(job.retire(), "CacheGen encode")
            return job.size_list

    def offload(self, job: EncodeJob, sizes: Optional[Sequence[int]], arena: PinnedArena) -> (List[HostBlob], torch.cuda.Event):
        """hipMemcpyAsync every blob to pinned host DRAM on the side streams, exact sizes.  With sizes=None the
        sizes are read range by range as the job's ranges complete, so the copies of one range overlap the
        encode of the next (job.size_list is filled on the way)."""
        blobs = []
        with self._lock:
            streams = [self.copy_stream]
            if self.d2h_streams > 1 and job.nchunks > 1:
                streams.append(self.copy_stream2)
            progressive = sizes is None and job.size_list is None and job.parts is not None
            if progressive:
                sizes = []
            elif sizes is None:
                sizes = self.sizes_of(job)
            for c0, c1, ev in (job.parts if progressive else [(0, job.nchunks, job.done)]):
                if progressive:
                    ev.synchronize()  # this range only
                    sizes.extend(job.sizes.tensor[4 * c0:4 * c1].view(torch.int32).tolist())
                for st in streams:
                    st.wait_event(ev)
                for i in range(c0, c1):
                    try:
                        hb = arena.alloc(sizes[i], streams=streams)
                    except ArenaFull:
                        evf = self._join_copy_streams(both=len(streams) > 1)
                        for b in blobs:  # (the copies queued so far still write them)
                            arena.free(b, [evf])
                        raise
                    native.memcpy_async(hb.ptr, job.arena.data_ptr() + i * job.stride, sizes[i], "d2h",
                                        streams[i % len(streams)].cuda_stream)
                    blobs.append(hb)
            if progressive:
                job.size_list = list(sizes)
                _raise_on(job.retire(), "CacheGen encode")  # every range's event has fired
            ev = self._join_copy_streams(both=len(streams) > 1)
            job.offload_issued = True
            if job.arena is self._enc_arena:
                self._arena_free = ev
        return blobs, ev

    def _join_copy_streams(self, both: bool = True) -> torch.cuda.Event:
        """-> an event behind what has been queued on the copy streams: the second queue is folded into the first (if it
        was used at all), so one event covers both."""
        if both:
            ev2 = torch.cuda.Event()
            ev2.record(self.copy_stream2)
            self.copy_stream.wait_event(ev2)
        ev = torch.cuda.Event()
        ev.record(self.copy_stream)
        return ev

    def keep_on_device(self, job: EncodeJob, arena: DeviceArena) -> List[torch.Tensor]:
        """The job's blobs copied (exact sizes, device to device, on the current stream) into a persistent HBM arena
        -- the store leg of the HBM-resident CacheGen tier."""
        sizes = self.sizes_of(job)
        out = []
        with self._lock, torch.cuda.device(self.device):
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(job.done)
            try:
                for i, n in enumerate(sizes):
                    t = arena.alloc(n, stream=cur)
                    native.memcpy_async(t.data_ptr(), job.arena.data_ptr() + i * job.stride, n, "d2d", cur.cuda_stream)
                    out.append(t)
            except ArenaFull:
                ev = torch.cuda.Event()
                ev.record(cur)
                for t in out:  # (the copies queued so far still write them)
                    arena.free(t, [ev])
                raise
            ev = torch.cuda.Event()
            ev.record(cur)
            job.offload_issued = True
            if job.arena is self._enc_arena:
                self._arena_free = ev
        return out

    # ---- decode ------------------------------------------------------------------
    def decode_device(self, blobs: Sequence[torch.Tensor], dst: native.KVLayout, dst_tok0: int, chunk_tokens: int,
                      layers_per_launch: Optional[int] = None, same_blobs_as=None,
                      post: Optional[native.RangePost] = None, model: Optional[str] = None,
                      heads: Optional[native.HeadWindow] = None) -> Optional[DecodeJob]:
        """Decode blobs that live in HBM (uint8 CUDA tensors, anywhere) straight into `dst` on the current stream,
        no staging copy: the kernel takes the blob addresses from a pointer table.  With layers_per_launch the
        retrieve is cut into one launch per range of layers with an event after each (DecodeJob.layer_events): the
        model can start on layer 0 after 1/L of the decode.  layers_per_launch is a range size or a schedule of
        range sizes whose last entry repeats, e.g. (2, 2, 4, 8, 16): small ranges first so that the model starts
        early, large ones later (a launch of few layers does not fill the GPU, and every launch costs an event).
        post: a native.RangePost done to every range between its launch and its event, by the same C call
        (lmc_decode_chunks_schedule_post); its struct is filled here, per call -- the kept tables are not touched.
        model "fixed": the blobs are LMC_MODEL_FIXED (lmc_decode_chunks_fixed_schedule; `dst` is 16-bit rows, or a 16-bit
        "NHDB" cache through lmc_decode_chunks_fixed_split_schedule); the ranges, their events and `post` are the same.
        heads: a native.HeadWindow -- the blobs have heads.src_heads heads, of which a window goes to heads of `dst`, which
        has a head count of its own (lmc_decode_chunks_heads_schedule / _fixed_heads_schedule).  No `post` then: it would
        act on every head of `dst`; the caller applies it once, behind the last window (RangePost.apply)."""
        n = len(blobs)
        if n == 0:
            return None
        if heads is not None and post is not None:
            raise ValueError("a head-window decode takes no post-op: apply it once behind the last window")
        # (the coded schedule without a post-op is an export of its own: lmc_decode_chunks_schedule)
        if heads is not None:
            schedule = self._entry(self._HEAD_SCHEDULES, model, dst, "decode_chunks_heads_schedule")
        else:
            schedule = self._entry(self._SCHEDULES, model, dst, "decode_chunks_schedule" if post is None else "decode_chunks_schedule_post")
        with self._lock, torch.cuda.device(self.device):
            cur = torch.cuda.current_stream(self.device)
            # The blob addresses of THIS call: any number of chunks (a 128 k-token retrieve is 512 of them), uploaded
            # stream-ordered from pinned memory of torch's caching host allocator -- no host wait.  The last few tables are
            # kept, keyed by the addresses themselves (round 6): the warm prefix of a serving engine -- a system prompt, the
            # earlier turns of a conversation -- is the SAME blob set call after call, and building + uploading the table was
            # a third of the host time in front of the first decode launch.  (A table is a function of its key: a stale
            # entry cannot be wrong, only unused.)
            # same_blobs_as: an object the caller hands over again whenever -- and only when -- `blobs` are the same
            # tensors (the backend's kept entry list of a prefix): then not even the 64 data_ptr() calls are repeated.  The
            # object is kept alive beside its key, so its id cannot be recycled while the entry exists.
            # The largest blob of the call -- what k_decode holds every header's total against -- is NOT a function of the
            # addresses (an arena closed and reopened hands out the same address for a blob of another size), so it is
            # never kept beside the table: it is taken from THIS call's blobs, or kept with same_blobs_as, whose promise of
            # "the same tensors" covers their sizes.
            ptrs = bound = None
            if same_blobs_as is not None:
                known = self._same_blobs.get(id(same_blobs_as))
                if known is not None and known[0] is same_blobs_as:
                    ptrs, bound = known[1], known[2]
            if ptrs is None:
                ptrs = tuple(b.data_ptr() for b in blobs)
                bound = max(b.numel() for b in blobs)
                if same_blobs_as is not None:
                    if len(self._same_blobs) >= 8:
                        self._same_blobs.pop(next(iter(self._same_blobs)))
                    self._same_blobs[id(same_blobs_as)] = (same_blobs_as, ptrs, bound)
            hit = self._table_cache.get(ptrs)
            if hit is None:
                table = torch.tensor(ptrs, dtype=torch.int64).pin_memory().to(self.device, non_blocking=True)
                if len(self._table_cache) >= 8:
                    self._table_cache.pop(next(iter(self._table_cache)))
                self._table_cache[ptrs] = (table, cur)
            else:
                table, up = hit
                if up is not cur:  # uploaded on another stream: order this one behind that copy (once)
                    cur.wait_stream(up)
                    self._table_cache[ptrs] = (table, cur)
            with self._launch(cur) as (st, st_ptr):
                events = self._run_schedule(schedule, table, bound, n, dst, dst_tok0, chunk_tokens, layers_per_launch, post,
                                            cur, st_ptr, heads)
            return DecodeJob(events[-1][1], events if layers_per_launch else None, table, status_idx=st, pool=self._status)

    @staticmethod
    def _run_schedule(schedule, table: torch.Tensor, bound: int, n: int, dst: native.KVLayout, dst_tok0: int, chunk_tokens: int,
                      layers_per_launch, post: Optional[native.RangePost], cur, st_ptr: int,
                      heads: Optional[native.HeadWindow] = None) -> list:
        """ONE C-ABI call (`schedule`) launches every range of layers over the n blobs `table` addresses, none larger than
        `bound`, and records the range's event behind it, `post` in between -> [(first layer after the range, event)].
        heads: the window of a head-window schedule (which takes no post)."""
        ends = [l1 for _, l1 in layer_ranges(dst.L, layers_per_launch)]
        evs = [native.NativeEvent() for _ in ends]
        kw = {} if post is None else {"post": post.struct(*post.window(dst, dst_tok0, n, chunk_tokens))}
        if heads is not None:
            kw["heads"] = heads
        schedule(table.data_ptr(), bound, n, dst, dst_tok0, chunk_tokens, ends, evs, stream=cur.cuda_stream, status_ptr=st_ptr, **kw)
        return list(zip(ends, evs))

    @staticmethod
    def _range_events(L: int, step: int):
        """An event per range of `step` layers for the loads that record them in ONE C-ABI call
        -> ([(first layer after the range, event)], the ctypes array of their handles)."""
        events = [(l1, native.NativeEvent()) for _, l1 in layer_ranges(L, step)]
        return events, (ctypes.c_void_p * len(events))(*[ev.handle for _, ev in events])

    def decode_host_layerwise(self, host_blobs: Sequence["HostBlob"], dst: native.KVLayout, dst_tok0: int,
                              chunk_tokens: int, layers_per_range) -> Optional[DecodeJob]:
        """Blobs in pinned host DRAM -> decoded KV, cut by layers through ONE C-ABI call (lmc_load_chunks): a gather
        kernel pulls the bytes of a range of layers over PCIe while the previous range is decoded, an event per
        range (DecodeJob.layer_events) lets the model start on layer 0 after 1/L of the transfer -- where decode()
        moves whole chunks first (the first layer is complete when the last chunk has landed).
        layers_per_range: see range_step (a schedule is not supported by the single call: its first entry is used)."""
        n = len(host_blobs)
        if n == 0:
            return None
        step = range_step(dst.L, layers_per_range)
        with self._lock, torch.cuda.device(self.device):
            cur = torch.cuda.current_stream(self.device)
            loans = []
            with self._launch(cur, loans) as (st, st_ptr):
                # (the kernels read the arrays: back in the pool at finish)
                meta = _borrow(loans, self._meta_pool, 12 * n, 12 * max(n, 256))
                meta.tensor[:8 * n].view(torch.int64).copy_(torch.tensor([hb.ptr for hb in host_blobs], dtype=torch.int64))
                meta.tensor[8 * n:12 * n].view(torch.int32).copy_(torch.tensor([hb.nbytes for hb in host_blobs], dtype=torch.int32))
                events, handles = self._range_events(dst.L, step)
                self.ctx.load_chunks(meta.ptr, meta.ptr + 8 * n, n, dst, dst_tok0, chunk_tokens, step,
                                     ctypes.cast(handles, ctypes.c_void_p).value, stream=cur.cuda_stream, status_ptr=st_ptr)
            return DecodeJob(events[-1][1], events, status_idx=st, pool=self._status, loans=loans)

    def decode_host_post(self, host_blobs: Sequence["HostBlob"], dst: native.KVLayout, dst_tok0: int, chunk_tokens: int,
                         layers_per_launch, post: native.RangePost) -> Optional[DecodeJob]:
        """Blobs in pinned host DRAM that are no pack (a store of a single chunk, LMCACHE_AMD_PINNED_PACKS=0) with a
        post-op: lmc_load_chunks has no post-op, so the blobs cross PCIe whole into the decode slots, as decode() moves
        them, and ONE lmc_decode_chunks_schedule_post over the slots decodes them range by range with `post` in front
        of every range's event (_run_schedule: the step decode_device takes for blobs that live in HBM)."""
        n = len(host_blobs)
        if n == 0:
            return None
        stride = native.r16(max(hb.nbytes for hb in host_blobs))
        with self._lock, torch.cuda.device(self.device):
            cur = torch.cuda.current_stream(self.device)
            arena = self._dec_slots(n, stride, cur)
            with self._launch(cur) as (st, st_ptr):
                if self._dec_free is not None:
                    self.copy_stream.wait_event(self._dec_free)  # previous decode has read the slots
                for i, hb in enumerate(host_blobs):
                    native.memcpy_async(arena.data_ptr() + i * stride, hb.ptr, hb.nbytes, "h2d", self.copy_stream.cuda_stream)
                ready = torch.cuda.Event()
                ready.record(self.copy_stream)
                cur.wait_event(ready)
                table = torch.tensor([arena.data_ptr() + i * stride for i in range(n)],
                                     dtype=torch.int64).pin_memory().to(self.device, non_blocking=True)
                events = self._run_schedule(self.ctx.decode_chunks_schedule_post, table, stride, n, dst, dst_tok0, chunk_tokens,
                                            layers_per_launch, post, cur, st_ptr)
                last = torch.cuda.Event()
                last.record(cur)
                self._dec_free = last
            return DecodeJob(events[-1][1], events, table, status_idx=st, pool=self._status)

    # ---- packs: the plane-major pinned tier ---------------------------------------------------------------
    def store_pack(self, src: native.KVLayout, tok_begin: int, tok_end: int, chunk_tokens: int, bins: Sequence[int],
                   arena: PinnedArena, direct: bool = False) -> PackJob:
        """lmc_store_pack_parts on the CURRENT stream: encode every chunk of [tok_begin, tok_end), then a copy kernel writes
        the blobs transposed (static sections, then streams ordered layer / K,V / chunk) into one region.  No host
        wait here; finish_pack() returns the pack in pinned host DRAM (`arena` is taken there, not here).
        The region is in HBM and finish_pack() moves the pack with copies of its exact size -- the copy kernel then runs
        at HBM speed (0.3 ms) and the PCIe leg disturbs nobody (a copy kernel whose own stores crossed PCIe made the
        kernels beside its 11 ms 4.3x slower: bench.py store_hidden).
        direct: see _readable; a split source is coded by the two kernels, so its pack leaves as ONE part."""
        src, tok_begin, tok_end = self._readable(src, tok_begin, tok_end, direct)
        L, H, D = src.L, src.H, src.D
        n, _ = self._job_size(src, tok_begin, tok_end, chunk_tokens)
        with self._lock, torch.cuda.device(self.device):
            cap = pack_cap(n, L, chunk_tokens, H, D, bins)
            cur = torch.cuda.current_stream(self.device)
            # (a weak reference: a job dropped unfinished -- an exception between store_pack and finish_pack -- has
            # waited for its kernels in __del__ and queued no copy, so the region is free again; a strong one would keep
            # such a job, and with it every later store on regions of their own, for the life of the codec)
            prev = self._pack_prev() if self._pack_prev is not None else None
            if prev is None or prev.d2h_issued:
                if self._pack_dev is None or self._pack_dev.numel() < cap:
                    self._pack_dev = torch.empty(cap, dtype=torch.uint8, device=self.device)
                dev = self._pack_dev
                if self._pack_dev_free is not None:
                    cur.wait_event(self._pack_dev_free)  # the previous pack has left the buffer
            else:
                dev = torch.empty(cap, dtype=torch.uint8, device=self.device)  # the previous store has not been finished yet
            loans = []
            with self._launch(cur, loans) as (st, st_ptr):
                sizes = _borrow(loans, self._size_pool, 4 * n, 4 * max(n, 256))
                # the encode in plane ranges, each packed as soon as it is coded (lmc_store_pack_parts): finish_pack
                # sends a range over PCIe while the later planes are still being encoded
                nparts = self.pack_parts if n * 2 * L >= 16 * self.pack_parts else 1
                part_events = [native.NativeEvent() for _ in range(nparts)]
                part_info = _borrow(loans, self._part_info_pool, 16 * 16, 16 * 16)
                self.ctx.store_pack_parts(src, tok_begin, tok_end, chunk_tokens, bins, dev.data_ptr(), cap, sizes.ptr,
                                          nparts, part_info.ptr, part_events, stream=cur.cuda_stream, status_ptr=st_ptr)
                done = torch.cuda.Event()
                done.record(cur)
            job = PackJob(n, chunk_tokens, (L, H, D), dev, cap, sizes, part_info, part_events,
                          done=done, status_idx=st, pool=self._status, loans=loans)
            if dev is self._pack_dev:
                self._pack_prev = weakref.ref(job)
            return job

    def pack_bytes(self, job: PackJob) -> int:
        """Wait for the store's last part and -> the size of its pack from the part words (0: the parts say it failed;
        finish_pack reads the verdict)."""
        off_streams = native.pack_off_streams(job.nchunks, job.geometry[0], job.chunk_tokens, job.geometry[1], job.geometry[2])
        job.part_events[-1].synchronize()
        info = job.part_info.tensor.view(torch.int64)
        total = 0
        for r in range(len(job.part_events)):
            off, nbytes = int(info[2 * r]), int(info[2 * r + 1])
            if nbytes > 0:
                total = off_streams + off + nbytes
        return total if total <= job.cap else 0

    def finish_pack(self, job: PackJob, arena: PinnedArena) -> HostPack:
        """Wait for THIS store (its events), raise NativeError if a kernel flagged it, return the pack in pinned host DRAM."""
        # The pack is being built in HBM part by part.  Part r leaves as soon as its event has fired -- the host waits
        # for that event only, reads where the part lies (two pinned words the GPU wrote) and queues ONE DMA copy, on
        # alternating copy streams (two DMA queues) -- while the later plane ranges are still being encoded; behind the
        # last part the static sections (header, offset table, static slots) follow.  The pinned region is taken at the
        # pack's upper bound and cut to its size afterwards.
        off_streams = native.pack_off_streams(job.nchunks, job.geometry[0], job.chunk_tokens, job.geometry[1], job.geometry[2])
        streams = [self.copy_stream, self.copy_stream2]
        # A BOUNDED arena is asked for the bound too, while it has room for it: the budget is tested against the bound here
        # and corrected by the cut below (shrink frees the tail).  When it has not -- an arena kept full by its budget is
        # the steady state -- it is asked for the pack's exact size instead, which the last part's words give: a hole of
        # the bound would evict groups for room the pack never uses.  The parts then leave behind the whole encode: that
        # store loses the overlap of its DMA with its encode.  (ArenaFull from here: nothing has been done to the job yet,
        # the caller makes room and calls again, or drops the job.)
        try:
            region = arena.alloc(job.cap, slab_hint=min(4 * job.cap, 4 << 30), streams=streams)
        except ArenaFull:
            region = arena.alloc(max(self.pack_bytes(job), off_streams), streams=streams)
        info = job.part_info.tensor.view(torch.int64)
        total, failed = off_streams, False
        with torch.cuda.device(self.device):
            for r, ev in enumerate(job.part_events):
                ev.synchronize()  # this part only
                off, nbytes = int(info[2 * r]), int(info[2 * r + 1])
                if nbytes <= 0:
                    # no bytes is no verdict: a first range of a single plane ships nothing (a part packs the planes coded
                    # so far but the newest one), the parts behind the only one of an unsplit job are empty by design, and
                    # a part that failed reads the same -- the job's status word and the check of the assembled pack decide
                    continue
                if off_streams + off + nbytes > min(job.cap, native.r16(max(region.nbytes, 16))):
                    failed = True
                    break
                native.memcpy_async(region.ptr + off_streams + off, job.dev.data_ptr() + off_streams + off, nbytes, "d2h",
                                    streams[r % 2].cuda_stream)
                total = off_streams + off + nbytes
            # (the last part's event has fired: every kernel of the store is done, every part's words have been read)
            with self._lock:
                st = job.retire()
                if st == 0 and not failed:
                    native.memcpy_async(region.ptr, job.dev.data_ptr(), off_streams, "d2h", streams[0].cuda_stream)
                evd = self._join_copy_streams()
                job.d2h_issued = True  # (whatever the status: the HBM region may be reused behind evd)
                if job.dev is self._pack_dev:
                    self._pack_dev_free = evd
            evd.synchronize()
        if st or failed:
            arena.shrink(region, 0)
            raise native.NativeError("CacheGen store (pack): " + (native.describe_status(st) if st else "the device left no pack"))
        try:
            h = native.pack_info(region.ptr, total)  # the pack checks out where it lies now
            if int(h.total_bytes) != total:
                raise native.NativeError("CacheGen store (pack): the parts do not add up to the pack")
        except native.NativeError:
            arena.shrink(region, 0)
            raise
        return HostPack(arena.shrink(region, total), job.nchunks, job.chunk_tokens)

    def load_pack(self, pack: HostPack, chunk_begin: int, nchunks: int, dst: native.KVLayout, dst_tok0: int,
                  layers_per_range, post: Optional[native.RangePost] = None) -> DecodeJob:
        """Chunks [chunk_begin, chunk_begin + nchunks) of a pack -> decoded KV through ONE C-ABI call (lmc_load_pack): the streams of a
        range of layers are one contiguous transfer, the range's decode follows it, an event per range
        (DecodeJob.layer_events) lets the model run layer 0 while the later ranges are still crossing PCIe.
        layers_per_range: see range_step.  post: a native.RangePost done to every range between its decode and its event
        (lmc_load_pack_post)."""
        step = range_step(dst.L, layers_per_range)
        with self._lock, torch.cuda.device(self.device):
            cur = torch.cuda.current_stream(self.device)
            with self._launch(cur) as (st, st_ptr):
                events, handles = self._range_events(dst.L, step)
                if post is None:
                    self.ctx.load_pack(pack.blob.ptr, pack.blob.nbytes, chunk_begin, nchunks, dst, dst_tok0, step,
                                       ctypes.cast(handles, ctypes.c_void_p).value, stream=cur.cuda_stream, status_ptr=st_ptr)
                else:
                    n = nchunks or pack.nchunks - chunk_begin
                    self.ctx.load_pack_post(pack.blob.ptr, pack.blob.nbytes, chunk_begin, nchunks, dst, dst_tok0, step,
                                            ctypes.cast(handles, ctypes.c_void_p).value,
                                            post.struct(*post.window(dst, dst_tok0, n, pack.chunk_tokens)),
                                            stream=cur.cuda_stream, status_ptr=st_ptr)
            return DecodeJob(events[-1][1], events, status_idx=st, pool=self._status)

    # ---- bounded tiers: HBM blobs <-> pinned pack, no re-encode ---------------------------------------------------------
    def transcode_fixed(self, blobs: Sequence[torch.Tensor], geometry: tuple, chunk_tokens: int, ntokens: int,
                        bins: Sequence[int], ready: Sequence = ()) -> List[torch.Tensor]:
        """Fixed-width HBM blobs of one store group (exact-size uint8 tensors, anywhere) -> the entropy-coded blobs
        encode() would have written from the same KV (lmc_transcode_fixed), as exact-size views of the codec's transcode
        staging: a transient HBM region at blob_bound stride, codec-owned, grown on demand and OUTSIDE every tier's
        budget (it holds a group only while that group is on its way out of HBM).  The views are good until the next
        transcode_fixed; the caller holds the codec's lock across their use (demote_blobs does).  Blocks until the sizes
        are there; NativeError if the job's status word is set -- a fixed blob that does not check out."""
        L, H, D = geometry
        n = len(blobs)
        stride = native.r16(native.blob_bound(L, chunk_tokens, H, D))
        with self._lock, torch.cuda.device(self.device):
            cur = torch.cuda.current_stream(self.device)
            if self._xcode_dev is None or self._xcode_dev.numel() < n * stride:
                cur.synchronize()  # (whoever read the views of the region that goes)
                self._xcode_dev = None
                self._xcode_dev = torch.empty(n * stride, dtype=torch.uint8, device=self.device)
            out = self._xcode_dev
            _stream_waits(cur, ready)
            # the stored KV's dtype is the blobs' own header word (a group is one store: one dtype)
            dtype = int(blobs[0][8:12].view(torch.int32).item())
            words = [b.data_ptr() for b in blobs]
            room = [b.numel() for b in blobs]
            words += [room[i] | (room[i + 1] << 32 if i + 1 < n else 0) for i in range(0, n, 2)]  # uint32 pairs
            table = torch.tensor(words, dtype=torch.int64).pin_memory().to(self.device, non_blocking=True)
            loans = []
            with self._launch(cur, loans) as (st, st_ptr):
                sizes = _borrow(loans, self._size_pool, 4 * n, 4 * max(n, 256))
                self.ctx.transcode_fixed(table.data_ptr(), table.data_ptr() + 8 * n, n, L, H, D, dtype, chunk_tokens, ntokens,
                                         bins, out.data_ptr(), stride, sizes.ptr, self.device, stream=cur.cuda_stream,
                                         status_ptr=st_ptr)
                done = torch.cuda.Event()
                done.record(cur)
            job = Job(done, status_idx=st, pool=self._status, loans=loans)
            done.synchronize()
            got = sizes.tensor[:4 * n].view(torch.int32).tolist()  # before the words go back
            _raise_on(job.retire(), "CacheGen demotion (lmc_transcode_fixed)")
            if any(nb <= 0 or nb > stride for nb in got):
                raise native.NativeError("CacheGen demotion (lmc_transcode_fixed): a chunk was not coded")
            return [out[i * stride:i * stride + nb] for i, nb in enumerate(got)]

    def demote_blobs(self, blobs: Sequence[torch.Tensor], geometry: tuple, chunk_tokens: int, ntokens: int,
                     arena: PinnedArena, ready: Sequence = (), model: Optional[str] = None,
                     bins: Optional[Sequence[int]] = None) -> HostPack:
        """The demotion leg: the HBM blobs of one store group (exact-size uint8 tensors, anywhere) -> one pack in pinned
        host DRAM, byte for byte the pack store_pack would have written.  lmc_pack_blobs repacks them on the GPU into the
        HBM pack staging, two DMA copies move the pack into a region of `arena` taken at its exact size (the blobs'
        sizes say what it is), and lmc_pack_info checks it where it landed.  Blocks until the pack is there (a worker's
        call, or set_capacity's); raises NativeError -- nothing kept -- if the job's status word or the check says no,
        ArenaFull if `arena` has no room.  ready: events behind the writes of the blobs.
        model "fixed" (with the planes' `bins`): the blobs are LMC_MODEL_FIXED and are transcoded first (transcode_fixed:
        into the codec's transient HBM staging, which no budget counts); the coded blobs' sizes are read, and from there
        the leg is the same leg -- the pack holds entropy-coded streams, whichever model the HBM tier keeps."""
        if model not in self._DEMOTERS:
            raise ValueError(f"unknown coder model {model!r} (None or 'fixed')")
        first = self._DEMOTERS[model]
        with self._lock:  # (re-entrant: the staging's views stay the group's until the pack has left)
            if first is not None:
                blobs, ready = getattr(self, first)(blobs, geometry, chunk_tokens, ntokens, bins, ready), ()
            return self._pack_out(blobs, geometry, chunk_tokens, ntokens, arena, ready)

    def _pack_out(self, blobs: Sequence[torch.Tensor], geometry: tuple, chunk_tokens: int, ntokens: int,
                  arena: PinnedArena, ready: Sequence = ()) -> HostPack:
        """demote_blobs behind its model: entropy-coded blobs -> the pack in `arena`."""
        L, H, D = geometry
        n = len(blobs)
        total = self.demoted_bytes([b.numel() for b in blobs], geometry, chunk_tokens, ntokens)
        with self._lock, torch.cuda.device(self.device):
            cur = torch.cuda.current_stream(self.device)
            streams = [self.copy_stream, self.copy_stream2]
            region = arena.alloc(total, streams=streams)
            try:
                prev = self._pack_prev() if self._pack_prev is not None else None
                shared = prev is None or prev.d2h_issued
                if shared:
                    if self._pack_dev is None or self._pack_dev.numel() < total:
                        self._pack_dev = torch.empty(total, dtype=torch.uint8, device=self.device)
                    dev = self._pack_dev
                    if self._pack_dev_free is not None:
                        cur.wait_event(self._pack_dev_free)  # the previous pack has left the buffer
                else:
                    dev = torch.empty(total, dtype=torch.uint8, device=self.device)  # a store has not been finished yet
                _stream_waits(cur, ready)
                # the blobs' addresses and room in DEVICE memory (the scan reads them dozens of times per thread): one
                # stream-ordered upload from pinned memory of torch's caching host allocator, as decode_device's table
                words = [b.data_ptr() for b in blobs]
                sizes = [b.numel() for b in blobs]
                words += [sizes[i] | (sizes[i + 1] << 32 if i + 1 < n else 0) for i in range(0, n, 2)]  # uint32 pairs
                table = torch.tensor(words, dtype=torch.int64).pin_memory().to(self.device, non_blocking=True)
                with self._launch(cur) as (st, st_ptr):
                    self.ctx.pack_blobs(table.data_ptr(), table.data_ptr() + 8 * n, n, L, H, D, chunk_tokens, ntokens,
                                        dev.data_ptr(), total, self.device, stream=cur.cuda_stream, status_ptr=st_ptr)
                    done = torch.cuda.Event()
                    done.record(cur)
                job = Job(done, status_idx=st, pool=self._status)
                half = (total // 2) & ~15
                for q, (lo, hi) in enumerate(((0, half), (half, total))):
                    streams[q].wait_event(done)
                    if hi > lo:
                        native.memcpy_async(region.ptr + lo, dev.data_ptr() + lo, hi - lo, "d2h", streams[q].cuda_stream)
                evd = self._join_copy_streams()
                if shared:
                    self._pack_dev_free = evd
                evd.synchronize()
                _raise_on(job.retire(), "CacheGen demotion (lmc_pack_blobs)")
                h = native.pack_info(region.ptr, total)  # only a pack that checks out where it lies is published
                if int(h.total_bytes) != total or int(h.nchunks) != n:
                    raise native.NativeError("CacheGen demotion: the pack is not the size its blobs add up to")
            except BaseException:
                arena.free(region)
                raise
        return HostPack(region, n, chunk_tokens)

    @staticmethod
    def demoted_bytes(blob_sizes: Sequence[int], geometry: tuple, chunk_tokens: int, ntokens: int) -> int:
        """Exact size of the pack demote_blobs writes for blobs of these sizes: header, table and static slots, and every
        blob's streams section."""
        L, H, D = geometry
        n = len(blob_sizes)
        total = native.pack_off_streams(n, L, chunk_tokens, H, D)
        for i, nb in enumerate(blob_sizes):
            T = chunk_tokens if i < n - 1 else ntokens - (n - 1) * chunk_tokens
            total += nb - native.blob_static_bytes(L, T, H, D)
        return total

    def transcode_to_fixed(self, blobs: Sequence[torch.Tensor], geometry: tuple, chunk_tokens: int, ntokens: int,
                           bins: Sequence[int], outs: Sequence[torch.Tensor], ready: Sequence = ()) -> None:
        """transcode_fixed's inverse: the entropy-coded blobs of one store group (uint8 tensors, anywhere in HBM) -> the
        fixed-width blobs encode(model="fixed") would have written from the same KV (lmc_transcode_to_fixed: one launch
        of the rANS decoder with its fixed-width sink, no workspace), chunk i into outs[i] -- a uint8 tensor of at least
        native.fixed_blob_bytes of that chunk's length, 16-byte aligned, anywhere.  Blocks until the blobs are there;
        NativeError if the job's status word is set -- a coded blob that does not check out; outs then hold nothing."""
        L, H, D = geometry
        n = len(blobs)
        assert len(outs) == n
        with self._lock, torch.cuda.device(self.device):
            cur = torch.cuda.current_stream(self.device)
            _stream_waits(cur, ready)
            # the stored KV's dtype is the blobs' own header word (a group is one store: one dtype)
            dtype = int(blobs[0][8:12].view(torch.int32).item())

            def pairs(v):  # uint32 pairs in int64 words
                return [v[i] | (v[i + 1] << 32 if i + 1 < n else 0) for i in range(0, n, 2)]
            h = (n + 1) // 2
            words = [b.data_ptr() for b in blobs] + [o.data_ptr() for o in outs]
            words += pairs([b.numel() for b in blobs]) + pairs([o.numel() for o in outs])
            table = torch.tensor(words, dtype=torch.int64).pin_memory().to(self.device, non_blocking=True)
            base = table.data_ptr()
            with self._launch(cur) as (st, st_ptr):
                self.ctx.transcode_to_fixed(base, base + 16 * n, n, L, H, D, dtype, chunk_tokens, ntokens, bins,
                                            base + 8 * n, base + 16 * n + 8 * h, self.device, stream=cur.cuda_stream,
                                            status_ptr=st_ptr)
                done = torch.cuda.Event()
                done.record(cur)
            job = Job(done, status_idx=st, pool=self._status)
            done.synchronize()
            _raise_on(job.retire(), "CacheGen promotion (lmc_transcode_to_fixed)")

    def promote_pack(self, pack: HostPack, arena: "DeviceArena", model: Optional[str] = None,
                     bins: Optional[Sequence[int]] = None) -> List[torch.Tensor]:
        """The promotion leg: every chunk of a pack in pinned host DRAM -> the blob it was made of, each in a region of
        its own size in the HBM arena (lmc_unpack_blobs: DMA into the context's load staging, one kernel that scatters
        static slots and segments).  Blocks until the blobs are there; NativeError (nothing kept) if the job's status
        word says no, ArenaFull if `arena` has no room.
        model "fixed" (with the planes' `bins`): the HBM tier keeps LMC_MODEL_FIXED blobs.  The pack is unpacked into the
        codec's transient HBM staging instead (transcode_fixed's, in the other direction: no budget counts it, it is
        grown on demand and held under the codec's lock), the arena's regions are taken at native.fixed_blob_bytes per
        chunk -- the last one may be shorter -- and transcode_to_fixed writes the fixed-width blobs into them."""
        if model not in self._PROMOTERS:
            raise ValueError(f"unknown coder model {model!r} (None or 'fixed')")
        last = self._PROMOTERS[model]
        n = pack.nchunks
        sizes = [native.pack_chunk_bytes(pack.blob.ptr, pack.blob.nbytes, i) for i in range(n)]
        out: List[torch.Tensor] = []
        with self._lock, torch.cuda.device(self.device):
            cur = torch.cuda.current_stream(self.device)
            try:
                if last is None:
                    dst = out
                    for nb in sizes:
                        out.append(arena.alloc(nb, stream=cur))
                else:
                    h = native.pack_info(pack.blob.ptr, pack.blob.nbytes)
                    L, H, D, ntokens = int(h.num_layers), int(h.num_heads), int(h.head_size), int(h.ntokens)
                    geometry = (L, H, D)
                    offs = [0]
                    for nb in sizes:
                        offs.append(offs[-1] + native.r16(nb))
                    if self._xcode_dev is None or self._xcode_dev.numel() < offs[-1]:
                        cur.synchronize()  # (whoever read the views of the region that goes)
                        self._xcode_dev = None
                        self._xcode_dev = torch.empty(offs[-1], dtype=torch.uint8, device=self.device)
                    dst = [self._xcode_dev[offs[i]:offs[i] + nb] for i, nb in enumerate(sizes)]
                    for i in range(n):
                        T = pack.chunk_tokens if i < n - 1 else ntokens - (n - 1) * pack.chunk_tokens
                        out.append(arena.alloc(native.fixed_blob_bytes(L, T, H, D, bins), stream=cur))
                with self._launch(cur) as (st, st_ptr):
                    self.ctx.unpack_blobs(pack.blob.ptr, pack.blob.nbytes, 0, n, [t.data_ptr() for t in dst], sizes,
                                          self.device, stream=cur.cuda_stream, status_ptr=st_ptr)
                    done = torch.cuda.Event()
                    done.record(cur)
                job = Job(done, status_idx=st, pool=self._status)
                done.synchronize()
                _raise_on(job.retire(), "CacheGen promotion (lmc_unpack_blobs)")
                if last is not None:
                    getattr(self, last)(dst, geometry, pack.chunk_tokens, ntokens, bins, out)
            except BaseException:
                ev = torch.cuda.Event()
                ev.record(cur)
                for t in out:
                    arena.free(t, [ev])
                raise
        return out

    def _dec_slots(self, n: int, stride: int, cur) -> torch.Tensor:
        if self._dec_arena is None or self._dec_arena.numel() < n * stride:
            self._dec_arena = torch.empty(n * stride, dtype=torch.uint8, device=self.device)
            # the caching allocator may hand out a block whose previous owner still has kernels queued on the
            # current stream: the side-stream copies into it must not start before those
            self.copy_stream.wait_stream(cur)
        return self._dec_arena

    def decode(self, host_blobs: Sequence, dst: native.KVLayout, dst_tok0: int, chunk_tokens: int,
               batch_chunks: Optional[int] = None, heads: Optional[native.HeadWindow] = None) -> Optional[DecodeJob]:
        """H2D the blobs on the side stream and decode them on the current stream straight into `dst`,
        pipelined in batches of `decode_batch_chunks` (copy of batch b+1 overlaps the decode of batch b).
        host_blobs: HostBlob (pinned), bytes-like (staged through pinned memory) or uint8 CUDA tensors (blobs
        that are already in HBM: copied device to device).
        heads: a native.HeadWindow (see decode_device): the blobs cross whole, and every batch is decoded through the
        pointer-table call lmc_decode_chunks_heads_schedule with one range of all layers.
        Asynchronous: returns a DecodeJob; finish_decode(job) waits for it and raises on a corrupt blob."""
        n = len(host_blobs)
        if n == 0:
            return None
        def _is_dev(b):
            return isinstance(b, torch.Tensor) and b.is_cuda

        sizes = [hb.nbytes if isinstance(hb, HostBlob) else (hb.numel() if _is_dev(hb) else len(hb)) for hb in host_blobs]
        stride = native.r16(max(sizes))
        with self._lock:
            with torch.cuda.device(self.device):
                cur = torch.cuda.current_stream(self.device)
                arena = self._dec_slots(n, stride, cur)
                with self._launch(cur) as (st, st_ptr):
                    if self._dec_free is not None:
                        self.copy_stream.wait_event(self._dec_free)  # previous decode has read the slots
                    cs = self.copy_stream.cuda_stream
                    staged_off = 0
                    pageable = [hb for hb in host_blobs if not isinstance(hb, HostBlob) and not _is_dev(hb)]
                    if pageable:
                        need = sum(native.r16(len(b)) for b in pageable)
                        if self._stage is None or self._stage.nbytes < need:
                            self.copy_stream.synchronize()
                            self._stage = native.PinnedBuffer(need)
                        else:
                            self.copy_stream.synchronize()  # staging buffer is reused: earlier H2D must be done
                    # H2D and decode are pipelined in batches: the copy stream runs ahead, the compute stream
                    # decodes batch b as soon as its blobs have landed (one event per batch)
                    B = batch_chunks or self.decode_batch_chunks
                    last = None
                    table, table_at = None, {}
                    if dst.struct.paged_kind == native.PAGED_SPLIT or heads is not None:
                        # lmc_decode_chunks stands for from_bytes and writes rows only (include/lmc_hip.h): an "NHDB"
                        # cache takes the same slots through a pointer table -- ONE for all n slots, made before the
                        # first batch and uploaded stream-ordered from pinned memory (no host wait, as decode_device's table);
                        # batch b reads its part of it; the job keeps it until it is finished
                        # (a batch's part starts on a 16-byte boundary, as the call asks of its table: an odd batch is padded)
                        ptrs = []
                        for b0 in range(0, n, B):
                            table_at[b0] = len(ptrs)
                            ptrs += [arena.data_ptr() + i * stride for i in range(b0, min(n, b0 + B))]
                            ptrs += [0] * (len(ptrs) & 1)
                        table = torch.tensor(ptrs, dtype=torch.int64).pin_memory().to(self.device, non_blocking=True)
                    for b0 in range(0, n, B):
                        b1 = min(n, b0 + B)
                        for i in range(b0, b1):
                            hb = host_blobs[i]
                            if _is_dev(hb):
                                # a blob already in HBM (xgmi:// connector): a device copy on the decoding stream itself,
                                # ordered behind whatever produced the tensor
                                native.memcpy_async(arena.data_ptr() + i * stride, hb.data_ptr(), sizes[i], "d2d",
                                                    cur.cuda_stream)
                                continue
                            if isinstance(hb, HostBlob):
                                src_ptr = hb.ptr
                            else:
                                data = hb if isinstance(hb, bytes) else bytes(hb)  # never mutates the caller's buffer
                                ctypes.memmove(self._stage.ptr + staged_off, data, len(data))
                                src_ptr = self._stage.ptr + staged_off
                                staged_off += native.r16(len(data))
                            native.memcpy_async(arena.data_ptr() + i * stride, src_ptr, sizes[i], "h2d", cs)
                        ready = torch.cuda.Event()
                        ready.record(self.copy_stream)
                        cur.wait_event(ready)
                        if heads is not None:
                            self.ctx.decode_chunks_heads_schedule(table.data_ptr() + 8 * table_at[b0], stride, b1 - b0, dst,
                                                                  dst_tok0 + b0 * chunk_tokens, chunk_tokens, [dst.L], None,
                                                                  heads, stream=cur.cuda_stream, status_ptr=st_ptr)
                        elif table is not None:
                            self.ctx.decode_chunks_layers(table.data_ptr() + 8 * table_at[b0], stride, b1 - b0, dst,
                                                          dst_tok0 + b0 * chunk_tokens, chunk_tokens, 0, dst.L,
                                                          stream=cur.cuda_stream, status_ptr=st_ptr)
                        else:
                            self.ctx.decode_chunks(arena.data_ptr() + b0 * stride, stride, b1 - b0, dst,
                                                   dst_tok0 + b0 * chunk_tokens, chunk_tokens, stream=cur.cuda_stream,
                                                   status_ptr=st_ptr)
                        last = torch.cuda.Event()
                        last.record(cur)
                    self._dec_free = last
                return DecodeJob(last, table=table, status_idx=st, pool=self._status)

    def finish_decode(self, job: Optional[DecodeJob], what: str = "CacheGen decode") -> None:
        """Wait for THIS decode (its event, not the device) and raise NativeError if a kernel flagged its blobs
        (bad header / directory / stream): the destination then holds garbage and must not be used."""
        if job is None:
            return
        job.done.synchronize()
        _raise_on(job.retire(), what)

    def close(self):
        """Return every pinned buffer the codec owns (its jobs must have been finished) and drop its device memory."""
        with self._lock:
            for words in (self._size_pool, self._meta_pool, self._part_info_pool, self._status):
                words.close()
            if self._stage is not None:
                self._stage.free()
                self._stage = None
            self._enc_arena = self._dec_arena = self._pack_dev = self._xcode_dev = None
            self._table_cache, self._same_blobs = {}, {}


_codecs = {}
_codecs_lock = threading.Lock()


def get_codec(device: Optional[int] = None) -> CacheGenDeviceCodec:
    dev = torch.cuda.current_device() if device is None else int(device)
    with _codecs_lock:
        if dev not in _codecs:
            _codecs[dev] = CacheGenDeviceCodec(dev)
        return _codecs[dev]
