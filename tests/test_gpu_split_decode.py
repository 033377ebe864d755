"""The decoder writes vLLM's ROCm paged-attention cache ("NHDB", LMC_PAGED_SPLIT) itself: k_decode.h, DEC_PAGED_SPLIT.

The expected value is always the path that existed before: decode into a [L,2,T,H,D] chunk, then scatter that chunk into
a clone of the cache by torch indexing on the two views (tests/test_gpu_paged_split.py: _torch_scatter).  Everything is
bit-exact on integer views and the WHOLE cache is compared, so one stray byte anywhere fails.  Shapes are the smallest
at which each path of the kernel exists: L = 2, 70 tokens in chunks of 32 (two chunks of four 8-token blocks each, a
last chunk of 6 tokens that only the one-token loop decodes)."""
import ctypes

import pytest
import torch

from lmcache_amd import native
from lmcache_amd.cache_engine import LMCacheEngine
from lmcache_amd.rope import RopeShift
from tests.test_gpu_engine import dumb_metadata, generate_tokens, make_cfg
from tests.test_gpu_paged_split import _ibits, _mapping, _nblocks, _split_caches, _torch_scatter, _views

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
L, NTOK, CS = 2, 70, 32
BINS = [32, 16, 16, 32]  # planes K0 K1 V0 V1: a 32-bin plane (33-entry search, top == 8) beside a 16-bin one, in K and in V
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "e4m3": torch.float8_e4m3fn}
GEOMS = [(2, 128, 16), (1, 64, 8), (2, 64, 32), (1, 80, 16)]  # the last: a group of 16 live lanes, 10 or 5 granules
MAPPINGS = ["blocks", "offset5", "random", "broken", "unaligned"]
INVALID = -1


@pytest.fixture(scope="module")
def ctx():
    native.build()
    return native.get_context(0)


class _Blobs:
    """`ntok` tokens of random bf16 KV of geometry (H, D), encoded once in chunks of CS: the blobs on the device, their
    pointer table, their bytes, and -- per destination dtype and dst_tok0 -- what the decoder writes into a chunk."""

    def __init__(self, ctx, H, D, ntok):
        g = torch.Generator().manual_seed(100 * H + D + ntok)
        kv = (torch.rand((L, 2, ntok, H, D), generator=g) - 0.5).to(torch.bfloat16).to(DEV)
        self.ctx, self.H, self.D, self.ntok = ctx, H, D, ntok
        self.n = (ntok + CS - 1) // CS
        self.stride = native.r16(native.blob_bound(L, CS, H, D))
        self.dev = torch.zeros(self.n * self.stride, dtype=torch.uint8, device=DEV)
        sizes = torch.zeros(self.n, dtype=torch.int32, device=DEV)
        ctx.encode_chunks(native.KVLayout.from_chunk(kv, "vllm"), 0, ntok, CS, BINS, self.dev.data_ptr(), self.stride,
                          sizes.data_ptr())
        torch.cuda.synchronize()
        ctx.raise_on_status("encode")
        self.sizes = [int(s) for s in sizes.cpu()]
        self.table = torch.tensor([self.dev.data_ptr() + i * self.stride for i in range(self.n)], dtype=torch.int64).to(DEV)
        self._chunks = {}

    def bytes(self):
        host = self.dev.cpu().numpy()
        return [host[i * self.stride:i * self.stride + s].tobytes() for i, s in enumerate(self.sizes)]

    def chunk_bits(self, dt, tok0=0):
        """[L,2,ntok+tok0,H,D] integer view of the decode into a chunk with dst_tok0 = tok0 (<= 0): the expected values."""
        key = (dt, tok0)
        if key not in self._chunks:
            chunk = torch.zeros((L, 2, self.ntok + tok0, self.H, self.D), dtype=dt, device=DEV)
            self.ctx.decode_chunks(self.dev.data_ptr(), self.stride, self.n, native.KVLayout.from_chunk(chunk, "vllm"), tok0, CS)
            torch.cuda.synchronize()
            self.ctx.raise_on_status("decode into a chunk")
            self._chunks[key] = _ibits(chunk)
        return self._chunks[key]


@pytest.fixture(scope="module")
def blobs(ctx):
    made = {}

    def get(H, D, ntok=NTOK):
        if (H, D, ntok) not in made:
            made[(H, D, ntok)] = _Blobs(ctx, H, D, ntok)
        return made[(H, D, ntok)]
    return get


def _case(b, dt, bs, kind, g, ntok=None, tok0=0):
    """(caches, expected caches, layout, slots) for one mapping: the expectation is the chunk scattered by torch."""
    n = (b.ntok if ntok is None else ntok) + tok0
    nb = _nblocks(bs)
    caches = _split_caches(b.H, b.D, bs, dt, g, unaligned=kind == "unaligned", nblocks=nb)
    slots = _mapping(kind, n, nb, bs, g).to(DEV)
    expect = [c.clone() for c in caches]
    _torch_scatter(expect, b.chunk_bits(dt, tok0), slots, bs)
    return caches, expect, native.KVLayout.paged(caches, slots, bs, "NHDB"), slots


def _same(caches, expect, what):
    torch.cuda.synchronize()
    for l, (c, e) in enumerate(zip(caches, expect)):
        assert torch.equal(_ibits(c), _ibits(e)), f"{what}: layer {l}"


# ------------------------------------------------------------------ 1. C ABI against decode-then-torch-scatter
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "H%d_D%d_bs%d" % g)
@pytest.mark.parametrize("dt", list(DTYPES))
def test_decode_into_the_split_cache_equals_decode_then_scatter(ctx, blobs, dt, geom):
    """lmc_decode_chunks_layers with an LMC_PAGED_SPLIT destination.  The mappings cover the block path (`blocks`), runs
    that enter a block at an odd slot and off a multiple of eight (`offset5`: no wide V store, then the one-token loop
    where a run would leave its block), slots in any order (`random`: the one-token loop throughout), a run that breaks
    (`broken`) and a base 2 bytes off alignment (`unaligned`); the last chunk has 6 tokens."""
    H, D, bs = geom
    dt = DTYPES[dt]
    b = blobs(H, D)
    g = torch.Generator().manual_seed(7 * H + D + bs)
    for kind in MAPPINGS:
        caches, expect, split, _ = _case(b, dt, bs, kind, g)
        ctx.decode_chunks_layers(b.table.data_ptr(), b.stride, b.n, split, 0, CS, 0, L)
        _same(caches, expect, kind)
        ctx.raise_on_status(kind)


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("kind", ["blocks", "random"])
def test_first_chunk_trim_and_a_range_of_layers(ctx, blobs, dt, kind):
    """dst_tok0 = -5: the first five tokens are decoded and dropped, token 5 goes to the slot of destination token 0 (the
    trim moves the 8-token blocks off the chunk's start).  layer_begin = 1: layer 0's cache keeps every byte."""
    H, D, bs = 2, 128, 16
    dt = DTYPES[dt]
    b = blobs(H, D)
    g = torch.Generator().manual_seed(21)
    caches, expect, split, _ = _case(b, dt, bs, kind, g, tok0=-5)
    ctx.decode_chunks_layers(b.table.data_ptr(), b.stride, b.n, split, -5, CS, 0, L)
    _same(caches, expect, "trim")
    caches, expect, split, _ = _case(b, dt, bs, kind, g)
    expect[0] = caches[0].clone()
    ctx.decode_chunks_layers(b.table.data_ptr(), b.stride, b.n, split, 0, CS, 1, 1)
    _same(caches, expect, "layers [1, 2)")
    ctx.raise_on_status("trim / layer range")


# ------------------------------------------------------------------ 2. the other entry points
def _pinned(data: bytes):
    buf = native.PinnedBuffer(native.r16(len(data)))
    ctypes.memmove(buf.ptr, data, len(data))
    return buf


@pytest.mark.parametrize("dt", ["bf16", "e4m3"])
def test_schedule_load_chunks_and_load_pack_write_the_same_cache(ctx, blobs, oracle, dt):
    H, D, bs = 2, 64, 32
    dt = DTYPES[dt]
    b = blobs(H, D)
    g = torch.Generator().manual_seed(31)
    data = b.bytes()
    keep = [_pinned(x) for x in data]
    pack_bytes = oracle.pack_from_blobs(data, CS)
    pack = _pinned(pack_bytes)
    keep.append(pack)
    ptrs = (ctypes.c_void_p * b.n)(*[h.ptr for h in keep[:b.n]])
    sizes = (ctypes.c_uint32 * b.n)(*[len(x) for x in data])
    try:
        for kind in ("offset5", "blocks"):
            caches, expect, split, _ = _case(b, dt, bs, kind, g)
            ctx.decode_chunks_schedule(b.table.data_ptr(), b.stride, b.n, split, 0, CS, [1, L], None)  # two ranges
            _same(caches, expect, f"schedule {kind}")
            for step in (0, 1):
                caches, expect, split, _ = _case(b, dt, bs, kind, g)
                ctx.load_chunks(ctypes.cast(ptrs, ctypes.c_void_p).value, ctypes.cast(sizes, ctypes.c_void_p).value, b.n,
                                split, 0, CS, step)
                _same(caches, expect, f"load_chunks {kind} step {step}")
                caches, expect, split, _ = _case(b, dt, bs, kind, g)
                ctx.load_pack(pack.ptr, len(pack_bytes), 0, 0, split, 0, step)
                _same(caches, expect, f"load_pack {kind} step {step}")
        ctx.raise_on_status("entry points")
    finally:
        torch.cuda.synchronize()
        for h in keep:
            h.free()


def test_the_codec_decodes_host_blobs_into_a_split_cache(ctx, blobs):
    """CacheGenDevice.decode -- blobs with no pack and no HBM arena behind them (a remote backend's bytes) -- used to end in
    lmc_decode_chunks, which writes rows only: a split destination takes the pointer-table call instead."""
    from lmcache_amd.storage_backend.serde.cachegen_device import get_codec
    H, D, bs, dt = 2, 64, 32, torch.bfloat16
    b = blobs(H, D)
    codec = get_codec(0)
    for batch in (None, 1):  # one batch; a batch per chunk (each reads its own part of the job's pointer table)
        caches, expect, split, _ = _case(b, dt, bs, "offset5", torch.Generator().manual_seed(33))
        codec.finish_decode(codec.decode(b.bytes(), split, 0, CS, batch_chunks=batch))
        _same(caches, expect, f"codec.decode, batch_chunks={batch}")


# ------------------------------------------------------------------ 3. both coder models, both searches
def test_a_one_token_chunk_and_32_bin_planes(ctx, blobs, oracle):
    """65 tokens: the last chunk has ONE token and is coded with LMC_MODEL_CDF16, the others with the counts model; BINS
    holds 32-bin planes (top == 8) beside 16-bin ones (top == 4) in both halves."""
    H, D, bs = 2, 64, 32
    b = blobs(H, D, 65)
    heads = [oracle.parse_header(x) for x in b.bytes()]
    assert [h["ntokens"] for h in heads] == [32, 32, 1]
    assert [h["model"] for h in heads] == [oracle.MODEL_COUNTS, oracle.MODEL_COUNTS, oracle.MODEL_CDF16]
    assert {x for x in BINS if x - 1 <= 16} and {x for x in BINS if x - 1 > 16}
    g = torch.Generator().manual_seed(41)
    for dt in DTYPES.values():
        for kind in ("blocks", "offset5", "random"):
            caches, expect, split, _ = _case(b, dt, bs, kind, g)
            ctx.decode_chunks_layers(b.table.data_ptr(), b.stride, b.n, split, 0, CS, 0, L)
            _same(caches, expect, f"{dt} {kind}")
    ctx.raise_on_status("models")


# ------------------------------------------------------------------ 4. the guard on the 32-bit offsets
def test_a_head_stride_past_the_store_range_is_refused_by_all_four(ctx, blobs, oracle):
    """((H-1)*stride_head + D*bs)*E + 7*16 <= 0xfffffff0 (lmc_api.hip: decode_dst_ok).  The first stride_head behind the
    limit is LMC_ERR_INVALID from every entry point that takes a split destination, nothing is queued; a negative one
    too.  (The stride at the limit itself would need 4 GiB of cache behind it: the rule's arithmetic is held on the host,
    tests/test_split_decode_host.py, and nothing is decoded here into memory that does not exist.)"""
    H, D, bs, dt = 2, 64, 32, torch.bfloat16
    b = blobs(H, D)
    g = torch.Generator().manual_seed(51)
    caches = _split_caches(H, D, bs, dt, g, nblocks=_nblocks(bs))
    before = [c.clone() for c in caches]
    blobs_before = b.dev.clone()
    slots = _mapping("blocks", NTOK, _nblocks(bs), bs, g).to(DEV)
    split = native.KVLayout.paged(caches, slots, bs, "NHDB")
    lib, ref = native.lib(), ctypes.byref
    st = native.current_stream_ptr(torch.device(DEV))
    data = b.bytes()
    keep = [_pinned(x) for x in data]
    pack_bytes = oracle.pack_from_blobs(data, CS)
    keep.append(_pinned(pack_bytes))
    ptrs = (ctypes.c_void_p * b.n)(*[h.ptr for h in keep[:b.n]])
    sizes = (ctypes.c_uint32 * b.n)(*[len(x) for x in data])
    ends = (ctypes.c_int32 * 2)(1, L)
    calls = {
        "layers": lambda s: lib.lmc_decode_chunks_layers(ctx.handle, b.table.data_ptr(), b.stride, b.n, ref(s), 0, CS, 0, L, None, st),
        "schedule": lambda s: lib.lmc_decode_chunks_schedule(ctx.handle, b.table.data_ptr(), b.stride, b.n, ref(s), 0, CS, 2, ends,
                                                             None, None, st),
        "load_chunks": lambda s: lib.lmc_load_chunks(ctx.handle, ptrs, sizes, b.n, ref(s), 0, CS, 0, None, None, st),
        "load_pack": lambda s: lib.lmc_load_pack(ctx.handle, keep[-1].ptr, len(pack_bytes), 0, 0, ref(s), 0, 0, None, None, st),
    }
    try:
        E = 2
        limit = (0xfffffff0 - 112) // E - D * bs  # the largest (H-1)*stride_head, H = 2
        over = native.KvLayoutStruct.from_buffer_copy(split.struct)
        over.stride_head = limit + 1
        neg = native.KvLayoutStruct.from_buffer_copy(split.struct)
        neg.stride_head = -split.struct.stride_head
        for name, call in calls.items():
            assert call(over) == INVALID, f"{name}: first refused head stride"
            assert call(neg) == INVALID, f"{name}: negative head stride"
        # lmc_decode_chunks refuses a split destination whatever its strides
        assert lib.lmc_decode_chunks(ctx.handle, b.dev.data_ptr(), b.stride, b.n, ref(split.struct), 0, CS, None, st) == INVALID
        torch.cuda.synchronize()
        assert torch.equal(b.dev, blobs_before)
        for c, k in zip(caches, before):
            assert torch.equal(_ibits(c), _ibits(k))
        assert ctx.status(clear=True) == 0
    finally:
        torch.cuda.synchronize()
        for h in keep:
            h.free()


# ------------------------------------------------------------------ 5. the engine
class _Counting:
    def __init__(self, fn):
        self.fn, self.calls = fn, 0

    def __call__(self, *a, **k):
        self.calls += 1
        return self.fn(*a, **k)


@pytest.mark.parametrize("backend", ["cachegen-host", "cachegen-hbm", "cuda"])
def test_direct_retrieve_into_nhdb_equals_the_staged_one(backend, monkeypatch):
    """retrieve_into_paged(..., "NHDB", direct=True) and the default staged call into two clones of one cache: whole caches
    and masks are equal.  On the CacheGen tiers the direct call issues no lmc_copy_kv at all."""
    H, D, bs = 2, 128, 16
    dt, model = torch.bfloat16, "Llama-3-8B"
    nb = _nblocks(bs)
    g = torch.Generator().manual_seed(61)
    tokens = generate_tokens(NTOK, DEV)
    kv = tuple((torch.rand((NTOK, H, D), generator=g).to(dt).to(DEV), torch.rand((NTOK, H, D), generator=g).to(dt).to(DEV))
               for _ in range(L))
    ctx = native.get_context(0)
    engine = LMCacheEngine(make_cfg(backend, CS), dumb_metadata("vllm", model))
    try:
        engine.store(tokens, kv)
        if backend == "cachegen-hbm":
            assert engine.engine_.mode == "hbm-cachegen"

        def both(kind, mask, pair):
            cache = _split_caches(H, D, bs, dt, g, unaligned=kind == "unaligned", nblocks=nb)
            staged, before = [c.clone() for c in cache], [c.clone() for c in cache]
            slots = _mapping(kind, NTOK, nb, bs, g).to(DEV)
            into = (lambda cs_: [_views(c) for c in cs_]) if pair else (lambda cs_: cs_)
            ms = engine.retrieve_into_paged(tokens, into(staged), slots, bs, "NHDB", mask=mask)
            counter = _Counting(ctx.copy_kv)
            monkeypatch.setattr(ctx, "copy_kv", counter)
            md = engine.retrieve_into_paged(tokens, into(cache), slots, bs, "NHDB", mask=mask, direct=True)
            monkeypatch.undo()
            torch.cuda.synchronize()
            nskip = 0 if mask is None else int((~mask).sum())
            assert torch.equal(md, ms) and int(md.sum()) == NTOK - nskip
            if backend != "cuda":
                assert counter.calls == 0, "the direct retrieve of a CacheGen tier scatters nothing"
            for l in range(L):
                assert torch.equal(_ibits(cache[l]), _ibits(staged[l])), f"{kind} layer {l}"
            assert any(not torch.equal(_ibits(c), _ibits(o)) for c, o in zip(cache, before))  # something was retrieved

        both("blocks", None, False)
        both("random", None, True)
        mask = torch.ones(NTOK, dtype=torch.bool, device=DEV)
        mask[:37] = False  # a suffix mask that cuts into the second chunk: the first-chunk trim
        both("offset5", mask, False)
        both("blocks", mask, True)
        # unknown tokens: nothing written
        dst = _split_caches(H, D, bs, dt, g, nblocks=nb)
        keep = [c.clone() for c in dst]
        slots = _mapping("blocks", NTOK, nb, bs, g).to(DEV)
        m = engine.retrieve_into_paged(tokens + 10000, dst, slots, bs, "NHDB", direct=True)
        torch.cuda.synchronize()
        assert not m.any()
        # direct + rope: refused before anything is queued
        rope = RopeShift.from_base(10000.0, D, 128, DEV, delta=3)
        with pytest.raises(ValueError, match="direct"):
            engine.retrieve_into_paged(tokens, dst, slots, bs, "NHDB", rope=rope, direct=True)
        torch.cuda.synchronize()
        for c, k in zip(dst, keep):
            assert torch.equal(_ibits(c), _ibits(k))
        # a row layout takes the keyword and does what it did
        rows = [[torch.zeros((2, nb, bs, H, D), dtype=dt, device=DEV) for _ in range(L)] for _ in range(2)]
        m0 = engine.retrieve_into_paged(tokens, rows[0], slots, bs, "NBHD")
        m1 = engine.retrieve_into_paged(tokens, rows[1], slots, bs, "NBHD", direct=True)
        torch.cuda.synchronize()
        assert torch.equal(m0, m1) and all(torch.equal(a, c) for a, c in zip(*rows))
        assert ctx.status(clear=True) == 0
    finally:
        engine.close()


# ------------------------------------------------------------------ 6. a damaged chunk
def test_a_damaged_chunk_is_a_miss_and_only_the_calls_slots_may_change(oracle):
    """A byte flipped in a stream of the SECOND chunk's blob on the HBM tier.  The direct retrieve decodes into the live
    cache, so the slots of the call's tokens may hold garbage -- the price the docstring names -- but: no token of the
    damaged chunk or behind it is reported (what is reported is a prefix that ends at the first chunk at the latest; the
    engine's rule for a blob that does not decode is the one the row layouts have, and the mask is held against theirs),
    and every byte OUTSIDE the slots of the call's tokens is unchanged."""
    H, D, bs = 2, 128, 16
    dt, model = torch.bfloat16, "Llama-3-8B"
    nb = _nblocks(bs)
    g = torch.Generator().manual_seed(71)
    tokens = generate_tokens(NTOK, DEV)
    kv = tuple((torch.rand((NTOK, H, D), generator=g).to(dt).to(DEV), torch.rand((NTOK, H, D), generator=g).to(dt).to(DEV))
               for _ in range(L))
    engine = LMCacheEngine(make_cfg("cachegen-hbm", CS), dumb_metadata("vllm", model))
    try:
        engine.store(tokens, kv)
        keys = [engine._make_key(h, "vllm") for h in engine._prefix_hash(engine._chunk_tokens(tokens))]
        blob = engine.engine_.dict[keys[1]].blob
        head = oracle.parse_header(blob[:128].cpu().numpy().tobytes())
        where = head["off_streams"] + head["stream_bytes"] // 2
        assert where < blob.numel()
        blob[where] ^= 0x5A
        torch.cuda.synchronize()
        slots = _mapping("blocks", NTOK, nb, bs, g).to(DEV)
        rows = [torch.zeros((2, nb, bs, H, D), dtype=dt, device=DEV) for _ in range(L)]
        m_rows = engine.retrieve_into_paged(tokens, rows, slots, bs, "NBHD")
        cache = _split_caches(H, D, bs, dt, g, nblocks=nb)
        before = [c.clone() for c in cache]
        m = engine.retrieve_into_paged(tokens, cache, slots, bs, "NHDB", direct=True)
        torch.cuda.synchronize()
        assert not m[CS:].any() and torch.equal(m, m_rows)
        n = int(m.sum())
        assert not m[n:].any()  # a prefix
        # outside the slots of the call's tokens: put the old bytes back INTO those slots and the caches are equal
        blk, off = slots // bs, slots % bs
        for c, o in zip(cache, before):
            for cv, ov in zip(_views(c), _views(o)):
                if cv.dim() == 5:
                    _ibits(cv)[blk, :, :, off, :] = _ibits(ov)[blk, :, :, off, :]
                else:
                    _ibits(cv)[blk, :, :, off] = _ibits(ov)[blk, :, :, off]
            assert torch.equal(_ibits(c), _ibits(o))
        native.get_context(0).status(clear=True)
    finally:
        engine.close()
