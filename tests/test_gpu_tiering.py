"""Bounded local tiers on the GPU: lmc_pack_blobs / lmc_unpack_blobs against the CPU oracle (bytes, no tolerance), the
codec's demotion and promotion legs, and LMCLocalBackend's budgets, LRU eviction, demotion and promotion (torch.equal on
decoded KV)."""
import ctypes

import numpy as np
import pytest
import torch

from lmcache_amd import native
from lmcache_amd.cache_engine import LMCacheEngine
from lmcache_amd.storage_backend.serde.cachegen_device import CacheGenDeviceCodec, DeviceArena, PinnedArena
from tests.test_gpu_codec import _make, _oracle_blobs, _words_out
from tests.test_gpu_engine import MODEL, dumb_metadata, generate_kv_cache, make_cfg
from tests.test_gpu_fp8 import _bins

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CS = 32
ARENA_FULL, BAD_HEADER = 32, 2   # LMC_STATUS_HOST_ARENA_FULL, LMC_STATUS_BAD_HEADER

# (L, H, D, tokens, dtype): C = 128 is two full 64-channel groups, C = 72 a full and a partial one; 71 tokens are two
# full chunks and a ragged one of 7
CASES = {"c128": (2, 2, 64, 71, torch.bfloat16), "c72": (2, 1, 72, 71, torch.bfloat16),
         "fp8": (2, 2, 64, 71, torch.float8_e4m3fn), "one": (2, 2, 64, 32, torch.bfloat16),
         "five": (2, 2, 64, 160, torch.bfloat16)}


@pytest.fixture(scope="module")
def ctx():
    return native.get_context(0)


@pytest.fixture(scope="module")
def words():
    w = native.StatusWords()
    yield w
    torch.cuda.synchronize()
    w.close()


@pytest.fixture(scope="module")
def built(oracle, ctx):
    """Per case, computed once and never changed: the oracle's blobs and pack, and the HIP encoder's blobs -- each in a
    separate allocation, in SHUFFLED address order, the first two chunks taken from two different encode calls."""
    out = {}
    for seed, (name, (L, H, D, T, dt)) in enumerate(CASES.items()):
        g = torch.Generator().manual_seed(100 + seed)
        x = _make(L, T, H, D, dt, g)
        bins = _bins(L, g)
        ref = _oracle_blobs(oracle, x, CS, H, D, bins)
        n = len(ref)
        xd = x.reshape(L, 2, T, H, D).to(DEV)
        stride = native.r16(native.blob_bound(L, CS, H, D))
        arenas = []
        for _ in range(2):
            arena = torch.zeros(n * stride, dtype=torch.uint8, device=DEV)
            sizes = torch.zeros(n, dtype=torch.int32, device=DEV)
            ctx.encode_chunks(native.KVLayout.from_chunk(xd, "vllm"), 0, T, CS, bins, arena.data_ptr(), stride, sizes.data_ptr())
            torch.cuda.synchronize()
            ctx.raise_on_status(name)
            assert sizes.tolist() == [len(b) for b in ref]
            arenas.append(arena)
        # every blob in an allocation of its own; which allocation takes which chunk is shuffled, so that the chunks'
        # address order is not their order in the pack
        order = torch.randperm(n, generator=g).tolist()
        if order == list(range(n)):
            order.reverse()
        room = max(len(r) for r in ref) + 64
        allocs = sorted((torch.full((room,), 0x5A, dtype=torch.uint8, device=DEV) for _ in ref), key=lambda t: t.data_ptr())
        pool = allocs
        blobs = [None] * n
        for place, i in enumerate(order):
            src = arenas[i % 2]  # chunk 0 from the first call, chunk 1 from the second
            view = allocs[place][:len(ref[i])]
            view.copy_(src[i * stride:i * stride + len(ref[i])])
            assert view.data_ptr() % 16 == 0
            blobs[i] = view
        if n > 1:
            assert [b.data_ptr() for b in blobs] != sorted(b.data_ptr() for b in blobs), "address order = chunk order"
        torch.cuda.synchronize()
        for b, r in zip(blobs, ref):
            assert b.cpu().numpy().tobytes() == r, "the HIP encoder's blob is the oracle's"
        out[name] = dict(geo=(L, H, D, T), bins=bins, ref=ref, pack=oracle.pack_from_blobs(ref, CS), blobs=blobs, pool=pool,
                         x=xd)
    return out


def _pack_blobs(ctx, words, case, blobs=None, sizes=None, cap=None):
    """lmc_pack_blobs over the case's blobs -> (status word, the bytes of the device region, pinned copy)."""
    L, H, D, T = case["geo"]
    blobs = case["blobs"] if blobs is None else blobs
    n = len(blobs)
    total = len(case["pack"])
    cap = total if cap is None else cap
    table = torch.tensor([b.data_ptr() for b in blobs], dtype=torch.int64).to(DEV)
    room = torch.tensor([b.numel() for b in blobs] if sizes is None else sizes, dtype=torch.int32).to(DEV)
    region = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    st = words.acquire()
    ctx.pack_blobs(table.data_ptr(), room.data_ptr(), n, L, H, D, CS, T, region.data_ptr(), cap, torch.device(DEV),
                   status_ptr=words.ptr(st))
    torch.cuda.synchronize()
    status = words.read_release(st)
    return status, region.cpu().numpy().tobytes()


def _pinned(data: bytes) -> native.PinnedBuffer:
    buf = native.PinnedBuffer(native.r16(len(data)))
    ctypes.memmove(buf.ptr, data, len(data))
    return buf


# ---- 1. lmc_pack_blobs equals the oracle -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_pack_blobs_equals_the_oracle(ctx, words, built, name):
    case = built[name]
    status, got = _pack_blobs(ctx, words, case)
    want = case["pack"]
    assert status == 0
    assert got[:len(want)] == want, "the pack is not the oracle's, byte for byte"
    assert got[len(want):] == b"\xa5" * 64, "bytes behind the pack were written"
    host = _pinned(got[:len(want)])
    try:
        h = native.pack_info(host.ptr, len(want))
        assert (h.nchunks, h.total_bytes, h.ntokens) == (len(case["ref"]), len(want), case["geo"][3])
        for i, ref in enumerate(case["ref"]):
            assert native.pack_extract(host.ptr, len(want), i) == ref
            assert native.pack_chunk_bytes(host.ptr, len(want), i) == len(ref)
    finally:
        host.free()


# ---- 2. it fails cleanly -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["magic", "short blob", "cap one granule short"])
def test_pack_blobs_fails_cleanly_and_the_next_call_succeeds(ctx, words, built, how):
    case = built["c128"]
    blobs, sizes, cap = list(case["blobs"]), None, None
    if how == "magic":
        bad = blobs[1].clone()
        bad[0] ^= 0xFF
        blobs[1] = bad
    elif how == "short blob":
        sizes = [b.numel() for b in blobs]
        sizes[2] -= 16  # shorter than its header's total
    else:
        cap = len(case["pack"]) - 16
    status, got = _pack_blobs(ctx, words, case, blobs, sizes, cap)
    assert status == ARENA_FULL
    h = native.PackHeader.from_buffer_copy(got[:ctypes.sizeof(native.PackHeader)])
    assert h.magic == 0 and h.total_bytes == 0
    status, got = _pack_blobs(ctx, words, case)
    assert status == 0 and got[:len(case["pack"])] == case["pack"]


# ---- 3. lmc_unpack_blobs is the inverse --------------------------------------------------------------------------------
def _unpack(ctx, words, host, nbytes, c0, m, short=None):
    sizes = [native.pack_chunk_bytes(host.ptr, nbytes, c0 + j) for j in range(m)]
    dst = [torch.full((s + 32,), 0xA5, dtype=torch.uint8, device=DEV) for s in sizes]
    caps = [s - 16 if j == short else s for j, s in enumerate(sizes)]
    st = words.acquire()
    ctx.unpack_blobs(host.ptr, nbytes, c0, m, [d.data_ptr() for d in dst], caps, torch.device(DEV), status_ptr=words.ptr(st))
    torch.cuda.synchronize()
    return words.read_release(st), [d.cpu().numpy().tobytes() for d in dst], sizes


@pytest.mark.parametrize("name", ["c128", "c72", "fp8", "one", "five"])
def test_unpack_blobs_is_the_inverse(ctx, words, built, name):
    case = built[name]
    host = _pinned(case["pack"])
    n = len(case["ref"])
    try:
        for c0 in ([0, 1] if n > 1 else [0]):
            status, got, sizes = _unpack(ctx, words, host, len(case["pack"]), c0, n - c0)
            assert status == 0
            for j, (b, s) in enumerate(zip(got, sizes)):
                assert b[:s] == case["ref"][c0 + j], f"chunk {c0 + j} of [{c0}, {n})"
                assert b[s:] == b"\xa5" * 32, "bytes behind the blob were written"
    finally:
        torch.cuda.synchronize()
        host.free()


def test_unpack_blobs_refuses_a_short_destination_and_a_damaged_table(ctx, words, built):
    case = built["c128"]
    nbytes = len(case["pack"])
    host = _pinned(case["pack"])
    try:
        status, got, sizes = _unpack(ctx, words, host, nbytes, 0, 3, short=1)
        assert status == BAD_HEADER
        assert got[1] == b"\xa5" * len(got[1]), "a chunk that does not fit is not written at all"
        for j in (0, 2):
            assert got[j][:sizes[j]] == case["ref"][j]
        # a damaged offset table: refused on the host, nothing queued
        h = native.pack_info(host.ptr, nbytes)
        entry = ctypes.c_uint64.from_address(host.ptr + h.off_table + 8 * 2)
        entry.value += 8   # off its 16-byte boundary
        dst = torch.full((len(case["ref"][0]),), 0xA5, dtype=torch.uint8, device=DEV)
        with pytest.raises(native.NativeError, match="invalid"):
            ctx.unpack_blobs(host.ptr, nbytes, 0, 1, [dst.data_ptr()], [dst.numel()], torch.device(DEV))
        torch.cuda.synchronize()
        assert bool((dst == 0xA5).all())
        with pytest.raises(native.NativeError):
            native.pack_chunk_bytes(host.ptr, nbytes, 0)
    finally:
        torch.cuda.synchronize()
        host.free()


# ---- 4. round trip through both, through the codec -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def codec():
    c = CacheGenDeviceCodec(0)
    yield c
    torch.cuda.synchronize()
    c.close()


def test_demote_then_promote_gives_the_same_bytes_and_the_same_kv(codec, built):
    case = built["c72"]
    L, H, D, T = case["geo"]
    pinned, hbm = PinnedArena(slab_bytes=1 << 20, budget=1 << 20), DeviceArena(torch.device(DEV), slab_bytes=1 << 20, budget=1 << 20)
    try:
        before = _words_out(codec)
        pack = codec.demote_blobs(case["blobs"], (L, H, D), CS, T, pinned)
        assert pack.blob.tobytes() == case["pack"] and pinned.live_bytes == native.r16(len(case["pack"]))
        back = codec.promote_pack(pack, hbm)
        assert _words_out(codec)[0] == before[0], "both jobs have returned their status words"
        for b, ref in zip(back, case["ref"]):
            assert b.cpu().numpy().tobytes() == ref
        outs = []
        for blobs in (case["blobs"], back):
            out = torch.zeros(L, 2, T, H, D, dtype=torch.bfloat16, device=DEV)
            codec.finish_decode(codec.decode_device(blobs, native.KVLayout.from_chunk(out, "vllm"), 0, CS))
            outs.append(out)
        assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)) and bool(outs[0].any())
    finally:
        torch.cuda.synchronize()
        pinned.close()
        hbm.close()


# ---- 5. - 8. the backend ---------------------------------------------------------------------------------------------------
L_, H_, D_ = 2, 2, 64


def _engine(backend):
    return LMCacheEngine(make_cfg(backend, CS), dumb_metadata("vllm", MODEL))


def _prompt(seed, chunks, kv_seed=None):
    g = torch.Generator().manual_seed(seed)
    tokens = torch.randint(0, 10000, (chunks * CS,), generator=g).to(DEV)
    torch.manual_seed(1000 + (seed if kv_seed is None else kv_seed))
    return tokens, generate_kv_cache(chunks * CS, "vllm", DEV, L_, H_, D_)


def _keys(engine, tokens):
    return [engine._make_key(h, "vllm") for h in engine._prefix_hashes_of(tokens)]


def _retrieve(engine, tokens):
    kv, mask = engine.retrieve(tokens)
    assert bool(mask.all()) and mask.numel() == len(tokens), "not a full hit"
    return torch.stack([torch.stack(l) for l in kv]).clone()


def _same_kv(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


def test_tiered_backend_demotes_serves_and_promotes():
    eng = _engine("cachegen-hbm")
    be = eng.engine_
    try:
        # A and B carry the same KV under different tokens: groups of exactly the same size, so that B's bytes are what
        # A needs to come back
        (ta, kva), (tb, kvb), (tc, kvc) = _prompt(1, 3, kv_seed=7), _prompt(2, 3, kv_seed=7), _prompt(3, 2)
        eng.store(ta, kva)
        live_a = be.tier_stats()["hbm"]["live_bytes"]
        ref_a = _retrieve(eng, ta)
        eng.store(tb, kvb)
        ref_b = _retrieve(eng, tb)
        eng.store(tc, kvc)
        ref_c = _retrieve(eng, tc)
        ka, kb, kc = _keys(eng, ta), _keys(eng, tb), _keys(eng, tc)
        assert (len(ka), len(kb), len(kc)) == (3, 3, 2)
        budget = be.tier_stats()["hbm"]["live_bytes"] - live_a
        be.set_capacity(hbm_bytes=budget, pinned_bytes=1 << 30)
        be.drain()
        assert [be.tier_of(k) for k in ka] == ["pinned"] * 3
        assert [be.tier_of(k) for k in kb + kc] == ["hbm"] * 5
        assert all(be.contains(k) for k in ka + kb + kc)
        st = be.tier_stats()
        assert st["demotions"] == 1 and st["evictions"] == 0 and st["hbm"]["live_bytes"] <= budget
        assert st["pinned"]["groups"] == 1 and st["hbm"]["groups"] == 2
        assert _same_kv(_retrieve(eng, ta), ref_a)      # served where it lies (lmc_load_pack)
        lw = eng.retrieve_layerwise(ta)
        lw.finish()
        assert bool(lw.ret_mask.all()) and _same_kv(torch.stack([torch.stack(l) for l in lw.kv]), ref_a)
        be.drain()                                      # ... and promoted behind the hit
        assert [be.tier_of(k) for k in ka] == ["hbm"] * 3
        assert [be.tier_of(k) for k in kb] == ["pinned"] * 3, "B was the LRU group of {B, C}"
        st = be.tier_stats()
        assert st["promotions"] == 1 and st["demotions"] == 2 and st["hbm"]["live_bytes"] <= budget
        assert all(be.contains(k) for k in ka + kb + kc)
        for t, ref in ((ta, ref_a), (tb, ref_b), (tc, ref_c)):
            assert _same_kv(_retrieve(eng, t), ref)
        be.drain()
        assert be.tier_stats()["hbm"]["live_bytes"] <= budget
    finally:
        torch.cuda.synchronize()
        eng.close()


def _group_bytes(backend):
    """Bytes of one three-chunk group of the test KV in `backend`'s tier (a throwaway engine)."""
    eng = _engine(backend)
    try:
        t, kv = _prompt(50, 3, kv_seed=9)
        eng.store(t, kv)
        st = eng.engine_.tier_stats()
        return st["pinned" if backend == "cachegen-host" else "hbm"]["live_bytes"]
    finally:
        torch.cuda.synchronize()
        eng.close()


def test_pinned_budget_drops_the_lru_group_and_memory_stops_growing():
    g = _group_bytes("cachegen-host")
    eng = _engine("cachegen-host")
    be = eng.engine_
    try:
        be.set_capacity(pinned_bytes=2 * g)             # the bytes of two groups; every group carries the same KV
        prompts = [_prompt(60 + i, 3, kv_seed=9) for i in range(15)]
        refs = []
        for t, kv in prompts[:2]:
            eng.store(t, kv)
            refs.append(_retrieve(eng, t))
        eng.store(*prompts[2])
        refs.append(_retrieve(eng, prompts[2][0]))
        assert not any(be.contains(k) for k in _keys(eng, prompts[0][0]))
        kv, mask = eng.retrieve(prompts[0][0])
        assert not bool(mask.any()) and len(kv) == 0
        for i in (1, 2):
            assert _same_kv(_retrieve(eng, prompts[i][0]), refs[i])
        for t, kv in prompts[3:]:
            eng.store(t, kv)
        st = be.tier_stats()
        assert st["pinned"]["reserved_bytes"] <= 2 * g and st["pinned"]["live_bytes"] <= 2 * g
        assert st["pinned"]["groups"] == 2 and st["evictions"] == 13
        assert _same_kv(_retrieve(eng, prompts[14][0]), refs[2])  # (the same KV under other tokens)
    finally:
        torch.cuda.synchronize()
        eng.close()


def test_a_retrieve_in_flight_survives_its_eviction():
    g = _group_bytes("cachegen-hbm")
    eng = _engine("cachegen-hbm")
    be = eng.engine_
    try:
        cap = g + g // 8                                # room for one group (B's KV differs: its size does by a little)
        be.set_capacity(hbm_bytes=cap)
        (ta, kva), (tb, kvb) = _prompt(80, 3, kv_seed=9), _prompt(81, 3, kv_seed=11)
        eng.store(ta, kva)
        ref = _retrieve(eng, ta)
        ka = _keys(eng, ta)
        out = torch.zeros(L_, 2, 3 * CS, H_, D_, dtype=torch.bfloat16, device=DEV)
        jobs = []
        got = be.get_kv_range(ka, native.KVLayout.from_chunk(out, "vllm"), "vllm", 0, CS, layers_per_launch=1, jobs_out=jobs)
        assert got == 3 and len(jobs) == 1
        be.set_capacity(hbm_bytes=0)                    # A is evicted while its decode may still be running ...
        assert not any(be.contains(k) for k in ka)
        be.set_capacity(hbm_bytes=cap)
        eng.store(tb, kvb)                              # ... and its bytes are taken by a new group
        assert be.tier_stats()["hbm"]["reserved_bytes"] <= cap and all(be.tier_of(k) == "hbm" for k in _keys(eng, tb))
        for codec, job in jobs:
            codec.finish_decode(job)
        assert _same_kv(out, ref)
        assert _retrieve(eng, tb).shape == ref.shape
    finally:
        torch.cuda.synchronize()
        eng.close()


def test_oversize_groups_and_a_demotion_that_fails(monkeypatch):
    g = _group_bytes("cachegen-hbm")
    eng = _engine("cachegen-hbm")
    be = eng.engine_
    codec = be._codec()
    try:
        small, big, huge = _prompt(90, 3, kv_seed=9), _prompt(91, 6, kv_seed=12), _prompt(92, 24, kv_seed=13)
        be.set_capacity(hbm_bytes=g + g // 2, pinned_bytes=6 * g)
        eng.store(*small)
        ref_small = _retrieve(eng, small[0])
        eng.store(*big)                                  # about 2 g: larger than the whole HBM budget -> pinned
        ref_big = _retrieve(eng, big[0])
        assert {be.tier_of(k) for k in _keys(eng, big[0])} == {"pinned"}
        assert {be.tier_of(k) for k in _keys(eng, small[0])} == {"hbm"}
        eng.store(*huge)                                 # about 8 g: larger than both -> not cached, nobody disturbed
        assert not any(be.contains(k) for k in _keys(eng, huge[0]))
        st = be.tier_stats()
        assert (st["evictions"], st["demotions"], st["hbm"]["groups"], st["pinned"]["groups"]) == (0, 0, 1, 1)
        assert _same_kv(_retrieve(eng, small[0]), ref_small) and _same_kv(_retrieve(eng, big[0]), ref_big)
        be.drain()                                       # (big stays pinned: it cannot be promoted into 1.5 g)
        assert {be.tier_of(k) for k in _keys(eng, big[0])} == {"pinned"}

        # a demotion whose launch raises: the group is dropped, nothing half-moved is published, the words are back
        words = _words_out(codec)

        def boom(*a, **k):
            raise RuntimeError("the demotion failed half way")
        other = _prompt(93, 3, kv_seed=14)
        with monkeypatch.context() as m:
            m.setattr(codec, "demote_blobs", boom)
            eng.store(*other)                            # needs small's room: small must go down, and cannot
        be.drain()
        assert _words_out(codec) == words
        assert not any(be.contains(k) for k in _keys(eng, small[0]))
        st = be.tier_stats()
        assert st["evictions"] == 1 and st["demotions"] == 0
        assert st["hbm"]["live_bytes"] <= g + g // 2 and st["pinned"]["live_bytes"] <= 6 * g
        ref_other = _retrieve(eng, other[0])
        again = _prompt(94, 3, kv_seed=14)
        eng.store(*again)                                # later stores work, demotion included
        be.drain()
        assert be.tier_stats()["demotions"] == 1 and {be.tier_of(k) for k in _keys(eng, other[0])} == {"pinned"}
        assert _same_kv(_retrieve(eng, other[0]), ref_other) and _same_kv(_retrieve(eng, again[0]), ref_other)
        assert _same_kv(_retrieve(eng, big[0]), ref_big)
    finally:
        torch.cuda.synchronize()
        eng.close()


def test_a_key_stored_again_gives_its_old_bytes_back():
    g = _group_bytes("cachegen-hbm")
    eng = _engine("cachegen-hbm")
    be = eng.engine_
    try:
        be.set_capacity(hbm_bytes=4 * g)
        t, kv = _prompt(120, 3, kv_seed=9)
        eng.store(t, kv)
        ref = _retrieve(eng, t)
        for _ in range(3):
            eng.store(t, kv, skip_existing=False)   # the same keys again: the entries they had go back to the arena
        st = be.tier_stats()
        assert st["hbm"]["groups"] == 1 and st["hbm"]["live_bytes"] == g == be.dev_arena.live_bytes
        assert _same_kv(_retrieve(eng, t), ref)
    finally:
        torch.cuda.synchronize()
        eng.close()
