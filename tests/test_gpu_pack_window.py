"""lmc_load_pack_heads: a window of heads out of a pack in pinned memory, gathered by k_pack_window, against the same heads
of lmc_load_pack's full decode -- bit for bit, and nothing else of the destination written."""
import ctypes
import functools

import pytest
import torch

from lmcache_amd import native
from lmcache_amd.cache_engine import LMCacheEngine
from lmcache_amd.config import LMCacheEngineConfig, LMCacheEngineMetadata
from tests.test_gpu_paged_split import DEV, _ibits, _mapping, _random, _torch_scatter

pytestmark = pytest.mark.gpu
L, CS, BS, NB = 2, 32, 16, 8


def _word(buf):
    return buf.tensor[:4].view(torch.int32)


@functools.lru_cache(None)
def _pack(H, D, T, dt):
    """(pinned pack, its header, lmc_load_pack's full decode as integers [L, 2, T, H, D]) of random bf16 KV."""
    ctx = native.get_context(0)
    kv = torch.randn(L, 2, T, H, D, generator=torch.Generator().manual_seed(H * D + T)).to(torch.bfloat16).to(DEV)
    region, st = native.PinnedBuffer(native.pack_bound(-(-T // CS), L, CS, H, D)), native.PinnedBuffer(64)
    st.tensor.zero_()
    ctx.store_pack(native.KVLayout.from_chunk(kv, "vllm"), 0, T, CS, [32, 16, 17, 16], region.ptr, region.nbytes, st.ptr + 16, status_ptr=st.ptr)
    torch.cuda.synchronize()
    h = native.pack_info(region.ptr, region.nbytes)
    full = torch.zeros(L, 2, T, H, D, dtype=dt, device=DEV)
    ctx.load_pack(region.ptr, h.total_bytes, 0, 0, native.KVLayout.from_chunk(full, "vllm"), 0, status_ptr=st.ptr)
    torch.cuda.synchronize()
    assert int(_word(st)[0]) == 0
    return region, h, _ibits(full)


def _check(region, h, want, win, Hd, dt, kind, c0=0, m=0, lpr=0, skip=()):
    """load_pack_heads into a destination of random bits with Hd heads: afterwards it is what it was, with heads
    [src_begin, +nheads) of `want` at heads [dst_begin, ...) of the call's tokens but those of the chunks in `skip`."""
    T, D, (_, sb, nh, db) = want.shape[2], want.shape[4], win
    g = torch.Generator().manual_seed(1)
    if kind == "rows":
        dst, slots = [_random((L, 2, T, Hd, D), dt, g).to(DEV)], None
        lay = native.KVLayout.from_chunk(dst[0], "vllm")
    else:
        dst, slots = [_random((2, NB, Hd, D, BS), dt, g).to(DEV) for _ in range(L)], _mapping("random", T, NB, BS, g).to(DEV)
        lay = native.KVLayout.paged(dst, slots, BS, "NHDB")
    exp, st = [d.clone() for d in dst], native.PinnedBuffer(64)
    st.tensor.zero_()
    events = [native.NativeEvent() for _ in range(-(-L // lpr) if lpr else 1)]
    handles = (ctypes.c_void_p * len(events))(*[e.handle for e in events])
    native.get_context(0).load_pack_heads(region.ptr, h.total_bytes, c0, m, lay, c0 * CS, lpr, ctypes.cast(handles, ctypes.c_void_p).value,
                                          native.HeadWindow(*win), status_ptr=st.ptr)
    for e in events:
        e.synchronize()
    torch.cuda.synchronize()
    toks = torch.tensor([t for t in range(c0 * CS, min(T, (c0 + m) * CS) if m else T) if t // CS not in skip], device=DEV)
    if kind == "rows":
        _ibits(exp[0])[:, :, toks, db:db + nh] = want[:, :, toks, sb:sb + nh]
    else:  # (the NHDB cases fill every head of their destination)
        _torch_scatter(exp, want[:, :, toks, sb:sb + nh], slots[toks], BS)
    for got, e in zip(dst, exp):
        assert torch.equal(_ibits(got), _ibits(e))
    return int(_word(st)[0])


@pytest.mark.parametrize("H,D,T,win,Hd,c0,m,lpr,dt,kind", [
    (8, 32, 64, (8, 3, 2, 0), 2, 0, 0, 0, torch.bfloat16, "rows"),  # channels 96 .. 160: inside groups
    (8, 32, 64, (8, 6, 2, 0), 2, 0, 0, 1, torch.float16, "NHDB"),   # ends with the plane, the last V plane included
    (3, 40, 64, (3, 1, 2, 0), 2, 0, 0, 0, torch.bfloat16, "rows"),  # C = 120
    (4, 32, 64, (4, 0, 4, 4), 8, 0, 0, 1, torch.float16, "rows"),   # a shard into the upper heads of a wider destination
    (8, 32, 70, (8, 3, 2, 0), 2, 0, 0, 1, torch.bfloat16, "NHDB"),  # a ragged last chunk
    (8, 32, 70, (8, 3, 2, 1), 4, 1, 1, 0, torch.bfloat16, "rows"),  # one chunk of three
    (8, 32, 70, (8, 0, 8, 0), 8, 0, 0, 1, torch.bfloat16, "rows"),  # the whole blob: lmc_load_pack itself
])
def test_a_window_from_the_pack_equals_the_full_load_sliced_and_nothing_else_is_written(H, D, T, win, Hd, c0, m, lpr, dt, kind):
    assert _check(*_pack(H, D, T, dt), win, Hd, dt, kind, c0, m, lpr) == 0


def test_a_static_slot_that_disagrees_with_the_table_fails_its_chunk_alone():
    good, h, want = _pack(8, 32, 70, torch.bfloat16)
    bad = native.PinnedBuffer(int(h.total_bytes))
    bad.tensor.copy_(good.tensor[:h.total_bytes])
    slot = bad.tensor[h.off_static + h.static_stride:h.off_static + 2 * h.static_stride]  # chunk 1
    at = int(slot[56:60].view(torch.int32)[0]) + 8 * 4  # header word 14: the directory; G = 4: the entry of stream (1, 0)
    slot[at:at + 4].view(torch.int32)[0] += 16  # plane 1 begins 16 bytes late: not what the table says
    assert _check(bad, h, want, (8, 3, 2, 0), 2, torch.bfloat16, "rows", skip=(1,)) == 2  # LMC_STATUS_BAD_HEADER


def test_the_engines_pinned_tier_gathers_the_window_when_switched_on(monkeypatch):
    """stored_at(1).retrieve_into_paged of a TP = 2 rank: the same cache bits with LMCACHE_AMD_PACK_WINDOW on as off, and
    with it on no pinned allocation (off: every chunk's blob is rebuilt in one)."""
    H, D, T, meta = 8, 64, 70, lambda w, r: LMCacheEngineMetadata("Llama-3-8B", w, r, "vllm", "half")
    g = torch.Generator().manual_seed(9)
    tokens = torch.randint(0, 10000, (T,), generator=g).to(DEV)
    kv = tuple(tuple(torch.rand((T, H, D), generator=g).to(torch.bfloat16).to(DEV) for _ in range(2)) for _ in range(L))
    slots, caches = _mapping("random", T, NB, BS, g).to(DEV), {}
    for switch in ("0", "1"):
        monkeypatch.setenv("LMCACHE_AMD_PACK_WINDOW", switch)
        base = LMCacheEngine(LMCacheEngineConfig.from_legacy(chunk_size=CS, backend="cpu", local_serde="cachegen"), meta(1, 0))
        try:
            base.store(tokens, kv)
            rank = LMCacheEngine.__new__(LMCacheEngine)
            rank.__dict__.update({k: v for k, v in base.__dict__.items() if k not in ("_hash_chain", "_key_memo")})
            rank.metadata = meta(2, 1)
            caches[switch] = [torch.zeros(2, NB, H // 2, D, BS, dtype=torch.bfloat16, device=DEV) for _ in range(L)]
            live = base.engine_.host_arena.live_bytes
            m = rank.stored_at(1).retrieve_into_paged(tokens, caches[switch], slots, BS, "NHDB", direct=True)
            torch.cuda.synchronize()
            assert int(m.sum()) == T and (base.engine_.host_arena.live_bytes == live) == (switch == "1")
        finally:
            base.close()
    assert all(torch.equal(_ibits(a), _ibits(b)) and _ibits(a).any() for a, b in zip(caches["0"], caches["1"]))
