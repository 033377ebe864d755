"""The encoder reads vLLM's ROCm paged-attention cache ("NHDB", LMC_PAGED_SPLIT) itself: k_quantize.h's split instances
behind lmc_encode_chunks_split and the stores, and store_paged(direct=True) above them.

Nothing here has a tolerance: a blob coded from the split cache is, byte for byte, the blob coded from the gathered chunk
by the same two kernels, and the oracle's blob of that chunk."""
import ctypes
import struct

import numpy as np
import pytest
import torch

from lmcache_amd import native
from lmcache_amd.cache_engine import LMCacheEngine
from tests import far_offsets as fo
from tests.test_gpu_engine import dumb_metadata, generate_tokens, make_cfg
from tests.test_gpu_paged_split import (DEV, L, NTOK, _ibits, _mapping, _nblocks, _split_caches, _torch_gather,
                                        _torch_scatter)

pytestmark = pytest.mark.gpu

CS = 32                  # 70 tokens: two full chunks and a ragged one of 6 tokens (a partial oct)
BINS = [32, 16, 16, 32]  # K of layer 0 / 1, V of layer 0 / 1: a byte plane and a nibble plane on each side
BF16, FP16, E4M3, E5M2 = torch.bfloat16, torch.float16, torch.float8_e4m3fn, torch.float8_e5m2
FP8 = (E4M3, E5M2)
NAMES = {BF16: "bf16", FP16: "fp16", E4M3: "e4m3", E5M2: "e5m2"}
INVALID = -1

# (H, D, bs): G = 16 (four octs per wave), G = 16 with two heads, G = 32, G = 64, NITER = 2, a partly filled last lane (10 and
# 5 granules), block size 32
GEOMS = [(1, 64, 8), (2, 64, 16), (2, 128, 16), (4, 128, 16), (8, 128, 16), (1, 80, 16), (2, 64, 32)]
KINDS = ["blocks", "offset5", "random", "broken", "unaligned"]
DTS = [BF16, FP16, E4M3, E5M2]
# every geometry with every mapping once and with two dtypes (the dtype walks with the mapping, so every geometry meets all
# four): 35 cases; every dtype 8 or 9 times, every mapping 7 times
CASES = [(geom, KINDS[k], DTS[(gi + k) % 4]) for gi, geom in enumerate(GEOMS) for k in range(5)]


@pytest.fixture(scope="module")
def ctx():
    native.build()
    return native.get_context(0)


@pytest.fixture(scope="module")
def oracle():
    from oracle import lmc_oracle
    lmc_oracle.build()
    return lmc_oracle


def _kv(H, D, dt, g, ntok=NTOK):
    """[L, 2, ntok, H, D] of dt (CPU): randn, with an all-zero token, a token with an inf and one with a NaN in every
    plane (fp8: drawn in bf16 and cast -- e4m3fn has no inf, the cast gives its NaN)."""
    x = torch.randn((L, 2, ntok, H, D), generator=g).to(torch.bfloat16)
    x[:, :, 9] = 0
    x[:, :, 21, 0, 3] = float("inf")
    x[:, :, ntok - 3, H - 1, D - 2] = float("nan")
    return x.to(dt)


def _oracle_blobs(oracle, x, cs, H, D, bins):
    """The oracle's blob of every chunk of x [L, 2, T, H, D] (fp8: the blob of the bf16 images, header word 23 set)."""
    out = []
    for t0 in range(0, x.shape[2], cs):
        part = x[:, :, t0:t0 + cs].reshape(L, 2, -1, H * D)
        bits, code = oracle.torch_to_bits((part.to(torch.bfloat16) if x.dtype in FP8 else part).contiguous())
        blob = oracle.encode_blob(bits, code, H, D, np.array(bins, np.int32))
        if x.dtype in FP8:
            blob = blob[:92] + struct.pack("<I", native.dtype_code(x.dtype)) + blob[96:]
        out.append(blob)
    return out


def _encode(ctx, fn, layout, ntok, cs, H, D, bins=BINS):
    """fn (ctx.encode_chunks / ctx.encode_chunks_split) under "two_kernels" -> (sizes, [blob bytes])."""
    stride = native.r16(native.blob_bound(L, cs, H, D))
    n = (ntok + cs - 1) // cs
    blobs = torch.zeros(n * stride, dtype=torch.uint8, device=DEV)
    sizes = torch.zeros(n, dtype=torch.int32, device=DEV)
    ctx.set_encode_path("two_kernels")
    try:
        fn(layout, 0, ntok, cs, bins, blobs.data_ptr(), stride, sizes.data_ptr())
        torch.cuda.synchronize()
    finally:
        ctx.set_encode_path("auto")
    ctx.raise_on_status("encode")
    sz, host = sizes.cpu().tolist(), blobs.cpu().numpy()
    return sz, [host[i * stride:i * stride + sz[i]].tobytes() for i in range(n)]


def _filled_split(H, D, bs, dt, kind, g, x):
    nb = _nblocks(bs)
    caches = _split_caches(H, D, bs, dt, g, unaligned=kind == "unaligned", nblocks=nb)
    slots = _mapping(kind, NTOK, nb, bs, g).to(DEV)
    _torch_scatter(caches, _ibits(x.to(DEV)), slots, bs)
    return caches, slots


# ------------------------------------------------------------------ 1. blob parity
@pytest.mark.parametrize("geom,kind,dt", CASES, ids=["H%d_D%d_bs%d-%s-%s" % (g + (k, NAMES[d])) for g, k, d in CASES])
def test_blobs_from_the_split_cache_equal_those_from_the_gathered_chunk(ctx, oracle, geom, kind, dt):
    H, D, bs = geom
    g = torch.Generator().manual_seed(100 * H + D + bs + KINDS.index(kind))
    x = _kv(H, D, dt, g)
    caches, slots = _filled_split(H, D, bs, dt, kind, g, x)
    before = [c.clone() for c in caches]
    chunk = _torch_gather(caches, slots, bs).view(dt).contiguous()
    assert torch.equal(_ibits(chunk).cpu(), _ibits(x))
    split = native.KVLayout.paged(caches, slots, bs, "NHDB")
    sz_s, blobs_s = _encode(ctx, ctx.encode_chunks_split, split, NTOK, CS, H, D)
    sz_r, blobs_r = _encode(ctx, ctx.encode_chunks, native.KVLayout.from_chunk(chunk, "vllm"), NTOK, CS, H, D)
    want = _oracle_blobs(oracle, x, CS, H, D, BINS)
    assert len(blobs_s) == 3 and sz_s == sz_r == [len(b) for b in want]
    for i in range(3):
        assert blobs_s[i] == blobs_r[i], f"chunk {i}: split source vs gathered chunk"
        assert blobs_s[i] == want[i], f"chunk {i}: split source vs oracle"
    for c, b in zip(caches, before):
        assert torch.equal(_ibits(c), _ibits(b)), "the cache keeps its bits"


# ------------------------------------------------------------------ 2. blocks past 4 GiB
@pytest.fixture(scope="module")
def arena():
    native.build()
    free, need = torch.cuda.mem_get_info()[0], fo.ARENA_BYTES + 4 * fo.GIB
    if free < need:
        pytest.skip(f"far-offset arena: {free} bytes of device memory are free, {need} are needed")
    a = torch.full((fo.ARENA_BYTES,), fo.FILL, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    yield a
    del a
    torch.cuda.empty_cache()


@pytest.mark.parametrize("swapped", [False, True], ids=["runs", "swapped"])
def test_blocks_beyond_4_gib_from_the_plane_base(ctx, oracle, arena, swapped):
    """far_offsets.paged_split: blocks on both sides of 2^31 and 2^32 bytes from the plane base and the arena's last one
    (the 64-bit block offset of split_load_oct), as runs (the V form) and with neighbours swapped (token-major)."""
    spec = fo.paged_split(2, swapped)
    H, D, T, cs, bs = fo.H, fo.D, fo.T, fo.CS, spec.bs
    assert (fo.L, len(BINS)) == (L, 2 * L) and int(spec.block_off().max()) > 4 * fo.GIB
    g = torch.Generator().manual_seed(50 + swapped)
    x = _kv(H, D, BF16, g, ntok=T)
    starts, img = fo.expected_windows(*spec.pieces(fo.to_bytes(x)))
    fo.write_windows(arena, starts, img)
    try:
        layout = native.KVLayout.paged(spec.views(arena, BF16), torch.from_numpy(spec.slots).to(DEV), bs, "NHDB")
        assert layout.struct.paged_kind == native.PAGED_SPLIT and layout.struct.stride_block * 2 == fo.STRIDE_BLOCK
        sz_s, blobs_s = _encode(ctx, ctx.encode_chunks_split, layout, T, cs, H, D)
        sz_r, blobs_r = _encode(ctx, ctx.encode_chunks, native.KVLayout.from_chunk(x.to(DEV), "vllm"), T, cs, H, D)
        want = _oracle_blobs(oracle, x, cs, H, D, BINS)
        assert sz_s == sz_r == [len(b) for b in want]
        assert blobs_s == blobs_r and blobs_s == want
        assert np.array_equal(fo.read_windows(arena, starts), img), "the cache keeps its bytes"
    finally:
        fo.restore_windows(arena, starts)


# ------------------------------------------------------------------ 3. the stores
def _store_pack_parts(ctx, layout, ntok, cs, H, D):
    n = (ntok + cs - 1) // cs
    cap = native.pack_bound(n, L, cs, H, D)
    dev = torch.zeros(cap, dtype=torch.uint8, device=DEV)
    n4 = (4 * n + 7) & ~7
    meta = native.PinnedBuffer(n4 + 64 + 16 * 16)
    meta.tensor[:] = 0
    nparts = 8
    events = [native.NativeEvent() for _ in range(nparts)]
    st = torch.cuda.Stream(device=DEV)
    st.wait_stream(torch.cuda.current_stream())
    ctx.set_encode_path("two_kernels")
    try:
        ctx.store_pack_parts(layout, 0, ntok, cs, BINS, dev.data_ptr(), cap, meta.ptr, nparts, meta.ptr + n4 + 64, events,
                             stream=st.cuda_stream, status_ptr=meta.ptr + n4)
    finally:
        ctx.set_encode_path("auto")
    st.synchronize()
    assert int(meta.tensor[n4:n4 + 4].view(torch.int32)[0]) == 0
    info = meta.tensor[n4 + 64:n4 + 64 + 16 * nparts].view(torch.int64).tolist()
    sizes = meta.tensor[:4 * n].view(torch.int32).tolist()
    total = native.pack_off_streams(n, L, cs, H, D) + sum(info[1::2])
    out = (sizes, info, dev[:total].cpu().numpy().tobytes())
    meta.free()
    return out


def _store_chunks(ctx, layout, ntok, cs, H, D):
    n = (ntok + cs - 1) // cs
    bound = native.r16(native.blob_bound(L, cs, H, D))
    arena_h = native.PinnedBuffer(n * bound)
    meta = native.PinnedBuffer(8 * (n + 1) + 4 * n + 64)
    meta.tensor[:] = 0
    o_sizes, o_status = 8 * (n + 1), 8 * (n + 1) + ((4 * n + 7) & ~7)
    st = torch.cuda.Stream(device=DEV)
    st.wait_stream(torch.cuda.current_stream())
    ctx.set_encode_path("two_kernels")
    try:
        ctx.store_chunks(layout, 0, ntok, cs, BINS, arena_h.ptr, arena_h.nbytes, meta.ptr, meta.ptr + o_sizes,
                         stream=st.cuda_stream, status_ptr=meta.ptr + o_status)
    finally:
        ctx.set_encode_path("auto")
    st.synchronize()
    assert int(meta.tensor[o_status:o_status + 4].view(torch.int32)[0]) == 0
    offs = meta.tensor[:8 * (n + 1)].view(torch.int64).tolist()
    sizes = meta.tensor[o_sizes:o_sizes + 4 * n].view(torch.int32).tolist()
    out = (offs, sizes, ctypes.string_at(arena_h.ptr, offs[n]))
    arena_h.free()
    meta.free()
    return out


@pytest.mark.parametrize("dt,kind", [(BF16, "blocks"), (E4M3, "offset5")], ids=["bf16-blocks", "e4m3-offset5"])
def test_stores_from_a_split_source_write_what_they_write_from_the_chunk(ctx, dt, kind):
    H, D, bs = 2, 128, 16
    g = torch.Generator().manual_seed(31)
    x = _kv(H, D, dt, g)
    caches, slots = _filled_split(H, D, bs, dt, kind, g, x)
    split = native.KVLayout.paged(caches, slots, bs, "NHDB")
    rows = native.KVLayout.from_chunk(x.to(DEV), "vllm")
    sizes_s, info_s, pack_s = _store_pack_parts(ctx, split, NTOK, CS, H, D)
    sizes_r, info_r, pack_r = _store_pack_parts(ctx, rows, NTOK, CS, H, D)
    assert sizes_s == sizes_r and all(sizes_s) and pack_s == pack_r
    assert sum(1 for nb in info_s[1::2] if nb) == 1, "a split source is one part"
    offs_s, sz_s, blobs_s = _store_chunks(ctx, split, NTOK, CS, H, D)
    offs_r, sz_r, blobs_r = _store_chunks(ctx, rows, NTOK, CS, H, D)
    assert offs_s == offs_r and sz_s == sz_r == sizes_s and blobs_s == blobs_r


# ------------------------------------------------------------------ 4. refusals launch nothing
def test_refusals_launch_nothing_and_rows_pass_through(ctx):
    lib, ref = native.lib(), ctypes.byref
    st = native.current_stream_ptr(torch.device(DEV))
    g = torch.Generator().manual_seed(13)
    bins = (ctypes.c_int32 * (2 * L))(*BINS)

    def refused(struct_, H, D):
        stride = native.r16(native.blob_bound(L, CS, H, D))
        blobs = torch.full((3 * stride,), 0x5A, dtype=torch.uint8, device=DEV)
        sizes = torch.full((3,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
        rc = lib.lmc_encode_chunks_split(ctx.handle, ref(struct_), 0, NTOK, CS, bins, blobs.data_ptr(), stride,
                                         sizes.data_ptr(), None, st)
        torch.cuda.synchronize()
        assert rc == INVALID and bool((blobs == 0x5A).all()) and bool((sizes == 0x5A5A5A5A).all())

    wide = _split_caches(16, 128, 16, BF16, g)  # H * D = 2048
    slots = _mapping("blocks", NTOK, _nblocks(16), 16, g).to(DEV)
    refused(native.KVLayout.paged(wide, slots, 16, "NHDB").struct, 16, 128)
    ok = native.KVLayout.paged(_split_caches(2, 64, 16, BF16, g), slots, 16, "NHDB")
    no_slots = native.KvLayoutStruct.from_buffer_copy(ok.struct)
    no_slots.slot_mapping = None
    refused(no_slots, 2, 64)
    assert ctx.status(clear=True) == 0
    # a rows source: what lmc_encode_chunks gives
    x = _kv(2, 64, BF16, g).to(DEV)
    rows = native.KVLayout.from_chunk(x, "vllm")
    assert _encode(ctx, ctx.encode_chunks_split, rows, NTOK, CS, 2, 64) == _encode(ctx, ctx.encode_chunks, rows, NTOK, CS, 2, 64)


# ------------------------------------------------------------------ 5. engine
def _engine_kv(H, D, bs, g, dt=BF16):
    nb = _nblocks(bs)
    x = torch.rand((L, 2, NTOK, H, D), generator=g).to(dt)
    slots = _mapping("offset5", NTOK, nb, bs, g).to(DEV)
    caches = _split_caches(H, D, bs, dt, g, nblocks=nb)
    _torch_scatter(caches, _ibits(x.to(DEV)), slots, bs)
    return x, caches, slots


def _count_copy_kv(monkeypatch):
    """Counts the calls of copy_kv of the device's context (the one the engine, the codec and the backends share).  On the
    instance: that counts whether or not an earlier test has left an attribute of its own there."""
    calls = []
    ctx = native.get_context(0)
    real = ctx.copy_kv

    def counted(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(ctx, "copy_kv", counted)
    return calls


def _store_both(monkeypatch, backend, H, D, bs, layout="NHDB", caches_of=None):
    """Two engines store the same cache, direct=True and direct=False -> (retrieved direct, retrieved staged, copy_kv calls
    during the direct store, during the staged store)."""
    g = torch.Generator().manual_seed(17)
    x, caches, slots = _engine_kv(H, D, bs, g)
    if caches_of is not None:
        caches = caches_of(x, slots)
    tokens = generate_tokens(NTOK, DEV)
    e_direct = LMCacheEngine(make_cfg(backend, CS), dumb_metadata("vllm", "Llama-3-8B"))
    e_staged = LMCacheEngine(make_cfg(backend, CS), dumb_metadata("vllm", "Llama-3-8B"))
    try:
        calls = _count_copy_kv(monkeypatch)
        e_direct.store_paged(tokens, caches, slots, bs, layout, direct=True)
        n_direct = len(calls)
        e_staged.store_paged(tokens, caches, slots, bs, layout, direct=False)
        n_staged = len(calls) - n_direct
        monkeypatch.undo()
        r1, m1 = e_direct.retrieve(tokens)
        r2, m2 = e_staged.retrieve(tokens)
        assert int(m1.sum()) == NTOK and torch.equal(m1, m2) and len(r1) == len(r2) == L
        for (k1, v1), (k2, v2) in zip(r1, r2):
            assert torch.equal(_ibits(k1), _ibits(k2)) and torch.equal(_ibits(v1), _ibits(v2))
        return x, r1, n_direct, n_staged
    finally:
        e_direct.close()
        e_staged.close()


@pytest.mark.parametrize("tier", ["cachegen-host", "cachegen-host-unpinned", "cachegen-hbm"])
def test_direct_store_paged_stores_what_the_staged_one_stores_without_a_gather(monkeypatch, tier):
    if tier == "cachegen-host-unpinned":
        monkeypatch.setenv("LMCACHE_AMD_PINNED_PACKS", "0")
    backend = "cachegen-host" if tier.startswith("cachegen-host") else tier
    _, _, n_direct, n_staged = _store_both(monkeypatch, backend, 2, 128, 16)
    assert n_direct == 0 and n_staged >= 1


def test_direct_means_nothing_for_the_raw_tier_and_for_row_blocks(monkeypatch):
    x, r, n_direct, n_staged = _store_both(monkeypatch, "cuda", 2, 64, 16)
    assert n_direct == n_staged >= 1  # the raw tier's gather is the store
    for l in range(L):  # raw chunks: lossless
        assert torch.equal(_ibits(r[l][0]), _ibits(x[l, 0].to(DEV))) and torch.equal(_ibits(r[l][1]), _ibits(x[l, 1].to(DEV)))

    def nbhd(x, slots):
        nb, bs = _nblocks(16), 16
        rows = [torch.zeros((2, nb, bs, 2, 64), dtype=BF16, device=DEV) for _ in range(L)]
        for c, layer in zip(rows, x.to(DEV)):
            c[0, slots // bs, slots % bs] = layer[0]
            c[1, slots // bs, slots % bs] = layer[1]
        return rows

    _, _, n_direct, n_staged = _store_both(monkeypatch, "cachegen-host", 2, 64, 16, layout="NBHD", caches_of=nbhd)
    assert n_direct == n_staged == 0  # read in place either way


def test_direct_with_planes_wider_than_1024_channels_falls_back_to_staging(monkeypatch):
    _, _, n_direct, n_staged = _store_both(monkeypatch, "cachegen-host", 16, 128, 16)
    assert n_direct >= 1 and n_staged >= 1
