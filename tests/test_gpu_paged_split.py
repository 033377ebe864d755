"""layout "NHDB": the cache of vLLM's ROCm paged-attention kernels (include/lmc_hip.h: LMC_PAGED_SPLIT) on the GPU.

    x = 16 / element bytes
    key_cache   = cache[0].view(num_blocks, H, D / x, block_size, x)
    value_cache = cache[1].view(num_blocks, H, D, block_size)

The reference is torch indexing on these two views, written out here.  Everything is a copy: bit-exact, compared on the
integer views of the elements (random bit patterns hold NaNs)."""
import ctypes

import pytest
import torch

from lmcache_amd import native
from lmcache_amd.cache_engine import LMCacheEngine
from tests.test_gpu_engine import dumb_metadata, generate_tokens, make_cfg

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
L, NTOK, NBLOCKS = 2, 70, 12
DTYPES = [torch.bfloat16, torch.float16, torch.float8_e4m3fn]
GEOMS = [(H, D, bs) for H in (1, 2) for D in (64, 128) for bs in (8, 16, 32)]
GEOMS.append((1, 80, 16))  # D / x = 10 granules per row (16-bit) and 5 (fp8: an odd count, the image's other rotation)
MAPPINGS = ["blocks", "offset5", "random", "broken", "unaligned"]


def _x(dt):
    return 16 // dt.itemsize


def _ibits(t):
    return t.view(torch.int16 if t.dtype.itemsize == 2 else torch.uint8)


def _random(shape, dt, g):
    """Random BIT PATTERNS of dtype dt (a copy must move every one of them)."""
    n = 1
    for s in shape:
        n *= s
    return torch.randint(0, 256, (n * dt.itemsize,), generator=g, dtype=torch.uint8).view(dt).view(shape)


def _split_caches(H, D, bs, dt, g, unaligned=False, nblocks=NBLOCKS):
    """Per layer a cache [2, nblocks, H, D, bs] filled with a position-dependent non-zero pattern; `unaligned`: its base
    2 bytes off a 16-byte boundary (a slice of a larger allocation)."""
    out = []
    n = 2 * nblocks * H * D * bs
    skip = 2 // dt.itemsize
    for _ in range(L):
        flat = _random((n + 16,), dt, g).to(DEV)
        _ibits(flat)[:] |= 1  # non-zero everywhere
        c = (flat[skip:skip + n] if unaligned else flat[:n]).view(2, nblocks, H, D, bs)
        assert c.data_ptr() % 16 == (2 if unaligned else 0)
        out.append(c)
    return out


def _views(c):
    """(key_cache, value_cache) of one layer's [2, nb, H, D, bs] cache, as PagedAttention.split_kv_cache views them."""
    _, nb, H, D, bs = c.shape
    x = _x(c.dtype)
    return c[0].view(nb, H, D // x, bs, x), c[1]


def _torch_gather(caches, slots, bs):
    """-> [L, 2, T, H, D], by indexing the two views."""
    blk, off = slots // bs, slots % bs
    out = []
    for c in caches:
        kc, vc = _views(c)
        k = _ibits(kc)[blk, :, :, off, :]            # [T, H, D/x, x]
        v = _ibits(vc)[blk, :, :, off]               # [T, H, D]
        out.append(torch.stack([k.reshape(k.shape[0], k.shape[1], -1), v]))
    return torch.stack(out)


def _torch_scatter(caches, chunk_bits, slots, bs):
    """chunk_bits [L, 2, T, H, D] (integer view) into slot slots[t] of every layer's cache, by indexing the two views."""
    blk, off = slots // bs, slots % bs
    for c, layer in zip(caches, chunk_bits):
        kc, vc = _views(c)
        T, H, D = layer[0].shape
        _ibits(kc)[blk, :, :, off, :] = layer[0].reshape(T, H, D // kc.shape[-1], kc.shape[-1])
        _ibits(vc)[blk, :, :, off] = layer[1]


def _mapping(kind, n, nblocks, bs, g):
    if kind == "random":  # every token at a slot of its own
        return torch.randperm(nblocks * bs, generator=g)[:n]
    start = 5 if kind == "offset5" else 0  # enters its first block at offset 5 and ends in the middle of its last
    need = (start + n + bs - 1) // bs
    blocks = torch.randperm(nblocks, generator=g)[:need]
    pos = torch.arange(start, start + n)
    slots = blocks[pos // bs] * bs + pos % bs  # blocks in shuffled order, a block's tokens in order
    if kind == "broken":
        # the run breaks in the middle of a tile: two neighbours swapped inside the second block, and from the middle of
        # the third block on the tokens continue in the blocks the mapping has not used (same offsets)
        j = bs + 3
        slots[[j, j + 1]] = slots[[j + 1, j]]
        cut = 2 * bs + bs // 2
        if cut < n:
            spare = torch.tensor([b for b in range(nblocks) if b not in set(blocks.tolist())] + blocks.tolist())
            slots[cut:] = spare[pos[cut:] // bs] * bs + pos[cut:] % bs
        assert slots.unique().numel() == n
    return slots


def _nblocks(bs):
    return max(NBLOCKS, 2 * ((NTOK + 5 + bs - 1) // bs) + 2)  # about a dozen; "broken" needs spare blocks


@pytest.fixture(scope="module")
def ctx():
    native.build()
    return native.get_context(0)


# ------------------------------------------------------------------ gather / scatter through ctx.copy_kv
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "H%d_D%d_bs%d" % g)
@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16", "e4m3"])
def test_gather_and_scatter_equal_torch_indexing(ctx, dt, geom):
    H, D, bs = geom
    nb = _nblocks(bs)
    g = torch.Generator().manual_seed(1000 * H + D + bs)
    for kind in MAPPINGS:
        caches = _split_caches(H, D, bs, dt, g, unaligned=kind == "unaligned", nblocks=nb)
        slots = _mapping(kind, NTOK, nb, bs, g).to(DEV)
        split = native.KVLayout.paged(caches, slots, bs, "NHDB")
        assert not split.vector_readable()
        want = _torch_gather(caches, slots, bs)
        # gather into a vllm chunk and into a huggingface-strided one
        chunk = torch.zeros((L, 2, NTOK, H, D), dtype=dt, device=DEV)
        ctx.copy_kv(split, 0, NTOK, native.KVLayout.from_chunk(chunk, "vllm"), 0)
        hf = torch.zeros((L, 2, H, NTOK, D), dtype=dt, device=DEV)
        ctx.copy_kv(split, 0, NTOK, native.KVLayout.from_chunk(hf, "huggingface"), 0)
        torch.cuda.synchronize()
        assert torch.equal(_ibits(chunk), want), f"gather {kind}"
        assert torch.equal(_ibits(hf).permute(0, 1, 3, 2, 4), want), f"gather into huggingface {kind}"
        # scatter: the WHOLE cache equals the torch-built expectation (nothing outside the given slots moves)
        new = _random((L, 2, NTOK, H, D), dt, g).to(DEV)
        expect = [c.clone() for c in caches]
        _torch_scatter(expect, _ibits(new), slots, bs)
        ctx.copy_kv(native.KVLayout.from_chunk(new, "vllm"), 0, NTOK, split, 0)
        torch.cuda.synchronize()
        for l in range(L):
            assert torch.equal(_ibits(caches[l]), _ibits(expect[l])), f"scatter {kind} layer {l}"
        # ... and from a huggingface-strided source
        new_hf = _random((L, 2, H, NTOK, D), dt, g).to(DEV)
        _torch_scatter(expect, _ibits(new_hf).permute(0, 1, 3, 2, 4), slots, bs)
        ctx.copy_kv(native.KVLayout.from_chunk(new_hf, "huggingface"), 0, NTOK, split, 0)
        torch.cuda.synchronize()
        for l in range(L):
            assert torch.equal(_ibits(caches[l]), _ibits(expect[l])), f"scatter from huggingface {kind} layer {l}"


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16", "e4m3"])
@pytest.mark.parametrize("kind", ["offset5", "random"])
def test_sub_ranges_of_both_sides(ctx, dt, kind):
    """tok_begin > 0 and dst_tok0 > 0, in both directions; what lies outside the range keeps its bytes."""
    H, D, bs = 2, 128, 16
    g = torch.Generator().manual_seed(77)
    caches = _split_caches(H, D, bs, dt, g)
    slots = _mapping(kind, NTOK, NBLOCKS, bs, g).to(DEV)
    split = native.KVLayout.paged(caches, slots, bs, "NHDB")
    tb, n, d0 = 7, 40, 3
    chunk = _random((L, 2, 50, H, D), dt, g).to(DEV)
    want = _ibits(chunk).clone()
    want[:, :, d0:d0 + n] = _torch_gather(caches, slots[tb:tb + n], bs)
    ctx.copy_kv(split, tb, n, native.KVLayout.from_chunk(chunk, "vllm"), d0)
    torch.cuda.synchronize()
    assert torch.equal(_ibits(chunk), want)
    # scatter tokens [4, 44) of a chunk to the slots of tokens 9 ..
    src = _random((L, 2, 50, H, D), dt, g).to(DEV)
    expect = [c.clone() for c in caches]
    _torch_scatter(expect, _ibits(src)[:, :, 4:4 + n], slots[9:9 + n], bs)
    ctx.copy_kv(native.KVLayout.from_chunk(src, "vllm"), 4, n, split, 9)
    torch.cuda.synchronize()
    for l in range(L):
        assert torch.equal(_ibits(caches[l]), _ibits(expect[l]))


def test_a_row_paged_cache_on_the_other_side(ctx):
    """The other side may be any layout lmc_copy_kv takes today: here an NBHD paged cache with a mapping of its own."""
    H, D, bs, dt = 2, 64, 16, torch.bfloat16
    g = torch.Generator().manual_seed(5)
    caches = _split_caches(H, D, bs, dt, g)
    slots = _mapping("blocks", NTOK, NBLOCKS, bs, g).to(DEV)
    rows = [torch.zeros((2, NBLOCKS, bs, H, D), dtype=dt, device=DEV) for _ in range(L)]
    rslots = _mapping("random", NTOK, NBLOCKS, bs, g).to(DEV)
    ctx.copy_kv(native.KVLayout.paged(caches, slots, bs, "NHDB"), 0, NTOK, native.KVLayout.paged(rows, rslots, bs, "NBHD"), 0)
    torch.cuda.synchronize()
    want = _torch_gather(caches, slots, bs)
    for l in range(L):
        for kv in range(2):
            assert torch.equal(_ibits(rows[l])[kv, rslots // bs, rslots % bs], want[l, kv])


# ------------------------------------------------------------------ Python binding
def test_paged_refuses_what_the_layout_cannot_hold():
    g = torch.Generator().manual_seed(3)
    slots = torch.arange(NTOK)
    # head_size % x: an fp8 head of 72 is whole 8-element vectors but not whole 16-element granules (80 = 5 * 16 is
    # fine, and is copied in test_gather_and_scatter_equal_torch_indexing)
    with pytest.raises(ValueError, match="multiple of x"):
        native.KVLayout.paged(_split_caches(1, 72, 16, torch.float8_e4m3fn, g), slots, 16, "NHDB")
    with pytest.raises(ValueError, match="multiple of x"):
        native.KVLayout.paged(_split_caches(2, 68, 16, torch.bfloat16, g), slots, 16, "NHDB")
    assert native.KVLayout.paged(_split_caches(1, 80, 16, torch.float8_e4m3fn, g), slots, 16, "NHDB").D == 80
    ok = _split_caches(2, 64, 16, torch.bfloat16, g)
    with pytest.raises(ValueError, match="block_size"):
        native.KVLayout.paged(ok, slots, 8, "NHDB")
    with pytest.raises(ValueError, match="dense"):
        native.KVLayout.paged([c[..., ::2] for c in ok], slots, 8, "NHDB")
    with pytest.raises(ValueError, match="fp8 view"):
        native.KVLayout.paged([c.view(torch.uint8) for c in _split_caches(1, 64, 16, torch.float8_e4m3fn, g)], slots, 16, "NHDB")
    with pytest.raises(ValueError):
        native.KVLayout.paged(ok, slots, 16, "NDHB")
    pair = [_views(c) for c in ok]
    assert native.KVLayout.paged(pair, slots, 16, "NHDB").struct.paged_kind == native.PAGED_SPLIT
    with pytest.raises(ValueError, match="key_cache"):
        native.KVLayout.paged([(k.transpose(2, 3), v) for k, v in pair], slots, 16, "NHDB")


# ------------------------------------------------------------------ C ABI: who takes the layout
def test_only_copy_kv_takes_a_split_layout_and_nothing_is_launched(ctx):
    H, D, bs, dt, cs = 2, 64, 16, torch.bfloat16, 32
    lib = native.lib()
    g = torch.Generator().manual_seed(9)
    caches = _split_caches(H, D, bs, dt, g)
    before = [c.clone() for c in caches]
    slots = _mapping("blocks", NTOK, NBLOCKS, bs, g).to(DEV)
    split = native.KVLayout.paged(caches, slots, bs, "NHDB")
    other = native.KVLayout.paged(_split_caches(H, D, bs, dt, g), slots, bs, "NHDB")
    st = native.current_stream_ptr(torch.device(DEV))
    stride = native.r16(native.blob_bound(L, cs, H, D))
    blobs = torch.full((2 * stride,), 0x5A, dtype=torch.uint8, device=DEV)
    sizes = torch.full((2,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    bins = (ctypes.c_int32 * (2 * L))(*([32] * (2 * L)))
    INVALID = -1
    ref = ctypes.byref
    assert lib.lmc_encode_chunks(ctx.handle, ref(split.struct), 0, 64, cs, bins, blobs.data_ptr(), stride, sizes.data_ptr(),
                                 None, st) == INVALID
    assert lib.lmc_decode_chunks(ctx.handle, blobs.data_ptr(), stride, 2, ref(split.struct), 0, cs, None, st) == INVALID
    assert lib.lmc_copy_kv(ctx.handle, ref(split.struct), 0, NTOK, ref(other.struct), 0, st) == INVALID
    sym = torch.zeros((2 * L, cs, H * D), dtype=torch.int8, device=DEV)
    scale = torch.zeros((2 * L, cs), dtype=torch.int16, device=DEV)
    assert lib.lmc_quantize(ctx.handle, ref(split.struct), 0, cs, bins, sym.data_ptr(), scale.data_ptr(), st) == INVALID
    # paged_kind = 2 is nobody's layout
    chunk = torch.zeros((L, 2, NTOK, H, D), dtype=dt, device=DEV)
    rows = native.KVLayout.from_chunk(chunk, "vllm")
    bad = native.KvLayoutStruct.from_buffer_copy(split.struct)
    bad.paged_kind = 2
    assert lib.lmc_copy_kv(ctx.handle, ref(bad), 0, NTOK, ref(rows.struct), 0, st) == INVALID
    assert lib.lmc_copy_kv(ctx.handle, ref(rows.struct), 0, NTOK, ref(bad), 0, st) == INVALID
    bad_rows = native.KvLayoutStruct.from_buffer_copy(rows.struct)
    bad_rows.paged_kind = 2
    assert lib.lmc_encode_chunks(ctx.handle, ref(bad_rows), 0, 64, cs, bins, blobs.data_ptr(), stride, sizes.data_ptr(),
                                 None, st) == INVALID
    # a split layout needs its slot mapping, and whole x-granules
    no_slots = native.KvLayoutStruct.from_buffer_copy(split.struct)
    no_slots.slot_mapping = None
    assert lib.lmc_copy_kv(ctx.handle, ref(no_slots), 0, NTOK, ref(rows.struct), 0, st) == INVALID
    odd, odd_rows = native.KvLayoutStruct.from_buffer_copy(split.struct), native.KvLayoutStruct.from_buffer_copy(rows.struct)
    odd.head_size = odd_rows.head_size = 60
    assert lib.lmc_copy_kv(ctx.handle, ref(odd), 0, NTOK, ref(odd_rows), 0, st) == INVALID
    torch.cuda.synchronize()
    assert bool((blobs == 0x5A).all()) and bool((sizes == 0x5A5A5A5A).all()) and not chunk.any() and not sym.any()
    for c, b in zip(caches, before):
        assert torch.equal(_ibits(c), _ibits(b))
    # ... while the one entry point that takes it does
    ctx.copy_kv(split, 0, NTOK, rows, 0)
    torch.cuda.synchronize()
    assert torch.equal(_ibits(chunk), _torch_gather(caches, slots, bs))


# ------------------------------------------------------------------ engine
def _row_caches(nb, bs, H, D, dt):
    return [torch.zeros((2, nb, bs, H, D), dtype=dt, device=DEV) for _ in range(L)]


def _rows_scatter(rows, kv, slots, bs):
    for c, (k, v) in zip(rows, kv):
        c[0, slots // bs, slots % bs] = k
        c[1, slots // bs, slots % bs] = v


def _rows_gather(rows, slots, bs):
    return torch.stack([torch.stack([c[0, slots // bs, slots % bs], c[1, slots // bs, slots % bs]]) for c in rows])


@pytest.mark.parametrize("geom", [(2, 128, 16), (1, 64, 8), (2, 64, 32)], ids=lambda g: "H%d_D%d_bs%d" % g)
@pytest.mark.parametrize("backend", ["cachegen-host", "cuda"])
def test_store_paged_and_retrieve_into_paged_nhdb_equal_the_nbhd_path(backend, geom):
    """The same logical KV in an NBHD cache and in a split cache, stored through two engines: retrieve() of both is
    equal (raw backend: equal to the KV itself); retrieve_into_paged("NHDB") into a second split cache equals
    retrieve_into_paged("NBHD") into a row cache, and leaves every other byte of the split cache alone."""
    H, D, bs = geom
    dt, cs, model = torch.bfloat16, 32, "Llama-3-8B"
    nb = _nblocks(bs)
    g = torch.Generator().manual_seed(11)
    tokens = generate_tokens(NTOK, DEV)
    kv = tuple((torch.rand((NTOK, H, D), generator=g).to(dt).to(DEV), torch.rand((NTOK, H, D), generator=g).to(dt).to(DEV))
               for _ in range(L))
    kv_bits = _ibits(torch.stack([torch.stack(p) for p in kv]))
    slots_src = _mapping("offset5", NTOK, nb, bs, g).to(DEV)
    src_rows = _row_caches(nb, bs, H, D, dt)
    _rows_scatter(src_rows, kv, slots_src, bs)
    src_split = _split_caches(H, D, bs, dt, g, nblocks=nb)
    _torch_scatter(src_split, kv_bits, slots_src, bs)
    e_rows = LMCacheEngine(make_cfg(backend, cs), dumb_metadata("vllm", model))
    e_split = LMCacheEngine(make_cfg(backend, cs), dumb_metadata("vllm", model))
    try:
        e_rows.store_paged(tokens, src_rows, slots_src, bs, "NBHD")
        e_split.store_paged(tokens, src_split, slots_src, bs, "NHDB")
        r_rows, m1 = e_rows.retrieve(tokens)
        r_split, m2 = e_split.retrieve(tokens)
        assert int(m1.sum()) == NTOK and int(m2.sum()) == NTOK
        for (k1, v1), (k2, v2), (k, v) in zip(r_rows, r_split, kv):
            assert torch.equal(k1, k2) and torch.equal(v1, v2)
            if backend == "cuda":  # raw chunks: lossless
                assert torch.equal(k2, k) and torch.equal(v2, v)

        def check_retrieve_into(slots_dst, mask, pair):
            dst_split = _split_caches(H, D, bs, dt, g, nblocks=nb)
            expect = [c.clone() for c in dst_split]
            dst_rows = _row_caches(nb, bs, H, D, dt)
            into = [_views(c) for c in dst_split] if pair else dst_split
            ms = e_split.retrieve_into_paged(tokens, into, slots_dst, bs, "NHDB", mask=mask)
            mr = e_rows.retrieve_into_paged(tokens, dst_rows, slots_dst, bs, "NBHD", mask=mask)
            torch.cuda.synchronize()
            nskip = 0 if mask is None else int((~mask).sum())
            assert torch.equal(ms, mr) and int(ms.sum()) == NTOK - nskip and not ms[:nskip].any()
            got_rows = _rows_gather(dst_rows, slots_dst[nskip:], bs)
            assert torch.equal(_torch_gather(dst_split, slots_dst[nskip:], bs), _ibits(got_rows))
            if backend == "cuda":
                assert torch.equal(_ibits(got_rows), kv_bits[:, :, nskip:])
            _torch_scatter(expect, _ibits(got_rows), slots_dst[nskip:], bs)
            for l in range(L):  # the whole cache: unchanged outside the slots of the tokens retrieved
                assert torch.equal(_ibits(dst_split[l]), _ibits(expect[l]))

        check_retrieve_into(_mapping("random", NTOK, nb, bs, g).to(DEV), None, False)
        check_retrieve_into(_mapping("blocks", NTOK, nb, bs, g).to(DEV), None, True)
        mask = torch.ones(NTOK, dtype=torch.bool, device=DEV)
        mask[:37] = False  # a suffix mask that cuts into the second chunk: the first-chunk trim
        check_retrieve_into(_mapping("offset5", NTOK, nb, bs, g).to(DEV), mask, False)
        check_retrieve_into(_mapping("random", NTOK, nb, bs, g).to(DEV), mask, True)
        # unknown tokens: nothing retrieved, the cache keeps every byte
        dst = _split_caches(H, D, bs, dt, g, nblocks=nb)
        keep = [c.clone() for c in dst]
        m = e_split.retrieve_into_paged(tokens + 10000, dst, slots_src, bs, "NHDB")
        torch.cuda.synchronize()
        assert not m.any()
        for c, k in zip(dst, keep):
            assert torch.equal(_ibits(c), _ibits(k))
    finally:
        e_rows.close()
        e_split.close()
