"""Planes of more than 1024 channels read straight from vLLM's ROCm paged-attention cache ("NHDB") under
LMCACHE_AMD_SPLIT_WIDE=1: k_quantize.h's WIDE split tasks behind lmc_encode_chunks_split and lmc_encode_chunks_fixed_split,
and store_paged(direct=True) above them.  The yardstick is the contiguous path, which runs none of that code: the blobs
coded from the cache are byte for byte the blobs coded from the rows.  No tolerance anywhere."""
import ctypes
import itertools

import pytest
import torch

from lmcache_amd import native
from tests.test_gpu_engine import generate_tokens
from tests.test_gpu_fixed_split import _engine
from tests.test_gpu_paged_split import DEV, L, _ibits, _mapping, _nblocks, _split_caches, _torch_gather, _torch_scatter

pytestmark = pytest.mark.gpu

CS, T = 16, 19           # a full chunk and a ragged one of 3 tokens: one ragged oct
BINS = [32, 16, 16, 32]  # K of layer 0 / 1, V of layer 0 / 1: a byte (wide) and a nibble (narrow) plane on each side
BF16, FP16, E4M3 = torch.bfloat16, torch.float16, torch.float8_e4m3fn
# C = 1032: SPLIT 2, the second slice one 8-channel run; 2048: SPLIT 2 full; 2056: SPLIT 4, a one-run third slice and an
# empty fourth; 4096: SPLIT 4 full
GEOMS = [(43, 24), (16, 128), (257, 8), (32, 128)]
# (block size, mapping): block-ordered runs (the V form), the same at block size 12 (no V form), every token in another block
SLOTS = [(16, "blocks"), (12, "blocks"), (16, "random")]
CASES = list(itertools.product(GEOMS, SLOTS, (0, 5), (BF16, FP16), (False, True))) + [((16, 128), (16, "blocks"), 5, E4M3, False)]


@pytest.fixture(autouse=True)
def wide_on(monkeypatch):
    monkeypatch.setenv("LMCACHE_AMD_SPLIT_WIDE", "1")
    native.build()


@pytest.mark.parametrize("geom,slots,tb,dt,fixed", CASES,
                         ids=["H%dD%d-bs%d%s-tb%d-%s-%s" % (g + s + (tb, str(dt)[6:], "fixed" if f else "coded")) for g, s, tb, dt, f in CASES])
def test_blobs_from_the_wide_split_cache_equal_those_from_the_rows(geom, slots, tb, dt, fixed):
    (H, D), (bs, kind), ctx = geom, slots, native.get_context(0)
    g = torch.Generator().manual_seed(H + D + bs + tb)
    x = torch.randn((L, 2, tb + T, H, D), generator=g).to(BF16)
    x[:, :, tb + 9] = 0                       # an all-zero token, an inf and a NaN (e4m3fn: the cast's NaN) in every plane
    x[:, :, tb + 2, H - 1, D - 1] = float("inf")
    x[:, :, tb + T - 1, 0, 3] = float("nan")
    x = x.to(dt).to(DEV)
    nb = _nblocks(bs)
    caches = _split_caches(H, D, bs, dt, g, nblocks=nb)
    slot_map = _mapping(kind, tb + T, nb, bs, g).to(DEV)
    _torch_scatter(caches, _ibits(x), slot_map, bs)
    stride, out = native.r16(native.blob_bound(L, CS, H, D)), []
    for layout, fn in ((native.KVLayout.paged(caches, slot_map, bs, "NHDB"), ctx.encode_chunks_fixed_split if fixed else ctx.encode_chunks_split),
                       (native.KVLayout.from_chunk(x, "vllm"), ctx.encode_chunks_fixed if fixed else ctx.encode_chunks)):
        blobs = torch.zeros(2 * stride, dtype=torch.uint8, device=DEV)
        sizes = torch.zeros(2, dtype=torch.int32, device=DEV)
        fn(layout, tb, tb + T, CS, BINS, blobs.data_ptr(), stride, sizes.data_ptr())
        torch.cuda.synchronize()
        ctx.raise_on_status("encode")
        out.append((sizes.cpu().tolist(), blobs.cpu()))
    (sz_s, b_s), (sz_r, b_r) = out
    assert sz_s == sz_r and all(sz_s)
    for i in range(2):
        assert torch.equal(b_s[i * stride:i * stride + sz_s[i]], b_r[i * stride:i * stride + sz_r[i]]), f"chunk {i}"


@pytest.mark.parametrize("serde", ["cachegen", "cachegen-fixed"])
def test_store_paged_direct_round_trip_equals_the_store_from_rows(serde):
    H, D, bs, n = 32, 128, 16, 70
    g, nb = torch.Generator().manual_seed(5), _nblocks(16)
    x = torch.rand((L, 2, n, H, D), generator=g).to(BF16).to(DEV)
    src, slots = _split_caches(H, D, bs, BF16, g, nblocks=nb), _mapping("offset5", n, nb, bs, g).to(DEV)
    _torch_scatter(src, _ibits(x), slots, bs)
    tokens, got = generate_tokens(n, DEV), []
    for store in (lambda e: e.store_paged(tokens, src, slots, bs, "NHDB", direct=True), lambda e: e.store(tokens, tuple((l[0], l[1]) for l in x))):
        e = _engine(serde)
        try:
            assert e.split_wide
            store(e)
            dst = _split_caches(H, D, bs, BF16, g, nblocks=nb)
            assert int(e.retrieve_into_paged(tokens, dst, slots, bs, "NHDB", direct=True).sum()) == n
            torch.cuda.synchronize()
            got.append(_torch_gather(dst, slots, bs))
        finally:
            e.close()
    assert torch.equal(got[0], got[1])


def test_wider_than_4096_channels_and_fp8_on_the_fixed_call_are_still_refused():
    lib, ctx, st = native.lib(), native.get_context(0), native.current_stream_ptr(torch.device(DEV))
    g, bins = torch.Generator().manual_seed(3), (ctypes.c_int32 * (2 * L))(*BINS)
    slots = _mapping("blocks", T, _nblocks(16), 16, g).to(DEV)
    for fn, H, D, dt in ((lib.lmc_encode_chunks_split, 513, 8, BF16), (lib.lmc_encode_chunks_fixed_split, 513, 8, BF16),
                         (lib.lmc_encode_chunks_fixed_split, 16, 128, E4M3)):
        layout = native.KVLayout.paged(_split_caches(H, D, 16, dt, g), slots, 16, "NHDB")
        stride = native.r16(native.blob_bound(L, CS, H, D))
        blobs = torch.zeros(2 * stride, dtype=torch.uint8, device=DEV)
        sizes = torch.full((2,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
        rc = fn(ctx.handle, ctypes.byref(layout.struct), 0, T, CS, bins, blobs.data_ptr(), stride, sizes.data_ptr(), None, st)
        torch.cuda.synchronize()
        assert rc == -1 and bool((sizes == 0x5A5A5A5A).all()), (H, D, dt)
