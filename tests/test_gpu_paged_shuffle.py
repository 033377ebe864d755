"""layout "NHBDx" (LMC_PAGED_SHUFFLE): lmc_copy_kv (k_copy_shuffle.h), lmc_kv_deviation, lmc_rope_shift_split and the engine's
staged paths, each against plain torch indexing on the CPU from the layout's two address formulas (include/lmc_hip.h)."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

from lmcache_amd import blend, native
from lmcache_amd.cache_engine import LMCacheEngine
from lmcache_amd.config import LMCacheEngineConfig
from lmcache_amd.rope import RopeShift
from tests.blend_ref import deviation_ref, logical
from tests.test_gpu_blend import _wide_range
from tests.test_gpu_engine import dumb_metadata, generate_tokens
from tests.test_gpu_paged_split import (L, _ibits, _mapping, _random, _row_caches, _rows_gather, _rows_scatter, _split_caches, _views,
                                        ctx)  # noqa: F401  (ctx: the context fixture)

pytestmark = pytest.mark.gpu
DEV, H, MAPPINGS, E4M3 = "cuda:0", 2, ["blocks", "random", "offset5"], torch.float8_e4m3fn


def _pairs(caches):
    """A [2, nb, H, D, bs] allocation per layer, viewed as (key_cache [nb, H, D/x, bs, x], value_cache [nb, H, bs/x, D, x])."""
    x = 16 // caches[0].dtype.itemsize
    return [(c[0].view(*c.shape[1:3], c.shape[3] // x, c.shape[4], x), c[1].view(*c.shape[1:3], c.shape[4] // x, c.shape[3], x))
            for c in caches]


def _cpu_bits(pairs):
    return [(_ibits(k).cpu(), _ibits(v).cpu()) for k, v in pairs]


def _ref_gather(pairs, slots, bs):
    """-> [L, 2, T, H, D] (integer bits, CPU): K(t, h, d) = kc[b, h, d / x, w, d % x], V(t, h, d) = vc[b, h, w / x, d, w % x]."""
    blk, off, x = slots.cpu() // bs, slots.cpu() % bs, pairs[0][0].shape[-1]
    return torch.stack([torch.stack([kc[blk, :, :, off, :].flatten(2), vc[blk, :, off // x, :, off % x]]) for kc, vc in _cpu_bits(pairs)])


def _ref_scatter(cpu_pairs, chunk_bits, slots, bs):
    """chunk_bits [L, 2, T, H, D] into the CPU copies (_cpu_bits) of every layer's pair, by the same two formulas."""
    blk, off, x = slots.cpu() // bs, slots.cpu() % bs, cpu_pairs[0][0].shape[-1]
    for (kc, vc), (k, v) in zip(cpu_pairs, chunk_bits.cpu()):
        kc[blk, :, :, off, :], vc[blk, :, off // x, :, off % x] = k.unflatten(2, (-1, x)), v


def _whole_cache_equals(pairs, cpu_pairs):
    return all(torch.equal(a, b) for got, want in zip(_cpu_bits(pairs), cpu_pairs) for a, b in zip(got, want))


@pytest.mark.parametrize("mapping", MAPPINGS)
@pytest.mark.parametrize("dt,D,bs", [(torch.bfloat16, 64, 16), (torch.bfloat16, 128, 32), (torch.float16, 64, 8), (E4M3, 64, 16),
                                     (E4M3, 128, 32)], ids=lambda v: str(v).replace("torch.", ""))
def test_gather_and_scatter_equal_torch_indexing(ctx, dt, D, bs, mapping):  # noqa: F811
    ntok, nb = 77, 82 // bs + 3  # ragged first and last tiles
    g = torch.Generator().manual_seed(D + bs + MAPPINGS.index(mapping))
    pairs = _pairs(_split_caches(H, D, bs, dt, g, nblocks=nb))
    slots = _mapping(mapping, ntok, nb, bs, g).to(DEV)
    lay = native.KVLayout.paged(pairs, slots, bs, "NHBDx")
    chunk = torch.zeros((L, 2, ntok, H, D), dtype=dt, device=DEV)
    ctx.copy_kv(lay, 0, ntok, native.KVLayout.from_chunk(chunk, "vllm"), 0)
    torch.cuda.synchronize()
    assert torch.equal(_ibits(chunk).cpu(), _ref_gather(pairs, slots, bs))
    # scatter over a fixed byte pattern: the WHOLE cache equals the reference (only the given slots were written)
    for t in (t for p in pairs for t in p):
        t.view(torch.uint8).fill_(0xA5)
    expect, new = _cpu_bits(pairs), _random((L, 2, ntok, H, D), dt, g).to(DEV)
    _ref_scatter(expect, _ibits(new), slots, bs)
    ctx.copy_kv(native.KVLayout.from_chunk(new, "vllm"), 0, ntok, lay, 0)
    torch.cuda.synchronize()
    assert _whole_cache_equals(pairs, expect)


def test_refusals_launch_nothing(ctx):  # noqa: F811
    D, bs, dt, ntok, nb, INVALID = 64, 16, torch.bfloat16, 40, 4, -1
    g = torch.Generator().manual_seed(5)
    slots = _mapping("blocks", ntok, nb, bs, g).to(DEV)
    caches, others = _split_caches(H, D, bs, dt, g, nblocks=nb), _split_caches(H, D, bs, dt, g, nblocks=nb)
    before = [c.clone() for c in caches + others]
    lay, other = (native.KVLayout.paged(_pairs(c), slots, bs, "NHBDx").struct for c in (caches, others))
    split = native.KVLayout.paged(others, slots, bs, "NHDB").struct
    chunk = torch.zeros((L, 2, ntok, H, D), dtype=dt, device=DEV)
    rows = native.KVLayout.from_chunk(chunk, "vllm").struct
    odd_bs, no_slots = (native.KvLayoutStruct.from_buffer_copy(lay) for _ in range(2))
    odd_bs.block_size, no_slots.slot_mapping = 12, None  # block_size % x != 0; a missing slot mapping; both sides shuffled; against split
    for a, b in ((odd_bs, rows), (no_slots, rows), (lay, other), (lay, split), (split, lay)):
        assert native.lib().lmc_copy_kv(ctx.handle, ctypes.byref(a), 0, ntok, ctypes.byref(b), 0,
                                        native.current_stream_ptr(torch.device(DEV))) == INVALID
    k12 = torch.zeros((nb, H, D // 8, 12, 8), dtype=dt, device=DEV)
    with pytest.raises(ValueError, match="multiple of x"):
        native.KVLayout.paged([(k12, k12.view(nb, H, 1, D, 12))], slots, 12, "NHBDx")
    with pytest.raises(ValueError, match="value_cache"):  # a value cache of NHDB shape
        native.KVLayout.paged([_views(c) for c in caches], slots, bs, "NHBDx")
    cfg = LMCacheEngineConfig.from_legacy(chunk_size=32, backend="cuda", local_serde="cachegen")
    with contextlib.closing(LMCacheEngine(cfg, dumb_metadata("vllm", "Llama-3-8B"))) as engine:
        for call in (engine.store_paged, engine.retrieve_into_paged):
            with pytest.raises(ValueError, match="direct=True"):
                call(generate_tokens(ntok, DEV), _pairs(caches), slots, bs, "NHBDx", direct=True)
    torch.cuda.synchronize()
    assert not chunk.any() and all(torch.equal(_ibits(c), _ibits(b)) for c, b in zip(caches + others, before))


@pytest.mark.parametrize("mapping", MAPPINGS)
@pytest.mark.parametrize("dt,h,D,bs", [(torch.bfloat16, 2, 128, 16), (torch.float16, 1, 64, 8)], ids=["bf16_H2_D128_bs16", "fp16_H1_D64_bs8"])
def test_deviation_is_within_the_bound_of_float64(ctx, dt, h, D, bs, mapping):  # noqa: F811
    """Per plane |dev - ref64| <= (C + 3) 2^-24 ref64, "kv": (2 C + 3) 2^-24: test_gpu_blend.py's derived bound for the "NHDB" tile
    form (test_deviation_is_within_the_derived_bound_of_float64).  On `random` slots the bits equal those on an "NBHD" cache of the
    same KV: K is the GROUP form on both, V the tile form's token-by-token path, which folds the C / 8 <= 64 partial sums in its tree."""
    ntok, nb, C = 77, 82 // bs + 3, h * D
    g = torch.Generator().manual_seed(17 + D + MAPPINGS.index(mapping))
    fresh, cached = _wide_range((1, 2, ntok, h, D), dt, g), _wide_range((1, 2, ntok, h, D), dt, g)
    slots = _mapping(mapping, ntok, nb, bs, g).to(DEV)
    pairs = _pairs([torch.zeros((2, nb, h, D, bs), dtype=dt, device=DEV)])
    cpu = _cpu_bits(pairs)
    _ref_scatter(cpu, _ibits(cached), slots, bs)
    for dst, src in zip(pairs[0], cpu[0]):
        _ibits(dst).copy_(src)
    fk, fv = fresh[0, 0].to(DEV), fresh[0, 1].to(DEV)
    got = {p: blend.kv_deviation(fk, fv, pairs, 0, slots, bs, "NHBDx", planes=p).cpu().numpy() for p in ("k", "v", "kv")}
    ref = [deviation_ref(logical(fresh), 0, 0, logical(cached), 0, 0, ntok, kv) for kv in (0, 1)]
    for p, r, n in (("k", ref[0], C), ("v", ref[1], C), ("kv", ref[0] + ref[1], 2 * C)):
        assert (np.abs(got[p].astype(np.float64) - r) <= (n + 3) * 2.0 ** -24 * r).all(), p
    if mapping == "random":
        rows = [torch.zeros((2, nb, bs, h, D), dtype=dt, device=DEV)]
        _rows_scatter(rows, [(cached[0, 0].to(DEV), cached[0, 1].to(DEV))], slots, bs)
        for p in ("k", "v"):
            same = blend.kv_deviation(fk, fv, rows, 0, slots, bs, "NBHD", planes=p).cpu().numpy()
            assert np.array_equal(same.view(np.uint32), got[p].view(np.uint32)), p


def _rope(per_token, ntok):
    delta = (torch.arange(ntok, dtype=torch.int32) % 23 - 9).to(DEV) if per_token else 7
    return RopeShift.from_base(10000.0, 64, 64, DEV, delta=delta)


@pytest.mark.parametrize("serde", ["cachegen", "cachegen-fixed"])
def test_store_paged_and_retrieve_into_paged_equal_the_nbhd_path(ctx, serde):  # noqa: F811
    """The same KV stored from an "NBHD" and from an "NHBDx" cache (an engine each) and retrieved into a second cache of the layout:
    read by reference indexing, the shuffled cache holds the NBHD cache's bits, and every other byte of it is untouched."""
    D, bs, dt, ntok, nb = 64, 16, torch.bfloat16, 300, 22
    g = torch.Generator().manual_seed(23)
    tokens = generate_tokens(ntok, DEV)
    kv = tuple(tuple(torch.rand((ntok, H, D), generator=g).to(dt).to(DEV) for _ in "kv") for _ in range(L))
    slots_src = _mapping("offset5", ntok, nb, bs, g).to(DEV)
    src_rows, src_pairs = _row_caches(nb, bs, H, D, dt), _pairs(_split_caches(H, D, bs, dt, g, nblocks=nb))
    _rows_scatter(src_rows, kv, slots_src, bs)
    ctx.copy_kv(native.KVLayout.from_kv_tuple(kv, "vllm"), 0, ntok, native.KVLayout.paged(src_pairs, slots_src, bs, "NHBDx"), 0)
    assert torch.equal(_ref_gather(src_pairs, slots_src, bs), _ibits(torch.stack([torch.stack(p) for p in kv])).cpu())
    cfg = LMCacheEngineConfig.from_legacy(chunk_size=256, backend="cuda", local_serde=serde)  # one full chunk and a ragged one
    with contextlib.closing(LMCacheEngine(cfg, dumb_metadata("vllm", "Llama-3-8B"))) as e_rows, \
            contextlib.closing(LMCacheEngine(cfg, dumb_metadata("vllm", "Llama-3-8B"))) as e_shuf:
        e_rows.store_paged(tokens, src_rows, slots_src, bs, "NBHD")
        e_shuf.store_paged(tokens, src_pairs, slots_src, bs, "NHBDx")
        for rope, layerwise in ((None, False), (_rope(False, ntok), False), (_rope(True, ntok), False), (_rope(True, ntok), True)):
            slots = _mapping("blocks" if layerwise else "random", ntok, nb, bs, g).to(DEV)
            dst_rows, dst_pairs = _row_caches(nb, bs, H, D, dt), _pairs(_split_caches(H, D, bs, dt, g, nblocks=nb))
            expect = _cpu_bits(dst_pairs)
            mr = e_rows.retrieve_into_paged(tokens, dst_rows, slots, bs, "NBHD", rope=rope)
            if layerwise:
                r = e_shuf.retrieve_into_paged_layerwise(tokens, dst_pairs, slots, bs, "NHBDx", rope=rope, layers_per_launch=1)
                r.finish()
                torch.cuda.synchronize()  # two layer ranges, and each range's event has fired
                assert [end for end, _ in r.layer_events] == [1, 2] and all(ev.query() for _, ev in r.layer_events)
                ms = r.ret_mask
            else:
                ms = e_shuf.retrieve_into_paged(tokens, dst_pairs, slots, bs, "NHBDx", rope=rope)
            torch.cuda.synchronize()
            got_rows = _ibits(_rows_gather(dst_rows, slots, bs)).cpu()
            assert torch.equal(ms, mr) and int(ms.sum()) == ntok and torch.equal(_ref_gather(dst_pairs, slots, bs), got_rows)
            _ref_scatter(expect, got_rows, slots, bs)
            assert _whole_cache_equals(dst_pairs, expect)


@pytest.mark.parametrize("mapping", ["blocks", "random"])
def test_rope_shift_split_rotates_the_keys_as_in_the_nhdb_cache(ctx, mapping):  # noqa: F811
    D, bs, dt, ntok, nb = 64, 16, torch.float16, 77, 9
    g = torch.Generator().manual_seed(31)
    pairs = _pairs([torch.rand((2, nb, H, D, bs), generator=g).to(dt).to(DEV) for _ in range(L)])
    nhdb = [(k.clone(), v.clone().view(nb, H, D, bs)) for k, v in pairs]  # the same keys under an "NHDB" layout
    before = [(k.clone(), v.clone()) for k, v in pairs]
    slots, r = _mapping(mapping, ntok, nb, bs, g).to(DEV), _rope(True, ntok)
    for caches, layout in ((pairs, "NHBDx"), (nhdb, "NHDB")):
        ctx.rope_shift_split(native.KVLayout.paged(caches, slots, bs, layout), 0, ntok, r.cos_sin, r.rot_dim, r.is_neox, deltas=r.delta)
    torch.cuda.synchronize()
    assert ctx.status(clear=True) == 0
    for (k, v), (k2, _), (kb, vb) in zip(pairs, nhdb, before):
        assert torch.equal(_ibits(k), _ibits(k2)) and not torch.equal(_ibits(k), _ibits(kb)) and torch.equal(_ibits(v), _ibits(vb))
