"""The fixed-width HBM tier ("cachegen-fixed") with both budgets and LMCACHE_AMD_FIXED_DEMOTE=1: its LRU group is demoted
by transcoding (lmc_transcode_fixed, then the coded tier's pack leg), served from the pinned pack by the rANS decoder, and
not promoted.  (Without the switch such a backend drops its LRU groups as it always did: test_gpu_fixed_model.py.)
Every comparison of KV is torch.equal on bits against the retrieve before the demotion."""
import ctypes

import pytest
import torch

from lmcache_amd import native
from lmcache_amd.cache_engine import LMCacheEngine
from lmcache_amd.config import LMCacheEngineConfig
from lmcache_amd.storage_backend.local_backend import _DevChunk, _PackChunk
from tests import fixed_model as fm
from tests.test_gpu_engine import dumb_metadata

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
L_, H_, D_, CS, NT = 2, 2, 64, 16, 40   # a prompt is a group of three chunks: 16, 16 and 8 tokens
BS = 16


@pytest.fixture(autouse=True)
def _fixed_tier_demotes(monkeypatch):
    monkeypatch.setenv("LMCACHE_AMD_FIXED_DEMOTE", "1")  # (read when a backend is built)


def _engine(serde="cachegen-fixed", backend="cuda"):
    cfg = LMCacheEngineConfig.from_legacy(chunk_size=CS, backend=backend, local_serde=serde)
    return LMCacheEngine(cfg, dumb_metadata("vllm", "Llama-3-8B"))


def _prompt(seed, n=NT):
    g = torch.Generator().manual_seed(seed)
    tokens = torch.randint(0, 10000, (n,), generator=g).to(DEV) + 20000 * seed
    kv = tuple((torch.randn((n, H_, D_), generator=g).to(torch.bfloat16).to(DEV),
                torch.randn((n, H_, D_), generator=g).to(torch.bfloat16).to(DEV)) for _ in range(L_))
    return tokens, kv


def _keys(eng, tokens):
    return [eng._make_key(h, "vllm") for h in eng._prefix_hashes_of(tokens)]


def _retrieve(eng, tokens):
    kv, mask = eng.retrieve(tokens)
    assert bool(mask.all()) and mask.numel() == len(tokens), "not a full hit"
    return torch.stack([torch.stack(l) for l in kv]).clone().view(torch.int16)


def _retrieve_layerwise(eng, tokens):
    lw = eng.retrieve_layerwise(tokens, layers_per_launch=1)
    for l in range(L_):
        lw.wait_layer(l)
    lw.finish()
    assert bool(lw.ret_mask.all())
    return torch.stack([torch.stack(l) for l in lw.kv]).clone().view(torch.int16)


def _retrieve_paged(eng, tokens, layerwise=False):
    """-> the bits of an "NHBD" cache the prefix was retrieved into (slots from 5 on)."""
    n = len(tokens)
    nb = (n + 5 + BS - 1) // BS + 1
    caches = [torch.zeros((2, nb, H_, BS, D_), dtype=torch.bfloat16, device=DEV) for _ in range(L_)]
    slots = (torch.arange(n, dtype=torch.int64) + 5).to(DEV)
    if layerwise:
        r = eng.retrieve_into_paged_layerwise(tokens, caches, slots, BS, "NHBD", layers_per_launch=1)
        for l in range(L_):
            r.wait_layer(l)
        r.finish()
        mask = r.ret_mask
    else:
        mask = eng.retrieve_into_paged(tokens, caches, slots, BS, "NHBD")
    torch.cuda.synchronize()
    assert bool(mask.all())
    return torch.stack(caches).view(torch.int16)


def _group_bytes(be, lengths=(16, 16, 8)):
    bins = be.cachegen_config.plane_bins(L_)
    return sum(native.r16(native.fixed_blob_bytes(L_, t, H_, D_, bins)) for t in lengths)


def _all_forms(eng, tokens):
    return [_retrieve(eng, tokens), _retrieve_layerwise(eng, tokens), _retrieve_paged(eng, tokens), _retrieve_paged(eng, tokens, True)]


def test_a_fixed_group_is_demoted_served_and_not_promoted():
    fx = _engine()
    be = fx.engine_
    try:
        assert be.model == "fixed" and be.fixed_demotes
        group = _group_bytes(be)
        (ta, kva), (tb, kvb) = _prompt(1), _prompt(2)
        fx.store(ta, kva)
        ka = _keys(fx, ta)
        assert all(isinstance(be.dict[k], _DevChunk) and be.dict[k].model == "fixed" for k in ka)
        refs = _all_forms(fx, ta)
        be.set_capacity(hbm_bytes=group + group // 2, pinned_bytes=1 << 30)
        assert be.tier_stats()["demotions"] == 0 and {be.tier_of(k) for k in ka} == {"hbm"}
        fx.store(tb, kvb)                                   # past the HBM budget: A goes down, transcoded
        kb = _keys(fx, tb)
        st = be.tier_stats()
        assert st["demotions"] == 1 and st["evictions"] == 0
        assert all(be.contains(k) for k in ka + kb)
        assert [be.tier_of(k) for k in ka] == ["pinned"] * 3 and [be.tier_of(k) for k in kb] == ["hbm"] * 3
        assert st["hbm"]["live_bytes"] <= group + group // 2 and st["pinned"]["groups"] == 1
        entries = [be.dict[k] for k in ka]
        assert all(isinstance(e, _PackChunk) and e.pack is entries[0].pack and e.index == i for i, e in enumerate(entries))
        pack = entries[0].pack
        assert st["pinned"]["live_bytes"] == native.r16(pack.blob.nbytes), "the group is filed at the size that landed, not at the bound"
        # byte for byte the pack a pinned cachegen backend stores for the same KV
        cg = _engine("cachegen", backend="cpu")
        try:
            cg.store(ta, kva)
            twin = cg.engine_.dict[_keys(cg, ta)[0]].pack
            assert ctypes.string_at(pack.blob.ptr, pack.blob.nbytes) == ctypes.string_at(twin.blob.ptr, twin.blob.nbytes)
        finally:
            torch.cuda.synchronize()
            cg.close()
        # served where it lies, by the rANS decoder: every form, bit-equal to the retrieve before the demotion
        for got, ref in zip(_all_forms(fx, ta), refs):
            assert torch.equal(got, ref)
        chunk = be.get(ka[1])
        assert torch.equal(chunk.view(torch.int16), refs[0][:, :, CS:2 * CS])
        # ... and not promoted behind the hits
        be.drain()
        st = be.tier_stats()
        assert st["promotions"] == 0 and st["demotions"] == 1 and not be._promoting
        assert all(isinstance(be.dict[k], _PackChunk) for k in ka)
    finally:
        torch.cuda.synchronize()
        fx.close()


def test_a_prefix_half_in_hbm_and_half_demoted():
    fx = _engine()
    be = fx.engine_
    try:
        tokens, kv = _prompt(3, n=4 * CS)
        half = 2 * CS
        fx.store(tokens[:half], tuple((k[:half], v[:half]) for k, v in kv))   # group 1: chunks 0, 1
        fx.store(tokens, kv)                                                  # group 2: chunks 2, 3 (the rest are there)
        keys = _keys(fx, tokens)
        assert len(keys) == 4 and len(be._groups) == 2
        refs = _all_forms(fx, tokens)
        two = _group_bytes(be, (16, 16))
        be.set_capacity(hbm_bytes=two + two // 2, pinned_bytes=1 << 30)       # room for one of the two groups
        st = be.tier_stats()
        assert st["demotions"] == 1 and st["evictions"] == 0
        tiers = [be.tier_of(k) for k in keys]
        assert sorted(tiers) == ["hbm", "hbm", "pinned", "pinned"] and tiers[0] == tiers[1] and tiers[2] == tiers[3]
        for got, ref in zip(_all_forms(fx, tokens), refs):
            assert torch.equal(got, ref)
        be.drain()
        assert be.tier_stats()["promotions"] == 0 and [be.tier_of(k) for k in keys] == tiers
    finally:
        torch.cuda.synchronize()
        fx.close()


def test_a_pinned_budget_too_small_for_the_pack_drops_the_group():
    fx = _engine()
    be = fx.engine_
    try:
        group = _group_bytes(be)
        (ta, kva), (tb, kvb) = _prompt(4), _prompt(5)
        be.set_capacity(hbm_bytes=group + group // 2, pinned_bytes=1024)
        fx.store(ta, kva)
        fx.store(tb, kvb)
        st = be.tier_stats()
        assert st["demotions"] == 0 and st["evictions"] == 1 and st["pinned"]["groups"] == 0
        assert not any(be.contains(k) for k in _keys(fx, ta)) and all(be.tier_of(k) == "hbm" for k in _keys(fx, tb))
    finally:
        torch.cuda.synchronize()
        fx.close()


def test_a_group_larger_than_the_hbm_budget_goes_straight_to_the_pinned_tier_as_a_pack():
    ta, kva = _prompt(9)
    free = _engine()
    try:
        free.store(ta, kva)
        ref = _retrieve(free, ta)
    finally:
        torch.cuda.synchronize()
        free.close()
    fx = _engine()
    be = fx.engine_
    try:
        group = _group_bytes(be)
        be.set_capacity(hbm_bytes=group // 2, pinned_bytes=1 << 30)
        fx.store(ta, kva)
        ka = _keys(fx, ta)
        st = be.tier_stats()
        assert [be.tier_of(k) for k in ka] == ["pinned"] * 3 and all(isinstance(be.dict[k], _PackChunk) for k in ka)
        assert (st["demotions"], st["evictions"], st["hbm"]["groups"], st["pinned"]["groups"]) == (0, 0, 0, 1)
        assert st["pinned"]["live_bytes"] == native.r16(be.dict[ka[0]].pack.blob.nbytes)
        assert torch.equal(_retrieve(fx, ta), ref)
        tb, kvb = _prompt(10)
        be.set_capacity(hbm_bytes=group // 2, pinned_bytes=4096)   # ... and one that fits neither is not cached
        fx.store(tb, kvb)
        assert not any(be.contains(k) for k in _keys(fx, tb))
    finally:
        torch.cuda.synchronize()
        fx.close()


def test_a_transcode_that_flags_a_blob_drops_the_group_and_publishes_nothing():
    fx = _engine()
    be = fx.engine_
    try:
        group = _group_bytes(be)
        (ta, kva), (tb, kvb), (tc, kvc) = _prompt(6), _prompt(7), _prompt(8)
        be.set_capacity(hbm_bytes=group + group // 2, pinned_bytes=1 << 30)
        fx.store(ta, kva)
        ka = _keys(fx, ta)
        blob = be.dict[ka[1]].blob                          # one `lo` byte of A's second chunk, through the entry's tensor
        spot = fm.stream_spans(bytes(blob.cpu().numpy()))[3][0] + 7
        blob[spot] = int(blob[spot]) ^ 0x3c
        torch.cuda.synchronize()
        fx.store(tb, kvb)                                   # A must go down, and its transcode says BAD_STREAM
        st = be.tier_stats()
        assert st["demotions"] == 0 and st["evictions"] == 1
        assert st["pinned"]["groups"] == 0 and st["pinned"]["live_bytes"] == 0
        assert not any(be.contains(k) for k in ka)
        ref_b = _retrieve(fx, tb)
        fx.store(tc, kvc)                                   # the next demotion is a good one
        st = be.tier_stats()
        assert st["demotions"] == 1 and st["evictions"] == 1 and {be.tier_of(k) for k in _keys(fx, tb)} == {"pinned"}
        assert torch.equal(_retrieve(fx, tb), ref_b)
    finally:
        torch.cuda.synchronize()
        fx.close()
