"""The fixed-width HBM tier ("cachegen-fixed") with both budgets, LMCACHE_AMD_FIXED_DEMOTE=1 and LMCACHE_AMD_FIXED_PROMOTE=1:
a demoted group that is hit is served from its pinned pack by the rANS decoder and then PROMOTED on the worker thread --
the pack unpacked into the codec's staging, lmc_transcode_to_fixed into the HBM arena -- and is a fixed-width group again.
(With the first switch alone it stays where it lies: test_gpu_fixed_tiering.py.)  Every comparison of KV is torch.equal
on bits against the retrieve before the demotion."""
import ctypes

import pytest
import torch

from lmcache_amd import native
from lmcache_amd.storage_backend.local_backend import _DevChunk, _PackChunk
from tests import fixed_model as fm
from tests.test_gpu_fixed_tiering import CS, DEV, D_, H_, L_, _all_forms, _engine, _group_bytes, _keys, _prompt, _retrieve

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _fixed_tier_demotes_and_promotes(monkeypatch):
    monkeypatch.setenv("LMCACHE_AMD_FIXED_DEMOTE", "1")   # (both read when a backend is built)
    monkeypatch.setenv("LMCACHE_AMD_FIXED_PROMOTE", "1")


def _is_fixed_blob(e, T):
    """The entry is a fixed-width HBM chunk whose blob checks out as one (header, bins, directory, every check word)."""
    assert isinstance(e, _DevChunk) and e.model == "fixed"
    blob = bytes(e.blob.cpu().numpy())
    h = fm.header(blob)
    assert int(h[fm.W_MODEL]) == fm.MODEL_FIXED and int(h[fm.W_T]) == T and int(h[fm.W_TOTAL]) == len(blob)
    fm.unpack_symbols(blob)  # (asserts every stream's check word and tail)


@pytest.mark.parametrize("n", [2 * CS + 8, 11], ids=["three-chunks", "one-chunk"])
def test_a_demoted_group_that_is_hit_is_promoted_back(n):
    lengths = [min(CS, n - i) for i in range(0, n, CS)]
    fx = _engine()
    be = fx.engine_
    try:
        assert be.model == "fixed" and be.fixed_demotes and be.fixed_promotes
        group = _group_bytes(be, lengths)
        (ta, kva), (tb, kvb) = _prompt(1, n), _prompt(2, n)
        fx.store(ta, kva)
        ka = _keys(fx, ta)
        refs = _all_forms(fx, ta)
        first = [bytes(be.dict[k].blob.cpu().numpy()) for k in ka]
        hbm = group + group // 2
        be.set_capacity(hbm_bytes=hbm, pinned_bytes=1 << 30)
        fx.store(tb, kvb)                                   # past the HBM budget: A goes down, transcoded
        kb = _keys(fx, tb)
        ref_b = _retrieve(fx, tb)                           # (B is the hotter group now ... )
        st = be.tier_stats()
        assert st["demotions"] == 1 and st["promotions"] == 0 and {be.tier_of(k) for k in ka} == {"pinned"}
        assert all(isinstance(be.dict[k], _PackChunk) for k in ka)
        got = _retrieve(fx, ta)                             # ( ... until this hit) served from the pinned tier
        assert torch.equal(got, refs[0])
        be.drain()
        st = be.tier_stats()
        assert st["promotions"] == 1 and not be._promoting
        assert [be.tier_of(k) for k in ka] == ["hbm"] * len(ka)
        for k, T, was in zip(ka, lengths, first):
            _is_fixed_blob(be.dict[k], T)
            assert bytes(be.dict[k].blob.cpu().numpy()) == was, "the promoted blob is the blob the store wrote"
        # a colder group went down to make room, and both tiers are within budget
        assert st["demotions"] == 2 and st["evictions"] == 0 and {be.tier_of(k) for k in kb} == {"pinned"}
        assert st["hbm"]["live_bytes"] <= hbm and st["pinned"]["live_bytes"] <= 1 << 30
        assert st["hbm"]["groups"] == 1 and st["pinned"]["groups"] == 1
        for got, ref in zip(_all_forms(fx, ta), refs):      # from HBM again, by the fixed-width decoder: every form
            assert torch.equal(got, ref)
        assert torch.equal(_retrieve(fx, tb), ref_b)
    finally:
        torch.cuda.synchronize()
        fx.close()


def test_a_prefix_half_promoted_and_half_still_demoted():
    fx = _engine()
    be = fx.engine_
    try:
        tokens, kv = _prompt(3, n=4 * CS)
        half = 2 * CS
        fx.store(tokens[:half], tuple((k[:half], v[:half]) for k, v in kv))   # group 1: chunks 0, 1
        fx.store(tokens, kv)                                                  # group 2: chunks 2, 3
        keys = _keys(fx, tokens)
        refs = _all_forms(fx, tokens)
        ref_half = _retrieve(fx, tokens[:half])
        two = _group_bytes(be, (16, 16))
        be.set_capacity(hbm_bytes=two // 2, pinned_bytes=1 << 30)             # both groups go down ...
        assert [be.tier_of(k) for k in keys] == ["pinned"] * 4 and be.tier_stats()["demotions"] == 2
        be.set_capacity(hbm_bytes=two + two // 2, pinned_bytes=1 << 30)       # ... and there is room for one to return
        assert torch.equal(_retrieve(fx, tokens[:half]), ref_half)            # a hit on group 1 alone
        be.drain()
        assert [be.tier_of(k) for k in keys] == ["hbm", "hbm", "pinned", "pinned"] and be.tier_stats()["promotions"] == 1
        assert all(be.dict[k].model == "fixed" for k in keys[:2])
        be._promote_group = lambda gid: be._promoting.discard(gid)            # (the whole-prefix hits must not move group 2)
        for got, ref in zip(_all_forms(fx, tokens), refs):                    # a fixed-width run and a pack run
            assert torch.equal(got, ref)
        be.drain()
        assert [be.tier_of(k) for k in keys] == ["hbm", "hbm", "pinned", "pinned"]
    finally:
        torch.cuda.synchronize()
        fx.close()


def test_a_pack_damaged_in_pinned_memory_is_not_published():
    fx = _engine()
    be = fx.engine_
    try:
        group = _group_bytes(be)
        (ta, kva), (tb, kvb) = _prompt(6), _prompt(7)
        be.set_capacity(hbm_bytes=group + group // 2, pinned_bytes=1 << 30)
        fx.store(ta, kva)
        ka = _keys(fx, ta)
        fx.store(tb, kvb)                                   # A goes down
        ref_b = _retrieve(fx, tb)
        assert {be.tier_of(k) for k in ka} == {"pinned"}
        pack = be.dict[ka[0]].pack
        h = native.pack_info(pack.blob.ptr, pack.blob.nbytes)
        # one bit of a scale in chunk 1's static slot (a blob's [0, off_streams) as it was): the unpack copies the slot --
        # it checks header and directory -- and the transcode's scale checksum says BAD_SCALES
        raw = torch.frombuffer((ctypes.c_uint8 * pack.blob.nbytes).from_address(pack.blob.ptr), dtype=torch.uint8)
        slot = int(h.off_static) + int(h.static_stride)
        head = fm.header(bytes(raw[slot:slot + 128].numpy()))
        assert int(head[fm.W_T]) == CS and int(head[fm.W_MODEL]) != fm.MODEL_FIXED
        spot = slot + int(head[fm.W_OFF_SCALES]) + 2 * 5
        raw[spot] = int(raw[spot]) ^ 0x04
        with be._tier_lock:
            be._touch(ka)                                   # (a hit's bookkeeping without its decode of the damaged pack)
        be.drain()
        st = be.tier_stats()
        assert st["promotions"] == 0 and not be._promoting
        for k in ka:  # left in the pinned tier, or dropped: never an HBM entry made of unchecked bytes
            assert be.tier_of(k) in ("pinned", None)
        assert st["hbm"]["live_bytes"] <= group + group // 2
        # (room was made before the transcode said no: B may have gone down for it -- it is still there, bit for bit)
        assert all(be.contains(k) for k in _keys(fx, tb)) and torch.equal(_retrieve(fx, tb), ref_b)
    finally:
        torch.cuda.synchronize()
        fx.close()
