"""lmc_transcode_fixed and the fixed-width tier's demotion, on the host: the export and its binding, the codec's model
tables and demote dispatch, the backend's demote callback, its bound for a pack that has not been transcoded yet, and the
gate that keeps a demoted fixed-width group from being promoted.  No GPU: the library is loaded for its symbols only, the
context and the codec are made without their constructors."""
import ctypes
import re
import threading
import types

import pytest
import torch

from lmcache_amd import native
from lmcache_amd.config import LMCacheEngineConfig, LMCacheEngineMetadata
from lmcache_amd.storage_backend import local_backend as lb
from lmcache_amd.storage_backend.serde.cachegen_device import CacheGenDeviceCodec

STREAM, STATUS = 0x5700, 0x57A7
# (H, D, chunk_tokens, tokens) of tests/test_gpu_transcode.py's cases, L = 2
GEOMETRIES = [(2, 64, 256, 512), (2, 64, 32, 96), (2, 64, 16, 48), (2, 64, 256, 261), (2, 64, 256, 257), (2, 64, 257, 357),
              (2, 64, 32, 45), (2, 64, 32, 62), (3, 64, 256, 261), (3, 64, 64, 128), (1, 72, 64, 141), (16, 128, 32, 32)]


def test_the_symbol_is_exported_with_the_argument_types_the_binding_declares():
    fn = getattr(native.lib(), "lmc_transcode_fixed")
    res, args = native.SYMBOLS["lmc_transcode_fixed"]
    assert fn.restype is res and list(fn.argtypes) == list(args)
    text = open(native.INCLUDE + "/lmc_hip.h").read()
    m = re.search(r"\bint\s+lmc_transcode_fixed\s*\((.*?)\)\s*;", text, re.S)
    params = [re.findall(r"\w+", p)[-1] for p in m.group(1).split(",")]
    assert params == ["ctx", "blob_ptrs", "blob_bytes", "nchunks", "L", "H", "D", "dtype", "chunk_tokens", "ntokens", "bins_h",
                      "blobs_out", "blob_stride", "sizes", "job_status", "stream"]
    assert len(args) == len(params)
    u32, u64 = ctypes.c_uint32, ctypes.c_uint64
    assert args[params.index("ntokens")] is u32 and args[params.index("blob_stride")] is u64
    assert all(args[params.index(p)] is ctypes.c_int32 for p in ("nchunks", "L", "H", "D", "dtype", "chunk_tokens"))
    assert native.lib().lmc_abi_version() == 6


def test_the_wrapper_calls_its_symbol_once_with_the_job_behind_the_source(monkeypatch):
    calls = []

    class Rec:
        def __getattr__(self, name):
            if name not in native.SYMBOLS:
                raise AttributeError(name)
            return lambda *a: calls.append((name, a)) or 0
    monkeypatch.setattr(native, "lib", lambda: Rec())
    c = native.Context.__new__(native.Context)
    c.device, c.handle = 0, ctypes.c_void_p(0xC0DE)
    try:
        bins = [16, 32, 17, 18]
        n = c.transcode_fixed(0x7AB1E, 0xB17E5, 3, 2, 2, 64, native.BF16, 256, 700, bins, 0xB10B, 4096, 0x5123, None,
                              stream=STREAM, status_ptr=STATUS)
        assert n == 3 and [name for name, _ in calls] == ["lmc_transcode_fixed"]
        a = calls[0][1]
        assert a[0].value == 0xC0DE and a[1:10] == (0x7AB1E, 0xB17E5, 3, 2, 2, 64, native.BF16, 256, 700)
        assert list(a[10]) == bins and a[11:] == (0xB10B, 4096, 0x5123, STATUS, STREAM)
        with pytest.raises(AssertionError):  # 700 tokens are three chunks of 256, not two
            c.transcode_fixed(0x7AB1E, 0xB17E5, 2, 2, 2, 64, native.BF16, 256, 700, bins, 0xB10B, 4096, 0x5123, None, stream=STREAM)
    finally:
        c.handle = None


def _codec(ctx):
    codec = CacheGenDeviceCodec.__new__(CacheGenDeviceCodec)
    codec.ctx, codec._lock = ctx, threading.RLock()
    return codec


def test_the_model_tables_and_the_demote_dispatch():
    ctx = types.SimpleNamespace(**{name: object() for name in
                                   ("encode_chunks", "encode_chunks_split", "encode_chunks_fixed", "encode_chunks_fixed_split",
                                    "decode_chunks_fixed_schedule", "decode_chunks_fixed_split_schedule", "transcode_fixed")})
    codec = _codec(ctx)
    rows = native.KVLayout(native.KvLayoutStruct(), [], 64, torch.device("cpu"))
    split = native.KVLayout(native.KvLayoutStruct(paged_kind=native.PAGED_SPLIT), [], 64, torch.device("cpu"))
    for model in (None, "fixed"):
        for lay, is_split in ((rows, False), (split, True)):
            assert codec._entry(codec._ENCODERS, model, lay) is getattr(ctx, codec._ENCODERS[(model, is_split)])
    with pytest.raises(ValueError):
        codec._entry(codec._ENCODERS, "rans", rows)
    assert codec._DEMOTERS == {None: None, "fixed": "transcode_fixed"} and callable(CacheGenDeviceCodec.transcode_fixed)
    # demote_blobs: a fixed-width group is transcoded first and the pack leg takes the coded blobs, behind no event;
    # a coded group goes to the pack leg as it is
    seen = []
    codec.transcode_fixed = lambda blobs, geo, cs, nt, bins, ready=(): seen.append(("transcode", blobs, geo, cs, nt, bins, ready)) or ["c0", "c1"]
    codec._pack_out = lambda blobs, geo, cs, nt, arena, ready=(): seen.append(("pack", blobs, geo, cs, nt, arena, ready)) or "pack"
    assert codec.demote_blobs(["f0", "f1"], (2, 2, 64), 16, 24, "arena", ready=["ev"], model="fixed", bins=[16] * 4) == "pack"
    assert seen == [("transcode", ["f0", "f1"], (2, 2, 64), 16, 24, [16] * 4, ["ev"]), ("pack", ["c0", "c1"], (2, 2, 64), 16, 24, "arena", ())]
    del seen[:]
    assert codec.demote_blobs(["b0", "b1"], (2, 2, 64), 16, 24, "arena", ready=["ev"]) == "pack"
    assert seen == [("pack", ["b0", "b1"], (2, 2, 64), 16, 24, "arena", ["ev"])]
    with pytest.raises(ValueError):
        codec.demote_blobs(["b0"], (2, 2, 64), 16, 16, "arena", model="lossless")
    assert seen == [("pack", ["b0", "b1"], (2, 2, 64), 16, 24, "arena", ["ev"])]
    # the table IS the dispatch: another method under "fixed" is the one that runs
    codec._DEMOTERS = {None: None, "fixed": "other"}
    codec.other = lambda *a: seen.append("other") or ["o"]
    codec.demote_blobs(["f0"], (2, 2, 64), 16, 16, "arena", model="fixed", bins=[16] * 4)
    assert seen[1:] == ["other", ("pack", ["o"], (2, 2, 64), 16, 16, "arena", ())]


@pytest.fixture
def make_backend(monkeypatch):
    monkeypatch.setattr(native, "lib", lambda: None)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    monkeypatch.delenv("LMCACHE_AMD_HBM_BYTES", raising=False)
    monkeypatch.delenv("LMCACHE_AMD_PINNED_BYTES", raising=False)
    made = []

    def make(serde, demote="1"):
        if demote is None:
            monkeypatch.delenv("LMCACHE_AMD_FIXED_DEMOTE", raising=False)
        else:
            monkeypatch.setenv("LMCACHE_AMD_FIXED_DEMOTE", demote)
        cfg = LMCacheEngineConfig.from_legacy(chunk_size=16, backend="cuda", local_serde=serde)
        be = lb.LMCLocalBackend(cfg, LMCacheEngineMetadata("Llama-3-8B", 1, 0, "vllm", "bfloat16"))
        made.append(be)
        return be
    yield make
    for be in made:
        be.close()


@pytest.mark.parametrize("serde,model", [("cachegen", "rans"), ("cachegen-fixed", "fixed")])
def test_tiers_gets_a_demote_callback_for_either_model(make_backend, serde, model):
    be = make_backend(serde)
    assert be.model == model and be._tiers._demote is not None and be._tiers._demote == be._demote_group
    assert not be._tiers.tiered()
    be._tiers.budget["hbm"], be._tiers.budget["pinned"] = 1 << 20, 1 << 20
    assert be._tiers.tiered()
    assert be.fixed_demotes == (model == "fixed")


@pytest.mark.parametrize("demote", [None, "0"])
def test_without_the_switch_a_fixed_backend_stays_untiered(make_backend, demote):
    be = make_backend("cachegen-fixed", demote)
    assert be.model == "fixed" and not be.fixed_demotes and be._tiers._demote is None
    be.set_capacity(hbm_bytes=1 << 20, pinned_bytes=1 << 20)
    assert not be._tiers.tiered() and be.host_arena is None  # (both budgets: its LRU groups are dropped, as before)
    assert make_backend("cachegen", demote)._tiers._demote is not None  # (the coded tier does not read the switch)


def _file_group(be, tier, sizes, model, geometry=(2, 2, 64), chunk_tokens=16, ntokens=None):
    keys = ["k%d" % i for i in range(len(sizes))]
    nt = ntokens if ntokens is not None else chunk_tokens * len(sizes)
    be._groups[0] = lb._Group(0, keys, sum(sizes), geometry, chunk_tokens, nt, [])
    for k, nb in zip(keys, sizes):
        be._key_gid[k] = 0
        be.dict[k] = lb._DevChunk(types.SimpleNamespace(numel=lambda nb=nb: nb), (), torch.bfloat16, model)
    be._lru.add(tier, 0, sum(sizes))
    return keys


@pytest.mark.parametrize("geo", GEOMETRIES, ids=lambda g: "H%dD%dcs%dn%d" % g)
def test_a_fixed_groups_pinned_size_is_a_bound_of_every_pack_it_can_become(make_backend, geo):
    H, D, cs, nt = geo
    L = 2
    n = -(-nt // cs)
    lengths = [min(cs, nt - i * cs) for i in range(n)]
    be = make_backend("cachegen-fixed")
    bins = [16, 32, 17, 18]
    _file_group(be, "hbm", [native.fixed_blob_bytes(L, t, H, D, bins) for t in lengths], "fixed", (L, H, D), cs, nt)
    bound = be._demoted_size(0)
    assert bound == native.r16(native.pack_bound(n, L, cs, H, D))
    # the largest pack the group can become: every coded blob at lmc_blob_bound for its own length
    worst = CacheGenDeviceCodec.demoted_bytes([native.blob_bound(L, t, H, D) for t in lengths], (L, H, D), cs, nt)
    assert worst == native.pack_off_streams(n, L, cs, H, D) + sum(native.blob_bound(L, t, H, D) - native.blob_static_bytes(L, t, H, D)
                                                                  for t in lengths)
    assert bound >= worst
    # ... and the smallest: streams of nothing but their 16-byte granule cannot be what the bound is about
    assert bound > native.pack_off_streams(n, L, cs, H, D)


def test_a_coded_groups_pinned_size_stays_exact(make_backend):
    be = make_backend("cachegen")
    be._codec = lambda: CacheGenDeviceCodec  # (demoted_bytes is a static method: no device codec is made for it)
    sizes = [5008, 4992]
    _file_group(be, "hbm", sizes, None)
    assert be._demoted_size(0) == native.r16(CacheGenDeviceCodec.demoted_bytes(sizes, (2, 2, 64), 16, 32))


@pytest.mark.parametrize("serde,promotes", [("cachegen", True), ("cachegen-fixed", False)])
def test_a_hit_on_a_pinned_group_queues_a_promotion_on_the_coded_tier_only(make_backend, serde, promotes):
    be = make_backend(serde)
    ran = []
    be._promote_group = lambda gid: ran.append(gid)
    keys = _file_group(be, "pinned", [4096, 4096], None)
    be._tiers.budget["hbm"], be._tiers.budget["pinned"] = 1 << 20, 1 << 20
    with be._tier_lock:
        be._touch(keys)
        assert be._promoting == ({0} if promotes else set())
        be._touch(keys)  # (a second hit queues nothing more)
    be._promoting.clear()
    be.drain()
    assert ran == ([0] if promotes else [])
    assert be._promotion_off_logged == (not promotes)
