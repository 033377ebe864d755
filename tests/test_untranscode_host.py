"""lmc_transcode_to_fixed and the fixed-width tier's promotion, on the host: the export and its binding, the codec's
promote dispatch, the backend's switch, the gate in front of a promotion and the room a promotion asks the HBM tier for.
No GPU: the library is loaded for its symbols only, the context and the codec are made without their constructors."""
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
BINS = [16, 32, 17, 18]


def test_the_symbol_is_exported_with_the_argument_types_the_binding_declares():
    fn = getattr(native.lib(), "lmc_transcode_to_fixed")
    res, args = native.SYMBOLS["lmc_transcode_to_fixed"]
    assert fn.restype is res and list(fn.argtypes) == list(args)
    text = open(native.INCLUDE + "/lmc_hip.h").read()
    m = re.search(r"\bint\s+lmc_transcode_to_fixed\s*\((.*?)\)\s*;", text, re.S)
    params = [re.findall(r"\w+", p)[-1] for p in m.group(1).split(",")]
    assert params == ["ctx", "blob_ptrs", "blob_bytes", "nchunks", "L", "H", "D", "dtype", "chunk_tokens", "ntokens", "bins_h",
                      "out_ptrs", "out_bytes", "job_status", "stream"]
    assert len(args) == len(params)
    assert args[params.index("ntokens")] is ctypes.c_uint32
    assert all(args[params.index(p)] is ctypes.c_int32 for p in ("nchunks", "L", "H", "D", "dtype", "chunk_tokens"))
    assert all(args[params.index(p)] is ctypes.c_void_p for p in ("ctx", "blob_ptrs", "blob_bytes", "bins_h", "out_ptrs", "out_bytes",
                                                                  "job_status", "stream"))
    assert native.lib().lmc_abi_version() == 6  # (an additive export)


def test_the_wrapper_calls_its_symbol_once_with_status_and_stream_in_place(monkeypatch):
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
        n = c.transcode_to_fixed(0x7AB1E, 0xB17E5, 3, 2, 2, 64, native.BF16, 256, 700, BINS, 0x0075, 0x0B17, None,
                                 stream=STREAM, status_ptr=STATUS)
        assert n == 3 and [name for name, _ in calls] == ["lmc_transcode_to_fixed"]
        a = calls[0][1]
        assert len(a) == len(native.SYMBOLS["lmc_transcode_to_fixed"][1])
        assert a[0].value == 0xC0DE and a[1:10] == (0x7AB1E, 0xB17E5, 3, 2, 2, 64, native.BF16, 256, 700)
        assert list(a[10]) == BINS and a[11:] == (0x0075, 0x0B17, STATUS, STREAM)
        with pytest.raises(AssertionError):  # 700 tokens are three chunks of 256, not two
            c.transcode_to_fixed(0x7AB1E, 0xB17E5, 2, 2, 2, 64, native.BF16, 256, 700, BINS, 0x0075, 0x0B17, None, stream=STREAM)
        assert len(calls) == 1
    finally:
        c.handle = None


class _Stream:
    cuda_stream = STREAM

    def synchronize(self):
        pass


class _Event:
    def record(self, s=None):
        pass

    def synchronize(self):
        pass


@pytest.fixture
def codec(monkeypatch):
    """A codec without a device: the context records, the launch bracket, events and streams are inert."""
    from lmcache_amd.storage_backend.serde import cachegen_device as cd
    import contextlib
    calls = []
    ctx = types.SimpleNamespace(unpack_blobs=lambda *a, **k: calls.append(("unpack_blobs", a, k)),
                                transcode_to_fixed=lambda *a, **k: calls.append(("ctx.transcode_to_fixed", a, k)))
    c = CacheGenDeviceCodec.__new__(CacheGenDeviceCodec)
    c.ctx, c._lock, c.device, c._status, c._xcode_dev = ctx, threading.RLock(), torch.device("cpu"), None, None
    c._launch = lambda cur, loans=None: contextlib.nullcontext((0, STATUS))
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "current_stream", lambda d=None: _Stream())
    monkeypatch.setattr(torch.cuda, "Event", _Event)
    monkeypatch.setattr(cd, "Job", lambda *a, **k: types.SimpleNamespace(retire=lambda: 0))
    monkeypatch.setattr(native, "pack_chunk_bytes", lambda ptr, nbytes, i: 1000 + 8 * i)
    monkeypatch.setattr(native, "pack_info", lambda ptr, nbytes: types.SimpleNamespace(num_layers=2, num_heads=2, head_size=64,
                                                                                    ntokens=37))
    c.calls = calls
    return c


class _Arena:
    def __init__(self):
        self.asked, self.freed = [], []

    def alloc(self, nb, stream=None):
        self.asked.append(nb)
        return torch.zeros(nb, dtype=torch.uint8)

    def free(self, t, events=()):
        self.freed.append(t.numel())


def _pack(n, cs):
    return types.SimpleNamespace(nchunks=n, chunk_tokens=cs, blob=types.SimpleNamespace(ptr=0xAC, nbytes=4096))


def test_promote_pack_without_a_model_makes_the_calls_it_made(codec):
    arena = _Arena()
    out = codec.promote_pack(_pack(3, 16), arena)
    assert arena.asked == [1000, 1008, 1016] and [t.numel() for t in out] == arena.asked
    assert [name for name, _, _ in codec.calls] == ["unpack_blobs"]
    a, k = codec.calls[0][1:]
    assert a[:4] == (0xAC, 4096, 0, 3) and a[4] == [t.data_ptr() for t in out] and a[5] == [1000, 1008, 1016]
    assert k == {"stream": STREAM, "status_ptr": STATUS}
    assert codec._xcode_dev is None  # (no staging: the blobs are unpacked into the arena's regions)
    assert codec.promote_pack(_pack(3, 16), _Arena(), model=None, bins=None) is not None and len(codec.calls) == 2


def test_the_promoters_table_is_the_dispatch(codec):
    assert codec._PROMOTERS == {None: None, "fixed": "transcode_to_fixed"} and callable(CacheGenDeviceCodec.transcode_to_fixed)
    assert codec._DEMOTERS == {None: None, "fixed": "transcode_fixed"}
    seen = []
    codec.transcode_to_fixed = lambda blobs, geo, cs, nt, bins, outs, ready=(): seen.append(("fixed", blobs, geo, cs, nt, bins, outs, ready))
    arena = _Arena()
    out = codec.promote_pack(_pack(3, 16), arena, model="fixed", bins=BINS)
    # the arena's regions are the fixed-width blobs' (37 tokens: 16, 16 and a ragged 5), the coded blobs go to the staging
    want = [native.fixed_blob_bytes(2, t, 2, 64, BINS) for t in (16, 16, 5)]
    assert arena.asked == want and [t.numel() for t in out] == want
    assert [name for name, _, _ in codec.calls] == ["unpack_blobs"]
    a = codec.calls[0][1]
    staged = a[4]
    assert a[5] == [1000, 1008, 1016] and len(staged) == 3 and not set(staged) & {t.data_ptr() for t in out}
    base = codec._xcode_dev.data_ptr()
    assert all(base <= p and p + nb <= base + codec._xcode_dev.numel() and (p - base) % 16 == 0 for p, nb in zip(staged, a[5]))
    assert len(seen) == 1
    tag, blobs, geo, cs, nt, bins, outs, ready = seen[0]
    assert [b.data_ptr() for b in blobs] == staged and [b.numel() for b in blobs] == [1000, 1008, 1016]
    assert (geo, cs, nt, bins) == ((2, 2, 64), 16, 37, BINS) and all(o is t for o, t in zip(outs, out))
    # the table IS the dispatch: another method under "fixed" is the one that runs
    codec._PROMOTERS = {None: None, "fixed": "other"}
    codec.other = lambda *a: seen.append("other")
    codec.promote_pack(_pack(3, 16), _Arena(), model="fixed", bins=BINS)
    assert seen[1:] == ["other"]
    with pytest.raises(ValueError):
        codec.promote_pack(_pack(3, 16), _Arena(), model="lossless")
    # a transcode that raises gives the regions back
    def boom(*a):
        raise native.NativeError("status")
    codec.other = boom
    arena = _Arena()
    with pytest.raises(native.NativeError):
        codec.promote_pack(_pack(3, 16), arena, model="fixed", bins=BINS)
    assert arena.freed == want


@pytest.fixture
def make_backend(monkeypatch):
    monkeypatch.setattr(native, "lib", lambda: None)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    monkeypatch.delenv("LMCACHE_AMD_HBM_BYTES", raising=False)
    monkeypatch.delenv("LMCACHE_AMD_PINNED_BYTES", raising=False)
    made = []

    def make(serde, demote="1", promote="1"):
        for name, v in (("LMCACHE_AMD_FIXED_DEMOTE", demote), ("LMCACHE_AMD_FIXED_PROMOTE", promote)):
            if v is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, v)
        cfg = LMCacheEngineConfig.from_legacy(chunk_size=16, backend="cuda", local_serde=serde)
        be = lb.LMCLocalBackend(cfg, LMCacheEngineMetadata("Llama-3-8B", 1, 0, "vllm", "bfloat16"))
        made.append(be)
        return be
    yield make
    for be in made:
        be.close()


@pytest.mark.parametrize("demote,promote,want", [("1", "1", True), ("1", None, False), ("1", "0", False), (None, "1", False),
                                                 ("0", "1", False), (None, None, False)])
def test_fixed_promotes_needs_both_switches(make_backend, demote, promote, want):
    be = make_backend("cachegen-fixed", demote, promote)
    assert be.fixed_promotes is want
    assert make_backend("cachegen", demote, promote).fixed_promotes is False  # (the coded tier reads neither)


def _file_pinned_group(be, lengths, chunk_tokens, geometry=(2, 2, 64), model_pack=True):
    n = len(lengths)
    keys = ["k%d" % i for i in range(n)]
    pack = types.SimpleNamespace(nchunks=n, chunk_tokens=chunk_tokens, blob=types.SimpleNamespace(ptr=0xAC, nbytes=4096))
    be._groups[0] = lb._Group(0, keys, 4096, geometry, chunk_tokens, sum(lengths), [])
    for i, k in enumerate(keys):
        be._key_gid[k] = 0
        be.dict[k] = lb._PackChunk(pack, i, (), torch.bfloat16)
    be._lru.add("pinned", 0, 4096)
    return keys


@pytest.mark.parametrize("promote", ["1", None])
def test_a_hit_on_a_demoted_fixed_group_queues_a_promotion_only_with_the_switch(make_backend, promote):
    be = make_backend("cachegen-fixed", "1", promote)
    ran = []
    be._promote_group = lambda gid: ran.append(gid)
    keys = _file_pinned_group(be, [16, 16], 16)
    be._tiers.budget["hbm"], be._tiers.budget["pinned"] = 1 << 20, 1 << 20
    with be._tier_lock:
        be._touch(keys)
        assert be._promoting == ({0} if promote else set())
        be._touch(keys)  # (a second hit queues nothing more)
    be._promoting.clear()
    be.drain()
    assert ran == ([0] if promote else [])
    assert be._promotion_off_logged == (not promote)


@pytest.mark.parametrize("lengths,cs", [([16, 16, 16], 16), ([16, 16, 5], 16), ([16], 16), ([13], 16), ([256, 1], 256)])
def test_a_promotion_asks_the_hbm_tier_for_the_fixed_width_sizes(make_backend, monkeypatch, lengths, cs):
    be = make_backend("cachegen-fixed")
    keys = _file_pinned_group(be, lengths, cs)
    be._tiers.budget["hbm"], be._tiers.budget["pinned"] = 1 << 30, 1 << 30
    bins = be.cachegen_config.plane_bins(2)
    asked, promoted = [], []
    monkeypatch.setattr(be._tiers, "make_room", lambda tier, nbytes, keep=(): asked.append((tier, nbytes, list(keep))) or False)
    be._codec = lambda: types.SimpleNamespace(promote_pack=lambda *a, **k: promoted.append((a, k)))
    be._promote_group(0)
    want = sum(native.r16(native.fixed_blob_bytes(2, t, 2, 64, bins)) for t in lengths)
    assert asked == [("hbm", want, [0])] and promoted == []  # (no room: nothing was moved)
    assert be.tier_of(keys[0]) == "pinned"
    # without the switch the worker does not even ask
    be.fixed_promotes = False
    be._promote_group(0)
    assert len(asked) == 1


def test_a_promotion_publishes_fixed_width_entries(make_backend, monkeypatch):
    be = make_backend("cachegen-fixed")
    lengths = [16, 5]
    keys = _file_pinned_group(be, lengths, 16)
    be._tiers.budget["hbm"], be._tiers.budget["pinned"] = 1 << 30, 1 << 30
    bins = be.cachegen_config.plane_bins(2)
    sizes = [native.fixed_blob_bytes(2, t, 2, 64, bins) for t in lengths]
    seen = []

    def promote_pack(pack, arena, model=None, bins=None):
        seen.append((pack, arena, model, bins))
        return [torch.zeros(nb, dtype=torch.uint8) for nb in sizes]
    be._codec = lambda: types.SimpleNamespace(promote_pack=promote_pack)
    be.dev_arena = types.SimpleNamespace(free=lambda t, ev=(): None, set_budget=lambda b: None, reserved_bytes=0,
                                         close=lambda: None)
    be.host_arena = types.SimpleNamespace(free=lambda hb, ev=(): None, set_budget=lambda b: None, reserved_bytes=0,
                                          close=lambda: None)
    monkeypatch.setattr(torch.cuda, "device", lambda d: __import__("contextlib").nullcontext())
    pack = be.dict[keys[0]].pack
    be._promote_group(0)
    assert len(seen) == 1 and seen[0][0] is pack and seen[0][2] == "fixed" and seen[0][3] == bins
    for k, nb in zip(keys, sizes):
        e = be.dict[k]
        assert isinstance(e, lb._DevChunk) and e.model == "fixed" and e.blob.numel() == nb
        assert be.tier_of(k) == "hbm"
    assert be._tiers.promotions == 1 and be._lru.live("hbm") == sum(native.r16(nb) for nb in sizes)
