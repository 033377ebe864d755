"""Retrieve across tensor-parallel degrees (head windows) as far as it shows without a GPU: the shard arithmetic of
lmcache_amd/resharding.py against a brute-force assignment of every head, the two exports (declared, exported at ABI 6,
bound, marshalled), the codec's one dispatch, and the refusals of the engine and the backends -- each raised before
anything is queued, which here means: before the fake backend or the recording library has seen a call."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from lmcache_amd import native, resharding
from lmcache_amd.cache_engine import LMCacheEngine
from lmcache_amd.config import LMCacheEngineMetadata
from lmcache_amd.storage_backend.local_backend import LMCLocalBackend
from lmcache_amd.storage_backend.serde.cachegen_device import CacheGenDeviceCodec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"lmc_decode_chunks_heads_schedule": "decode_chunks_heads_schedule",
       "lmc_decode_chunks_fixed_heads_schedule": "decode_chunks_fixed_heads_schedule"}
TOTALS = (1, 2, 4, 8, 32)


def _divisors(total):
    return [w for w in range(1, 9) if total % w == 0]


# ------------------------------------------------------------------ resharding.head_sources
def _owner(total, world, head):
    """Brute force: the rank of `world` that owns model head `head` (contiguous shards), and the head's index there."""
    per = total // world
    for rank in range(world):
        if rank * per <= head < (rank + 1) * per:
            return rank, head - rank * per
    raise AssertionError


@pytest.mark.parametrize("total", TOTALS)
def test_head_sources_equal_a_brute_force_assignment_of_every_head(total):
    for W in _divisors(total):
        for Ws in _divisors(total):
            seen = set()
            for rank in range(W):
                covered = {}
                srcs = resharding.head_sources(total, W, rank, Ws)
                assert [s[0] for s in srcs] == sorted({s[0] for s in srcs}), "ascending source ranks, each once"
                for src_rank, src_begin, nheads, dst_begin in srcs:
                    assert nheads >= 1 and 0 <= src_begin and src_begin + nheads <= total // Ws
                    for i in range(nheads):
                        assert dst_begin + i not in covered, "a destination head is covered once"
                        covered[dst_begin + i] = (src_rank, src_begin + i)
                assert sorted(covered) == list(range(total // W)), (total, W, rank, Ws)
                for local, got in covered.items():
                    head = rank * (total // W) + local  # the model's numbering
                    assert _owner(total, W, head) == (rank, local)
                    assert got == _owner(total, Ws, head), (total, W, rank, Ws, local)
                    seen.add(head)
                # the first source does not depend on the head count (the engine reads the geometry from it)
                assert srcs[0][0] == (rank * Ws) // W
            assert seen == set(range(total))


def test_head_sources_of_the_issues_two_examples():
    # a TP = 8 rank reads one eighth of a TP = 1 blob; a TP = 2 rank assembles its heads from four TP = 8 shards
    assert resharding.head_sources(8, 8, 5, 1) == [(0, 5, 1, 0)]
    assert resharding.head_sources(8, 2, 1, 8) == [(4, 0, 1, 0), (5, 0, 1, 1), (6, 0, 1, 2), (7, 0, 1, 3)]
    assert resharding.head_sources(32, 4, 3, 4) == [(3, 0, 8, 0)]


@pytest.mark.parametrize("args", [(8, 3, 0, 1), (8, 2, 0, 3), (4, 8, 0, 1), (4, 1, 0, 8), (8, 2, 2, 1), (8, 2, -1, 1),
                                  (0, 1, 0, 1), (8, 0, 0, 1), (8, 2, 0, 0)])
def test_head_sources_refuses_what_contiguous_shards_cannot_describe(args):
    with pytest.raises(ValueError):
        resharding.head_sources(*args)


# ------------------------------------------------------------------ the exports
def _params(hdr, name):
    m = re.search(r"\bint %s\(([^;]*)\);" % name, hdr)
    assert m, name
    return re.sub(r"\s+", " ", m.group(1)).strip()


def test_the_header_declares_the_window_and_the_two_exports_at_abi_6():
    hdr = open(os.path.join(ROOT, "include", "lmc_hip.h")).read()
    assert re.search(r"#define LMC_ABI_VERSION 6\b", hdr)
    m = re.search(r"typedef struct lmc_head_window \{(.*?)\} lmc_head_window;", hdr, re.S)
    assert m, "lmc_head_window"
    fields = re.findall(r"int32_t\s+(\w+);", m.group(1))
    assert fields == ["src_heads", "src_head_begin", "nheads", "dst_head_begin"]
    assert fields == [f for f, _ in native.HeadWindowStruct._fields_] == list(native.HeadWindow._fields)
    assert ctypes.sizeof(native.HeadWindowStruct) == 16
    # one signature for both, the fixed-width twin's with the window where that has its post
    want = _params(hdr, "lmc_decode_chunks_fixed_split_schedule").replace("const lmc_range_post* post", "const lmc_head_window* win")
    hw = ctypes.POINTER(native.HeadWindowStruct)
    for sym in NEW:
        assert _params(hdr, sym) == want, sym
        res, args = native.SYMBOLS[sym]
        twin = native.SYMBOLS["lmc_decode_chunks_fixed_split_schedule"][1]
        assert res is ctypes.c_int and len(args) == len(twin)
        assert [a for a in args if a is not hw] == [a for a in twin if a is not ctypes.POINTER(native.RangePostStruct)]
        assert args.index(hw) == len(args) - 3, "win, job_status, stream"


def test_the_library_exports_them_and_refuses_null_arguments():
    native.build()
    lib = native.lib()
    assert lib.lmc_abi_version() == 6
    ends = (ctypes.c_int32 * 1)(2)
    lay = native.KvLayoutStruct(dtype=native.BF16, num_layers=2, num_heads=4, head_size=64, base=0x1000, stride_layer=2 * 32 * 256,
                                stride_kv=32 * 256, stride_token=256, stride_head=64)
    win = native.HeadWindowStruct(8, 0, 4, 0)
    for sym in NEW:
        fn = getattr(lib, sym)
        # no context; no window (with everything else as a caller would pass it)
        assert fn(None, 0x2000, 4096, 1, ctypes.byref(lay), 0, 32, 1, ends, None, ctypes.byref(win), None, None) == native.ERR_INVALID
        assert fn(None, 0x2000, 4096, 1, ctypes.byref(lay), 0, 32, 1, ends, None, None, None, None) == native.ERR_INVALID
        assert fn(None, None, 0, 0, None, 0, 0, 0, None, None, None, None, None) == native.ERR_INVALID


def test_the_context_methods_follow_the_schedules_and_take_the_window_before_the_stream():
    twin = list(inspect.signature(native.Context.decode_chunks_fixed_split_schedule).parameters)
    for name in NEW.values():
        got = list(inspect.signature(getattr(native.Context, name)).parameters)
        assert got == [("heads" if p == "post" else p) for p in twin], name


# ------------------------------------------------------------------ marshalling (a recording library, no device)
class _Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if name not in native.SYMBOLS:
            raise AttributeError(name)

        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


@pytest.fixture
def rec(monkeypatch):
    r = _Recorder()
    monkeypatch.setattr(native, "lib", lambda: r)
    return r


@pytest.fixture
def ctx(rec):
    c = native.Context.__new__(native.Context)
    c.device, c.handle = 0, ctypes.c_void_p(0xC0DE)
    yield c
    c.handle = None


def _layout(kind=native.PAGED_ROWS, dtype=native.BF16):
    return native.KVLayout(native.KvLayoutStruct(dtype=dtype, num_layers=8, paged_kind=kind), [], 700, torch.device("cpu"))


@pytest.mark.parametrize("sym,name", sorted(NEW.items()))
def test_the_wrappers_call_their_own_symbol_with_the_window_in_its_slot(ctx, rec, sym, name):
    dst = _layout()
    getattr(ctx, name)(0x7AB1E, 9000, 5, dst, -40, 256, [1, 3, 8], None, native.HeadWindow(8, 2, 3, 1), stream=0x5700, status_ptr=0x57A7)
    assert [n for n, _ in rec.calls] == [sym]
    args = rec.calls[0][1]
    assert len(args) == len(native.SYMBOLS[sym][1]) and args[0].value == 0xC0DE
    assert args[1:4] == (0x7AB1E, 9000, 5) and args[4]._obj is dst.struct and args[5:8] == (-40, 256, 3)
    assert list(args[8]) == [1, 3, 8] and args[9] is None
    w = args[10]._obj
    assert isinstance(w, native.HeadWindowStruct)
    assert (w.src_heads, w.src_head_begin, w.nheads, w.dst_head_begin) == (8, 2, 3, 1)
    assert args[11:] == (0x57A7, 0x5700)


class _Ctx:
    """What CacheGenDeviceCodec._entry looks its methods up on."""
    def __getattr__(self, name):
        if name.startswith("decode_chunks") or name.startswith("encode_chunks"):
            return name
        raise AttributeError(name)


def test_the_codec_keeps_one_dispatch_and_names_the_new_exports():
    codec = CacheGenDeviceCodec.__new__(CacheGenDeviceCodec)
    codec.ctx = _Ctx()
    rows, split = _layout(), _layout(native.PAGED_SPLIT)
    pick = lambda model, lay: codec._entry(codec._HEAD_SCHEDULES, model, lay, "decode_chunks_heads_schedule")
    assert pick(None, rows) == pick(None, split) == "decode_chunks_heads_schedule"
    assert pick("fixed", rows) == pick("fixed", split) == "decode_chunks_fixed_heads_schedule"
    with pytest.raises(ValueError):
        pick("fixed", _layout(dtype=native.FP8_E4M3))
    with pytest.raises(ValueError):
        pick("other", rows)
    for fn in (CacheGenDeviceCodec.decode_device, CacheGenDeviceCodec.decode):
        assert inspect.signature(fn).parameters["heads"].default is None
    # a window takes no post-op: refused before a stream, a table or a status word is touched
    with pytest.raises(ValueError, match="post"):
        codec.decode_device([object()], rows, 0, 32, post=object(), heads=native.HeadWindow(8, 0, 4, 0))


# ------------------------------------------------------------------ refusals of the backends and the engine
def test_the_raw_tiers_refuse_a_window_before_anything_is_looked_up():
    for mode in ("raw", "hbm"):
        b = LMCLocalBackend.__new__(LMCLocalBackend)  # (no lock, no dict: touching either would raise AttributeError)
        b.mode, b.supports_head_window, b.put_thread = mode, False, None
        with pytest.raises(ValueError, match="raw chunks"):
            b.get_kv_range([], None, "vllm", 0, 32, heads=native.HeadWindow(8, 0, 4, 0))
    b = LMCLocalBackend.__new__(LMCLocalBackend)
    b.mode, b.supports_head_window, b.put_thread = "hbm-cachegen", True, None
    with pytest.raises(ValueError, match="post"):
        b.get_kv_range([], None, "vllm", 0, 32, post=object(), heads=native.HeadWindow(8, 0, 4, 0))
    assert inspect.signature(LMCLocalBackend.get_kv_range).parameters["heads"].default is None
    from lmcache_amd.storage_backend.abstract_backend import LMCBackendInterface
    from lmcache_amd.storage_backend.remote_backend import LMCPipelinedRemoteBackend
    assert LMCBackendInterface.supports_head_window is False
    assert inspect.signature(LMCPipelinedRemoteBackend.get_kv_range).parameters["heads"].default is None


class _Backend:
    """Records every call the engine makes; holds nothing."""

    def __init__(self, **flags):
        self.calls = []
        self.__dict__.update(flags)

    def __getattr__(self, name):
        def call(*a, **k):
            self.calls.append(name)
            return 0
        return call


def _engine(backend, world=2, rank=1):
    e = LMCacheEngine.__new__(LMCacheEngine)
    e.metadata = LMCacheEngineMetadata("m", world, rank, "vllm", "half")
    e.chunk_size, e.engine_, e.split_rope = 32, backend, False
    return e


def test_the_engine_refuses_before_anything_is_queued():
    tokens = torch.arange(70)
    # a backend without the window decode: the raw tiers, chunk-tensor backends
    for layout, window in ((False, False), (True, False), (False, True)):
        b = _Backend(supports_kv_layout=layout, supports_head_window=window)
        e = _engine(b)
        with pytest.raises(ValueError, match="window of heads"):
            e.retrieve(tokens, stored_world_size=1)
        with pytest.raises(ValueError, match="window of heads"):
            e.stored_at(4)
        assert b.calls == []
    # the layer-wise calls have no window form, whatever the backend
    b = _Backend(supports_kv_layout=True, supports_head_window=True)
    e = _engine(b)
    view = e.stored_at(1)
    assert view is not e and view.engine_ is b and view.metadata == e.metadata and view._stored_ws == 1
    with pytest.raises(ValueError, match="not built"):
        view.retrieve_layerwise(tokens)
    with pytest.raises(ValueError, match="not built"):
        view.retrieve_into_paged_layerwise(tokens, [torch.zeros(2, 4, 16, 4, 64, dtype=torch.bfloat16)], torch.arange(70), 16, "NBHD")
    with pytest.raises(ValueError):
        e.retrieve(tokens, stored_world_size=0)
    with pytest.raises(ValueError):
        e.stored_at(-2)
    assert b.calls == []
    # None and the engine's own degree are the engine itself: today's path, no refusal consulted
    assert e.stored_at(None) is e and e.stored_at(2) is e
    assert inspect.signature(LMCacheEngine.stored_at).parameters["stored_world_size"].default is inspect.Parameter.empty
    # retrieve() keeps the reference's named parameters and takes this one keyword beyond them
    assert [p.kind.name for p in inspect.signature(LMCacheEngine.retrieve).parameters.values()][-1] == "VAR_KEYWORD"
    with pytest.raises(TypeError, match="stored_world"):
        e.retrieve(tokens, stored_world=1)
    assert b.calls == []


def test_head_counts_the_two_degrees_do_not_divide_are_refused_before_a_destination_is_made():
    """H_src = 3 heads stored at TP = 2 (6 KV heads) for a TP = 4 engine: ValueError once the geometry is known, with
    only the index consulted -- no destination made, no get_kv_range."""
    class B(_Backend):
        def contains_prefix(self, keys):
            self.calls.append("contains_prefix")
            return len(keys)

        def chunk_meta(self, key):
            self.calls.append("chunk_meta")
            return (2, 2, 32, 3, 64), torch.bfloat16
    b = B(supports_kv_layout=True, supports_head_window=True)
    e = _engine(b, world=4, rank=1)

    def make_dst(*a):
        raise AssertionError("no destination before the refusal")
    with pytest.raises(ValueError, match="divisible"):
        e.stored_at(2)._retrieve_into(torch.arange(70), None, make_dst)
    assert set(b.calls) <= {"contains_prefix", "chunk_meta"}


def test_keys_of_a_resharded_retrieve_name_the_stored_shard():
    e = _engine(_Backend())
    own, other = e._make_key("abc", "vllm"), e._make_key("abc", "vllm", (8, 5))
    assert (own.world_size, own.worker_id) == (2, 1) and (other.world_size, other.worker_id) == (8, 5)
    assert (own.fmt, own.model_name, own.chunk_hash) == (other.fmt, other.model_name, other.chunk_hash)
