"""lmc_rope_shift_split on the host: the export as include/lmc_hip.h declares it and native.py binds it, where
native.RangePost.apply sends a rotation (the split kernels for a PAGED_SPLIT destination that names itself, the row
kernels and the scatter otherwise), and where the engine reads LMCACHE_AMD_SPLIT_ROPE.

No GPU and no library: the context is a recorder, as in tests/test_binding_dispatch_host.py."""
import ctypes
import os
import re

import pytest
import torch

from lmcache_amd import native
from lmcache_amd.cache_engine import LMCacheEngine, _PagedTarget
from tests.test_binding_dispatch_host import _header_params, _only_call, ctx, rec  # noqa: F401  (fixtures)

STREAM, STATUS = 0x5700, 0x57A7


def _layout(kind=native.PAGED_ROWS, ntokens=700, **fields):
    s = native.KvLayoutStruct()
    s.paged_kind = kind
    for k, v in fields.items():
        setattr(s, k, v)
    return native.KVLayout(s, [], ntokens, torch.device("cpu"))


class _Table:
    """What the binding reads of a cos/sin table or a delta tensor (no device here)."""

    def __init__(self, shape, dtype, ptr):
        self.shape, self.dtype, self._ptr, self.is_cuda = shape, dtype, ptr, True

    def dim(self):
        return len(self.shape)

    def is_contiguous(self):
        return True

    def numel(self):
        n = 1
        for s in self.shape:
            n *= s
        return n

    def data_ptr(self):
        return self._ptr

    def __getitem__(self, sl):
        assert isinstance(sl, slice) and len(self.shape) == 1
        b, e, _ = sl.indices(self.shape[0])
        return _Table((e - b,), self.dtype, self._ptr + b * 4)


# ------------------------------------------------------------------ the export
def test_the_export_is_declared_as_lmc_rope_shift_is_and_bound_with_matching_types():
    params = _header_params("lmc_rope_shift_split")
    assert params == _header_params("lmc_rope_shift")
    assert params == ["ctx", "kv", "tok_begin", "ntok", "cos_sin", "table_rows", "rot_dim", "is_neox", "delta", "deltas",
                      "job_status", "stream"]
    restype, argtypes = native.SYMBOLS["lmc_rope_shift_split"]
    assert restype is ctypes.c_int and len(argtypes) == len(params)
    assert argtypes == native.SYMBOLS["lmc_rope_shift"][1]
    text = open(os.path.join(native.INCLUDE, "lmc_hip.h")).read()
    decl = re.search(r"\bint\s+lmc_rope_shift_split\s*\((.*?)\)\s*;", text, re.S).group(1)
    want = {"kv": native._PL, "tok_begin": native._i32, "ntok": native._i32, "table_rows": native._i32,
            "rot_dim": native._i32, "is_neox": native._i32, "delta": native._i32}
    for i, piece in enumerate(decl.split(",")):
        name = re.findall(r"\w+", piece)[-1]
        if name in want:
            assert argtypes[i] is want[name], name
            assert ("int32_t" in piece) == (want[name] is native._i32), piece
        else:  # pointers and the stream handle
            assert argtypes[i] is ctypes.c_void_p, name
    assert "LMC_ABI_VERSION 6" in text  # additive: the version does not move


def test_the_wrapper_calls_its_own_symbol(ctx, rec):  # noqa: F811
    table, deltas = _Table((64, 32), torch.float32, 0x7AB000), _Table((9,), torch.int32, 0xDE17A0)
    dst = _layout(native.PAGED_SPLIT)
    ctx.rope_shift_split(dst, 3, 9, table, 32, False, delta=0, deltas=deltas, job_status=STATUS, stream=STREAM)
    args, params = _only_call(rec, "lmc_rope_shift_split")
    assert args[1]._obj is dst.struct
    assert args[2:10] == (3, 9, 0x7AB000, 64, 32, 0, 0, 0xDE17A0)
    assert args[params.index("job_status")] == STATUS and args[params.index("stream")] == STREAM
    del rec.calls[:]
    ctx.rope_shift_split(dst, 0, 5, table, 32, True, delta=-7, stream=STREAM)
    args, params = _only_call(rec, "lmc_rope_shift_split")
    assert args[2:10] == (0, 5, 0x7AB000, 64, 32, 1, -7, None) and args[params.index("job_status")] is None
    with pytest.raises(ValueError):  # the binding's own checks are rope_shift's
        ctx.rope_shift_split(dst, 0, 5, _Table((64, 32), torch.bfloat16, 1), 32)
    with pytest.raises(ValueError):
        ctx.rope_shift_split(dst, 0, 5, table, 32, deltas=_Table((4,), torch.int32, 1))


# ------------------------------------------------------------------ RangePost.apply
class _FakeContext:
    def __init__(self):
        self.calls = []

    def rope_shift(self, *a, **kw):
        self.calls.append(("rope_shift", a, kw))

    def rope_shift_split(self, *a, **kw):
        self.calls.append(("rope_shift_split", a, kw))

    def copy_kv(self, *a, **kw):
        self.calls.append(("copy_kv", a, kw))


@pytest.fixture
def no_arg_checks(monkeypatch):
    monkeypatch.setattr(native.Context, "_check_rope_args", staticmethod(lambda *a: None))


def test_apply_rotates_a_split_destination_that_names_itself_in_place(no_arg_checks):
    table, deltas = _Table((64, 32), torch.float32, 0x7AB000), _Table((50,), torch.int32, 0xDE17A0)
    split = _layout(native.PAGED_SPLIT, block_size=16, stride_block=4096)
    twin = _layout(native.PAGED_SPLIT, block_size=16, stride_block=4096)  # another object, the same cache
    for target in (split, twin):
        for per_token in (False, True):
            fake = _FakeContext()
            post = native.RangePost(table, 32, False, delta=0 if per_token else 5, deltas=deltas if per_token else None,
                                    scatter_dst=target)
            assert post.in_place(split)
            post.apply(fake, split, 4, 20)
            (name, a, kw), = fake.calls  # one launch, nothing copied
            assert name == "rope_shift_split" and a[0] is split and a[1:] == (4, 20, table, 32, False)
            assert kw["delta"] == (0 if per_token else 5)
            if per_token:
                assert kw["deltas"].data_ptr() == 0xDE17A0 + 16 and kw["deltas"].numel() == 20
            else:
                assert kw["deltas"] is None
            # the struct of the same post is the in-place form of lmc_range_post: scatter_tok0 == tok_begin
            p = post.struct(4, 20)
            assert p.scatter_tok0 == p.tok_begin == 4 and bytes(p.scatter_dst.contents) == bytes(split.struct)


def test_apply_keeps_the_existing_calls_for_everything_else(no_arg_checks):
    table = _Table((64, 32), torch.float32, 0x7AB000)
    rows, split = _layout(), _layout(native.PAGED_SPLIT, block_size=16, stride_block=4096)
    other = _layout(native.PAGED_SPLIT, block_size=16, stride_block=8192)  # differs in one field

    def names(post, dst):
        fake = _FakeContext()
        post.apply(fake, dst, 0, 10)
        return [c[0] for c in fake.calls]

    assert names(native.RangePost(table, 32, True, delta=3), rows) == ["rope_shift"]
    assert names(native.RangePost(table, 32, True, delta=3, scatter_dst=split), rows) == ["rope_shift", "copy_kv"]
    assert names(native.RangePost(scatter_dst=split), rows) == ["copy_kv"]
    assert names(native.RangePost(), rows) == []
    # a split destination that does not name itself is what it was: the C side refuses the rotation of it
    assert names(native.RangePost(table, 32, True, delta=3), split) == ["rope_shift"]
    assert names(native.RangePost(table, 32, True, delta=3, scatter_dst=other), split) == ["rope_shift", "copy_kv"]
    assert names(native.RangePost(table, 32, True, delta=3, scatter_dst=split, scatter_tok0=1), split) == ["rope_shift", "copy_kv"]
    assert names(native.RangePost(scatter_dst=split), split) == ["copy_kv"]  # (no rotation: not the in-place form)


# ------------------------------------------------------------------ the switch
def _engine(monkeypatch):
    import lmcache_amd.cache_engine as ce
    monkeypatch.setattr(ce, "CreateStorageBackend", lambda config, metadata: object())

    class Cfg:
        chunk_size, save_decode_cache = 32, False
    return LMCacheEngine(Cfg(), object())


def test_the_switch_is_read_at_construction_only(monkeypatch):
    monkeypatch.delenv("LMCACHE_AMD_SPLIT_ROPE", raising=False)
    off = _engine(monkeypatch)
    monkeypatch.setenv("LMCACHE_AMD_SPLIT_ROPE", "1")
    on = _engine(monkeypatch)
    monkeypatch.setenv("LMCACHE_AMD_SPLIT_ROPE", "0")
    off2 = _engine(monkeypatch)
    assert (off.split_rope, on.split_rope, off2.split_rope) == (False, True, False)
    monkeypatch.setenv("LMCACHE_AMD_SPLIT_ROPE", "1")  # set after construction: without effect
    assert not off.split_rope and not off2.split_rope
    monkeypatch.delenv("LMCACHE_AMD_SPLIT_ROPE")
    assert on.split_rope
    rope = object()
    assert on._direct_retrieve(True, "NHDB", rope) is True and on._direct_retrieve(False, "NHDB", rope) is False
    src = open(os.path.join(os.path.dirname(native.__file__), "cache_engine.py")).read()
    assert len(re.findall(r"environ[^\n]*LMCACHE_AMD_SPLIT_ROPE", src)) == 1
    assert re.search(r"self\.split_rope = .*LMCACHE_AMD_SPLIT_ROPE", src)


def test_without_the_switch_the_coded_tiers_refuse_and_the_fixed_tier_stages(monkeypatch):
    monkeypatch.delenv("LMCACHE_AMD_SPLIT_ROPE", raising=False)
    eng = _engine(monkeypatch)
    rope = object()
    assert eng._direct_retrieve(True, "NHDB", rope) is True  # (a coded tier: _PagedTarget raises on it)

    class Meta:
        fmt = "vllm"
    eng.metadata = Meta()
    tokens = torch.zeros(4, dtype=torch.long)
    with pytest.raises(ValueError, match="direct=True with rope"):
        _PagedTarget(eng, tokens, [], torch.zeros(4, dtype=torch.long), 16, "NHDB", None, rope, True)

    class Fixed:
        model = "fixed"
    eng.engine_ = Fixed()
    assert eng._direct_retrieve(True, "NHDB", rope) is False
    eng.split_rope = True
    assert eng._direct_retrieve(True, "NHDB", rope) is True


def test_the_switch_is_documented():
    root = os.path.dirname(os.path.dirname(os.path.abspath(native.__file__)))
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        assert "LMCACHE_AMD_SPLIT_ROPE" in open(os.path.join(root, doc)).read(), doc
