"""native.Context's encode, schedule and load-pack wrappers, on the host: every wrapper calls its own C symbol, once, with
the argument list native.SYMBOLS declares and with the post pointer, the status pointer and the stream where
include/lmc_hip.h puts them (the symbols end in "status, stream, post" or in "post, status, stream").

No GPU and no library: the object native.lib() returns is replaced by a recorder, the context is made without
lmc_ctx_create, and every call names its stream."""
import ctypes
import os
import re

import pytest
import torch

from lmcache_amd import native

ENCODERS = ["encode_chunks", "encode_chunks_split", "encode_chunks_fixed", "encode_chunks_fixed_split"]
SCHEDULES = ["decode_chunks_schedule", "decode_chunks_schedule_post", "decode_chunks_fixed_schedule",
             "decode_chunks_fixed_split_schedule"]
STREAM, STATUS = 0x5700, 0x57A7


class _Recorder:
    """Stands for the loaded library: records (symbol, arguments) and reports success."""

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
    c.handle = None  # (nothing for close() to destroy)


def _layout():
    return native.KVLayout(native.KvLayoutStruct(), [], 700, torch.device("cpu"))


def _header_params(symbol):
    """The parameter names of `symbol` as include/lmc_hip.h declares them."""
    text = open(os.path.join(native.INCLUDE, "lmc_hip.h")).read()
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % re.escape(symbol), text, re.S)
    assert m, f"{symbol} is not declared in lmc_hip.h"
    return [re.findall(r"\w+", p)[-1] for p in m.group(1).split(",")]


def _only_call(rec, symbol):
    assert [name for name, _ in rec.calls] == [symbol], f"{symbol}: the wrapper called {[n for n, _ in rec.calls]}"
    args = rec.calls[0][1]
    params = _header_params(symbol)
    assert len(args) == len(native.SYMBOLS[symbol][1]) == len(params), symbol
    assert args[0].value == 0xC0DE
    return args, params


def _check_tail(symbol, args, params, post):
    """Status, stream and post where the header has them; the post slot is also where SYMBOLS has its pointer type."""
    assert args[params.index("job_status")] == STATUS and args[params.index("stream")] == STREAM, symbol
    argtypes = native.SYMBOLS[symbol][1]
    rp = ctypes.POINTER(native.RangePostStruct)
    assert ("post" in params) == (rp in argtypes), symbol
    if "post" in params:
        at = params.index("post")
        assert argtypes[at] is rp, symbol
        if post is None:
            assert args[at] is None, symbol
        else:
            assert args[at]._obj is post, symbol  # byref(post)
    assert sorted(params.index(p) for p in ("job_status", "stream", "post") if p in params) == \
        list(range(len(params) - (3 if "post" in params else 2), len(params))), f"{symbol}: they are the last arguments"


@pytest.mark.parametrize("tok_end,chunk_tokens", [(700, 256), (512, 256), (3, 256)])
@pytest.mark.parametrize("name", ENCODERS)
def test_encode_wrappers_call_their_own_symbol(ctx, rec, name, tok_end, chunk_tokens):
    src, bins = _layout(), [32, 16, 16, 32]
    n = getattr(ctx, name)(src, 2, tok_end, chunk_tokens, bins, 0xB10B, 4096, 0x5123, stream=STREAM, status_ptr=STATUS)
    assert n == -(-(tok_end - 2) // chunk_tokens)
    args, params = _only_call(rec, "lmc_" + name)
    _check_tail("lmc_" + name, args, params, None)
    assert args[1]._obj is src.struct
    assert args[2:5] == (2, tok_end, chunk_tokens) and list(args[5]) == bins and args[6:9] == (0xB10B, 4096, 0x5123)


@pytest.mark.parametrize("ends_as", ["list", "array"])
@pytest.mark.parametrize("name,with_post", [(n, p) for n in SCHEDULES for p in (False, True) if n != SCHEDULES[0] or not p])
def test_schedule_wrappers_call_their_own_symbol(ctx, rec, name, ends_as, with_post):
    takes_post = name != "decode_chunks_schedule"
    dst, ends = _layout(), [1, 3, 8]
    given = ends if ends_as == "list" else (ctypes.c_int32 * 3)(*ends)
    post = native.RangePostStruct() if with_post else None
    kw = {"post": post} if takes_post else {}
    getattr(ctx, name)(0x7AB1E, 9000, 5, dst, -40, 256, given, None, stream=STREAM, status_ptr=STATUS, **kw)
    args, params = _only_call(rec, "lmc_" + name)
    _check_tail("lmc_" + name, args, params, post)
    assert args[1:4] == (0x7AB1E, 9000, 5) and args[4]._obj is dst.struct and args[5:8] == (-40, 256, 3)
    sent = args[params.index("layer_ends_h")]
    assert isinstance(sent, ctypes.c_int32 * 3) and list(sent) == ends
    if ends_as == "array":
        assert sent is given  # a prebuilt array goes through as it is
    assert args[params.index("events_h")] is None


def test_schedule_wrappers_marshal_events(ctx, rec):
    class Ev:  # what the wrappers read of a NativeEvent
        def __init__(self, h):
            self.handle = ctypes.c_void_p(h)
    for name in SCHEDULES:
        kw = {"post": None} if name == "decode_chunks_schedule_post" else {}  # (the others default it, or have none)
        del rec.calls[:]
        getattr(ctx, name)(1, 2, 3, _layout(), 0, 256, [4, 8], [Ev(0xE1), Ev(0xE2)], stream=STREAM, status_ptr=STATUS, **kw)
        args, params = _only_call(rec, "lmc_" + name)
        sent = args[params.index("events_h")]
        assert isinstance(sent, ctypes.c_void_p * 2) and list(sent) == [0xE1, 0xE2]
        del rec.calls[:]
        prebuilt = (ctypes.c_void_p * 2)(0xE3, 0xE4)
        getattr(ctx, name)(1, 2, 3, _layout(), 0, 256, [4, 8], prebuilt, stream=STREAM, status_ptr=STATUS, **kw)
        args, params = _only_call(rec, "lmc_" + name)
        assert args[params.index("events_h")] is prebuilt
        _check_tail("lmc_" + name, args, params, None)


@pytest.mark.parametrize("name,with_post", [("load_pack", False), ("load_pack_post", False), ("load_pack_post", True)])
def test_load_pack_wrappers_call_their_own_symbol(ctx, rec, name, with_post):
    dst = _layout()
    post = native.RangePostStruct() if with_post else None
    extra = (post,) if name == "load_pack_post" else ()
    getattr(ctx, name)(0xFACC, 1 << 20, 2, 5, dst, -7, 4, 0xE7E7, *extra, stream=STREAM, status_ptr=STATUS)
    args, params = _only_call(rec, "lmc_" + name)
    _check_tail("lmc_" + name, args, params, post)
    assert args[1:5] == (0xFACC, 1 << 20, 2, 5) and args[5]._obj is dst.struct and args[6:9] == (-7, 4, 0xE7E7)
