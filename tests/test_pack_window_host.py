"""A head window out of a pack (lmc_load_pack_heads / lmc_pack_window_bytes) as far as it shows without a GPU: the
bytes the gather moves against the stream directories of the pack's own blobs, the refusals, the exports."""
import ctypes
import functools
import os

import numpy as np
import pytest

from lmcache_amd import native
from lmcache_amd.storage_backend.serde.cachegen_device import CacheGenDeviceCodec

L, CS, T = 2, 32, 70  # two whole chunks and a ragged one
HW = native.HeadWindowStruct


@functools.lru_cache(None)
def _pack(oracle, H, D):
    """(buffer, address, size) of an oracle pack of geometry (L, H, D)."""
    kv = np.random.default_rng(H * 1000 + D).standard_normal((L, 2, T, H * D)).astype(np.float32)
    bits = (kv.view(np.uint32) >> 16).astype(np.uint16)  # truncated bf16: any bits do
    bins = np.array([32, 16, 17, 16], np.int32)
    pack = oracle.pack_from_blobs([oracle.encode_blob(np.ascontiguousarray(bits[:, :, t:t + CS]), oracle.BF16, H, D, bins)
                                   for t in range(0, T, CS)], CS)
    buf = ctypes.create_string_buffer(pack, len(pack))
    return buf, ctypes.addressof(buf), len(pack)


@pytest.mark.parametrize("H,D,begin,nheads,c0,m,whole", [
    (8, 32, 3, 2, 0, 0, False),  # channels 96 .. 160: starts and ends inside groups
    (8, 32, 6, 2, 0, 0, False),  # ends in the last group: the plane's end
    (8, 32, 0, 8, 0, 0, True),   # the whole blob
    (3, 40, 1, 2, 0, 0, True),   # C = 120, no multiple of 64: heads 1 and 2 touch both groups
    (8, 32, 3, 2, 1, 1, False),  # a sub-run of chunks
])
def test_window_bytes_are_the_directory_runs_of_the_packs_blobs(oracle, H, D, begin, nheads, c0, m, whole):
    _, ptr, size = _pack(oracle, H, D)
    G, g_lo, g_hi = (H * D + 63) // 64, begin * D // 64, ((begin + nheads) * D - 1) // 64 + 1
    want = segments = 0
    for c in range(c0, c0 + m if m else 3):
        blob = native.pack_extract(ptr, size, c)
        beg = oracle.stream_dir(blob)[:, 0].reshape(2 * L, G)
        ends = np.append(beg[1:, 0], oracle.parse_header(blob)["stream_bytes"])  # a plane ends where its successor begins
        want += sum(int((beg[p, g_hi] if g_hi < G else ends[p]) - beg[p, g_lo]) for p in range(2 * L))
        segments += int(ends[-1])
    got = native.pack_window_bytes(ptr, size, c0, m, native.HeadWindow(H, begin, nheads, 0))
    assert got == want and (got == segments if whole else 0 < got < segments)


@pytest.mark.parametrize("heads,cut,c0", [(None, 0, 0), ((8, 7, 2, 0), 0, 0), ((8, -1, 2, 0), 0, 0), ((8, 0, 0, 0), 0, 0),
                                          ((4, 0, 2, 0), 0, 0), ((8, 3, 2, 0), 16, 0), ((8, 3, 2, 0), 0, 3)])
def test_window_bytes_refusals_are_invalid(oracle, heads, cut, c0):
    _, ptr, size = _pack(oracle, 8, 32)
    out = ctypes.c_uint64(0)
    win = None if heads is None else ctypes.byref(HW(*heads))
    assert native.lib().lmc_pack_window_bytes(ptr, size - cut, c0, 0, win, ctypes.byref(out)) == native.ERR_INVALID


def test_both_exports_are_declared_at_abi_6_and_bound():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lmc_hip.h")).read()
    assert "#define LMC_ABI_VERSION 6\n" in hdr and "int lmc_load_pack_heads(" in hdr and "int lmc_pack_window_bytes(" in hdr
    assert native.lib().lmc_pack_window_bytes and native.lib().lmc_abi_version() == 6
    twin = native.SYMBOLS["lmc_load_pack"][1]  # lmc_load_pack's arguments, the window in front of the status word
    assert native.SYMBOLS["lmc_load_pack_heads"][1] == twin[:-2] + [ctypes.POINTER(HW)] + twin[-2:]


def test_load_pack_refuses_post_with_heads_before_anything_is_touched():
    codec = CacheGenDeviceCodec.__new__(CacheGenDeviceCodec)  # (no context, no lock: touching either raises AttributeError)
    with pytest.raises(ValueError, match="post"):
        codec.load_pack(object(), 0, 1, object(), 0, None, post=object(), heads=native.HeadWindow(8, 0, 4, 0))
