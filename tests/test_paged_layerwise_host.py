"""retrieve_into_paged_layerwise, the parts that need no GPU: the method's signature, the ctypes image of lmc_range_post
against the header's text, the bindings of the two new entry points, the layer schedules, and the layer window."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from lmcache_amd import native
from lmcache_amd.cache_engine import LayerwiseRetrieval, LMCacheEngine
from lmcache_amd.storage_backend.serde.cachegen_device import layer_ranges

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lmc_hip.h")).read(), flags=re.S)


def test_signature_and_defaults():
    sig = inspect.signature(LMCacheEngine.retrieve_into_paged_layerwise)
    assert list(sig.parameters) == ["self", "tokens", "kv_caches", "slot_mapping", "block_size", "layout", "mask", "rope",
                                    "direct", "layers_per_launch"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["layout"], d["mask"], d["rope"], d["direct"], d["layers_per_launch"]) == ("NBHD", None, None, False, 1)
    # the arguments it shares with retrieve_into_paged come in the same order with the same defaults
    one_shot = inspect.signature(LMCacheEngine.retrieve_into_paged).parameters
    for name, par in one_shot.items():
        assert sig.parameters[name].default == par.default, name
    assert list(sig.parameters)[:len(one_shot)] == list(one_shot)
    r = LayerwiseRetrieval((), torch.zeros(4, dtype=torch.bool), [], [])  # what a miss returns
    assert r.kv == () and not r.ret_mask.any() and not r.layer_events
    r.wait_layer(0, None)  # no events: launches nothing, waits for nothing
    r.finish()


def test_range_post_struct_is_the_header_struct():
    m = re.search(r"typedef struct lmc_range_post\s*\{(.*?)\}\s*lmc_range_post\s*;", _header(), flags=re.S)
    assert m, "lmc_range_post is not declared"
    ctype_of = {"const float*": ctypes.c_void_p, "const int32_t*": ctypes.c_void_p, "int32_t": ctypes.c_int32,
                "const lmc_kv_layout*": ctypes.POINTER(native.KvLayoutStruct)}
    declared = []
    for decl in m.group(1).split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        typ, names = decl.rsplit(" ", 1) if "," not in decl else decl.split(" ", 1)
        for name in names.split(","):
            declared.append((name.strip(), ctype_of[typ.strip()]))
    assert declared == list(native.RangePostStruct._fields_)
    assert [n for n, _ in declared] == ["cos_sin", "table_rows", "rot_dim", "is_neox", "delta", "deltas", "tok_begin", "ntok",
                                        "scatter_dst", "scatter_tok0"]
    # natural alignment: pointers on 8-byte boundaries, no surprise in the middle
    S = native.RangePostStruct
    assert (S.cos_sin.offset, S.table_rows.offset, S.deltas.offset, S.tok_begin.offset, S.scatter_dst.offset,
            S.scatter_tok0.offset, ctypes.sizeof(S)) == (0, 8, 24, 32, 40, 48, 56)


def test_the_two_entry_points_are_declared_and_bound():
    hdr = _header()
    assert re.search(r"#define\s+LMC_ABI_VERSION\s+6\b", open(os.path.join(ROOT, "include", "lmc_hip.h")).read())
    u64, PP = ctypes.c_uint64, ctypes.POINTER(native.RangePostStruct)

    def params(name):
        m = re.search(r"int\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, f"{name} is not declared"
        return [" ".join(p.split()) for p in m.group(1).split(",")]

    # the _post entry points are the plain ones' arguments and the post-op
    for name in ("lmc_decode_chunks_schedule", "lmc_load_pack"):
        assert params(name + "_post") == params(name) + ["const lmc_range_post* post"]
        res, args = native.SYMBOLS[name + "_post"]
        assert res is ctypes.c_int and args == native.SYMBOLS[name][1] + [PP]
    assert u64 in native.SYMBOLS["lmc_load_pack_post"][1]
    lib = native.lib()  # raises if a symbol is missing
    assert lib.lmc_load_pack_post.argtypes == native.SYMBOLS["lmc_load_pack_post"][1]


@pytest.mark.parametrize("L,schedule,want", [
    (32, 1, [(l, l + 1) for l in range(32)]),
    (32, (2, 6, 24), [(0, 2), (2, 8), (8, 32)]),
    (32, 8, [(0, 8), (8, 16), (16, 24), (24, 32)]),
    (3, 1, [(0, 1), (1, 2), (2, 3)]),
    (3, (1, 2), [(0, 1), (1, 3)]),
    (3, 3, [(0, 3)]),
    (3, (2, 6, 24), [(0, 2), (2, 3)]),  # a schedule longer than the model: the last range ends with it
])
def test_layer_ranges_of_the_schedules(L, schedule, want):
    got = layer_ranges(L, schedule)
    assert got == want
    assert got[0][0] == 0 and got[-1][1] == L and all(a[1] == b[0] for a, b in zip(got, got[1:]))


def test_layer_window_of_a_layout():
    """KVLayout.layers(l0, nl): a pointer into the layer-major plane table, or the base moved by l0 layer strides."""
    s = native._layout_struct(torch.bfloat16, 8, 2, 64, 128, 64, base=0x10000, stride_layer=4096, stride_kv=2048)
    w = native.KVLayout(s, [], 70, torch.device("cpu")).layers(3, 2)
    assert (w.L, w.H, w.D, w.ntokens) == (2, 2, 64, 70)
    assert w.struct.base == 0x10000 + 3 * 4096 * 2 and w.struct.stride_layer == 4096 and not w.struct.plane_ptrs
    f8 = native._layout_struct(torch.float8_e4m3fn, 8, 2, 64, 128, 64, base=0x10000, stride_layer=4096, stride_kv=2048)
    assert native.KVLayout(f8, [], 70, torch.device("cpu")).layers(3, 2).struct.base == 0x10000 + 3 * 4096
    t = native._layout_struct(torch.float16, 8, 2, 64, 128, 64, plane_ptrs=0x20000, slot_mapping=0x30000, block_size=16,
                              stride_block=2048, paged_kind=native.PAGED_SPLIT)
    full = native.KVLayout(t, [], 70, torch.device("cpu"))
    w = full.layers(5, 3)
    assert w.struct.plane_ptrs == 0x20000 + 16 * 5 and w.L == 3 and w.struct.paged_kind == native.PAGED_SPLIT
    assert w.struct.slot_mapping == 0x30000 and full.L == 8 and full.struct.plane_ptrs == 0x20000  # the original is not touched
    for l0, nl in ((-1, 1), (0, 0), (6, 3), (8, 1)):
        with pytest.raises(ValueError):
            full.layers(l0, nl)


def test_range_post_struct_is_filled_per_job():
    """One lmc_range_post per decode job: its token window, the deltas' offset, the scatter's first token."""
    s = native._layout_struct(torch.bfloat16, 3, 2, 64, 128, 64, base=0x10000, stride_layer=4096, stride_kv=2048)
    dst = native.KVLayout(s, [], 70, torch.device("cpu"))
    # a first-chunk trim of 8 tokens, two chunks of 32; then the job behind it (one ragged chunk)
    assert native.RangePost.window(dst, -8, 2, 32) == (0, 56)
    assert native.RangePost.window(dst, 56, 1, 32) == (56, 14)
    post = native.RangePost(scatter_dst=dst, scatter_tok0=0)
    p = post.struct(56, 14)
    assert (p.tok_begin, p.ntok, p.scatter_tok0, p.cos_sin, p.deltas) == (56, 14, 56, None, None)
    assert ctypes.addressof(p.scatter_dst.contents) == ctypes.addressof(dst.struct)
