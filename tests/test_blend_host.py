"""CacheBlend token selection, the parts that need no GPU: the two C-ABI declarations against the binding table and the
built library, what lmcache_amd/blend.py refuses before it reaches the native layer, the k = ceil(ratio n) rule, and
the numpy statement of the stable top-k (tests/blend_ref.py) against hand-written cases."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from lmcache_amd import blend, native
from tests.blend_ref import deviation_ref, topk_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(name):
    hdr = open(os.path.join(ROOT, "include", "lmc_hip.h")).read()
    m = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % name, re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert m, f"{name} is not declared"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


# ------------------------------------------------------------------ C ABI
def test_both_calls_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "lmc_hip.h")).read()
    assert re.search(r"#define\s+LMC_ABI_VERSION\s+6\b", hdr)  # additive
    assert _declared("lmc_kv_deviation") == [
        "lmc_ctx* ctx", "const lmc_kv_layout* a", "int32_t a_layer", "int32_t a_tok0", "const lmc_kv_layout* b",
        "int32_t b_layer", "int32_t b_tok0", "int32_t ntok", "float* dev_k", "float* dev_v", "lmc_stream_t stream"]
    assert _declared("lmc_select_topk") == ["lmc_ctx* ctx", "const float* dev", "int32_t n", "int32_t k", "int32_t* idx_out",
                                            "lmc_stream_t stream"]
    vp, i32, pl = ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(native.KvLayoutStruct)
    want = {"lmc_kv_deviation": [vp, pl, i32, i32, pl, i32, i32, i32, vp, vp, vp],
            "lmc_select_topk": [vp, vp, i32, i32, vp, vp]}
    lib = native.lib()
    out = subprocess.check_output(["nm", "-D", "--defined-only", native.SO_PATH], text=True)
    for name, args in want.items():
        res, got = native.SYMBOLS[name]
        assert res is ctypes.c_int and got == args
        assert getattr(lib, name).argtypes == args
        assert re.search(r" T %s\b" % name, out)


# ------------------------------------------------------------------ blend.py refuses before the native layer
class _NoNative:
    """Stands for native.get_context: a refusal must come before anybody asks for a context."""

    def __init__(self):
        self.calls = []

    def __call__(self, *a, **kw):
        self.calls.append(a)
        raise AssertionError("the native layer was reached")


@pytest.fixture
def no_native(monkeypatch):
    r = _NoNative()
    monkeypatch.setattr(native, "get_context", r)
    monkeypatch.setattr(native, "lib", r)
    return r


T, H, D, NB, BS = 10, 2, 64, 4, 8


def _fresh(dt=torch.bfloat16, t=T, h=H, d=D):
    return torch.zeros((t, h, d), dtype=dt), torch.zeros((t, h, d), dtype=dt)


def _caches(layout="NBHD", dt=torch.bfloat16, nl=2, h=H, d=D, bs=BS):
    shape = {"NBHD": (2, NB, bs, h, d), "NHBD": (2, NB, h, bs, d), "NHDB": (2, NB, h, d, bs)}[layout]
    if dt in (torch.float8_e4m3fn, torch.float8_e5m2):
        return [torch.zeros(shape, dtype=torch.uint8).view(dt) for _ in range(nl)]
    return [torch.zeros(shape, dtype=dt) for _ in range(nl)]


SLOTS = torch.arange(T)


@pytest.mark.parametrize("fn", [blend.kv_deviation, blend.select_recompute], ids=["kv_deviation", "select_recompute"])
def test_shape_dtype_and_device_mismatches_are_value_errors(no_native, fn):
    k, v = _fresh()
    bad = [
        dict(fresh_v=torch.zeros((T, H, D + 8), dtype=torch.bfloat16)),             # K and V differ in shape
        dict(fresh_v=torch.zeros((T, H, D), dtype=torch.float16)),                   # ... in dtype
        dict(fresh_k=torch.zeros((T, H * D), dtype=torch.bfloat16)),                 # not [T, H, D]
        dict(fresh_k=torch.zeros((T, H, D)), fresh_v=torch.zeros((T, H, D))),        # fp32 KV
        dict(kv_caches=_caches(dt=torch.float16)),                                   # cache dtype differs
        dict(kv_caches=_caches(h=H + 1)),                                            # heads differ
        dict(kv_caches=_caches(d=D // 2)),                                           # head size differs
        dict(kv_caches=_caches("NHBD"), layout="NBHD"),                              # the layout says another shape
        dict(kv_caches=_caches("NHDB", d=D // 2), layout="NHDB"),
        dict(kv_caches=[(torch.zeros((NB, H, D // 8, BS, 8), dtype=torch.bfloat16),) * 3] * 2, layout="NHDB"),
        dict(kv_caches=_caches(dt=torch.float8_e4m3fn)),                             # fp8 caches
        dict(kv_caches=_caches(dt=torch.float8_e5m2)),
        dict(kv_caches=_caches("NHDB", dt=torch.float8_e4m3fn), layout="NHDB"),
        dict(kv_caches=_caches(dt=torch.uint8)),                                     # a raw uint8 cache
        dict(kv_caches=[c.to("meta") for c in _caches()]),                           # another device
        dict(kv_caches=[]),
        dict(layer=2), dict(layer=-1),                                               # no such layer
        dict(block_size=BS * 2),
        dict(slot_mapping=torch.arange(T + 1)),                                      # one slot per token
        dict(slot_mapping=torch.zeros(T)),                                           # ... an integer one
        dict(slot_mapping=torch.arange(T).reshape(2, -1)),
        dict(layout="BNHD"), dict(planes="vk"),
    ]
    for kw in bad:
        args = dict(fresh_k=k, fresh_v=v, kv_caches=_caches(), layer=1, slot_mapping=SLOTS, block_size=BS)
        args.update(kw)
        with pytest.raises(ValueError):
            fn(**args)
    assert no_native.calls == []


def test_ratio_and_mask_are_checked_before_anything_is_queued(no_native):
    k, v = _fresh()
    args = dict(fresh_k=k, fresh_v=v, kv_caches=_caches(), layer=0, slot_mapping=SLOTS, block_size=BS)
    for ratio in (0, 0.0, -0.1, 1.0001, 2, float("nan"), None, "0.15"):
        with pytest.raises(ValueError, match="ratio"):
            blend.select_recompute(ratio=ratio, **args)
    for mask in (torch.ones(T + 1, dtype=torch.bool), torch.ones(T - 1, dtype=torch.bool), torch.ones(T, dtype=torch.int32),
                 torch.ones((T, 1), dtype=torch.bool), torch.zeros(T, dtype=torch.bool), [True] * T):
        with pytest.raises(ValueError, match="mask"):
            blend.select_recompute(mask=mask, **args)
    with pytest.raises(ValueError):
        blend.select_tokens(torch.zeros(4, dtype=torch.float64), 2)
    with pytest.raises(ValueError):
        blend.select_tokens(torch.zeros((4, 1)), 2)
    with pytest.raises(ValueError):
        blend.select_tokens(torch.zeros(4), -1)
    with pytest.raises(ValueError):
        blend.select_tokens(torch.zeros(0), 1)
    assert no_native.calls == []


def test_recompute_count_is_the_ceiling():
    assert blend.recompute_count(0.15, 1) == 1 and blend.recompute_count(1e-9, 1) == 1      # n = 1
    assert blend.recompute_count(1.0, 1) == 1 and blend.recompute_count(1, 40) == 40         # ratio = 1
    assert blend.recompute_count(0.15, 41) == 7                                              # 6.15 -> 7
    assert blend.recompute_count(0.15, 39) == 6                                              # 5.85 -> 6
    assert blend.recompute_count(0.5, 3) == 2 and blend.recompute_count(1 / 3, 10) == 4
    assert blend.recompute_count(1e-9, 1000) == 1
    # a product that is an integer: that integer, however the division that made the ratio was rounded
    for n in range(1, 200):
        for k in range(1, n + 1):
            assert blend.recompute_count(k / n, n) == k
    assert blend.recompute_count(6 / 40, 40) == 6 and blend.recompute_count(4 / 38, 38) == 4
    for ratio in (0, -1, 1.5):
        with pytest.raises(ValueError):
            blend.recompute_count(ratio, 10)


def test_runs_of_a_mask():
    m = torch.tensor([0, 1, 1, 0, 0, 1, 0, 1, 1, 1], dtype=torch.bool)
    assert blend._runs(m) == [(1, 3), (5, 6), (7, 10)]
    assert blend._runs(torch.ones(4, dtype=torch.bool)) == [(0, 4)]
    assert blend._runs(torch.zeros(4, dtype=torch.bool)) == []


# ------------------------------------------------------------------ the reference statements
def test_reference_topk_against_hand_written_cases():
    f = np.float32
    assert topk_ref(np.array([1, 5, 3, 5, 2], f), 2).tolist() == [1, 3]
    assert topk_ref(np.array([1, 5, 3, 5, 2], f), 1).tolist() == [1]            # the tie goes to the lower index
    assert topk_ref(np.array([1, 5, 3, 5, 2], f), 3).tolist() == [1, 2, 3]
    assert topk_ref(np.array([7, 7, 7, 7], f), 2).tolist() == [0, 1]
    assert topk_ref(np.array([7, 7, 7, 7], f), 9).tolist() == [0, 1, 2, 3]      # min(k, n)
    assert topk_ref(np.array([7, 7, 7, 7], f), 0).tolist() == []
    assert topk_ref(np.array([3, np.inf, np.nan, 1e30], f), 1).tolist() == [2]  # NaN above +inf
    assert topk_ref(np.array([3, np.inf, np.nan, 1e30], f), 2).tolist() == [1, 2]
    assert topk_ref(np.array([3, np.inf, np.nan, 1e30], f), 3).tolist() == [1, 2, 3]
    assert topk_ref(np.array([0.0, 1e-45, -0.0, 1e-40], f), 2).tolist() == [1, 3]  # subnormals above the zeros
    assert topk_ref(np.array([0.0, 1e-45, -0.0, 1e-40], f), 3).tolist() == [0, 1, 3]  # -0.0 ties with 0.0: the sign is not key
    assert topk_ref(np.array([-4.0, 3.0], f), 1).tolist() == [0]                # magnitude bits: what the header says
    assert topk_ref(np.array([2.0], f), 1).dtype == np.int32


def test_reference_deviation_is_exact_for_integers_and_ieee_otherwise():
    A = np.zeros((1, 2, 3, 1, 2))
    B = np.zeros((2, 2, 5, 1, 2))
    A[0, 1] = [[[1, 2]], [[3, 4]], [[-8, 8]]]
    B[1, 1, 2:5] = [[[0, 0]], [[3, 5]], [[8, -8]]]
    got = deviation_ref(A, 0, 0, B, 1, 2, 3, 1)
    assert got.dtype == np.int64 and got.tolist() == [5, 1, 512]
    assert deviation_ref(A, 0, 1, B, 1, 3, 2, 0).tolist() == [0, 0]
    B[1, 1, 3, 0, 0] = np.inf
    A[0, 1, 2, 0, 1] = 0.5
    got = deviation_ref(A, 0, 0, B, 1, 2, 3, 1)
    assert got.dtype == np.float64 and got[0] == 5 and got[1] == np.inf and got[2] == 256 + 8.5 ** 2
    A[0, 1, 1, 0, 0] = np.inf  # inf - inf
    assert np.isnan(deviation_ref(A, 0, 0, B, 1, 2, 3, 1)[1])
