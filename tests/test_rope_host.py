"""RoPE shift, the parts that need no GPU: the C ABI's declaration and export, the table RopeShift builds, its host-side
refusals, and the CPU statement of the rotation (the reference the GPU tests hold lmc_rope_shift to, bit for bit) with
the error bound derived for it."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from lmcache_amd import native
from lmcache_amd.rope import RopeShift

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cpu_shift(K, table, deltas, rot, neox=True):
    """include/lmc_hip.h's formula in torch on the CPU, separate fp32 tensor ops, one cast at the end.
    K [..., T, H, D] (any 16-bit float dtype), table fp32 [rows, rot], deltas int [T] (|d| < rows)."""
    x = K[..., :rot].float()  # (only the rotated channels are ever converted: the others keep their bits, NaNs included)
    h = rot // 2
    d = torch.as_tensor(deltas, dtype=torch.int64)
    c = table[d.abs(), :h][:, None, :]
    s = table[d.abs(), h:][:, None, :] * torch.where(d < 0, -1.0, 1.0)[:, None, None]
    if neox:
        x1, x2 = x[..., :h], x[..., h:]
    else:
        x1, x2 = x[..., 0::2], x[..., 1::2]
    a, b = x1 * c, x2 * s
    o1 = a - b
    a, b = x2 * c, x1 * s
    o2 = a + b
    out = K.clone()
    if neox:
        out[..., :h], out[..., h:rot] = o1.to(K.dtype), o2.to(K.dtype)
    else:
        out[..., 0:rot:2], out[..., 1:rot:2] = o1.to(K.dtype), o2.to(K.dtype)
    return out


def formula_table(base, rot, rows):
    inv_freq = 1.0 / (base ** (torch.arange(0, rot, 2, dtype=torch.float32) / rot))
    f = torch.outer(torch.arange(rows, dtype=torch.float32), inv_freq)
    return torch.cat((f.cos(), f.sin()), dim=-1), inv_freq


# ------------------------------------------------------------------ C ABI
def test_rope_shift_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "lmc_hip.h")).read()
    assert re.search(r"#define\s+LMC_STATUS_BAD_POSITION\s+64u", hdr)
    assert re.search(r"#define\s+LMC_ABI_VERSION\s+6\b", hdr)
    m = re.search(r"int\s+lmc_rope_shift\s*\(([^;]*)\)\s*;", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert m, "lmc_rope_shift is not declared"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["lmc_ctx* ctx", "const lmc_kv_layout* kv", "int32_t tok_begin", "int32_t ntok", "const float* cos_sin",
                      "int32_t table_rows", "int32_t rot_dim", "int32_t is_neox", "int32_t delta", "const int32_t* deltas",
                      "uint32_t* job_status", "lmc_stream_t stream"]
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    res, args = native.SYMBOLS["lmc_rope_shift"]
    assert res is ctypes.c_int
    assert args == [vp, ctypes.POINTER(native.KvLayoutStruct), i32, i32, vp, i32, i32, i32, i32, vp, vp, vp]
    lib = native.lib()
    assert lib.lmc_rope_shift.argtypes == args
    out = subprocess.check_output(["nm", "-D", "--defined-only", native.SO_PATH], text=True)
    assert re.search(r" T lmc_rope_shift\b", out)
    assert "rope" in native.describe_status(64)


# ------------------------------------------------------------------ the table
@pytest.mark.parametrize("base,rot,rows", [(10000.0, 128, 64), (500000.0, 64, 2049), (10000.0, 24, 7)])
def test_from_base_is_the_stated_formula_bitwise(base, rot, rows):
    r = RopeShift.from_base(base, rot, rows, "cpu")
    want, _ = formula_table(base, rot, rows)
    assert r.cos_sin.shape == (rows, rot) and r.cos_sin.dtype == torch.float32 and r.cos_sin.is_contiguous()
    assert torch.equal(r.cos_sin.view(torch.int32), want.view(torch.int32))
    assert (r.rot_dim, r.is_neox, r.delta, r.table_rows) == (rot, True, 0, rows)
    assert torch.equal(r.cos_sin[0], torch.cat((torch.ones(rot // 2), torch.zeros(rot // 2))))


def test_from_cos_sin_cache_widens_any_float_dtype():
    table, _ = formula_table(10000.0, 64, 33)
    for dt in (torch.bfloat16, torch.float16, torch.float32):
        cache = table.to(dt)
        r = RopeShift.from_cos_sin_cache(cache, is_neox=False, delta=-5)
        assert r.cos_sin.dtype == torch.float32 and r.cos_sin.is_contiguous()
        assert torch.equal(r.cos_sin, cache.float())
        assert (r.rot_dim, r.is_neox, r.delta) == (64, False, -5)
    # a strided cache (every other row of a larger one) is made contiguous
    r = RopeShift.from_cos_sin_cache(table[::2])
    assert r.cos_sin.is_contiguous() and torch.equal(r.cos_sin, table[::2])


def test_host_side_refusals():
    table, _ = formula_table(10000.0, 64, 32)
    ok = RopeShift(table, 64, True, 31)
    assert ok.delta == 31 and RopeShift(table, 64, True, -31).delta == -31
    with pytest.raises(ValueError):  # wrong shape: one dimension
        RopeShift(table.reshape(-1), 64)
    with pytest.raises(ValueError):  # columns are not rot_dim
        RopeShift(table, 32)
    with pytest.raises(ValueError):  # no rows
        RopeShift(table[:0], 64)
    with pytest.raises(ValueError):  # wrong dtype
        RopeShift(table.to(torch.bfloat16), 64)
    with pytest.raises(ValueError):
        RopeShift(table.double(), 64)
    with pytest.raises(ValueError):  # odd rot_dim
        RopeShift(torch.zeros(32, 63), 63)
    with pytest.raises(ValueError):
        RopeShift.from_base(10000.0, 63, 32, "cpu")
    with pytest.raises(ValueError):
        RopeShift.from_cos_sin_cache(torch.zeros(32, 63))
    for d in (32, -32, 1000):  # a uniform |delta| outside the table
        with pytest.raises(ValueError):
            RopeShift(table, 64, True, d)
        with pytest.raises(ValueError):
            RopeShift.from_base(10000.0, 64, 32, "cpu", delta=d)
    with pytest.raises(ValueError):  # a delta tensor of the wrong dtype
        RopeShift(table, 64, True, torch.zeros(10, dtype=torch.int64))
    with pytest.raises(ValueError):
        RopeShift(table, 64, True, torch.zeros(10, dtype=torch.float32))
    with pytest.raises(ValueError):  # ... of the wrong shape
        RopeShift(table, 64, True, torch.zeros((2, 5), dtype=torch.int32))
    per_tok = RopeShift(table, 64, True, torch.arange(10, dtype=torch.int32))
    with pytest.raises(ValueError):  # ... of the wrong length for the call
        per_tok.deltas_for(0, 5, 12, "cpu")
    assert torch.equal(per_tok.deltas_for(3, 4, 10, "cpu"), torch.arange(3, 7, dtype=torch.int32))
    assert ok.deltas_for(0, 5, 12, "cpu") is None
    with pytest.raises(ValueError):
        RopeShift.from_cos_sin_cache(torch.zeros(32, 64, dtype=torch.int32))


def test_engine_refuses_before_anything_is_queued():
    """retrieve_into_paged's own checks need no GPU: they look at shapes and dtypes only."""
    from lmcache_amd.cache_engine import LMCacheEngine
    table, _ = formula_table(10000.0, 64, 32)
    rope = RopeShift(table, 64, True, 3)
    nb, bs, H = 4, 8, 2
    check = LMCacheEngine._check_rope
    check(rope, [torch.zeros((2, nb, bs, H, 64), dtype=torch.bfloat16)], "NBHD", 10)
    check(rope, [torch.zeros((2, nb, H, bs, 64), dtype=torch.float16)], "NHBD", 10)
    check(rope, [torch.zeros((2, nb, H, 64, bs), dtype=torch.bfloat16)], "NHDB", 10)
    check(rope, [(torch.zeros((nb, H, 8, bs, 8), dtype=torch.bfloat16), torch.zeros((nb, H, 64, bs), dtype=torch.bfloat16))],
          "NHDB", 10)
    with pytest.raises(ValueError, match="head size"):
        check(rope, [torch.zeros((2, nb, bs, H, 32), dtype=torch.bfloat16)], "NBHD", 10)
    with pytest.raises(ValueError, match="head size"):
        check(rope, [torch.zeros((2, nb, H, 32, bs), dtype=torch.bfloat16)], "NHDB", 10)
    with pytest.raises(ValueError, match="head size"):
        check(rope, [(torch.zeros((nb, H, 4, bs, 8), dtype=torch.bfloat16), torch.zeros((nb, H, 32, bs), dtype=torch.bfloat16))],
              "NHDB", 10)
    for fp8 in (torch.float8_e4m3fn, torch.float8_e5m2):
        with pytest.raises(ValueError, match="fp8"):
            check(rope, [torch.zeros((2, nb, bs, H, 64), dtype=fp8)], "NBHD", 10)
        with pytest.raises(ValueError, match="fp8"):
            check(rope, [torch.zeros((2, nb, H, 64, bs), dtype=fp8)], "NHDB", 10)
    per_tok = RopeShift(table, 64, True, torch.arange(10, dtype=torch.int32))
    check(per_tok, [torch.zeros((2, nb, bs, H, 64), dtype=torch.bfloat16)], "NBHD", 10)
    with pytest.raises(ValueError, match="one entry per token"):
        check(per_tok, [torch.zeros((2, nb, bs, H, 64), dtype=torch.bfloat16)], "NBHD", 11)
    far = RopeShift(table, 64, True, torch.full((10,), -32, dtype=torch.int32))
    with pytest.raises(ValueError, match="outside the table"):
        check(far, [torch.zeros((2, nb, bs, H, 64), dtype=torch.bfloat16)], "NBHD", 10)


# ------------------------------------------------------------------ the CPU statement of the rotation
@pytest.mark.parametrize("neox", [True, False], ids=["neox", "gptj"])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_cpu_statement_leaves_everything_outside_the_rotated_channels(dt, neox):
    g = torch.Generator().manual_seed(4)
    T, H, D, rot = 9, 2, 72, 24
    table, _ = formula_table(10000.0, rot, 64)
    K = torch.randint(0, 65536, (T, H, D), generator=g).to(torch.int32).to(torch.int16).view(dt)  # random bit patterns
    K[..., :rot] = (torch.randn((T, H, rot), generator=g) * 8).to(dt)
    deltas = torch.randint(-63, 64, (T,), generator=g)
    out = cpu_shift(K, table, deltas, rot, neox)
    assert torch.equal(out[..., rot:].view(torch.int16), K[..., rot:].view(torch.int16))
    assert not torch.equal(out[..., :rot].view(torch.int16), K[..., :rot].view(torch.int16))
    # delta 0 is the identity on finite keys (row 0 is cos = 1, sin = 0), up to the sign of a zero
    same = cpu_shift(K, table, torch.zeros(T, dtype=torch.int64), rot, neox)
    assert torch.equal(same[..., :rot].float(), K[..., :rot].float())
    # a rotation and its inverse give the key back to within the two casts: each is at most u |value| with
    # |value| <= r <= sqrt(2) max|x|, and the second rotation keeps the first cast's error: 2 sqrt(2) u max|x|, doubled
    # for the fp32 steps and the table
    back = cpu_shift(out, table, -deltas, rot, neox)
    u = 2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11
    x = K[..., :rot].float()
    assert float((back[..., :rot].float() - x).abs().max()) <= 4 * u * float(x.abs().max()) * 2 ** 0.5


def rope_accuracy_case(dt, shift_fn, d, generator, T=64, H=2, rot=128, base=10000.0):
    """Section 5 of the design: x fp64 random, K = dtype(R64(p_old) x) with fp64 angles from the fp32 inv_freq, shifted by
    d with shift_fn(K [T,H,rot], table, d) -> the worst |err| / (u r) against R64(p_old + d) x.  Shared with the GPU test."""
    u, dmax = (2.0 ** -8, 2048) if dt == torch.bfloat16 else (2.0 ** -11, 256)
    assert abs(d) <= dmax
    table, inv_freq = formula_table(base, rot, dmax + 1)
    f = inv_freq.double()
    h = rot // 2
    x = torch.randn((T, H, rot), dtype=torch.float64, generator=generator)
    p_old = torch.arange(T, dtype=torch.float64)[:, None, None] + (dmax if d < 0 else 0)

    def rot64(p):
        ang = p * f
        c, s = ang.cos(), ang.sin()
        x1, x2 = x[..., :h], x[..., h:]
        return torch.cat((x1 * c - x2 * s, x2 * c + x1 * s), dim=-1)

    K = rot64(p_old).to(dt)
    got = shift_fn(K, table, d).double()
    r = (x[..., :h] ** 2 + x[..., h:] ** 2).sqrt()
    r = torch.cat((r, r), dim=-1)
    return float(((got - rot64(p_old + d)).abs() / (u * r)).max())


ACCURACY_DELTAS = {torch.bfloat16: (1, 37, 2048, -9, -2048), torch.float16: (1, 37, 256, -9, -256)}


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_derived_error_bound_holds_for_the_cpu_statement(dt):
    """|err| <= 2.25 u r per component: the stored key is off by <= u r as a vector and a rotation keeps that norm, the
    final cast adds <= u r, and the fp32 angle of table row d adds <= |d| 2^-22 r <= 0.125 u r (|d| <= 2048 for bf16's
    u = 2^-8, <= 256 for fp16's u = 2^-11); the fp32 products and sums are far below that."""
    g = torch.Generator().manual_seed(0)
    worst = 0.0
    for d in ACCURACY_DELTAS[dt]:
        worst = max(worst, rope_accuracy_case(dt, lambda K, table, d: cpu_shift(K, table, torch.full((K.shape[0],), d), 128), d, g))
    print(f"{dt}: worst |err| / (u r) = {worst:.3f}")
    assert worst <= 2.25
