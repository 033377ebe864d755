"""lmc_kv_deviation and lmc_select_topk (include/lmc_hip.h, csrc/k_blend.h) on the GPU, and lmcache_amd/blend.py.

The references are the numpy statements of tests/blend_ref.py on the logical view [L, 2, T, H, D] of both sides; the
layouts are built here from that view: tuples of [T, H, D] tensors, a vllm chunk, NBHD / NHBD blocks and the NHDB cache
of vLLM's ROCm paged-attention kernels (5-d and as the (key_cache, value_cache) pair).  Whatever a layout stores outside
the tokens of the logical view is random bit patterns, NaNs included: a token read from a wrong slot shows."""
import ctypes

import numpy as np
import pytest
import torch

from lmcache_amd import blend, native
from lmcache_amd.cache_engine import LMCacheEngine
from lmcache_amd.rope import RopeShift
from tests import far_offsets as fo
from tests.blend_ref import deviation_ref, logical, topk_ref
from tests.test_gpu_engine import dumb_metadata, generate_tokens, make_cfg
from tests.test_gpu_far_offsets import Far, arena, far  # noqa: F401  (the arena fixtures)
from tests.test_gpu_rope_shift import _ibits, _mapping, _random_bits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INVALID = -1  # LMC_ERR_INVALID
LA, LB, A_LAYER, B_LAYER = 2, 3, 1, 2  # both layer indices non-zero and different
NTOK, A_TOK0, B_TOK0 = 37, 5, 3
TA, TB = A_TOK0 + NTOK + 2, B_TOK0 + NTOK + 2
BS, NBLOCKS = 16, 8
GUARD = 8
SENTINEL = -12345.0
DTYPES = [torch.bfloat16, torch.float16]


@pytest.fixture(scope="module")
def ctx():
    native.build()
    return native.get_context(0)


def _small_ints(shape, dt, g):
    """Integers in [-8, 8]: every difference, square and sum over C <= 2^16 channels is exact in fp32 (C * 256 < 2^24)."""
    return torch.randint(-8, 9, shape, generator=g).to(dt)


def _slots(mapping, n, g):
    if mapping == "blocks":  # token t at offset t % BS of its block: aligned runs, the V tile form's fast tiles
        blocks = torch.randperm(NBLOCKS, generator=g)[:(n + BS - 1) // BS]
        pos = torch.arange(n)
        return blocks[pos // BS] * BS + pos % BS
    return _mapping(mapping, n, NBLOCKS, BS, g)  # "random", or "offset5": a run that enters its first block at offset 5


class SideA:
    """The fresh side: per layer a (K, V) pair of [T, H, D] tensors holding the logical view X [L, 2, T, H, D] from token
    `tok0` on.  "tuple": the tensors themselves; "slice": slices of longer tensors (tok0 = 5 into the view);
    "unaligned": tensors 2 bytes off a 16-byte boundary (the element form)."""

    def __init__(self, kind, X, g):
        L, _, T, H, D = X.shape
        self.kind, self.tok0 = kind, (A_TOK0 if kind == "slice" else 0)
        self.store, pairs = [], []
        for l in range(L):
            pair = []
            for kv in range(2):
                if kind == "slice":  # the view begins 4 tokens into a longer tensor and the range 5 tokens into the view
                    big = _random_bits((T + 9, H, D), X.dtype, g)
                    big[4 + A_TOK0:4 + A_TOK0 + T] = X[l, kv]
                    big = big.to(DEV)
                    view = big[4:]
                elif kind == "unaligned":
                    big = _random_bits((T * H * D + 16,), X.dtype, g)
                    big[1:1 + T * H * D] = X[l, kv].reshape(-1)
                    big = big.to(DEV)
                    view = big[1:1 + T * H * D].view(T, H, D)
                    assert view.data_ptr() % 16 == 2
                else:
                    big = X[l, kv].clone().to(DEV)
                    view = big
                self.store.append(big)
                pair.append(view)
            pairs.append(tuple(pair))
        self.layout = native.KVLayout.from_kv_tuple(tuple(pairs), "vllm")


class SideB:
    """The cached side holding the logical view X [L, 2, T, H, D]: "chunk" (a vllm chunk), "NBHD", "NHBD", "NHDB" (5-d) or
    "NHDB_pair", the paged ones through `slots`."""

    def __init__(self, kind, X, slots, g):
        L, _, T, H, D = X.shape
        dt = X.dtype
        self.kind, self.slots = kind, slots
        if kind == "chunk":
            cpu = [X.clone()]
        else:
            shape = {"NBHD": (2, NBLOCKS, BS, H, D), "NHBD": (2, NBLOCKS, H, BS, D)}.get(kind, (2, NBLOCKS, H, D, BS))
            cpu = [_random_bits(shape, dt, g) for _ in range(L)]
            blk, off = slots // BS, slots % BS
            for l in range(L):
                c = cpu[l]
                if kind == "NBHD":
                    c[0][blk, off], c[1][blk, off] = X[l, 0], X[l, 1]
                elif kind == "NHBD":
                    c[0][blk, :, off], c[1][blk, :, off] = X[l, 0], X[l, 1]
                else:  # keys x-split [num_blocks, H, D / 8, block_size, 8], values [num_blocks, H, D, block_size]
                    c[0].view(NBLOCKS, H, D // 8, BS, 8)[blk, :, :, off] = X[l, 0].reshape(T, H, D // 8, 8)
                    c[1][blk, :, :, off] = X[l, 1]
        self.store = [c.to(DEV) for c in cpu]
        if kind == "chunk":
            self.layout = native.KVLayout.from_chunk(self.store[0], "vllm")
        elif kind == "NHDB_pair":
            # two allocations per layer, as PagedAttention.split_kv_cache hands them over
            self.store = [t for c in self.store for t in (c[0].view(NBLOCKS, H, D // 8, BS, 8).clone(), c[1].clone())]
            pairs = [(self.store[2 * l], self.store[2 * l + 1]) for l in range(L)]
            self.layout = native.KVLayout.paged(pairs, slots.to(DEV), BS, "NHDB")
        else:
            self.layout = native.KVLayout.paged(self.store, slots.to(DEV), BS, kind)


def _outputs(n=NTOK):
    return [torch.full((n + GUARD,), SENTINEL, dtype=torch.float32, device=DEV) for _ in range(2)]


def _run(ctx, a, b, a_layer, a_tok0, b_layer, b_tok0, ntok, planes="kv"):
    """One lmc_kv_deviation with guarded outputs -> (dev_k, dev_v) as float64 numpy (None for a skipped plane); both sides
    must hold the bits they held, the guard words their sentinel, and the status word 0."""
    keep = [[t.clone() for t in side.store] for side in (a, b)]
    dk, dv = _outputs(ntok)
    ctx.kv_deviation(a.layout, a_layer, a_tok0, b.layout, b_layer, b_tok0, ntok, dk if "k" in planes else None,
                     dv if "v" in planes else None)
    torch.cuda.synchronize()
    for side, before in zip((a, b), keep):
        assert all(torch.equal(_ibits(x), _ibits(y)) for x, y in zip(side.store, before)), "a KV side was written"
    out = []
    for t, on in ((dk, "k" in planes), (dv, "v" in planes)):
        assert bool((t[ntok:] == SENTINEL).all()), "words behind dev[ntok] were written"
        assert on or bool((t == SENTINEL).all()), "a skipped plane was written"
        out.append(t[:ntok].cpu().numpy() if on else None)
    assert ctx.status(clear=True) == 0
    return out


# ------------------------------------------------------------------ 1. exact addressing
B_KINDS = [("chunk", None)] + [(k, m) for k in ("NBHD", "NHBD", "NHDB", "NHDB_pair") for m in ("blocks", "random", "offset5")]
GEOMS = [(2, 64), (3, 40), (2, 12)]  # C = 128; C = 120, no multiple of 64; head_size % 8 != 0: rows only, the element form


# (the split layout has whole 8-element granules: head_size % 8 == 0)
EXACT_CASES = [(geom, k) for geom in GEOMS for k in B_KINDS if not (geom[1] % 8 and k[0].startswith("NHDB"))]


@pytest.mark.parametrize("geom,b_kind", EXACT_CASES,
                         ids=["H%d_D%d_%s" % (g[0], g[1], k[0] if k[1] is None else f"{k[0]}_{k[1]}") for g, k in EXACT_CASES])
def test_deviation_equals_the_integer_reference(ctx, geom, b_kind):
    """Small integers: every sum is exact in fp32, so dev_k / dev_v must EQUAL the int64 reference whatever the order of
    the additions -- any difference is a wrongly addressed element."""
    H, D = geom
    kind, mapping = b_kind
    g = torch.Generator().manual_seed(1000 * GEOMS.index(geom) + B_KINDS.index(b_kind))
    for dt in DTYPES:
        XA, XB = _small_ints((LA, 2, NTOK, H, D), dt, g), _small_ints((LB, 2, TB, H, D), dt, g)
        A, B = logical(XA), logical(XB)
        b = SideB(kind, XB, None if mapping is None else _slots(mapping, TB, g), g)
        for a_kind in ("tuple", "slice", "unaligned"):
            a = SideA(a_kind, XA, g)
            dk, dv = _run(ctx, a, b, A_LAYER, a.tok0, B_LAYER, B_TOK0, NTOK)
            for kv, got in ((0, dk), (1, dv)):
                want = deviation_ref(A, A_LAYER, 0, B, B_LAYER, B_TOK0, NTOK, kv)
                assert want.dtype == np.int64 and want.max() > 0
                assert np.array_equal(got.astype(np.int64), want) and np.array_equal(got, want.astype(np.float32)), \
                    f"{dt} a={a_kind} b={kind}/{mapping} plane {'KV'[kv]}: tokens {np.nonzero(got != want)[0][:8]}"
            # one plane at a time: the other output is not touched, the values are the same bits
            only_k, none = _run(ctx, a, b, A_LAYER, a.tok0, B_LAYER, B_TOK0, NTOK, "k")
            none2, only_v = _run(ctx, a, b, A_LAYER, a.tok0, B_LAYER, B_TOK0, NTOK, "v")
            assert none is None and none2 is None and np.array_equal(only_k, dk) and np.array_equal(only_v, dv)
        if kind != "chunk":  # the split (or paged) side as `a`, rows as `b`: the call is symmetric in its sides
            a = SideA("tuple", XA, g)
            dk, dv = _run(ctx, b, a, B_LAYER, B_TOK0, A_LAYER, 0, NTOK)
            for kv, got in ((0, dk), (1, dv)):
                assert np.array_equal(got.astype(np.int64), deviation_ref(A, A_LAYER, 0, B, B_LAYER, B_TOK0, NTOK, kv))


def test_single_tokens_and_ranges_that_end_inside_a_tile(ctx):
    """ntok = 1 .. 17 from every offset 0 .. 8 into a block-ordered NHDB cache: every way a range can begin and end
    inside a tile of eight slots."""
    H, D, dt = 2, 64, torch.bfloat16
    g = torch.Generator().manual_seed(7)
    XA, XB = _small_ints((1, 2, 32, H, D), dt, g), _small_ints((1, 2, 32, H, D), dt, g)
    A, B = logical(XA), logical(XB)
    a, b = SideA("tuple", XA, g), SideB("NHDB", XB, _slots("blocks", 32, g), g)
    for tok0 in range(9):
        for n in (1, 2, 7, 8, 9, 16, 17):
            dk, dv = _outputs(n)
            ctx.kv_deviation(a.layout, 0, tok0, b.layout, 0, tok0, n, dk, dv)
            for kv, t in ((0, dk), (1, dv)):
                got = t.cpu().numpy()
                assert np.array_equal(got[:n].astype(np.int64), deviation_ref(A, 0, tok0, B, 0, tok0, n, kv)), (tok0, n, kv)
                assert (got[n:] == SENTINEL).all()
    assert ctx.status(clear=True) == 0


# ------------------------------------------------------------------ 2. accuracy
def _wide_range(shape, dt, g):
    """|x| in [2^-6, 2^6], random signs: no square overflows or underflows, in fp32 or in either 16-bit format."""
    mag = torch.exp2(torch.rand(shape, generator=g, dtype=torch.float64) * 12 - 6)
    sign = torch.randint(0, 2, shape, generator=g) * 2 - 1
    return (mag * sign).to(dt)


@pytest.mark.parametrize("kind", ["NBHD", "NHDB"])
@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
def test_deviation_is_within_the_derived_bound_of_float64(ctx, dt, kind):
    """|dev - ref64| <= (n + 3) 2^-24 ref64 per token, n = the number of terms (C per plane, 2 C for "kv").
    Derived, not measured: the 16-bit inputs widen exactly, so a term is (a - b)^2 (1 + d)^3 with |d| <= 2^-24 -- one
    rounding of the difference, counted twice by the square, and one of the product -- and a sum of n non-negative fp32
    terms in ANY order multiplies each by at most (1 + 2^-24)^(n - 1).  (1 + 2^-24)^(n + 2) - 1 <= (n + 3) 2^-24 for the n
    here.  A square and an add contracted into one fma only remove a rounding.  The "kv" sum of blend.kv_deviation adds
    one more rounding to 2 C terms already counted with n = C each: within (2 C + 3) 2^-24 as well."""
    H, D, n_tok = 8, 128, 64
    C = H * D
    g = torch.Generator().manual_seed(11 + DTYPES.index(dt))
    XA, XB = _wide_range((1, 2, n_tok, H, D), dt, g), _wide_range((2, 2, n_tok, H, D), dt, g)
    A, B = logical(XA), logical(XB)
    slots = _slots("blocks" if kind == "NHDB" else "random", n_tok, g)
    a, b = SideA("tuple", XA, g), SideB(kind, XB, slots, g)
    dk, dv = _run(ctx, a, b, 0, 0, 1, 0, n_tok)
    worst = 0.0
    for kv, got in ((0, dk), (1, dv)):
        ref = deviation_ref(A, 0, 0, B, 1, 0, n_tok, kv)
        assert ref.dtype == np.float64 and (ref > 0).all()
        err = np.abs(got.astype(np.float64) - ref) / ref
        worst = max(worst, float(err.max()) * 2.0 ** 24)
        print(f"{dt} {kind} plane {'KV'[kv]}: worst |dev - ref| / ref = {err.max() * 2.0 ** 24:.2f} x 2^-24 (bound {C + 3})")
        assert (err <= (C + 3) * 2.0 ** -24).all()
    # the same call again: the same bits
    dk2, dv2 = _run(ctx, a, b, 0, 0, 1, 0, n_tok)
    assert np.array_equal(dk.view(np.uint32), dk2.view(np.uint32)) and np.array_equal(dv.view(np.uint32), dv2.view(np.uint32))
    # blend.kv_deviation: the three plane choices through the Python layer
    fk, fv = a.layout._keep[0], a.layout._keep[1]
    caches = b.store
    got = {p: blend.kv_deviation(fk, fv, caches, 1, slots.to(DEV), BS, kind, planes=p).cpu().numpy() for p in ("k", "v", "kv")}
    assert np.array_equal(got["k"], dk) and np.array_equal(got["v"], dv) and np.array_equal(got["kv"], dk + dv)
    ref = deviation_ref(A, 0, 0, B, 1, 0, n_tok, 0) + deviation_ref(A, 0, 0, B, 1, 0, n_tok, 1)
    assert (np.abs(got["kv"].astype(np.float64) - ref) <= (2 * C + 3) * 2.0 ** -24 * ref).all()


# ------------------------------------------------------------------ 3. special values
@pytest.mark.parametrize("kind,mapping", [("NBHD", "random"), ("NHDB", "blocks"), ("NHDB", "random"), ("chunk", None)],
                         ids=["NBHD", "NHDB_tiles", "NHDB_elements", "chunk"])
@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
def test_nan_and_inf_reach_exactly_their_own_tokens(ctx, dt, kind, mapping):
    H, D = 2, 64
    g = torch.Generator().manual_seed(5)
    XA, XB = _small_ints((LA, 2, NTOK, H, D), dt, g), _small_ints((LB, 2, TB, H, D), dt, g)
    t_nan, t_inf, t_pair = 4, 17, 30  # tokens of the range; in a block-ordered cache 17 and 30 lie inside whole tiles
    for kv in range(2):
        XB[B_LAYER, kv, B_TOK0 + t_nan, 1, 9] = float("nan")
        XB[B_LAYER, kv, B_TOK0 + t_inf, 0, 63] = float("inf")
        XB[B_LAYER, kv, B_TOK0 + t_pair, 1, 0] = float("inf")
        XA[A_LAYER, kv, t_pair, 1, 0] = float("inf")  # inf - inf
    A, B = logical(XA), logical(XB)
    a, b = SideA("tuple", XA, g), SideB(kind, XB, None if mapping is None else _slots(mapping, TB, g), g)
    special = np.zeros(NTOK, bool)
    special[[t_nan, t_inf, t_pair]] = True
    clean_a, clean_b = A.copy(), B.copy()
    clean_a[~np.isfinite(clean_a)] = 0
    clean_b[~np.isfinite(clean_b)] = 0
    for kv, got in enumerate(_run(ctx, a, b, A_LAYER, 0, B_LAYER, B_TOK0, NTOK)):
        assert np.isnan(got[t_nan]) and np.isposinf(got[t_inf]) and np.isnan(got[t_pair])
        want = deviation_ref(clean_a, A_LAYER, 0, clean_b, B_LAYER, B_TOK0, NTOK, kv)
        assert np.array_equal(got[~special].astype(np.int64), want[~special]) and np.isfinite(got[~special]).all()
        ieee = deviation_ref(A, A_LAYER, 0, B, B_LAYER, B_TOK0, NTOK, kv)  # float64: the same NaN / inf pattern
        assert np.array_equal(np.isnan(got), np.isnan(ieee)) and np.array_equal(np.isinf(got), np.isinf(ieee))


# ------------------------------------------------------------------ 4. refusals
def test_refusals_launch_nothing(ctx):
    H, D, dt = 2, 64, torch.bfloat16
    g = torch.Generator().manual_seed(9)
    XA, XB = _small_ints((LA, 2, NTOK, H, D), dt, g), _small_ints((LB, 2, TB, H, D), dt, g)
    a = SideA("tuple", XA, g)
    b = SideB("NHDB", XB, _slots("blocks", TB, g), g)
    b_rows = SideB("NBHD", XB, _slots("random", TB, g), g)
    other = {
        "fp16": SideA("tuple", XA.to(torch.float16), g),
        "heads": SideA("tuple", _small_ints((LA, 2, NTOK, H + 1, D), dt, g), g),
        "head_size": SideA("tuple", _small_ints((LA, 2, NTOK, H, D + 8), dt, g), g),
        "split": SideB("NHDB", XB, _slots("random", TB, g), g),
    }
    fp8 = [torch.zeros((NTOK, H, D), dtype=torch.uint8, device=DEV).view(torch.float8_e4m3fn) for _ in range(4)]
    fp8_layout = native.KVLayout.from_kv_tuple(((fp8[0], fp8[1]),), "vllm")
    sides = [a, b, b_rows] + list(other.values())
    keep = [[t.clone() for t in s.store] for s in sides]
    dk, dv = _outputs()
    lib, h = native.lib(), ctx.handle
    st = native.current_stream_ptr(torch.device(DEV))

    def call(la, al, at, lb, bl, bt, n, k=dk, v=dv):
        return lib.lmc_kv_deviation(h, ctypes.byref(la.struct), al, at, ctypes.byref(lb.struct), bl, bt, n,
                                    None if k is None else k.data_ptr(), None if v is None else v.data_ptr(), st)

    A, Bl = a.layout, b.layout
    assert call(other["fp16"].layout, A_LAYER, 0, Bl, B_LAYER, B_TOK0, NTOK) == INVALID       # dtype mismatch
    assert call(fp8_layout, 0, 0, fp8_layout, 0, 0, NTOK) == INVALID                          # fp8
    assert call(other["heads"].layout, A_LAYER, 0, b_rows.layout, B_LAYER, B_TOK0, NTOK) == INVALID   # H mismatch
    assert call(other["head_size"].layout, A_LAYER, 0, b_rows.layout, B_LAYER, B_TOK0, NTOK) == INVALID  # D mismatch
    assert call(other["split"].layout, B_LAYER, 0, Bl, B_LAYER, B_TOK0, NTOK) == INVALID      # both sides split
    for al, bl in ((LA, B_LAYER), (-1, B_LAYER), (A_LAYER, LB), (A_LAYER, -1)):               # a layer out of range
        assert call(A, al, 0, Bl, bl, B_TOK0, NTOK) == INVALID
    assert call(A, A_LAYER, 0, Bl, B_LAYER, B_TOK0, 0) == INVALID                             # ntok = 0
    assert call(A, A_LAYER, 0, Bl, B_LAYER, B_TOK0, -3) == INVALID
    assert call(A, A_LAYER, 0, Bl, B_LAYER, B_TOK0, NTOK, None, None) == INVALID              # both outputs NULL
    assert call(A, A_LAYER, -1, Bl, B_LAYER, B_TOK0, NTOK) == INVALID                         # a negative token offset
    assert call(A, A_LAYER, 0, Bl, B_LAYER, -1, NTOK) == INVALID
    assert lib.lmc_kv_deviation(None, ctypes.byref(A.struct), A_LAYER, 0, ctypes.byref(Bl.struct), B_LAYER, B_TOK0, NTOK,
                                dk.data_ptr(), dv.data_ptr(), st) == INVALID
    with pytest.raises(ValueError):  # the wrapper's own checks: an output of the wrong dtype, one that is too short
        ctx.kv_deviation(A, A_LAYER, 0, Bl, B_LAYER, B_TOK0, NTOK, dk.double(), dv)
    with pytest.raises(ValueError):
        ctx.kv_deviation(A, A_LAYER, 0, Bl, B_LAYER, B_TOK0, NTOK, dk[:NTOK - 1], dv)
    torch.cuda.synchronize()
    assert bool((dk == SENTINEL).all()) and bool((dv == SENTINEL).all())
    for s, before in zip(sides, keep):
        assert all(torch.equal(_ibits(x), _ibits(y)) for x, y in zip(s.store, before))
    assert ctx.status(clear=True) == 0
    # ... and the same arguments without the fault are taken
    assert call(A, A_LAYER, 0, Bl, B_LAYER, B_TOK0, NTOK) == 0
    torch.cuda.synchronize()
    assert not bool((dk[:NTOK] == SENTINEL).any())


# ------------------------------------------------------------------ 5. lmc_select_topk
def _topk(ctx, dev_cpu, k):
    """One lmc_select_topk -> (return code, the min(k, n) indices); the words behind them keep their sentinel."""
    n = len(dev_cpu)
    kk = max(0, min(k, n))
    dev = torch.from_numpy(np.ascontiguousarray(dev_cpu, np.float32)).to(DEV)
    out = torch.full((kk + GUARD,), -7, dtype=torch.int32, device=DEV)
    rc = native.lib().lmc_select_topk(ctx.handle, dev.data_ptr(), n, k, out.data_ptr(), native.current_stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[kk:] == -7).all(), "words behind idx_out[min(k, n)] were written"
    return rc, got[:kk]


def _keys(kind, n, rng):
    if kind == "distinct":
        return (rng.permutation(n) + 1).astype(np.float32) * np.float32(0.25)
    if kind == "equal":
        return np.full(n, 3.5, np.float32)
    if kind == "two_values":  # many ties on both sides of every wave and tile boundary
        return rng.choice(np.array([1.0, 2.0], np.float32), n)
    if kind == "inf_nan":
        x = (rng.standard_normal(n) ** 2 * 100).astype(np.float32)
        x[rng.random(n) < 0.1] = np.inf
        x[rng.random(n) < 0.1] = np.nan
        x[rng.random(n) < 0.05] = -np.nan  # the sign is not part of the key
        x[rng.random(n) < 0.05] = -1e30
        return x
    assert kind == "subnormal_zero"
    return rng.choice(np.array([0.0, -0.0, 1e-45, 1e-40, 3e-39, 1.1754944e-38], np.float32), n)


@pytest.mark.parametrize("kind", ["distinct", "equal", "two_values", "inf_nan", "subnormal_zero"])
def test_topk_equals_the_stable_reference(ctx, kind):
    rng = np.random.default_rng(17)
    for n in (1, 2, 63, 64, 65, 1000, 4099):
        dev = _keys(kind, n, rng)
        for k in (0, 1, n // 2, n - 1, n, n + 5):
            rc, got = _topk(ctx, dev, k)
            assert rc == 0
            assert np.array_equal(got, topk_ref(dev, k)), f"{kind} n={n} k={k}"
    assert ctx.status(clear=True) == 0


def test_topk_at_the_largest_n_and_the_refusals(ctx):
    rng = np.random.default_rng(3)
    n = 1 << 20
    dev = rng.choice(np.array([1.0, 2.0, 2.0000002, 0.5], np.float32), n)
    dev[rng.integers(0, n, 5)] = np.nan
    rc, got = _topk(ctx, dev, n // 7)
    assert rc == 0 and np.array_equal(got, topk_ref(dev, n // 7))
    again = _topk(ctx, dev, n // 7)[1]
    assert np.array_equal(got, again)
    out = torch.full((16,), -7, dtype=torch.int32, device=DEV)
    big = torch.zeros(n + 1, dtype=torch.float32, device=DEV)
    lib, st = native.lib(), native.current_stream_ptr(torch.device(DEV))
    assert lib.lmc_select_topk(ctx.handle, big.data_ptr(), n + 1, 4, out.data_ptr(), st) == INVALID
    assert lib.lmc_select_topk(ctx.handle, big.data_ptr(), 0, 4, out.data_ptr(), st) == INVALID
    assert lib.lmc_select_topk(ctx.handle, big.data_ptr(), 100, -1, out.data_ptr(), st) == INVALID
    assert lib.lmc_select_topk(ctx.handle, None, 100, 4, out.data_ptr(), st) == INVALID
    assert lib.lmc_select_topk(ctx.handle, big.data_ptr(), 100, 4, None, st) == INVALID
    assert lib.lmc_select_topk(None, big.data_ptr(), 100, 4, out.data_ptr(), st) == INVALID
    assert lib.lmc_select_topk(ctx.handle, big.data_ptr(), 100, 0, out.data_ptr(), st) == 0  # k == 0 writes nothing
    torch.cuda.synchronize()
    assert bool((out == -7).all()) and ctx.status(clear=True) == 0
    # blend.select_tokens: min(k, T) indices, int32, ascending
    dev_t = torch.tensor([1.0, 9.0, 3.0, 9.0, float("nan")], device=DEV)
    assert blend.select_tokens(dev_t, 2).tolist() == [1, 4] and blend.select_tokens(dev_t, 3).tolist() == [1, 3, 4]
    assert blend.select_tokens(dev_t, 9).tolist() == [0, 1, 2, 3, 4] and blend.select_tokens(dev_t, 0).numel() == 0
    assert blend.select_tokens(dev_t, 2).dtype == torch.int32


# ------------------------------------------------------------------ 6. the flow
def _gather(caches, slots, layout, kv):
    """[T, H, D] of one layer's cache at `slots`."""
    blk, off = slots // BS, slots % BS
    c = caches
    if layout == "NBHD":
        return c[kv][blk, off]
    if kv == 1:
        return c[1][blk, :, :, off]
    _, nb, H, D, _ = c.shape
    return c[0].view(nb, H, D // 8, BS, 8)[blk, :, :, off].reshape(len(slots), H, D)


def test_store_retrieve_with_rope_then_select_recompute():
    """A segment stored on its own, retrieved at new positions into an NHDB and an NBHD cache, the check layer "recomputed"
    as the cache's own content with V of six known tokens moved far away: select_recompute names exactly those six, and
    with two of them masked out (and the ratio for four of 38) the other four."""
    L, H, D, T, cs, dt = 2, 2, 64, 40, 16, torch.bfloat16
    g = torch.Generator().manual_seed(23)
    tokens = generate_tokens(T, DEV)
    kv = tuple((torch.rand((T, H, D), generator=g).to(dt).to(DEV), torch.rand((T, H, D), generator=g).to(dt).to(DEV))
               for _ in range(L))
    rope = RopeShift.from_base(10000.0, D, 64, DEV, delta=7)
    S = [3, 11, 16, 17, 30, 39]
    engine = LMCacheEngine(make_cfg("cachegen-hbm", cs), dumb_metadata("vllm", "Llama-3-8B"))
    try:
        engine.store(tokens, kv)
        for layout, mapping in (("NHDB", "blocks"), ("NHDB", "random"), ("NBHD", "random")):
            shape = (2, NBLOCKS, H, D, BS) if layout == "NHDB" else (2, NBLOCKS, BS, H, D)
            caches = [_random_bits(shape, dt, g).to(DEV) for _ in range(L)]
            slots = _slots(mapping, T, g).to(DEV)
            ret_mask = engine.retrieve_into_paged(tokens, caches, slots, BS, layout, rope=rope)
            assert bool(ret_mask.all())
            fresh_k = _gather(caches[1], slots, layout, 0).contiguous()
            fresh_v = _gather(caches[1], slots, layout, 1).contiguous()
            assert torch.isfinite(fresh_v.float()).all()
            fresh_v[S] += 64.0
            got = blend.select_recompute(fresh_k, fresh_v, caches, 1, slots, BS, layout, planes="v", ratio=6 / 40)
            assert got.dtype == torch.int32 and got.tolist() == S, f"{layout} {mapping}"
            assert blend.select_recompute(fresh_k, fresh_v, caches, 1, slots, BS, layout, ratio=6 / 40, mask=ret_mask).tolist() == S
            # the keys agree everywhere: with planes="k" every deviation is 0 and the ties go to the first tokens
            assert blend.select_recompute(fresh_k, fresh_v, caches, 1, slots, BS, layout, planes="k", ratio=6 / 40).tolist() == list(range(6))
            mask = torch.ones(T, dtype=torch.bool)
            mask[[11, 30]] = False
            got = blend.select_recompute(fresh_k, fresh_v, caches, 1, slots, BS, layout, planes="v", ratio=4 / 38, mask=mask)
            assert got.tolist() == [3, 16, 17, 39], f"{layout} {mapping} masked"
            # a masked-out token's slot is never looked up: an entry no cache has does no harm
            wild = slots.clone()
            wild[[11, 30]] = -1
            got = blend.select_recompute(fresh_k, fresh_v, caches, 1, wild, BS, layout, planes="kv", ratio=4 / 38, mask=mask.to(DEV))
            assert got.tolist() == [3, 16, 17, 39]
        torch.cuda.synchronize()
        assert native.get_context(0).status(clear=True) == 0
    finally:
        engine.close()


# ------------------------------------------------------------------ 7. far offsets
@pytest.mark.parametrize("spec", [fo.paged_split(2, False), fo.paged_rows("NBHD", 2, 16, True)], ids=lambda s: s.name)
def test_deviation_reads_blocks_past_2_and_4_gib(ctx, far, spec):
    """The cached side in the far-offset arena: blocks on both sides of 2^31 and 2^32 bytes from the plane base (and the
    arena's last block).  Exact integer data as in test 1; the arena is only read, so it must hold what was placed and
    the fill pattern everywhere else."""
    dt = torch.bfloat16
    g = torch.Generator().manual_seed(31)
    XB = _small_ints((fo.L, 2, fo.T, fo.H, fo.D), dt, g)
    ntok = fo.T - A_TOK0 - 2
    XA = _small_ints((1, 2, ntok, fo.H, fo.D), dt, g)
    far.place(spec, fo.to_bytes(XB))
    layout = far.layout(spec, dt)
    assert (layout.struct.paged_kind == native.PAGED_SPLIT) == (spec.kind == "NHDB")
    a = SideA("slice", XA, g)
    dk, dv = _outputs(ntok)
    ctx.kv_deviation(a.layout, 0, a.tok0, layout, 1, B_TOK0, ntok, dk, dv)
    far.check(f"lmc_kv_deviation over {spec.name}: the arena is only read", (spec, fo.to_bytes(XB)))
    A, B = logical(XA), logical(XB)
    for kv, t in ((0, dk), (1, dv)):
        got = t.cpu().numpy()
        assert np.array_equal(got[:ntok].astype(np.int64), deviation_ref(A, 0, 0, B, 1, B_TOK0, ntok, kv)), f"{spec.name} plane {'KV'[kv]}"
        assert (got[ntok:] == SENTINEL).all()
    assert ctx.status(clear=True) == 0
