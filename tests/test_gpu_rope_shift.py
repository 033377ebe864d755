"""lmc_rope_shift (include/lmc_hip.h, csrc/k_rope.h) on the GPU, and retrieve_into_paged(..., rope=...).

The reference is the header's formula in torch ON THE CPU (tests/test_rope_host.py: cpu_shift), separate fp32 tensor ops
and one cast, applied to what the GPU memory held before the call, with the table read back from the device.  Every
comparison is on integer views, bit for bit, over the WHOLE storage: the keys in range are finite (randn * 8 with zeros,
a few denormals and values near 1e4 mixed in), everything else -- V, tokens outside the range, channels >= rot_dim,
unused slots -- is random bit patterns, NaNs included, and must come back as it was."""
import ctypes

import pytest
import torch

from lmcache_amd import native
from lmcache_amd.cache_engine import LMCacheEngine
from lmcache_amd.rope import RopeShift
from tests.test_gpu_engine import dumb_metadata, generate_tokens, make_cfg
from tests.test_rope_host import ACCURACY_DELTAS, cpu_shift, rope_accuracy_case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
L, NTOK, NBLOCKS, BS, ROWS = 2, 70, 12, 16, 64
DTYPES = [torch.bfloat16, torch.float16]
LAYOUTS = ["vllm", "huggingface", "tuple", "nbhd_offset5", "nhbd_offset5", "nbhd_random", "nhbd_random", "unaligned"]
# (H, D, rot, neox)
GEOMS = [(2, 128, 128, True), (1, 64, 64, True), (2, 128, 64, True), (1, 80, 80, True), (1, 72, 24, True),
         (2, 64, 64, False), (1, 64, 32, False), (1, 72, 20, False)]
BAD_POSITION = 64  # LMC_STATUS_BAD_POSITION
INVALID = -1       # LMC_ERR_INVALID


def _ibits(t):
    return t.view(torch.int16 if t.dtype.itemsize == 2 else torch.uint8)


def _random_bits(shape, dt, g):
    n = 1
    for s in shape:
        n *= s
    return torch.randint(0, 256, (n * dt.itemsize,), generator=g, dtype=torch.uint8).view(dt).view(shape)


def _finite_keys(shape, dt, g):
    x = torch.randn(shape, generator=g) * 8
    flat = x.view(-1)
    n = flat.numel()
    idx = torch.randperm(n, generator=g)
    flat[idx[:n // 16]] = 0.0
    tiny = torch.finfo(dt).smallest_normal / 4  # a denormal of dt
    flat[idx[n // 16:n // 16 + 6]] = tiny * torch.tensor([1.0, -1.0, 3.0, -3.0, 0.5, -2.0])
    flat[idx[n // 16 + 6:n // 16 + 12]] = torch.tensor([1e4, -1e4, 9984.0, -12000.0, 1.1e4, -9000.0])
    return x.to(dt)


def _mapping(kind, n, nblocks, bs, g):
    if kind == "random":  # every token at a slot of its own
        return torch.randperm(nblocks * bs, generator=g)[:n]
    start = 5  # block-ordered: enters its first block at offset 5 and ends in the middle of its last
    need = (start + n + bs - 1) // bs
    blocks = torch.randperm(nblocks, generator=g)[:need]
    pos = torch.arange(start, start + n)
    return blocks[pos // bs] * bs + pos % bs


class Case:
    """One layout of L layers x NTOK tokens: `cpu` is its whole storage (a list of tensors) on the CPU, `gpu` the copy on
    the device that `layout` points into; get_k / put_k read and write the logical keys [L, T, H, D] of either list."""

    def __init__(self, kind, H, D, dt, g, ntok=NTOK):
        self.kind, self.H, self.D, self.dt, self.T = kind, H, D, dt, ntok
        T = ntok
        self.slots = None
        if kind == "vllm":
            self.cpu = [_random_bits((L, 2, T, H, D), dt, g)]
        elif kind == "huggingface":
            self.cpu = [_random_bits((L, 2, H, T, D), dt, g)]
        elif kind == "tuple":
            self.cpu = [_random_bits((T, H, D), dt, g) for _ in range(2 * L)]
        elif kind == "unaligned":
            self.cpu = [_random_bits((L * 2 * T * H * D + 16,), dt, g)]
        else:
            shape = (2, NBLOCKS, BS, H, D) if kind.startswith("nbhd") else (2, NBLOCKS, H, BS, D)
            self.cpu = [_random_bits(shape, dt, g) for _ in range(L)]
            self.slots = _mapping(kind.split("_")[1], T, NBLOCKS, BS, g)

    def upload(self):
        self.gpu = [t.to(DEV) for t in self.cpu]
        k, s = self.kind, self.gpu
        if k in ("vllm", "huggingface"):
            self.layout = native.KVLayout.from_chunk(s[0], k)
        elif k == "tuple":
            self.layout = native.KVLayout.from_kv_tuple(tuple((s[2 * l], s[2 * l + 1]) for l in range(L)), "vllm")
        elif k == "unaligned":
            chunk = self._chunk_of(s[0])
            assert chunk.data_ptr() % 16 == 2
            self.layout = native.KVLayout.from_chunk(chunk, "vllm")
        else:
            self.layout = native.KVLayout.paged(s, self.slots.to(DEV), BS, "NBHD" if k.startswith("nbhd") else "NHBD")
        assert self.layout.vector_readable() == (k != "unaligned")
        return self

    def _chunk_of(self, flat):
        n = L * 2 * self.T * self.H * self.D
        return flat[1:1 + n].view(L, 2, self.T, self.H, self.D)  # 2 bytes off a 16-byte boundary

    def _planes(self, store):
        """Per layer, a (tensor, index) pair with tensor[index] = the layer's keys [T, H, D]."""
        k = self.kind
        if k == "vllm":
            return [(store[0], (l, 0)) for l in range(L)]
        if k == "unaligned":
            return [(self._chunk_of(store[0]), (l, 0)) for l in range(L)]
        if k == "huggingface":
            return [(store[0].permute(0, 1, 3, 2, 4), (l, 0)) for l in range(L)]
        if k == "tuple":
            return [(store[2 * l], (slice(None),)) for l in range(L)]
        blk, off = self.slots // BS, self.slots % BS
        if k.startswith("nbhd"):
            return [(store[l], (0, blk, off)) for l in range(L)]
        return [(store[l], (0, blk, slice(None), off)) for l in range(L)]

    def get_k(self, store):
        return torch.stack([t[i].clone() for t, i in self._planes(store)])

    def put_k(self, store, K):
        for (t, i), k in zip(self._planes(store), K):
            t[i] = k

    def fill_keys(self, g, tb, n, rot):
        """Finite keys in the rotated channels of tokens [tb, tb + n); everything else keeps its random bits."""
        K = self.get_k(self.cpu)
        K[:, tb:tb + n, :, :rot] = _finite_keys((L, n, self.H, rot), self.dt, g)
        self.put_k(self.cpu, K)
        return self

    def shift_and_check(self, ctx, rope_table, table_cpu, tb, n, rot, neox, delta, what):
        """One lmc_rope_shift of tokens [tb, tb + n) by `delta` (int, or a CPU int32 tensor [n]); the whole storage is
        then compared with the CPU statement applied to what it held before."""
        before = [t.cpu() for t in self.gpu]
        per_tok = isinstance(delta, torch.Tensor)
        ctx.rope_shift(self.layout, tb, n, rope_table, rot, neox, delta=0 if per_tok else delta,
                       deltas=delta.to(DEV) if per_tok else None)
        torch.cuda.synchronize()
        K = self.get_k(before)
        K[:, tb:tb + n] = cpu_shift(K[:, tb:tb + n], table_cpu, delta if per_tok else torch.full((n,), delta), rot, neox)
        self.put_k(before, K)
        for i, (got, want) in enumerate(zip(self.gpu, before)):
            assert torch.equal(_ibits(got.cpu()), _ibits(want)), f"{what}: storage tensor {i} differs"


@pytest.fixture(scope="module")
def ctx():
    native.build()
    return native.get_context(0)


_tables = {}


def _table(rot, rows=ROWS):
    """(device table, the same table read back from the device), shared by the tests and never written."""
    if (rot, rows) not in _tables:
        t = RopeShift.from_base(10000.0, rot, rows, DEV).cos_sin
        _tables[(rot, rows)] = (t, t.cpu())
    return _tables[(rot, rows)]


# ------------------------------------------------------------------ 1. the kernels against the formula
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "H%d_D%d_rot%d_%s" % (g[0], g[1], g[2], "neox" if g[3] else "gptj"))
@pytest.mark.parametrize("kind", LAYOUTS)
@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
def test_shift_equals_the_cpu_formula_bit_for_bit(ctx, dt, kind, geom):
    H, D, rot, neox = geom
    g = torch.Generator().manual_seed(100 * LAYOUTS.index(kind) + GEOMS.index(geom))
    table, table_cpu = _table(rot)
    case = Case(kind, H, D, dt, g).fill_keys(g, 0, NTOK, rot).upload()
    for d in (0, 1, 37, -9, ROWS - 1, -(ROWS - 1)):
        case.shift_and_check(ctx, table, table_cpu, 0, NTOK, rot, neox, d, f"uniform delta {d}")
    deltas = torch.randint(-(ROWS - 1), ROWS, (NTOK,), generator=g, dtype=torch.int32)
    case.shift_and_check(ctx, table, table_cpu, 0, NTOK, rot, neox, deltas, "per-token deltas")
    # a sub-range: the tokens in front of it and behind it hold random bit patterns and keep them
    tb, n = 5, 50
    sub = Case(kind, H, D, dt, g).fill_keys(g, tb, n, rot).upload()
    sub.shift_and_check(ctx, table, table_cpu, tb, n, rot, neox, -9, "sub-range, uniform")
    sub.shift_and_check(ctx, table, table_cpu, tb, n, rot, neox, deltas[:n].contiguous(), "sub-range, per token")
    assert ctx.status(clear=True) == 0


@pytest.mark.parametrize("form", ["vector", "element"])
def test_more_work_than_the_grid_holds(ctx, form):
    """One layer with more work items than 64 workgroups per CU of 256 threads: the grid-stride loop of both forms.
    Only the keys cross to the CPU; V is compared on the device."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    H, D, rot, neox = (32, 128, 128, False) if form == "vector" else (8, 24, 24, True)
    per_token = H * (rot // 8 if form == "vector" else rot // 2)
    T = 64 * cus * 256 // per_token + 37
    dt = torch.bfloat16
    g = torch.Generator(device=DEV).manual_seed(3)
    chunk = torch.randint(-32768, 32768, (1, 2, T, H, D), generator=g, device=DEV, dtype=torch.int16).view(dt)
    chunk[:, 0] = (torch.randn((1, T, H, D), generator=g, device=DEV) * 8).to(dt)
    before_k, before_v = chunk[0, 0].cpu(), chunk[:, 1].clone()
    table, table_cpu = _table(rot)
    deltas = torch.randint(-(ROWS - 1), ROWS, (T,), generator=torch.Generator().manual_seed(4), dtype=torch.int32)
    ctx.rope_shift(native.KVLayout.from_chunk(chunk, "vllm"), 0, T, table, rot, neox, deltas=deltas.to(DEV))
    torch.cuda.synchronize()
    want = cpu_shift(before_k, table_cpu, deltas, rot, neox)
    assert torch.equal(_ibits(chunk[0, 0].cpu()), _ibits(want))
    assert torch.equal(_ibits(chunk[:, 1]), _ibits(before_v))
    assert ctx.status(clear=True) == 0


# ------------------------------------------------------------------ 2. a token outside the table
@pytest.mark.parametrize("kind,geom", [("vllm", (2, 128, 128, True)), ("nhbd_random", (2, 64, 64, False)),
                                       ("unaligned", (1, 72, 24, True))], ids=["neox_vector", "gptj_vector", "element"])
def test_a_delta_outside_the_table_skips_that_token_and_raises_the_status_bit(ctx, kind, geom):
    H, D, rot, neox = geom
    dt = torch.bfloat16
    g = torch.Generator().manual_seed(21)
    table, table_cpu = _table(rot)
    case = Case(kind, H, D, dt, g).fill_keys(g, 0, NTOK, rot).upload()
    deltas = torch.randint(-(ROWS - 1), ROWS, (NTOK,), generator=g, dtype=torch.int32)
    deltas[11], deltas[40] = ROWS, -ROWS
    words = native.StatusWords()
    for job_word in (True, False):  # the job's own word, then the context's sticky one
        before = [t.cpu() for t in case.gpu]
        w = words.acquire() if job_word else None
        ctx.rope_shift(case.layout, 0, NTOK, table, rot, neox, deltas=deltas.to(DEV), job_status=words.ptr(w) if job_word else None)
        torch.cuda.synchronize()
        if job_word:
            assert words.read_release(w) == BAD_POSITION and ctx.status() == 0
        else:
            assert ctx.status(clear=True) == BAD_POSITION and ctx.status() == 0
        K = case.get_k(before)
        ok = torch.ones(NTOK, dtype=torch.bool)
        ok[11] = ok[40] = False
        K[:, ok] = cpu_shift(K[:, ok], table_cpu, deltas[ok], rot, neox)  # the two tokens stay as they were
        case.put_k(before, K)
        for got, want in zip(case.gpu, before):
            assert torch.equal(_ibits(got.cpu()), _ibits(want))
    words.close()


# ------------------------------------------------------------------ 3. refusals
def test_refusals_launch_nothing(ctx):
    H, D, rot = 2, 64, 64
    lib, ref = native.lib(), ctypes.byref
    g = torch.Generator().manual_seed(31)
    st = native.current_stream_ptr(torch.device(DEV))
    table, _ = _table(rot)
    tp = table.data_ptr()
    chunk = _random_bits((L, 2, NTOK, H, D), torch.bfloat16, g).to(DEV)
    rows = native.KVLayout.from_chunk(chunk, "vllm")
    fp8 = _random_bits((L, 2, NTOK, H, D), torch.float8_e4m3fn, g).to(DEV)
    fp8_rows = native.KVLayout.from_chunk(fp8, "vllm")
    split_caches = [_random_bits((2, NBLOCKS, H, D, BS), torch.bfloat16, g).to(DEV) for _ in range(L)]
    split = native.KVLayout.paged(split_caches, _mapping("random", NTOK, NBLOCKS, BS, g).to(DEV), BS, "NHDB")
    keep = [t.clone() for t in [chunk, fp8] + split_caches]

    def call(layout, tok_begin=0, ntok=NTOK, table_ptr=tp, table_rows=ROWS, rot_dim=rot, neox=1, delta=1, deltas=None):
        return lib.lmc_rope_shift(ctx.handle, ref(layout.struct), tok_begin, ntok, table_ptr, table_rows, rot_dim, neox, delta,
                                  deltas, None, st)

    assert call(split) == INVALID
    assert call(fp8_rows) == INVALID
    for r in (0, 3, D + 2, -2):
        assert call(rows, rot_dim=r) == INVALID, r
    assert call(rows, delta=ROWS) == INVALID and call(rows, delta=-ROWS) == INVALID
    assert call(rows, table_ptr=None) == INVALID
    assert call(rows, ntok=0) == INVALID and call(rows, ntok=-1) == INVALID
    assert call(rows, tok_begin=-1) == INVALID
    assert call(rows, table_rows=0) == INVALID
    bad = native.KvLayoutStruct.from_buffer_copy(rows.struct)
    bad.paged_kind = 2
    assert lib.lmc_rope_shift(ctx.handle, ref(bad), 0, NTOK, tp, ROWS, rot, 1, 1, None, None, st) == INVALID
    assert lib.lmc_rope_shift(ctx.handle, None, 0, NTOK, tp, ROWS, rot, 1, 1, None, None, st) == INVALID
    torch.cuda.synchronize()
    for t, k in zip([chunk, fp8] + split_caches, keep):
        assert torch.equal(_ibits(t), _ibits(k))
    assert ctx.status(clear=True) == 0
    # the binding's own checks
    with pytest.raises(ValueError):
        ctx.rope_shift(rows, 0, NTOK, table.to(torch.bfloat16), rot)
    with pytest.raises(ValueError):
        ctx.rope_shift(rows, 0, NTOK, table, rot, deltas=torch.zeros(NTOK - 1, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        ctx.rope_shift(rows, 0, NTOK, table, rot, deltas=torch.zeros(NTOK, dtype=torch.int64, device=DEV))
    with pytest.raises(native.NativeError):
        ctx.rope_shift(rows, 0, NTOK, table, rot, delta=ROWS)
    # ... while the largest delta of the table is taken
    ctx.rope_shift(rows, 0, NTOK, table, rot, delta=ROWS - 1)
    torch.cuda.synchronize()
    assert torch.equal(_ibits(chunk[:, 1]), _ibits(keep[0][:, 1])) and not torch.equal(_ibits(chunk[:, 0]), _ibits(keep[0][:, 0]))


# ------------------------------------------------------------------ 4. the engine
def _paged_k(caches, slots, bs, layout):
    """Per layer a (tensor, index) pair with tensor[index] = the keys [T, H, D] at `slots` (copied from the helpers of
    tests/test_gpu_engine.py and tests/test_gpu_paged_split.py)."""
    blk, off = slots // bs, slots % bs
    out = []
    for c in caches:
        if layout == "NBHD":
            out.append((c, (0, blk, off), None))
        elif layout == "NHBD":
            out.append((c, (0, blk, slice(None), off), None))
        else:  # NHDB: key_cache = cache[0].view(num_blocks, H, D / x, block_size, x), x = 8 for 16-bit elements
            _, nb, H, D, _ = c.shape
            out.append((c[0].view(nb, H, D // 8, bs, 8), (blk, slice(None), slice(None), off), (H, D)))
    return out


def _expect_shifted(caches_cpu, slots, bs, layout, table_cpu, deltas, rot, neox):
    """The CPU formula on the gathered key rows of a cache that was retrieved into WITHOUT rope, scattered back."""
    for t, i, hd in _paged_k(caches_cpu, slots, bs, layout):
        k = t[i].clone()
        rows = k.reshape(k.shape[0], hd[0], hd[1]) if hd else k
        rows = cpu_shift(rows, table_cpu, deltas, rot, neox)
        t[i] = rows.reshape(k.shape) if hd else rows


@pytest.mark.parametrize("geom", [(2, 128, 16), (1, 64, 8)], ids=lambda g: "H%d_D%d_bs%d" % g)
@pytest.mark.parametrize("backend", ["cachegen-host", "cuda"])
def test_retrieve_into_paged_with_rope_equals_retrieve_then_the_cpu_formula(backend, geom):
    H, D, bs = geom
    dt, cs, p = torch.bfloat16, 32, 37
    nb = 2 * ((NTOK + 5 + bs - 1) // bs) + 2
    g = torch.Generator().manual_seed(51)
    tokens = generate_tokens(NTOK, DEV)
    kv = tuple((torch.rand((NTOK, H, D), generator=g).to(dt).to(DEV), torch.rand((NTOK, H, D), generator=g).to(dt).to(DEV))
               for _ in range(L))
    rot, neox = (D, True) if D == 128 else (32, False)  # full NeoX rotary; partial GPT-J rotary
    uniform = RopeShift.from_base(10000.0, rot, 128, DEV, is_neox=neox, delta=p)
    table_cpu = uniform.cos_sin.cpu()
    per_tok = torch.randint(-127, 128, (NTOK,), generator=g, dtype=torch.int32)
    engine = LMCacheEngine(make_cfg(backend, cs), dumb_metadata("vllm", "Llama-3-8B"))
    try:
        engine.store(tokens, kv)

        def fresh(layout):
            shape = {"NBHD": (2, nb, bs, H, D), "NHBD": (2, nb, H, bs, D), "NHDB": (2, nb, H, D, bs)}[layout]
            return [_random_bits(shape, dt, g).to(DEV) for _ in range(L)]

        def into(caches, layout, pair):
            if not pair:
                return caches
            return [(c[0].view(nb, H, D // 8, bs, 8), c[1]) for c in caches]

        def check(layout, pair, kind, mask, rope, deltas):
            slots = _mapping(kind, NTOK, nb, bs, g)
            a = fresh(layout)
            b = [c.clone() for c in a]
            untouched = [c.cpu() for c in a]
            ma = engine.retrieve_into_paged(tokens, into(a, layout, pair), slots.to(DEV), bs, layout, mask=mask, rope=rope)
            mb = engine.retrieve_into_paged(tokens, into(b, layout, pair), slots.to(DEV), bs, layout, mask=mask)
            torch.cuda.synchronize()
            nskip = 0 if mask is None else int((~mask).sum())
            assert torch.equal(ma, mb) and int(ma.sum()) == NTOK - nskip and not ma[:nskip].any()
            plain = [c.cpu() for c in b]
            assert any(not torch.equal(_ibits(x), _ibits(y)) for x, y in zip(plain, untouched)), "nothing was retrieved"
            _expect_shifted(plain, slots[nskip:], bs, layout, table_cpu, deltas[nskip:], rot, neox)
            for l in range(L):  # K shifted, V as retrieved, every slot outside the mapping as it was: the whole cache
                assert torch.equal(_ibits(a[l].cpu()), _ibits(plain[l])), f"{layout} pair={pair} layer {l}"

        everywhere = torch.full((NTOK,), p, dtype=torch.int32)
        tail = torch.ones(NTOK, dtype=torch.bool, device=DEV)
        tail[:40] = False  # a suffix mask of 40 skipped tokens: cuts into the second chunk
        by_token = RopeShift(uniform.cos_sin, rot, neox, per_tok.to(DEV))
        for layout, pair in (("NBHD", False), ("NHBD", False), ("NHDB", False), ("NHDB", True)):
            check(layout, pair, "random", None, uniform, everywhere)
            check(layout, pair, "offset5", None, by_token, per_tok)
            check(layout, pair, "offset5", tail, uniform, everywhere)
            check(layout, pair, "random", tail, by_token, per_tok)  # entry t of the delta tensor belongs to tokens[t]
            # tokens the engine has never seen: all False, the cache keeps every byte
            c = fresh(layout)
            keep = [x.clone() for x in c]
            m = engine.retrieve_into_paged(tokens + 10000, into(c, layout, pair), _mapping("random", NTOK, nb, bs, g).to(DEV), bs,
                                           layout, rope=uniform)
            torch.cuda.synchronize()
            assert not m.any() and all(torch.equal(_ibits(x), _ibits(y)) for x, y in zip(c, keep))
            # rope=None is the call without the keyword
            c, slots = fresh(layout), _mapping("random", NTOK, nb, bs, g).to(DEV)
            c2 = [x.clone() for x in c]
            engine.retrieve_into_paged(tokens, into(c, layout, pair), slots, bs, layout, rope=None)
            engine.retrieve_into_paged(tokens, into(c2, layout, pair), slots, bs, layout)
            torch.cuda.synchronize()
            assert all(torch.equal(_ibits(x), _ibits(y)) for x, y in zip(c, c2))
        # refused before anything is queued
        c = fresh("NBHD")
        keep = [x.clone() for x in c]
        wide = RopeShift.from_base(10000.0, D + 2, 128, DEV, delta=1)
        with pytest.raises(ValueError, match="head size"):
            engine.retrieve_into_paged(tokens, c, _mapping("random", NTOK, nb, bs, g).to(DEV), bs, "NBHD", rope=wide)
        fp8 = [torch.zeros((2, nb, bs, H, D), dtype=torch.uint8, device=DEV).view(torch.float8_e4m3fn) for _ in range(L)]
        with pytest.raises(ValueError, match="fp8"):
            engine.retrieve_into_paged(tokens, fp8, _mapping("random", NTOK, nb, bs, g).to(DEV), bs, "NBHD", rope=uniform)
        torch.cuda.synchronize()
        assert all(torch.equal(_ibits(x), _ibits(y)) for x, y in zip(c, keep))
        assert native.get_context(0).status(clear=True) == 0
    finally:
        engine.close()


# ------------------------------------------------------------------ 5. accuracy against exact positions
@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
def test_shifted_keys_are_within_the_derived_bound_of_the_exact_rotation(ctx, dt):
    """K = dtype(R64(p_old) x) shifted by d on the GPU against R64(p_old + d) x: |err| <= 2.25 u r per component (the
    derivation stands in tests/test_rope_host.py, where the same construction runs on the CPU statement)."""
    g = torch.Generator().manual_seed(0)

    def gpu_shift(K, table, d):
        T, H, rot = K.shape
        chunk = torch.zeros((1, 2, T, H, rot), dtype=K.dtype)
        chunk[0, 0] = K
        chunk = chunk.to(DEV)
        ctx.rope_shift(native.KVLayout.from_chunk(chunk, "vllm"), 0, T, table.to(DEV), rot, True, delta=d)
        torch.cuda.synchronize()
        assert not chunk[0, 1].any()
        return chunk[0, 0].cpu()

    worst = 0.0
    for d in ACCURACY_DELTAS[dt]:
        worst = max(worst, rope_accuracy_case(dt, gpu_shift, d, g))
    print(f"{dt}: worst |err| / (u r) = {worst:.3f}")
    assert worst <= 2.25
    assert ctx.status(clear=True) == 0
