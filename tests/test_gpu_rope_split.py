"""lmc_rope_shift_split (include/lmc_hip.h, csrc/k_rope.h: k_rope_split_vec / k_rope_split_elem) on the GPU: the keys of
an "NHDB" cache (LMC_PAGED_SPLIT) re-rotated where they lie, and the in-place form of lmc_range_post.

The reference is tests/test_rope_host.py::cpu_shift, the CPU statement the row kernels are held to, applied to the keys
gathered from the split cache as it was before the call.  Every comparison is bit for bit on integer views of the WHOLE
key and value storage: it starts from random bit patterns (NaNs included) with finite keys in the rotated channels of
the named tokens only, so a byte written outside the owned granules shows."""
import ctypes

import numpy as np
import pytest
import torch

from lmcache_amd import native
from tests import far_offsets as fo
from tests.test_gpu_rope_shift import BAD_POSITION, INVALID, ROWS, _finite_keys, _ibits, _random_bits, _table
from tests.test_rope_host import cpu_shift

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
L, H, BS, NB, NTOK = 3, 2, 16, 8, 37  # a partial wave and a partial block
DTYPES = [torch.bfloat16, torch.float16]
FORMS = ["tensor", "pair"]  # [2, num_blocks, H, D, bs] per layer, or (key_cache, value_cache)
# (D, rot, neox)
VECTOR = [(64, 64, True), (64, 32, True), (128, 128, True), (32, 16, False), (64, 64, False)]
ELEMENT = [(64, 24, True), (32, 12, False)]
MAPPINGS = ["offset5", "random", "reversed"]


def _geom_id(g):
    return "D%d_rot%d_%s" % (g[0], g[1], "neox" if g[2] else "gptj")


def _slots(kind, n, nblocks, bs, g):
    if kind == "random":
        return torch.randperm(nblocks * bs, generator=g)[:n]
    start = 5  # block-ordered: enters its first block at offset 5 and ends in the middle of its last
    need = (start + n + bs - 1) // bs
    blocks = torch.randperm(nblocks, generator=g)[:need]
    pos = torch.arange(start, start + n)
    s = blocks[pos // bs] * bs + pos % bs
    return s.flip(0) if kind == "reversed" else s


class SplitCase:
    """L layers of an "NHDB" cache: `cpu` is its whole storage (a list of tensors), `gpu` the copy on the device that
    `layout` points into.  form "tensor" / "pair" as KVLayout.paged takes them; "pair_off1": a pair whose key caches begin
    one element behind a 16-byte boundary (the storage is one element longer at either end)."""

    def __init__(self, form, D, dt, g, slots, layers=L, heads=H, nblocks=NB, bs=BS):
        self.form, self.D, self.dt, self.slots = form, D, dt, slots
        self.L, self.H, self.nb, self.bs = layers, heads, nblocks, bs
        n = nblocks * heads * D * bs
        if form == "tensor":
            self.cpu = [_random_bits((2, nblocks, heads, D, bs), dt, g) for _ in range(layers)]
        elif form == "pair":
            self.cpu = [_random_bits((n,), dt, g) for _ in range(2 * layers)]
        else:
            self.cpu = [_random_bits((n + (16 if i % 2 == 0 else 0),), dt, g) for i in range(2 * layers)]

    def _kv(self, store, l):
        nb, Hh, D, bs = self.nb, self.H, self.D, self.bs
        if self.form == "tensor":
            return store[l][0].view(nb, Hh, D // 8, bs, 8), store[l][1]
        k = store[2 * l] if self.form == "pair" else store[2 * l][1:1 + nb * Hh * D * bs]
        return k.view(nb, Hh, D // 8, bs, 8), store[2 * l + 1].view(nb, Hh, D, bs)

    def upload(self):
        self.gpu = [t.to(DEV) for t in self.cpu]
        if self.form == "tensor":
            caches = self.gpu
        else:
            caches = [self._kv(self.gpu, l) for l in range(self.L)]
            if self.form == "pair_off1":
                assert all(k.data_ptr() % 16 == 2 for k, _ in caches)
        self.layout = native.KVLayout.paged(caches, self.slots.to(DEV), self.bs, "NHDB")
        assert self.layout.struct.paged_kind == native.PAGED_SPLIT
        return self

    def get_k(self, store, slots=None):
        """The logical keys [L, T, H, D] at `slots` (default: the case's own)."""
        s = self.slots if slots is None else slots
        blk, off = s // self.bs, s % self.bs
        return torch.stack([self._kv(store, l)[0][blk, :, :, off].reshape(len(s), self.H, self.D) for l in range(self.L)])

    def put_k(self, store, K, slots=None):
        s = self.slots if slots is None else slots
        blk, off = s // self.bs, s % self.bs
        for l in range(self.L):
            self._kv(store, l)[0][blk, :, :, off] = K[l].reshape(len(s), self.H, self.D // 8, 8)

    def fill_keys(self, g, tb, n, rot):
        K = self.get_k(self.cpu)
        K[:, tb:tb + n, :, :rot] = _finite_keys((self.L, n, self.H, rot), self.dt, g)
        self.put_k(self.cpu, K)
        return self

    def snapshot(self):
        return [t.cpu() for t in self.gpu]

    def assert_equals(self, want, what):
        for i, (got, w) in enumerate(zip(self.gpu, want)):
            assert torch.equal(_ibits(got.cpu()), _ibits(w)), f"{what}: storage tensor {i} differs"

    def shift_and_check(self, ctx, table, table_cpu, tb, n, rot, neox, delta, what, layout=None, layers=None):
        """One lmc_rope_shift_split of tokens [tb, tb + n) by `delta` (an int, or a CPU int32 tensor [n]); the whole
        storage is then compared with the CPU statement applied to what it held before."""
        before = self.snapshot()
        per_tok = isinstance(delta, torch.Tensor)
        ctx.rope_shift_split(layout or self.layout, tb, n, table, rot, neox, delta=0 if per_tok else delta,
                             deltas=delta.to(DEV) if per_tok else None)
        torch.cuda.synchronize()
        K = self.get_k(before)
        sel = slice(None) if layers is None else layers
        K[sel, tb:tb + n] = cpu_shift(K[sel, tb:tb + n], table_cpu, delta if per_tok else torch.full((n,), delta), rot, neox)
        self.put_k(before, K)
        self.assert_equals(before, what)


@pytest.fixture(scope="module")
def ctx():
    native.build()
    return native.get_context(0)


# ------------------------------------------------------------------ 1. the kernels against the formula
@pytest.mark.parametrize("geom", VECTOR + ELEMENT, ids=_geom_id)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
def test_shift_in_the_split_cache_equals_the_cpu_formula_bit_for_bit(ctx, dt, form, geom):
    D, rot, neox = geom
    g = torch.Generator().manual_seed(1000 * FORMS.index(form) + 10 * (VECTOR + ELEMENT).index(geom))
    table, table_cpu = _table(rot)
    for kind in MAPPINGS:
        case = SplitCase(form, D, dt, g, _slots(kind, NTOK, NB, BS, g)).fill_keys(g, 0, NTOK, rot).upload()
        for d in (3, -7, 0):
            case.shift_and_check(ctx, table, table_cpu, 0, NTOK, rot, neox, d, f"{kind}: uniform delta {d}")
        deltas = torch.randint(-(ROWS - 1), ROWS, (NTOK,), generator=g, dtype=torch.int32)
        deltas[[4, 20]] = 0
        case.shift_and_check(ctx, table, table_cpu, 0, NTOK, rot, neox, deltas, f"{kind}: per-token deltas")
        # a sub-range: the tokens in front of it and behind it hold random bit patterns and keep them
        sub = SplitCase(form, D, dt, g, _slots(kind, NTOK, NB, BS, g)).fill_keys(g, 5, 20, rot).upload()
        sub.shift_and_check(ctx, table, table_cpu, 5, 20, rot, neox, -7, f"{kind}: sub-range, uniform")
        sub.shift_and_check(ctx, table, table_cpu, 5, 20, rot, neox, deltas[:20].contiguous(), f"{kind}: sub-range, per token")
    assert ctx.status(clear=True) == 0


@pytest.mark.parametrize("geom", [(64, 64, True), (64, 64, False)], ids=_geom_id)
@pytest.mark.parametrize("what", ["key_cache_one_element_off", "table_4_bytes_off"])
@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
def test_the_element_form_takes_what_is_off_a_16_byte_boundary(ctx, dt, what, geom):
    """A geometry the vector form would take, but the key caches begin 2 bytes behind a 16-byte boundary, or the cos/sin
    table 4 bytes behind one: the same bits, and not a byte of the margins."""
    D, rot, neox = geom
    g = torch.Generator().manual_seed(77)
    table, table_cpu = _table(rot)
    if what == "table_4_bytes_off":
        flat = torch.zeros(ROWS * rot + 4, dtype=torch.float32, device=DEV)
        assert flat.data_ptr() % 16 == 0
        flat[1:1 + ROWS * rot] = table.reshape(-1)
        table = flat[1:1 + ROWS * rot].view(ROWS, rot)
        assert table.data_ptr() % 16 == 4 and table.is_contiguous()
    form = "pair_off1" if what == "key_cache_one_element_off" else "pair"
    for kind in MAPPINGS:
        case = SplitCase(form, D, dt, g, _slots(kind, NTOK, NB, BS, g)).fill_keys(g, 0, NTOK, rot).upload()
        case.shift_and_check(ctx, table, table_cpu, 0, NTOK, rot, neox, 3, f"{kind}: uniform")
        deltas = torch.randint(-(ROWS - 1), ROWS, (NTOK,), generator=g, dtype=torch.int32)
        case.shift_and_check(ctx, table, table_cpu, 0, NTOK, rot, neox, deltas, f"{kind}: per token")
    assert ctx.status(clear=True) == 0


@pytest.mark.parametrize("form", ["vector", "element"])
def test_more_work_than_the_grid_holds(ctx, form):
    """One layer with more work items than 64 workgroups per CU of 256 threads (sized as the row kernels' test of that
    name sizes it): the grid-stride loop of both forms.  Only the keys cross to the CPU; the whole caches are compared on
    the device."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    Hh, D, rot, neox = (32, 128, 128, False) if form == "vector" else (8, 24, 24, True)
    per_token = Hh * (rot // 8 if form == "vector" else rot // 2)
    T = 64 * cus * 256 // per_token + 37
    nb, dt = (T + 5 + BS - 1) // BS, torch.bfloat16
    g = torch.Generator(device=DEV).manual_seed(3)
    cache = torch.randint(-32768, 32768, (2, nb, Hh, D, BS), generator=g, device=DEV, dtype=torch.int16).view(dt)
    slots = (torch.arange(T) + 5).to(DEV)  # block-ordered from offset 5 of block 0
    kview = cache[0].view(nb, Hh, D // 8, BS, 8)
    blk, off = slots // BS, slots % BS
    kview[blk, :, :, off] = (torch.randn((T, Hh, D // 8, 8), generator=g, device=DEV) * 8).to(dt)
    before = cache.clone()
    table, table_cpu = _table(rot)
    deltas = torch.randint(-(ROWS - 1), ROWS, (T,), generator=torch.Generator().manual_seed(4), dtype=torch.int32)
    ctx.rope_shift_split(native.KVLayout.paged([cache], slots, BS, "NHDB"), 0, T, table, rot, neox, deltas=deltas.to(DEV))
    torch.cuda.synchronize()
    keys = before[0].view(nb, Hh, D // 8, BS, 8)[blk, :, :, off].reshape(T, Hh, D).cpu()
    want = cpu_shift(keys, table_cpu, deltas, rot, neox)
    before[0].view(nb, Hh, D // 8, BS, 8)[blk, :, :, off] = want.reshape(T, Hh, D // 8, 8).to(DEV)
    assert torch.equal(_ibits(cache), _ibits(before))
    assert ctx.status(clear=True) == 0


# ------------------------------------------------------------------ 2. a token outside the table
@pytest.mark.parametrize("geom", [(64, 64, True), (64, 64, False), (64, 24, True)], ids=["neox_vector", "gptj_vector", "element"])
def test_a_delta_outside_the_table_skips_that_token_and_raises_the_status_bit(ctx, geom):
    D, rot, neox = geom
    dt = torch.bfloat16
    g = torch.Generator().manual_seed(21)
    table, table_cpu = _table(rot)
    case = SplitCase("tensor", D, dt, g, _slots("random", NTOK, NB, BS, g)).fill_keys(g, 0, NTOK, rot).upload()
    deltas = torch.randint(-(ROWS - 1), ROWS, (NTOK,), generator=g, dtype=torch.int32)
    deltas[11] = ROWS
    words = native.StatusWords()
    for job_word in (True, False):  # the job's own word, then the context's sticky one
        before = case.snapshot()
        w = words.acquire() if job_word else None
        ctx.rope_shift_split(case.layout, 0, NTOK, table, rot, neox, deltas=deltas.to(DEV),
                             job_status=words.ptr(w) if job_word else None)
        torch.cuda.synchronize()
        if job_word:
            assert words.read_release(w) == BAD_POSITION and ctx.status() == 0
        else:
            assert ctx.status(clear=True) == BAD_POSITION and ctx.status() == 0
        K = case.get_k(before)
        ok = torch.ones(NTOK, dtype=torch.bool)
        ok[11] = False
        K[:, ok] = cpu_shift(K[:, ok], table_cpu, deltas[ok], rot, neox)  # token 11 stays as it was
        case.put_k(before, K)
        case.assert_equals(before, "job word" if job_word else "sticky word")
    words.close()


# ------------------------------------------------------------------ 3. a window of layers
@pytest.mark.parametrize("form", FORMS)
def test_a_layer_window_changes_its_layer_only_and_as_the_whole_call_does(ctx, form):
    D, rot = 64, 64
    g = torch.Generator().manual_seed(41)
    table, table_cpu = _table(rot)
    slots = _slots("random", NTOK, NB, BS, g)
    deltas = torch.randint(-(ROWS - 1), ROWS, (NTOK,), generator=g, dtype=torch.int32)
    whole = SplitCase(form, D, torch.bfloat16, g, slots).fill_keys(g, 0, NTOK, rot)
    part = SplitCase(form, D, torch.bfloat16, g, slots)
    part.cpu = [t.clone() for t in whole.cpu]
    whole.upload(), part.upload()
    ctx.rope_shift_split(whole.layout, 0, NTOK, table, rot, True, deltas=deltas.to(DEV))
    part.shift_and_check(ctx, table, table_cpu, 0, NTOK, rot, True, deltas, "layers(1, 1)", layout=part.layout.layers(1, 1),
                         layers=slice(1, 2))
    kw, kp = whole.get_k(whole.snapshot()), part.get_k(part.snapshot())
    assert torch.equal(_ibits(kw[1]), _ibits(kp[1])) and not torch.equal(_ibits(kw[0]), _ibits(kp[0]))
    assert ctx.status(clear=True) == 0


# ------------------------------------------------------------------ 4. blocks past 4 GiB of the cache
@pytest.fixture(scope="module")
def arena():
    native.build()
    free, need = torch.cuda.mem_get_info()[0], fo.ARENA_BYTES + 4 * fo.GIB
    if free < need:
        pytest.skip(f"far-offset arena: {free} bytes of device memory are free, {need} are needed")
    a = torch.full((fo.ARENA_BYTES,), fo.FILL, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    yield a
    del a
    torch.cuda.empty_cache()


def test_rotated_blocks_past_4_gib_of_the_cache(ctx, arena):
    """The "NHDB" layout of tests/far_offsets.py (blocks at 0, on both sides of 2^31 and of 2^32 bytes and at the arena's
    end; safety held by tests/test_far_offsets_host.py): rot 64 is the vector form, rot 24 the element form.  After each
    call the arena holds the CPU statement's keys at the layout's elements and the fill pattern everywhere else."""
    spec = fo.REGISTRY[fo.paged_split(2, False).name]
    dt, T = torch.bfloat16, fo.T
    assert int(spec.block_off().max()) > (1 << 32)
    g = torch.Generator().manual_seed(8)
    x = _random_bits((fo.L, 2, T, fo.H, fo.D), dt, g)
    x[:, 0] = _finite_keys((fo.L, T, fo.H, fo.D), dt, g)
    starts, img = fo.expected_windows(*spec.pieces(fo.to_bytes(x)))
    fo.write_windows(arena, starts, img)
    layout = native.KVLayout.paged(spec.views(arena, dt), torch.from_numpy(spec.slots).to(DEV), spec.bs, "NHDB")
    try:
        for rot, neox in ((64, True), (24, True)):
            table, table_cpu = _table(rot)
            deltas = torch.randint(-(ROWS - 1), ROWS, (T,), generator=g, dtype=torch.int32)
            for delta in (-9, deltas):
                per_tok = isinstance(delta, torch.Tensor)
                ctx.rope_shift_split(layout, 0, T, table, rot, neox, delta=0 if per_tok else delta,
                                     deltas=delta.to(DEV) if per_tok else None)
                torch.cuda.synchronize()
                x[:, 0] = cpu_shift(x[:, 0], table_cpu, delta if per_tok else torch.full((T,), delta), rot, neox)
                off, data = spec.pieces(fo.to_bytes(x))
                byte = (off[:, None] + np.arange(data.shape[1], dtype=np.int64)).reshape(-1)
                fo.check_arena(arena, byte, data.reshape(-1, 1), f"{spec.name} rot {rot} {'per token' if per_tok else 'uniform'}")
        assert ctx.status(clear=True) == 0
    finally:
        torch.cuda.synchronize()
        fo.restore_windows(arena, starts)


# ------------------------------------------------------------------ 5. refusals
def test_refusals_launch_nothing(ctx):
    D, rot = 64, 64
    lib, ref = native.lib(), ctypes.byref
    g = torch.Generator().manual_seed(31)
    st = native.current_stream_ptr(torch.device(DEV))
    table, _ = _table(rot)
    tp = table.data_ptr()
    slots = _slots("random", NTOK, NB, BS, g).to(DEV)
    caches = [_random_bits((2, NB, H, D, BS), torch.bfloat16, g).to(DEV) for _ in range(L)]
    split = native.KVLayout.paged(caches, slots, BS, "NHDB")
    fp8 = [_random_bits((2, NB, H, D, BS), torch.float8_e4m3fn, g).to(DEV) for _ in range(L)]
    fp8_split = native.KVLayout.paged(fp8, slots, BS, "NHDB")
    chunk = _random_bits((L, 2, NTOK, H, D), torch.bfloat16, g).to(DEV)
    rows = native.KVLayout.from_chunk(chunk, "vllm")
    nhbd = [_random_bits((2, NB, H, BS, D), torch.bfloat16, g).to(DEV) for _ in range(L)]
    paged_rows = native.KVLayout.paged(nhbd, slots, BS, "NHBD")
    everything = caches + fp8 + [chunk] + nhbd
    keep = [t.clone() for t in everything]

    def call(layout, tok_begin=0, ntok=NTOK, table_ptr=tp, table_rows=ROWS, rot_dim=rot, neox=1, delta=1, deltas=None, handle=None):
        return lib.lmc_rope_shift_split(ctx.handle if handle is None else handle, ref(layout.struct), tok_begin, ntok, table_ptr,
                                        table_rows, rot_dim, neox, delta, deltas, None, st)

    assert call(rows) == INVALID and call(paged_rows) == INVALID  # rows: lmc_rope_shift takes those
    assert call(fp8_split) == INVALID
    for r in (3, 63, D + 2, D + 16, 1, 0, -2):
        assert call(split, rot_dim=r) == INVALID, r
    assert call(split, delta=ROWS) == INVALID and call(split, delta=-ROWS) == INVALID
    assert call(split, ntok=0) == INVALID and call(split, ntok=-1) == INVALID
    assert call(split, tok_begin=-1) == INVALID
    assert call(split, table_ptr=None) == INVALID
    assert call(split, table_rows=0) == INVALID
    assert call(split, handle=ctypes.c_void_p(None)) == INVALID
    assert lib.lmc_rope_shift_split(ctx.handle, None, 0, NTOK, tp, ROWS, rot, 1, 1, None, None, st) == INVALID
    bad = native.KvLayoutStruct.from_buffer_copy(split.struct)
    bad.paged_kind = 2
    assert lib.lmc_rope_shift_split(ctx.handle, ref(bad), 0, NTOK, tp, ROWS, rot, 1, 1, None, None, st) == INVALID
    # ... and lmc_rope_shift keeps refusing the split cache
    assert lib.lmc_rope_shift(ctx.handle, ref(split.struct), 0, NTOK, tp, ROWS, rot, 1, 1, None, None, st) == INVALID
    with pytest.raises(native.NativeError):
        ctx.rope_shift_split(rows, 0, NTOK, table, rot)
    with pytest.raises(ValueError):
        ctx.rope_shift_split(split, 0, NTOK, table, rot, deltas=torch.zeros(NTOK - 1, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    for t, k in zip(everything, keep):
        assert torch.equal(_ibits(t), _ibits(k))
    assert ctx.status(clear=True) == 0
    # ... while the largest delta of the table is taken
    ctx.rope_shift_split(split, 0, NTOK, table, rot, delta=ROWS - 1)
    torch.cuda.synchronize()
    assert all(torch.equal(_ibits(c[1]), _ibits(k[1])) for c, k in zip(caches, keep))
    assert all(not torch.equal(_ibits(c[0]), _ibits(k[0])) for c, k in zip(caches, keep))


# ------------------------------------------------------------------ 6. the in-place form of lmc_range_post
def _blobs(ctx, kv, cs, fixed):
    Lb, _, T, Hh, D = kv.shape
    n = (T + cs - 1) // cs
    stride = native.r16(native.blob_bound(Lb, cs, Hh, D))
    arena = torch.zeros(n * stride, dtype=torch.uint8, device=DEV)
    sizes = torch.zeros(n, dtype=torch.int32, device=DEV)
    call = ctx.encode_chunks_fixed if fixed else ctx.encode_chunks
    call(native.KVLayout.from_chunk(kv, "vllm"), 0, T, cs, [32, 32, 32, 16, 16, 16], arena.data_ptr(), stride, sizes.data_ptr())
    torch.cuda.synchronize()
    assert ctx.status(clear=True) == 0
    table = torch.tensor([arena.data_ptr() + i * stride for i in range(n)], dtype=torch.int64).to(DEV)
    return arena, table, stride, n


@pytest.mark.parametrize("per_token", [False, True], ids=["uniform", "per_token"])
@pytest.mark.parametrize("fixed", [False, True], ids=["schedule_post", "fixed_split_schedule"])
def test_a_range_post_that_names_its_split_destination_rotates_in_place(ctx, fixed, per_token):
    """Two ranges with events: behind the last event the cache equals decode-then-lmc_rope_shift_split over all layers.
    A post whose scatter_dst differs from `dst` in any one field, or whose scatter_tok0 is not tok_begin, is
    LMC_ERR_INVALID with nothing queued -- as the rotation of a split `dst` without a scatter_dst stays."""
    Lb, T, D, cs, rot = 3, 80, 64, 32, 64
    g = torch.Generator().manual_seed(5 + fixed)
    kv = torch.randn((Lb, 2, T, H, D), generator=g).to(torch.bfloat16).to(DEV)
    arena, table, stride, n = _blobs(ctx, kv, cs, fixed)
    nb = 8
    slots = _slots("random", T, nb, BS, g).to(DEV)
    start = [_random_bits((2, nb, H, D, BS), torch.bfloat16, g).to(DEV) for _ in range(Lb)]
    rope_table, _ = _table(rot)
    deltas = torch.randint(-(ROWS - 1), ROWS, (T,), generator=g, dtype=torch.int32).to(DEV) if per_token else None
    schedule = ctx.decode_chunks_fixed_split_schedule if fixed else ctx.decode_chunks_schedule_post

    def run(caches, post, events=None):
        dst = native.KVLayout.paged(caches, slots, BS, "NHDB")
        p = None if post is None else post(dst)
        if fixed:
            schedule(table.data_ptr(), stride, n, dst, 0, cs, [1, 3], events, post=p)
        else:
            schedule(table.data_ptr(), stride, n, dst, 0, cs, [1, 3], events, p)
        return dst

    # the reference: the plain direct decode, then one lmc_rope_shift_split over all layers
    want = [c.clone() for c in start]
    dst = run(want, None)
    ctx.rope_shift_split(dst, 0, T, rope_table, rot, True, delta=0 if per_token else 11, deltas=deltas)
    torch.cuda.synchronize()
    assert any(not torch.equal(_ibits(a), _ibits(b)) for a, b in zip(want, start))

    def in_place(dst, **kw):
        return native.RangePost(cos_sin=rope_table, rot_dim=rot, is_neox=True, delta=0 if per_token else 11, deltas=deltas,
                                scatter_dst=dst, **kw).struct(0, T)
    got = [c.clone() for c in start]
    evs = [native.NativeEvent() for _ in range(2)]
    run(got, in_place, evs)
    evs[-1].synchronize()
    for l in range(Lb):
        assert torch.equal(_ibits(got[l]), _ibits(want[l])), f"layer {l}"
    torch.cuda.synchronize()
    ctx.raise_on_status("decode")

    # refused before anything is queued
    untouched = [c.clone() for c in start]
    holders = []

    def differs(field, value):
        def post(dst):
            other = native.KVLayout(native.KvLayoutStruct.from_buffer_copy(dst.struct), dst._keep, dst.ntokens, dst.device)
            setattr(other.struct, field, value(getattr(dst.struct, field)))
            holders.append(other)
            return in_place(other)
        return post
    bad = [differs(f, lambda v: (v or 0) + 16) for f in ("base", "plane_ptrs", "stride_layer", "stride_kv", "stride_token",
                                                         "stride_head", "slot_mapping", "stride_block")]
    bad += [differs("dtype", lambda v: 1 - v), differs("num_layers", lambda v: v - 1), differs("num_heads", lambda v: v + 1),
            differs("head_size", lambda v: v + 8), differs("block_size", lambda v: 2 * v), differs("paged_kind", lambda v: 0)]
    bad.append(lambda dst: in_place(dst, scatter_tok0=1))
    bad.append(lambda dst: native.RangePost(cos_sin=rope_table, rot_dim=rot, delta=11).struct(0, T))  # no scatter_dst: as before
    for i, post in enumerate(bad):
        with pytest.raises(native.NativeError):
            run(untouched, post)
        torch.cuda.synchronize()
        assert all(torch.equal(_ibits(a), _ibits(b)) for a, b in zip(untouched, start)), f"refusal {i} wrote"
    assert ctx.status(clear=True) == 0
