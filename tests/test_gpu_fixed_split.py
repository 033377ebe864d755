"""The fixed-width model (LMC_MODEL_FIXED) straight from and into vLLM's ROCm paged-attention cache ("NHDB",
LMC_PAGED_SPLIT): k_fixed.h's split instances behind lmc_encode_chunks_fixed_split and
lmc_decode_chunks_fixed_split_schedule, and the engine's direct paths on local_serde="cachegen-fixed".

Nothing here has a tolerance.  A blob coded from the split cache is, byte for byte, the numpy reference's blob
(tests/fixed_model.py over the oracle's quantisation) of the tokens gathered by torch indexing, and the blob
lmc_encode_chunks_fixed writes from that chunk.  A decode into the split cache leaves the WHOLE cache equal to the
oracle's decode of the blob scattered by torch indexing into a clone: one stray element anywhere fails.  Shapes are the
coded split tests' (tests/test_gpu_split_encode.py): L = 2, 70 tokens in chunks of 32 -- two full chunks and a ragged
one of 6 tokens, a partial oct."""
import ctypes

import numpy as np
import pytest
import torch

from lmcache_amd import native
from lmcache_amd.cache_engine import LMCacheEngine
from lmcache_amd.config import LMCacheEngineConfig
from lmcache_amd.rope import RopeShift
from tests import far_offsets as fo
from tests import fixed_model as fm
from tests.test_gpu_engine import dumb_metadata, generate_tokens
from tests.test_gpu_paged_split import (DEV, L, NTOK, _ibits, _mapping, _nblocks, _random, _split_caches, _torch_gather,
                                        _torch_scatter, _views)

pytestmark = pytest.mark.gpu

CS = 32
BINS = [32, 16, 16, 32]  # K of layer 0 / 1, V of layer 0 / 1: a wide (5-bit) and a narrow (4-bit) plane on each side
BF16, FP16 = torch.bfloat16, torch.float16
NAMES = {BF16: "bf16", FP16: "fp16"}
INVALID = -1
BAD_HEADER, BAD_STREAM, BAD_SCALES = 2, 4, 16

# (H, D, bs): G = 16 (four octs per wave), two heads, G = 32, a second group of 16 live channels, block size 32
GEOMS = [(1, 64, 8), (2, 64, 16), (2, 128, 16), (1, 80, 16), (2, 64, 32)]
KINDS = ["blocks", "offset5", "random", "broken", "unaligned"]
# every geometry with every mapping; the dtype walks with the mapping, so every geometry meets both; and the 1024-channel
# instance (G = 64, two channel runs per lane) once
CASES = [(geom, KINDS[k], (BF16, FP16)[(gi + k) % 2]) for gi, geom in enumerate(GEOMS) for k in range(5)]
CASES.append(((8, 128, 16), "blocks", BF16))
IDS = ["H%d_D%d_bs%d-%s-%s" % (g + (k, NAMES[d])) for g, k, d in CASES]


@pytest.fixture(scope="module")
def ctx():
    native.build()
    return native.get_context(0)


def _finite(shape, dt, g):
    """Random bit patterns of dt made finite (CPU)."""
    x = _random(shape, dt, g)
    return torch.nan_to_num(x.float(), nan=1.0, posinf=2.0, neginf=-2.0).clamp(-1e4, 1e4).to(dt)


def _code(oracle, dt):
    return oracle.BF16 if dt == BF16 else oracle.FP16


def _reference_blobs(oracle, x, cs, H, D, bins):
    """The numpy reference's blob of every chunk of x [L, 2, T, H, D] (CPU)."""
    out = []
    for t0 in range(0, x.shape[2], cs):
        part = x[:, :, t0:t0 + cs].reshape(x.shape[0], 2, -1, H * D).contiguous()
        bits, code = oracle.torch_to_bits(part)
        out.append(fm.encode_blob(oracle, bits, code, H, D, np.array(bins, np.int32)))
    return out


def _encode(ctx, fn, layout, ntok, cs, bins=BINS):
    """fn (ctx.encode_chunks_fixed / _fixed_split) -> (sizes, [blob bytes], the arena, its stride)."""
    stride = native.r16(native.blob_bound(layout.L, cs, layout.H, layout.D))
    n = (ntok + cs - 1) // cs
    arena = torch.zeros(n * stride, dtype=torch.uint8, device=DEV)
    sizes = torch.zeros(n, dtype=torch.int32, device=DEV)
    fn(layout, 0, ntok, cs, bins, arena.data_ptr(), stride, sizes.data_ptr())
    torch.cuda.synchronize()
    assert ctx.status(clear=True) == 0
    sz, host = sizes.cpu().tolist(), arena.cpu().numpy()
    return sz, [host[i * stride:i * stride + sz[i]].tobytes() for i in range(n)], arena, stride


def _host_gather(caches, slots, bs, dt):
    """[L, 2, T, H, D] of dt: the tokens' elements by torch indexing on host copies of the caches."""
    return _torch_gather([c.cpu() for c in caches], slots.cpu(), bs).view(dt).contiguous()


# ------------------------------------------------------------------ 1. encode
@pytest.mark.parametrize("geom,kind,dt", CASES, ids=IDS)
def test_blobs_from_the_split_cache_equal_the_reference_and_the_row_encode(ctx, oracle, geom, kind, dt):
    H, D, bs = geom
    g = torch.Generator().manual_seed(100 * H + D + bs + KINDS.index(kind))
    nb = _nblocks(bs)
    x = _finite((L, 2, NTOK, H, D), dt, g)
    caches = _split_caches(H, D, bs, dt, g, unaligned=kind == "unaligned", nblocks=nb)  # foreign slots: other random bits
    slots = _mapping(kind, NTOK, nb, bs, g).to(DEV)
    _torch_scatter(caches, _ibits(x.to(DEV)), slots, bs)
    before = [c.clone() for c in caches]
    chunk = _host_gather(caches, slots, bs, dt)
    assert torch.equal(_ibits(chunk), _ibits(x))
    split = native.KVLayout.paged(caches, slots, bs, "NHDB")
    sz_s, blobs_s, _, _ = _encode(ctx, ctx.encode_chunks_fixed_split, split, NTOK, CS)
    sz_r, blobs_r, _, _ = _encode(ctx, ctx.encode_chunks_fixed, native.KVLayout.from_chunk(chunk.to(DEV), "vllm"), NTOK, CS)
    want = _reference_blobs(oracle, chunk, CS, H, D, BINS)
    assert len(blobs_s) == 3 and sz_s == sz_r == [len(b) for b in want]
    for i in range(3):
        assert blobs_s[i] == want[i], f"chunk {i}: split source vs the numpy reference"
        assert blobs_s[i] == blobs_r[i], f"chunk {i}: split source vs lmc_encode_chunks_fixed on the gathered chunk"
    for c, b in zip(caches, before):
        assert torch.equal(_ibits(c), _ibits(b)), "the cache keeps its bits"


# ------------------------------------------------------------------ 2. decode
class _Blobs:
    """NTOK tokens of finite random bf16 KV of geometry (H, D), encoded once from rows in chunks of CS: the blobs on the
    device, their pointer table, and -- per destination dtype and dst_tok0 -- the oracle's decode of them."""

    def __init__(self, ctx, oracle, H, D):
        g = torch.Generator().manual_seed(7 * H + D)
        self.x = _finite((L, 2, NTOK, H, D), BF16, g)
        self.H, self.D, self.oracle = H, D, oracle
        rows = native.KVLayout.from_chunk(self.x.to(DEV), "vllm")
        self.sizes, self.bytes, self.arena, self.stride = _encode(ctx, ctx.encode_chunks_fixed, rows, NTOK, CS)
        self.n = len(self.sizes)
        self.table = torch.tensor([self.arena.data_ptr() + i * self.stride for i in range(self.n)], dtype=torch.int64).to(DEV)
        self._want = {}

    def chunk_bits(self, dt, tok0=0):
        """int16 [L, 2, NTOK + tok0, H, D] on the device: the oracle's decode to dt, the first -tok0 tokens dropped."""
        if (dt, tok0) not in self._want:
            o = self.oracle
            dec = np.concatenate([fm.decode_blob(o, b, _code(o, dt)) for b in self.bytes], axis=2)
            t = torch.from_numpy(dec.view(np.int16).reshape(L, 2, NTOK, self.H, self.D)[:, :, -tok0:].copy())
            self._want[(dt, tok0)] = t.to(DEV)
        return self._want[(dt, tok0)]


@pytest.fixture(scope="module")
def blobs(ctx, oracle):
    made = {}

    def get(H, D):
        if (H, D) not in made:
            made[(H, D)] = _Blobs(ctx, oracle, H, D)
        return made[(H, D)]
    return get


def _case(b, dt, bs, kind, g, tok0=0):
    """(caches of random bits, expected caches, layout, slots): the expectation is the oracle's decode scattered by torch."""
    n = NTOK + tok0
    nb = _nblocks(bs)
    caches = _split_caches(b.H, b.D, bs, dt, g, unaligned=kind == "unaligned", nblocks=nb)
    slots = _mapping(kind, n, nb, bs, g).to(DEV)
    expect = [c.clone() for c in caches]
    _torch_scatter(expect, b.chunk_bits(dt, tok0), slots, bs)
    return caches, expect, native.KVLayout.paged(caches, slots, bs, "NHDB"), slots


def _decode(ctx, b, dst, tok0=0, ends=None, events=None, table=None):
    ctx.decode_chunks_fixed_split_schedule((b.table if table is None else table).data_ptr(), b.stride, b.n, dst, tok0, CS,
                                           ends or [dst.L], events)
    torch.cuda.synchronize()
    return ctx.status(clear=True)


def _same(caches, expect, what):
    torch.cuda.synchronize()
    for l, (c, e) in enumerate(zip(caches, expect)):
        assert torch.equal(_ibits(c), _ibits(e)), f"{what}: layer {l}"


@pytest.mark.parametrize("geom,kind,dt", CASES, ids=IDS)
def test_decode_into_the_split_cache_equals_the_oracles_decode_scattered(ctx, blobs, geom, kind, dt):
    H, D, bs = geom
    b = blobs(H, D)
    g = torch.Generator().manual_seed(11 * H + D + bs + KINDS.index(kind))
    caches, expect, split, _ = _case(b, dt, bs, kind, g)
    assert _decode(ctx, b, split) == 0
    _same(caches, expect, kind)


@pytest.mark.parametrize("kind,dt", [("blocks", BF16), ("random", FP16), ("offset5", FP16)], ids=["blocks-bf16", "random-fp16", "offset5-fp16"])
def test_first_chunk_trim_and_a_schedule_of_two_ranges_with_events(ctx, blobs, kind, dt):
    """dst_tok0 = -5: the first five tokens are dropped (never looked up in slot_mapping: the mapping has five entries
    fewer), so the trim cuts the first oct and moves every later one off the destination's multiples of eight.  Then two
    ranges, [0, 1) and [1, 2), each with its event."""
    H, D, bs = 2, 128, 16
    b = blobs(H, D)
    g = torch.Generator().manual_seed(21 + KINDS.index(kind))
    caches, expect, split, slots = _case(b, dt, bs, kind, g, tok0=-5)
    assert slots.numel() == NTOK - 5
    assert _decode(ctx, b, split, tok0=-5) == 0
    _same(caches, expect, "trim")
    caches, expect, split, _ = _case(b, dt, bs, kind, g)
    evs = [native.NativeEvent(timing=True) for _ in range(2)]
    assert _decode(ctx, b, split, ends=[1, L], events=evs) == 0
    assert all(e.query() for e in evs)
    ms = ctypes.c_float(-1.0)
    native.check(native.lib().lmc_event_elapsed_ms(evs[0].handle, evs[1].handle, ctypes.byref(ms)))
    assert ms.value >= 0.0
    _same(caches, expect, "two ranges")


def test_a_launch_writes_the_planes_of_its_layers_only(ctx, blobs):
    """A blob of layer 1 alone into a one-layer layout over layer 1's cache: that cache holds layer 1 of the whole decode
    (a plane is quantised on its own), layer 0's cache keeps every bit."""
    H, D, bs, dt = 2, 128, 16, BF16
    b = blobs(H, D)
    g = torch.Generator().manual_seed(23)
    caches, expect, _, slots = _case(b, dt, bs, "blocks", g)
    keep0 = caches[0].clone()
    one = native.KVLayout.from_chunk(b.x[1:2].contiguous().to(DEV), "vllm")
    sizes, _, arena, stride = _encode(ctx, ctx.encode_chunks_fixed, one, NTOK, CS, bins=[BINS[1], BINS[L + 1]])
    table = torch.tensor([arena.data_ptr() + i * stride for i in range(len(sizes))], dtype=torch.int64).to(DEV)
    dst = native.KVLayout.paged(caches[1:], slots, bs, "NHDB")
    ctx.decode_chunks_fixed_split_schedule(table.data_ptr(), stride, len(sizes), dst, 0, CS, [1], None)
    torch.cuda.synchronize()
    assert ctx.status(clear=True) == 0
    assert torch.equal(_ibits(caches[0]), _ibits(keep0))
    assert torch.equal(_ibits(caches[1]), _ibits(expect[1]))


# ------------------------------------------------------------------ 3. blocks past 4 GiB
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


@pytest.mark.parametrize("swapped", [False, True], ids=["runs", "swapped"])
def test_blocks_beyond_4_gib_from_the_plane_base(ctx, oracle, arena, swapped):
    """far_offsets.paged_split (a layout whose safety tests/test_far_offsets_host.py has checked): blocks on both sides of
    2^31 and 2^32 bytes from the plane base and the arena's last one -- the 64-bit block offset of the loads and of the
    stores, as runs (the V form, the 16-byte stores) and with neighbours swapped (element by element)."""
    spec = fo.REGISTRY[fo.paged_split(2, swapped).name]
    H, D, T, cs, bs = fo.H, fo.D, fo.T, fo.CS, spec.bs
    assert (fo.L, len(BINS)) == (L, 2 * L) and int(spec.block_off().max()) > 4 * fo.GIB
    g = torch.Generator().manual_seed(50 + swapped)
    x = _finite((L, 2, T, H, D), BF16, g)
    starts, img = fo.expected_windows(*spec.pieces(fo.to_bytes(x)))
    fo.write_windows(arena, starts, img)
    touched = [starts]
    try:
        layout = native.KVLayout.paged(spec.views(arena, BF16), torch.from_numpy(spec.slots).to(DEV), bs, "NHDB")
        assert layout.struct.paged_kind == native.PAGED_SPLIT and layout.struct.stride_block * 2 == fo.STRIDE_BLOCK
        sz_s, blobs_s, dev, stride = _encode(ctx, ctx.encode_chunks_fixed_split, layout, T, cs)
        sz_r, blobs_r, _, _ = _encode(ctx, ctx.encode_chunks_fixed, native.KVLayout.from_chunk(x.to(DEV), "vllm"), T, cs)
        want = _reference_blobs(oracle, x, cs, H, D, BINS)
        assert sz_s == sz_r == [len(b) for b in want]
        assert blobs_s == blobs_r and blobs_s == want
        assert np.array_equal(fo.read_windows(arena, starts), img), "the cache keeps its bytes"
        # ... and back: the blobs into the same far blocks of an arena that holds nothing but the fill pattern
        fo.restore_windows(arena, starts)
        table = torch.tensor([dev.data_ptr() + i * stride for i in range(len(sz_s))], dtype=torch.int64).to(DEV)
        ctx.decode_chunks_fixed_split_schedule(table.data_ptr(), stride, len(sz_s), layout, 0, cs, [L], None)
        torch.cuda.synchronize()
        assert ctx.status(clear=True) == 0
        dec = np.concatenate([fm.decode_blob(oracle, b, oracle.BF16) for b in want], axis=2).reshape(L, 2, T, H, D)
        touched.append(fo.check_arena(arena, *spec.pieces(np.ascontiguousarray(dec).view(np.uint8).reshape(L, 2, T, H, 2 * D)),
                                      what=f"decode into {spec.name}"))
    finally:
        torch.cuda.synchronize()
        for s in touched:
            fo.restore_windows(arena, s)
        ctx.status(clear=True)


# ------------------------------------------------------------------ 4. refusals launch nothing; rows pass through
def test_refusals_launch_nothing_and_rows_pass_through(ctx, blobs):
    lib, ref = native.lib(), ctypes.byref
    st = native.current_stream_ptr(torch.device(DEV))
    g = torch.Generator().manual_seed(13)
    bins = (ctypes.c_int32 * (2 * L))(*BINS)
    H, D, bs = 2, 64, 16
    nb = _nblocks(bs)
    slots = _mapping("blocks", NTOK, nb, bs, g).to(DEV)

    def encode_refused(struct_, H, D, what):
        stride = native.r16(native.blob_bound(L, CS, H, D))
        arena = torch.full((3 * stride,), 0x5A, dtype=torch.uint8, device=DEV)
        sizes = torch.full((3,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
        rc = lib.lmc_encode_chunks_fixed_split(ctx.handle, ref(struct_), 0, NTOK, CS, bins, arena.data_ptr(), stride,
                                               sizes.data_ptr(), None, st)
        torch.cuda.synchronize()
        assert rc == INVALID, what
        assert bool((arena == 0x5A).all()) and bool((sizes == 0x5A5A5A5A).all()), what

    wide = _split_caches(16, 128, 16, BF16, g)  # H * D = 2048
    encode_refused(native.KVLayout.paged(wide, _mapping("blocks", NTOK, _nblocks(16), 16, g).to(DEV), 16, "NHDB").struct, 16, 128,
                   "more than 1024 channels")
    fp8 = torch.float8_e4m3fn
    encode_refused(native.KVLayout.paged(_split_caches(H, D, bs, fp8, g, nblocks=nb), slots, bs, "NHDB").struct, H, D, "fp8 split source")
    fp8_rows = torch.zeros((L, 2, NTOK, H, D), dtype=torch.uint8, device=DEV).view(fp8)
    encode_refused(native.KVLayout.from_chunk(fp8_rows, "vllm").struct, H, D, "fp8 rows")
    caches = _split_caches(H, D, bs, BF16, g, nblocks=nb)
    before = [c.clone() for c in caches]
    ok = native.KVLayout.paged(caches, slots, bs, "NHDB")
    over = native.KvLayoutStruct.from_buffer_copy(ok.struct)
    over.stride_head = 0xfffffff0 // 2 - D * bs + 1  # ((H-1)*stride_head + D*bs)*E <= 0xfffffff0, H = 2: the first value behind
    neg = native.KvLayoutStruct.from_buffer_copy(ok.struct)
    neg.stride_head = -ok.struct.stride_head
    encode_refused(over, H, D, "head stride past the 32-bit range")
    encode_refused(neg, H, D, "negative head stride")

    # decode
    b = blobs(H, D)
    blobs_before = b.arena.clone()
    ends = (ctypes.c_int32 * 1)(L)

    def decode_rc(struct_, post=None):
        return lib.lmc_decode_chunks_fixed_split_schedule(ctx.handle, b.table.data_ptr(), b.stride, b.n, ref(struct_), 0, CS, 1, ends,
                                                          None, None if post is None else ref(post), None, st)

    d_over = native.KvLayoutStruct.from_buffer_copy(ok.struct)
    d_over.stride_head = (0xfffffff0 - 112) // 2 - D * bs + 1  # decode_dst_ok: ... * E + 7 * 16 <= 0xfffffff0
    assert decode_rc(d_over) == INVALID and decode_rc(neg) == INVALID
    fp8_caches = _split_caches(H, D, bs, fp8, g, nblocks=nb)
    fp8_before = [c.clone() for c in fp8_caches]
    assert decode_rc(native.KVLayout.paged(fp8_caches, slots, bs, "NHDB").struct) == INVALID
    assert decode_rc(native.KVLayout.from_chunk(fp8_rows, "vllm").struct) == INVALID
    rope = RopeShift.from_base(10000.0, D, 128, DEV, is_neox=True, delta=3)
    post = native.RangePost(cos_sin=rope.cos_sin, rot_dim=rope.rot_dim, is_neox=True, delta=3).struct(0, NTOK)
    assert decode_rc(ok.struct, post) == INVALID, "a rotation of a split destination"
    torch.cuda.synchronize()
    assert torch.equal(b.arena, blobs_before) and int(fp8_rows.view(torch.uint8).max()) == 0
    for c, k in zip(caches + fp8_caches, before + fp8_before):
        assert torch.equal(_ibits(c), _ibits(k))
    assert ctx.status(clear=True) == 0
    assert decode_rc(ok.struct) == 0  # the same call without the post-op is taken
    torch.cuda.synchronize()
    assert ctx.status(clear=True) == 0

    # row layouts through the two new calls: exactly the row calls' bytes
    rows = native.KVLayout.from_chunk(b.x.to(DEV), "vllm")
    assert _encode(ctx, ctx.encode_chunks_fixed_split, rows, NTOK, CS)[:2] == (b.sizes, b.bytes)
    seed = _random((L, 2, NTOK, H, D), FP16, g).to(DEV)
    out_a, out_b = seed.clone(), seed.clone()
    assert _decode(ctx, b, native.KVLayout.from_chunk(out_a, "vllm")) == 0
    ctx.decode_chunks_fixed_schedule(b.table.data_ptr(), b.stride, b.n, native.KVLayout.from_chunk(out_b, "vllm"), 0, CS, [L], None)
    torch.cuda.synchronize()
    assert ctx.status(clear=True) == 0
    assert torch.equal(_ibits(out_a), _ibits(out_b)) and torch.equal(_ibits(out_a), b.chunk_bits(FP16))


# ------------------------------------------------------------------ 5. damage
def test_damage_is_flagged_only_the_calls_slots_change_and_the_intact_blob_decodes(ctx, blobs):
    """A byte of the SECOND chunk's blob flipped in a stream, in the scales, in the header: the miss is flagged, and
    whatever was stored by then went to slots of the call's tokens.  Only blob bytes are damaged -- everything an address
    comes from is validated by the kernel before it is used, which is what the statuses show."""
    H, D, bs, dt = 2, 64, 16, BF16
    b = blobs(H, D)
    g = torch.Generator().manual_seed(61)
    blob = b.bytes[1]
    h = fm.header(blob)
    span = fm.stream_spans(blob)[3]
    places = [((span[0] + span[1]) // 2, BAD_STREAM), (int(h[fm.W_OFF_SCALES]) + 3, BAD_SCALES), (4 * fm.W_MODEL, BAD_HEADER),
              (int(h[fm.W_OFF_GDIR]) + 8 * 2 + 4, BAD_HEADER)]
    for kind in ("blocks", "offset5"):
        for where, flag in places:
            caches, expect, split, slots = _case(b, dt, bs, kind, g)
            before = [c.clone() for c in caches]
            damaged = b.arena.clone()
            damaged[b.stride + where] ^= 0x10
            table = torch.tensor([damaged.data_ptr() + i * b.stride for i in range(b.n)], dtype=torch.int64).to(DEV)
            status = _decode(ctx, b, split, table=table)
            assert status & flag and (flag != BAD_STREAM or status == BAD_STREAM), (kind, where, status)
            # outside the slots of the call's tokens: with the old bits put back INTO those slots the caches are equal
            blk, off = slots // bs, slots % bs
            for c, o in zip(caches, before):
                kc, vc = _views(c)
                ko, vo = _views(o)
                _ibits(kc)[blk, :, :, off, :] = _ibits(ko)[blk, :, :, off, :]
                _ibits(vc)[blk, :, :, off] = _ibits(vo)[blk, :, :, off]
                assert torch.equal(_ibits(c), _ibits(o)), (kind, where)
            assert _decode(ctx, b, split) == 0  # the intact blobs, into the same cache
            _same(caches, expect, f"intact after {where}")


# ------------------------------------------------------------------ 6. the engine on the fixed-width tier
def _engine(serde):
    cfg = LMCacheEngineConfig.from_legacy(chunk_size=CS, backend="cuda", local_serde=serde)
    return LMCacheEngine(cfg, dumb_metadata("vllm", "Llama-3-8B"))


def _count_copy_kv(monkeypatch):
    """Counts the calls of copy_kv of the device's context (the one the engine, the codec and the backends share)."""
    calls = []
    ctx = native.get_context(0)
    real = ctx.copy_kv

    def counted(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(ctx, "copy_kv", counted)
    return calls


def test_engine_direct_store_and_retrieve_copy_nothing_and_equal_the_staged_paths(monkeypatch):
    H, D, bs = 2, 128, 16
    nb = _nblocks(bs)
    g = torch.Generator().manual_seed(71)
    tokens = generate_tokens(NTOK, DEV)
    x = _finite((L, 2, NTOK, H, D), BF16, g)
    src = _split_caches(H, D, bs, BF16, g, nblocks=nb)
    slots = _mapping("offset5", NTOK, nb, bs, g).to(DEV)
    _torch_scatter(src, _ibits(x.to(DEV)), slots, bs)
    rope = RopeShift.from_base(10000.0, D, 128, DEV, is_neox=True, delta=17)
    direct, staged, coded = _engine("cachegen-fixed"), _engine("cachegen-fixed"), _engine("cachegen")
    try:
        assert direct.engine_.model == "fixed" and coded.engine_.model == "rans"
        calls = _count_copy_kv(monkeypatch)
        direct.store_paged(tokens, src, slots, bs, "NHDB", direct=True)
        assert len(calls) == 0, "store_paged(direct=True) on the fixed-width tier gathers nothing"
        staged.store_paged(tokens, src, slots, bs, "NHDB")
        assert len(calls) >= 1
        monkeypatch.undo()
        coded.store_paged(tokens, src, slots, bs, "NHDB")
        keys = [direct._make_key(h, "vllm") for h in direct._prefix_hashes_of(tokens)]
        assert len(keys) == 3 and direct.engine_.contains_prefix(keys) == staged.engine_.contains_prefix(keys) == 3
        for k in keys:
            assert torch.equal(direct.engine_.dict[k].blob, staged.engine_.dict[k].blob), k

        def fresh(kind):
            a = _split_caches(H, D, bs, BF16, g, nblocks=nb)
            return a, [c.clone() for c in a], [c.clone() for c in a], _mapping(kind, NTOK, nb, bs, g).to(DEV)

        def same(p, q, what):
            torch.cuda.synchronize()
            for l in range(L):
                assert torch.equal(_ibits(p[l]), _ibits(q[l])), (l, what)

        for kind in ("blocks", "random"):
            a, s, c, slots2 = fresh(kind)
            calls = _count_copy_kv(monkeypatch)
            ma = direct.retrieve_into_paged(tokens, a, slots2, bs, "NHDB", direct=True)
            assert len(calls) == 0, "retrieve_into_paged(direct=True) on the fixed-width tier scatters nothing"
            monkeypatch.undo()
            ms = direct.retrieve_into_paged(tokens, s, slots2, bs, "NHDB")
            mc = coded.retrieve_into_paged(tokens, c, slots2, bs, "NHDB")
            torch.cuda.synchronize()
            assert bool(ma.all()) and torch.equal(ma, ms) and torch.equal(ma, mc)
            for l in range(L):
                assert torch.equal(_ibits(a[l]), _ibits(s[l])), (kind, l, "direct vs staged")
                assert torch.equal(_ibits(a[l]), _ibits(c[l])), (kind, l, "fixed-width vs coded tier")
            # layer by layer: one event per layer, nothing scattered
            a2, s2, _, _ = fresh(kind)
            calls = _count_copy_kv(monkeypatch)
            r = direct.retrieve_into_paged_layerwise(tokens, a2, slots2, bs, "NHDB", direct=True, layers_per_launch=1)
            assert [end for end, _ in r.layer_events] == [1, 2]
            for l in range(L):
                r.wait_layer(l)
            r.finish()
            assert len(calls) == 0
            monkeypatch.undo()
            assert bool(r.ret_mask.all())
            direct.retrieve_into_paged(tokens, s2, slots2, bs, "NHDB")
            same(a2, s2, (kind, "layer-wise direct vs staged"))
        # a mask that cuts into the second chunk: the first-chunk trim, direct
        mask = torch.ones(NTOK, dtype=torch.bool, device=DEV)
        mask[:37] = False
        a, s, _, slots2 = fresh("offset5")
        ma = direct.retrieve_into_paged(tokens, a, slots2, bs, "NHDB", mask=mask, direct=True)
        ms = direct.retrieve_into_paged(tokens, s, slots2, bs, "NHDB", mask=mask)
        torch.cuda.synchronize()
        assert int(ma.sum()) == NTOK - 37 and torch.equal(ma, ms)
        for l in range(L):
            assert torch.equal(_ibits(a[l]), _ibits(s[l])), (l, "trim")
        # with a rope, direct=True still succeeds: the staged result
        for lw in (False, True):
            a, s, _, slots2 = fresh("blocks")
            if lw:
                r = direct.retrieve_into_paged_layerwise(tokens, a, slots2, bs, "NHDB", rope=rope, direct=True, layers_per_launch=1)
                r.finish()
                ma = r.ret_mask
            else:
                ma = direct.retrieve_into_paged(tokens, a, slots2, bs, "NHDB", rope=rope, direct=True)
            ms = direct.retrieve_into_paged(tokens, s, slots2, bs, "NHDB", rope=rope)
            torch.cuda.synchronize()
            assert bool(ma.all()) and torch.equal(ma, ms)
            for l in range(L):
                assert torch.equal(_ibits(a[l]), _ibits(s[l])), (l, lw, "rope")
        assert native.get_context(0).status(clear=True) == 0
    finally:
        monkeypatch.undo()
        torch.cuda.synchronize()
        for e in (direct, staged, coded):
            e.close()
