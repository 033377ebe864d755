"""A window of heads out of every blob (lmc_decode_chunks_heads_schedule, lmc_decode_chunks_fixed_heads_schedule): KV stored
under one tensor-parallel degree decoded into a destination that has a head count of its own.

Nothing here has a tolerance.  The expected value is always the path that existed before: the whole blob decoded into an
[L, 2, T, H_src, D] chunk by lmc_decode_chunks_schedule / lmc_decode_chunks_fixed_schedule, sliced along the heads with
torch and placed by torch indexing into a clone of the destination.  The destination is prefilled with random bits and
compared WHOLE, on integer views: one stray byte outside the window's heads or the call's tokens fails.

L = 2, bins [32, 16, 16, 32] (a wide and a narrow plane on each side), both coder models.  70 tokens in chunks of 32: the
eight-token block path, a ragged last chunk of 6, the counts model; 33 tokens: a last chunk of one token, which is CDF16.
The geometries put every edge of the lane mask somewhere: a head that is two groups (8 x 128), one group (4 x 64), half a
group (6 x 32: windows that enter and leave a group in its middle), and heads that straddle groups with a last group that
is half idle (5 x 96, C = 480)."""
import ctypes

import pytest
import torch

from lmcache_amd import native
from tests.test_gpu_fixed_split import _encode, _finite
from tests.test_gpu_paged_split import DEV, L, _ibits, _mapping, _nblocks, _random, _views

pytestmark = pytest.mark.gpu

CS, BS = 32, 16
BINS = [32, 16, 16, 32]
BF16, FP16, E4M3 = torch.bfloat16, torch.float16, torch.float8_e4m3fn
NAMES = {BF16: "bf16", FP16: "fp16", E4M3: "e4m3"}
INVALID = -1
BAD_HEADER, BAD_STREAM, BAD_SCALES = 2, 4, 16
MODELS = ["coded", "fixed"]

# (H_src, D) -> windows (src_head_begin, nheads, H of the destination, dst_head_begin)
WINDOWS = {
    (8, 128): [(0, 4, 4, 0), (4, 4, 4, 0), (2, 1, 4, 3)],      # the halves; one head of 8 to head 3 of 4
    (4, 64): [(1, 2, 2, 0), (3, 1, 1, 0), (0, 2, 3, 1)],        # a head is a group
    (6, 32): [(3, 1, 1, 0), (2, 1, 2, 1), (1, 4, 4, 0)],        # upper / lower half of a group; heads 1..4: in and out mid-group
    (5, 96): [(1, 3, 3, 0), (4, 1, 1, 0)],                      # heads straddle groups; head 4 ends in the half-idle last group
}
KINDS = ["chunk", "NBHD", "NHBD", "NHDB"]
CASES = [(geom, w) for geom, ws in WINDOWS.items() for w in ws]
IDS = ["H%d_D%d-h%d+%d_to_%dof%d" % (g[0], g[1], w[0], w[1], w[3], w[2]) for g, w in CASES]


@pytest.fixture(scope="module")
def ctx():
    native.build()
    return native.get_context(0)


class _Blobs:
    """ntok tokens of finite random bf16 KV of geometry (H, D), encoded once in chunks of CS in `model`: the blobs on the
    device, their pointer table, and -- per destination dtype and dst_tok0 -- the existing full decode of them."""

    def __init__(self, ctx, model, H, D, ntok, seed=0):
        g = torch.Generator().manual_seed(1000 * seed + 7 * H + D + ntok)
        self.model, self.H, self.D, self.ntok, self.ctx = model, H, D, ntok, ctx
        x = _finite((L, 2, ntok, H, D), BF16, g)
        rows = native.KVLayout.from_chunk(x.to(DEV), "vllm")
        enc = ctx.encode_chunks if model == "coded" else ctx.encode_chunks_fixed
        self.sizes, self.bytes, self.arena, self.stride = _encode(ctx, enc, rows, ntok, CS, BINS)
        self.n = len(self.sizes)
        self.table = torch.tensor([self.arena.data_ptr() + i * self.stride for i in range(self.n)], dtype=torch.int64).to(DEV)
        self._full = {}

    def full(self, dt, tok0=0):
        """Integer view [L, 2, ntok + tok0, H, D] on the device: the whole blobs decoded to dt by the schedule that has
        always done it, the first -tok0 tokens dropped by the decoder's own trim."""
        if (dt, tok0) not in self._full:
            chunk = torch.zeros((L, 2, self.ntok + tok0, self.H, self.D), dtype=dt, device=DEV)
            dec = self.ctx.decode_chunks_schedule if self.model == "coded" else self.ctx.decode_chunks_fixed_schedule
            dec(self.table.data_ptr(), self.stride, self.n, native.KVLayout.from_chunk(chunk, "vllm"), tok0, CS, [L], None)
            torch.cuda.synchronize()
            assert self.ctx.status(clear=True) == 0
            self._full[(dt, tok0)] = _ibits(chunk)
        return self._full[(dt, tok0)]


@pytest.fixture(scope="module")
def blobs(ctx):
    made = {}

    def get(model, H, D, ntok=70, seed=0):
        key = (model, H, D, ntok, seed)
        if key not in made:
            made[key] = _Blobs(ctx, model, H, D, ntok, seed)
        return made[key]
    return get


def _window_decode(ctx, b, dst, win, tok0=0, ends=None, events=None, table=None, src_heads=None, n=None):
    fn = ctx.decode_chunks_heads_schedule if b.model == "coded" else ctx.decode_chunks_fixed_heads_schedule
    fn((b.table if table is None else table).data_ptr(), b.stride, b.n if n is None else n, dst, tok0, CS, ends or [L], events,
       native.HeadWindow(b.H if src_heads is None else src_heads, win[0], win[1], win[3]))
    torch.cuda.synchronize()
    return ctx.status(clear=True)


class _Dst:
    """A destination of `kind` with Hd heads for T tokens, prefilled with random bits; put(bits, h0) writes integer
    [L, 2, T, n, D] into heads [h0, h0 + n) of the EXPECTED copy by torch indexing; same() compares every byte."""

    def __init__(self, kind, Hd, D, T, dt, g, mapping="random"):
        self.kind, self.T = kind, T
        nb = _nblocks(BS)
        if kind == "chunk":
            self.t = [_random((L, 2, T, Hd, D), dt, g).to(DEV)]
            self.layout = native.KVLayout.from_chunk(self.t[0], "vllm")
        else:
            shape = {"NBHD": (2, nb, BS, Hd, D), "NHBD": (2, nb, Hd, BS, D), "NHDB": (2, nb, Hd, D, BS)}[kind]
            self.t = [_random(shape, dt, g).to(DEV) for _ in range(L)]
            self.slots = _mapping(mapping, T, nb, BS, g).to(DEV)
            self.layout = native.KVLayout.paged(self.t, self.slots, BS, kind)
        self.want = [c.clone() for c in self.t]

    def put(self, bits, h0):
        n = bits.shape[3]
        if self.kind == "chunk":
            _ibits(self.want[0])[:, :, :, h0:h0 + n] = bits
            return
        blk, off = self.slots // BS, self.slots % BS
        for l, c in enumerate(self.want):
            for kv in range(2):
                v = bits[l, kv]  # [T, n, D]
                if self.kind == "NBHD":
                    _ibits(c)[kv, blk, off, h0:h0 + n] = v
                elif self.kind == "NHBD":
                    _ibits(c)[kv][blk, h0:h0 + n, off] = v
                elif kv == 0:
                    kc = _views(c)[0]  # [nb, H, D / x, bs, x]
                    _ibits(kc)[blk, h0:h0 + n, :, off, :] = v.reshape(v.shape[0], n, -1, kc.shape[-1])
                else:
                    _ibits(c[1])[blk, h0:h0 + n, :, off] = v

    def same(self, what):
        torch.cuda.synchronize()
        for l, (c, w) in enumerate(zip(self.t, self.want)):
            assert torch.equal(_ibits(c), _ibits(w)), f"{what}: tensor {l}"


def _check(ctx, b, kind, win, dt, g, mapping="random", tok0=0, ends=None, events=None):
    s0, n, Hd, d0 = win
    d = _Dst(kind, Hd, b.D, b.ntok + tok0, dt, g, mapping)
    d.put(b.full(dt, tok0)[:, :, :, s0:s0 + n], d0)
    assert _window_decode(ctx, b, d.layout, win, tok0, ends, events) == 0
    d.same(f"{b.model} {kind} {win}")


# ------------------------------------------------------------------ 1. every window, every destination, both models
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("geom,win", CASES, ids=IDS)
def test_a_window_equals_the_full_decode_sliced_and_nothing_else_is_written(ctx, blobs, geom, win, model, kind):
    i = CASES.index((geom, win)) + KINDS.index(kind) + MODELS.index(model)
    dt = (BF16, FP16)[i % 2]  # the dtype walks with the case: every geometry and destination meets both
    mapping = ("blocks", "random", "offset5")[i % 3]  # block-ordered slots (the eight-row blocks, the wide V stores), shuffled, ragged
    g = torch.Generator().manual_seed(17 * i + geom[0])
    _check(ctx, blobs(model, *geom), kind, win, dt, g, mapping)


@pytest.mark.parametrize("kind", ["chunk", "NHDB"])
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("geom", list(WINDOWS), ids=lambda g: "H%d_D%d" % g)
def test_a_last_chunk_of_one_token(ctx, blobs, geom, model, kind):
    """33 tokens: the second chunk has one token (the coded models fall back to CDF16 there; the fixed-width model a
    single partial oct), and only the one-token loop stores it."""
    g = torch.Generator().manual_seed(5 + geom[1])
    b = blobs(model, *geom, ntok=33)
    for win in WINDOWS[geom][-2:]:
        _check(ctx, b, kind, win, BF16, g, "blocks")


@pytest.mark.parametrize("kind,mapping", [("chunk", "random"), ("NBHD", "random"), ("NHDB", "blocks"), ("NHDB", "random")])
@pytest.mark.parametrize("model", MODELS)
def test_first_chunk_trim_and_a_schedule_of_two_ranges_with_events(ctx, blobs, model, kind, mapping):
    """dst_tok0 = -5: the first five tokens are decoded and dropped, every later token moves off the destination's
    multiples of eight.  Then two ranges of layers, each with its event."""
    g = torch.Generator().manual_seed(31)
    b = blobs(model, 6, 32)
    _check(ctx, b, kind, (1, 4, 4, 0), BF16, g, mapping, tok0=-5)
    b = blobs(model, 8, 128)
    _check(ctx, b, kind, (2, 1, 4, 3), FP16, g, mapping, tok0=-5)
    evs = [native.NativeEvent(timing=True) for _ in range(2)]
    _check(ctx, b, kind, (4, 4, 4, 0), BF16, g, mapping, ends=[1, L], events=evs)
    assert all(e.query() for e in evs)


@pytest.mark.parametrize("geom,win", [((8, 128), (2, 1, 4, 3)), ((6, 32), (1, 4, 4, 0)), ((5, 96), (4, 1, 2, 1))],
                         ids=["H8_D128", "H6_D32", "H5_D96"])
def test_an_e4m3_row_destination_of_the_coded_decoder(ctx, blobs, geom, win):
    g = torch.Generator().manual_seed(41)
    _check(ctx, blobs("coded", *geom), "chunk", win, E4M3, g)


# ------------------------------------------------------------------ 2. assembly, the full window
@pytest.mark.parametrize("order", [(0, 1), (1, 0)], ids=["low_first", "high_first"])
@pytest.mark.parametrize("kind", ["chunk", "NHDB"])
@pytest.mark.parametrize("model", MODELS)
def test_two_blob_sets_assemble_one_destination_in_either_order(ctx, blobs, model, kind, order):
    """What a TP = 1 rank does with the blobs of two TP = 2 ranks: two DIFFERENT H = 4 blob sets into heads 0..3 and 4..7
    of one H = 8 destination."""
    g = torch.Generator().manual_seed(51)
    parts = [blobs(model, 4, 64, seed=1), blobs(model, 4, 64, seed=2)]
    assert not torch.equal(parts[0].full(BF16), parts[1].full(BF16))
    d = _Dst(kind, 8, 64, 70, BF16, g, "blocks")
    for k in (0, 1):
        d.put(parts[k].full(BF16), 4 * k)
    for k in order:
        assert _window_decode(ctx, parts[k], d.layout, (0, 4, 8, 4 * k)) == 0
    d.same("assembly")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("model", MODELS)
def test_a_window_that_is_the_whole_blob_is_the_schedule_byte_for_byte(ctx, blobs, model, kind):
    b = blobs(model, 5, 96)
    g = torch.Generator().manual_seed(61)
    d = _Dst(kind, 5, 96, 70, BF16, g)
    for c, w in zip(d.t, d.want):  # `want` takes the schedule that exists, `t` the window call: same sentinel under both
        assert torch.equal(_ibits(c), _ibits(w))
    twin = native.KVLayout.from_chunk(d.want[0], "vllm") if kind == "chunk" else native.KVLayout.paged(d.want, d.slots, BS, kind)
    dec = {"coded": ctx.decode_chunks_schedule, "fixed": ctx.decode_chunks_fixed_split_schedule}[model]
    dec(b.table.data_ptr(), b.stride, b.n, twin, 0, CS, [L], None)
    torch.cuda.synchronize()
    assert ctx.status(clear=True) == 0
    assert _window_decode(ctx, b, d.layout, (0, 5, 5, 0)) == 0
    d.same("full window")


# ------------------------------------------------------------------ 3. damaged blobs: status results on in-bounds blobs
def _damaged(b, chunk, edit):
    """The table of `b` with chunk `chunk` replaced by an edited copy (same size, same slot stride: every read stays inside
    the copy) -> (table, the copy)."""
    raw = bytearray(b.bytes[chunk])
    edit(raw, native.blob_info(bytes(raw)))
    copy = torch.zeros(b.stride, dtype=torch.uint8, device=DEV)
    copy[:len(raw)] = torch.frombuffer(raw, dtype=torch.uint8).to(DEV)
    ptrs = b.table.cpu().tolist()
    ptrs[chunk] = copy.data_ptr()
    return torch.tensor(ptrs, dtype=torch.int64).to(DEV), copy


@pytest.mark.parametrize("model", MODELS)
def test_a_damaged_scale_is_seen_by_a_window_that_does_not_hold_group_0(ctx, blobs, model):
    b = blobs(model, 8, 128)
    win = (4, 4, 4, 0)  # channels 512 .. 1023: groups 8 .. 15
    g = torch.Generator().manual_seed(71)

    def flip(raw, h):  # plane 1 (K of layer 1), token 3 of the chunk's T tokens: one bit of its scale
        raw[h.off_scales + 2 * (1 * h.ntokens + 3)] ^= 0x04
    table, keep = _damaged(b, 1, flip)
    d = _Dst("chunk", 4, 128, 70, BF16, g)
    assert _window_decode(ctx, b, d.layout, win, table=table) == BAD_SCALES
    # ... and the undamaged table decodes clean into the same destination
    d.put(b.full(BF16)[:, :, :, 4:8], 0)
    assert _window_decode(ctx, b, d.layout, win) == 0
    d.same("after the damage")


@pytest.mark.parametrize("model", MODELS)
def test_a_damaged_stream_inside_the_windows_groups_is_seen_and_one_outside_is_not_read(ctx, blobs, model):
    b = blobs(model, 8, 128)
    win = (4, 4, 4, 0)
    G = 16
    g = torch.Generator().manual_seed(73)

    def flip_in(group):
        def edit(raw, h):  # a byte in the middle of stream (plane 3, group): directory entry {beg, end}
            e = h.off_gdir + 8 * (3 * G + group)
            beg, end = int.from_bytes(raw[e:e + 4], "little"), int.from_bytes(raw[e + 4:e + 8], "little")
            raw[h.off_streams + (beg + end) // 2] ^= 0x10
        return edit
    table, keep = _damaged(b, 0, flip_in(9))
    d = _Dst("chunk", 4, 128, 70, BF16, g)
    assert _window_decode(ctx, b, d.layout, win, table=table) & BAD_STREAM
    table, keep = _damaged(b, 0, flip_in(2))  # group 2 is outside the window: its stream is not among those read
    d = _Dst("chunk", 4, 128, 70, BF16, g)
    d.put(b.full(BF16)[:, :, :, 4:8], 0)
    assert _window_decode(ctx, b, d.layout, win, table=table) == 0
    d.same("damage outside the window")


@pytest.mark.parametrize("model", MODELS)
def test_blobs_of_another_head_count_are_a_bad_header(ctx, blobs, model):
    """8 heads of 128 read as 16 heads of 64: the channel count (header word 7) agrees, num_heads and head_size do not."""
    b = blobs(model, 8, 128)
    g = torch.Generator().manual_seed(79)
    d = _Dst("chunk", 8, 64, 70, BF16, g)
    assert _window_decode(ctx, b, d.layout, (0, 8, 8, 0), src_heads=16) == BAD_HEADER
    d.same("nothing is written for a refused blob")
    d = _Dst("chunk", 4, 128, 70, BF16, g)  # ... and 4 heads of 128 where the blobs have 8: word 7 already disagrees
    assert _window_decode(ctx, b, d.layout, (0, 4, 4, 0), src_heads=4) == BAD_HEADER
    d.same("nothing is written for a refused blob")


# ------------------------------------------------------------------ 4. LMC_ERR_INVALID, nothing queued
@pytest.mark.parametrize("model", MODELS)
def test_refusals_return_invalid_and_write_nothing(ctx, blobs, model):
    b = blobs(model, 8, 128)
    g = torch.Generator().manual_seed(83)
    lib = native.lib()
    fn = lib.lmc_decode_chunks_heads_schedule if model == "coded" else lib.lmc_decode_chunks_fixed_heads_schedule
    ends = (ctypes.c_int32 * 1)(L)
    stream = native.current_stream_ptr(torch.device(DEV))

    def rc(layout, win, ends_=ends, nranges=1, table=b.table.data_ptr()):
        w = None if win is None else ctypes.byref(native.HeadWindowStruct(*win))
        return fn(ctx.handle, table, b.stride, b.n, ctypes.byref(layout.struct), 0, CS, nranges, ends_, None, w, None, stream)

    d = _Dst("chunk", 4, 128, 70, BF16, g)
    lay = d.layout
    assert rc(lay, None) == INVALID                      # no window
    for win in [(0, 0, 4, 0), (-3, 0, 4, 0),            # src_heads < 1
                (8, 0, 0, 0), (8, 0, -2, 0),            # nheads < 1
                (8, 5, 4, 0), (8, -1, 2, 0), (8, 8, 1, 0),      # outside [0, src_heads)
                (8, 0, 4, 1), (8, 0, 5, 0), (8, 0, 1, -1), (8, 0, 1, 4),  # outside [0, dst->num_heads)
                (33, 0, 4, 0)]:                         # 33 * 128 channels: above LMC_MAX_CHANNELS
        assert rc(lay, win) == INVALID, win
    small = _Dst("chunk", 2, 4, 70, BF16, g)             # D = 4: 3 heads are 12 channels, no multiple of 8
    assert rc(small.layout, (3, 0, 2, 0)) == INVALID
    small.same("refused")
    # what the twin refuses: a schedule that does not end at num_layers, no table, an fp8 destination of the fixed-width model
    assert rc(lay, (8, 0, 4, 0), (ctypes.c_int32 * 1)(1)) == INVALID
    assert rc(lay, (8, 0, 4, 0), table=None) == INVALID
    if model == "fixed":
        f8 = _Dst("chunk", 4, 128, 70, E4M3, g)
        assert rc(f8.layout, (8, 0, 4, 0)) == INVALID
        f8.same("refused")
    torch.cuda.synchronize()
    assert ctx.status(clear=True) == 0
    d.same("refused")
    assert rc(lay, (8, 0, 4, 0)) == 0                    # the same call with a window that fits goes through
    d.put(b.full(BF16)[:, :, :, 0:4], 0)
    torch.cuda.synchronize()
    assert ctx.status(clear=True) == 0
    d.same("accepted")
