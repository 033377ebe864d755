"""lmc_decode_chunks_fixed_rope_schedule (k_fixed_decode_rope): the rotation of a RoPE shift inside the fixed-width decode.

Reference of the rotated channels, plain numpy over the oracle's symbols and scales: x = float32(q - C) / float32(C) *
float32(scale) in fp32, rotated in float64 with the fp32 table, e = x1 c - x2 s (and x2 c + x1 s), s negated for a negative
delta.  Every rotated key must satisfy |out - e| <= u |e| + 2^-22 (|x1| + |x2|) (+ 2^-25 for fp16), u = 2^-8 bf16 / 2^-11
fp16: one rounding of the output type plus rope_pair's fp32 arithmetic.  Everything else -- V planes, channels at or past
rot_dim, tokens not written, the rest of the destination -- equals, bit for bit, the same blobs decoded without a post.

93 tokens in chunks of 40 (40, 40, 13: a second tile of one oct, a ragged oct), dst_tok0 = -5 (the first-chunk trim);
L = 2 with a 5-bit K plane in layer 0 and a 4-bit one in layer 1."""
import numpy as np
import pytest
import torch

from lmcache_amd import native
from lmcache_amd.rope import RopeShift
from tests import fixed_model as fm

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
L, NTOK, CS, TRIM, BS, ROWS = 2, 93, 40, 5, 16, 128
NW = NTOK - TRIM            # destination tokens written
NB = (NW + BS - 1) // BS + 1  # blocks: more slots than tokens, the permutation leaves some untouched
BINS = [32, 16, 16, 32]     # K of layer 0 / 1, V of layer 0 / 1
BAD_STREAM, BAD_POSITION = 4, 64
BF16, FP16 = torch.bfloat16, torch.float16
# (H, D, rot, neox): partners in two streams | inside one stream | U = 4 | two heads per stream | partial rotary | GPT-J
GEOMS = [(2, 128, 128, True), (2, 64, 64, True), (1, 256, 256, True), (4, 32, 32, True), (2, 128, 64, True), (2, 128, 128, False)]
CASES = [(g, dt) for g in GEOMS for dt in ((BF16, FP16) if g is GEOMS[0] else (BF16,))]
IDS = ["H%d_D%d_rot%d_%s-%s" % (g[0], g[1], g[2], "neox" if g[3] else "gptj", "bf16" if dt == BF16 else "fp16") for g, dt in CASES]


@pytest.fixture(scope="module")
def ctx():
    native.build()
    return native.get_context(0)


_stored = {}


def stored(ctx, oracle, H, D):
    """KV of geometry (H, D) encoded once: (pointer table, largest blob, [blob bytes], arena, stride, x) with x float32
    [L, NTOK, H, D], the dequantised keys in fp32 as the reference states them."""
    if (H, D) not in _stored:
        g = torch.Generator().manual_seed(1000 * H + D)
        kv = torch.rand((L, 2, NTOK, H, D), generator=g).to(BF16)
        stride = native.r16(native.blob_bound(L, CS, H, D))
        n = (NTOK + CS - 1) // CS
        arena = torch.zeros(n * stride, dtype=torch.uint8, device=DEV)
        sizes = torch.zeros(n, dtype=torch.int32, device=DEV)
        ctx.encode_chunks_fixed(native.KVLayout.from_chunk(kv.to(DEV), "vllm"), 0, NTOK, CS, BINS, arena.data_ptr(), stride, sizes.data_ptr())
        torch.cuda.synchronize()
        assert ctx.status(clear=True) == 0
        sz, host = sizes.cpu().tolist(), arena.cpu().numpy()
        blobs = [host[i * stride:i * stride + sz[i]].tobytes() for i in range(n)]
        table = torch.tensor([arena.data_ptr() + i * stride for i in range(n)], dtype=torch.int64).to(DEV)
        _stored[(H, D)] = (table, max(sz), blobs, arena, stride, exact_keys(oracle, kv, BINS[:L]))
    return _stored[(H, D)]


def exact_keys(oracle, kv, kbins):
    """kv bf16 / fp16 [L, 2, T, H, D] (CPU) -> float32 [L, T, H, D]: x = float32(q - C) / float32(C) * float32(scale) of
    the K planes, from the oracle's symbols and scales."""
    nl, _, T, H, D = kv.shape
    bits, code = oracle.torch_to_bits(kv.reshape(nl, 2, T, H * D))
    bins = np.array(list(kbins) + [16] * nl, np.int32)  # (the V planes' bins do not matter here)
    sym, scale = oracle.quantize(bits, code, bins)
    sc = oracle.bits_to_torch(scale[:nl], code).float().numpy()  # [L, T]
    C = (bins[:nl] // 2 - 1).astype(np.float32)[:, None, None]
    x = (sym[:nl].astype(np.float32) - C) / C * sc[:, :, None]
    assert x.dtype == np.float32
    return x.reshape(nl, T, H, D)


def rotated(x, table, deltas, rot, neox):
    """x float32 [L, n, H, D], deltas int [n] -> (e float64 [L, n, H, rot], the bound's |x1| + |x2| in the same shape)."""
    half = rot // 2
    rows = np.abs(deltas)
    c = table[rows, :half].astype(np.float64)[None, :, None, :]
    s = (table[rows, half:].astype(np.float64) * np.sign(deltas)[:, None])[None, :, None, :]
    xr = x[..., :rot].astype(np.float64)
    i1, i2 = (np.arange(half), np.arange(half) + half) if neox else (2 * np.arange(half), 2 * np.arange(half) + 1)
    x1, x2 = xr[..., i1], xr[..., i2]
    e, mag = np.empty_like(xr), np.empty_like(xr)
    e[..., i1], e[..., i2] = x1 * c - x2 * s, x2 * c + x1 * s
    mag[..., i1] = mag[..., i2] = np.abs(x1) + np.abs(x2)
    return e, mag


def bound(e, mag, dt):
    u = 2.0 ** -8 if dt == BF16 else 2.0 ** -11
    return u * np.abs(e) + 2.0 ** -22 * mag + (2.0 ** -25 if dt == FP16 else 0.0)


class Dst:
    """A destination of NW tokens with random bits everywhere: rows [L, 2, NW + 2, H, D], or paged caches with a slot
    permutation.  tokens() gathers [L, 2, NW, H, D]; put_keys() writes the first `rot` channels of the K tokens back."""

    def __init__(self, kind, H, D, dt, g, slots):
        self.kind, self.H, self.D, self.slots = kind, H, D, slots
        shape = {"rows": (L, 2, NW + 2, H, D), "NHBD": (L, 2, NB, H, BS, D), "NHDB": (L, 2, NB, H, D, BS)}[kind]
        self.base = torch.randint(-2 ** 15, 2 ** 15, shape, generator=g, dtype=torch.int16).view(dt).to(DEV)

    @property
    def caches(self):
        return list(self.base.unbind(0))

    def clone(self):
        d = Dst.__new__(Dst)
        d.__dict__.update(self.__dict__)
        d.base = self.base.clone()
        return d

    def layout(self):
        if self.kind == "rows":
            return native.KVLayout.from_chunk(self.base, "vllm")
        return native.KVLayout.paged(self.caches, self.slots, BS, self.kind)

    def _plane(self, c, kv):
        """-> (a view indexed [token...] of plane kv of layer cache c, the index that selects the NW tokens as [NW, H, D...])"""
        b, w = self.slots // BS, self.slots % BS
        if self.kind == "rows":
            return c[kv], (slice(0, NW),)
        if self.kind == "NHBD":
            return c[kv], (b, slice(None), w)
        if kv == 1:
            return c[1], (b, slice(None), slice(None), w)
        return c[0].view(NB, self.H, self.D // 8, BS, 8), (b, slice(None), slice(None), w)

    def tokens(self):
        out = []
        for c in self.caches:
            pl = []
            for kv in (0, 1):
                v, ix = self._plane(c, kv)
                pl.append(v[ix].reshape(NW, self.H, self.D))
            out.append(torch.stack(pl))
        return torch.stack(out)

    def put_keys(self, keys, rot):
        for c, k in zip(self.caches, keys):
            v, ix = self._plane(c, 0)
            if self.kind == "NHDB":
                v[ix[0], :, :rot // 8, ix[3]] = k[..., :rot].reshape(NW, self.H, rot // 8, 8)
            else:
                v[ix + (slice(None),) * (self.kind == "rows") + (slice(0, rot),)] = k[..., :rot]


def run(ctx, st, dst, post):
    """Decode st's blobs into dst with `post` (None: the plain schedule) -> the context's status word."""
    table, room = st[0], st[1]
    lay = dst.layout()
    if post is None:
        ctx.decode_chunks_fixed_split_schedule(table.data_ptr(), room, len(st[2]), lay, -TRIM, CS, [L], None)
    else:
        p = native.RangePost(post.cos_sin, post.rot_dim, post.is_neox, delta=0 if isinstance(post.delta, torch.Tensor) else post.delta,
                             deltas=post.delta if isinstance(post.delta, torch.Tensor) else None,
                             scatter_dst=lay if dst.kind == "NHDB" else None)
        ctx.decode_chunks_fixed_rope_schedule(table.data_ptr(), room, len(st[2]), lay, -TRIM, CS, [L], None, p.struct(0, NW))
    torch.cuda.synchronize()
    return ctx.status(clear=True)


def _bits(t):
    return t.view(torch.int16)


@pytest.mark.parametrize("kind", ["rows", "NHBD", "NHDB"])
@pytest.mark.parametrize("delta", ["+37", "-37", "per_token"])
@pytest.mark.parametrize("geom,dt", CASES, ids=IDS)
def test_rotated_keys_meet_the_one_rounding_bound_and_the_rest_is_the_plain_decode(ctx, oracle, geom, dt, delta, kind):
    H, D, rot, neox = geom
    st = stored(ctx, oracle, H, D)
    g = torch.Generator().manual_seed(GEOMS.index(geom) * 100 + len(delta) + len(kind))
    deltas = torch.randint(-(ROWS - 1), ROWS, (NW,), generator=g, dtype=torch.int32)
    rope = RopeShift.from_base(10000.0, rot, ROWS, DEV, is_neox=neox,
                               delta=deltas.to(DEV) if delta == "per_token" else int(delta))
    if delta != "per_token":
        deltas = torch.full((NW,), int(delta), dtype=torch.int32)
    start = Dst(kind, H, D, dt, g, torch.randperm(NB * BS, generator=g)[:NW].to(DEV))
    plain, fused = start.clone(), start.clone()
    assert run(ctx, st, plain, None) == 0 and run(ctx, st, fused, rope) == 0
    a, b = plain.tokens(), fused.tokens()
    assert not torch.equal(_bits(a), _bits(start.tokens())), "nothing was decoded"
    assert torch.equal(_bits(a[:, 1]), _bits(b[:, 1])), "V planes"
    assert torch.equal(_bits(a[:, 0, ..., rot:]), _bits(b[:, 0, ..., rot:])), "channels at or past rot_dim"
    e, mag = rotated(st[5][:, TRIM:], rope.cos_sin.cpu().numpy(), deltas.numpy().astype(np.int64), rot, neox)
    err = np.abs(b[:, 0, ..., :rot].double().cpu().numpy() - e)
    lim = bound(e, mag, dt)
    print(f"worst |out - e| / bound = {(err[lim > 0] / lim[lim > 0]).max():.3f}")
    assert (err <= lim).all()
    fused.put_keys(a[:, 0], rot)  # the rotated channels aside, the whole destination: trim, ragged tail, foreign slots
    for x, y in zip(fused.caches, plain.caches):
        assert torch.equal(_bits(x), _bits(y)), "bytes outside the rotated keys"


def test_a_delta_outside_the_table_leaves_that_token_unrotated(ctx, oracle):
    H, D, rot, neox = GEOMS[0]
    st = stored(ctx, oracle, H, D)
    g = torch.Generator().manual_seed(5)
    deltas = torch.randint(-(ROWS - 1), ROWS, (NW,), generator=g, dtype=torch.int32)
    deltas[41] = ROWS + 72
    rope = RopeShift.from_base(10000.0, rot, ROWS, DEV, is_neox=neox, delta=deltas.to(DEV))
    start = Dst("NHDB", H, D, BF16, g, torch.randperm(NB * BS, generator=g)[:NW].to(DEV))
    plain, fused = start.clone(), start.clone()
    assert run(ctx, st, plain, None) == 0
    assert run(ctx, st, fused, rope) == BAD_POSITION
    a, b = plain.tokens(), fused.tokens()
    assert torch.equal(_bits(a[:, :, 41]), _bits(b[:, :, 41]))
    assert not torch.equal(_bits(a[:, 0, 40]), _bits(b[:, 0, 40]))


def test_a_flipped_byte_in_a_units_second_stream_is_a_bad_stream(ctx, oracle):
    H, D, rot, neox = GEOMS[0]
    st = stored(ctx, oracle, H, D)
    table, room, blobs, arena, stride = st[:5]
    at = fm.stream_spans(blobs[1])[0 * (H * D // 64) + 1][0] + 7  # chunk 1, K plane of layer 0, stream 1: head 0's second
    rope = RopeShift.from_base(10000.0, rot, ROWS, DEV, is_neox=neox, delta=3)
    g = torch.Generator().manual_seed(6)
    dst = Dst("rows", H, D, BF16, g, torch.arange(NW).to(DEV))
    arena[stride + at] ^= 0x10
    try:
        assert run(ctx, st, dst, rope) == BAD_STREAM
    finally:
        arena[stride + at] ^= 0x10
