"""LMC_MODEL_FIXED on the GPU: lmc_encode_chunks_fixed / lmc_decode_chunks_fixed_schedule against the numpy reference of
the bytes (tests/fixed_model.py), the CPU oracle's quantise / dequantise, and the entropy-coded path for the same input
(the two models must decode to the same bits); refusals, damaged blobs, and the engine on local_serde="cachegen-fixed"
held against an engine on "cachegen"."""
import ctypes

import numpy as np
import pytest
import torch

from lmcache_amd import native
from lmcache_amd.cache_engine import LMCacheEngine
from lmcache_amd.config import LMCacheEngineConfig
from lmcache_amd.rope import RopeShift
from tests import fixed_model as fm
from tests.test_gpu_engine import dumb_metadata, generate_tokens
from tests.test_gpu_rope_shift import _ibits, _mapping, _random_bits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BAD_HEADER, BAD_STREAM, BAD_SCALES = 2, 4, 16
BINS = [32, 18, 17, 16, 4]


@pytest.fixture(scope="module")
def ctx():
    native.lib()
    return native.get_context(0)


def bits_np(t):
    return t.contiguous().cpu().view(torch.int16).numpy().view(np.uint16)


def make_kv(L, T, H, D, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(L, 2, T, H, D, generator=g) * torch.exp(1.5 * torch.randn(H * D, generator=g)).reshape(H, D)
    return x.to(dtype)


def plane_bins(L, shift=0):
    return [BINS[(p + shift) % len(BINS)] for p in range(2 * L)]


def encode(ctx, layout, t0, t1, cs, bins, fixed=True, poison=0):
    """-> (blob bytes per chunk, arena, stride)."""
    L, H, D = layout.L, layout.H, layout.D
    stride = native.r16(native.blob_bound(L, cs, H, D))
    n = (t1 - t0 + cs - 1) // cs
    arena = torch.full((n * stride,), poison, dtype=torch.uint8, device=DEV)
    sizes = torch.zeros(n, dtype=torch.int32, device=DEV)
    call = ctx.encode_chunks_fixed if fixed else ctx.encode_chunks
    call(layout, t0, t1, cs, bins, arena.data_ptr(), stride, sizes.data_ptr())
    torch.cuda.synchronize()
    assert ctx.status(clear=True) == 0
    sz = sizes.cpu().tolist()
    host = arena.cpu().numpy()
    return [host[i * stride:i * stride + sz[i]].tobytes() for i in range(n)], arena, stride


def decode(ctx, blobs, dst, dst_tok0, cs, ends=None, events=None):
    """Fixed-width decode of device blobs (uint8 tensors) -> the status word."""
    table = torch.tensor([b.data_ptr() for b in blobs], dtype=torch.int64, device=DEV)
    ctx.decode_chunks_fixed_schedule(table.data_ptr(), max(b.numel() for b in blobs), len(blobs), dst, dst_tok0, cs,
                                     ends or [dst.L], events)
    torch.cuda.synchronize()
    return ctx.status(clear=True)


def dev_blobs(blobs):
    return [torch.from_numpy(np.frombuffer(b, np.uint8).copy()).to(DEV) for b in blobs]


def reference(oracle, kv, H, D, bins):
    L, _, T = kv.shape[:3]
    b, code = oracle.torch_to_bits(kv.reshape(L, 2, T, H * D))
    return fm.encode_blob(oracle, b, code, H, D, np.array(bins, np.int32)), b, code


SHAPES = [(1, 1, 1, 8), (2, 20, 3, 40), (2, 100, 8, 128), (1, 256, 8, 128), (1, 9, 32, 128), (3, 300, 2, 64),
          (1, 70, 16, 128)]  # (the last: 2048 channels, two waves share a row oct -- the path between 1024 and 4096)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "L%dT%dH%dD%d" % s)
def test_blob_and_decode_bit_exact(ctx, oracle, shape, dtype):
    L, T, H, D = shape
    kv = make_kv(L, T, H, D, dtype, seed=1000 * L + T)
    for shift in (0, 2):  # every plane sees a wide and a narrow bin count
        bins = plane_bins(L, shift)
        src = native.KVLayout.from_chunk(kv.to(DEV), "vllm")
        blobs, arena, stride = encode(ctx, src, 0, T, T, bins, poison=0xa5)
        ref, b, code = reference(oracle, kv, H, D, bins)
        assert len(blobs[0]) == len(ref) == native.fixed_blob_bytes(L, T, H, D, bins)
        assert blobs[0] == ref
        assert native.blob_info(blobs[0]).model == 2
        sym, scale = oracle.quantize(b, code, np.array(bins, np.int32))
        _, coded_arena, cstride = encode(ctx, src, 0, T, T, bins, fixed=False)
        for odt, ocode in ((torch.bfloat16, oracle.BF16), (torch.float16, oracle.FP16)):
            out = torch.zeros(L, 2, T, H, D, dtype=odt, device=DEV)
            assert decode(ctx, [arena[:len(ref)]], native.KVLayout.from_chunk(out, "vllm"), 0, T) == 0
            got = bits_np(out).reshape(L, 2, T, H * D)
            assert np.array_equal(got, oracle.dequantize(sym, scale, code, np.array(bins, np.int32), ocode))
            coded = torch.zeros_like(out)
            ctx.decode_chunks(coded_arena.data_ptr(), cstride, 1, native.KVLayout.from_chunk(coded, "vllm"), 0, T)
            torch.cuda.synchronize()
            assert ctx.status(clear=True) == 0
            assert torch.equal(_ibits(out), _ibits(coded)), "the two models decode to different bits"
        # a huggingface destination: the heads of a token lie T rows apart
        if D % 8 == 0 and H > 1:
            out = torch.zeros(L, 2, H, T, D, dtype=dtype, device=DEV)
            assert decode(ctx, [arena[:len(ref)]], native.KVLayout.from_chunk(out, "huggingface"), 0, T) == 0
            want = oracle.dequantize(sym, scale, code, np.array(bins, np.int32), code).reshape(L, 2, T, H, D)
            assert np.array_equal(bits_np(out), want.transpose(0, 1, 3, 2, 4))


@pytest.mark.parametrize("trim", [0, 5])
def test_a_job_of_three_chunks_with_a_ragged_last_one_and_the_first_chunk_trim(ctx, oracle, trim):
    L, H, D, cs, n = 2, 3, 40, 64, 150
    kv = make_kv(L, n, H, D, torch.bfloat16, seed=7)
    bins = plane_bins(L, 1)
    blobs, arena, stride = encode(ctx, native.KVLayout.from_chunk(kv.to(DEV), "vllm"), 0, n, cs, bins)
    assert [native.blob_info(b).ntokens for b in blobs] == [64, 64, 22]
    for i, b in enumerate(blobs):
        assert b == reference(oracle, kv[:, :, i * cs:(i + 1) * cs].contiguous(), H, D, bins)[0], i
    want = torch.cat([native_bits(oracle, b) for b in blobs], dim=2)
    out = _random_bits((L, 2, n - trim, H, D), torch.bfloat16, torch.Generator().manual_seed(1)).to(DEV)
    views = [arena[i * stride:i * stride + len(b)] for i, b in enumerate(blobs)]
    assert decode(ctx, views, native.KVLayout.from_chunk(out, "vllm"), -trim, cs) == 0
    assert torch.equal(_ibits(out.cpu()), _ibits(want[:, :, trim:]))


def native_bits(oracle, blob):
    h = fm.header(blob)
    out = fm.decode_blob(oracle, blob, oracle.BF16)
    return oracle.bits_to_torch(out, oracle.BF16).reshape(out.shape[0], 2, out.shape[2], int(h[5]), int(h[6]))


def test_edge_rows(ctx, oracle, golden_dir):
    import os
    z = np.load(os.path.join(golden_dir, "quant_edge.npz"))
    x = torch.from_numpy(z["x"].view(np.int16)).view(torch.bfloat16)  # [2, T, 64]
    Lk, T, C = x.shape
    extra = torch.zeros(Lk, 5, C, dtype=torch.float32)
    extra[:, 1, 3] = float("inf")
    extra[:, 2, 5] = float("nan")
    extra[:, 3, :] = 1e-40          # a denormal scale (bf16 keeps fp32's exponent range)
    extra[:, 4, 0::2] = -float("inf")
    x = torch.cat([x, extra.to(torch.bfloat16)], dim=1)
    T = x.shape[1]
    kv = torch.stack([x, x], dim=1).reshape(Lk, 2, T, 1, C)
    for bins in ([int(v) for v in z["bins"].tolist()] * 2, [32, 17, 18, 4][:2 * Lk] if Lk == 2 else [18, 17]):
        src = native.KVLayout.from_chunk(kv.to(DEV), "vllm")
        blobs, arena, _ = encode(ctx, src, 0, T, T, bins)
        blob = blobs[0]
        sym, scale = ctx.quantize(src, 0, T, bins)  # the quantiser the coded path runs: held to the oracle elsewhere
        torch.cuda.synchronize()
        sym, scale = sym.cpu().numpy(), scale.cpu().numpy().view(np.uint16)
        assert int(sym.view(np.uint8).max()) <= 30
        # the whole blob from those symbols and scales: NaN rows keep the payload of the row's own NaN
        h = fm.header(blob)
        assert np.array_equal(np.frombuffer(blob, "<u2", 2 * Lk * T, int(h[fm.W_OFF_SCALES])).reshape(2 * Lk, T), scale)
        cs = [(sum((t + 1) * (int(s) + 1) for t, s in enumerate(row)) & 0xffffffff) for row in scale]
        assert np.frombuffer(blob, "<u4", 2 * Lk, int(h[fm.W_OFF_SCSUM])).tolist() == cs
        assert fm.from_static(blob, sym, np.array(bins)) == blob
        assert np.array_equal(fm.unpack_symbols(blob), sym)
        _, coded_arena, cstride = encode(ctx, src, 0, T, T, bins, fixed=False)
        for odt, ocode in ((torch.bfloat16, oracle.BF16), (torch.float16, oracle.FP16)):
            out = torch.zeros(Lk, 2, T, 1, C, dtype=odt, device=DEV)
            coded = torch.zeros_like(out)
            assert decode(ctx, [arena[:len(blob)]], native.KVLayout.from_chunk(out, "vllm"), 0, T) == 0
            ctx.decode_chunks(coded_arena.data_ptr(), cstride, 1, native.KVLayout.from_chunk(coded, "vllm"), 0, T)
            torch.cuda.synchronize()
            assert ctx.status(clear=True) == 0
            assert torch.equal(_ibits(out), _ibits(coded))
            want = oracle.dequantize(sym, scale, oracle.BF16, np.array(bins, np.int32), ocode)
            got = bits_np(out).reshape(Lk, 2, T, C)
            nan = lambda a: (a & 0x7fff) > (0x7f80 if ocode == oracle.BF16 else 0x7c00)
            assert np.array_equal(nan(got), nan(want)) and np.array_equal(got[~nan(want)], want[~nan(want)])


def _as_rows(c, layout):
    """A paged cache tensor [2, nb, bs, H, D] ("NBHD") or [2, nb, H, bs, D] ("NHBD") as [2, nb, bs, H, D]."""
    return c if layout == "NBHD" else c.permute(0, 1, 3, 2, 4)


@pytest.mark.parametrize("mapping", ["offset5", "random"])
@pytest.mark.parametrize("layout", ["NBHD", "NHBD"])
def test_paged_sources_and_destinations(ctx, oracle, layout, mapping):
    L, H, D, bs, n, cs = 2, 3, 40, 16, 50, 32
    g = torch.Generator().manual_seed(5)
    nb = 2 * ((n + 5 + bs - 1) // bs) + 2
    kv = make_kv(L, n, H, D, torch.bfloat16, seed=3)
    bins = plane_bins(L, 3)
    slots = _mapping(mapping, n, nb, bs, g)
    blk, w = slots // bs, slots % bs
    shape = (2, nb, bs, H, D) if layout == "NBHD" else (2, nb, H, bs, D)
    caches = [_random_bits(shape, torch.bfloat16, g) for _ in range(L)]
    for l in range(L):
        _as_rows(caches[l], layout)[:, blk, w] = kv[l]
    dev = [c.to(DEV) for c in caches]
    ref_blobs, _, _ = encode(ctx, native.KVLayout.from_chunk(kv.to(DEV), "vllm"), 0, n, cs, bins)
    paged = native.KVLayout.paged(dev, slots.to(DEV), bs, layout)
    blobs, arena, stride = encode(ctx, paged, 0, n, cs, bins)
    assert blobs == ref_blobs
    tup = tuple((kv[l, 0].to(DEV), kv[l, 1].to(DEV)) for l in range(L))
    assert encode(ctx, native.KVLayout.from_kv_tuple(tup, "vllm"), 0, n, cs, bins)[0] == ref_blobs
    # ... and back into a cache of random bits at another mapping: the call's slots hold the decoded rows, every other byte stays
    slots2 = _mapping(mapping, n, nb, bs, g)
    fresh = [_random_bits(shape, torch.bfloat16, g) for _ in range(L)]
    out = [c.to(DEV) for c in fresh]
    views = [arena[i * stride:i * stride + len(b)] for i, b in enumerate(blobs)]
    assert decode(ctx, views, native.KVLayout.paged(out, slots2.to(DEV), bs, layout), 0, cs) == 0
    want = torch.cat([native_bits(oracle, b) for b in blobs], dim=2)
    for l in range(L):
        exp = fresh[l].clone()
        _as_rows(exp, layout)[:, slots2 // bs, slots2 % bs] = want[l]
        assert torch.equal(_ibits(out[l].cpu()), _ibits(exp)), (layout, mapping, l)


def test_layer_ranges_and_the_schedule(ctx, oracle):
    """Ranges of layers: every schedule gives the one-piece result and fires its events in order.  (The entry point takes
    schedules that end at num_layers -- the shared body's rule -- so a range is observed through its event, not alone.)"""
    L, T, H, D = 3, 40, 2, 64
    kv = make_kv(L, T, H, D, torch.bfloat16, seed=9)
    bins = plane_bins(L)
    blobs, arena, _ = encode(ctx, native.KVLayout.from_chunk(kv.to(DEV), "vllm"), 0, T, T, bins)
    blob = arena[:len(blobs[0])]
    whole = torch.zeros(L, 2, T, H, D, dtype=torch.bfloat16, device=DEV)
    assert decode(ctx, [blob], native.KVLayout.from_chunk(whole, "vllm"), 0, T) == 0
    assert np.array_equal(bits_np(whole).reshape(L, 2, T, H * D), fm.decode_blob(oracle, blobs[0], oracle.BF16))
    seed = _random_bits((L, 2, T, H, D), torch.bfloat16, torch.Generator().manual_seed(2))
    table = torch.tensor([blob.data_ptr()], dtype=torch.int64, device=DEV)
    for ends in ([1, 3], [1, 2, 3], [2, 3]):  # (1, 2): layer 0, then layers 1 and 2
        out = seed.to(DEV)
        evs = [native.NativeEvent(timing=True) for _ in ends]
        ctx.decode_chunks_fixed_schedule(table.data_ptr(), blob.numel(), 1, native.KVLayout.from_chunk(out, "vllm"), 0, T, ends, evs)
        evs[-1].synchronize()
        assert all(e.query() for e in evs), ends  # the last event has fired: so have the ones recorded before it
        for e0, e1 in zip(evs, evs[1:]):
            ms = ctypes.c_float(-1.0)
            native.check(native.lib().lmc_event_elapsed_ms(e0.handle, e1.handle, ctypes.byref(ms)))
            assert ms.value >= 0.0, ends
        torch.cuda.synchronize()
        assert ctx.status(clear=True) == 0
        assert torch.equal(_ibits(out), _ibits(whole)), ends
    # a range's launch writes the planes of its layers only: a blob of layer 1 alone decodes to layer 1 of the whole
    one_blob, one_arena, _ = encode(ctx, native.KVLayout.from_chunk(kv[1:2].contiguous().to(DEV), "vllm"), 0, T, T, [bins[1], bins[L + 1]])
    one = torch.zeros(1, 2, T, H, D, dtype=torch.bfloat16, device=DEV)
    assert decode(ctx, [one_arena[:len(one_blob[0])]], native.KVLayout.from_chunk(one, "vllm"), 0, T) == 0
    assert torch.equal(_ibits(one[0]), _ibits(whole[1]))
    # schedules that do not end at num_layers, or do not ascend, are refused with nothing written
    out = seed.to(DEV)
    for ends in ([2], [2, 1, 3], [1, 4]):
        with pytest.raises(native.NativeError, match="rc=-1"):
            ctx.decode_chunks_fixed_schedule(table.data_ptr(), blob.numel(), 1, native.KVLayout.from_chunk(out, "vllm"), 0, T, ends, None)
    torch.cuda.synchronize()
    assert torch.equal(_ibits(out), _ibits(seed.to(DEV)))


def test_a_destination_whose_rows_take_no_vectors_is_stored_element_by_element(ctx, oracle):
    L, T, H, D = 1, 19, 2, 12  # huggingface rows of 12 channels: a head is no multiple of 8 and the heads lie T rows apart
    kv = make_kv(L, T, H, D, torch.float16, seed=12)
    bins = [18, 16]
    blobs, arena, _ = encode(ctx, native.KVLayout.from_chunk(kv.to(DEV), "vllm"), 0, T, T, bins)
    assert blobs[0] == reference(oracle, kv, H, D, bins)[0]
    seed = _random_bits((L, 2, H, T + 2, D), torch.float16, torch.Generator().manual_seed(3))
    out = seed.to(DEV)
    dst = native.KVLayout.from_chunk(out[:, :, :, 1:T + 1], "huggingface")  # rows off the 16-byte grid as well
    assert not dst.vector_readable()
    assert decode(ctx, [arena[:len(blobs[0])]], dst, 0, T) == 0
    want = seed.clone()
    dec = oracle.bits_to_torch(fm.decode_blob(oracle, blobs[0], oracle.FP16), oracle.FP16).reshape(L, 2, T, H, D)
    want[:, :, :, 1:T + 1] = dec.permute(0, 1, 3, 2, 4)
    assert torch.equal(_ibits(out.cpu()), _ibits(want))


def test_refusals_leave_destination_and_arena_as_they_were(ctx, oracle):
    L, T, H, D, bs = 1, 16, 2, 64, 16
    g = torch.Generator().manual_seed(4)
    kv = make_kv(L, T, H, D, torch.bfloat16, seed=1).to(DEV)
    bins = plane_bins(L)
    stride = native.r16(native.blob_bound(L, T, H, D))
    arena = _random_bits((stride,), torch.uint8, g).to(DEV)
    keep = arena.clone()
    sizes = torch.zeros(1, dtype=torch.int32, device=DEV)
    slots = torch.arange(T).to(DEV)
    split = native.KVLayout.paged([_random_bits((2, 2, H, D, bs), torch.bfloat16, g).to(DEV)], slots, bs, "NHDB")
    fp8 = native.KVLayout.from_chunk(torch.zeros(L, 2, T, H, D, dtype=torch.uint8, device=DEV).view(torch.float8_e4m3fn), "vllm")
    c12 = native.KVLayout.from_chunk(torch.zeros(L, 2, T, 1, 12, dtype=torch.bfloat16, device=DEV), "vllm")
    for src in (split, fp8, c12):
        with pytest.raises(native.NativeError, match="rc=-1"):
            ctx.encode_chunks_fixed(src, 0, T, T, bins, arena.data_ptr(), stride, sizes.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(arena, keep) and int(sizes[0]) == 0
    fixed, farena, _ = encode(ctx, native.KVLayout.from_chunk(kv, "vllm"), 0, T, T, bins)
    coded, carena, cstride = encode(ctx, native.KVLayout.from_chunk(kv, "vllm"), 0, T, T, bins, fixed=False)
    fblob, cblob = farena[:len(fixed[0])], carena[:len(coded[0])]
    cache = _random_bits((2, 2, H, D, bs), torch.bfloat16, g).to(DEV)
    cache_keep = cache.clone()
    table = torch.tensor([fblob.data_ptr()], dtype=torch.int64, device=DEV)
    fp8_out = torch.zeros(L, 2, T, H, D, dtype=torch.uint8, device=DEV)
    for dst in (native.KVLayout.paged([cache], slots, bs, "NHDB"), native.KVLayout.from_chunk(fp8_out.view(torch.float8_e4m3fn), "vllm")):
        with pytest.raises(native.NativeError, match="rc=-1"):
            ctx.decode_chunks_fixed_schedule(table.data_ptr(), fblob.numel(), 1, dst, 0, T, [L], None)
    torch.cuda.synchronize()
    assert torch.equal(_ibits(cache), _ibits(cache_keep)) and int(fp8_out.max()) == 0
    # each model's decoder refuses the other's blob: BAD_HEADER, nothing stored
    seed = _random_bits((L, 2, T, H, D), torch.bfloat16, g).to(DEV)
    out = seed.clone()
    assert decode(ctx, [cblob], native.KVLayout.from_chunk(out, "vllm"), 0, T) == BAD_HEADER
    ctx.decode_chunks(farena.data_ptr(), native.r16(native.blob_bound(L, T, H, D)), 1, native.KVLayout.from_chunk(out, "vllm"), 0, T)
    torch.cuda.synchronize()
    assert ctx.status(clear=True) == BAD_HEADER
    assert torch.equal(_ibits(out), _ibits(seed))


def test_damage_is_flagged_and_the_intact_blob_still_decodes(ctx, oracle):
    L, T, H, D = 2, 100, 3, 40
    kv = make_kv(L, T, H, D, torch.bfloat16, seed=21)
    bins = plane_bins(L, 1)
    blobs, arena, _ = encode(ctx, native.KVLayout.from_chunk(kv.to(DEV), "vllm"), 0, T, T, bins)
    blob = blobs[0]
    assert blob == reference(oracle, kv, H, D, bins)[0]
    out = torch.zeros(L, 2, T, H, D, dtype=torch.bfloat16, device=DEV)
    dst = native.KVLayout.from_chunk(out, "vllm")
    spans = fm.stream_spans(blob)
    rng = np.random.default_rng(2024)

    def status_of(damaged):
        return decode(ctx, dev_blobs([bytes(damaged)]), dst, 0, T)

    for case in range(40):
        b, e = spans[int(rng.integers(len(spans)))]
        nflip = 1 + case % 16
        pos = rng.choice(np.arange(b, e + 4), size=nflip, replace=False)  # lo, hi and the check word
        d = bytearray(blob)
        for q in pos:
            d[q] ^= int(rng.integers(1, 256))
        payload = np.frombuffer(bytes(d), "<u4", (e - b) // 4, b)
        assert fm.check_word(payload) != int(np.frombuffer(bytes(d), "<u4", 1, e)[0]), "the damage cancels in the check word"
        assert status_of(d) == BAD_STREAM, (case, sorted(pos.tolist()))
    h = fm.header(blob)
    off_scales, off_scsum, off_gdir = int(h[fm.W_OFF_SCALES]), int(h[fm.W_OFF_SCSUM]), int(h[fm.W_OFF_GDIR])
    for where in (off_scales + 3, off_scales + 2 * (2 * L * T) - 1, off_scsum, off_scsum + 4 * (2 * L) - 1):
        d = bytearray(blob)
        d[where] ^= 0x10
        assert status_of(d) & BAD_SCALES, where
    for where in (0, 4 * fm.W_TOTAL, 4 * fm.W_MODEL, 4 * fm.W_STREAM_BYTES, off_gdir, off_gdir + 8 * 3 + 4, off_gdir + 8 * (len(spans) - 1)):
        d = bytearray(blob)
        d[where] ^= 0x10
        assert status_of(d) & BAD_HEADER, where
    assert status_of(blob) == 0
    assert np.array_equal(bits_np(out).reshape(L, 2, T, H * D), fm.decode_blob(oracle, blob, oracle.BF16))


# ---- the engine on the fixed-width HBM tier ---------------------------------------------------------------------------
EL, EH, ED, ECS, ENT = 2, 2, 64, 16, 40


def _engine(serde):
    cfg = LMCacheEngineConfig.from_legacy(chunk_size=ECS, backend="cuda", local_serde=serde)
    return LMCacheEngine(cfg, dumb_metadata("vllm", "Llama-3-8B"))


def _kv_tuple(seed, n=ENT):
    g = torch.Generator().manual_seed(seed)
    return tuple((torch.randn((n, EH, ED), generator=g).to(torch.bfloat16).to(DEV),
                  torch.randn((n, EH, ED), generator=g).to(torch.bfloat16).to(DEV)) for _ in range(EL))


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(_ibits(x), _ibits(y)) for la, lb in zip(a, b) for x, y in zip(la, lb))


def test_engine_store_and_retrieve_equal_the_coded_tier():
    fx, cg = _engine("cachegen-fixed"), _engine("cachegen")
    try:
        assert fx.engine_.mode == cg.engine_.mode == "hbm-cachegen" and fx.engine_.model == "fixed" and cg.engine_.model == "rans"
        tokens = generate_tokens(ENT, DEV)
        kv = _kv_tuple(1)
        for e in (fx, cg):
            e.store(tokens, kv)
        keys = [fx._make_key(h, "vllm") for h in fx._prefix_hashes_of(tokens)]
        be = fx.engine_
        assert be.contains_prefix(keys) == 3
        bins = be.cachegen_config.plane_bins(EL)
        assert [be.dict[k].blob.numel() for k in keys] == [native.fixed_blob_bytes(EL, t, EH, ED, bins) for t in (16, 16, 8)]
        assert be.chunk_meta(keys[2]) == ((EL, 2, 8, EH, ED), torch.bfloat16)
        assert be.tier_stats()["hbm"]["live_bytes"] == sum(native.r16(be.dict[k].blob.numel()) for k in keys)
        a, ma = fx.retrieve(tokens)
        b, mb = cg.retrieve(tokens)
        assert bool(ma.all()) and torch.equal(ma, mb) and _same(a, b)
        chunk = be.get(keys[1])
        assert torch.equal(_ibits(chunk), _ibits(cg.engine_.get(keys[1])))
        for lpl in (1, 2):
            lw, ref = fx.retrieve_layerwise(tokens, layers_per_launch=lpl), cg.retrieve_layerwise(tokens, layers_per_launch=lpl)
            assert [end for end, _ in lw.layer_events] == [end for end, _ in ref.layer_events] == ([1, 2] if lpl == 1 else [2])
            for l in range(EL):
                lw.wait_layer(l)
            lw.finish()
            ref.finish()
            assert _same(lw.kv, ref.kv) and _same(lw.kv, a)
        # a suffix mask: the first-chunk trim
        mask = torch.ones(ENT, dtype=torch.bool, device=DEV)
        mask[:21] = False
        a2, m2 = fx.retrieve(tokens, mask)
        b2, _ = cg.retrieve(tokens, mask)
        assert int(m2.sum()) == ENT - 21 and _same(a2, b2)
        # a blob damaged in the arena is a miss, not garbage
        blob = be.dict[keys[1]].blob
        spot = fm.stream_spans(bytes(blob.cpu().numpy()))[3][0] + 7
        old = int(blob[spot])
        blob[spot] = old ^ 0x3c
        ret, m = fx.retrieve(tokens)
        assert ret == () and not m.any()
        assert be.get(keys[1]) is None and be.get(keys[0]) is not None
        blob[spot] = old
        ret, m = fx.retrieve(tokens)
        assert bool(m.all()) and _same(ret, a)
    finally:
        torch.cuda.synchronize()
        fx.close()
        cg.close()


@pytest.mark.parametrize("layout", ["NBHD", "NHBD", "NHDB"])
def test_engine_paged_store_and_retrieve_equal_the_coded_tier(layout):
    bs = 16
    nb = 2 * ((ENT + 5 + bs - 1) // bs) + 2
    g = torch.Generator().manual_seed(33)
    shape = {"NBHD": (2, nb, bs, EH, ED), "NHBD": (2, nb, EH, bs, ED), "NHDB": (2, nb, EH, ED, bs)}[layout]
    tokens = generate_tokens(ENT, DEV)
    uniform = RopeShift.from_base(10000.0, ED, 128, DEV, is_neox=True, delta=17)
    per_tok = RopeShift(uniform.cos_sin, ED, True, torch.randint(-100, 100, (ENT,), generator=g, dtype=torch.int32).to(DEV))
    fx, cg = _engine("cachegen-fixed"), _engine("cachegen")
    try:
        src = [_random_bits(shape, torch.bfloat16, g).to(DEV) for _ in range(EL)]
        finite = [torch.nan_to_num(c.float(), nan=1.0, posinf=2.0, neginf=-2.0).clamp(-1e4, 1e4).to(torch.bfloat16) for c in src]
        slots = _mapping("offset5", ENT, nb, bs, g).to(DEV)
        # the prefix layer-wise (the documented fallback: one piece at finish()), the rest with store_paged
        st = fx.store_paged_layerwise(tokens[:ECS], finite, slots[:ECS], bs, layout, direct=layout == "NHDB")
        assert not st.layerwise and st.layer_event(0) is None
        st.save_layer(0)
        assert st.finish() == 1
        fx.store_paged(tokens, finite, slots, bs, layout, direct=layout == "NHDB")
        twin = _engine("cachegen-fixed")
        try:
            twin.store_paged(tokens, finite, slots, bs, layout)
            keys = [fx._make_key(h, "vllm") for h in fx._prefix_hashes_of(tokens)]
            for k in keys:  # the fallback's blobs, the direct store's and the staged store's are the same bytes
                assert torch.equal(fx.engine_.dict[k].blob, twin.engine_.dict[k].blob), k
        finally:
            twin.close()
        cg.store_paged(tokens, finite, slots, bs, layout)
        for direct in ((False, True) if layout == "NHDB" else (False,)):
            for rope in (None, uniform, per_tok):
                for lw in (False, True):
                    slots2 = _mapping("random", ENT, nb, bs, g).to(DEV)
                    a = [_random_bits(shape, torch.bfloat16, g).to(DEV) for _ in range(EL)]
                    b = [c.clone() for c in a]
                    what = (layout, direct, rope is not None and rope is per_tok, lw)
                    if lw:
                        r = fx.retrieve_into_paged_layerwise(tokens, a, slots2, bs, layout, rope=rope, direct=direct, layers_per_launch=1)
                        assert [end for end, _ in r.layer_events] == [1, 2], what
                        for l in range(EL):
                            r.wait_layer(l)
                        r.finish()
                        ma = r.ret_mask
                    else:
                        ma = fx.retrieve_into_paged(tokens, a, slots2, bs, layout, rope=rope, direct=direct)
                    mb = cg.retrieve_into_paged(tokens, b, slots2, bs, layout, rope=rope)
                    torch.cuda.synchronize()
                    assert bool(ma.all()) and torch.equal(ma, mb), what
                    for l in range(EL):
                        assert torch.equal(_ibits(a[l]), _ibits(b[l])), what
    finally:
        torch.cuda.synchronize()
        fx.close()
        cg.close()


def test_engine_hbm_budget_evicts_in_lru_order():
    fx = _engine("cachegen-fixed")
    try:
        be = fx.engine_
        bins = be.cachegen_config.plane_bins(EL)
        group = sum(native.r16(native.fixed_blob_bytes(EL, t, EH, ED, bins)) for t in (16, 16, 8))
        be.set_capacity(hbm_bytes=2 * group, pinned_bytes=1 << 30)  # (a pinned budget too: dropped all the same, not demoted)
        prompts = [(generate_tokens(ENT, DEV) + 20000 * i, _kv_tuple(40 + i)) for i in range(4)]
        for t, kv in prompts[:2]:
            fx.store(t, kv)
        assert bool(fx.retrieve(prompts[0][0])[1].all())  # a hit: prompt 0 is now the most recent, prompt 1 the LRU group
        fx.store(*prompts[2])
        assert not fx.retrieve(prompts[1][0])[1].any()
        assert bool(fx.retrieve(prompts[0][0])[1].all()) and bool(fx.retrieve(prompts[2][0])[1].all())
        fx.store(*prompts[3])
        assert not fx.retrieve(prompts[0][0])[1].any() and bool(fx.retrieve(prompts[3][0])[1].all())
        st = be.tier_stats()
        assert st["evictions"] == 2 and st["demotions"] == 0 and st["hbm"]["live_bytes"] <= 2 * group and st["pinned"]["groups"] == 0
    finally:
        torch.cuda.synchronize()
        fx.close()
