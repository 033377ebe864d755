"""fp8 KV (OCP float8_e4m3fn / float8_e5m2) on the GPU.

The contract (include/lmc_format.h): an fp8 chunk x encodes exactly as the bf16 chunk u = x.to(bfloat16) does -- the
blob is the oracle's blob of u with header word 23 (bytes 92..95) set to the fp8 code -- and a decode into an fp8
destination is torch's CPU cast of the fp32 dequantisation (s - C) / C * max1.  NaN is compared by NaN-ness."""
import struct

import numpy as np
import pytest
import torch

from lmcache_amd import native
from tests.test_gpu_engine import MODEL, dumb_metadata, generate_tokens, make_cfg

pytestmark = pytest.mark.gpu

FP8 = [torch.float8_e4m3fn, torch.float8_e5m2]
IDS = ["e4m3", "e5m2"]
FMAX = {torch.float8_e4m3fn: 448.0, torch.float8_e5m2: 57344.0}


def _bytes(t):
    return t.contiguous().view(torch.uint8).cpu()


def _data(kind, shape, dt, g):
    if kind == "rand":
        x = torch.rand(shape, generator=g) * 2 - 1
    elif kind == "randn":
        x = torch.randn(shape, generator=g) * (8 if dt == torch.float8_e4m3fn else 200)
    else:  # outliers: mostly small values, a few near the format's max
        x = torch.randn(shape, generator=g) * 0.05
        m = torch.rand(shape, generator=g) < 0.002
        x[m] = torch.randn(int(m.sum()), generator=g) * FMAX[dt] / 3
    return x.clamp(-FMAX[dt], FMAX[dt]).to(dt)


def _edge_rows(x, dt):
    """Rows (tokens) with special maxima, on the [L, 2, T, C] view: all zero, a NaN, +-max, subnormal only, e5m2 +-inf."""
    v = x.view(torch.uint8)
    T = x.shape[2]
    rows = [t for t in (0, 1, 2, 3, 4, 5) if t < T]
    sub = 0x07 if dt == torch.float8_e4m3fn else 0x03  # largest subnormal
    for i, t in enumerate(rows):
        r = v[:, :, t]
        if i == 0:
            r.zero_()
        elif i == 1:
            r[..., 3] = 0x7F
        elif i == 2:
            r[..., 5] = 0x7E if dt == torch.float8_e4m3fn else 0x7B  # +max
            r[..., 6] = r[..., 5] | 0x80
        elif i == 3:
            r.copy_(r & 0x80 | (r & sub))
        elif i == 4 and dt == torch.float8_e5m2:
            r[..., 1] = 0x7C
        elif i == 5 and dt == torch.float8_e5m2:
            r[..., 2] = 0xFC
    return x


def _oracle_blob(oracle, x, H, D, bins):
    """The oracle's blob of the bf16 images of x [L, 2, T, C], with word 23 = x's fp8 code."""
    bits, code = oracle.torch_to_bits(x.cpu().to(torch.bfloat16))
    blob = oracle.encode_blob(bits, code, H, D, np.array(bins, np.int32))
    return blob[:92] + struct.pack("<I", native.dtype_code(x.dtype)) + blob[96:]


def _formula(oracle, x, bins, dt):
    """torch CPU: do_dequantize in fp32 of the oracle's symbols / scales of x's images, then ONE cast to dt.
    x [L, 2, T, C] (any 16- or 8-bit dtype).  -> [L, 2, T, C] in dt."""
    bits, code = oracle.torch_to_bits(x.cpu().to(torch.bfloat16) if x.dtype in FP8 else x.cpu())
    bins = np.array(bins, np.int32)
    sym, scale = oracle.quantize(bits, code, bins)  # [P, T, C] int8, [P, T] u16
    L, _, T, C = x.shape
    sc = oracle.bits_to_torch(scale, code).float().reshape(2 * L, T, 1)
    cc = torch.tensor([b // 2 - 1 for b in bins], dtype=torch.float32).reshape(-1, 1, 1)
    q = torch.from_numpy(sym.astype(np.int16)).float()
    t = (q - cc) / cc * sc  # three separately rounded fp32 ops
    t = t.reshape(2, L, T, C).permute(1, 0, 2, 3)
    return t.to(dt)


def _cat8(ts, dim):
    """torch.cat of fp8 tensors through their bytes."""
    return torch.cat([t.cpu().view(torch.uint8) for t in ts], dim).view(ts[0].dtype)


def _stack_kv(kv):
    """A per-layer (K, V) tuple -> [L, 2, ...] on the host, through the bytes."""
    return torch.stack([torch.stack((k.cpu().view(torch.uint8), v.cpu().view(torch.uint8))) for k, v in kv]).view(kv[0][0].dtype)


def _same(a, b):
    """Bit equality of two fp8 tensors, NaN by NaN-ness."""
    a, b = a.cpu(), b.cpu()
    na, nb = torch.isnan(a.float()), torch.isnan(b.float())
    assert torch.equal(na, nb)
    assert torch.equal(a.view(torch.uint8)[~na], b.view(torch.uint8)[~nb])


def _encode(layout, T, cs, bins, path):
    ctx = native.get_context(0)
    L, H, D = layout.L, layout.H, layout.D
    stride = native.r16(native.blob_bound(L, cs, H, D))
    n = (T + cs - 1) // cs
    blobs = torch.zeros(n * stride, dtype=torch.uint8, device="cuda")
    sizes = torch.zeros(n, dtype=torch.int32, device="cuda")
    ctx.set_encode_path(path)
    try:
        ctx.encode_chunks(layout, 0, T, cs, bins, blobs.data_ptr(), stride, sizes.data_ptr())
        torch.cuda.synchronize()
    finally:
        ctx.set_encode_path("auto")
    ctx.raise_on_status("encode")
    sz = sizes.cpu().tolist()
    host = blobs.cpu().numpy()
    return [host[i * stride:i * stride + sz[i]].tobytes() for i in range(n)], blobs, stride


def _bins(L, g):
    choice = [32, 16, 23, 32, 16]
    return [choice[int(i)] for i in torch.randint(0, len(choice), (2 * L,), generator=g)]


def _check_chunks(oracle, x, blobs, cs, H, D, bins):
    """x [L, 2, T, C] (fp8, cpu); blobs: the GPU's chunk blobs."""
    T = x.shape[2]
    for i, b in enumerate(blobs):
        part = x[:, :, i * cs:min(T, (i + 1) * cs)]
        want = _oracle_blob(oracle, part, H, D, bins)
        assert b == want, f"chunk {i}: blob differs from the oracle's blob of the bf16 images"
        assert struct.unpack_from("<II", b, 88)[1] == native.dtype_code(x.dtype) and struct.unpack_from("<I", b, 8)[0] == 0


GEOMS = [(2, 256, 8, 128), (3, 600, 2, 64), (1, 7, 1, 8)]


@pytest.mark.parametrize("dt", FP8, ids=IDS)
@pytest.mark.parametrize("path", ["two_kernels", "fused"])
def test_blob_parity_contiguous_fixed_and_edge_rows(oracle, dt, path):
    g = torch.Generator().manual_seed(11)
    for (L, T, H, D), kind in zip(GEOMS, ["randn", "outlier", "rand"]):
        x = _edge_rows(_data(kind, (L, 2, T, H * D), dt, g), dt)
        bins = _bins(L, g)
        xd = x.reshape(L, 2, T, H, D).cuda()
        blobs, dev, stride = _encode(native.KVLayout.from_chunk(xd, "vllm"), T, 256, bins, path)
        _check_chunks(oracle, x, blobs, 256, H, D, bins)
        # decode back into an fp8 chunk: torch's cast of the fp32 formula, chunk by chunk
        out = torch.zeros_like(xd)
        native.get_context(0).decode_chunks(dev.data_ptr(), stride, len(blobs), native.KVLayout.from_chunk(out, "vllm"), 0, 256)
        torch.cuda.synchronize()
        native.get_context(0).raise_on_status("decode")
        for i in range(len(blobs)):
            sl = slice(i * 256, min(T, (i + 1) * 256))
            _same(out.reshape(L, 2, T, H * D)[:, :, sl], _formula(oracle, x[:, :, sl], bins, dt))


@pytest.mark.parametrize("dt", FP8, ids=IDS)
def test_blob_parity_random_geometry_sweep(oracle, dt):
    g = torch.Generator().manual_seed(12 + native.dtype_code(dt))
    for it, T in enumerate([1, 2, 7, 255, 256, 257, 512 + 37]):
        L = int(torch.randint(1, 4, (1,), generator=g))
        D = [8, 24, 40, 100, 128, 72][it % 6]
        H = int(torch.randint(1, 9, (1,), generator=g))
        while (H * D) % 8:
            H += 1
        if it == 6:
            H, D = 32, 128  # C = 4096: the wide-plane (two-kernel, split) quantiser
        x = _data(["rand", "randn", "outlier"][it % 3], (L, 2, T, H * D), dt, g)
        bins = _bins(L, g)
        xd = x.reshape(L, 2, T, H, D).cuda()
        for path in ("two_kernels", "fused"):
            blobs, _, _ = _encode(native.KVLayout.from_chunk(xd, "vllm"), T, 256, bins, path)
            _check_chunks(oracle, x, blobs, 256, H, D, bins)


@pytest.mark.parametrize("dt", FP8, ids=IDS)
def test_blob_parity_tuple_and_paged_sources(oracle, dt):
    g = torch.Generator().manual_seed(13)
    L, T, H, D, bs = 2, 300, 4, 128, 16
    x = _data("randn", (L, 2, T, H * D), dt, g)
    bins = _bins(L, g)
    x5 = x.reshape(L, 2, T, H, D)
    kv = tuple((x5[l, 0].cuda(), x5[l, 1].cuda()) for l in range(L))
    for path in ("two_kernels", "fused"):
        blobs, _, _ = _encode(native.KVLayout.from_kv_tuple(kv, "vllm"), T, 256, bins, path)
        _check_chunks(oracle, x, blobs, 256, H, D, bins)
    nblocks = (T + bs - 1) // bs + 5
    slots = torch.randperm(nblocks * bs, generator=g)[:T]
    blk, off = slots // bs, slots % bs
    for layout in ("NHBD", "NBHD"):
        shape = (2, nblocks, bs, H, D) if layout == "NBHD" else (2, nblocks, H, bs, D)
        caches = []
        for l in range(L):
            c = torch.zeros(shape, dtype=torch.uint8)
            for kvi in range(2):
                if layout == "NBHD":
                    c[kvi, blk, off] = x5[l, kvi].view(torch.uint8)
                else:
                    c[kvi, blk, :, off] = x5[l, kvi].view(torch.uint8)
            caches.append(c.view(dt).cuda())
        lay = native.KVLayout.paged(caches, slots.cuda(), bs, layout)
        for path in ("two_kernels", "fused"):
            blobs, dev, stride = _encode(lay, T, 256, bins, path)
            _check_chunks(oracle, x, blobs, 256, H, D, bins)
        # decode into ANOTHER paged cache at other random slots; the slots outside the mapping stay untouched
        slots2 = torch.randperm(nblocks * bs, generator=g)[:T]
        dst = [torch.full(shape, 0x11, dtype=torch.uint8).view(dt).cuda() for _ in range(L)]
        native.get_context(0).decode_chunks(dev.data_ptr(), stride, len(blobs),
                                            native.KVLayout.paged(dst, slots2.cuda(), bs, layout), 0, 256)
        torch.cuda.synchronize()
        native.get_context(0).raise_on_status("decode")
        b2, o2 = slots2 // bs, slots2 % bs
        want = _cat8([_formula(oracle, x[:, :, i:i + 256], bins, dt) for i in range(0, T, 256)], 2)
        for l in range(L):
            c = dst[l].view(torch.uint8).cpu()
            for kvi in range(2):
                got = c[kvi, b2, o2] if layout == "NBHD" else c[kvi, b2, :, o2]
                _same(got.view(dt).reshape(T, H * D), want[l, kvi])
            used = torch.zeros(nblocks * bs, dtype=torch.bool)
            used[slots2] = True
            free = (~used).nonzero().flatten()
            rest = c[:, free // bs, free % bs] if layout == "NBHD" else c[:, free // bs, :, free % bs]
            assert (rest == 0x11).all()


@pytest.mark.parametrize("dt", FP8, ids=IDS)
def test_exhaustive_decode_cast(oracle, dt):
    """Every positive finite fp8 value as a row max, elements spread over the symbols, bins 32 / 16 / 23."""
    vals = torch.arange(1, 256, dtype=torch.int32).to(torch.uint8).view(dt).float()
    vals = vals[torch.isfinite(vals) & (vals > 0)]
    T, C = vals.numel(), 64
    L = 2
    bins = [32, 16, 23, 32]
    j = torch.arange(C, dtype=torch.float32)
    rows = []
    for p in range(2 * L):
        mx = bins[p] // 2 - 1
        frac = ((j % (2 * mx + 1)) - mx) / mx  # -1 .. 1 in symbol steps
        r = (frac[None, :] * vals[:, None]).to(dt)
        r.view(torch.uint8)[:, 0] = vals.to(dt).view(torch.uint8)  # the row max itself
        rows.append(r)
    x = torch.stack([r.view(torch.uint8) for r in rows]).reshape(2, L, T, C).permute(1, 0, 2, 3).contiguous().view(dt)
    xd = x.reshape(L, 2, T, 8, 8).cuda()
    blobs, dev, stride = _encode(native.KVLayout.from_chunk(xd, "vllm"), T, 256, bins, "two_kernels")
    _check_chunks(oracle, x, blobs, 256, 8, 8, bins)
    out = torch.zeros_like(xd)
    native.get_context(0).decode_chunks(dev.data_ptr(), stride, 1, native.KVLayout.from_chunk(out, "vllm"), 0, 256)
    torch.cuda.synchronize()
    native.get_context(0).raise_on_status("decode")
    _same(out.reshape(L, 2, T, C), _formula(oracle, x, bins, dt))


@pytest.mark.parametrize("dt", FP8, ids=IDS)
def test_cross_dtype_decodes(oracle, dt):
    """An fp8 blob into a bf16 destination (= the oracle's decode of the images' blob) and a bf16 blob into fp8."""
    g = torch.Generator().manual_seed(14)
    L, T, H, D = 2, 256, 2, 64
    bins = [32, 16, 16, 32]
    x = _data("randn", (L, 2, T, H * D), dt, g)
    blob = _oracle_blob(oracle, x, H, D, bins)
    ctx = native.get_context(0)
    dev = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
    out = torch.zeros(L, 2, T, H, D, dtype=torch.bfloat16, device="cuda")
    ctx.decode_chunks(dev.data_ptr(), native.r16(len(blob)), 1, native.KVLayout.from_chunk(out, "vllm"), 0, T)
    torch.cuda.synchronize()
    ctx.raise_on_status("decode")
    want = oracle.bits_to_torch(oracle.decode_blob(blob, oracle.BF16), oracle.BF16)
    assert torch.equal(out.cpu().reshape(-1).view(torch.int16), want.reshape(-1).view(torch.int16))
    y = torch.randn(L, 2, T, H * D, generator=g).to(torch.bfloat16)
    bits, code = oracle.torch_to_bits(y)
    blob2 = oracle.encode_blob(bits, code, H, D, np.array(bins, np.int32))
    dev2 = torch.frombuffer(bytearray(blob2), dtype=torch.uint8).cuda()
    out8 = torch.zeros(L, 2, T, H, D, dtype=dt, device="cuda")
    ctx.decode_chunks(dev2.data_ptr(), native.r16(len(blob2)), 1, native.KVLayout.from_chunk(out8, "vllm"), 0, T)
    torch.cuda.synchronize()
    ctx.raise_on_status("decode")
    _same(out8.reshape(L, 2, T, H * D), _formula(oracle, y, bins, dt))


@pytest.mark.parametrize("dt", FP8, ids=IDS)
def test_copy_kv_vector_and_element_paths(dt):
    g = torch.Generator().manual_seed(15)
    ctx = native.get_context(0)
    for D in (128, 100):  # 100 under huggingface: not vector-readable -> the element path
        x = _data("randn", (2, 2, 4, 70, D), dt, g).cuda()  # [L,2,H,T,D]
        dst = torch.zeros(2, 2, 70, 4, D, dtype=dt, device="cuda")
        ctx.copy_kv(native.KVLayout.from_chunk(x, "huggingface"), 0, 70, native.KVLayout.from_chunk(dst, "vllm"), 0)
        torch.cuda.synchronize()
        assert torch.equal(_bytes(dst), _bytes(x.permute(0, 1, 3, 2, 4)))
    x = _data("rand", (2, 2, 64, 4, 128), dt, g).cuda()
    y = torch.zeros_like(x)
    ctx.copy_kv(native.KVLayout.from_chunk(x, "vllm"), 0, 64, native.KVLayout.from_chunk(y, "vllm"), 0)
    torch.cuda.synchronize()
    assert torch.equal(_bytes(y), _bytes(x))


def _kv(T, L, H, D, dt, g):
    x = _data("randn", (L, 2, T, H, D), dt, g)
    return tuple((x[l, 0].cuda(), x[l, 1].cuda()) for l in range(L)), x


def _engine_bins(oracle, L):
    b, _ = oracle.cachegen_bins(MODEL)
    return list(np.concatenate([b[:len(b) // 2][:L], b[len(b) // 2:][:L]]))


def _prefix_hits_of_a_bf16_engine(backend, x, L, H, D, T, n):
    """What the same backend returns for an n-token prefix of a T-token bf16 prompt: (hit count, the tensor [L,2,hits,C])."""
    from lmcache_amd.cache_engine import LMCacheEngine
    tokens = generate_tokens(T, "cuda")  # its own prompt: a shared store must not answer with the fp8 chunks
    kv = tuple((x[l, 0].to(torch.bfloat16).cuda(), x[l, 1].to(torch.bfloat16).cuda()) for l in range(L))
    engine = LMCacheEngine(make_cfg(backend), dumb_metadata("vllm", MODEL))
    try:
        engine.store(tokens, kv)
        got, m = engine.retrieve(tokens[:n])
        hits = int(m.sum())
        return hits, torch.stack([torch.stack(p) for p in got]).reshape(L, 2, hits, H * D).cpu() if hits else None
    finally:
        engine.close()


REMOTE = ["mem://cachegen:1", "mem://cachegenpipe:1", "xgmi://cachegen:1", "xgmi://cachegenpipe:1"]


@pytest.mark.parametrize("dt", FP8, ids=IDS)
@pytest.mark.parametrize("backend", ["cuda", "cpu", "cachegen-host", "cachegen-hbm"] + REMOTE)
def test_engine_store_retrieve(oracle, dt, backend):
    from lmcache_amd.cache_engine import LMCacheEngine
    g = torch.Generator().manual_seed(16)
    L, H, D, T = 4, 8, 128, 600
    kv, x = _kv(T, L, H, D, dt, g)
    ref_hits, ref = _prefix_hits_of_a_bf16_engine(backend, x, L, H, D, T, 300)  # (before: one engine at a time)
    tokens = generate_tokens(T, "cuda")
    engine = LMCacheEngine(make_cfg(backend), dumb_metadata("vllm", MODEL))
    try:
        engine.store(tokens, kv)
        got, mask = engine.retrieve(tokens)
        assert int(mask.sum()) == T
        assert got[0][0].dtype == dt
        lossless = backend in ("cuda", "cpu")
        x4 = x.reshape(L, 2, T, H * D)
        bins = _engine_bins(oracle, L)
        want = x4 if lossless else _cat8([_formula(oracle, x4[:, :, i:i + 256], bins, dt) for i in range(0, T, 256)], 2)
        have = _stack_kv(got).reshape(L, 2, T, H * D)
        _same(have, want)
        # layer by layer
        r = engine.retrieve_layerwise(tokens, layers_per_launch=1)
        for l in range(L):
            r.wait_layer(l)
            assert r.kv[l][0].dtype == dt
            _same(_stack_kv((r.kv[l],))[0].reshape(2, T, H * D), want[l])
        r.finish()
        # a suffix mask: the masked-out prefix is not returned
        mask = torch.ones(T, dtype=torch.bool, device="cuda")
        mask[:200] = False
        got1, m1 = engine.retrieve(tokens, mask)
        assert int(m1.sum()) == T - 200
        _same(_stack_kv(got1).reshape(L, 2, T - 200, H * D), want[:, :, 200:])
        # a 300-token prefix of the prompt: the same hits as a bf16 prompt on the same backend, and their values
        got2, mask2 = engine.retrieve(tokens[:300])
        hits = int(mask2.sum())
        assert hits == ref_hits and hits > 0
        _same(_stack_kv(got2).reshape(L, 2, hits, H * D), want[:, :, :hits])
        if lossless:
            assert torch.equal(ref, want[:, :, :hits].to(torch.bfloat16))
        engine.store(tokens, kv)  # skip_existing
        got3, mask3 = engine.retrieve(tokens)
        assert int(mask3.sum()) == T
        _same(_stack_kv(got3).reshape(L, 2, T, H * D), want)
    finally:
        engine.close()


@pytest.mark.parametrize("dt", FP8, ids=IDS)
@pytest.mark.parametrize("backend", ["cuda", "cpu", "cachegen-host", "cachegen-hbm"])
def test_engine_paged_store_and_retrieve_into_paged(oracle, dt, backend):
    from lmcache_amd.cache_engine import LMCacheEngine
    g = torch.Generator().manual_seed(17)
    L, H, D, T, bs = 2, 8, 128, 512, 16
    x = _data("randn", (L, 2, T, H, D), dt, g)
    nblocks = T // bs + 4
    shape = (2, nblocks, bs, H, D)
    slots = torch.randperm(nblocks * bs, generator=g)[:T]
    src = []
    for l in range(L):
        c = torch.zeros(shape, dtype=torch.uint8)
        for kvi in range(2):
            c[kvi, slots // bs, slots % bs] = x[l, kvi].view(torch.uint8)
        src.append(c.view(dt).cuda())
    dst = [torch.zeros(shape, dtype=dt, device="cuda") for _ in range(L)]
    tokens = generate_tokens(T, "cuda")
    engine = LMCacheEngine(make_cfg(backend), dumb_metadata("vllm", MODEL))
    try:
        engine.store_paged(tokens, src, slots.cuda(), bs, "NBHD")
        m = engine.retrieve_into_paged(tokens, dst, slots.cuda(), bs, "NBHD")
        assert int(m.sum()) == T
        torch.cuda.synchronize()
        x4 = x.reshape(L, 2, T, H * D)
        bins = _engine_bins(oracle, L)
        want = x4 if backend in ("cuda", "cpu") else _cat8([_formula(oracle, x4[:, :, i:i + 256], bins, dt) for i in range(0, T, 256)], 2)
        for l in range(L):
            c = dst[l].view(torch.uint8).cpu()
            for kvi in range(2):
                _same(c[kvi, slots // bs, slots % bs].view(dt).reshape(T, H * D), want[l, kvi])
    finally:
        engine.close()


@pytest.mark.parametrize("dt", FP8, ids=IDS)
def test_serde_round_trip(oracle, dt):
    from lmcache_amd.config import LMCacheEngineConfig, LMCacheEngineMetadata
    from lmcache_amd.storage_backend.serde.cachegen_decoder import CacheGenDeserializer
    from lmcache_amd.storage_backend.serde.cachegen_encoder import CacheGenSerializer
    g = torch.Generator().manual_seed(18)
    config = LMCacheEngineConfig.from_defaults(chunk_size=256)
    meta = LMCacheEngineMetadata(MODEL, 1, 0, "vllm", "bfloat16")
    L, T, H, D = 4, 256, 8, 128
    x = _data("randn", (L, 2, T, H, D), dt, g)
    bs = CacheGenSerializer(config, meta).to_bytes(x.cuda())
    bins = _engine_bins(oracle, L)
    assert bs == _oracle_blob(oracle, x.reshape(L, 2, T, H * D), H, D, bins)
    out = CacheGenDeserializer(config, meta).from_bytes(bs)
    assert out.dtype == torch.bfloat16  # the reference's rule for from_bytes
    bits, code = oracle.torch_to_bits(x.reshape(L, 2, T, H * D).to(torch.bfloat16))
    want = oracle.bits_to_torch(oracle.decode_blob(oracle.encode_blob(bits, code, H, D, np.array(bins, np.int32)), oracle.BF16),
                                oracle.BF16)
    assert torch.equal(out.cpu().reshape(-1).view(torch.int16), want.reshape(-1).view(torch.int16))


def test_uint8_cache_is_refused_with_the_view_hint():
    c = torch.zeros(2, 4, 16, 2, 64, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="float8_e4m3fn"):
        native.KVLayout.paged([c], torch.arange(10, device="cuda"), 16, "NBHD")


@pytest.mark.parametrize("dt", FP8, ids=IDS)
def test_disk_tier_returns_fp8(oracle, dt, tmp_path):
    from lmcache_amd.cache_engine import LMCacheEngine
    from lmcache_amd.config import LMCacheEngineConfig
    from lmcache_amd.storage_backend.local_backend import LMCLocalDiskBackend
    g = torch.Generator().manual_seed(19)
    L, H, D, T = 2, 8, 128, 600
    kv, x = _kv(T, L, H, D, dt, g)
    cfg = LMCacheEngineConfig.from_legacy(chunk_size=256, backend="file://" + str(tmp_path) + "/")
    cfg.local_serde = "cachegen"
    engine = LMCacheEngine(cfg, dumb_metadata("vllm", MODEL))
    try:
        assert isinstance(engine.engine_, LMCLocalDiskBackend)
        tokens = generate_tokens(T, "cuda")
        engine.store(tokens, kv)
        got, mask = engine.retrieve(tokens)
        assert int(mask.sum()) == T and got[0][0].dtype == dt
        x4 = x.reshape(L, 2, T, H * D)
        want = _cat8([_formula(oracle, x4[:, :, i:i + 256], _engine_bins(oracle, L), dt) for i in range(0, T, 256)], 2)
        _same(_stack_kv(got).reshape(L, 2, T, H * D), want)
    finally:
        engine.close()


@pytest.mark.parametrize("dt", FP8, ids=IDS)
def test_huggingface_odd_head_size_through_the_engine(oracle, dt):
    """head_size 100 under the huggingface layout is not vector-readable: the codec stages the range into a vllm chunk
    (lmc_copy_kv, element path, 1-byte elements) before it encodes."""
    from lmcache_amd.cache_engine import LMCacheEngine
    g = torch.Generator().manual_seed(20)
    L, H, D, T = 2, 4, 100, 300
    x = _data("randn", (L, 2, T, H, D), dt, g)  # [L,2,T,H,D]
    xh = x.permute(0, 1, 3, 2, 4).contiguous()  # [L,2,H,T,D]
    kv = tuple((xh[l, 0].cuda(), xh[l, 1].cuda()) for l in range(L))
    tokens = generate_tokens(T, "cuda")
    engine = LMCacheEngine(make_cfg("cachegen-host"), dumb_metadata("huggingface", MODEL))
    try:
        engine.store(tokens, kv)
        got, mask = engine.retrieve(tokens)
        assert int(mask.sum()) == T and got[0][0].dtype == dt
        x4 = x.reshape(L, 2, T, H * D)
        want = _cat8([_formula(oracle, x4[:, :, i:i + 256], _engine_bins(oracle, L), dt) for i in range(0, T, 256)], 2)
        have = _stack_kv(got)  # [L,2,H,T,D]
        _same(have.view(torch.uint8).permute(0, 1, 3, 2, 4).contiguous().view(dt).reshape(L, 2, T, H * D), want)
    finally:
        engine.close()


@pytest.mark.parametrize("dt", FP8, ids=IDS)
def test_decode_layers_and_schedule_into_fp8(oracle, dt):
    """lmc_decode_chunks_layers and lmc_decode_chunks_schedule (blobs through a pointer table) into fp8 chunks."""
    g = torch.Generator().manual_seed(21)
    L, T, H, D = 4, 512, 2, 64
    x = _data("randn", (L, 2, T, H * D), dt, g)
    bins = _bins(L, g)
    xd = x.reshape(L, 2, T, H, D).cuda()
    blobs, dev, stride = _encode(native.KVLayout.from_chunk(xd, "vllm"), T, 256, bins, "fused")
    ctx = native.get_context(0)
    table = native.pointer_table([dev.data_ptr() + i * stride for i in range(len(blobs))], torch.device("cuda"))
    want = _cat8([_formula(oracle, x[:, :, i:i + 256], bins, dt) for i in range(0, T, 256)], 2)
    out = torch.zeros_like(xd)
    ctx.decode_chunks_layers(table.data_ptr(), stride, len(blobs), native.KVLayout.from_chunk(out, "vllm"), 0, 256, 1, 2)
    torch.cuda.synchronize()
    ctx.raise_on_status("decode layers")
    o = out.reshape(L, 2, T, H * D).cpu()
    _same(o[1:3], want[1:3])
    assert not o.view(torch.uint8)[0].any() and not o.view(torch.uint8)[3].any()  # layers outside the range: untouched
    out2 = torch.zeros_like(xd)
    ctx.decode_chunks_schedule(table.data_ptr(), stride, len(blobs), native.KVLayout.from_chunk(out2, "vllm"), 0, 256,
                               [1, 3, 4], None)
    torch.cuda.synchronize()
    ctx.raise_on_status("decode schedule")
    _same(out2.reshape(L, 2, T, H * D), want)
