"""CacheGenDeviceCodec (storage_backend/serde/cachegen_device.py) on the GPU: the Python sequencing between the kernels
and the engine -- store_pack -> finish_pack (the multi-part loop behind a store in pinned host DRAM) -> load_pack, stores
in flight, a pack that does not fit, decode_device and its kept pointer tables -- held against the CPU oracle byte for
byte and bit for bit.  There are no tolerances in this file.

The kernels themselves are pinned by test_gpu_parity.py / test_gpu_fp8.py and the C ABI's store / pack / load calls by
test_c_abi_store_load.py; what is checked here is that the codec hands them the right regions, sizes and bounds, at the
geometries where its own bookkeeping changes: a first plane range that ships nothing, unused parts, uneven ranges, a
job that is not split at all."""
import ctypes

import numpy as np
import pytest
import torch

from lmcache_amd import native
from lmcache_amd.storage_backend.serde import cachegen_device
from lmcache_amd.storage_backend.serde.cachegen_device import CacheGenDeviceCodec, PinnedArena
from tests.test_gpu_engine import MODEL, dumb_metadata, generate_tokens, make_cfg, oracle_roundtrip
from tests.test_gpu_fp8 import FP8, _bins, _data, _formula, _oracle_blob, _same

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def codec():
    """A codec of the tests' own (get_codec()'s is the engines'): the cases set pack_parts."""
    c = CacheGenDeviceCodec(0)
    c.shipped_pack_parts = c.pack_parts
    yield c
    c.close()


@pytest.fixture
def arena():
    a = PinnedArena()
    yield a
    a.close()


def _u16(t):
    """A 16-bit tensor's bits, on the host."""
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _make(L, T, H, D, dt, g):
    """KV [L, 2, T, H * D] on the host from the seeded generator g."""
    if dt in FP8:
        return _data("randn", (L, 2, T, H * D), dt, g)
    return torch.randn(L, 2, T, H * D, generator=g).to(dt)


def _oracle_blobs(oracle, x, cs, H, D, bins):
    """The oracle's blob of every chunk of x [L, 2, T, C] (fp8: the blob of the bf16 images, header word 23 set)."""
    out = []
    for t0 in range(0, x.shape[2], cs):
        part = x[:, :, t0:t0 + cs]
        if x.dtype in FP8:
            out.append(_oracle_blob(oracle, part, H, D, bins))
        else:
            bits, code = oracle.torch_to_bits(part.contiguous())
            out.append(oracle.encode_blob(bits, code, H, D, np.array(bins, np.int32)))
    return out


def _store(codec, lay, T, cs, bins, arena, path):
    """store_pack under `path`, then the part words the GPU wrote, read behind the last part's event and BEFORE
    finish_pack (which hands them back to their pool): -> (job, [(offset, bytes)] per part)."""
    codec.ctx.set_encode_path(path)
    try:
        job = codec.store_pack(lay, 0, T, cs, bins, arena)
    finally:
        codec.ctx.set_encode_path("auto")
    job.part_events[-1].synchronize()
    words = job.part_info.tensor.view(torch.int64)[:2 * len(job.part_events)].tolist()
    return job, list(zip(words[0::2], words[1::2]))


def _check_parts(parts, split):
    """A *split* case must have reached the multi-part loop (it fails rather than passing vacuously): at least two parts
    carry bytes.  "second part only" is the one split geometry where that cannot be -- two planes in two ranges, planes
    per part 0, 2: the loop shows in part 0 reading no bytes and part 1 carrying the pack's.  A *one part* case must not
    have been split: part 0 carries everything.  The parts that carry bytes are consecutive pieces of the streams region."""
    moved, nonempty = 0, []
    for r, (off, nb) in enumerate(parts):
        if nb > 0:
            assert off == moved, parts
            moved += nb
            nonempty.append(r)
    if split == "second part only":
        assert nonempty == [1], parts
    elif split:
        assert len(nonempty) >= 2, parts
    else:
        assert nonempty == [0], parts
    return moved


def _planes_per_part(pack_bytes, parts, L, n):
    """How many planes each part carried, from the finished pack's offset table (entry p * n is where plane p begins)."""
    h = native.PackHeader.from_buffer_copy(pack_bytes[:ctypes.sizeof(native.PackHeader)])
    table = np.frombuffer(pack_bytes, np.uint64, 2 * L * n + 1, h.off_table)
    begins = [int(table[p * n]) for p in range(2 * L)]
    return [sum(1 for b in begins if off <= b < off + nb) for off, nb in parts]


def _load(codec, pack, shape, dst_dt, cs, c0, m, lpr):
    L, T, H, D = shape
    out = torch.zeros(L, 2, T, H, D, dtype=dst_dt, device=DEV)
    job = codec.load_pack(pack, c0, m, native.KVLayout.from_chunk(out, "vllm"), c0 * cs, lpr)
    assert len(job.layer_events) == ((L + lpr - 1) // lpr if lpr else 1)
    codec.finish_decode(job)  # raises on a flagged status
    return out


def _check_load(codec, pack, shape, dst_dt, cs, refs, c0, m, lpr):
    """Chunks [c0, c0 + m) of the pack into a zeroed destination: the oracle's decode inside the run, zero outside."""
    L, T, H, D = shape
    got = _u16(_load(codec, pack, shape, dst_dt, cs, c0, m, lpr)).reshape(L, 2, T, H * D)
    for i, ref in enumerate(refs):
        sl = got[:, :, i * cs:min(T, (i + 1) * cs)]
        if c0 <= i < c0 + m:
            assert np.array_equal(sl, ref), f"chunk {i} of [{c0}, {c0 + m}), layers_per_range {lpr}"
        else:
            assert not sl.any(), f"chunk {i} is outside the run [{c0}, {c0 + m}) and must stay zero"


def _pack_case(oracle, codec, arena, name, x, H, D, cs, bins, path, split, lay=None):
    """store_pack -> finish_pack -> load_pack of x [L, 2, T, C] (host) against the oracle; every chunk is checked."""
    L, _, T, _ = x.shape
    n = (T + cs - 1) // cs
    if lay is None:
        xd = x.reshape(L, 2, T, H, D).to(DEV)
        lay = native.KVLayout.from_chunk(xd, "vllm")
    before = arena.total_allocated
    job, parts = _store(codec, lay, T, cs, bins, arena, path)
    moved = _check_parts(parts, split)
    pack = codec.finish_pack(job, arena)
    blobs = _oracle_blobs(oracle, x, cs, H, D, bins)
    assert len(blobs) == n == pack.nchunks
    have = ctypes.string_at(pack.blob.ptr, pack.blob.nbytes)
    print(f"\n[{name}] parts (offset, bytes): {parts}; planes per part: {_planes_per_part(have, parts, L, n)}")
    assert have == oracle.pack_from_blobs(blobs, cs)
    h = native.pack_info(pack.blob.ptr, pack.blob.nbytes)
    assert int(h.total_bytes) == pack.blob.nbytes == int(h.off_streams) + moved
    assert arena.total_allocated - before == native.r16(int(h.total_bytes))  # the bound-sized region was cut back
    for i in range(n):
        assert pack.extract(i) == blobs[i], f"chunk {i}"
    fp8 = x.dtype in FP8
    dst_dt = torch.bfloat16 if fp8 else x.dtype
    code = oracle.FP16 if dst_dt == torch.float16 else oracle.BF16
    refs = [oracle.decode_blob(b, code) for b in blobs]
    shape = (L, T, H, D)
    _check_load(codec, pack, shape, dst_dt, cs, refs, 0, n, 1)
    _check_load(codec, pack, shape, dst_dt, cs, refs, 0, n, None)
    _check_load(codec, pack, shape, dst_dt, cs, refs, 1, n - 2, 1)
    if fp8:  # and into a destination of the KV's own dtype: one cast of the fp32 dequantisation (test_gpu_fp8.py)
        got = _load(codec, pack, shape, x.dtype, cs, 0, n, None).reshape(L, 2, T, H * D).cpu()
        for i in range(n):
            _same(got[:, :, i * cs:(i + 1) * cs], _formula(oracle, x[:, :, i * cs:(i + 1) * cs], bins, x.dtype))
    return pack, blobs


# (L, H, D, chunks, chunk_tokens, pack_parts, dtype, path, split).  Planes per part as the GPU reported them (MI355X,
# printed by _pack_case from the part words and the finished pack's offset table):
#   L4_first_range_one_plane   0,1,1,1,1,1,1,2      L8_first_range_two_planes  1,2,2,2,2,2,2,3
#   L1_two_parts               0,2                  C256_two_planes_per_item   1,2,2,3
#   C384_six_items             0,1,1,1,1,2,-,-      sixteen_parts              0,1,1,2 and twelve unused
#   L7_uneven                  0,2,2,2,1,2,2,3      chunks_of_128_C512         0,1,1,2,1,1,1,3
#   fp16 / e4m3 / e5m2 / paged_NHBD on L = 4: as the first; e4m3 / e5m2 on C = 256: 1,2,2,3
#   auto_as_shipped_L4         0,1,1,1,1,1,1,2      production shape (L = 32)  7,8,8,8,8,8,8,9
CASES = {
    "L4_first_range_one_plane": (4, 8, 128, 16, 256, 8, torch.bfloat16, "fused", True),
    "L1_two_parts": (1, 8, 128, 16, 256, 2, torch.bfloat16, "fused", "second part only"),
    "C384_six_items": (3, 3, 128, 24, 256, 8, torch.bfloat16, "fused", True),
    "L7_uneven": (7, 8, 128, 10, 256, 8, torch.bfloat16, "fused", True),
    "L8_first_range_two_planes": (8, 8, 128, 8, 256, 8, torch.bfloat16, "fused", True),
    "C256_two_planes_per_item": (4, 2, 128, 16, 256, 8, torch.bfloat16, "fused", True),
    "sixteen_parts": (2, 8, 128, 64, 256, 16, torch.bfloat16, "fused", True),
    "chunks_of_128_C512": (5, 4, 128, 13, 128, 8, torch.bfloat16, "fused", True),
    "fp16": (4, 8, 128, 16, 256, 8, torch.float16, "fused", True),
    "e4m3": (4, 8, 128, 16, 256, 8, torch.float8_e4m3fn, "fused", True),
    "e5m2": (4, 8, 128, 16, 256, 8, torch.float8_e5m2, "fused", True),
    "e4m3_C256": (4, 2, 128, 16, 256, 8, torch.float8_e4m3fn, "fused", True),
    "e5m2_C256": (4, 2, 128, 16, 256, 8, torch.float8_e5m2, "fused", True),
    "auto_small_job": (32, 8, 128, 8, 256, 8, torch.bfloat16, "auto", False),  # 8 chunks x 64 items = 512 < 4 x CUs
}


@pytest.mark.parametrize("name", list(CASES))
def test_store_pack_finish_load_equal_the_oracle(oracle, codec, arena, name):
    L, H, D, n, cs, parts, dt, path, split = CASES[name]
    g = torch.Generator().manual_seed(1000 + list(CASES).index(name))
    x = _make(L, n * cs, H, D, dt, g)
    codec.pack_parts = parts
    _pack_case(oracle, codec, arena, name, x, H, D, cs, _bins(L, g), path, split)


def test_store_pack_from_a_paged_source(oracle, codec, arena):
    """KVLayout.paged, NHBD blocks of 16 tokens at random slots: the split store gathers through the slot mapping."""
    L, H, D, n, cs, bs = 4, 8, 128, 16, 256, 16
    T = n * cs
    g = torch.Generator().manual_seed(31)
    x = _make(L, T, H, D, torch.bfloat16, g)
    x5 = x.reshape(L, 2, T, H, D)
    nblocks = T // bs + 7
    slots = torch.randperm(nblocks * bs, generator=g)[:T]
    caches = []
    for l in range(L):
        c = torch.zeros((2, nblocks, H, bs, D), dtype=torch.bfloat16)
        for kvi in range(2):
            c[kvi, slots // bs, :, slots % bs] = x5[l, kvi]
        caches.append(c.to(DEV))
    lay = native.KVLayout.paged(caches, slots.to(DEV), bs, "NHBD")
    codec.pack_parts = 8
    _pack_case(oracle, codec, arena, "paged_NHBD", x, H, D, cs, _bins(L, g), "fused", True, lay=lay)


def test_a_ragged_store_is_one_part(oracle, codec, arena):
    """16 chunks and 100 tokens: a job with a ragged last chunk is not split (lmc_hip.h), whatever pack_parts says."""
    L, H, D, cs = 4, 8, 128, 256
    g = torch.Generator().manual_seed(32)
    x = _make(L, 16 * cs + 100, H, D, torch.bfloat16, g)
    codec.pack_parts = 8
    _pack_case(oracle, codec, arena, "ragged_tail", x, H, D, cs, _bins(L, g), "fused", False)


def _device_kv(L, T, H, D, seed):
    """A KV tuple on the device from a seeded device generator (the large shapes: 0.5 and 2 GiB)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    return tuple((torch.randn((T, H, D), generator=g, device=DEV).to(torch.bfloat16),
                  (torch.rand((T, H, D), generator=g, device=DEV) * 3 - 1).to(torch.bfloat16)) for _ in range(L))


def _host_chunk(kv, i, cs):
    """Chunk i of a KV tuple as [L, 2, cs, C] on the host."""
    return torch.stack([torch.stack((k[i * cs:(i + 1) * cs], v[i * cs:(i + 1) * cs])) for k, v in kv]).flatten(3).cpu()


def test_auto_as_shipped_four_layers_128_chunks(oracle, codec, arena):
    """Nothing forced: path `auto`, pack_parts as shipped, L = 4, H = 8, D = 128, 128 chunks of 256 tokens (512 MiB).
    Eight plane ranges of one plane each: part 0 legitimately ships nothing.  Every chunk against the oracle."""
    L, H, D, n, cs = 4, 8, 128, 128, 256
    kv = _device_kv(L, n * cs, H, D, 33)
    x = torch.cat([_host_chunk(kv, i, cs) for i in range(n)], 2)
    g = torch.Generator().manual_seed(33)
    codec.pack_parts = codec.shipped_pack_parts
    assert codec.pack_parts == 8
    _pack_case(oracle, codec, arena, "auto_as_shipped_L4", x, H, D, cs, _bins(L, g), "auto", True,
               lay=native.KVLayout.from_kv_tuple(kv, "vllm"))


def test_production_shape_ships_in_eight_parts(oracle, codec):
    """32 layers x 16384 tokens x 8 x 128 bf16 (2 GiB, 64 chunks) through store_pack on path `auto`: 8 non-empty parts;
    chunks 0, 1, n/2, n-1 byte-equal to the oracle's blobs; every chunk extractable, and the pack's decode equal to
    lmc_decode_chunks of the extracted blobs (GPU against GPU for the rest: the sampled chunks pin both to the oracle)."""
    from lmcache_amd.storage_backend.serde.cachegen_basics import CacheGenConfig
    L, H, D, n, cs = 32, 8, 128, 64, 256
    T = n * cs
    bins = CacheGenConfig.from_model_name("meta-llama/Llama-3.1-8B-Instruct").plane_bins(L)
    kv = _device_kv(L, T, H, D, 34)
    arena = PinnedArena()
    try:
        codec.pack_parts = codec.shipped_pack_parts
        before = arena.total_allocated
        job, parts = _store(codec, native.KVLayout.from_kv_tuple(kv, "vllm"), T, cs, bins, arena, "auto")
        assert len(parts) == 8 and all(nb > 0 for _, nb in parts), parts
        moved = _check_parts(parts, True)
        pack = codec.finish_pack(job, arena)
        h = native.pack_info(pack.blob.ptr, pack.blob.nbytes)
        assert int(h.total_bytes) == pack.blob.nbytes == int(h.off_streams) + moved
        assert arena.total_allocated - before == native.r16(pack.blob.nbytes)
        have = ctypes.string_at(pack.blob.ptr, pack.blob.nbytes)
        print(f"\n[production] parts (offset, bytes): {parts}; planes per part: {_planes_per_part(have, parts, L, n)}")
        del have
        stride = native.r16(native.blob_bound(L, cs, H, D))
        dev = torch.zeros(n * stride, dtype=torch.uint8, device=DEV)
        refs = {}
        for i in range(n):
            blob = pack.extract(i)
            assert 0 < len(blob) <= stride
            dev[i * stride:i * stride + len(blob)].copy_(torch.frombuffer(bytearray(blob), dtype=torch.uint8))
            if i in (0, 1, n // 2, n - 1):
                want = _oracle_blobs(oracle, _host_chunk(kv, i, cs), cs, H, D, bins)[0]
                assert blob == want, f"chunk {i}"
                refs[i] = oracle.decode_blob(want, oracle.BF16)
        out = _load(codec, pack, (L, T, H, D), torch.bfloat16, cs, 0, n, 4)
        del kv
        out2 = torch.zeros_like(out)
        codec.ctx.decode_chunks(dev.data_ptr(), stride, n, native.KVLayout.from_chunk(out2, "vllm"), 0, cs)
        torch.cuda.synchronize()
        codec.ctx.raise_on_status("decode of the extracted blobs")
        assert torch.equal(out.view(torch.int16), out2.view(torch.int16))
        for i, ref in refs.items():
            assert np.array_equal(_u16(out[:, :, i * cs:(i + 1) * cs]).reshape(L, 2, cs, H * D), ref), f"chunk {i}"
    finally:
        arena.close()


# ---- b. stores in flight -------------------------------------------------------------------------------------------
def test_two_stores_in_flight_and_the_shared_region_reused(oracle, codec, arena):
    L, H, D, n, cs = 4, 8, 128, 16, 256
    T = n * cs
    g = torch.Generator().manual_seed(41)
    bins = _bins(L, g)
    xs = [_make(L, T, H, D, torch.bfloat16, g) for _ in range(4)]
    want = [oracle.pack_from_blobs(_oracle_blobs(oracle, x, cs, H, D, bins), cs) for x in xs]
    xd = [x.reshape(L, 2, T, H, D).to(DEV) for x in xs]
    codec.pack_parts = 8
    codec.ctx.set_encode_path("fused")
    try:
        # two stores before either is finished: the second must not build its pack where the first one's still lies
        j0 = codec.store_pack(native.KVLayout.from_chunk(xd[0], "vllm"), 0, T, cs, bins, arena)
        j1 = codec.store_pack(native.KVLayout.from_chunk(xd[1], "vllm"), 0, T, cs, bins, arena)
        assert j0.dev is codec._pack_dev and j1.dev is not j0.dev and j1.dev.data_ptr() != j0.dev.data_ptr()
        assert j0.sizes is not j1.sizes and j0.status_idx != j1.status_idx and j0.part_info is not j1.part_info
        p1 = codec.finish_pack(j1, arena)  # finished in reverse order
        p0 = codec.finish_pack(j0, arena)
        assert p1.blob.tobytes() == want[1]
        assert p0.blob.tobytes() == want[0]
        # store / finish / store / finish: both on the shared region, one behind the other
        j2 = codec.store_pack(native.KVLayout.from_chunk(xd[2], "vllm"), 0, T, cs, bins, arena)
        assert j2.dev is codec._pack_dev
        p2 = codec.finish_pack(j2, arena)
        first = p2.blob.tobytes()
        assert first == want[2]
        j3 = codec.store_pack(native.KVLayout.from_chunk(xd[3], "vllm"), 0, T, cs, bins, arena)
        assert j3.dev is codec._pack_dev and j3.dev is j2.dev
        p3 = codec.finish_pack(j3, arena)
    finally:
        codec.ctx.set_encode_path("auto")
    assert p3.blob.tobytes() == want[3]
    assert p2.blob.tobytes() == first and p1.blob.tobytes() == want[1] and p0.blob.tobytes() == want[0]


def test_a_store_dropped_unfinished_gives_the_shared_region_back(oracle, codec, arena):
    """A PackJob nobody finishes (an exception between store_pack and finish_pack) must not leave the codec's shared HBM
    region taken for good: the next store builds its pack there again, and it is the oracle's."""
    import gc
    L, H, D, n, cs = 8, 8, 128, 8, 256  # (a geometry whose part 0 ships: this test is about the region alone)
    T = n * cs
    g = torch.Generator().manual_seed(43)
    bins = _bins(L, g)
    x = _make(L, T, H, D, torch.bfloat16, g)
    lay = native.KVLayout.from_chunk(x.reshape(L, 2, T, H, D).to(DEV), "vllm")
    codec.pack_parts = 8
    job, _ = _store(codec, lay, T, cs, bins, arena, "fused")
    if job.dev is not codec._pack_dev:  # (whatever an earlier test left: from a finished store on the shared region)
        codec.finish_pack(job, arena)
        job, _ = _store(codec, lay, T, cs, bins, arena, "fused")
    assert job.dev is codec._pack_dev
    del job
    gc.collect()
    job, _ = _store(codec, lay, T, cs, bins, arena, "fused")
    assert job.dev is codec._pack_dev
    assert codec.finish_pack(job, arena).blob.tobytes() == oracle.pack_from_blobs(_oracle_blobs(oracle, x, cs, H, D, bins), cs)


# ---- c. a pack that does not fit -----------------------------------------------------------------------------------
def test_a_pack_that_does_not_fit_is_an_error_and_costs_one_granule(oracle, codec, arena, monkeypatch):
    L, H, D, n, cs = 4, 8, 128, 16, 256
    T = n * cs
    g = torch.Generator().manual_seed(42)
    bins = _bins(L, g)
    x = _make(L, T, H, D, torch.bfloat16, g)
    want = oracle.pack_from_blobs(_oracle_blobs(oracle, x, cs, H, D, bins), cs)
    lay = native.KVLayout.from_chunk(x.reshape(L, 2, T, H, D).to(DEV), "vllm")
    codec.pack_parts = 8
    job, _ = _store(codec, lay, T, cs, bins, arena, "fused")
    good = codec.finish_pack(job, arena)
    total = good.blob.nbytes
    assert good.blob.tobytes() == want and total == len(want)
    before = arena.total_allocated
    with monkeypatch.context() as m:
        m.setattr(cachegen_device, "pack_cap", lambda *a, **k: total - 16)
        job, parts = _store(codec, lay, T, cs, bins, arena, "fused")
        assert job.cap == total - 16
        with pytest.raises(native.NativeError, match="host arena full"):
            codec.finish_pack(job, arena)
    # the bound-sized region went back but for the one granule PinnedArena.shrink(region, 0) keeps
    assert arena.total_allocated == before + 16
    job, _ = _store(codec, lay, T, cs, bins, arena, "fused")
    again = codec.finish_pack(job, arena)
    assert again.blob.tobytes() == want
    assert good.blob.tobytes() == want  # (and the failed store wrote over nobody)


# ---- d. the same through the engine --------------------------------------------------------------------------------
@pytest.mark.parametrize("blocking", [True, False], ids=["blocking", "nonblocking"])
def test_engine_store_of_four_layers_32k_tokens(oracle, blocking):
    """LMCacheEngine on the pinned CacheGen tier, L = 4, H = 8, D = 128, T = 32768, nothing forced: the store's first
    plane range is a single plane.  The store must not be lost, blocking or not."""
    import time
    from lmcache_amd.cache_engine import LMCacheEngine
    L, H, D, T, cs = 4, 8, 128, 32768, 256
    n = T // cs
    kv = _device_kv(L, T, H, D, 51)
    tokens = generate_tokens(T, "cuda")
    engine = LMCacheEngine(make_cfg("cachegen-host"), dumb_metadata("vllm", MODEL))
    try:
        engine.store(tokens, kv, blocking=blocking)
        got, mask = engine.retrieve(tokens)
        if not blocking:
            for _ in range(500):
                if int(mask.sum()) == T:
                    break
                time.sleep(0.01)
                got, mask = engine.retrieve(tokens)
        assert int(mask.sum()) == T
        for i in (0, 1, n // 2, n - 1):
            part = tuple((k[i * cs:(i + 1) * cs], v[i * cs:(i + 1) * cs]) for k, v in kv)
            want = oracle_roundtrip(oracle, part, "vllm", MODEL, torch.bfloat16)
            have = torch.stack([torch.stack((k[i * cs:(i + 1) * cs], v[i * cs:(i + 1) * cs])) for k, v in got]).cpu()
            assert torch.equal(have.view(torch.int16), want.view(torch.int16)), f"chunk {i}"
    finally:
        engine.close()


# ---- e. decode_device and its kept tables --------------------------------------------------------------------------
def _two_blobs(oracle, L, H, D, T, bins, seed):
    """Two chunks of one geometry whose blobs differ clearly in size: randn data, and constant / sparse channels
    (as test_counts_model_constant_and_sparse_channels builds them).  -> [(blob, decoded bits [L, 2, T, C])] small, large."""
    g = torch.Generator().manual_seed(seed)
    big = torch.randn(L, 2, T, H, D, generator=g)
    small = torch.zeros(L, 2, T, H, D)
    small[..., 0, 0] = 1.0                    # the row maximum: every other channel is the middle symbol ...
    small[:, :, 100, 0, 8:16] = -1.0          # ... but for one outlier token in eight channels
    small[:, :, ::2, H - 1, 5] = 0.5          # and a two-symbol channel
    out = []
    for x in (small, big):
        bits, code = oracle.torch_to_bits(x.to(torch.bfloat16).reshape(L, 2, T, H * D))
        blob = oracle.encode_blob(bits, code, H, D, np.array(bins, np.int32))
        out.append((blob, oracle.decode_blob(blob, oracle.BF16)))
    assert native.r16(len(out[0][0])) + 4096 < len(out[1][0])
    return out


def _put(dev, off, blob):
    dev[off:off + len(blob)].copy_(torch.frombuffer(bytearray(blob), dtype=torch.uint8))
    return dev[off:off + len(blob)]


@pytest.fixture
def schedule_spy(codec, monkeypatch):
    """Records (blob_ptrs, max_blob_bytes) of every lmc_decode_chunks_schedule call the codec makes."""
    calls = []
    real = codec.ctx.decode_chunks_schedule

    def spy(blob_ptrs, max_blob_bytes, *a, **k):
        calls.append((blob_ptrs, max_blob_bytes))
        return real(blob_ptrs, max_blob_bytes, *a, **k)

    monkeypatch.setattr(codec.ctx, "decode_chunks_schedule", spy)
    return calls


def test_decode_device_bound_follows_the_blobs_not_their_address(oracle, codec, schedule_spy):
    """Blobs of another size at an address the codec has seen (an HBM tier closed and reopened): the bound k_decode holds
    the headers against is this call's largest blob.  Too small a bound is a standing false miss (bad blob header), too
    large a bound a header check looser than the blob."""
    L, H, D, T = 2, 3, 128, 256
    (small, small_ref), (large, large_ref) = _two_blobs(oracle, L, H, D, T, [32, 16, 16, 32], 61)
    dev = torch.zeros(native.r16(len(large)) + 64, dtype=torch.uint8, device=DEV)

    def step(blob, ref, same):
        blobs = [_put(dev, 0, blob)]
        out = torch.zeros(L, 2, T, H, D, dtype=torch.bfloat16, device=DEV)
        before = len(schedule_spy)
        job = codec.decode_device(blobs, native.KVLayout.from_chunk(out, "vllm"), 0, T,
                                  same_blobs_as=[blobs[0]] if same else None)
        codec.finish_decode(job)  # no NativeError
        assert len(schedule_spy) == before + 1
        assert schedule_spy[-1][1] == max(b.numel() for b in blobs) == len(blob)
        assert job._table.data_ptr() == schedule_spy[-1][0]
        assert np.array_equal(_u16(out).reshape(L, 2, T, H * D), ref)

    for same in (False, True):
        step(small, small_ref, same)
        step(large, large_ref, same)   # small then large at the same address
        step(small, small_ref, same)   # large then small


def test_decode_device_more_blob_sets_than_kept_tables(oracle, codec, schedule_spy):
    """Ten blob sets (eight tables are kept), then the first and the last again on a second stream; the caller's list
    handed over as same_blobs_as for half of them.  A DecodeJob keeps the table its kernels read."""
    L, H, D, T = 2, 3, 128, 256
    pair = _two_blobs(oracle, L, H, D, T, [32, 16, 16, 32], 62)
    slot = native.r16(len(pair[1][0])) + 256
    dev = torch.zeros(11 * slot, dtype=torch.uint8, device=DEV)
    views = [_put(dev, k * slot, pair[k % 2][0]) for k in range(11)]
    sets = [[views[k], views[k + 1]] for k in range(10)]  # set k: chunks of kind k % 2, (k + 1) % 2

    def run(k, same):
        out = torch.zeros(L, 2, 2 * T, H, D, dtype=torch.bfloat16, device=DEV)
        torch.cuda.current_stream().wait_stream(torch.cuda.default_stream())  # (the zeroing and the uploads)
        job = codec.decode_device(sets[k], native.KVLayout.from_chunk(out, "vllm"), 0, T, same_blobs_as=sets[k] if same else None)
        assert job._table.data_ptr() == schedule_spy[-1][0] and job._table.numel() == 2 and job._table.is_cuda
        assert job._table.cpu().tolist() == [b.data_ptr() for b in sets[k]]
        assert schedule_spy[-1][1] == max(b.numel() for b in sets[k])
        codec.finish_decode(job)
        got = _u16(out).reshape(L, 2, 2 * T, H * D)
        torch.cuda.current_stream().synchronize()
        assert np.array_equal(got[:, :, :T], pair[k % 2][1]) and np.array_equal(got[:, :, T:], pair[(k + 1) % 2][1]), k

    for k in range(10):
        run(k, same=bool(k & 1))
    assert len(codec._table_cache) <= 8 and len(codec._same_blobs) <= 8
    s2 = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s2):
        run(0, same=False)   # its table has been dropped since: built again
        run(9, same=True)    # kept, and uploaded on another stream: ordered behind that copy
        run(9, same=True)


def test_decode_device_layer_events_cover_the_layers_below(oracle, codec):
    """layers_per_launch = (1, 2) on four layers: launches of layers 0-1, 1-3, 3-4.  After waiting for ONE entry of
    layer_events (nothing else: the read goes over a stream of its own) the layers below its first value are complete."""
    L, H, D, T = 4, 3, 128, 256
    bins = [32, 16, 23, 16, 16, 32, 23, 32]
    (_, _), (blob, ref) = _two_blobs(oracle, L, H, D, T, bins, 63)
    dev = torch.zeros(native.r16(len(blob)), dtype=torch.uint8, device=DEV)
    blobs = [_put(dev, 0, blob)]
    out = torch.zeros(L, 2, T, H, D, dtype=torch.bfloat16, device=DEV)
    work, reader = torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)
    work.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(work):
        job = codec.decode_device(blobs, native.KVLayout.from_chunk(out, "vllm"), 0, T, layers_per_launch=(1, 2))
    assert [end for end, _ in job.layer_events] == [1, 3, 4]
    for end, ev in job.layer_events:
        ev.synchronize()
        with torch.cuda.stream(reader):
            got = out[:end].to("cpu", non_blocking=False)
        assert np.array_equal(_u16(got).reshape(end, 2, T, H * D), ref[:end]), f"layers below {end}"
    codec.finish_decode(job)
    assert np.array_equal(_u16(out).reshape(L, 2, T, H * D), ref)


# ---- f. a launch that fails half way, and close() ------------------------------------------------------------------
def _words_out(codec):
    """What a job in flight holds of the codec's: free status words, and the buffers lying in each pool of pinned words."""
    return len(codec._status._free), len(codec._size_pool), len(codec._meta_pool), len(codec._part_info_pool)


def _boom(*a, **k):
    raise RuntimeError("the launch failed half way")


def _small_chunk(seed, L=4, H=8, D=128, n=2, cs=256):
    g = torch.Generator().manual_seed(seed)
    x = _make(L, n * cs, H, D, torch.bfloat16, g).reshape(L, 2, n * cs, H, D).to(DEV)
    return x, native.KVLayout.from_chunk(x, "vllm"), _bins(L, g), n * cs, cs


def test_a_store_pack_that_fails_half_way_gives_its_words_back(codec, arena, monkeypatch):
    x, lay, bins, T, cs = _small_chunk(71)
    want = codec.finish_pack(codec.store_pack(lay, 0, T, cs, bins, arena), arena).blob.tobytes()  # (and the pools are filled)
    before = _words_out(codec)
    with monkeypatch.context() as m:
        m.setattr(codec.ctx, "store_pack_parts", _boom)
        with pytest.raises(RuntimeError, match="failed half way"):
            codec.store_pack(lay, 0, T, cs, bins, arena)
    assert _words_out(codec) == before
    job = codec.store_pack(lay, 0, T, cs, bins, arena)
    assert _words_out(codec) == (before[0] - 1, before[1] - 1, before[2], before[3] - 1)
    assert codec.finish_pack(job, arena).blob.tobytes() == want
    assert _words_out(codec) == before


def test_a_layerwise_load_that_fails_half_way_gives_its_words_back(codec, arena, monkeypatch):
    x, lay, bins, T, cs = _small_chunk(72)
    blobs, ev = codec.offload(codec.encode(lay, 0, T, cs, bins), None, arena)
    ev.synchronize()

    def load():
        out = torch.zeros_like(x)
        job = codec.decode_host_layerwise(blobs, native.KVLayout.from_chunk(out, "vllm"), 0, cs, 2)
        return out, job

    want, job = load()
    codec.finish_decode(job)  # (and the pools are filled)
    before = _words_out(codec)
    with monkeypatch.context() as m:
        m.setattr(codec.ctx, "load_chunks", _boom)
        with pytest.raises(RuntimeError, match="failed half way"):
            load()
    assert _words_out(codec) == before
    got, job = load()
    assert _words_out(codec) == (before[0] - 1, before[1], before[2] - 1, before[3])
    codec.finish_decode(job)
    assert _words_out(codec) == before and torch.equal(got.view(torch.int16), want.view(torch.int16))


def test_close_frees_every_pinned_buffer_of_the_codec(monkeypatch):
    """A codec of this test's own through every path that borrows pinned memory -- size words (encode, store_pack), part
    words (store_pack), pointer / size arrays (decode_host_layerwise), staging of pageable blobs (decode), the status
    words' block -- then close(): every native.PinnedBuffer made on the way has been freed.  A second close() is a no-op."""
    arena = PinnedArena(slab_bytes=64 << 20)
    arena.reserve(1)  # the arena's slab is allocated before PinnedBuffer is wrapped: only the codec's buffers are counted
    made = []

    class Counted(native.PinnedBuffer):
        def __init__(self, nbytes):
            super().__init__(nbytes)
            made.append(self)

    monkeypatch.setattr(native, "PinnedBuffer", Counted)
    c = CacheGenDeviceCodec(0)
    try:
        x, lay, bins, T, cs = _small_chunk(73)
        blobs, ev = c.offload(c.encode(lay, 0, T, cs, bins), None, arena)
        ev.synchronize()
        pack = c.finish_pack(c.store_pack(lay, 0, T, cs, bins, arena), arena)
        outs = [torch.zeros_like(x) for _ in range(3)]
        dst = [native.KVLayout.from_chunk(o, "vllm") for o in outs]
        c.finish_decode(c.decode_host_layerwise(blobs, dst[0], 0, cs, 2))
        c.finish_decode(c.decode([hb.tobytes() for hb in blobs], dst[1], 0, cs))
        c.finish_decode(c.load_pack(pack, 0, 0, dst[2], 0, None))
        assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))
        assert torch.equal(outs[0].view(torch.int16), outs[2].view(torch.int16))
        assert len(made) >= 5 and all(b.ptr for b in made)
        assert c._stage is not None and c._pack_dev is not None
    finally:
        c.close()
        arena_slabs = len(arena._slabs) + len(arena._spare)
        arena.close()
    assert arena_slabs == 1  # (nothing of the arena's is in `made`)
    assert all(b.ptr == 0 for b in made), [b.nbytes for b in made if b.ptr]
    assert c._stage is None and c._pack_dev is None and not c._table_cache and not c._same_blobs
    c.close()
