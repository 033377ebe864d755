"""The layer-by-layer store of the fixed-width model: lmc_encode_layers_begin_fixed (csrc/k_fixed.h: the sliced per-layer
launches of k_fixed_encode with their partial check sums, k_fixed_layers_finish), lmc_ctx_set_fixed_layer_slices,
CacheGenDeviceCodec.encode_layers_fixed, LMCLocalBackend.begin_put_kv_layers behind LMCACHE_AMD_FIXED_LAYERWISE=1 and
LMCacheEngine.store_paged_layerwise on the "cachegen-fixed" tier.

Nothing here has a tolerance: a blob whose encode was issued per layer, in however many slices, is byte for byte the blob
of the one-piece encode of the same source and tests/fixed_model.py's blob of the gathered chunk.

Geometries (the smallest that reach every branch; per-plane bins mix narrow (<= 17) and wide planes):
  A  L=3 H=2 D=64   C=128  G=2   <16,1>  chunk 32,  3*32+7 tokens   one pass: forced S = 2 or 4 clips to 1; a one-oct tail
  B  L=2 H=8 D=128  C=1024 G=16  <64,2>  chunk 256, 256+70 tokens   four passes; the tail has 9 octs: a second pass with
                                                                    one live oct, the last two slices of S = 4 empty
  C  L=2 H=3 D=80   C=240  G=4   <32,1>  chunk 200, 2*200+1 tokens  25 octs make two passes, a partial last group; a
                                                                    1-token last chunk"""
import numpy as np
import pytest
import torch

from lmcache_amd import native
from lmcache_amd.cache_engine import LMCacheEngine
from lmcache_amd.config import LMCacheEngineConfig
from lmcache_amd.storage_backend.local_backend import _DevChunk, _PackChunk
from tests import fixed_model as fm
from tests.test_gpu_engine import dumb_metadata, generate_tokens
from tests.test_gpu_layerwise_store import _as_arg, _empty_caches, _fill_layer, _layout_name, _poison
from tests.test_gpu_paged_split import _ibits, _mapping

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BS = 16
BF16, FP16 = torch.bfloat16, torch.float16
NAMES = {BF16: "bf16", FP16: "fp16"}
INVALID = -1
POISON = 0xA5
#        L  H  D    chunk tokens
GEOMS = {"A": (3, 2, 64, 32, 3 * 32 + 7),
         "B": (2, 8, 128, 256, 256 + 70),
         "C": (2, 3, 80, 200, 2 * 200 + 1)}
BIN_CYCLE = [32, 16, 12, 20, 17, 24]
SOURCES = ["NBHD", "NHBD", "NHDB", "NHDB-pair"]
MAPPINGS = ["blocks", "random"]
SLICES = [0, 1, 2, 4]  # 0: the library's own rule


def _thinned():
    """Every (geometry, source), every (geometry, slices), every (source, mapping), both dtypes per geometry -- not the
    whole product: 8 cases a geometry, each with all four slice counts in one test (they share the references)."""
    out = []
    for gn in GEOMS:
        for i, src in enumerate(SOURCES):
            for j, m in enumerate(MAPPINGS):
                out.append((gn, src, m, (BF16, FP16)[(i + j + ord(gn)) % 2]))
    return out


CASES = _thinned()


def _bins(L):
    return [BIN_CYCLE[p % len(BIN_CYCLE)] for p in range(2 * L)]


@pytest.fixture(scope="module")
def ctx():
    native.build()
    c = native.get_context(0)
    yield c
    c.set_fixed_layer_slices(0)


@pytest.fixture(scope="module")
def oracle():
    from oracle import lmc_oracle
    lmc_oracle.build()
    return lmc_oracle


def _kv(gn, dt, seed=0):
    """[L, 2, ntok, H, D] of dt (CPU): randn with an all-zero token, a token with an inf and one with a NaN per plane."""
    L, H, D, cs, ntok = GEOMS[gn]
    g = torch.Generator().manual_seed(1000 + 7 * ord(gn) + seed)
    x = torch.randn((L, 2, ntok, H, D), generator=g).to(torch.bfloat16)
    x[:, :, 9] = 0
    x[:, :, 21, 0, 3] = float("inf")
    x[:, :, ntok - 2, H - 1, D - 2] = float("nan")
    return x.to(dt)


_MODEL = {}


def _model_blobs(oracle, gn, dt, seed=0):
    """tests/fixed_model.py's blob of every gathered chunk, computed once per (geometry, dtype) and shared."""
    key = (gn, dt, seed)
    if key not in _MODEL:
        L, H, D, cs, ntok = GEOMS[gn]
        x, out = _kv(gn, dt, seed), []
        for t0 in range(0, ntok, cs):
            part = x[:, :, t0:t0 + cs].reshape(L, 2, -1, H * D)
            bits, code = oracle.torch_to_bits(part.contiguous())
            out.append(fm.encode_blob(oracle, bits, code, H, D, np.array(_bins(L), np.int32)))
        _MODEL[key] = out
    return _MODEL[key]


def _source(gn, source, mapping, dt, seed=0, fill=True):
    L, H, D, cs, ntok = GEOMS[gn]
    nb = (ntok + BS - 1) // BS + 3
    g = torch.Generator().manual_seed(5 + SOURCES.index(source) + 10 * MAPPINGS.index(mapping))
    slots = _mapping(mapping, ntok, nb, BS, g).to(DEV)
    x = _kv(gn, dt, seed).to(DEV)
    caches = _empty_caches(source, L, H, D, dt, nb)
    if fill:
        for l in range(L):
            _fill_layer(source, caches, l, x[l], slots)
    else:
        for c in caches:
            _poison(c)
    return x, caches, slots


class _Arena:
    """Blob arena (0xA5 everywhere), size words and a status word of one C-ABI encode job."""

    def __init__(self, gn, fill=0x5A5A5A5A):
        L, H, D, cs, ntok = GEOMS[gn]
        self.n = (ntok + cs - 1) // cs
        self.stride = native.r16(native.blob_bound(L, cs, H, D))
        self.blobs = torch.full((self.n * self.stride,), POISON, dtype=torch.uint8, device=DEV)
        self.sizes = torch.full((self.n,), fill, dtype=torch.int32, device=DEV)
        self.status = torch.zeros(1, dtype=torch.int32, device=DEV)

    def args(self, gn):
        L, H, D, cs, ntok = GEOMS[gn]
        return (0, ntok, cs, _bins(L), self.blobs.data_ptr(), self.stride, self.sizes.data_ptr())

    def read(self):
        """-> (sizes, blob bytes [0, size) per chunk); the bytes of [size, stride) must still be the fill."""
        torch.cuda.synchronize()
        sz, host = self.sizes.cpu().tolist(), self.blobs.cpu().numpy()
        for i in range(self.n):
            assert 0 < sz[i] <= self.stride
            assert (host[i * self.stride + sz[i]:(i + 1) * self.stride] == POISON).all(), f"chunk {i}: bytes behind the blob were written"
        return sz, [host[i * self.stride:i * self.stride + sz[i]].tobytes() for i in range(self.n)]


def _want_sizes(gn):
    L, H, D, cs, ntok = GEOMS[gn]
    return [native.fixed_blob_bytes(L, min(cs, ntok - t0), H, D, _bins(L)) for t0 in range(0, ntok, cs)]


def _one_piece(ctx, layout, gn):
    a = _Arena(gn)
    ctx.encode_chunks_fixed_split(layout, *a.args(gn), status_ptr=a.status.data_ptr())
    out = a.read()
    assert int(a.status[0]) == 0
    return out


def _begin(ctx, layout, gn, a):
    h = ctx.encode_layers_begin_fixed(layout, *a.args(gn), status_ptr=a.status.data_ptr())
    assert h is not None, "these geometries are eligible"
    return h


def _run_job(h, L, stream):
    for l in range(L):
        h.encode_layer(l, stream)
    h.finish(stream)


# ------------------------------------------------------------------ 1. per-layer reading and byte equality
@pytest.mark.parametrize("gn,source,mapping,dt", CASES, ids=["%s-%s-%s-%s" % (g, s, m, NAMES[d]) for g, s, m, d in CASES])
def test_layers_are_read_when_they_are_encoded_and_the_blobs_equal_the_one_piece_and_the_model(ctx, oracle, gn, source, mapping, dt):
    L, H, D, cs, ntok = GEOMS[gn]
    _, full, slots = _source(gn, source, mapping, dt)
    sz1, blobs1 = _one_piece(ctx, native.KVLayout.paged(_as_arg(source, full), slots, BS, _layout_name(source)), gn)
    want = _model_blobs(oracle, gn, dt)
    assert sz1 == _want_sizes(gn) == [len(b) for b in want]
    for i in range(len(want)):
        assert blobs1[i] == want[i], f"chunk {i}: one piece vs model"
    for S in SLICES:
        ctx.set_fixed_layer_slices(S)
        x, caches, slots2 = _source(gn, source, mapping, dt, fill=False)  # every layer NaN
        assert torch.equal(slots, slots2)
        layout = native.KVLayout.paged(_as_arg(source, caches), slots, BS, _layout_name(source))
        a = _Arena(gn)
        h = _begin(ctx, layout, gn, a)
        cur = torch.cuda.current_stream()
        side = torch.cuda.Stream(device=DEV)
        for l in range(L):
            _fill_layer(source, caches, l, x[l], slots)
            ready = torch.cuda.Event()
            ready.record(cur)
            side.wait_event(ready)
            h.encode_layer(l, side.cuda_stream)
            ev = torch.cuda.Event()
            ev.record(side)
            cur.wait_event(ev)  # behind it the layer has been read
            _poison(caches[l])
        side.synchronize()
        assert a.sizes.cpu().tolist() == [0] * a.n, "a size word stays 0 until the finish launch"
        h.finish(side.cuda_stream)
        sz, blobs = a.read()
        assert int(a.status[0]) == 0
        assert sz == sz1, f"S={S}"
        for i in range(a.n):
            assert blobs[i] == blobs1[i], f"S={S} chunk {i}: layer-wise vs one piece"
            native.blob_info(blobs[i])
    ctx.set_fixed_layer_slices(0)


# ------------------------------------------------------------------ 2. lifecycle
def test_out_of_order_calls_are_refused_and_the_job_still_finishes_and_abort_frees_the_buffers(ctx, oracle):
    gn, dt = "B", BF16
    L, H, D, cs, ntok = GEOMS[gn]
    x, caches, slots = _source(gn, "NBHD", "blocks", dt)
    layout = native.KVLayout.paged(caches, slots, BS, "NBHD")
    want = _model_blobs(oracle, gn, dt)
    PAT = 0x5A5A5A5A
    ctx.set_fixed_layer_slices(2)
    a = _Arena(gn, fill=PAT)
    st = torch.cuda.current_stream().cuda_stream
    h = _begin(ctx, layout, gn, a)
    assert h.encode_layer_rc(1, st) == INVALID, "layer 1 before layer 0"
    assert h.finish_rc(st) == INVALID, "finish before any layer"
    torch.cuda.synchronize()
    assert a.sizes.cpu().tolist() == [PAT] * a.n and bool((a.blobs == POISON).all()), "a refused call queues nothing"
    h.encode_layer(0, st)
    assert h.encode_layer_rc(0, st) == INVALID, "a layer given twice"
    assert h.encode_layer_rc(L, st) == INVALID, "layer index L"
    assert h.finish_rc(st) == INVALID, "finish after L - 1 layers"
    torch.cuda.synchronize()
    assert a.sizes.cpu().tolist() == [0] * a.n, "no size word before the finish launch"
    h.encode_layer(1, st)
    h.finish(st)
    sz, blobs = a.read()
    assert int(a.status[0]) == 0 and blobs == want, "the job finishes correctly after the refusals"
    # abort after two layers of three, then a new job on the same buffers
    gn = "A"
    L, H, D, cs, ntok = GEOMS[gn]
    x, caches, slots = _source(gn, "NHDB", "random", dt)
    layout = native.KVLayout.paged(caches, slots, BS, "NHDB")
    a = _Arena(gn)
    h = _begin(ctx, layout, gn, a)
    h.encode_layer(0, st)
    h.encode_layer(1, st)
    h.abort()
    torch.cuda.synchronize()
    assert a.sizes.cpu().tolist() == [0] * a.n and int(a.status[0]) == 0
    a = _Arena(gn)
    h = _begin(ctx, layout, gn, a)
    _run_job(h, L, st)
    sz, blobs = a.read()
    assert int(a.status[0]) == 0 and blobs == _model_blobs(oracle, gn, dt)
    ctx.set_fixed_layer_slices(0)


def test_two_jobs_interleaved_layer_by_layer_on_two_streams(ctx, oracle):
    gn, dt = "C", FP16
    L, H, D, cs, ntok = GEOMS[gn]
    jobs = []
    for k, source in enumerate(("NBHD", "NHDB")):
        x, caches, slots = _source(gn, source, "blocks", dt, seed=k)
        lay = native.KVLayout.paged(caches, slots, BS, source)
        a = _Arena(gn)
        jobs.append(dict(a=a, lay=lay, keep=(caches, slots), h=_begin(ctx, lay, gn, a), stream=torch.cuda.Stream(device=DEV), seed=k))
    torch.cuda.synchronize()
    for l in range(L):
        for j in jobs:
            j["h"].encode_layer(l, j["stream"].cuda_stream)
    for j in jobs:
        j["h"].finish(j["stream"].cuda_stream)
    for j in jobs:
        sz, blobs = j["a"].read()
        assert int(j["a"].status[0]) == 0 and blobs == _model_blobs(oracle, gn, dt, j["seed"])


def test_begin_refuses_what_the_one_piece_entry_refuses_and_wide_planes_are_not_layerwise(ctx):
    gn = "A"
    L, H, D, cs, ntok = GEOMS[gn]
    x, caches, slots = _source(gn, "NBHD", "blocks", BF16)
    layout = native.KVLayout.paged(caches, slots, BS, "NBHD")
    a = _Arena(gn, fill=7)
    with pytest.raises(native.NativeError):  # a short blob_stride
        ctx.encode_layers_begin_fixed(layout, 0, ntok, cs, _bins(L), a.blobs.data_ptr(), a.stride - 16, a.sizes.data_ptr())
    with pytest.raises(native.NativeError):  # no tokens
        ctx.encode_layers_begin_fixed(layout, 5, 5, cs, _bins(L), a.blobs.data_ptr(), a.stride, a.sizes.data_ptr())
    # fp8 KV
    c8 = [torch.zeros((2, 4, H, D, BS), dtype=torch.uint8, device=DEV).view(torch.float8_e4m3fn) for _ in range(L)]
    lay8 = native.KVLayout.paged(c8, torch.arange(32, dtype=torch.int64, device=DEV), BS, "NHDB")
    s8 = native.r16(native.blob_bound(L, 32, H, D))
    with pytest.raises(native.NativeError):
        ctx.encode_layers_begin_fixed(lay8, 0, 32, 32, _bins(L), a.blobs.data_ptr(), s8, a.sizes.data_ptr())
    torch.cuda.synchronize()
    assert a.sizes.cpu().tolist() == [7] * a.n and bool((a.blobs == POISON).all()), "nothing was written"
    # C = 2048: the one-piece encode takes it, the layer-wise one says so
    Lw, Hw, Dw, T = 1, 16, 128, 24
    wide = torch.randn((Lw, 2, T, Hw, Dw)).to(BF16).to(DEV)
    layw = native.KVLayout.from_chunk(wide, "vllm")
    sw = native.r16(native.blob_bound(Lw, T, Hw, Dw))
    arena = torch.zeros(sw, dtype=torch.uint8, device=DEV)
    sizes = torch.zeros(1, dtype=torch.int32, device=DEV)
    assert ctx.encode_layers_begin_fixed(layw, 0, T, T, [32, 16], arena.data_ptr(), sw, sizes.data_ptr()) is None
    ctx.encode_chunks_fixed(layw, 0, T, T, [32, 16], arena.data_ptr(), sw, sizes.data_ptr())
    torch.cuda.synchronize()
    assert int(sizes[0]) == native.fixed_blob_bytes(Lw, T, Hw, Dw, [32, 16])
    assert ctx.status(clear=True) == 0


# ------------------------------------------------------------------ 3. engine
def _engine(cs):
    return LMCacheEngine(LMCacheEngineConfig.from_legacy(chunk_size=cs, backend="cuda", local_serde="cachegen-fixed"),
                         dumb_metadata("vllm", "Llama-3-8B"))


def _keys(e, tokens):
    return [e._make_key(h, "vllm") for h in e._prefix_hashes_of(tokens)]


def _stored(e, tokens):
    torch.cuda.synchronize()
    entries = [e.engine_.dict[k] for k in _keys(e, tokens)]
    assert all(isinstance(c, _DevChunk) and c.model == "fixed" for c in entries)
    return [c.blob.cpu().numpy().tobytes() for c in entries]


def _retrieved(e, tokens, gn, source, dt, slots):
    L, H, D, cs, ntok = GEOMS[gn]
    dst = _empty_caches(source, L, H, D, dt, (len(tokens) + BS - 1) // BS + 3)
    mask = e.retrieve_into_paged(tokens, _as_arg(source, dst), slots, BS, _layout_name(source), direct=True)
    torch.cuda.synchronize()
    assert int(mask.sum()) == len(tokens)
    return [_ibits(c).clone() for c in dst]


def _store_layerwise(e, tokens, gn, source, x, caches, slots, blocking=True):
    """The forward pass: layer l's KV lands in the (NaN) cache, save_layer(l), NaN again behind layer_event(l)."""
    L = GEOMS[gn][0]
    store = e.store_paged_layerwise(tokens, _as_arg(source, caches), slots, BS, _layout_name(source), direct=True)
    assert store.layerwise
    for l in range(L):
        _fill_layer(source, caches, l, x[l], slots)
        store.save_layer(l)
        ev = store.layer_event(l)
        assert isinstance(ev, torch.cuda.Event)
        torch.cuda.current_stream().wait_event(ev)
        _poison(caches[l])
    store.finish(blocking=blocking)
    return store


@pytest.mark.parametrize("gn,source", [("A", "NHDB"), ("B", "NBHD"), ("C", "NHDB-pair")])
def test_engine_stores_layer_by_layer_what_store_paged_stores(monkeypatch, gn, source):
    dt = BF16  # (a "vllm" engine retrieves its CacheGen tiers as bf16: the cache retrieved into is bf16; fp16 sources: above)
    monkeypatch.setenv("LMCACHE_AMD_FIXED_LAYERWISE", "1")
    L, H, D, cs, ntok = GEOMS[gn]
    n = (ntok + cs - 1) // cs
    tokens = generate_tokens(ntok, DEV)
    e_lw, e_pre, e_nb = _engine(cs), _engine(cs), _engine(cs)
    monkeypatch.delenv("LMCACHE_AMD_FIXED_LAYERWISE")
    e_ref = _engine(cs)
    try:
        assert e_lw.engine_.fixed_layerwise and not e_ref.engine_.fixed_layerwise
        _, full, slots = _source(gn, source, "random", dt)
        e_ref.store_paged(tokens, _as_arg(source, full), slots, BS, _layout_name(source), direct=True)
        want = _stored(e_ref, tokens)
        x, caches, _ = _source(gn, source, "random", dt, fill=False)
        store = _store_layerwise(e_lw, tokens, gn, source, x, caches, slots)
        assert store.nchunks == n
        assert _stored(e_lw, tokens) == want
        kv_lw, kv_ref = (_retrieved(e, tokens, gn, source, dt, slots) for e in (e_lw, e_ref))
        assert all(torch.equal(p, q) for p, q in zip(kv_lw, kv_ref))
        # a stored prefix is skipped: only the missing range is encoded and published
        npre = (n - 1) * cs
        e_pre.store_paged(tokens[:npre], _as_arg(source, full), slots[:npre], BS, _layout_name(source), direct=True)
        before = [e_pre.engine_.dict[k] for k in _keys(e_pre, tokens)[:n - 1]]
        x2, c2, _ = _source(gn, source, "random", dt, fill=False)
        store = _store_layerwise(e_pre, tokens, gn, source, x2, c2, slots)
        assert store.nchunks == 1
        assert all(e_pre.engine_.dict[k] is b for k, b in zip(_keys(e_pre, tokens), before)), "the prefix's entries are untouched"
        assert _stored(e_pre, tokens) == want
        # finish(blocking=False), then drain()
        x3, c3, _ = _source(gn, source, "random", dt, fill=False)
        _store_layerwise(e_nb, tokens, gn, source, x3, c3, slots, blocking=False)
        e_nb.engine_.drain()
        assert _stored(e_nb, tokens) == want
        # the switch unset: today's fallback
        st = e_ref.store_paged_layerwise(tokens + 1, _as_arg(source, full), slots, BS, _layout_name(source), direct=True)
        assert not st.layerwise and st.layer_event(0) is None and st.finish() == n
    finally:
        torch.cuda.synchronize()
        for e in (e_lw, e_ref, e_pre, e_nb):
            e.close()


def test_a_group_stored_layer_by_layer_is_demoted_and_served_like_any_other(monkeypatch):
    monkeypatch.setenv("LMCACHE_AMD_FIXED_LAYERWISE", "1")
    monkeypatch.setenv("LMCACHE_AMD_FIXED_DEMOTE", "1")
    gn, source, dt = "A", "NBHD", BF16
    L, H, D, cs, ntok = GEOMS[gn]
    fx, twin = _engine(cs), _engine(cs)
    try:
        be = fx.engine_
        assert be.fixed_layerwise and be.fixed_demotes
        group = sum(native.r16(s) for s in [native.fixed_blob_bytes(L, min(cs, ntok - t0), H, D, be.cachegen_config.plane_bins(L))
                                            for t0 in range(0, ntok, cs)])
        be.set_capacity(hbm_bytes=group + group // 2, pinned_bytes=1 << 30)
        ta, tb = generate_tokens(ntok, DEV), generate_tokens(ntok, DEV) + 20000
        _, full, slots = _source(gn, source, "blocks", dt)
        twin.store_paged(ta, full, slots, BS, source)
        ref = _retrieved(twin, ta, gn, source, dt, slots)
        x, caches, _ = _source(gn, source, "blocks", dt, fill=False)
        _store_layerwise(fx, ta, gn, source, x, caches, slots)
        ka = _keys(fx, ta)
        assert {be.tier_of(k) for k in ka} == {"hbm"} and be.tier_stats()["demotions"] == 0
        x, caches, _ = _source(gn, source, "blocks", dt, seed=1, fill=False)
        _store_layerwise(fx, tb, gn, source, x, caches, slots)  # past the HBM budget: A goes down, transcoded
        st = be.tier_stats()
        assert st["demotions"] == 1 and st["evictions"] == 0
        assert [be.tier_of(k) for k in ka] == ["pinned"] * len(ka) and all(isinstance(be.dict[k], _PackChunk) for k in ka)
        assert {be.tier_of(k) for k in _keys(fx, tb)} == {"hbm"}
        got = _retrieved(fx, ta, gn, source, dt, slots)
        assert all(torch.equal(p, q) for p, q in zip(got, ref))
    finally:
        torch.cuda.synchronize()
        fx.close()
        twin.close()
