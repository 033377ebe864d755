"""The layer-by-layer store from the paged cache: lmc_encode_layers_* (csrc/k_layers.h, the plane-subset launches of
k_quantize and the counts-only k_cdf_encode), CacheGenDeviceCodec.encode_layers, LMCLocalBackend.begin_put_kv_layers and
LMCacheEngine.store_paged_layerwise.

Nothing here has a tolerance: a blob whose encode was issued per layer is, byte for byte, the blob of the one-piece encode
of the same source, and the oracle's blob of the gathered chunk.

Geometries (the smallest that reach every branch; bins are explicit and mix nibble (<= 17) and byte planes):
  A  L=3 H=2 D=64   C=128  G=2   chunk 32, 3*32+7 tokens   per-wave granules, a ragged tail
  B  L=2 H=8 D=128  C=1024 G=16  chunk 64, 128 tokens      workgroup granules, the NITER=2 quantiser instances
  C  L=2 H=3 D=80   C=240  G=4   chunk 40, 2*40+2 tokens   a partial last group, the shortest counts-model tail"""
import struct

import numpy as np
import pytest
import torch

from lmcache_amd import native
from lmcache_amd.cache_engine import LMCacheEngine
from tests.test_gpu_engine import dumb_metadata, generate_tokens, make_cfg
from tests.test_gpu_paged_split import _ibits, _mapping, _torch_scatter, _views

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BS = 16
BF16, FP16, E4M3 = torch.bfloat16, torch.float16, torch.float8_e4m3fn
NAMES = {BF16: "bf16", FP16: "fp16", E4M3: "e4m3"}
INVALID = -1
#        L  H  D    chunk tokens
GEOMS = {"A": (3, 2, 64, 32, 3 * 32 + 7),
         "B": (2, 8, 128, 64, 128),
         "C": (2, 3, 80, 40, 2 * 40 + 2)}
BIN_CYCLE = [32, 16, 12, 20, 17, 24]  # per plane: byte, nibble, nibble, byte, nibble (the limit), byte
SOURCES = ["NBHD", "NHBD", "NHDB", "NHDB-pair"]
MAPPINGS = ["blocks", "random"]
CASES = [(gn, src, m, dt) for gn in GEOMS for src in SOURCES for m in MAPPINGS for dt in (BF16, FP16)]
CASES += [("C", src, m, E4M3) for src in ("NHDB", "NHDB-pair") for m in MAPPINGS]


def _bins(L):
    return [BIN_CYCLE[p % len(BIN_CYCLE)] for p in range(2 * L)]


@pytest.fixture(scope="module")
def ctx():
    native.build()
    return native.get_context(0)


@pytest.fixture(scope="module")
def oracle():
    from oracle import lmc_oracle
    lmc_oracle.build()
    return lmc_oracle


def _kv(gn, dt, seed=0):
    """[L, 2, ntok, H, D] of dt (CPU), the same for every source and mapping of a geometry: randn with an all-zero token, a
    token with an inf and one with a NaN in every plane (fp8: drawn in bf16 and cast)."""
    L, H, D, cs, ntok = GEOMS[gn]
    g = torch.Generator().manual_seed(1000 + 7 * ord(gn) + seed)
    x = torch.randn((L, 2, ntok, H, D), generator=g).to(torch.bfloat16)
    x[:, :, 9] = 0
    x[:, :, 21, 0, 3] = float("inf")
    x[:, :, ntok - 2, H - 1, D - 2] = float("nan")
    return x.to(dt)


_ORACLE = {}


def _oracle_blobs(oracle, gn, dt, seed=0):
    """The oracle's blob of every chunk, computed once per (geometry, dtype) and shared (fp8: the blob of the bf16 images
    with header word 23 set)."""
    key = (gn, dt, seed)
    if key not in _ORACLE:
        L, H, D, cs, ntok = GEOMS[gn]
        x, out = _kv(gn, dt, seed), []
        for t0 in range(0, ntok, cs):
            part = x[:, :, t0:t0 + cs].reshape(L, 2, -1, H * D)
            bits, code = oracle.torch_to_bits((part.to(BF16) if dt == E4M3 else part).contiguous())
            blob = oracle.encode_blob(bits, code, H, D, np.array(_bins(L), np.int32))
            if dt == E4M3:
                blob = blob[:92] + struct.pack("<I", native.dtype_code(dt)) + blob[96:]
            out.append(blob)
        _ORACLE[key] = out
    return _ORACLE[key]


def _empty_caches(source, L, H, D, dt, nb):
    """Per layer an empty (non-zero garbage) cache of the source's form."""
    shape = {"NBHD": (2, nb, BS, H, D), "NHBD": (2, nb, H, BS, D)}.get(source, (2, nb, H, D, BS))
    out = []
    for _ in range(L):
        c = torch.full(shape, 0x3c if dt.itemsize == 1 else 0x3c3c, dtype=torch.uint8 if dt.itemsize == 1 else torch.int16,
                       device=DEV).view(dt)
        out.append(c)
    return out


def _fill_layer(source, caches, l, xl, slots):
    """Layer l's K and V (xl [2, T, H, D] on the device) into slot slots[t] of caches[l]."""
    blk, off = slots // BS, slots % BS
    c = caches[l]
    if source == "NBHD":
        _ibits(c)[0, blk, off] = _ibits(xl[0])
        _ibits(c)[1, blk, off] = _ibits(xl[1])
    elif source == "NHBD":
        _ibits(c)[0, blk, :, off] = _ibits(xl[0])
        _ibits(c)[1, blk, :, off] = _ibits(xl[1])
    else:
        _torch_scatter([c], _ibits(xl)[None], slots, BS)


def _as_arg(source, caches):
    """What store_paged / KVLayout.paged take: the tensors, or for "NHDB-pair" the (key_cache, value_cache) views."""
    return [_views(c) for c in caches] if source == "NHDB-pair" else caches


def _layout_name(source):
    return "NHDB" if source.startswith("NHDB") else source


def _poison(c):
    if c.dtype.itemsize == 1:
        c.view(torch.uint8).fill_(0x7f)  # e4m3fn's NaN
    else:
        c.fill_(float("nan"))


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
    return x, caches, slots


class _Arena:
    """Blob arena, size words and a status word of one C-ABI encode job."""

    def __init__(self, gn, fill=0):
        L, H, D, cs, ntok = GEOMS[gn]
        self.n = (ntok + cs - 1) // cs
        self.stride = native.r16(native.blob_bound(L, cs, H, D))
        self.blobs = torch.zeros(self.n * self.stride, dtype=torch.uint8, device=DEV)
        self.sizes = torch.full((self.n,), fill, dtype=torch.int32, device=DEV)
        self.status = torch.zeros(1, dtype=torch.int32, device=DEV)

    def read(self):
        torch.cuda.synchronize()
        sz, host = self.sizes.cpu().tolist(), self.blobs.cpu().numpy()
        return sz, [host[i * self.stride:i * self.stride + sz[i]].tobytes() for i in range(self.n)]


def _one_piece(ctx, layout, gn):
    L, H, D, cs, ntok = GEOMS[gn]
    a = _Arena(gn)
    fn = ctx.encode_chunks_split if layout.struct.paged_kind == native.PAGED_SPLIT else ctx.encode_chunks
    fn(layout, 0, ntok, cs, _bins(L), a.blobs.data_ptr(), a.stride, a.sizes.data_ptr(), status_ptr=a.status.data_ptr())
    out = a.read()
    assert int(a.status[0]) == 0
    return out


def _begin(ctx, layout, gn, a):
    L, H, D, cs, ntok = GEOMS[gn]
    h = ctx.encode_layers_begin(layout, 0, ntok, cs, _bins(L), a.blobs.data_ptr(), a.stride, a.sizes.data_ptr(),
                                status_ptr=a.status.data_ptr())
    assert h is not None, "these geometries are eligible"
    return h


# ------------------------------------------------------------------ 1. byte equality
@pytest.mark.parametrize("gn,source,mapping,dt", CASES, ids=["%s-%s-%s-%s" % (g, s, m, NAMES[d]) for g, s, m, d in CASES])
def test_blobs_of_the_layerwise_encode_equal_the_one_piece_and_the_oracle(ctx, oracle, gn, source, mapping, dt):
    L, H, D, cs, ntok = GEOMS[gn]
    x, caches, slots = _source(gn, source, mapping, dt)
    layout = native.KVLayout.paged(_as_arg(source, caches), slots, BS, _layout_name(source))
    a = _Arena(gn)
    h = _begin(ctx, layout, gn, a)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    for l in range(L):
        h.encode_layer(l, side.cuda_stream)
    side.synchronize()
    assert a.sizes.cpu().tolist() == [0] * a.n, "a size word stays 0 until the finish launch"
    h.finish(side.cuda_stream)
    sz, blobs = a.read()
    assert int(a.status[0]) == 0
    sz1, blobs1 = _one_piece(ctx, layout, gn)
    want = _oracle_blobs(oracle, gn, dt)
    assert sz == sz1 == [len(b) for b in want]
    for i in range(a.n):
        assert blobs[i] == blobs1[i], f"chunk {i}: layer-wise vs one piece"
        assert blobs[i] == want[i], f"chunk {i}: layer-wise vs oracle"
        native.blob_info(blobs[i])
    # ... and decodes to the oracle's tensor (an fp8 blob: into its bf16 images)
    out_dt = BF16 if dt == E4M3 else dt
    dst = torch.zeros((L, 2, ntok, H, D), dtype=out_dt, device=DEV)
    ctx.decode_chunks(a.blobs.data_ptr(), a.stride, a.n, native.KVLayout.from_chunk(dst, "vllm"), 0, cs,
                      status_ptr=a.status.data_ptr())
    torch.cuda.synchronize()
    assert int(a.status[0]) == 0
    code = native.dtype_code(out_dt)
    ref = np.concatenate([oracle.decode_blob(b, code) for b in want], axis=2)
    got = _ibits(dst).cpu().numpy().view(np.uint16).reshape(L, 2, ntok, H * D)
    # (the rows with a NaN or a 0 x inf product are NaN on both sides, whatever the payload bits of each cast)
    inf_bits = 0x7f80 if out_dt == BF16 else 0x7c00
    nan_w, nan_g = (ref & 0x7fff) > inf_bits, (got & 0x7fff) > inf_bits
    assert np.array_equal(nan_w, nan_g) and np.array_equal(got[~nan_w], ref[~nan_w])


# ------------------------------------------------------------------ 3. refusals
def test_out_of_order_calls_are_refused_and_queue_nothing_and_abort_frees_the_buffers(ctx, oracle):
    gn, dt = "A", BF16
    L, H, D, cs, ntok = GEOMS[gn]
    x, caches, slots = _source(gn, "NBHD", "blocks", dt)
    layout = native.KVLayout.paged(caches, slots, BS, "NBHD")
    PAT = 0x5A5A5A5A
    a = _Arena(gn, fill=PAT)
    st = torch.cuda.current_stream().cuda_stream
    h = _begin(ctx, layout, gn, a)
    assert h.encode_layer_rc(1, st) == INVALID, "layer 1 before layer 0"
    assert h.finish_rc(st) == INVALID
    torch.cuda.synchronize()
    assert a.sizes.cpu().tolist() == [PAT] * a.n and not bool(a.blobs.any()), "a refused call queues nothing"
    h.encode_layer(0, st)
    assert h.encode_layer_rc(0, st) == INVALID, "a layer given twice"
    assert h.encode_layer_rc(2, st) == INVALID, "a layer skipped"
    h.encode_layer(1, st)
    assert h.finish_rc(st) == INVALID, "finish after L - 1 layers"
    torch.cuda.synchronize()
    assert a.sizes.cpu().tolist() == [0] * a.n, "no size word before the finish launch"
    h.encode_layer(2, st)
    assert h.encode_layer_rc(L, st) == INVALID, "layer index L"
    torch.cuda.synchronize()
    assert a.sizes.cpu().tolist() == [0] * a.n
    h.abort()
    torch.cuda.synchronize()
    assert a.sizes.cpu().tolist() == [0] * a.n and int(a.status[0]) == 0
    # a fresh job on the same buffers
    h = _begin(ctx, layout, gn, a)
    for l in range(L):
        h.encode_layer(l, st)
    h.finish(st)
    sz, blobs = a.read()
    want = _oracle_blobs(oracle, gn, dt)
    assert int(a.status[0]) == 0 and sz == [len(b) for b in want] and blobs == want


def test_begin_refuses_what_the_one_piece_entry_refuses_and_names_what_is_not_layerwise(ctx):
    gn = "A"
    L, H, D, cs, ntok = GEOMS[gn]
    x, caches, slots = _source(gn, "NBHD", "blocks", BF16)
    layout = native.KVLayout.paged(caches, slots, BS, "NBHD")
    a = _Arena(gn)
    args = (_bins(L), a.blobs.data_ptr(), a.stride, a.sizes.data_ptr())
    with pytest.raises(native.NativeError):
        ctx.encode_layers_begin(layout, 0, ntok, cs, _bins(L), a.blobs.data_ptr(), a.stride - 16, a.sizes.data_ptr())
    with pytest.raises(native.NativeError):
        ctx.encode_layers_begin(layout, 5, 5, cs, *args)
    # a one-token tail, a chunk longer than 256 tokens: fine for the one-piece encode, not layer-wise
    assert ctx.encode_layers_begin(layout, 0, 2 * cs + 1, cs, *args) is None
    big = native.r16(native.blob_bound(L, 300, H, D))
    blobs = torch.zeros(big, dtype=torch.uint8, device=DEV)
    assert ctx.encode_layers_begin(layout, 0, ntok, 300, _bins(L), blobs.data_ptr(), big, a.sizes.data_ptr()) is None
    assert ctx.status(clear=True) == 0


# ------------------------------------------------------------------ engine level
def _engine(backend, cs):
    return LMCacheEngine(make_cfg(backend, cs), dumb_metadata("vllm", "Llama-3-8B"))


def _keys(e, tokens):
    return [e._make_key(h, "vllm") for h in e._prefix_hashes_of(tokens)]


def _entry_bytes(entry):
    blob = getattr(entry, "blob", None)
    if hasattr(entry, "pack") and blob is None:
        return entry.pack.extract(entry.index)
    return blob.cpu().numpy().tobytes() if isinstance(blob, torch.Tensor) else blob.tobytes()


def _stored(e, tokens):
    """The stored blob of every chunk of `tokens` (all present)."""
    torch.cuda.synchronize()
    return [_entry_bytes(e.engine_.dict[k]) for k in _keys(e, tokens)]


def _retrieved(e, tokens, gn, source, dt, slots):
    """retrieve_into_paged into a second, empty cache -> its integer views."""
    L, H, D, cs, ntok = GEOMS[gn]
    dst = _empty_caches(source, L, H, D, dt, (len(tokens) + BS - 1) // BS + 3)
    mask = e.retrieve_into_paged(tokens, _as_arg(source, dst), slots, BS, _layout_name(source), direct=True)
    torch.cuda.synchronize()
    assert int(mask.sum()) == len(tokens)
    return [_ibits(c).clone() for c in dst]


def _store_layerwise(e, tokens, gn, source, dt, x, caches, slots, poison=True, blocking=True, **kw):
    """The forward pass: layer l's KV lands in the cache, save_layer(l); with `poison` the cache is overwritten with NaN
    behind layer_event(l)."""
    L = GEOMS[gn][0]
    store = e.store_paged_layerwise(tokens, _as_arg(source, caches), slots, BS, _layout_name(source), direct=True, **kw)
    for l in range(L):
        _fill_layer(source, caches, l, x[l], slots)
        store.save_layer(l)
        if poison and store.layerwise:
            torch.cuda.current_stream().wait_event(store.layer_event(l))
            _poison(caches[l])
    store.finish(blocking=blocking)
    return store


# ------------------------------------------------------------------ 2. encoded at layer time
@pytest.mark.parametrize("gn,source,dt", [("A", "NBHD", BF16), ("A", "NHDB", FP16), ("B", "NHBD", FP16), ("B", "NHDB-pair", BF16),
                                          ("C", "NHDB", E4M3), ("C", "NBHD", BF16)],
                         ids=lambda v: NAMES.get(v, v))
def test_a_layer_is_read_when_it_is_saved_and_may_be_overwritten_behind_its_event(gn, source, dt):
    """Each layer's cache is filled just before save_layer(l) and overwritten with NaN behind layer_event(l): the blobs are
    those of the unpoisoned cache.  A store that reads the cache at finish() cannot pass."""
    L, H, D, cs, ntok = GEOMS[gn]
    tokens = generate_tokens(ntok, DEV)
    x, caches, slots = _source(gn, source, "blocks", dt, fill=False)
    e_lw, e_ref = _engine("cachegen-hbm", cs), _engine("cachegen-hbm", cs)
    try:
        store = _store_layerwise(e_lw, tokens, gn, source, dt, x, caches, slots)
        assert store.layerwise and store.nchunks == (ntok + cs - 1) // cs, "these geometries are eligible: no fallback"
        _, full, _ = _source(gn, source, "blocks", dt)
        e_ref.store_paged(tokens, _as_arg(source, full), slots, BS, _layout_name(source), direct=True)
        got, want = _stored(e_lw, tokens), _stored(e_ref, tokens)
        assert len(got) == len(want) and all(len(b) > 0 for b in want)
        for i, (g_, w_) in enumerate(zip(got, want)):
            assert g_ == w_, f"chunk {i}"
    finally:
        e_lw.close()
        e_ref.close()


# ------------------------------------------------------------------ 4. fallbacks
@pytest.mark.parametrize("backend,extra", [("cuda", 1), ("cpu", 1), ("cuda", -6), ("cachegen-hbm", -6)],
                         ids=["hbm-raw", "pinned-raw", "hbm-raw-tail1", "cachegen-hbm-tail1"])
def test_what_is_not_layerwise_stores_in_one_piece_at_finish(backend, extra):
    """Geometry A's tokens plus one on the raw tiers, which have no layer-wise path; and 3 * 32 + 1 tokens -- a tail chunk of
    ONE token -- on a raw tier and on the CacheGen tier, whose encoder declares such a job not layer-wise.  finish()
    leaves what store_paged leaves: the same keys, the same retrieved KV."""
    gn, source, dt = "A", "NBHD", BF16
    L, H, D, cs, ntok = GEOMS[gn]
    ntok += extra
    assert extra == 1 or ntok % cs == 1
    tokens = generate_tokens(ntok, DEV)
    g = torch.Generator().manual_seed(3)
    nb = (ntok + BS - 1) // BS + 3
    slots = _mapping("blocks", ntok, nb, BS, g).to(DEV)
    x = torch.randn((L, 2, ntok, H, D), generator=g).to(dt).to(DEV)
    caches = _empty_caches(source, L, H, D, dt, nb)
    e_lw, e_ref = _engine(backend, cs), _engine(backend, cs)
    try:
        store = e_lw.store_paged_layerwise(tokens, caches, slots, BS, "NBHD")
        for l in range(L):
            _fill_layer(source, caches, l, x[l], slots)
            store.save_layer(l)
            assert store.layer_event(l) is None
        assert not store.layerwise and store.finish() == 4
        e_ref.store_paged(tokens, caches, slots, BS, "NBHD")
        assert all(e_lw.engine_.contains(k) for k in _keys(e_lw, tokens))
        outs = []
        for e in (e_lw, e_ref):
            dst = _empty_caches(source, L, H, D, dt, nb)
            assert int(e.retrieve_into_paged(tokens, dst, slots, BS, "NBHD").sum()) == ntok
            torch.cuda.synchronize()
            outs.append([_ibits(c).clone() for c in dst])
        assert all(torch.equal(p, q) for p, q in zip(*outs))
    finally:
        e_lw.close()
        e_ref.close()


# ------------------------------------------------------------------ 5. engine: the three tiers
@pytest.mark.parametrize("tier", ["cachegen-hbm", "cachegen-host", "cachegen-host-unpinned"])
def test_the_tiers_hold_what_store_paged_leaves(monkeypatch, tier):
    if tier == "cachegen-host-unpinned":
        monkeypatch.setenv("LMCACHE_AMD_PINNED_PACKS", "0")
    backend = "cachegen-host" if tier.startswith("cachegen-host") else tier
    gn, source, dt = "A", "NHDB", BF16
    L, H, D, cs, ntok = GEOMS[gn]
    tokens = generate_tokens(ntok, DEV)
    x, caches, slots = _source(gn, source, "random", dt, fill=False)
    _, full, _ = _source(gn, source, "random", dt)
    e_lw, e_ref, e_pre, e_nb = (_engine(backend, cs) for _ in range(4))
    try:
        store = _store_layerwise(e_lw, tokens, gn, source, dt, x, caches, slots)
        assert store.layerwise
        e_ref.store_paged(tokens, full, slots, BS, "NHDB", direct=True)
        assert _stored(e_lw, tokens) == _stored(e_ref, tokens)
        if tier == "cachegen-host":  # the pack is the pack store_pack makes of the range
            p_lw, p_ref = (e.engine_.dict[_keys(e, tokens)[0]].pack for e in (e_lw, e_ref))
            assert p_lw.nchunks == p_ref.nchunks == 4 and p_lw.blob.tobytes() == p_ref.blob.tobytes()
        kv_lw, kv_ref = (_retrieved(e, tokens, gn, source, dt, slots) for e in (e_lw, e_ref))
        assert all(torch.equal(p, q) for p, q in zip(kv_lw, kv_ref))
        # a stored two-chunk prefix is skipped: only the rest is encoded and published
        e_pre.store_paged(tokens[:2 * cs], full, slots[:2 * cs], BS, "NHDB", direct=True)
        before = [e_pre.engine_.dict[k] for k in _keys(e_pre, tokens)[:2]]
        x2, c2, _ = _source(gn, source, "random", dt, fill=False)
        store = _store_layerwise(e_pre, tokens, gn, source, dt, x2, c2, slots)
        assert store.layerwise and store.nchunks == 2
        assert all(e_pre.engine_.dict[k] is b for k, b in zip(_keys(e_pre, tokens), before)), "the prefix's entries are untouched"
        assert _stored(e_pre, tokens) == _stored(e_ref, tokens)
        # everything present: every method is a no-op
        store = _store_layerwise(e_pre, tokens, gn, source, dt, x2, c2, slots)
        assert store.nchunks == 0 and not store.layerwise and store.layer_event(0) is None
        # finish(blocking=False), then drain(): the same entries
        x3, c3, _ = _source(gn, source, "random", dt, fill=False)
        _store_layerwise(e_nb, tokens, gn, source, dt, x3, c3, slots, blocking=False)
        e_nb.engine_.drain()
        assert _stored(e_nb, tokens) == _stored(e_ref, tokens)
    finally:
        for e in (e_lw, e_ref, e_pre, e_nb):
            e.close()


# ------------------------------------------------------------------ 6. two jobs at once
def test_two_stores_with_interleaved_layers_on_two_streams():
    gn, dt = "A", BF16
    L, H, D, cs, ntok = GEOMS[gn]
    e_lw, e_ref = _engine("cachegen-hbm", cs), _engine("cachegen-hbm", cs)
    try:
        jobs = []
        for k, source in enumerate(("NBHD", "NHDB")):
            x, caches, slots = _source(gn, source, "blocks", dt, seed=k, fill=False)
            jobs.append(dict(source=source, x=x, caches=caches, slots=slots, tokens=generate_tokens(ntok, DEV),
                             stream=torch.cuda.Stream(device=DEV)))
        torch.cuda.synchronize()
        for j in jobs:
            j["store"] = e_lw.store_paged_layerwise(j["tokens"], j["caches"], j["slots"], BS, j["source"], direct=True)
            assert j["store"].layerwise
        for l in range(L):
            for j in jobs:
                with torch.cuda.stream(j["stream"]):
                    _fill_layer(j["source"], j["caches"], l, j["x"][l], j["slots"])
                    j["store"].save_layer(l)
                    j["stream"].wait_event(j["store"].layer_event(l))
                    _poison(j["caches"][l])
        for j in jobs:
            with torch.cuda.stream(j["stream"]):
                j["store"].finish()
        for k, j in enumerate(jobs):
            _, full, _ = _source(gn, j["source"], "blocks", dt, seed=k)
            e_ref.store_paged(j["tokens"], full, j["slots"], BS, j["source"], direct=True)
            assert _stored(e_lw, j["tokens"]) == _stored(e_ref, j["tokens"]), j["source"]
    finally:
        e_lw.close()
        e_ref.close()
