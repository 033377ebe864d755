"""retrieve_into_paged / retrieve_into_paged_layerwise with direct=True AND rope on an "NHDB" cache, behind
LMCACHE_AMD_SPLIT_ROPE=1 (read when the engine is built): the KV goes straight into the split blocks and the keys are
re-rotated there (lmc_rope_shift_split), no staged chunk.  The reference is the staged call (direct=False) of the same
engine into a second set of caches: every cache tensor and ret_mask, bit for bit."""
import pytest
import torch

from lmcache_amd import native
from lmcache_amd.cache_engine import LMCacheEngine
from lmcache_amd.config import LMCacheEngineConfig
from lmcache_amd.rope import RopeShift
from tests.test_gpu_engine import dumb_metadata, generate_tokens
from tests.test_gpu_rope_shift import _ibits, _random_bits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CS, NTOK, L, H, D, BS = 32, 80, 4, 2, 64, 16  # a ragged last chunk
NB = 2 * ((NTOK + BS - 1) // BS) + 2
BACKENDS = ["coded-hbm", "cachegen-fixed", "pinned-pack", "raw-hbm"]
TABLE_ROWS = 128


def _cfg(backend, cs=CS):
    device, serde = {"coded-hbm": ("cuda", "cachegen"), "cachegen-fixed": ("cuda", "cachegen-fixed"),
                     "pinned-pack": ("cpu", "cachegen"), "raw-hbm": ("cuda", None)}[backend]
    kw = {} if serde is None else {"local_serde": serde}
    return LMCacheEngineConfig.from_legacy(chunk_size=cs, backend=device, **kw)


def _engine(monkeypatch, backend, switch=True, cs=CS):
    if switch:
        monkeypatch.setenv("LMCACHE_AMD_SPLIT_ROPE", "1")  # (read when the engine is built)
    else:
        monkeypatch.delenv("LMCACHE_AMD_SPLIT_ROPE", raising=False)
    native.build()
    eng = LMCacheEngine(_cfg(backend, cs), dumb_metadata("vllm", "Llama-3-8B"))
    assert eng.split_rope == switch
    return eng


def _kv(g, ntok=NTOK, layers=L, heads=H, hd=D):
    return tuple((torch.rand((ntok, heads, hd), generator=g).to(torch.bfloat16).to(DEV),
                  torch.rand((ntok, heads, hd), generator=g).to(torch.bfloat16).to(DEV)) for _ in range(layers))


def _fresh(g):
    return [_random_bits((2, NB, H, D, BS), torch.bfloat16, g).to(DEV) for _ in range(L)]


def _as(caches, pair):
    if not pair:
        return caches
    return [(c[0].view(c.shape[1], c.shape[2], c.shape[3] // 8, c.shape[4], 8), c[1]) for c in caches]


def _ropes(g):
    uniform = RopeShift.from_base(10000.0, D, TABLE_ROWS, DEV, is_neox=True, delta=37)
    per_tok = torch.randint(-(TABLE_ROWS - 1), TABLE_ROWS, (NTOK,), generator=g, dtype=torch.int32)
    return {"uniform": uniform, "per_token": RopeShift(uniform.cos_sin, D, True, per_tok.to(DEV))}


def _same(a, b, what):
    for l, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(_ibits(x), _ibits(y)), f"{what}: layer {l}"


@pytest.mark.parametrize("backend", BACKENDS)
def test_direct_with_rope_leaves_what_the_staged_call_leaves(monkeypatch, backend):
    g = torch.Generator().manual_seed(60 + BACKENDS.index(backend))
    tokens, kv = generate_tokens(NTOK, DEV), _kv(g)
    engine = _engine(monkeypatch, backend)
    try:
        engine.store(tokens, kv)
        tail = torch.ones(NTOK, dtype=torch.bool, device=DEV)
        tail[:40] = False  # a suffix mask that cuts into the second chunk: the first-chunk trim
        for name, rope in _ropes(g).items():
            for pair in (False, True):
                for mask in (None, tail):
                    slots = torch.randperm(NB * BS, generator=g)[:NTOK].to(DEV)
                    start = _fresh(g)
                    what = f"{backend} {name} pair={pair} mask={'tail' if mask is not None else None}"
                    # the one-piece call
                    a, b = [c.clone() for c in start], [c.clone() for c in start]
                    ma = engine.retrieve_into_paged(tokens, _as(a, pair), slots, BS, "NHDB", mask=mask, rope=rope, direct=True)
                    mb = engine.retrieve_into_paged(tokens, _as(b, pair), slots, BS, "NHDB", mask=mask, rope=rope, direct=False)
                    torch.cuda.synchronize()
                    nskip = 0 if mask is None else 40
                    assert torch.equal(ma, mb) and int(ma.sum()) == NTOK - nskip, what
                    assert any(not torch.equal(_ibits(x), _ibits(y)) for x, y in zip(b, start)), "nothing was retrieved"
                    _same(a, b, what + " one piece")
                    # the layer-wise call
                    for lpl in ((1, 3), 1, 3):  # a schedule of two ranges (1 layer, then 3), and one range size
                        c = [x.clone() for x in start]
                        r = engine.retrieve_into_paged_layerwise(tokens, _as(c, pair), slots, BS, "NHDB", mask=mask, rope=rope,
                                                                 direct=True, layers_per_launch=lpl)
                        r.finish()
                        torch.cuda.synchronize()
                        assert torch.equal(r.ret_mask, mb), what
                        _same(c, b, what + f" layer-wise {lpl}")
        assert native.get_context(0).status(clear=True) == 0
    finally:
        engine.close()


@pytest.mark.parametrize("backend", BACKENDS)
def test_a_layers_event_says_rotated(monkeypatch, backend):
    """A copy of layer 0 queued on a side stream behind wait_layer(0) already holds layer 0's final bits."""
    g = torch.Generator().manual_seed(70 + BACKENDS.index(backend))
    tokens, kv = generate_tokens(NTOK, DEV), _kv(g)
    engine = _engine(monkeypatch, backend)
    try:
        engine.store(tokens, kv)
        rope = _ropes(g)["per_token"]
        slots = torch.randperm(NB * BS, generator=g)[:NTOK].to(DEV)
        start = _fresh(g)
        want = [c.clone() for c in start]
        engine.retrieve_into_paged(tokens, want, slots, BS, "NHDB", rope=rope, direct=False)
        torch.cuda.synchronize()
        got = [c.clone() for c in start]
        early = torch.zeros_like(got[0])
        side = torch.cuda.Stream(device=DEV)
        torch.cuda.synchronize()
        r = engine.retrieve_into_paged_layerwise(tokens, got, slots, BS, "NHDB", rope=rope, direct=True, layers_per_launch=(1, 3))
        r.wait_layer(0, side)
        with torch.cuda.stream(side):
            early.copy_(got[0], non_blocking=True)
        r.finish()
        torch.cuda.synchronize()
        assert torch.equal(_ibits(early), _ibits(want[0])), "layer 0 behind its event is not final"
        _same(got, want, "after finish")
    finally:
        engine.close()


@pytest.mark.parametrize("backend", BACKENDS)
def test_a_miss_launches_nothing(monkeypatch, backend):
    g = torch.Generator().manual_seed(80)
    tokens, kv = generate_tokens(NTOK, DEV), _kv(g)
    engine = _engine(monkeypatch, backend)
    try:
        engine.store(tokens, kv)
        rope = _ropes(g)["uniform"]
        slots = torch.randperm(NB * BS, generator=g)[:NTOK].to(DEV)
        c = _fresh(g)
        keep = [x.clone() for x in c]
        m = engine.retrieve_into_paged(tokens + 10000, c, slots, BS, "NHDB", rope=rope, direct=True)
        r = engine.retrieve_into_paged_layerwise(tokens + 10000, c, slots, BS, "NHDB", rope=rope, direct=True)
        r.finish()
        torch.cuda.synchronize()
        assert not m.any() and not r.ret_mask.any() and not r.layer_events
        _same(c, keep, "a miss")
        assert native.get_context(0).status(clear=True) == 0
    finally:
        engine.close()


def test_without_the_switch_nothing_changes(monkeypatch):
    """The coded tier still raises ValueError before anything is queued; the fixed-width tier still returns the staged result."""
    g = torch.Generator().manual_seed(90)
    tokens, kv = generate_tokens(NTOK, DEV), _kv(g)
    rope = _ropes(g)["uniform"]
    slots = torch.randperm(NB * BS, generator=g)[:NTOK].to(DEV)
    start = _fresh(g)
    engine = _engine(monkeypatch, "coded-hbm", switch=False)
    try:
        engine.store(tokens, kv)
        c = [x.clone() for x in start]
        with pytest.raises(ValueError, match="direct=True with rope"):
            engine.retrieve_into_paged(tokens, c, slots, BS, "NHDB", rope=rope, direct=True)
        with pytest.raises(ValueError, match="direct=True with rope"):
            engine.retrieve_into_paged_layerwise(tokens, c, slots, BS, "NHDB", rope=rope, direct=True)
        torch.cuda.synchronize()
        _same(c, start, "refused")
    finally:
        engine.close()
    engine = _engine(monkeypatch, "cachegen-fixed", switch=False)
    try:
        engine.store(tokens, kv)
        a, b = [x.clone() for x in start], [x.clone() for x in start]
        ma = engine.retrieve_into_paged(tokens, a, slots, BS, "NHDB", rope=rope, direct=True)
        mb = engine.retrieve_into_paged(tokens, b, slots, BS, "NHDB", rope=rope, direct=False)
        torch.cuda.synchronize()
        assert torch.equal(ma, mb) and ma.all()
        _same(a, b, "the fixed-width tier without the switch")
        assert engine._direct_retrieve(True, "NHDB", rope) is False  # (it staged)
    finally:
        engine.close()


@pytest.mark.parametrize("backend", ["coded-hbm", "cachegen-fixed"])
def test_the_direct_call_allocates_no_staged_chunk(monkeypatch, backend):
    """A retrieved KV of 16 MiB (L 4, H 8, D 128, 1024 tokens): across the direct call the peak allocation grows by less
    than half of that, while the staged call of the same engine holds the whole of it."""
    Lm, Hm, Dm, T, cs = 4, 8, 128, 1024, 256
    kv_bytes = Lm * 2 * T * Hm * Dm * 2
    assert kv_bytes >= 16 << 20
    g = torch.Generator().manual_seed(95)
    tokens, kv = generate_tokens(T, DEV), _kv(g, T, Lm, Hm, Dm)
    nb = T // BS + 2
    engine = _engine(monkeypatch, backend, cs=cs)
    try:
        engine.store(tokens, kv)
        rope = RopeShift.from_base(10000.0, Dm, TABLE_ROWS, DEV, is_neox=True, delta=37)
        slots = torch.randperm(nb * BS, generator=g)[:T].to(DEV)
        caches = [torch.zeros((2, nb, Hm, Dm, BS), dtype=torch.bfloat16, device=DEV) for _ in range(Lm)]
        staged = [c.clone() for c in caches]
        # once before the measurement: whatever the tier keeps across calls (tables, staging of its own) is there then
        engine.retrieve_into_paged(tokens, caches, slots, BS, "NHDB", rope=rope, direct=True)
        engine.retrieve_into_paged(tokens, staged, slots, BS, "NHDB", rope=rope, direct=False)
        torch.cuda.synchronize()
        _same(caches, staged, "16 MiB")
        grown = {}
        for direct in (True, False):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            m = engine.retrieve_into_paged(tokens, caches, slots, BS, "NHDB", rope=rope, direct=direct)
            torch.cuda.synchronize()
            assert m.all()
            grown[direct] = torch.cuda.max_memory_allocated() - before
        print(f"{backend}: peak allocation across the call: direct {grown[True]} bytes, staged {grown[False]} bytes, "
              f"retrieved KV {kv_bytes} bytes")
        assert grown[True] < kv_bytes // 2
        assert grown[False] >= kv_bytes  # (the measurement sees a staged chunk where there is one)
    finally:
        engine.close()
