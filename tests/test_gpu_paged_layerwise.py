"""LMCacheEngine.retrieve_into_paged_layerwise on the GPU: the paged cache filled range of layers by range of layers,
with the post-ops of a range (RoPE shift, the scatter of a staged "NHDB" retrieve) in front of the range's event.

The reference is retrieve_into_paged with the same arguments into a twin cache: every comparison is on integer views
of the WHOLE cache tensors (the unused slots hold random bit patterns and must keep them)."""
import pytest
import torch

from lmcache_amd import native
from lmcache_amd.cache_engine import LMCacheEngine
from lmcache_amd.rope import RopeShift
from tests.test_gpu_engine import dumb_metadata, generate_tokens, make_cfg
from tests.test_gpu_rope_shift import _ibits, _mapping, _random_bits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
L, NTOK, CS = 3, 70, 32
# (layout, the NHDB cache as a (key_cache, value_cache) pair, direct)
LAYOUTS = [("NBHD", False, False), ("NHBD", False, False), ("NHDB", False, False), ("NHDB", True, False), ("NHDB", False, True)]
# (slot mapping, suffix mask, rope, layers_per_launch): every value of every axis at least twice, every pair of
# (rope, layers_per_launch) values once
COMBOS = [("offset5", False, None, 1), ("random", True, "uniform", (1, 2)), ("offset5", True, "per_token", 3),
          ("random", False, "per_token", 1), ("offset5", False, "uniform", 3), ("random", True, None, (1, 2)),
          ("random", False, "uniform", 1), ("offset5", True, "per_token", (1, 2)), ("random", False, None, 3)]


class _Count:
    """Counts the calls of Context.rope_shift / Context.copy_kv while it is active (the calls still go through)."""

    def __enter__(self):
        self.n = 0
        self.saved = (native.Context.rope_shift, native.Context.copy_kv)

        def counted(f):
            def g(*a, **k):
                self.n += 1
                return f(*a, **k)
            return g
        native.Context.rope_shift, native.Context.copy_kv = counted(self.saved[0]), counted(self.saved[1])
        return self

    def __exit__(self, *exc):
        native.Context.rope_shift, native.Context.copy_kv = self.saved


@pytest.mark.parametrize("backend", ["cachegen-hbm", "cachegen-host"])
def test_retrieve_into_paged_queues_each_post_op_once_behind_the_decode(backend, monkeypatch):
    """What retrieve_into_paged (not layer-wise) launches from Python behind its decode: at most one lmc_rope_shift over
    tokens [0, got) of the rows, then at most one lmc_copy_kv of [0, got) into the cache at token 0, neither on a miss.
    (The cache contents are held by the test below and by tests/test_gpu_rope_shift.py.)"""
    nl, H, D, bs, skip = 2, 2, 128, 16, 40
    dt = torch.bfloat16
    nb = 2 * ((NTOK + 5 + bs - 1) // bs) + 2
    g = torch.Generator().manual_seed(73)
    tokens = generate_tokens(NTOK, DEV)  # three chunks of CS tokens, the last one short
    kv = tuple((torch.rand((NTOK, H, D), generator=g).to(dt).to(DEV), torch.rand((NTOK, H, D), generator=g).to(dt).to(DEV))
               for _ in range(nl))
    uniform = RopeShift.from_base(10000.0, D, 128, DEV, delta=37)
    per_tok = torch.randint(-127, 128, (NTOK,), generator=g, dtype=torch.int32).to(DEV)
    by_token = RopeShift(uniform.cos_sin, D, True, per_tok)
    tail = torch.ones(NTOK, dtype=torch.bool, device=DEV)
    tail[:skip] = False  # cuts into the second chunk
    engine = LMCacheEngine(make_cfg(backend, CS), dumb_metadata("vllm", "Llama-3-8B"))
    ctx = native.get_context(0)
    calls = []

    def recording(name, real):
        def f(*a, **k):
            calls.append((name, a, k))
            return real(*a, **k)
        return f

    try:
        engine.store(tokens, kv)
        for name in ("rope_shift", "copy_kv"):  # on the context instance: the engine reaches both through its attributes
            monkeypatch.setattr(ctx, name, recording(name, getattr(ctx, name)))

        def run(layout, toks=tokens, **kw):
            shape = {"NBHD": (2, nb, bs, H, D), "NHDB": (2, nb, H, D, bs)}[layout]
            caches = [_random_bits(shape, dt, g).to(DEV) for _ in range(nl)]
            del calls[:]
            m = engine.retrieve_into_paged(toks, caches, _mapping("random", NTOK, nb, bs, g).to(DEV), bs, layout, **kw)
            torch.cuda.synchronize()
            return int(m.sum())

        def is_rows(layout):  # a chunk of token rows: not paged at all
            return layout.struct.paged_kind == native.PAGED_ROWS and not layout.struct.slot_mapping

        # staged "NHDB", a per-token delta, a suffix mask: one rotation of the staged rows, then their one scatter
        got = run("NHDB", mask=tail, rope=by_token)
        assert got == NTOK - skip
        assert [c[0] for c in calls] == ["rope_shift", "copy_kv"], calls
        (_, a, k), (_, b, kb) = calls
        assert is_rows(a[0]) and a[1:3] == (0, got) and a[3].data_ptr() == uniform.cos_sin.data_ptr() and a[4:6] == (D, True)
        assert k["delta"] == 0 and torch.equal(k["deltas"], per_tok[skip:skip + got])
        assert is_rows(b[0]) and b[1:3] == (0, got) and b[3].struct.paged_kind == native.PAGED_SPLIT and b[4] == 0 and not kb
        assert b[0].struct.base == a[0].struct.base  # the chunk that was rotated is the one that is scattered
        # direct, no rope: the decoder writes the split blocks, nothing is queued from Python
        assert run("NHDB", direct=True) == NTOK and calls == []
        # a row layout with a rope: the one rotation is on the paged cache itself, and nothing is scattered
        got = run("NBHD", mask=tail, rope=uniform)
        assert got == NTOK - skip and [c[0] for c in calls] == ["rope_shift"], calls
        _, a, k = calls[0]
        assert a[0].struct.paged_kind == native.PAGED_ROWS and a[0].struct.slot_mapping and a[1:3] == (0, got)
        assert k["delta"] == 37 and k["deltas"] is None
        # a miss: neither
        assert run("NHDB", toks=tokens + 10000, rope=by_token) == 0 and calls == []
        assert run("NBHD", toks=tokens + 10000, rope=uniform) == 0 and calls == []
        assert ctx.status(clear=True) == 0
    finally:
        engine.close()


@pytest.mark.parametrize("geom", [(2, 128, 16), (1, 64, 8)], ids=lambda g: "H%d_D%d_bs%d" % g)
@pytest.mark.parametrize("backend", ["cachegen-host", "cachegen-hbm", "cuda"])
def test_layerwise_equals_retrieve_into_paged_and_every_event_means_final(backend, geom):
    H, D, bs = geom
    dt, p = torch.bfloat16, 37
    nb = 2 * ((NTOK + 5 + bs - 1) // bs) + 2
    g = torch.Generator().manual_seed(71)
    tokens = generate_tokens(NTOK, DEV)
    kv = tuple((torch.rand((NTOK, H, D), generator=g).to(dt).to(DEV), torch.rand((NTOK, H, D), generator=g).to(dt).to(DEV))
               for _ in range(L))
    rot, neox = (D, True) if D == 128 else (32, False)  # full NeoX rotary; partial GPT-J rotary
    uniform = RopeShift.from_base(10000.0, rot, 128, DEV, is_neox=neox, delta=p)
    per_tok = torch.randint(-127, 128, (NTOK,), generator=g, dtype=torch.int32)
    ropes = {None: None, "uniform": uniform, "per_token": RopeShift(uniform.cos_sin, rot, neox, per_tok.to(DEV))}
    tail = torch.ones(NTOK, dtype=torch.bool, device=DEV)
    tail[:40] = False  # a suffix mask of 40 skipped tokens: cuts into the second chunk
    engine = LMCacheEngine(make_cfg(backend, CS), dumb_metadata("vllm", "Llama-3-8B"))
    ctx = native.get_context(0)
    s2 = torch.cuda.Stream(device=DEV)
    try:
        # the context in two store() calls, prefix first: the retrieve spans two stores (two packs: two decode jobs)
        engine.store(tokens[:CS], tuple((k[:CS], v[:CS]) for k, v in kv))
        engine.store(tokens, kv)

        def fresh(layout):
            shape = {"NBHD": (2, nb, bs, H, D), "NHBD": (2, nb, H, bs, D), "NHDB": (2, nb, H, D, bs)}[layout]
            return [_random_bits(shape, dt, g).to(DEV) for _ in range(L)]

        def into(caches, pair):
            return [(c[0].view(nb, H, D // 8, bs, 8), c[1]) for c in caches] if pair else caches

        for layout, pair, direct in LAYOUTS:
            for kind, masked, rope_kind, lpl in COMBOS:
                if direct and rope_kind is not None:
                    continue
                what = f"{layout} pair={pair} direct={direct} {kind} mask={masked} rope={rope_kind} lpl={lpl}"
                rope, mask = ropes[rope_kind], tail if masked else None
                slots = _mapping(kind, NTOK, nb, bs, g).to(DEV)
                a = fresh(layout)
                b = [c.clone() for c in a]
                untouched = [c.clone() for c in a]
                torch.cuda.synchronize()
                with _Count() as calls:
                    r = engine.retrieve_into_paged_layerwise(tokens, into(a, pair), slots, bs, layout, mask=mask, rope=rope,
                                                             direct=direct, layers_per_launch=lpl)
                if backend != "cuda":
                    assert calls.n == 0, f"{what}: {calls.n} post-ops were launched from Python"  # 5. the post-ops are in C
                # 4. behind wait_layer(l, s2), s2 sees layer l in its final state
                seen = []
                for l in range(L):
                    r.wait_layer(l, s2)
                    with torch.cuda.stream(s2):
                        seen.append(a[l].clone())
                assert r.kv == ()
                # 3. the events of every decode job: ascending, ending at L
                assert r._event_sets, what
                for events in r._event_sets:
                    ends = [end for end, _ in events]
                    assert ends == sorted(set(ends)) and ends[-1] == L, f"{what}: {ends}"
                if backend == "cachegen-hbm":
                    assert [end for end, _ in r.layer_events] == {1: [1, 2, 3], 3: [3]}.get(lpl, [1, 3]), what
                r.finish()
                mb = engine.retrieve_into_paged(tokens, into(b, pair), slots, bs, layout, mask=mask, rope=rope, direct=direct)
                torch.cuda.synchronize()
                nskip = 40 if masked else 0
                assert torch.equal(r.ret_mask, mb) and int(mb.sum()) == NTOK - nskip, what  # 2.
                for l in range(L):
                    assert torch.equal(_ibits(a[l]), _ibits(b[l])), f"{what}: layer {l} differs from retrieve_into_paged"  # 1.
                    assert torch.equal(_ibits(seen[l]), _ibits(a[l])), f"{what}: layer {l} was not final behind its event"
                    assert not torch.equal(_ibits(a[l]), _ibits(untouched[l])), f"{what}: nothing was retrieved"
            # 6. tokens the engine has never seen: an all-False mask, no events, every byte kept
            c = fresh(layout)
            keep = [x.clone() for x in c]
            r = engine.retrieve_into_paged_layerwise(tokens + 10000, into(c, pair), _mapping("random", NTOK, nb, bs, g).to(DEV), bs,
                                                     layout, rope=None if direct else uniform, direct=direct)
            r.wait_layer(0)
            r.finish()
            torch.cuda.synchronize()
            assert not r.ret_mask.any() and r.kv == () and not r.layer_events
            assert all(torch.equal(_ibits(x), _ibits(y)) for x, y in zip(c, keep))
        # 7. / 8. refused before anything is queued
        c = fresh("NHDB")
        keep = [x.clone() for x in c]
        slots = _mapping("random", NTOK, nb, bs, g).to(DEV)
        with pytest.raises(ValueError, match="direct"):
            engine.retrieve_into_paged_layerwise(tokens, c, slots, bs, "NHDB", rope=uniform, direct=True)
        fp8 = [torch.zeros((2, nb, bs, H, D), dtype=torch.uint8, device=DEV).view(torch.float8_e4m3fn) for _ in range(L)]
        with pytest.raises(ValueError, match="fp8"):
            engine.retrieve_into_paged_layerwise(tokens, fp8, slots, bs, "NBHD", rope=uniform)
        torch.cuda.synchronize()
        assert all(torch.equal(_ibits(x), _ibits(y)) for x, y in zip(c, keep))
        assert all(int(x.view(torch.uint8).max()) == 0 for x in fp8)
        assert ctx.status(clear=True) == 0  # 9.
    finally:
        engine.close()
