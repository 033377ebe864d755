"""retrieve(..., stored_world_size=W) and stored_at(W).retrieve_into_paged(...): KV stored by the ranks of one
tensor-parallel degree, retrieved by the ranks of another.  ONE backend object is shared by engines whose metadata differ in
(world_size, worker_id) -- the instances of a node sharing a store.

Bit-exact throughout, against the path that existed before: what a storing engine's own retrieve() returns, sliced (or
concatenated) along the heads with torch.  (Not against the raw KV: a stored chunk is quantised per shard, so KV stored by
four TP = 4 ranks decodes to what THOSE four blobs hold.)  On the coded HBM tier, the fixed-width tier, the pinned tier, and
the pipelined remote backend with the CacheGen serde -- over a host store and over the device store (xgmi://)."""
import pytest
import torch

from lmcache_amd.cache_engine import LMCacheEngine
from lmcache_amd.config import LMCacheEngineConfig, LMCacheEngineMetadata
from lmcache_amd.rope import RopeShift
from tests.test_gpu_engine import make_cfg
from tests.test_gpu_paged_split import DEV, _ibits, _mapping, _nblocks, _random, _torch_scatter

pytestmark = pytest.mark.gpu

MODEL = "Llama-3-8B"
L, H, D, NTOK, CS, BS = 2, 8, 64, 70, 32, 16
DT = torch.bfloat16
TIERS = {"hbm": ("cuda", "cachegen"), "fixed": ("cuda", "cachegen-fixed"), "pinned": ("cpu", "cachegen"),
         "remote": "mem://hwpipe:1", "xgmi": "xgmi://hwpipe:1"}


def _meta(world, rank):
    return LMCacheEngineMetadata(MODEL, world, rank, "vllm", "half")


@pytest.fixture(params=list(TIERS))
def base(request):
    """The TP = 1 engine; it owns the backend every other engine of the test shares."""
    tier = TIERS[request.param]
    cfg = make_cfg(tier, CS) if isinstance(tier, str) else LMCacheEngineConfig.from_legacy(chunk_size=CS, backend=tier[0],
                                                                                          local_serde=tier[1])
    e = LMCacheEngine(cfg, _meta(1, 0))
    yield e
    e.close()


def _rank(base, world, rank):
    """An engine of rank `rank` of a TP = `world` instance on the backend of `base`."""
    e = LMCacheEngine.__new__(LMCacheEngine)
    e.__dict__.update({k: v for k, v in base.__dict__.items() if k not in ("_hash_chain", "_key_memo")})
    e.metadata = _meta(world, rank)
    return e


def _kv(seed=3):
    g = torch.Generator().manual_seed(seed)
    tokens = torch.randint(0, 10000, (NTOK,), generator=g).to(DEV)
    kv = tuple((torch.rand((NTOK, H, D), generator=g).to(DT).to(DEV), torch.rand((NTOK, H, D), generator=g).to(DT).to(DEV))
               for _ in range(L))
    return tokens, kv


def _heads(kv, h0, h1):
    return tuple((k[:, h0:h1].contiguous(), v[:, h0:h1].contiguous()) for k, v in kv)


def _bits(kv):
    """[L, 2, T, h, D] integer view of a per-layer (K, V) tuple."""
    return _ibits(torch.stack([torch.stack([k, v]) for k, v in kv]))


def _same_kv(got, want, what):
    assert len(got) == len(want) == L, what
    assert torch.equal(_bits(got), _bits(want)), what


def _paged_check(engine, tokens, want_bits, layout, direct, g, mask=None, rope=None, stored_world_size=None):
    """retrieve_into_paged into a cache of random bits with want_bits.shape[3] heads; the WHOLE cache afterwards equals
    a clone with want_bits [L, 2, T', h, D] placed by torch indexing at the slots of the retrieved tokens."""
    h, nb = want_bits.shape[3], _nblocks(BS)
    shape = (2, nb, BS, h, D) if layout == "NBHD" else (2, nb, h, D, BS)
    caches = [_random(shape, DT, g).to(DEV) for _ in range(L)]
    expect = [c.clone() for c in caches]
    slots = _mapping("random" if layout == "NBHD" else "blocks", NTOK, nb, BS, g).to(DEV)
    m = engine.stored_at(stored_world_size).retrieve_into_paged(tokens, caches, slots, BS, layout, mask=mask, rope=rope, direct=direct)
    torch.cuda.synchronize()
    nskip = 0 if mask is None else int((~mask).sum())
    got = int(m.sum())
    assert got == want_bits.shape[2] and not m[:nskip].any() and m[nskip:nskip + got].all()
    s = slots[nskip:nskip + got]
    if layout == "NBHD":
        for c, layer in zip(expect, want_bits):
            _ibits(c)[0, s // BS, s % BS] = layer[0]
            _ibits(c)[1, s // BS, s % BS] = layer[1]
    else:
        _torch_scatter(expect, want_bits, s, BS)
    for l in range(L):
        assert torch.equal(_ibits(caches[l]), _ibits(expect[l])), f"{layout} direct={direct}: layer {l}"
    return caches


# ------------------------------------------------------------------ stored at TP = 1, retrieved at TP = 2 and TP = 4
def test_a_tp1_store_serves_the_ranks_of_tp2_and_tp4(base):
    tokens, kv = _kv()
    base.store(tokens, kv)
    full, m = base.retrieve(tokens)
    assert int(m.sum()) == NTOK
    mask = torch.ones(NTOK, dtype=torch.bool, device=DEV)
    mask[:37] = False  # a suffix mask that cuts into the second chunk: the first-chunk trim
    full_tail, _ = base.retrieve(tokens, mask)
    g = torch.Generator().manual_seed(5)
    for world in (2, 4):
        per = H // world
        for rank in range(world):
            e = _rank(base, world, rank)
            got, m = e.retrieve(tokens, stored_world_size=1)
            assert int(m.sum()) == NTOK and got[0][0].shape == (NTOK, per, D)
            again, m2 = e.stored_at(1).retrieve(tokens)  # the keyword is the view
            assert torch.equal(m, m2) and torch.equal(_bits(again), _bits(got))
            _same_kv(got, _heads(full, rank * per, (rank + 1) * per), f"TP={world} rank {rank}")
            # its own degree is the call it always was: nothing of this rank's own is stored
            assert e.retrieve(tokens)[0] == () and e.retrieve(tokens, stored_world_size=world)[0] == ()
        rank = world - 1
        e = _rank(base, world, rank)
        got, m = e.retrieve(tokens, mask, stored_world_size=1)
        assert int(m.sum()) == NTOK - 37 and not m[:37].any()
        _same_kv(got, _heads(full_tail, rank * per, (rank + 1) * per), f"TP={world} rank {rank}, suffix mask")
        want = _bits(_heads(full, rank * per, (rank + 1) * per))
        for layout, direct in (("NBHD", False), ("NHDB", False), ("NHDB", True)):
            _paged_check(e, tokens, want, layout, direct, g, stored_world_size=1)
        _paged_check(e, tokens, want[:, :, 37:], "NHDB", True, g, mask=mask, stored_world_size=1)


# ------------------------------------------------------------------ stored at TP = 4, retrieved at TP = 1 and TP = 2
def _store_tp4(base, tokens, kv, short_rank=None):
    """Four TP = 4 engines store their two heads each; -> what each of them retrieves of its own store."""
    parts = []
    for rank in range(4):
        e = _rank(base, 4, rank)
        n = 64 if rank == short_rank else NTOK  # (the first two chunks of the same prefix: the same keys)
        e.store(tokens[:n], tuple((k[:n], v[:n]) for k, v in _heads(kv, 2 * rank, 2 * rank + 2)))
        got, m = e.retrieve(tokens[:n])
        assert int(m.sum()) == n
        parts.append(got)
    return parts


def _cat(parts, n=NTOK):
    return tuple((torch.cat([p[l][0][:n] for p in parts], dim=1), torch.cat([p[l][1][:n] for p in parts], dim=1)) for l in range(L))


def test_four_tp4_stores_assemble_at_tp1_and_tp2(base):
    tokens, kv = _kv(seed=9)
    parts = _store_tp4(base, tokens, kv)
    got, m = base.retrieve(tokens, stored_world_size=4)
    assert int(m.sum()) == NTOK and got[0][0].shape == (NTOK, H, D)
    _same_kv(got, _cat(parts), "TP=1 from four TP=4 shards")
    for rank in range(2):
        got, m = _rank(base, 2, rank).retrieve(tokens, stored_world_size=4)
        assert int(m.sum()) == NTOK
        _same_kv(got, _cat(parts[2 * rank:2 * rank + 2]), f"TP=2 rank {rank} from two TP=4 shards")
    g = torch.Generator().manual_seed(15)
    for layout, direct in (("NBHD", False), ("NHDB", False), ("NHDB", True)):
        _paged_check(base, tokens, _bits(_cat(parts)), layout, direct, g, stored_world_size=4)


def test_a_shard_whose_last_chunk_is_missing_shortens_the_prefix(base):
    tokens, kv = _kv(seed=13)
    parts = _store_tp4(base, tokens, kv, short_rank=2)
    got, m = base.retrieve(tokens, stored_world_size=4)
    assert int(m.sum()) == 64 and m[:64].all() and not m[64:].any()
    assert got[0][0].shape == (64, H, D)
    _same_kv(got, _cat(parts, 64), "two whole chunks of every shard")
    # the TP = 2 rank whose shards are complete still gets everything; the other one the shorter prefix
    got, m = _rank(base, 2, 0).retrieve(tokens, stored_world_size=4)
    assert int(m.sum()) == NTOK
    _same_kv(got, _cat(parts[0:2]), "complete shards")
    got, m = _rank(base, 2, 1).retrieve(tokens, stored_world_size=4)
    assert int(m.sum()) == 64 and not m[64:].any()
    _same_kv(got, _cat(parts[2:4], 64), "one short shard")
    g = torch.Generator().manual_seed(19)
    _paged_check(base, tokens, _bits(_cat(parts, 64)), "NHDB", False, g, stored_world_size=4)
    # stored at a degree nobody stored at: a miss, an all-False mask
    got, m = base.retrieve(tokens, stored_world_size=2)
    assert got == () and not m.any()


# ------------------------------------------------------------------ with a rotation
@pytest.mark.parametrize("layout", ["NBHD", "NHDB"])
def test_rope_on_a_resharded_retrieve_is_the_rotation_of_the_slice(base, layout):
    """The rotation acts per head, so the slice of a rotated TP = 1 retrieve is the rotation of the slice; it is queued
    once, behind the last source's window -- two sources here (a TP = 2 rank reads two TP = 4 shards)."""
    tokens, kv = _kv(seed=21)
    parts = _store_tp4(base, tokens, kv)
    g = torch.Generator().manual_seed(23)
    delta = torch.randint(-40, 41, (NTOK,), generator=g, dtype=torch.int32)
    for d in (11, delta):
        rope = RopeShift.from_base(10000.0, D, 128, DEV, delta=d)
        # the reference: each TP = 4 rank's own rotated retrieve into a cache of its own (zeros), then the heads side by side
        nb = _nblocks(BS)
        slots = _mapping("blocks", NTOK, nb, BS, g).to(DEV)
        own = []
        for rank in (2, 3):
            shape = (2, nb, BS, 2, D) if layout == "NBHD" else (2, nb, 2, D, BS)
            caches = [torch.zeros(shape, dtype=DT, device=DEV) for _ in range(L)]
            m = _rank(base, 4, rank).retrieve_into_paged(tokens, caches, slots, BS, layout, rope=rope)
            assert int(m.sum()) == NTOK
            own.append(caches)
        hdim = 3 if layout == "NBHD" else 2
        want = [torch.cat([own[0][l], own[1][l]], dim=hdim) for l in range(L)]
        got = [torch.zeros_like(w) for w in want]
        m = _rank(base, 2, 1).stored_at(4).retrieve_into_paged(tokens, got, slots, BS, layout, rope=rope)
        torch.cuda.synchronize()
        assert int(m.sum()) == NTOK
        for l in range(L):
            assert torch.equal(_ibits(got[l]), _ibits(want[l])), f"{layout}: layer {l}"
        # ... and it did rotate: the keys differ from the unrotated retrieve, the values do not
        plain = [torch.zeros_like(w) for w in want]
        _rank(base, 2, 1).stored_at(4).retrieve_into_paged(tokens, plain, slots, BS, layout)
        torch.cuda.synchronize()
        assert not torch.equal(_ibits(plain[0][0]), _ibits(got[0][0])) and torch.equal(_ibits(plain[0][1]), _ibits(got[0][1]))
