"""LMCACHE_AMD_FUSED_ROPE=1 on local_serde="cachegen-fixed": retrieve_into_paged / retrieve_into_paged_layerwise with
`rope` rotate the keys inside the fixed-width decode.  Against the same engine's calls with the switch off: ret_mask
equal, V planes bit-equal, and every key within 2 B + 2.25 u r of the two-pass key -- B the one-rounding bound of
tests/test_gpu_fused_rope.py, 2.25 u r the two-pass path's (tests/test_rope_host.py), both around the same exact value."""
import numpy as np
import pytest
import torch

from lmcache_amd import native
from lmcache_amd.cache_engine import LMCacheEngine
from lmcache_amd.config import LMCacheEngineConfig
from lmcache_amd.rope import RopeShift
from tests.test_gpu_engine import dumb_metadata, generate_tokens
from tests.test_gpu_fused_rope import BF16, bound, exact_keys, rotated

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CS, NTOK, L, H, BS, ROWS = 32, 80, 4, 2, 16, 128
NB = (NTOK + BS - 1) // BS + 2
MODES = [("NHDB", True), ("NHDB", False), ("NHBD", False)]  # (layout, direct)


def _engine(monkeypatch, on):
    monkeypatch.delenv("LMCACHE_AMD_SPLIT_ROPE", raising=False)
    monkeypatch.setenv("LMCACHE_AMD_FUSED_ROPE", "1" if on else "0")
    native.build()
    cfg = LMCacheEngineConfig.from_legacy(chunk_size=CS, backend="cuda", local_serde="cachegen-fixed")
    eng = LMCacheEngine(cfg, dumb_metadata("vllm", "Llama-3-8B"))
    assert eng.fused_rope == on
    return eng


def _setup(monkeypatch, D, seed):
    g = torch.Generator().manual_seed(seed)
    tokens = generate_tokens(NTOK, DEV)
    kv = tuple((torch.rand((NTOK, H, D), generator=g).to(BF16).to(DEV), torch.rand((NTOK, H, D), generator=g).to(BF16).to(DEV))
               for _ in range(L))
    engines = [_engine(monkeypatch, on) for on in (False, True)]
    for e in engines:
        e.store(tokens, kv)
    deltas = torch.randint(-(ROWS - 1), ROWS, (NTOK,), generator=g, dtype=torch.int32)
    rope = RopeShift.from_base(10000.0, D, ROWS, DEV, is_neox=True, delta=deltas.to(DEV))
    slots = torch.randperm(NB * BS, generator=g)[:NTOK].to(DEV)
    return g, tokens, kv, engines, deltas, rope, slots


def _fresh(layout, D, g):
    shape = (2, NB, H, D, BS) if layout == "NHDB" else (2, NB, H, BS, D)
    return [torch.randint(-2 ** 15, 2 ** 15, shape, generator=g, dtype=torch.int16).view(BF16).to(DEV) for _ in range(L)]


def _tokens(caches, layout, slots, D):
    """[L, 2, NTOK, H, D] out of the paged caches."""
    b, w = slots // BS, slots % BS
    if layout == "NHBD":
        return torch.stack([c[:, b, :, w].transpose(0, 1) for c in caches])
    return torch.stack([torch.stack([c[0].view(NB, H, D // 8, BS, 8)[b, :, :, w].reshape(NTOK, H, D), c[1][b, :, :, w]]) for c in caches])


@pytest.mark.parametrize("layout,direct", MODES, ids=["NHDB-direct", "NHDB-staged", "NHBD"])
def test_fused_retrieves_stay_within_both_paths_bounds_of_the_two_pass_ones(monkeypatch, oracle, layout, direct):
    D = 64
    g, tokens, kv, (off, on), deltas, rope, slots = _setup(monkeypatch, D, 11 + MODES.index((layout, direct)))
    try:
        start = _fresh(layout, D, g)
        want = [c.clone() for c in start]
        m_off = off.retrieve_into_paged(tokens, want, slots, BS, layout, rope=rope, direct=direct)
        plain = [c.clone() for c in start]
        off.retrieve_into_paged(tokens, plain, slots, BS, layout)
        torch.cuda.synchronize()
        ref = _tokens(want, layout, slots, D)
        # the exact value both paths round: the engine's bins are held to the reference through the unrotated decode
        x = exact_keys(oracle, torch.stack([torch.stack(p) for p in kv]).cpu(), [32] * L)
        assert torch.equal(torch.from_numpy(x).to(BF16).view(torch.int16), _tokens(plain, layout, slots, D)[:, 0].cpu().view(torch.int16))
        e, mag = rotated(x, rope.cos_sin.cpu().numpy(), deltas.numpy().astype(np.int64), D, True)
        half = D // 2
        r = np.sqrt(x[..., :half].astype(np.float64) ** 2 + x[..., half:].astype(np.float64) ** 2)
        lim = 2 * bound(e, mag, BF16) + 2.25 * 2.0 ** -8 * np.concatenate([r, r], axis=-1)

        def check(caches, mask, what):
            got = _tokens(caches, layout, slots, D)
            assert torch.equal(mask, m_off) and mask.all(), what
            assert torch.equal(got[:, 1].view(torch.int16), ref[:, 1].view(torch.int16)), what + ": V planes"
            err = np.abs(got[:, 0].double().cpu().numpy() - ref[:, 0].double().cpu().numpy())
            print(f"{what}: worst |fused - two-pass| / bound = {(err[lim > 0] / lim[lim > 0]).max():.3f}")
            assert (err <= lim).all(), what
            assert not torch.equal(got[:, 0].view(torch.int16), plain_k), what + ": the keys were not rotated"
            assert not torch.equal(got[:, 0].view(torch.int16), ref[:, 0].view(torch.int16)), what + ": two-pass bits, not the fused decode's"

        plain_k = _tokens(plain, layout, slots, D)[:, 0].view(torch.int16)
        a = [c.clone() for c in start]
        check(a, on.retrieve_into_paged(tokens, a, slots, BS, layout, rope=rope, direct=direct), "one piece")
        for lpl in ((1, 3), 3):
            c = [x_.clone() for x_ in start]
            rr = on.retrieve_into_paged_layerwise(tokens, c, slots, BS, layout, rope=rope, direct=direct, layers_per_launch=lpl)
            rr.finish()
            torch.cuda.synchronize()
            check(c, rr.ret_mask, f"layer-wise {lpl}")
        assert native.get_context(0).status(clear=True) == 0
    finally:
        off.close()
        on.close()


def test_a_layers_event_says_rotated_and_head_size_96_takes_the_two_passes(monkeypatch):
    """A copy of layer 0 behind wait_layer(0) on a side stream is layer 0 after finish(); with D = 96, which the fused form
    does not serve, the switch changes no bit."""
    g, tokens, kv, (off, on), deltas, rope, slots = _setup(monkeypatch, 64, 21)
    try:
        got = _fresh("NHDB", 64, g)
        early, side = torch.zeros_like(got[0]), torch.cuda.Stream(device=DEV)
        torch.cuda.synchronize()
        r = on.retrieve_into_paged_layerwise(tokens, got, slots, BS, "NHDB", rope=rope, direct=True, layers_per_launch=(1, 3))
        r.wait_layer(0, side)
        with torch.cuda.stream(side):
            early.copy_(got[0], non_blocking=True)
        r.finish()
        torch.cuda.synchronize()
        assert torch.equal(early.view(torch.int16), got[0].view(torch.int16)), "layer 0 behind its event is not final"
    finally:
        off.close()
        on.close()
    g, tokens, kv, (off, on), deltas, rope, slots = _setup(monkeypatch, 96, 22)
    try:
        start = _fresh("NHDB", 96, g)
        for direct in (True, False):
            a, b = [c.clone() for c in start], [c.clone() for c in start]
            ma = off.retrieve_into_paged(tokens, a, slots, BS, "NHDB", rope=rope, direct=direct)
            mb = on.retrieve_into_paged(tokens, b, slots, BS, "NHDB", rope=rope, direct=direct)
            torch.cuda.synchronize()
            assert torch.equal(ma, mb) and ma.all()
            assert all(torch.equal(x.view(torch.int16), y.view(torch.int16)) for x, y in zip(a, b))
    finally:
        off.close()
        on.close()
