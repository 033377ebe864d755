"""Time of lmc_rope_shift_split (k_rope.h: k_rope_split_vec) on one 16 k Llama-3-8B context (L = 32, H = 8, D = rot = 128,
bf16, block size 16, block-ordered slots) against its yardstick, and of the whole retrieve_into_paged(rope=...) of that
context, staged against direct + in place.  HIP events, one process, medians of RUNS runs behind a clock ramp.

  pass       lmc_rope_shift_split of all 16 k tokens in an "NHDB" cache, one delta and per-token deltas
  yardstick  lmc_rope_shift (unchanged code) of the same tokens in a block-ordered "NHBD" cache of the same context: the
             same bytes.  The four legs are timed ALTERNATING, run by run
  ratio      pass / yardstick; above 1.25 is a finding (profiles/rope_shift.md)
  retrieve   engine.retrieve_into_paged(tokens, "NHDB" caches, rope=...) of the stored context, one delta and per-token
             deltas, from the call to the end of its last kernel: direct=False (a staged chunk, the rotation there, the
             scatter) against direct=True of an engine built with LMCACHE_AMD_SPLIT_ROPE=1 (decode into the split blocks,
             the rotation there), on the coded and on the fixed-width HBM tier; the peak device allocation across each
             call beside it

The result of every timed pass is also checked, on the device, against the formula in torch (separate fp32 ops), and the
two retrieves against each other, bit for bit.

    python tools/probes/rope_split_rates.py [out.json] [--pass-only]

LMCACHE_AMD_SO=<another build> times that build instead (e.g. one compiled with -DLMC_ROPE_SPLIT_NT=1: non-temporal
instead of plain loads and stores in k_rope_split_vec); --pass-only leaves the retrieves out."""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from lmcache_amd import native  # noqa: E402
from lmcache_amd.cache_engine import LMCacheEngine  # noqa: E402
from lmcache_amd.config import LMCacheEngineConfig, LMCacheEngineMetadata  # noqa: E402
from lmcache_amd.rope import RopeShift  # noqa: E402

RUNS = 30
L, H, D, T, BS = 32, 8, 128, 16384, 16
ROWS = 32768
CHUNK = 256


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def torch_shift(k, table, deltas):
    """k [..., T, H, D] on the device, rotated by deltas [T] (NeoX, rot = D): the header's formula, one op per step."""
    x = k.float()
    h = D // 2
    c = table[deltas.abs().long(), :h][:, None, :]
    s = table[deltas.abs().long(), h:][:, None, :] * torch.where(deltas < 0, -1.0, 1.0)[:, None, None]
    x1, x2 = x[..., :h], x[..., h:]
    a, b = x1 * c, x2 * s
    o1 = a - b
    a, b = x2 * c, x1 * s
    o2 = a + b
    return torch.cat((o1, o2), dim=-1).to(k.dtype)


def the_pass(out, dev, ctx, table):
    deltas = torch.randint(-(ROWS - 1), ROWS, (T,), dtype=torch.int32).to(dev)
    uniform = torch.full((T,), 4097, dtype=torch.int32, device=dev)
    nb = T // BS
    slots = (torch.randperm(nb)[:, None] * BS + torch.arange(BS)[None, :]).reshape(-1).to(dev)  # block-ordered, blocks shuffled
    blk, off = slots // BS, slots % BS
    nhbd = [torch.randn(2, nb, H, BS, D, device=dev).to(torch.bfloat16) for _ in range(L)]
    nhdb = [torch.randn(2, nb, H, D, BS, device=dev).to(torch.bfloat16) for _ in range(L)]
    rows = native.KVLayout.paged(nhbd, slots, BS, "NHBD")
    split = native.KVLayout.paged(nhdb, slots, BS, "NHDB")

    def split_keys():
        return torch.stack([c[0].view(nb, H, D // 8, BS, 8)[blk, :, :, off].reshape(T, H, D) for c in nhdb])

    legs = {
        "split_uniform_ms": lambda: ctx.rope_shift_split(split, 0, T, table, D, True, delta=4097),
        "nhbd_uniform_ms": lambda: ctx.rope_shift(rows, 0, T, table, D, True, delta=4097),
        "split_per_token_ms": lambda: ctx.rope_shift_split(split, 0, T, table, D, True, deltas=deltas),
        "nhbd_per_token_ms": lambda: ctx.rope_shift(rows, 0, T, table, D, True, deltas=deltas),
    }
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.5:  # ramp the clock
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in legs}
    for _ in range(RUNS):  # alternating: a drift of the clock falls on all four alike
        for name, fn in legs.items():
            ms[name].append(once(fn))
    r = {name: statistics.median(v) for name, v in ms.items()}
    r["ratio_uniform"] = r["split_uniform_ms"] / r["nhbd_uniform_ms"]
    r["ratio_per_token"] = r["split_per_token_ms"] / r["nhbd_per_token_ms"]
    k_bytes = L * T * H * D * 2
    r["split_uniform_GBps"] = 2 * k_bytes / r["split_uniform_ms"] / 1e6  # K read once and written once
    r["nhbd_uniform_GBps"] = 2 * k_bytes / r["nhbd_uniform_ms"] / 1e6
    for name, d, fn in (("uniform", uniform, legs["split_uniform_ms"]), ("per_token", deltas, legs["split_per_token_ms"])):
        before = split_keys()
        values = [c[1].clone() for c in nhdb[:2]]
        fn()
        torch.cuda.synchronize()
        r["bit_equal_to_torch_" + name] = bool(torch.equal(split_keys().view(torch.int16), torch_shift(before, table, d).view(torch.int16))
                                               and all(torch.equal(v.view(torch.int16), c[1].view(torch.int16)) for v, c in zip(values, nhdb)))
    out["pass"] = r
    out["k_bytes"] = k_bytes


def the_retrieves(out, dev, rope):
    torch.manual_seed(1)
    tokens = torch.randint(0, 10000, (T,)).to(dev)
    kv = tuple((torch.rand((T, H, D), device=dev).to(torch.bfloat16), torch.rand((T, H, D), device=dev).to(torch.bfloat16))
               for _ in range(L))
    nb = T // BS
    slots = (torch.randperm(nb)[:, None] * BS + torch.arange(BS)[None, :]).reshape(-1).to(dev)
    meta = LMCacheEngineMetadata("Llama-3-8B", 1, 0, "vllm", "half")
    per_token = torch.randint(-(ROWS - 1), ROWS, (T,), dtype=torch.int32).to(dev)
    ropes = {"one_delta": rope, "per_token": RopeShift(rope.cos_sin, D, True, per_token)}
    out["retrieve"] = {"kv_bytes": 2 * L * T * H * D * 2, "chunk_tokens": CHUNK}
    for tier, serde in (("coded", "cachegen"), ("fixed", "cachegen-fixed")):
        os.environ["LMCACHE_AMD_SPLIT_ROPE"] = "1"  # (read when the engine is built)
        engine = LMCacheEngine(LMCacheEngineConfig.from_legacy(chunk_size=CHUNK, backend="cuda", local_serde=serde), meta)
        del os.environ["LMCACHE_AMD_SPLIT_ROPE"]
        try:
            engine.store(tokens, kv)
            torch.cuda.synchronize()
            caches = {d: [torch.zeros(2, nb, H, D, BS, device=dev, dtype=torch.bfloat16) for _ in range(L)] for d in (False, True)}

            for deltas_name, rp in ropes.items():
                def call(direct):
                    m = engine.retrieve_into_paged(tokens, caches[direct], slots, BS, "NHDB", rope=rp, direct=direct)
                    assert bool(m.all())

                t0 = time.perf_counter()
                while time.perf_counter() - t0 < 0.5:  # ramp the clock, and whatever the tier keeps across calls is there
                    call(False), call(True)
                torch.cuda.synchronize()
                ms, wall = {False: [], True: []}, {False: [], True: []}
                for _ in range(RUNS):
                    for direct in (False, True):
                        torch.cuda.synchronize()
                        w0 = time.perf_counter()
                        ms[direct].append(once(lambda: call(direct)))
                        wall[direct].append((time.perf_counter() - w0) * 1e3)
                r = {}
                for direct, name in ((False, "staged"), (True, "direct_in_place")):
                    r[name + "_ms"] = statistics.median(ms[direct])
                    r[name + "_wall_ms"] = statistics.median(wall[direct])
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    before = torch.cuda.memory_allocated()
                    call(direct)
                    torch.cuda.synchronize()
                    r[name + "_peak_bytes"] = torch.cuda.max_memory_allocated() - before
                r["ratio"] = r["direct_in_place_ms"] / r["staged_ms"]
                r["bit_equal"] = all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(caches[False], caches[True]))
                out["retrieve"].setdefault(tier, {})[deltas_name] = r
            del caches
        finally:
            engine.close()
        torch.cuda.empty_cache()


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    dev = torch.device("cuda:0")
    ctx = native.get_context(0)
    torch.manual_seed(0)
    rope = RopeShift.from_base(500000.0, D, ROWS, dev, is_neox=True, delta=4097)
    out = {"runs": RUNS, "shape": {"L": L, "H": H, "D": D, "rot": D, "tokens": T, "dtype": "bf16", "block_size": BS},
           "library": native.SO_PATH}
    the_pass(out, dev, ctx, rope.cos_sin)
    torch.cuda.empty_cache()
    if "--pass-only" not in sys.argv:
        the_retrieves(out, dev, rope)
    ctx.raise_on_status("rope split probe")
    line = json.dumps(out)
    print(line)
    if args:
        open(args[0], "w").write(line + "\n")


if __name__ == "__main__":
    main()
