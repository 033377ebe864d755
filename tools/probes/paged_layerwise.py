"""retrieve_into_paged_layerwise on one 16 k Llama-3-8B context (L 32, H 8, D 128, block 16, bf16, block-ordered slots),
one process, medians of RUNS runs behind a clock ramp:

  (c) two_launches_ms       lmc_rope_shift on the chunk + lmc_copy_kv chunk -> NHDB cache, uniform and per-token deltas, and
      rope_alone / scatter_alone  each of the two by itself (HIP events): what a range's post-op costs for NHDB + rope, and
                            the yardstick a scatter that rotates on the way has to beat (the one that was built did not:
                            profiles/paged_layerwise.md)
  (a) layer0_ms / last_ms   host clock from the call to the completion of the first / the last range's event, per tier
                            (HBM-resident CacheGen tier "hbm", pinned packs "pinned"), layout (NBHD, NHDB + rope) and
                            schedule (layers_per_launch 1, (2, 6, 24), 8)
  (b) one_shot_ms           retrieve_into_paged with the same arguments + synchronize, same process

    python tools/probes/paged_layerwise.py [out.json]
"""
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__)))))
from lmcache_amd import native  # noqa: E402
from lmcache_amd.rope import RopeShift  # noqa: E402

RUNS = 15
L, H, D, T, BS = 32, 8, 128, 16384, 16
MODEL = "Llama-3-8B"
SCHEDULES = {"1": 1, "2_6_24": (2, 6, 24), "8": 8}


def timed(fn, runs=RUNS):
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def main():
    dev = torch.device("cuda:0")
    ctx = native.get_context(0)
    g = torch.Generator().manual_seed(0)
    nb = T // BS + 64
    chunk = torch.randn(L, 2, T, H, D, device=dev).to(torch.bfloat16)
    split = [torch.zeros((2, nb, H, D, BS), dtype=torch.bfloat16, device=dev) for _ in range(L)]
    blocks = torch.randperm(nb, generator=g)[:T // BS]
    pos = torch.arange(T)
    ordered = (blocks[pos // BS] * BS + pos % BS).to(dev)
    src, dst = native.KVLayout.from_chunk(chunk, "vllm"), native.KVLayout.paged(split, ordered, BS, "NHDB")
    rope = RopeShift.from_base(500000.0, D, 32768, dev, delta=4096)
    deltas = torch.randint(-8192, 8192, (T,), generator=g, dtype=torch.int32).to(dev)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.5:  # ramp the clock
        ctx.copy_kv(src, 0, T, dst, 0)
    torch.cuda.synchronize()
    out = {"runs": RUNS}
    for tag, kw in (("uniform", dict(delta=4096)), ("per_token", dict(deltas=deltas))):
        def two():
            ctx.rope_shift(src, 0, T, rope.cos_sin, D, True, **kw)
            ctx.copy_kv(src, 0, T, dst, 0)
        out[f"two_launches_{tag}_ms"] = timed(two)
        out[f"rope_alone_{tag}_ms"] = timed(lambda: ctx.rope_shift(src, 0, T, rope.cos_sin, D, True, **kw))
    out["scatter_alone_ms"] = timed(lambda: ctx.copy_kv(src, 0, T, dst, 0))

    from lmcache_amd.cache_engine import LMCacheEngine
    from lmcache_amd.config import LMCacheEngineConfig, LMCacheEngineMetadata
    tokens = torch.randint(0, 30000, (T,), generator=g).to(dev)
    kv = tuple(tuple(l.unbind(0)) for l in torch.randn(L, 2, T, H, D, device=dev).to(torch.bfloat16).unbind(0))
    nbhd = [torch.zeros((2, nb, BS, H, D), dtype=torch.bfloat16, device=dev) for _ in range(L)]
    for tier, cfg in (("hbm", dict(backend="cuda", local_serde="cachegen")), ("pinned", dict(backend="cpu", local_serde="cachegen"))):
        eng = LMCacheEngine(LMCacheEngineConfig.from_legacy(chunk_size=256, **cfg), LMCacheEngineMetadata(MODEL, 1, 0, "vllm", "half"))
        eng.store(tokens, kv)
        torch.cuda.synchronize()
        for name, caches, layout, rp in (("nbhd", nbhd, "NBHD", None), ("nhdb_rope", split, "NHDB", rope)):
            def one_shot():
                t0 = time.perf_counter()
                eng.retrieve_into_paged(tokens, caches, ordered, BS, layout, rope=rp)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3
            one = [one_shot() for _ in range(RUNS + 2)][2:]
            out[f"{tier}_{name}_one_shot_ms"] = statistics.median(one)
            for sname, sched in SCHEDULES.items():
                first, last = [], []
                for _ in range(RUNS + 2):
                    t0 = time.perf_counter()
                    r = eng.retrieve_into_paged_layerwise(tokens, caches, ordered, BS, layout, rope=rp, layers_per_launch=sched)
                    events = r._event_sets[-1]
                    events[0][1].synchronize()
                    t1 = time.perf_counter()
                    events[-1][1].synchronize()
                    t2 = time.perf_counter()
                    r.finish()
                    first.append((t1 - t0) * 1e3)
                    last.append((t2 - t0) * 1e3)
                out[f"{tier}_{name}_lpl{sname}_layer0_ms"] = statistics.median(first[2:])
                out[f"{tier}_{name}_lpl{sname}_last_ms"] = statistics.median(last[2:])
                out[f"{tier}_{name}_lpl{sname}_ranges"] = len(events)
        eng.close()
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(line + "\n")


if __name__ == "__main__":
    main()
