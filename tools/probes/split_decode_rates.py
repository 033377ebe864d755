"""retrieve_into_paged of one 16 k Llama-3-8B context (L 32, H 8, D 128, block 16, bf16) from an HBM-resident CacheGen
tier into a paged cache, three ways, one process, medians of RUNS runs behind a clock ramp:

  nhdb_direct   direct=True: k_decode stores into the split blocks of vLLM's ROCm paged-attention cache (DEC_PAGED_SPLIT)
  nhdb_staged   the default: decode into a [L,2,T,H,D] chunk, then lmc_copy_kv (k_copy_split) scatters it
  nbhd          the yardstick: the decode into NBHD rows

each for a block-ordered mapping (blocks in shuffled order, a block's tokens in order: the decoder's 8-token block path)
and a token-random one (the one-token loop).  Per leg the wall time of the engine call + synchronize (what
paged_split_rates.py reports) and the device time between two HIP events around the call.

    python tools/probes/split_decode_rates.py [out.json]
"""
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__)))))
from lmcache_amd import native  # noqa: E402
from lmcache_amd.cache_engine import LMCacheEngine  # noqa: E402
from lmcache_amd.config import LMCacheEngineConfig, LMCacheEngineMetadata  # noqa: E402

RUNS = 30
L, H, D, T, BS = 32, 8, 128, 16384, 16
MODEL = "Llama-3-8B"


def measure(fn, runs=RUNS):
    """-> (median wall ms of call + synchronize, median ms between HIP events around the call)"""
    wall, evt = [], []
    for _ in range(runs + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        evt.append(a.elapsed_time(b))
    return statistics.median(wall[2:]), statistics.median(evt[2:])


def main():
    dev = torch.device("cuda:0")
    native.build()
    g = torch.Generator().manual_seed(0)
    nb = T // BS + 64
    kv = tuple((torch.randn(T, H, D, device=dev).to(torch.bfloat16), torch.randn(T, H, D, device=dev).to(torch.bfloat16))
               for _ in range(L))
    split = [torch.zeros((2, nb, H, D, BS), dtype=torch.bfloat16, device=dev) for _ in range(L)]
    split2 = [torch.zeros((2, nb, H, D, BS), dtype=torch.bfloat16, device=dev) for _ in range(L)]
    nbhd = [torch.zeros((2, nb, BS, H, D), dtype=torch.bfloat16, device=dev) for _ in range(L)]
    blocks = torch.randperm(nb, generator=g)[:T // BS]
    pos = torch.arange(T)
    maps = {"ordered": (blocks[pos // BS] * BS + pos % BS).to(dev), "random": torch.randperm(nb * BS, generator=g)[:T].to(dev)}
    eng = LMCacheEngine(LMCacheEngineConfig.from_legacy(chunk_size=256, backend="cuda", local_serde="cachegen"),
                        LMCacheEngineMetadata(MODEL, 1, 0, "vllm", "half"))
    tokens = torch.randint(0, 30000, (T,), generator=g).to(dev)
    eng.store(tokens, kv)
    torch.cuda.synchronize()
    legs = {"nhdb_direct": lambda m: eng.retrieve_into_paged(tokens, split, m, BS, "NHDB", direct=True),
            "nhdb_staged": lambda m: eng.retrieve_into_paged(tokens, split2, m, BS, "NHDB"),
            "nbhd": lambda m: eng.retrieve_into_paged(tokens, nbhd, m, BS, "NBHD")}
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.5:  # ramp the clock
        legs["nbhd"](maps["ordered"])
    torch.cuda.synchronize()
    out = {"runs": RUNS, "tokens": T, "kv_bytes": 2 * L * T * H * D * 2}
    for mname, m in maps.items():
        for leg, fn in legs.items():
            mask = fn(m)  # (once unmeasured: the plans and tables of this mapping)
            assert bool(mask.all()), (leg, mname)
            out[f"{leg}_{mname}_wall_ms"], out[f"{leg}_{mname}_event_ms"] = measure(lambda: fn(m))
        torch.cuda.synchronize()
        for a, b in zip(split, split2):  # the two NHDB legs wrote the same cache
            assert torch.equal(a, b), mname
        for k in ("wall", "event"):
            out[f"direct_over_staged_{mname}_{k}"] = out[f"nhdb_direct_{mname}_{k}_ms"] / out[f"nhdb_staged_{mname}_{k}_ms"]
            out[f"direct_over_nbhd_{mname}_{k}"] = out[f"nhdb_direct_{mname}_{k}_ms"] / out[f"nbhd_{mname}_{k}_ms"]
    eng.close()
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(line + "\n")


if __name__ == "__main__":
    main()
