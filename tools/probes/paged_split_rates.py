"""Rates of the split-layout copies (k_copy_split.h) on one 16 k Llama-3-8B range (L 32, H 8, D 128, block 16, bf16), HIP
events, one process, medians of RUNS runs behind a clock ramp:

  nhdb_gather / nhdb_scatter        block-ordered mapping (blocks in shuffled order, a block's tokens in order): split cache
                                    <-> vllm chunk through lmc_copy_kv
  nhdb_*_random                     every token at a random slot (the element path), for the record
  nhbd_gather / nhbd_scatter        the yardstick: k_copy_kv moving the same range between an NHBD cache and the chunk
  retrieve_into_paged_{nbhd,nhdb}   wall time of the engine call + synchronize on an HBM-resident CacheGen tier: the direct
                                    decode into NBHD blocks against the staged decode + scatter into the split cache

    python tools/probes/paged_split_rates.py [out.json]
"""
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__)))))
from lmcache_amd import native  # noqa: E402

RUNS = 30
L, H, D, T, BS = 32, 8, 128, 16384, 16
MODEL = "Llama-3-8B"


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
    out_chunk = torch.empty_like(chunk)
    split = [torch.zeros((2, nb, H, D, BS), dtype=torch.bfloat16, device=dev) for _ in range(L)]
    nhbd = [torch.zeros((2, nb, H, BS, D), dtype=torch.bfloat16, device=dev) for _ in range(L)]
    blocks = torch.randperm(nb, generator=g)[:T // BS]
    pos = torch.arange(T)
    ordered = (blocks[pos // BS] * BS + pos % BS).to(dev)
    rand = torch.randperm(nb * BS, generator=g)[:T].to(dev)
    src, dst = native.KVLayout.from_chunk(chunk, "vllm"), native.KVLayout.from_chunk(out_chunk, "vllm")
    lay = {("nhdb", "ordered"): native.KVLayout.paged(split, ordered, BS, "NHDB"),
           ("nhdb", "random"): native.KVLayout.paged(split, rand, BS, "NHDB"),
           ("nhbd", "ordered"): native.KVLayout.paged(nhbd, ordered, BS, "NHBD"),
           ("nhbd", "random"): native.KVLayout.paged(nhbd, rand, BS, "NHBD")}
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.5:  # ramp the clock
        ctx.copy_kv(src, 0, T, lay["nhbd", "ordered"], 0)
    torch.cuda.synchronize()
    out = {"runs": RUNS, "bytes_moved_each_way": chunk.numel() * 2}
    for kind in ("nhbd", "nhdb"):
        for m in ("ordered", "random"):
            tag = "" if m == "ordered" else "_random"
            p = lay[kind, m]
            out[f"{kind}_scatter{tag}_ms"] = timed(lambda: ctx.copy_kv(src, 0, T, p, 0))
            out[f"{kind}_gather{tag}_ms"] = timed(lambda: ctx.copy_kv(p, 0, T, dst, 0))
            torch.cuda.synchronize()
            assert torch.equal(out_chunk, chunk), (kind, m)  # scatter then gather is the identity
            out_chunk.zero_()
    for leg in ("gather", "scatter"):
        out[f"{leg}_ratio_ordered"] = out[f"nhdb_{leg}_ms"] / out[f"nhbd_{leg}_ms"]
        out[f"{leg}_ratio_random"] = out[f"nhdb_{leg}_random_ms"] / out[f"nhbd_{leg}_random_ms"]
        out[f"nhdb_{leg}_TBps"] = 2 * out["bytes_moved_each_way"] / out[f"nhdb_{leg}_ms"] / 1e9
        out[f"nhbd_{leg}_TBps"] = 2 * out["bytes_moved_each_way"] / out[f"nhbd_{leg}_ms"] / 1e9

    # end to end: retrieve_into_paged of the same 16 k context from an HBM-resident CacheGen tier
    from lmcache_amd.cache_engine import LMCacheEngine
    from lmcache_amd.config import LMCacheEngineConfig, LMCacheEngineMetadata
    eng = LMCacheEngine(LMCacheEngineConfig.from_legacy(chunk_size=256, backend="cuda", local_serde="cachegen"),
                        LMCacheEngineMetadata(MODEL, 1, 0, "vllm", "half"))
    tokens = torch.randint(0, 30000, (T,), generator=g).to(dev)
    eng.store(tokens, tuple(tuple(l.unbind(0)) for l in chunk.unbind(0)))
    torch.cuda.synchronize()
    nbhd = [c.view(2, nb, BS, H, D) for c in nhbd]

    def wall(fn, runs=10):
        ts = []
        for _ in range(runs + 2):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts[2:])

    out["retrieve_into_paged_nbhd_ms"] = wall(lambda: eng.retrieve_into_paged(tokens, nbhd, ordered, BS, "NBHD"))
    out["retrieve_into_paged_nhdb_ms"] = wall(lambda: eng.retrieve_into_paged(tokens, split, ordered, BS, "NHDB"))
    out["retrieve_into_paged_ratio"] = out["retrieve_into_paged_nhdb_ms"] / out["retrieve_into_paged_nbhd_ms"]
    eng.close()
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(line + "\n")


if __name__ == "__main__":
    main()
