"""Rates of the shuffled-layout copies (k_copy_shuffle.h, layout "NHBDx") against the split-layout copies (k_copy_split.h,
"NHDB") on one 16 k Llama-3-8B range (L 32, H 8, D 128, block 16, bf16), the method of paged_split_rates.py: HIP events, one
process, RUNS runs behind a clock ramp; median, and the spread as (min, max).

  {nhdb,nhbdx}_{gather,scatter}         block-ordered mapping (blocks in shuffled order, a block's tokens in order)
  {nhdb,nhbdx}_{gather,scatter}_random  every token at a random slot (the element path)

    python tools/probes/paged_shuffle_rates.py [out.json]
"""
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__)))))
from lmcache_amd import native  # noqa: E402

RUNS = 30
L, H, D, T, BS, X = 32, 8, 128, 16384, 16, 8


def timed(fn, runs=RUNS):
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def main():
    dev = torch.device("cuda:0")
    ctx = native.get_context(0)
    g = torch.Generator().manual_seed(0)
    nb = T // BS + 64
    chunk = torch.randn(L, 2, T, H, D, device=dev).to(torch.bfloat16)
    out_chunk = torch.empty_like(chunk)
    split = [torch.zeros((2, nb, H, D, BS), dtype=torch.bfloat16, device=dev) for _ in range(L)]
    shuf = [torch.zeros((2, nb, H, D, BS), dtype=torch.bfloat16, device=dev) for _ in range(L)]
    pairs = [(c[0].view(nb, H, D // X, BS, X), c[1].view(nb, H, BS // X, D, X)) for c in shuf]
    blocks = torch.randperm(nb, generator=g)[:T // BS]
    pos = torch.arange(T)
    maps = {"ordered": (blocks[pos // BS] * BS + pos % BS).to(dev), "random": torch.randperm(nb * BS, generator=g)[:T].to(dev)}
    src, dst = native.KVLayout.from_chunk(chunk, "vllm"), native.KVLayout.from_chunk(out_chunk, "vllm")
    lay = {(k, m): native.KVLayout.paged(c, s, BS, name) for k, c, name in (("nhdb", split, "NHDB"), ("nhbdx", pairs, "NHBDx"))
           for m, s in maps.items()}
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.5:  # ramp the clock
        ctx.copy_kv(src, 0, T, lay["nhdb", "ordered"], 0)
    torch.cuda.synchronize()
    out = {"runs": RUNS, "bytes_moved_each_way": chunk.numel() * 2}
    for m in ("ordered", "random"):
        tag = "" if m == "ordered" else "_random"
        for kind in ("nhdb", "nhbdx", "nhdb", "nhbdx"):  # each twice, interleaved: the second pass is the one kept
            p = lay[kind, m]
            for leg, fn in (("scatter", lambda: ctx.copy_kv(src, 0, T, p, 0)), ("gather", lambda: ctx.copy_kv(p, 0, T, dst, 0))):
                med, lo, hi = timed(fn)
                out[f"{kind}_{leg}{tag}_ms"], out[f"{kind}_{leg}{tag}_min_max_ms"] = med, (lo, hi)
            torch.cuda.synchronize()
            assert torch.equal(out_chunk, chunk), (kind, m)  # scatter then gather is the identity
            out_chunk.zero_()
        for leg in ("gather", "scatter"):
            out[f"{leg}_ratio_{m}"] = out[f"nhbdx_{leg}{tag}_ms"] / out[f"nhdb_{leg}{tag}_ms"]
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(line + "\n")


if __name__ == "__main__":
    main()
