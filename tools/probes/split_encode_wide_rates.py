"""The encode of one 16 k context of a model with 4096 KV channels per plane (L 32, H 32, D 128 -- Llama-2-7B --, block 16,
bf16) that lies in vLLM's ROCm paged-attention cache ("NHDB"), under LMCACHE_AMD_SPLIT_WIDE=1, one process, the two legs of
a pair ALTERNATING run by run behind a clock ramp, medians of RUNS runs of the device time between two HIP events:

  staged   lmc_copy_kv gathers the range into a [L,2,T,H,D] chunk (k_copy_split), then the contiguous encode of the chunk
  direct   the split encode on the cache: k_quantize_wide_split + k_cdf_encode / k_fixed_wide_split

for the coded and the fixed-width tier, each for a block-ordered mapping (blocks in shuffled order, a block's tokens in
order) and a token-random one.  The staged leg launches only kernels that the wide split kernels left untouched.

    LMCACHE_AMD_SPLIT_WIDE=1 python tools/probes/split_encode_wide_rates.py [out.json]
"""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from lmcache_amd import native  # noqa: E402

RUNS = 20
L, H, D, T, BS, CS = 32, 32, 128, 16384, 16, 256


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    assert native.split_wide_enabled(), "set LMCACHE_AMD_SPLIT_WIDE=1"
    dev = torch.device("cuda:0")
    native.build()
    ctx = native.get_context(0)
    g = torch.Generator().manual_seed(0)
    nb = T // BS + 64
    split = [torch.randn((2, nb, H, D, BS), device=dev).to(torch.bfloat16) for _ in range(L)]
    blocks = torch.randperm(nb, generator=g)[:T // BS]
    pos = torch.arange(T)
    maps = {"ordered": (blocks[pos // BS] * BS + pos % BS).to(dev), "random": torch.randperm(nb * BS, generator=g)[:T].to(dev)}
    bins = [32] * 10 + [16] * 22 + [32] * 2 + [16] * 30
    n = T // CS
    stride = native.r16(native.blob_bound(L, CS, H, D))
    blobs, blobs2 = (torch.zeros(n * stride, dtype=torch.uint8, device=dev) for _ in range(2))
    sizes, sizes2 = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(2))
    chunk = torch.zeros((L, 2, T, H, D), dtype=torch.bfloat16, device=dev)
    rows = native.KVLayout.from_chunk(chunk, "vllm")
    out = {"runs": RUNS, "tokens": T, "kv_bytes": 2 * L * T * H * D * 2}
    tiers = {"coded": (ctx.encode_chunks, ctx.encode_chunks_split), "fixed": (ctx.encode_chunks_fixed, ctx.encode_chunks_fixed_split)}
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.5:  # ramp the clock
        ctx.encode_chunks(rows, 0, T, CS, bins, blobs.data_ptr(), stride, sizes.data_ptr())
    torch.cuda.synchronize()
    for mname, m in maps.items():
        lay = native.KVLayout.paged(split, m, BS, "NHDB")
        for tier, (enc_rows, enc_split) in tiers.items():
            def staged():
                ctx.copy_kv(lay, 0, T, rows, 0)
                enc_rows(rows, 0, T, CS, bins, blobs.data_ptr(), stride, sizes.data_ptr())

            def direct():
                enc_split(lay, 0, T, CS, bins, blobs2.data_ptr(), stride, sizes2.data_ptr())

            ms = {"staged": [], "direct": []}
            for i in range(RUNS + 2):
                for leg, fn in (("staged", staged), ("direct", direct)):
                    t = timed(fn)
                    if i >= 2:
                        ms[leg].append(t)
            ctx.raise_on_status(f"{tier} {mname}")
            assert torch.equal(sizes, sizes2) and torch.equal(blobs, blobs2), (tier, mname)  # the same blobs either way
            for leg, v in ms.items():
                out[f"{tier}_{mname}_{leg}_ms"] = statistics.median(v)
                out[f"{tier}_{mname}_{leg}_min_max_ms"] = [min(v), max(v)]
            out[f"{tier}_{mname}_direct_over_staged"] = out[f"{tier}_{mname}_direct_ms"] / out[f"{tier}_{mname}_staged_ms"]
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(line + "\n")


if __name__ == "__main__":
    main()
