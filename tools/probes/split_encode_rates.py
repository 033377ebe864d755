"""The encode of one 16 k Llama-3-8B context (L 32, H 8, D 128, block 16, bf16) that lies in vLLM's ROCm paged-attention
cache ("NHDB"), one process, medians of RUNS runs behind a clock ramp:

  a  today's path: lmc_copy_kv gathers the range into a [L,2,T,H,D] chunk (k_copy_split), then lmc_encode_chunks, AUTO
  b  lmc_encode_chunks under set_encode_path("two_kernels") on the already gathered chunk: the launch path of (c), on rows
  c  lmc_encode_chunks_split on the cache: k_quantize's split instances + k_cdf_encode
  d  engine.store_paged(..., "NHDB") on the pinned CacheGen tier, blocking: staged
  e  the same with direct=True (one pack part: no overlap of the part copies with the encode)

each for a block-ordered mapping (blocks in shuffled order, a block's tokens in order) and a token-random one.  Per leg the
wall time of the call + synchronize and the device time between two HIP events around the call.  (c) / (b) is what the
split addressing costs, (c) / (a) what a caller gains.

    python tools/probes/split_encode_rates.py [out.json]
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
L, H, D, T, BS, CS = 32, 8, 128, 16384, 16, 256
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
    blobs = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
    blobs2 = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
    sizes = torch.zeros(n, dtype=torch.int32, device=dev)
    sizes2 = torch.zeros(n, dtype=torch.int32, device=dev)
    chunk = torch.zeros((L, 2, T, H, D), dtype=torch.bfloat16, device=dev)
    rows = native.KVLayout.from_chunk(chunk, "vllm")
    cfg = LMCacheEngineConfig.from_legacy(chunk_size=CS, backend="cpu", local_serde="cachegen")
    out = {"runs": RUNS, "tokens": T, "kv_bytes": 2 * L * T * H * D * 2}

    def two_kernels(fn):
        ctx.set_encode_path("two_kernels")
        try:
            fn()
        finally:
            ctx.set_encode_path("auto")

    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.5:  # ramp the clock
        ctx.encode_chunks(rows, 0, T, CS, bins, blobs.data_ptr(), stride, sizes.data_ptr())
    torch.cuda.synchronize()
    for mname, m in maps.items():
        lay = native.KVLayout.paged(split, m, BS, "NHDB")

        def leg_a():
            ctx.copy_kv(lay, 0, T, rows, 0)
            ctx.encode_chunks(rows, 0, T, CS, bins, blobs.data_ptr(), stride, sizes.data_ptr())

        legs = {"a_gather_encode_auto": leg_a,
                "b_rows_two_kernels": lambda: two_kernels(lambda: ctx.encode_chunks(rows, 0, T, CS, bins, blobs.data_ptr(), stride, sizes.data_ptr())),
                "c_split": lambda: ctx.encode_chunks_split(lay, 0, T, CS, bins, blobs2.data_ptr(), stride, sizes2.data_ptr())}
        for leg, fn in legs.items():
            fn()
            out[f"{leg}_{mname}_wall_ms"], out[f"{leg}_{mname}_event_ms"] = measure(fn)
        torch.cuda.synchronize()
        ctx.raise_on_status(mname)
        assert torch.equal(sizes, sizes2) and torch.equal(blobs, blobs2), mname  # the same blobs either way
        for leg, direct in (("d_store_paged_staged", False), ("e_store_paged_direct", True)):
            tokens = torch.randint(0, 30000, (T,), generator=g).to(dev)

            def store():
                eng = store.eng
                eng.store_paged(tokens, split, m, BS, "NHDB", skip_existing=False, direct=direct)

            store.eng = LMCacheEngine(cfg, LMCacheEngineMetadata(MODEL, 1, 0, "vllm", "half"))
            store()
            out[f"{leg}_{mname}_wall_ms"], out[f"{leg}_{mname}_event_ms"] = measure(store)
            store.eng.close()
        for k in ("wall", "event"):
            out[f"c_over_b_{mname}_{k}"] = out[f"c_split_{mname}_{k}_ms"] / out[f"b_rows_two_kernels_{mname}_{k}_ms"]
            out[f"c_over_a_{mname}_{k}"] = out[f"c_split_{mname}_{k}_ms"] / out[f"a_gather_encode_auto_{mname}_{k}_ms"]
        out[f"e_over_d_{mname}_wall"] = out[f"e_store_paged_direct_{mname}_wall_ms"] / out[f"d_store_paged_staged_{mname}_wall_ms"]
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(line + "\n")


if __name__ == "__main__":
    main()
