"""Times of the two repack legs of the bounded tiers on one 16 k Llama-3-8B context (64 chunks of 256 tokens), HIP events,
one process, medians of RUNS runs behind a clock ramp:

  pack_store    the store path's pack kernels into device memory: lmc_store_pack_parts (one part) minus lmc_encode_chunks
                on the same input (the pack kernels are not bracketed by events of their own)
  pack_blobs    lmc_pack_blobs over the same blobs through a pointer table (events around the call, and the context's
                profile marks around its two kernels)
  unpack        k_unpack alone (profile marks), and lmc_unpack_blobs with its DMA staging (events around the call)
  demotion      wall time of backend.set_capacity() that demotes the context's group (the pinned slab's hipHostMalloc
                included), against its bytes at 52 GB/s

    python tools/probes/repack_times.py [out.json]
"""
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__)))))
from lmcache_amd import native  # noqa: E402
from lmcache_amd.storage_backend.serde.cachegen_basics import CacheGenConfig  # noqa: E402
from lmcache_amd.storage_backend.serde.cachegen_device import pack_cap  # noqa: E402

RUNS = 30
L, H, D, T, CS = 32, 8, 128, 16384, 256
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
    torch.manual_seed(0)
    kv = torch.randn(L, 2, T, H, D, device=dev).to(torch.bfloat16)
    lay = native.KVLayout.from_chunk(kv, "vllm")
    bins = CacheGenConfig.from_model_name(MODEL).plane_bins(L)
    n = T // CS
    stride = native.r16(native.blob_bound(L, CS, H, D))
    arena = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
    sizes = native.PinnedBuffer(4 * n)
    part_info = native.PinnedBuffer(256)
    cap = pack_cap(n, L, CS, H, D, bins)
    region = torch.zeros(cap, dtype=torch.uint8, device=dev)
    ev = [native.NativeEvent()]

    def encode():
        ctx.encode_chunks(lay, 0, T, CS, bins, arena.data_ptr(), stride, sizes.ptr)

    def store_pack():
        ctx.store_pack_parts(lay, 0, T, CS, bins, region.data_ptr(), cap, sizes.ptr, 1, part_info.ptr, ev)

    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.5:  # ramp the clock
        encode()
    torch.cuda.synchronize()
    out = {"runs": RUNS, "chunks": n}
    out["encode_ms"] = timed(encode)
    out["store_pack_one_part_ms"] = timed(store_pack)
    out["pack_store_ms"] = out["store_pack_one_part_ms"] - out["encode_ms"]
    encode()
    torch.cuda.synchronize()
    ctx.raise_on_status("encode")
    blob_sizes = sizes.tensor.view(torch.int32)[:n].tolist()
    total = native.pack_off_streams(n, L, CS, H, D) + sum(s - native.blob_static_bytes(L, CS, H, D) for s in blob_sizes)
    out["pack_bytes"] = total
    table = torch.tensor([arena.data_ptr() + i * stride for i in range(n)], dtype=torch.int64).to(dev)
    room = torch.tensor(blob_sizes, dtype=torch.int32).to(dev)

    def pack_blobs():
        ctx.pack_blobs(table.data_ptr(), room.data_ptr(), n, L, H, D, CS, T, region.data_ptr(), total, dev)

    out["pack_blobs_call_ms"] = timed(pack_blobs)
    ctx.profile(True)
    ks = []
    for _ in range(RUNS):
        pack_blobs()
        torch.cuda.synchronize()
        ks.append(sum(ctx.profile_read()))
    out["pack_blobs_kernels_ms"] = statistics.median(ks)
    ctx.profile(False)
    ctx.raise_on_status("pack_blobs")
    host = native.PinnedBuffer(native.r16(total))
    native.memcpy_async(host.ptr, region.data_ptr(), total, "d2h", torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    native.pack_info(host.ptr, total)
    dst = [torch.zeros(s, dtype=torch.uint8, device=dev) for s in blob_sizes]
    ptrs = [d.data_ptr() for d in dst]

    def unpack():
        ctx.unpack_blobs(host.ptr, total, 0, n, ptrs, blob_sizes, dev)

    out["unpack_call_with_dma_ms"] = timed(unpack)
    ctx.profile(True)
    ks = []
    for _ in range(RUNS):
        unpack()
        torch.cuda.synchronize()
        ks.append(sum(ctx.profile_read()))
    out["unpack_kernel_ms"] = statistics.median(ks)
    ctx.profile(False)
    ctx.raise_on_status("unpack_blobs")
    for i, d in enumerate(dst):
        assert torch.equal(d, arena[i * stride:i * stride + blob_sizes[i]]), "unpack is not the inverse"
    out["pack_blobs_over_store"] = out["pack_blobs_kernels_ms"] / out["pack_store_ms"]
    out["unpack_over_store"] = out["unpack_kernel_ms"] / out["pack_store_ms"]

    # wall time of a demotion through the backend
    from lmcache_amd.cache_engine import LMCacheEngine
    from lmcache_amd.config import LMCacheEngineConfig, LMCacheEngineMetadata
    eng = LMCacheEngine(LMCacheEngineConfig.from_legacy(chunk_size=CS, backend="cuda", local_serde="cachegen"),
                        LMCacheEngineMetadata(MODEL, 1, 0, "vllm", "half"))
    be = eng.engine_
    walls = []
    for r in range(5):
        tokens = torch.randint(0, 30000, (T,), generator=torch.Generator().manual_seed(r)).to(dev)
        be.set_capacity(hbm_bytes=8 << 30, pinned_bytes=16 << 30)
        eng.store(tokens, tuple(tuple(l.unbind(0)) for l in kv.unbind(0)))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        be.set_capacity(hbm_bytes=1 << 20, pinned_bytes=16 << 30)  # the group goes down; returns when it is published
        walls.append((time.perf_counter() - t0) * 1e3)
        st = be.tier_stats()
        assert st["demotions"] == r + 1 and st["evictions"] == 0, st
    # (every round's pack takes a pinned slab of its own from the system: the hipHostMalloc is inside the wall time)
    out["demotion_wall_ms"] = walls
    out["demotion_wall_ms_median_after_first"] = statistics.median(walls[1:])
    out["demotion_pcie_ms_at_52GBps"] = total / 52e9 * 1e3
    eng.close()
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(line + "\n")


if __name__ == "__main__":
    main()
