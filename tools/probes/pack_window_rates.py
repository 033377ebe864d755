"""Measure lmc_load_pack_heads on a 16 k Llama-3-8B context.  Modes:
  c      C-level: full lmc_load_pack vs windows of 1/2, 1/4, 1/8 of the heads (ms, bytes, GB/s), and a decode-step proxy beside the gather
  engine engine-level: stored_at(1).retrieve of a TP = 2 / 4 / 8 rank, LMCACHE_AMD_PACK_WINDOW off vs on, alternating
Usage: python tools/probes/pack_window_rates.py MODE TAG; prints one JSON line per leg.  LMCACHE_AMD_SO picks a build with
another -DPACK_WINDOW_WGS (the grid-size sweep): TAG names it in the output."""
import ctypes
import json
import os
import sys
import time
from statistics import median

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from lmcache_amd import native  # noqa: E402

DEV = "cuda:0"
L, H, D, T, CS = 32, 8, 128, 16384, 256


def emit(tag, rec):
    print(json.dumps(dict(rec, tag=tag)), flush=True)


def timed(fn, reps=15, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"median_ms": round(median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def mode_c(tag):
    from oracle import lmc_oracle
    from lmcache_amd.storage_backend.serde.cachegen_device import pack_cap
    bins = [int(b) for b in lmc_oracle.cachegen_bins("meta-llama/Llama-3.1-8B-Instruct")[0]]
    ctx = native.get_context(0)
    kv = torch.randn(L, 2, T, H, D, generator=torch.Generator(device=DEV).manual_seed(1), device=DEV, dtype=torch.float32).to(torch.bfloat16)
    n = T // CS
    region = native.PinnedBuffer(pack_cap(n, L, CS, H, D, bins))
    meta = native.PinnedBuffer(4096)
    meta.tensor.zero_()
    ctx.store_pack(native.KVLayout.from_chunk(kv, "vllm"), 0, T, CS, bins, region.ptr, region.nbytes, meta.ptr + 64, status_ptr=meta.ptr)
    torch.cuda.synchronize()
    assert int(meta.tensor[:4].view(torch.int32)[0]) == 0
    h = native.pack_info(region.ptr, region.nbytes)
    total, static = int(h.total_bytes), int(h.off_streams)
    full = torch.zeros(L, 2, T, H, D, dtype=torch.bfloat16, device=DEV)
    lay_full = native.KVLayout.from_chunk(full, "vllm")
    r = timed(lambda: ctx.load_pack(region.ptr, total, 0, 0, lay_full, 0, 0, None, status_ptr=meta.ptr))
    emit(tag, dict(r, what="load_pack full", bytes=total, GBps=round(total / r["median_ms"] / 1e6, 2)))
    wins = {}
    for nh in (4, 2, 1):
        win = native.HeadWindow(H, H - nh, nh, 0)
        dst = torch.zeros(L, 2, T, nh, D, dtype=torch.bfloat16, device=DEV)
        lay = native.KVLayout.from_chunk(dst, "vllm")
        moved = native.pack_window_bytes(region.ptr, total, 0, 0, win)
        fn = lambda lay=lay, win=win: ctx.load_pack_heads(region.ptr, total, 0, 0, lay, 0, 0, None, win, status_ptr=meta.ptr)
        r = timed(fn)
        torch.cuda.synchronize()
        assert int(meta.tensor[:4].view(torch.int32)[0]) == 0
        assert torch.equal(dst.view(torch.int16), full[:, :, :, H - nh:].view(torch.int16)), "window differs from the full load"
        emit(tag, dict(r, what=f"load_pack_heads {nh}/{H}", stream_bytes=moved, bytes=moved + static, share_of_total=round((moved + static) / total, 4),
                       GBps=round((moved + static) / r["median_ms"] / 1e6, 2)))
        wins[nh] = fn
    # a decode-step proxy beside back-to-back gathers of half the heads
    import bench
    proxy = bench.DecodeStepProxy(DEV)
    proxy.time_steps(3)
    alone = median(proxy.time_steps(10))
    side = torch.cuda.Stream(device=DEV)
    for nh in (4, 1):
        beside = []
        for _ in range(3):
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                for _ in range(12):
                    wins[nh]()
            beside += proxy.time_steps(4)
            torch.cuda.synchronize()
        emit(tag, {"what": f"proxy step beside gathers of {nh}/{H}", "alone_ms": round(alone, 3), "beside_ms": round(median(beside), 3),
                   "ratio": round(median(beside) / alone, 4), "max_ratio": round(max(beside) / alone, 4)})
    beside = []
    for _ in range(3):
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            for _ in range(6):
                ctx.load_pack(region.ptr, total, 0, 0, lay_full, 0, 0, None, status_ptr=meta.ptr)
        beside += proxy.time_steps(4)
        torch.cuda.synchronize()
    emit(tag, {"what": "proxy step beside full load_pack (DMA)", "alone_ms": round(alone, 3), "beside_ms": round(median(beside), 3),
               "ratio": round(median(beside) / alone, 4)})


def mode_engine(tag):
    from lmcache_amd.cache_engine import LMCacheEngine
    from lmcache_amd.config import LMCacheEngineConfig, LMCacheEngineMetadata
    g = torch.Generator().manual_seed(2)
    tokens = torch.randint(0, 32000, (T,), generator=g)
    kv = tuple((torch.randn(T, H, D, device=DEV).to(torch.bfloat16), torch.randn(T, H, D, device=DEV).to(torch.bfloat16)) for _ in range(L))
    engines = {}
    for sw in ("0", "1"):
        os.environ["LMCACHE_AMD_PACK_WINDOW"] = sw
        e = LMCacheEngine(LMCacheEngineConfig.from_legacy(chunk_size=CS, backend="cpu", local_serde="cachegen"),
                          LMCacheEngineMetadata("Llama-3-8B", 1, 0, "vllm", "bfloat16"))
        e.store(tokens, kv)
        torch.cuda.synchronize()
        engines[sw] = e

    def rank(base, world):
        r = LMCacheEngine.__new__(LMCacheEngine)
        r.__dict__.update({k: v for k, v in base.__dict__.items() if k not in ("_hash_chain", "_key_memo")})
        r.metadata = LMCacheEngineMetadata("Llama-3-8B", world, world - 1, "vllm", "bfloat16")
        return r.stored_at(1)

    for world in (2, 4, 8):
        views = {sw: rank(engines[sw], world) for sw in ("0", "1")}
        ms = {"0": [], "1": []}
        first, outs = {}, {}
        for rep in range(9):
            for sw in ("0", "1"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out, m = views[sw].retrieve(tokens)
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) * 1e3
                assert int(m.sum()) == T
                if rep == 0:
                    first[sw], outs[sw] = dt, out
                elif rep >= 2:
                    ms[sw].append(dt)
        same = all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for x, y in zip(outs["0"], outs["1"]) for a, b in zip(x, y))
        emit(tag, {"what": f"engine retrieve TP=1 -> TP={world}", "same_bits": same,
                   "off_first_ms": round(first["0"], 2), "on_first_ms": round(first["1"], 2),
                   "off_ms": [round(median(ms["0"]), 3), round(min(ms["0"]), 3), round(max(ms["0"]), 3)],
                   "on_ms": [round(median(ms["1"]), 3), round(min(ms["1"]), 3), round(max(ms["1"]), 3)]})
    for e in engines.values():
        e.close()


if __name__ == "__main__":
    {"c": mode_c, "engine": mode_engine}[sys.argv[1]](sys.argv[2])
