"""A window of heads out of every blob (lmc_decode_chunks_heads_schedule / _fixed_heads_schedule) against the full decode,
on one 16 k Llama-3-8B bf16 context (L 32, H 8, D 128, 64 chunks of 256 tokens), both coder models.  One process, the
same blobs for every leg, a clock ramp, the legs ALTERNATING inside each of RUNS rounds, device-event times around each
leg (one C call), median / min / max per leg, one JSON line.

  full     the whole blobs into an [L,2,T,8,128] chunk: lmc_decode_chunks_schedule / lmc_decode_chunks_fixed_schedule
  w1of2    heads 4..7 -> a destination of 4 heads      (what a TP = 2 rank reads of a TP = 1 store)
  w1of4    heads 6..7 -> a destination of 2 heads      (TP = 4)
  w1of8    head 7     -> a destination of 1 head       (TP = 8)
  share    the window's share of the streams; `over_full` = leg time / full time.  The expectation put to the test: time
           roughly proportional to the share.  A launch of few streams need not fill the chip: that is a finding.

Before anything is timed every window's destination is held against the slice of the full decode, bit for bit.

  --full-only   time only the two full decodes, through lmc_decode_chunks into per-layer [T,H,D] tensors as bench.py's
                decode leg does.  Uses nothing this feature added, so with --tree DIR it runs against another checkout's
                package and library (the parent commit's): the A/B of the common path, one process per side, alternated
                by the caller.

    python tools/probes/head_window_rates.py [out.json] [--full-only] [--tree DIR] [--runs N]
"""
import json
import os
import statistics
import sys
import time

import torch


def _opt(name, default=None, flag=False):
    if name not in sys.argv:
        return default
    i = sys.argv.index(name)
    if flag:
        del sys.argv[i]
        return True
    v = sys.argv[i + 1]
    del sys.argv[i:i + 2]
    return v


FULL_ONLY = _opt("--full-only", False, flag=True)
TREE = _opt("--tree", os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
RUNS = int(_opt("--runs", 30))
sys.path.insert(0, os.path.abspath(TREE))
from lmcache_amd import native  # noqa: E402
from lmcache_amd.storage_backend.serde.cachegen_basics import CacheGenConfig  # noqa: E402

L, H, D, T, CS = 32, 8, 128, 16384, 256
MODEL = "Llama-3-8B"
WINDOWS = {"w1of2": (4, 4), "w1of4": (6, 2), "w1of8": (7, 1)}  # (src_head_begin, nheads): the upper heads, no group 0


def timed(legs):
    """{name: fn} -> {name: (median, min, max) ms}: RUNS rounds, every leg once per round in turn, device events around each."""
    ms = {k: [] for k in legs}
    for _ in range(RUNS):
        for name, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}


def main():
    dev = torch.device("cuda:0")
    ctx = native.get_context(0)
    bins = CacheGenConfig.from_model_name(MODEL).plane_bins(L)
    n = T // CS
    stride = native.r16(native.blob_bound(L, CS, H, D))
    gd = torch.Generator(device=dev).manual_seed(0)
    kv = tuple((torch.rand(T, H, D, generator=gd, device=dev).to(torch.bfloat16), torch.rand(T, H, D, generator=gd, device=dev).to(torch.bfloat16))
               for _ in range(L))
    src = native.KVLayout.from_kv_tuple(kv, "vllm")
    arenas = {m: torch.zeros(n * stride, dtype=torch.uint8, device=dev) for m in ("coded", "fixed")}
    sizes = {m: torch.zeros(n, dtype=torch.int32, device=dev) for m in arenas}
    ctx.encode_chunks(src, 0, T, CS, bins, arenas["coded"].data_ptr(), stride, sizes["coded"].data_ptr())
    ctx.encode_chunks_fixed(src, 0, T, CS, bins, arenas["fixed"].data_ptr(), stride, sizes["fixed"].data_ptr())
    torch.cuda.synchronize()
    ctx.raise_on_status("encode")
    out = {"runs": RUNS, "tokens": T, "chunks": n, "tree": os.path.abspath(TREE), "library": native.SO_PATH,
           "raw_bytes": L * 2 * T * H * D * 2, "blob_bytes": {m: int(s.sum()) for m, s in sizes.items()}}

    if FULL_ONLY:
        outs = tuple((torch.empty_like(k), torch.empty_like(v)) for k, v in kv)
        ol = native.KVLayout.from_kv_tuple(outs, "vllm")
        # (lmc_decode_chunks is the coded models' call -- bench.py's decode leg; the fixed-width full decode goes through its schedule)
        legs = {"coded": lambda: ctx.decode_chunks(arenas["coded"].data_ptr(), stride, n, ol, 0, CS)}
        tables = {m: torch.tensor([arenas[m].data_ptr() + i * stride for i in range(n)], dtype=torch.int64).to(dev) for m in arenas}
        legs["fixed"] = lambda: ctx.decode_chunks_fixed_schedule(tables["fixed"].data_ptr(), stride, n, ol, 0, CS, [L], None)
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.5:  # ramp the clock
            legs["coded"]()
        torch.cuda.synchronize()
        res = timed(legs)
        ctx.raise_on_status("timed legs")
        for m, (med, lo, hi) in res.items():
            out[f"{m}_full_ms"] = {"median": round(med, 4), "min": round(lo, 4), "max": round(hi, 4)}
    else:
        tables = {m: torch.tensor([arenas[m].data_ptr() + i * stride for i in range(n)], dtype=torch.int64).to(dev) for m in arenas}
        full = torch.zeros(L, 2, T, H, D, dtype=torch.bfloat16, device=dev)
        full_l = native.KVLayout.from_chunk(full, "vllm")
        dsts = {w: torch.zeros(L, 2, T, nh, D, dtype=torch.bfloat16, device=dev) for w, (_, nh) in WINDOWS.items()}
        lays = {w: native.KVLayout.from_chunk(t, "vllm") for w, t in dsts.items()}
        for m in ("coded", "fixed"):
            sched = ctx.decode_chunks_schedule if m == "coded" else ctx.decode_chunks_fixed_schedule
            heads = ctx.decode_chunks_heads_schedule if m == "coded" else ctx.decode_chunks_fixed_heads_schedule
            legs = {"full": lambda: sched(tables[m].data_ptr(), stride, n, full_l, 0, CS, [L], None)}
            for w, (h0, nh) in WINDOWS.items():
                legs[w] = (lambda w=w, h0=h0, nh=nh: heads(tables[m].data_ptr(), stride, n, lays[w], 0, CS, [L], None,
                                                           native.HeadWindow(H, h0, nh, 0)))
            for fn in legs.values():
                fn()
            torch.cuda.synchronize()
            ctx.raise_on_status(f"{m} decode")
            for w, (h0, nh) in WINDOWS.items():
                assert torch.equal(dsts[w].view(torch.int16), full[:, :, :, h0:h0 + nh].view(torch.int16)), f"{m} {w}: not the slice"
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < 0.5:  # ramp the clock
                legs["full"]()
            torch.cuda.synchronize()
            res = timed(legs)
            ctx.raise_on_status("timed legs")
            for leg, (med, lo, hi) in res.items():
                row = {"median_ms": round(med, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4)}
                if leg != "full":
                    row["share"] = WINDOWS[leg][1] / H
                    row["over_full"] = round(med / res["full"][0], 3)
                    row["streams_per_launch"] = n * 2 * L * (WINDOWS[leg][1] * D // 64)
                else:
                    row["streams_per_launch"] = n * 2 * L * (H * D // 64)
                out[f"{m}_{leg}"] = row
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(line + "\n")


if __name__ == "__main__":
    main()
