"""The fixed-width model (LMC_MODEL_FIXED, csrc/k_fixed.h) on an "NHDB" cache (LMC_PAGED_SPLIT): direct against staged,
on one 16 k Llama-3-8B bf16 context (L 32, H 8, D 128, 64 chunks of 256 tokens, block size 16).  One process, the same
tensors for every leg, a clock ramp, the legs ALTERNATING inside each of RUNS rounds, medians of device-event times
around each leg (a leg is one or two C calls), one JSON line.  fixed_rates.py has the row figures.

  encode   direct   lmc_encode_chunks_fixed_split from the cache
           staged   lmc_copy_kv gather into a [L,2,T,H,D] chunk (allocated once, outside the clock) + lmc_encode_chunks_fixed
  decode   direct   lmc_decode_chunks_fixed_split_schedule into the cache (one range)
           staged   lmc_decode_chunks_fixed_schedule into the chunk + lmc_copy_kv scatter
           coded    lmc_decode_chunks_schedule of the entropy-coded blobs into the same cache (the coded tier's direct decode)
  mappings blocks   block-ordered slots (blocks in shuffled order, a block's 16 tokens in order)
           random   every token at a random slot of its own

Before anything is timed the legs are held against each other: the direct blobs are the staged blobs, byte for byte, and
the three decodes leave the same cache.

    python tools/probes/fixed_split_rates.py [out.json] [--tokens N]
"""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from lmcache_amd import native  # noqa: E402
from lmcache_amd.storage_backend.serde.cachegen_basics import CacheGenConfig  # noqa: E402

RUNS = 30
L, H, D, T, CS, BS = 32, 8, 128, 16384, 256, 16
if "--tokens" in sys.argv:
    _i = sys.argv.index("--tokens")
    T = int(sys.argv[_i + 1])
    del sys.argv[_i:_i + 2]
MODEL = "Llama-3-8B"
HBM_PEAK = 8.0e12  # bytes / s: the figure profiles/fixed_model.md takes its shares against


def timed(legs):
    """{name: fn} -> {name: median ms}: RUNS rounds, every leg once per round in turn, device events around each."""
    ms = {k: [] for k in legs}
    for _ in range(RUNS):
        for name, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b))
    return {k: statistics.median(v) for k, v in ms.items()}


def main():
    dev = torch.device("cuda:0")
    ctx = native.get_context(0)
    bins = CacheGenConfig.from_model_name(MODEL).plane_bins(L)
    n = T // CS
    stride = native.r16(native.blob_bound(L, CS, H, D))
    arenas = {m: torch.zeros(n * stride, dtype=torch.uint8, device=dev) for m in ("direct", "staged", "coded")}
    sizes = {m: torch.zeros(n, dtype=torch.int32, device=dev) for m in arenas}
    raw_bytes = L * 2 * T * H * D * 2
    fixed_bytes = native.fixed_blob_bytes(L, CS, H, D, bins) * n
    nb = T // BS + 4
    g = torch.Generator().manual_seed(1)
    perm = torch.randperm(nb, generator=g)[:T // BS]
    mappings = {"blocks": (perm[:, None] * BS + torch.arange(BS)[None, :]).reshape(-1).to(dev),
                "random": torch.randperm(nb * BS, generator=g)[:T].to(dev)}
    gd = torch.Generator(device=dev).manual_seed(0)
    caches = [torch.rand(2, nb, H, D, BS, generator=gd, device=dev).to(torch.bfloat16) for _ in range(L)]
    chunk = torch.zeros(L, 2, T, H, D, dtype=torch.bfloat16, device=dev)
    rows = native.KVLayout.from_chunk(chunk, "vllm")
    out = {"runs": RUNS, "tokens": T, "chunks": n, "block_size": BS, "raw_bytes": raw_bytes, "fixed_blob_bytes": fixed_bytes,
           "bytes_moved_direct": raw_bytes + fixed_bytes, "bytes_moved_staged": 3 * raw_bytes + fixed_bytes}

    for name, slots in mappings.items():
        split = native.KVLayout.paged(caches, slots, BS, "NHDB")
        tables = {m: torch.tensor([arenas[m].data_ptr() + i * stride for i in range(n)], dtype=torch.int64).to(dev) for m in arenas}

        def enc_direct():
            ctx.encode_chunks_fixed_split(split, 0, T, CS, bins, arenas["direct"].data_ptr(), stride, sizes["direct"].data_ptr())

        def enc_staged():
            ctx.copy_kv(split, 0, T, rows, 0)
            ctx.encode_chunks_fixed(rows, 0, T, CS, bins, arenas["staged"].data_ptr(), stride, sizes["staged"].data_ptr())

        def dec_direct():
            ctx.decode_chunks_fixed_split_schedule(tables["direct"].data_ptr(), stride, n, split, 0, CS, [L], None)

        def dec_staged():
            ctx.decode_chunks_fixed_schedule(tables["direct"].data_ptr(), stride, n, rows, 0, CS, [L], None)
            ctx.copy_kv(rows, 0, T, split, 0)

        def dec_coded():
            ctx.decode_chunks_schedule(tables["coded"].data_ptr(), stride, n, split, 0, CS, [L], None)

        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.5:  # ramp the clock
            enc_direct()
        enc_staged()
        ctx.encode_chunks_split(split, 0, T, CS, bins, arenas["coded"].data_ptr(), stride, sizes["coded"].data_ptr())
        torch.cuda.synchronize()
        ctx.raise_on_status("encode")
        assert torch.equal(sizes["direct"], sizes["staged"]) and torch.equal(arenas["direct"], arenas["staged"]), \
            "the direct blobs differ from the staged ones"
        # the three decodes leave the same cache (the slots of the call's tokens are rewritten with their own decode)
        seen = []
        for fn in (dec_coded, dec_staged, dec_direct):
            fn()
            torch.cuda.synchronize()
            ctx.raise_on_status("decode")
            seen.append([c.clone() for c in caches])
        assert all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(*seen)), "the decodes leave different caches"
        del seen
        enc = timed({"direct": enc_direct, "staged": enc_staged})
        dec = timed({"direct": dec_direct, "staged": dec_staged, "coded": dec_coded})
        ctx.raise_on_status("timed legs")
        for leg, v in enc.items():
            out[f"{name}_encode_{leg}_ms"] = round(v, 4)
        for leg, v in dec.items():
            out[f"{name}_decode_{leg}_ms"] = round(v, 4)
        for what, r in (("encode", enc), ("decode", dec)):
            out[f"{name}_{what}_direct_over_staged"] = round(r["direct"] / r["staged"], 3)
            out[f"{name}_{what}_direct_share_of_hbm_peak"] = round((raw_bytes + fixed_bytes) / (r["direct"] * 1e-3) / HBM_PEAK, 3)
            out[f"{name}_{what}_staged_share_of_hbm_peak"] = round((3 * raw_bytes + fixed_bytes) / (r["staged"] * 1e-3) / HBM_PEAK, 3)
        out[f"{name}_decode_direct_over_coded"] = round(dec["direct"] / dec["coded"], 3)
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(line + "\n")


if __name__ == "__main__":
    main()
