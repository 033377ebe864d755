"""Rates of lmc_transcode_fixed (csrc/k_fixed.h, k_fixed_expand + the two-kernel encode's coder launch) on one 16 k
Llama-3-8B bf16 context (64 chunks of 256 tokens): one process, a clock ramp, medians of RUNS runs taken ALTERNATING
between the two sides, per-kernel times from lmc_ctx_profile (HIP events around each kernel), one JSON line.

  transcode   lmc_transcode_fixed of the context's fixed-width blobs  |  the two-kernel lmc_encode_chunks of the same KV
              (lmc_ctx_set_encode_path): the coder launch is the same launch, so the difference is the first kernel's
  kernels     k_fixed_expand  |  k_quantize (the first profile interval of either call), k_cdf_encode behind each
  demotion    wall time of CacheGenDeviceCodec.demote_blobs(model="fixed") of the whole context as one group -- transcode,
              sizes, lmc_pack_blobs, two DMA copies, the check of the landed pack -- against its pack bytes at 52 GB/s,
              and against the coded tier's demote_blobs of the same context (the same leg without the transcode)

    python tools/probes/transcode_rates.py [out.json] [--tokens N]       (N: the context's length, default 16384)
"""
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__)))))
from lmcache_amd import native  # noqa: E402
from lmcache_amd.storage_backend.serde.cachegen_basics import CacheGenConfig  # noqa: E402
from lmcache_amd.storage_backend.serde.cachegen_device import PinnedArena, get_codec  # noqa: E402

RUNS = 30
DEMOTIONS = 7
L, H, D, T, CS = 32, 8, 128, 16384, 256
if "--tokens" in sys.argv:
    _i = sys.argv.index("--tokens")
    T = int(sys.argv[_i + 1])
    del sys.argv[_i:_i + 2]
MODEL = "Llama-3-8B"
PCIE = 52.0e9  # bytes / s: what the pinned tier's DMA copies reach


def main():
    dev = torch.device("cuda:0")
    ctx = native.get_context(0)
    bins = CacheGenConfig.from_model_name(MODEL).plane_bins(L)
    n = T // CS
    stride = native.r16(native.blob_bound(L, CS, H, D))
    g = torch.Generator(device=dev).manual_seed(0)
    kv = torch.rand(L, 2, T, H, D, generator=g, device=dev).to(torch.bfloat16)
    lay = native.KVLayout.from_chunk(kv, "vllm")
    raw_bytes = kv.numel() * 2
    fixed_size = native.fixed_blob_bytes(L, CS, H, D, bins)
    fstride = stride  # (lmc_encode_chunks_fixed wants the coded bound of a slot too)
    fixed = torch.zeros(n * fstride, dtype=torch.uint8, device=dev)
    coded = {k: torch.zeros(n * stride, dtype=torch.uint8, device=dev) for k in ("encode", "transcode")}
    sizes = {k: native.PinnedBuffer(4 * n) for k in ("fixed", "encode", "transcode")}
    ctx.encode_chunks_fixed(lay, 0, T, CS, bins, fixed.data_ptr(), fstride, sizes["fixed"].ptr)
    torch.cuda.synchronize()
    ctx.raise_on_status("fixed encode")
    views = [fixed[i * fstride:i * fstride + fixed_size] for i in range(n)]
    table = torch.tensor([v.data_ptr() for v in views], dtype=torch.int64).to(dev)
    room = torch.tensor([fixed_size] * n, dtype=torch.int32).to(dev)
    code = native.dtype_code(torch.bfloat16)

    def encode():
        ctx.encode_chunks(lay, 0, T, CS, bins, coded["encode"].data_ptr(), stride, sizes["encode"].ptr)

    def transcode():
        ctx.transcode_fixed(table.data_ptr(), room.data_ptr(), n, L, H, D, code, CS, T, bins, coded["transcode"].data_ptr(), stride,
                            sizes["transcode"].ptr, dev)

    ctx.set_encode_path("two_kernels")
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.5:  # ramp the clock
        encode()
        transcode()
    torch.cuda.synchronize()
    ctx.raise_on_status("ramp")
    assert torch.equal(coded["encode"], coded["transcode"]), "the transcoded blobs differ from the encoded ones"
    assert sizes["encode"].tensor[:4 * n].tolist() == sizes["transcode"].tensor[:4 * n].tolist()
    coded_bytes = sum(sizes["encode"].tensor.view(torch.int32)[:n].tolist())
    ms = {"encode": [], "transcode": []}
    ctx.profile(True)
    for _ in range(RUNS):  # alternating: both sides see the same clock and the same neighbours
        for name, fn in (("encode", encode), ("transcode", transcode)):
            fn()
            torch.cuda.synchronize()
            ms[name].append(ctx.profile_read())
    ctx.profile(False)
    ctx.set_encode_path("auto")
    med = lambda rows, pick: statistics.median(pick(r) for r in rows)
    out = {"runs": RUNS, "tokens": T, "chunks": n, "raw_bytes": raw_bytes, "fixed_bytes": fixed_size * n, "coded_bytes": coded_bytes,
           "encode_two_kernels_ms": med(ms["encode"], sum), "transcode_ms": med(ms["transcode"], sum),
           "k_quantize_ms": med(ms["encode"], lambda r: r[0]), "k_fixed_expand_ms": med(ms["transcode"], lambda r: r[0]),
           "k_cdf_encode_behind_quantize_ms": med(ms["encode"], lambda r: r[1]),
           "k_cdf_encode_behind_expand_ms": med(ms["transcode"], lambda r: r[1]),
           "encode_two_kernels_min_ms": min(sum(r) for r in ms["encode"]), "transcode_min_ms": min(sum(r) for r in ms["transcode"])}
    out["transcode_over_encode"] = round(out["transcode_ms"] / out["encode_two_kernels_ms"], 3)
    out["expand_over_quantize"] = round(out["k_fixed_expand_ms"] / out["k_quantize_ms"], 3)
    ws_bytes = sum((CS // (8 if b <= native.FIXED_NARROW_BINS else 4)) * H * D * 4 for b in bins) * n  # the symbol workspace both kernels write
    out["workspace_bytes"] = ws_bytes
    out["k_fixed_expand_bytes_per_s"] = round((fixed_size * n + ws_bytes) / (out["k_fixed_expand_ms"] * 1e-3))
    out["k_quantize_bytes_per_s"] = round((raw_bytes + ws_bytes) / (out["k_quantize_ms"] * 1e-3))
    # ---- a fixed group's demotion, end to end ----
    codec = get_codec(0)
    arena = PinnedArena()
    walls, pack_bytes = [], 0
    for _ in range(DEMOTIONS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pack = codec.demote_blobs(views, (L, H, D), CS, T, arena, model="fixed", bins=bins)
        walls.append((time.perf_counter() - t0) * 1e3)
        pack_bytes = pack.blob.nbytes
        arena.free(pack.blob)
    out["demotion_wall_ms"] = statistics.median(walls[1:])  # (the first takes the staging and the pinned slab)
    # the coded tier's demotion of the same context (the same leg without the transcode in front), for the difference
    csz = sizes["encode"].tensor.view(torch.int32)[:n].tolist()
    cviews = [coded["encode"][i * stride:i * stride + csz[i]] for i in range(n)]
    cwalls = []
    for _ in range(DEMOTIONS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pack = codec.demote_blobs(cviews, (L, H, D), CS, T, arena)
        cwalls.append((time.perf_counter() - t0) * 1e3)
        assert pack.blob.nbytes == pack_bytes
        arena.free(pack.blob)
    out["demotion_coded_wall_ms"] = statistics.median(cwalls[1:])
    out["demotion_first_wall_ms"] = walls[0]
    out["pack_bytes"] = pack_bytes
    out["pack_at_52GBps_ms"] = round(pack_bytes / PCIE * 1e3, 3)
    out["demotion_over_pcie"] = round(out["demotion_wall_ms"] / out["pack_at_52GBps_ms"], 3)
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(line + "\n")
    arena.close()


if __name__ == "__main__":
    main()
