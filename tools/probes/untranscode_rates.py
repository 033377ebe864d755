"""Rates of lmc_transcode_to_fixed (csrc/k_decode.h, DEC_SINK_FIXED: the rANS decoder with a fixed-width sink) on one 16 k
Llama-3-8B bf16 context (64 chunks of 256 tokens): one process, a clock ramp, medians of RUNS runs taken ALTERNATING
between the two sides, kernel times from lmc_ctx_profile (HIP events around each kernel), one JSON line.

  untranscode  lmc_transcode_to_fixed of the context's entropy-coded blobs  |  the plain lmc_decode_chunks of the same blobs
               into contiguous bf16 KV: the same token loop, 2 bytes stored per symbol against 4 or 5 bits
  promotion    wall time of CacheGenDeviceCodec.promote_pack(model="fixed") of the whole context as one pack -- the unpack
               into the codec's staging (DMA + one scatter kernel), the table upload, the transcode, the host waits --
               against the coded tier's promote_pack of the same pack (the unpack alone, into the arena), and against the
               pack's bytes at 52 GB/s

    python tools/probes/untranscode_rates.py [out.json] [--tokens N]       (N: the context's length, default 16384)
"""
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__)))))
from lmcache_amd import native  # noqa: E402
from lmcache_amd.storage_backend.serde.cachegen_basics import CacheGenConfig  # noqa: E402
from lmcache_amd.storage_backend.serde.cachegen_device import DeviceArena, PinnedArena, get_codec  # noqa: E402

RUNS = 30
PROMOTIONS = 7
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
    coded = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
    want = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
    got = torch.zeros(n * stride, dtype=torch.uint8, device=dev)
    sizes = native.PinnedBuffer(4 * n)
    fsizes = native.PinnedBuffer(4 * n)
    ctx.encode_chunks(lay, 0, T, CS, bins, coded.data_ptr(), stride, sizes.ptr)
    ctx.encode_chunks_fixed(lay, 0, T, CS, bins, want.data_ptr(), stride, fsizes.ptr)
    torch.cuda.synchronize()
    ctx.raise_on_status("encode")
    csz = sizes.tensor.view(torch.int32)[:n].tolist()
    table = torch.tensor([coded.data_ptr() + i * stride for i in range(n)], dtype=torch.int64).to(dev)
    room = torch.tensor(csz, dtype=torch.int32).to(dev)
    outs = torch.tensor([got.data_ptr() + i * stride for i in range(n)], dtype=torch.int64).to(dev)
    oroom = torch.tensor([fixed_size] * n, dtype=torch.int32).to(dev)
    code = native.dtype_code(torch.bfloat16)
    dst = torch.zeros_like(kv)
    dlay = native.KVLayout.from_chunk(dst, "vllm")

    def decode():
        ctx.decode_chunks(coded.data_ptr(), stride, n, dlay, 0, CS)

    def untranscode():
        ctx.transcode_to_fixed(table.data_ptr(), room.data_ptr(), n, L, H, D, code, CS, T, bins, outs.data_ptr(), oroom.data_ptr(), dev)

    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.5:  # ramp the clock
        decode()
        untranscode()
    torch.cuda.synchronize()
    ctx.raise_on_status("ramp")
    assert torch.equal(got, want), "the transcoded blobs differ from the fixed-width encode's"
    ms = {"decode": [], "untranscode": []}
    ctx.profile(True)
    for _ in range(RUNS):  # alternating: both sides see the same clock and the same neighbours
        for name, fn in (("decode", decode), ("untranscode", untranscode)):
            fn()
            torch.cuda.synchronize()
            ms[name].append(sum(ctx.profile_read()))
    ctx.profile(False)
    out = {"runs": RUNS, "tokens": T, "chunks": n, "raw_bytes": raw_bytes, "fixed_bytes": fixed_size * n, "coded_bytes": sum(csz),
           "decode_ms": statistics.median(ms["decode"]), "untranscode_ms": statistics.median(ms["untranscode"]),
           "decode_min_ms": min(ms["decode"]), "untranscode_min_ms": min(ms["untranscode"])}
    out["untranscode_over_decode"] = round(out["untranscode_ms"] / out["decode_ms"], 3)
    # ---- a demoted fixed-width group's promotion, end to end, against the coded tier's of the same pack ----
    codec = get_codec(0)
    host = PinnedArena()
    cviews = [coded[i * stride:i * stride + csz[i]] for i in range(n)]
    pack = codec.demote_blobs(cviews, (L, H, D), CS, T, host)
    walls = {"fixed": [], "coded": []}
    for _ in range(PROMOTIONS):
        for name, kw in (("coded", {}), ("fixed", {"model": "fixed", "bins": bins})):
            hbm = DeviceArena(dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            blobs = codec.promote_pack(pack, hbm, **kw)
            walls[name].append((time.perf_counter() - t0) * 1e3)
            if name == "fixed":
                assert all(torch.equal(b, want[i * stride:i * stride + fixed_size]) for i, b in enumerate(blobs))
            del blobs
            hbm.close()
    out["promotion_wall_ms"] = statistics.median(walls["fixed"][1:])  # (the first takes the staging and the arena's slab)
    out["promotion_coded_wall_ms"] = statistics.median(walls["coded"][1:])
    out["promotion_first_wall_ms"] = walls["fixed"][0]
    out["pack_bytes"] = pack.blob.nbytes
    out["pack_at_52GBps_ms"] = round(pack.blob.nbytes / PCIE * 1e3, 3)
    out["promotion_over_pcie"] = round(out["promotion_wall_ms"] / out["pack_at_52GBps_ms"], 3)
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(line + "\n")
    host.close()


if __name__ == "__main__":
    main()
