"""Rates of the fixed-width model (LMC_MODEL_FIXED, csrc/k_fixed.h) against the entropy-coded path on one 16 k Llama-3-8B
bf16 context (64 chunks of 256 tokens): one process, a clock ramp, medians of RUNS runs, per-kernel times from
lmc_ctx_profile (HIP events around each kernel), one JSON line.

  encode   lmc_encode_chunks_fixed  |  the fused lmc_encode_chunks  |  the k_quantize launch alone of the two-kernel path
           (the same reads, about the same bytes written: the fixed-width encoder's streaming yardstick)
  decode   lmc_decode_chunks_fixed_schedule (one range) | lmc_decode_chunks_schedule, into contiguous rows and into "NHBD"
           blocks through a block-ordered slot mapping; lmc_copy_kv of the raw KV as the streaming yardstick
  size     blob bytes of both models on rand / randn / outlier data

    python tools/probes/fixed_rates.py [out.json] [--tokens N]       (N: the context's length, default 16384)
"""
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__)))))
from lmcache_amd import native  # noqa: E402
from lmcache_amd.storage_backend.serde.cachegen_basics import CacheGenConfig  # noqa: E402

RUNS = 30
L, H, D, T, CS = 32, 8, 128, 16384, 256
if "--tokens" in sys.argv:
    _i = sys.argv.index("--tokens")
    T = int(sys.argv[_i + 1])
    del sys.argv[_i:_i + 2]
MODEL = "Llama-3-8B"
HBM_PEAK = 8.0e12  # bytes / s, the datasheet figure DESIGN.md's shares of peak are taken against


def make(kind, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    if kind == "rand":
        x = torch.rand(L, 2, T, H, D, generator=g, device=dev)
    else:
        x = torch.randn(L, 2, T, H, D, generator=g, device=dev)
        if kind == "outlier":
            x *= torch.exp(1.5 * torch.randn(H, D, generator=g, device=dev))
    return x.to(torch.bfloat16)


def main():
    dev = torch.device("cuda:0")
    ctx = native.get_context(0)
    bins = CacheGenConfig.from_model_name(MODEL).plane_bins(L)
    n = T // CS
    stride = native.r16(native.blob_bound(L, CS, H, D))
    arenas = {m: torch.zeros(n * stride, dtype=torch.uint8, device=dev) for m in ("fixed", "coded")}
    sizes = native.PinnedBuffer(4 * n)
    kv = make("rand", dev)
    lay = native.KVLayout.from_chunk(kv, "vllm")
    raw_bytes = kv.numel() * 2

    def enc(model):
        call = ctx.encode_chunks_fixed if model == "fixed" else ctx.encode_chunks
        call(lay, 0, T, CS, bins, arenas[model].data_ptr(), stride, sizes.ptr)

    def profiled(fn, pick=sum):
        ctx.profile(True)
        ms = []
        for _ in range(RUNS):
            fn()
            torch.cuda.synchronize()
            ms.append(pick(ctx.profile_read()))
        ctx.profile(False)
        return statistics.median(ms)

    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.5:  # ramp the clock
        enc("fixed")
    torch.cuda.synchronize()
    out = {"runs": RUNS, "tokens": T, "chunks": n, "raw_bytes": raw_bytes}
    # ---- sizes ----
    for kind in ("rand", "randn", "outlier"):
        x = make(kind, dev)
        xl = native.KVLayout.from_chunk(x, "vllm")
        for model, call in (("fixed", ctx.encode_chunks_fixed), ("coded", ctx.encode_chunks)):
            call(xl, 0, T, CS, bins, arenas[model].data_ptr(), stride, sizes.ptr)
            torch.cuda.synchronize()
            ctx.raise_on_status("encode")
            total = sum(sizes.tensor.view(torch.int32)[:n].tolist())
            out[f"{kind}_{model}_bytes"] = total
            out[f"{kind}_{model}_ratio"] = round(raw_bytes / total, 3)
        del x, xl
    # ---- encode ----
    out["encode_fixed_ms"] = profiled(lambda: enc("fixed"))
    ctx.set_encode_path("fused")
    out["encode_fused_ms"] = profiled(lambda: enc("coded"))
    ctx.set_encode_path("two_kernels")
    out["k_quantize_ms"] = profiled(lambda: enc("coded"), pick=lambda ms: ms[0])
    out["encode_two_kernels_ms"] = profiled(lambda: enc("coded"))
    ctx.set_encode_path("auto")
    fixed_bytes = native.fixed_blob_bytes(L, CS, H, D, bins) * n
    out["encode_fixed_bytes_moved"] = raw_bytes + fixed_bytes
    out["encode_fixed_share_of_hbm_peak"] = round((raw_bytes + fixed_bytes) / (out["encode_fixed_ms"] * 1e-3) / HBM_PEAK, 3)
    out["encode_fixed_over_k_quantize"] = round(out["encode_fixed_ms"] / out["k_quantize_ms"], 3)
    out["encode_fixed_over_fused"] = round(out["encode_fixed_ms"] / out["encode_fused_ms"], 3)
    # ---- decode ----
    for m in ("fixed", "coded"):
        enc(m)
    torch.cuda.synchronize()
    ctx.raise_on_status("encode")
    tables = {m: torch.tensor([arenas[m].data_ptr() + i * stride for i in range(n)], dtype=torch.int64).to(dev) for m in arenas}
    rows = torch.zeros(L, 2, T, H, D, dtype=torch.bfloat16, device=dev)
    bs = 16
    nb = T // bs + 4
    perm = torch.randperm(nb, generator=torch.Generator().manual_seed(1))[:T // bs]
    slots = (perm[:, None] * bs + torch.arange(bs)[None, :]).reshape(-1).to(dev)
    caches = [torch.zeros(2, nb, H, bs, D, dtype=torch.bfloat16, device=dev) for _ in range(L)]
    dsts = {"rows": native.KVLayout.from_chunk(rows, "vllm"), "nhbd": native.KVLayout.paged(caches, slots, bs, "NHBD")}
    for name, dst in dsts.items():
        fx = lambda: ctx.decode_chunks_fixed_schedule(tables["fixed"].data_ptr(), stride, n, dst, 0, CS, [L], None)
        cd = lambda: ctx.decode_chunks_schedule(tables["coded"].data_ptr(), stride, n, dst, 0, CS, [L], None)
        cd()
        torch.cuda.synchronize()
        ctx.raise_on_status("decode")
        want = [c.clone() for c in caches] if name == "nhbd" else rows.clone()
        fx()
        torch.cuda.synchronize()
        ctx.raise_on_status("fixed decode")
        same = all(torch.equal(a, b) for a, b in zip(caches, want)) if name == "nhbd" else torch.equal(rows, want)
        assert same, "the two models decode to different bits"
        out[f"decode_fixed_{name}_ms"] = profiled(fx)
        out[f"decode_coded_{name}_ms"] = profiled(cd)
        out[f"decode_fixed_over_coded_{name}"] = round(out[f"decode_fixed_{name}_ms"] / out[f"decode_coded_{name}_ms"], 3)
        out[f"decode_fixed_{name}_share_of_hbm_peak"] = round((raw_bytes + fixed_bytes) / (out[f"decode_fixed_{name}_ms"] * 1e-3) / HBM_PEAK, 3)
    copy = torch.zeros_like(rows)
    cl = native.KVLayout.from_chunk(copy, "vllm")
    ms = []
    for _ in range(RUNS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ctx.copy_kv(lay, 0, T, cl, 0)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    out["copy_kv_ms"] = statistics.median(ms)
    out["copy_kv_share_of_hbm_peak"] = round(2 * raw_bytes / (out["copy_kv_ms"] * 1e-3) / HBM_PEAK, 3)
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(line + "\n")


if __name__ == "__main__":
    main()
