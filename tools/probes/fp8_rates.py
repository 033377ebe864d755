"""fp8 KV against its bf16 upcast on bench.py's shape (Llama-3-8B: L = 32, H = 8, D = 128, 16 k tokens, 256-token chunks):
encode, decode into a contiguous and into a paged (NBHD, random slots) destination, the pinned cachegen / raw tiers'
store and retrieve, blob bytes.  The same seeded values as fp8 and as their bf16 images, timed alternately in one
process with device events after a warm-up; median and spread (min .. max) of --steps runs each.

  python tools/probes/fp8_rates.py --steps 20            # JSON on stdout; profiles/fp8_kv.md holds a run's figures
Kernel times: the same script with --no-engine under rocprofv3 --kernel-trace --stats (a run of its own), counters in a
third run (rocprofv3 --pmc).  Both fp8 formats are measured against the same bf16 images."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from lmcache_amd import native  # noqa: E402

L, H, D, CS = 32, 8, 128, 256


def _t(fn, steps, warm=3):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    out.sort()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--tokens", type=int, default=16384)
    ap.add_argument("--no-engine", action="store_true", help="kernels only: skip the engine tiers")
    args = ap.parse_args()
    T = args.tokens
    torch.manual_seed(0)
    x8 = (torch.randn(L, 2, T, H, D, device="cuda") * 4).to(torch.float8_e4m3fn)
    x5 = (torch.randn(L, 2, T, H, D, device="cuda") * 4).to(torch.float8_e5m2)
    xs = {"fp8_e4m3": x8, "bf16": x8.to(torch.bfloat16), "fp8_e5m2": x5, "bf16_of_e5m2": x5.to(torch.bfloat16)}
    ctx = native.get_context(0)
    bins = [32] * 4 + [16] * (L - 4) + [16] * L
    n = T // CS
    stride = native.r16(native.blob_bound(L, CS, H, D))
    blobs = torch.zeros(n * stride, dtype=torch.uint8, device="cuda")
    sizes = torch.zeros(n, dtype=torch.int32, device="cuda")
    bs = 16
    nblocks = T // bs + 8
    slots = torch.randperm(nblocks * bs, device="cuda")[:T]
    res = {k: {} for k in xs}
    # alternate the two dtypes step by step
    for rep in range(args.steps):
        for name, x in xs.items():
            src = native.KVLayout.from_chunk(x, "vllm")
            enc = lambda: ctx.encode_chunks(src, 0, T, CS, bins, blobs.data_ptr(), stride, sizes.data_ptr())
            r = res[name]
            r.setdefault("encode_ms", []).extend(_t(enc, 1, warm=2 if rep == 0 else 0))
            total = int(sizes.sum())
            r["blob_bytes"] = total
            out = torch.empty_like(x)
            dst = native.KVLayout.from_chunk(out, "vllm")
            r.setdefault("decode_contiguous_ms", []).extend(
                _t(lambda: ctx.decode_chunks(blobs.data_ptr(), stride, n, dst, 0, CS), 1, warm=2 if rep == 0 else 0))
            pc = [torch.empty((2, nblocks, bs, H, D), dtype=x.dtype, device="cuda") for _ in range(L)]
            pdst = native.KVLayout.paged(pc, slots, bs, "NBHD")
            r.setdefault("decode_paged_ms", []).extend(
                _t(lambda: ctx.decode_chunks(blobs.data_ptr(), stride, n, pdst, 0, CS), 1, warm=2 if rep == 0 else 0))
            ctx.raise_on_status("probe")
    for name, r in res.items():
        for k in list(r):
            if k.endswith("_ms"):
                v = sorted(r[k])
                r[k] = {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "n": len(v)}
        raw = L * 2 * T * H * D * (1 if name.startswith("fp8") else 2)
        r["raw_bytes"] = raw
        r["ratio_vs_raw"] = raw / r["blob_bytes"]
    if args.no_engine:
        print(json.dumps(res, indent=1))
        return
    # the engine's pinned tiers (store + retrieve of the whole context), same alternation
    from lmcache_amd.cache_engine import LMCacheEngine
    from lmcache_amd.config import LMCacheEngineConfig, LMCacheEngineMetadata
    meta = LMCacheEngineMetadata("meta-llama/Meta-Llama-3-8B", 1, 0, "vllm", "bfloat16")
    for tier, cfg in (("cachegen", dict(backend="cpu", local_serde="cachegen")), ("raw", dict(backend="cpu"))):
        tok = torch.randint(0, 30000, (T,), device="cuda")
        for name, x in xs.items():
            kv = tuple((x[l, 0], x[l, 1]) for l in range(L))
            st, rt = [], []
            for rep in range(max(3, args.steps // 4)):
                eng = LMCacheEngine(LMCacheEngineConfig.from_legacy(chunk_size=CS, **cfg), meta)
                try:
                    st += _t(lambda: eng.store(tok, kv), 1, warm=0)
                    rt += _t(lambda: eng.retrieve(tok), 1, warm=1)
                finally:
                    eng.close()
            st.sort(), rt.sort()
            res[name][f"{tier}_store_ms"] = {"median": st[len(st) // 2], "min": st[0], "max": st[-1], "n": len(st)}
            res[name][f"{tier}_retrieve_ms"] = {"median": rt[len(rt) // 2], "min": rt[0], "max": rt[-1], "n": len(rt)}
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
