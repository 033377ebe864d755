"""Time of the CacheBlend selection step (k_blend.h) on ONE layer of a 16 k Llama-3-8B context (H = 8, D = 128, bf16:
64 MiB per side) against its yardstick, HIP events, one process, medians of RUNS runs behind a clock ramp:

  deviation  lmc_kv_deviation, both planes: side a = the model's fresh (K, V) pair [T, H, D], side b = the cached layer in
               chunk        a contiguous [1,2,T,H,D] chunk
               nbhd / nhbd  block-ordered paged rows, block size 16
               nhdb         the ROCm paged-attention cache, block-ordered (the V tile form's fast tiles)
               nhdb_random  the same cache, every token at a random slot (element loads on the V side)
  copy       lmc_copy_kv of the same layer between the same two layouts (a -> b): it reads 64 MiB and writes 64 MiB where
             the deviation reads 128 MiB -- the same bytes; alternated with the deviation in two passes
  ratio      deviation / copy; above 1.25 is a finding (reported, not a failure)
  topk       lmc_select_topk at n = 16384, k = 2458 (15 %)
  torch      the connector's formulation for NBHD: index gather of the cached K and V, subtract, square, sum, topk, sort

Every timed deviation is also checked on the device against torch (float64), every selection against torch's sort.

    python tools/probes/blend_select_rates.py [out.json]"""
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__)))))
from lmcache_amd import native  # noqa: E402

RUNS = 30
H, D, T, BS = 8, 128, 16384, 16
K_SEL = 2458


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
    nb = T // BS
    fresh_k = torch.randn(T, H, D, device=dev).to(torch.bfloat16)
    fresh_v = torch.randn(T, H, D, device=dev).to(torch.bfloat16)
    a = native.KVLayout.from_kv_tuple(((fresh_k, fresh_v),), "vllm")
    ordered = (torch.randperm(nb)[:, None] * BS + torch.arange(BS)[None, :]).reshape(-1).to(dev)  # block-ordered, blocks shuffled
    scattered = torch.randperm(nb * BS).to(dev)

    def make(kind):
        """-> (what to keep alive, the layout, a function that gathers the layer as [2, T, H, D])"""
        if kind == "chunk":
            t = torch.randn(1, 2, T, H, D, device=dev).to(torch.bfloat16)
            return t, native.KVLayout.from_chunk(t, "vllm"), lambda: t[0]
        slots = scattered if kind == "nhdb_random" else ordered
        blk, off = slots // BS, slots % BS
        if kind == "nbhd":
            c = torch.randn(2, nb, BS, H, D, device=dev).to(torch.bfloat16)
            return c, native.KVLayout.paged([c], slots, BS, "NBHD"), lambda: c[:, blk, off]
        if kind == "nhbd":
            c = torch.randn(2, nb, H, BS, D, device=dev).to(torch.bfloat16)
            return c, native.KVLayout.paged([c], slots, BS, "NHBD"), lambda: c[:, blk, :, off].permute(1, 0, 2, 3)
        c = torch.randn(2, nb, H, D, BS, device=dev).to(torch.bfloat16)

        def rows():
            k = c[0].view(nb, H, D // 8, BS, 8)[blk, :, :, off].reshape(T, H, D)
            return torch.stack((k, c[1][blk, :, :, off]))
        return c, native.KVLayout.paged([c], slots, BS, "NHDB"), rows

    out = {"runs": RUNS, "shape": {"H": H, "D": D, "tokens": T, "dtype": "bf16", "block_size": BS}, "library": native.SO_PATH,
           "bytes_per_side": 2 * T * H * D * 2}
    dev_k = torch.empty(T, dtype=torch.float32, device=dev)
    dev_v = torch.empty(T, dtype=torch.float32, device=dev)
    for kind in ("chunk", "nbhd", "nhbd", "nhdb", "nhdb_random"):
        keep, b, rows = make(kind)

        def deviation():
            ctx.kv_deviation(a, 0, 0, b, 0, 0, T, dev_k, dev_v)

        # the reference first: the copy below overwrites the cached side with the fresh one
        deviation()
        cached = rows().double()
        want = torch.stack((((fresh_k.double() - cached[0]) ** 2).sum(dim=(1, 2)), ((fresh_v.double() - cached[1]) ** 2).sum(dim=(1, 2))))
        got = torch.stack((dev_k, dev_v)).double()
        r = {"max_rel_err_vs_float64": float(((got - want).abs() / want).max())}
        del cached, want, got

        def copy():
            ctx.copy_kv(a, 0, T, b, 0)

        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.5:  # ramp the clock
            deviation()
        torch.cuda.synchronize()
        for p in ("a", "b"):  # alternating, twice: a drift of the clock shows as a difference between the passes
            r["deviation_ms_" + p] = timed(deviation)
            r["copy_ms_" + p] = timed(copy)
        for name in ("deviation_ms", "copy_ms"):
            r[name] = min(r[name + "_a"], r[name + "_b"])
        r["ratio"] = r["deviation_ms"] / r["copy_ms"]
        r["deviation_GBps"] = 2 * out["bytes_per_side"] / r["deviation_ms"] / 1e6
        r["copy_GBps"] = 2 * out["bytes_per_side"] / r["copy_ms"] / 1e6
        out[kind] = r
        del keep, b, rows
        torch.cuda.empty_cache()

    # selection
    devs = (torch.randn(T, device=dev) ** 2).contiguous()
    idx = torch.empty(K_SEL, dtype=torch.int32, device=dev)

    def topk():
        ctx.select_topk(devs, K_SEL, idx)

    topk()
    order = torch.sort(devs, descending=True, stable=True).indices[:K_SEL]
    out["topk"] = {"n": T, "k": K_SEL, "ms": timed(topk),
                   "equal_to_torch_stable_sort": bool(torch.equal(idx.long(), torch.sort(order).values))}

    # the torch formulation, NBHD
    c = torch.randn(2, nb, BS, H, D, device=dev).to(torch.bfloat16)
    blk, off = ordered // BS, ordered % BS

    def torch_deviation():
        ck, cv = c[0][blk, off], c[1][blk, off]
        return ((fresh_k.float() - ck.float()) ** 2).sum(dim=(1, 2)), ((fresh_v.float() - cv.float()) ** 2).sum(dim=(1, 2))

    def torch_select():
        return torch.sort(torch.topk(torch_deviation()[1], K_SEL).indices).values

    def torch_topk_only():
        return torch.sort(torch.topk(devs, K_SEL).indices).values

    for _ in range(3):
        torch_select()
    b = native.KVLayout.paged([c], ordered, BS, "NBHD")

    def ours():
        ctx.kv_deviation(a, 0, 0, b, 0, 0, T, dev_k, dev_v)
        ctx.select_topk(dev_v, K_SEL, idx)

    out["torch_nbhd"] = {"deviation_both_planes_ms": timed(lambda: torch_deviation()), "topk_sort_ms": timed(torch_topk_only),
                         "ours_deviation_and_topk_ms": timed(ours)}
    out["torch_nbhd"]["ratio_torch_over_ours"] = (out["torch_nbhd"]["deviation_both_planes_ms"] + out["torch_nbhd"]["topk_sort_ms"]) / \
        out["torch_nbhd"]["ours_deviation_and_topk_ms"]
    ctx.raise_on_status("blend select probe")
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(line + "\n")


if __name__ == "__main__":
    main()
