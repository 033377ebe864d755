"""Time of lmc_rope_shift (k_rope.h) on one 16 k Llama-3-8B context (L = 32, H = 8, D = rot = 128, bf16) against its
yardstick, HIP events, one process, medians of RUNS runs behind a clock ramp:

  shift      lmc_rope_shift of all 16 k tokens, uniform delta and per-token deltas, on
               chunk   a contiguous [L,2,T,H,D] chunk
               nhbd    a block-ordered "NHBD" paged cache, block size 16
  copy       lmc_copy_kv of the same token range between two such layouts (chunk -> chunk, nhbd -> nhbd).  The copy reads
             and writes K and V, the shift reads and writes K only: the yardstick is HALF the copy's time
  ratio      shift / (copy / 2); above 1.25 ("same bytes at HBM speed") is a finding

The result of every timed shift is also checked, on the device, against the formula in torch (separate fp32 ops).

    python tools/probes/rope_shift_rates.py [out.json]

LMCACHE_AMD_SO=<another build> times that build instead (e.g. one compiled with -DLMC_ROPE_NT=0: k_rope.h with plain
instead of non-temporal loads and stores)."""
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__)))))
from lmcache_amd import native  # noqa: E402
from lmcache_amd.rope import RopeShift  # noqa: E402

RUNS = 30
L, H, D, T, BS = 32, 8, 128, 16384, 16
ROWS = 32768


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


def torch_shift(k, table, deltas):
    """k [..., T, H, D] on the device, rotated by deltas [T] (NeoX, rot = D): the header's formula, one op per step."""
    x = k.float()
    h = D // 2
    c = table[deltas.abs().long(), :h][:, None, :]
    s = table[deltas.abs().long(), h:][:, None, :] * torch.where(deltas < 0, -1.0, 1.0)[:, None, None]
    x1, x2 = x[..., :h], x[..., h:]
    a, b = x1 * c, x2 * s
    o1 = a - b
    a, b = x2 * c, x1 * s
    o2 = a + b
    return torch.cat((o1, o2), dim=-1).to(k.dtype)


def main():
    dev = torch.device("cuda:0")
    ctx = native.get_context(0)
    torch.manual_seed(0)
    rope = RopeShift.from_base(500000.0, D, ROWS, dev)
    table = rope.cos_sin
    deltas = torch.randint(-(ROWS - 1), ROWS, (T,), dtype=torch.int32).to(dev)
    uniform = torch.full((T,), 4097, dtype=torch.int32, device=dev)
    nb = T // BS
    slots = (torch.randperm(nb)[:, None] * BS + torch.arange(BS)[None, :]).reshape(-1).to(dev)  # block-ordered, blocks shuffled

    def make(kind):
        if kind == "chunk":
            t = torch.randn(L, 2, T, H, D, device=dev).to(torch.bfloat16)
            return t, native.KVLayout.from_chunk(t, "vllm"), lambda: t[:, 0]
        caches = [torch.randn(2, nb, H, BS, D, device=dev).to(torch.bfloat16) for _ in range(L)]
        blk, off = slots // BS, slots % BS
        return caches, native.KVLayout.paged(caches, slots, BS, "NHBD"), lambda: torch.stack([c[0, blk, :, off] for c in caches])

    out = {"runs": RUNS, "shape": {"L": L, "H": H, "D": D, "rot": D, "tokens": T, "dtype": "bf16", "block_size": BS},
           "library": native.SO_PATH, "k_bytes": L * T * H * D * 2}
    for kind in ("chunk", "nhbd"):
        _, src, keys = make(kind)
        _, dst, _ = make(kind)

        def copy():
            ctx.copy_kv(src, 0, T, dst, 0)

        def shift_uniform():
            ctx.rope_shift(src, 0, T, table, D, True, delta=4097)

        def shift_per_token():
            ctx.rope_shift(src, 0, T, table, D, True, deltas=deltas)

        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.5:  # ramp the clock
            copy()
        torch.cuda.synchronize()
        r = {}
        # the three timed back to back, twice, so that a drift of the clock shows as a difference between the passes
        for p in ("a", "b"):
            r["copy_ms_" + p] = timed(copy)
            r["shift_uniform_ms_" + p] = timed(shift_uniform)
            r["shift_per_token_ms_" + p] = timed(shift_per_token)
        for name in ("copy_ms", "shift_uniform_ms", "shift_per_token_ms"):
            r[name] = min(r[name + "_a"], r[name + "_b"])
        r["yardstick_ms"] = r["copy_ms"] / 2
        r["ratio_uniform"] = r["shift_uniform_ms"] / r["yardstick_ms"]
        r["ratio_per_token"] = r["shift_per_token_ms"] / r["yardstick_ms"]
        r["shift_uniform_GBps"] = 2 * out["k_bytes"] / r["shift_uniform_ms"] / 1e6  # K read once and written once
        r["copy_GBps"] = 4 * out["k_bytes"] / r["copy_ms"] / 1e6                     # K and V read and written
        # what the kernel computes, against torch on the device (the keys have been rotated many times by now: still finite)
        for name, d, fn in (("uniform", uniform, shift_uniform), ("per_token", deltas, shift_per_token)):
            before = keys().clone()
            fn()
            torch.cuda.synchronize()
            r["bit_equal_to_torch_" + name] = bool(torch.equal(keys().view(torch.int16), torch_shift(before, table, d).view(torch.int16)))
        out[kind] = r
        del src, dst, keys
        torch.cuda.empty_cache()
    ctx.raise_on_status("rope shift probe")
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(line + "\n")


if __name__ == "__main__":
    main()
