"""Time of a rope-shifted retrieve from the fixed-width HBM tier with the rotation INSIDE the decode
(LMCACHE_AMD_FUSED_ROPE=1: lmc_decode_chunks_fixed_rope_schedule, k_fixed.h: k_fixed_decode_rope) against the two-pass
path, on one 16 k Llama-3-8B context (L = 32, H = 8, D = rot = 128, bf16, block size 16, block-ordered slots).  HIP events,
one process, the two engines ALTERNATING run by run, medians of RUNS runs behind a clock ramp, with the run-to-run spread
(the quartiles) beside every median.

  NHDB direct  fused against direct + lmc_rope_shift_split (the off side is built with LMCACHE_AMD_SPLIT_ROPE=1)
  NHBD         fused against decode + lmc_rope_shift in the cache
  each with one delta and with per-token deltas
  plain        the same retrieve WITHOUT rope on both engines (k_fixed_decode, which the fused switch must not touch);
               LMCACHE_AMD_SO=<the parent commit's build> times that library's plain decode for the comparison across builds

    python tools/probes/fused_rope_rates.py [out.json]"""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from lmcache_amd import native  # noqa: E402
from lmcache_amd.cache_engine import LMCacheEngine  # noqa: E402
from lmcache_amd.config import LMCacheEngineConfig, LMCacheEngineMetadata  # noqa: E402
from lmcache_amd.rope import RopeShift  # noqa: E402

RUNS = 30
L, H, D, T, BS = 32, 8, 128, 16384, 16
ROWS = 32768
CHUNK = 256


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def engine(fused, split):
    os.environ["LMCACHE_AMD_FUSED_ROPE"] = "1" if fused else "0"  # (both read when the engine is built)
    os.environ["LMCACHE_AMD_SPLIT_ROPE"] = "1" if split else "0"
    try:
        meta = LMCacheEngineMetadata("Llama-3-8B", 1, 0, "vllm", "half")
        return LMCacheEngine(LMCacheEngineConfig.from_legacy(chunk_size=CHUNK, backend="cuda", local_serde="cachegen-fixed"), meta)
    finally:
        del os.environ["LMCACHE_AMD_FUSED_ROPE"], os.environ["LMCACHE_AMD_SPLIT_ROPE"]


def summary(v):
    q = statistics.quantiles(v, n=4)
    return {"median_ms": statistics.median(v), "q1_ms": q[0], "q3_ms": q[2]}


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    has_fused = hasattr(native.lib(), "lmc_decode_chunks_fixed_rope_schedule")  # (the parent's build: the plain legs only)
    tokens = torch.randint(0, 10000, (T,)).to(dev)
    kv = tuple((torch.rand((T, H, D), device=dev).to(torch.bfloat16), torch.rand((T, H, D), device=dev).to(torch.bfloat16))
               for _ in range(L))
    nb = T // BS
    slots = (torch.randperm(nb)[:, None] * BS + torch.arange(BS)[None, :]).reshape(-1).to(dev)  # block-ordered, blocks shuffled
    one = RopeShift.from_base(500000.0, D, ROWS, dev, is_neox=True, delta=4097)
    per_token = RopeShift(one.cos_sin, D, True, torch.randint(-(ROWS - 1), ROWS, (T,), dtype=torch.int32).to(dev))
    out = {"runs": RUNS, "shape": {"L": L, "H": H, "D": D, "rot": D, "tokens": T, "dtype": "bf16", "block_size": BS},
           "library": native.SO_PATH, "cases": {}}
    engines = {"two_pass": engine(False, True)}
    if has_fused:
        engines["fused"] = engine(True, False)
    try:
        for e in engines.values():
            e.store(tokens, kv)
        torch.cuda.synchronize()
        for layout, shape in (("NHDB", (2, nb, H, D, BS)), ("NHBD", (2, nb, H, BS, D))):
            caches = {n: [torch.zeros(shape, device=dev, dtype=torch.bfloat16) for _ in range(L)] for n in engines}
            for rope_name, rope in (("plain", None), ("one_delta", one), ("per_token", per_token)):
                def call(n):
                    m = engines[n].retrieve_into_paged(tokens, caches[n], slots, BS, layout, rope=rope, direct=True)
                    assert bool(m.all())

                t0 = time.perf_counter()
                while time.perf_counter() - t0 < 0.5:  # ramp the clock; whatever the tier keeps across calls is there
                    for n in engines:
                        call(n)
                torch.cuda.synchronize()
                ms = {n: [] for n in engines}
                for _ in range(RUNS):  # alternating: a drift of the clock falls on both alike
                    for n in engines:
                        torch.cuda.synchronize()
                        ms[n].append(once(lambda: call(n)))
                r = {n: summary(v) for n, v in ms.items()}
                if has_fused:
                    r["ratio"] = r["fused"]["median_ms"] / r["two_pass"]["median_ms"]
                    a, b = caches["two_pass"], caches["fused"]
                    r["v_bit_equal"] = all(torch.equal(x[1].view(torch.int16), y[1].view(torch.int16)) for x, y in zip(a, b))
                    r["k_max_abs_diff"] = max(float((x[0].float() - y[0].float()).abs().max()) for x, y in zip(a, b))
                out["cases"][f"{layout}/{rope_name}"] = r
            del caches
            torch.cuda.empty_cache()
    finally:
        for e in engines.values():
            e.close()
    native.get_context(0).raise_on_status("fused rope probe")
    line = json.dumps(out)
    print(line)
    if args:
        open(args[0], "w").write(line + "\n")


if __name__ == "__main__":
    main()
