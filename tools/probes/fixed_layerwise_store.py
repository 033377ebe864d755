"""Times of the fixed-width layer-by-layer store (lmc_encode_layers_begin_fixed, csrc/k_fixed.h) on Llama-3-8B contexts
of 64, 8 and 1 chunks of 256 tokens (block size 16, block-ordered slots), from an "NBHD" cache and from an "NHDB" cache
read in place, HIP events, one process, medians of RUNS runs behind a clock ramp:

  one_piece_ms       lmc_encode_chunks_fixed / _fixed_split of the same source by THIS library
  S=<n>              the layer-wise job with lmc_ctx_set_fixed_layer_slices(n) (0: the library's own rule):
      layer_ms         median per-layer encode time (events on the job's side stream around every encode_layer(l))
      layers_sum_ms    ... summed over the layers
      finish_ms        from finish() to the job's `done` event: k_fixed_layers_finish alone
  event_floor_ms     what the same pair of events shows around ONE launch of a one-element fill: the per-layer and finish
                     figures of small jobs sit on it
  one_piece_ab       lmc_encode_chunks_fixed on the 16 k "NBHD" context by this library and by the parent commit's library
                     loaded beside it, both through the same bare ctypes call, alternating run by run; the _b series
                     are second series in the same rounds, so _a against _b of one library is the A/A spread of the box:
                         LMCACHE_AMD_SO=/path/to/parent/liblmc_hip.so python tools/probes/fixed_layerwise_store.py [out.json]
                     (the variable is taken out of the environment before lmcache_amd.native reads it; without it the
                     comparison is left out)
"""
import ctypes
import json
import os
import statistics
import sys
import time

PARENT_SO = os.environ.pop("LMCACHE_AMD_SO", None)

import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from lmcache_amd import native  # noqa: E402
from lmcache_amd.storage_backend.serde.cachegen_basics import CacheGenConfig  # noqa: E402
from lmcache_amd.storage_backend.serde.cachegen_device import get_codec  # noqa: E402

RUNS = 30
L, H, D, CS, BS = 32, 8, 128, 256, 16
TMAX = 16384
MODEL = "Llama-3-8B"
DEV = torch.device("cuda:0")


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def timed(fn, runs=RUNS):
    return statistics.median(once(fn) for _ in range(runs))


def caches_of(layout, slots, T):
    """Per layer a bf16 cache of the layout holding randn KV at the slots."""
    g = torch.Generator(device=DEV).manual_seed(1)
    nb = TMAX // BS
    out = []
    blk, off = slots // BS, slots % BS
    for _ in range(L):
        x = torch.randn((2, T, H, D), generator=g, device=DEV).to(torch.bfloat16)
        if layout == "NBHD":
            c = torch.zeros((2, nb, BS, H, D), dtype=torch.bfloat16, device=DEV)
            c[:, blk, off] = x
        else:  # NHDB: value cache [nb, H, D, bs]; key cache [nb, H, D / 8, bs, 8] viewed as [nb, H, D, bs]
            c = torch.zeros((2, nb, H, D, BS), dtype=torch.bfloat16, device=DEV)
            c[1][blk, :, :, off] = x[1]
            c[0].view(nb, H, D // 8, BS, 8)[blk, :, :, off, :] = x[0].view(T, H, D // 8, 8)
        out.append(c)
    return out


def raw_encoder(path, lay, T, bins, arena, stride, sizes):
    """lmc_encode_chunks_fixed of the library at `path` through ctypes alone, on a context of its own: the SAME host path
    for both sides of the A/B -- a pair of events around a call also times the host work between the first record and
    the launch, and native.Context's marshalling in front of one side only showed as 4 - 7 us."""
    lib = ctypes.CDLL(path)
    for name in ("lmc_ctx_create", "lmc_encode_chunks_fixed"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = native.SYMBOLS[name]
    pctx = ctypes.c_void_p()
    native.check(lib.lmc_ctx_create(0, ctypes.byref(pctx)), "parent lmc_ctx_create")
    arr = (ctypes.c_int32 * len(bins))(*bins)
    return lambda: native.check(lib.lmc_encode_chunks_fixed(pctx, ctypes.byref(lay.struct), 0, T, CS, arr, arena.data_ptr(), stride,
                                                            sizes.ptr, None, native.current_stream_ptr(DEV)), "parent encode")


def main():
    ctx = native.get_context(0)
    codec = get_codec(0)
    bins = CacheGenConfig.from_model_name(MODEL).plane_bins(L)
    stride = native.r16(native.blob_bound(L, CS, H, D))
    arena = torch.zeros((TMAX // CS) * stride, dtype=torch.uint8, device=DEV)
    sizes = native.PinnedBuffer(4 * (TMAX // CS))
    g = torch.Generator().manual_seed(0)
    all_slots = (torch.randperm(TMAX // BS, generator=g)[:, None] * BS + torch.arange(BS)[None, :]).reshape(-1).to(DEV)
    out = {"runs": RUNS, "parent": bool(PARENT_SO), "cus": torch.cuda.get_device_properties(0).multi_processor_count}
    tiny = torch.zeros(1, dtype=torch.int32, device=DEV)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.5:  # ramp the clock
        tiny.fill_(1)
    out["event_floor_ms"] = timed(lambda: tiny.fill_(1))
    for layout in ("NBHD", "NHDB"):
        for n in (64, 8, 1):
            T = n * CS
            slots = all_slots[:T]
            caches = caches_of(layout, slots, T)
            lay = native.KVLayout.paged(caches, slots, BS, layout)
            one = ctx.encode_chunks_fixed_split if layout == "NHDB" else ctx.encode_chunks_fixed

            def one_piece():
                one(lay, 0, T, CS, bins, arena.data_ptr(), stride, sizes.ptr)

            t0 = time.perf_counter()
            while time.perf_counter() - t0 < 0.5:  # ramp the clock
                one_piece()
            torch.cuda.synchronize()
            r = {"one_piece_ms": timed(one_piece)}
            want = sizes.tensor.view(torch.int32)[:n].tolist()
            if PARENT_SO and layout == "NBHD" and n == 64:
                parent = raw_encoder(PARENT_SO, lay, T, bins, arena, stride, sizes)
                this = raw_encoder(native.SO_PATH, lay, T, bins, arena, stride, sizes)
                series = {"this_a": [], "parent_a": [], "this_b": [], "parent_b": []}
                for _ in range(3 * RUNS):
                    series["this_a"].append(once(this))
                    series["parent_a"].append(once(parent))
                    series["this_b"].append(once(this))
                    series["parent_b"].append(once(parent))
                out["one_piece_ab"] = {k: {"median_ms": statistics.median(v), "min_ms": min(v)} for k, v in series.items()}
            for S in (1, 2, 4, 0):
                ctx.set_fixed_layer_slices(S)
                sums, fins, per_layer = [], [], []
                for run in range(RUNS):
                    job = codec.encode_layers_fixed(lay, 0, T, CS, bins)
                    assert job is not None
                    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * L + 2)]
                    for l in range(L):
                        ev[2 * l].record(job.stream)
                        job.encode_layer(l)
                        ev[2 * l + 1].record(job.stream)
                    ev[2 * L].record(job.stream)
                    job.finish()
                    ev[2 * L + 1].record(job.stream)
                    got = codec.sizes_of(job)  # waits for `done`, raises on a status bit
                    assert got == want, "the layer-wise blobs are not the size of the one-piece blobs"
                    job.offload_issued = True
                    codec.release_layer_stream(job)
                    ms = [ev[2 * l].elapsed_time(ev[2 * l + 1]) for l in range(L)]
                    per_layer.append(statistics.median(ms))
                    sums.append(sum(ms))
                    fins.append(ev[2 * L].elapsed_time(ev[2 * L + 1]))
                r[f"S={S}"] = {"layer_ms": statistics.median(per_layer), "layers_sum_ms": statistics.median(sums),
                               "finish_ms": statistics.median(fins)}
            ctx.set_fixed_layer_slices(0)
            out[f"{layout}/{n}"] = r
            del caches, lay
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(line + "\n")


if __name__ == "__main__":
    main()
