"""Times of the layer-by-layer store (lmc_encode_layers_*, csrc/k_layers.h) on one 16 k Llama-3-8B context (64 chunks of
256 tokens, block size 16, block-ordered slots), from an "NBHD" cache and from an "NHDB" cache read in place
(direct=True), HIP events, one process, medians of RUNS runs behind a clock ramp:

  layers_sum_ms      the summed per-layer encode times: events on the job's side stream around every encode_layer(l)
  layer_ms           ... and their median per layer
  finish_ms          from finish() to the job's `done` event: k_layers_finish alone (the tier's copies come behind it)
  one_piece_ms       the one-piece encode of the same source by THIS library (lmc_encode_chunks / lmc_encode_chunks_split),
                     as the library chooses its kernels ("auto") and with the two kernels the layer launches use
  parent_*_ms        the same by the parent commit's library, loaded into this process beside this one:
                         LMCACHE_AMD_SO=/path/to/parent/liblmc_hip.so python tools/probes/layerwise_store.py [out.json]
                     (the variable is taken out of the environment before lmcache_amd.native reads it: the package runs on
                     the tree's own library; without it the parent columns are left out)
  engine             wall times through LMCacheEngine on the HBM-encoded tier: store_paged(blocking=True) against the
                     finish() of store_paged_layerwise behind a forward pass that has already saved every layer
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
L, H, D, T, CS, BS = 32, 8, 128, 16384, 256, 16
MODEL = "Llama-3-8B"
DEV = torch.device("cuda:0")


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


def caches_of(layout, slots):
    """Per layer a bf16 cache of the layout holding randn KV at the slots."""
    g = torch.Generator(device=DEV).manual_seed(1)
    nb = T // BS
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


class Parent:
    """The parent commit's library beside this one: its own context, the two one-piece entry points."""

    def __init__(self, path):
        self.lib = ctypes.CDLL(path)
        for name in ("lmc_ctx_create", "lmc_ctx_destroy", "lmc_ctx_set_encode_path", "lmc_encode_chunks", "lmc_encode_chunks_split"):
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = native.SYMBOLS[name]
        self.ctx = ctypes.c_void_p()
        native.check(self.lib.lmc_ctx_create(0, ctypes.byref(self.ctx)), "parent lmc_ctx_create")

    def encoder(self, lay, bins, arena, stride, sizes):
        fn = self.lib.lmc_encode_chunks_split if lay.struct.paged_kind == native.PAGED_SPLIT else self.lib.lmc_encode_chunks
        arr = (ctypes.c_int32 * len(bins))(*bins)
        return lambda: native.check(fn(self.ctx, ctypes.byref(lay.struct), 0, T, CS, arr, arena.data_ptr(), stride, sizes.ptr, None,
                                       native.current_stream_ptr(DEV)), "parent encode")

    def path(self, p):
        native.check(self.lib.lmc_ctx_set_encode_path(self.ctx, native.ENCODE_PATHS[p]), "parent set_encode_path")


def main():
    ctx = native.get_context(0)
    codec = get_codec(0)
    bins = CacheGenConfig.from_model_name(MODEL).plane_bins(L)
    n = T // CS
    stride = native.r16(native.blob_bound(L, CS, H, D))
    arena = torch.zeros(n * stride, dtype=torch.uint8, device=DEV)
    sizes = native.PinnedBuffer(4 * n)
    parent = Parent(PARENT_SO) if PARENT_SO else None
    g = torch.Generator().manual_seed(0)
    slots = (torch.randperm(T // BS, generator=g)[:, None] * BS + torch.arange(BS)[None, :]).reshape(-1).to(DEV)
    out = {"runs": RUNS, "chunks": n, "parent": bool(parent)}
    for layout in ("NBHD", "NHDB"):
        caches = caches_of(layout, slots)
        lay = native.KVLayout.paged(caches, slots, BS, layout)
        one = ctx.encode_chunks_split if layout == "NHDB" else ctx.encode_chunks

        def one_piece():
            one(lay, 0, T, CS, bins, arena.data_ptr(), stride, sizes.ptr)

        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.5:  # ramp the clock
            one_piece()
        torch.cuda.synchronize()
        r = {}
        for path in ("auto", "two_kernels"):
            ctx.set_encode_path(path)
            r[f"one_piece_{path}_ms"] = timed(one_piece)
            if parent:
                parent.path(path)
                r[f"parent_{path}_ms"] = timed(parent.encoder(lay, bins, arena, stride, sizes))
        ctx.set_encode_path("auto")
        if parent:
            parent.path("auto")
        one_piece()
        torch.cuda.synchronize()
        want = sizes.tensor.view(torch.int32)[:n].tolist()
        sums, fins, per_layer = [], [], []
        for run in range(RUNS):
            job = codec.encode_layers(lay, 0, T, CS, bins)
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
        r["layers_sum_ms"], r["layer_ms"], r["finish_ms"] = statistics.median(sums), statistics.median(per_layer), statistics.median(fins)
        r["blob_bytes"] = sum(want)
        out[layout] = r
        del caches, lay
    # through the engine, HBM-encoded tier
    from lmcache_amd.cache_engine import LMCacheEngine
    from lmcache_amd.config import LMCacheEngineConfig, LMCacheEngineMetadata
    eng = LMCacheEngine(LMCacheEngineConfig.from_legacy(chunk_size=CS, backend="cuda", local_serde="cachegen"),
                        LMCacheEngineMetadata(MODEL, 1, 0, "vllm", "half"))
    caches = caches_of("NBHD", slots)
    walls = {"store_paged": [], "layerwise_finish": []}
    for run in range(6):
        for kind in walls:
            tokens = torch.randint(0, 30000, (T,), generator=torch.Generator().manual_seed(100 + 2 * run + (kind == "store_paged"))).to(DEV)
            if kind == "store_paged":
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                eng.store_paged(tokens, caches, slots, BS, "NBHD")
            else:
                st = eng.store_paged_layerwise(tokens, caches, slots, BS, "NBHD")
                assert st.layerwise
                for l in range(L):
                    st.save_layer(l)
                torch.cuda.synchronize()  # the forward pass is over and every layer has been coded
                t0 = time.perf_counter()
                st.finish()
            torch.cuda.synchronize()
            walls[kind].append((time.perf_counter() - t0) * 1e3)
    out["engine_wall_ms_median_after_first"] = {k: statistics.median(v[1:]) for k, v in walls.items()}
    eng.close()
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(line + "\n")


if __name__ == "__main__":
    main()
