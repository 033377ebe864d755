// k_layers.h -- the last launch of a layer-wise store (lmc_encode_layers_*, include/lmc_hip.h).
//
// Stands where the reference's store path stands AFTER the forward pass: cache_engine.py:268-282 (store: every chunk is
// serialised once the whole KV tuple exists) behind the connector's per-layer gather of the paged cache
// (docs/source/developer_tutorial/LLM_Engine.rst:91-122).  Here layer l's two planes are quantised and entropy-coded the
// moment layer l has written its KV -- plane-subset launches of k_quantize and the counts-only k_cdf_encode
// (k_quantize.h: QuantArgs::plane0; k_encode.h: EncodeArgs::chain_gran) -- and what is left for the end of the step is
// this kernel: one pass at HBM speed over the V half of the blobs.
//
// Why the V half.  A stream's place in its blob is the sum of the allocations in front of it, in plane order
// p = kv * L + layer.  The K planes of layer l follow those of layer l - 1, so their streams are coded straight into the
// blob; a V stream's offset needs every K allocation of the chunk, which is known behind layer L - 1 only.  The layer
// launches code the V streams into a region of the job at V-relative offsets (a second placement chain rooted at plane L).
// Per chunk this kernel
//   reads K_total and V_total from the two chains' last granules (inclusive prefixes),
//   moves the V region to streams + K_total (16-byte non-temporal loads and stores: streamed once),
//   adds K_total to the V planes' directory entries,
//   writes what the chunk's last stream writes in a one-piece encode: header, static sections and pads
//   (write_blob_static), header word 23 for fp8 KV, and the size word -- which stays 0 until then.
// The blob is byte for byte the one lmc_encode_chunks / lmc_encode_chunks_split writes.
#pragma once
#include "k_encode.h"

struct LayersFinishArgs {
  EncodeArgs e;   // the job's geometry, blobs, sizes, status, bins, granules, V region (chain_gran != 0)
  u32 kv_dtype;   // header word 23: the KV's own dtype for fp8 KV, else 0 (lmc_format.h)
};

// grid = (pieces of the move, chunks), 256 threads
__global__ __launch_bounds__(256) void k_layers_finish(LayersFinishArgs f) {
  const EncodeArgs& a = f.e;
  const int chunk = (int)blockIdx.y;
  const int lane = threadIdx.x & 63;
  const int T = min(a.chunk_tokens, a.tok_end - (a.tok_begin + chunk * a.chunk_tokens));
  const BlobOff bo = lmc_blob_off((u32)a.P, (u32)T, (u32)a.G);
  const long long clen = (long long)a.L * a.chain_gran;  // granules of a chain
  unsigned long long* const agg = a.agg + (long long)chunk * 2 * clen;
  const unsigned long long kg = agg_load(agg + clen - 1), vg = agg_load(agg + 2 * clen - 1);
  const u32 K = (u32)kg, V = (u32)vg;  // bytes of the chunk's K and V streams: sums of allocations, multiples of 16
  u8* const blob = a.blobs + (long long)chunk * a.blob_stride;
  // A chain whose last granule is no inclusive prefix did not finish (a look-back timed out: the status word says so
  // already); totals past the blob's slot or the region cannot happen (the allocations are bounded by lmc_blob_bound).
  // Either way nothing is moved and the size word stays 0.
  const bool done = (kg >> 62) == AGG_P && (vg >> 62) == AGG_P;
  const bool fits = (unsigned long long)bo.streams + K + V <= (unsigned long long)a.blob_stride && (long long)V <= a.vstride;
  if (!done || !fits) {
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(a.status, done ? LMC_ST_STREAM_OVERFLOW : LMC_ST_LOOKBACK_TIMEOUT);
    return;
  }
  const LMC_GLOBAL u32x4_t* const src = reinterpret_cast<const LMC_GLOBAL u32x4_t*>((const LMC_GLOBAL u8*)(a.vregion + (long long)chunk * a.vstride));
  LMC_GLOBAL u32x4_t* const dst = reinterpret_cast<LMC_GLOBAL u32x4_t*>((LMC_GLOBAL u8*)(blob + bo.streams + K));
  const u32 n16 = V >> 4;
  for (u32 i = blockIdx.x * 256u + threadIdx.x; i < n16; i += gridDim.x * 256u)
    __builtin_nontemporal_store(__builtin_nontemporal_load(src + i), dst + i);
  if (blockIdx.x != 0) return;
  // the V planes' directory entries were written V-relative
  u32* const vdir = reinterpret_cast<u32*>(blob + bo.gdir) + 2 * a.L * a.G;
  for (u32 i = threadIdx.x; i < 2u * (u32)(a.L * a.G); i += 256u) vdir[i] += K;
  if (threadIdx.x >= 64) return;
  write_blob_static(blob, bo, a, (u32)T, K + V, lane);
  if (lane == 23 && f.kv_dtype) reinterpret_cast<u32*>(blob)[23] = f.kv_dtype;  // (the lane that wrote the word as 0)
  if (lane == 0) a.sizes[chunk] = bo.streams + K + V;
}
