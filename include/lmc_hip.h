/*
 * lmc_hip.h -- C ABI of liblmc_hip.so, the MI355X (gfx950) KV hot path.
 *
 * Drop-in boundary for LMCache's CacheGen serde + host-DRAM offload path.
 * Every entry point cites the reference interface it replaces (paths relative
 * to the reference tree).  Conventions:
 *   - plain C types only; pointers are DEVICE pointers unless suffixed _h
 *     (host) -- no torch types cross this boundary;
 *   - every call that touches the GPU takes the hipStream_t to run on
 *     (`lmc_stream_t`, NULL = default stream), is ASYNCHRONOUS and never calls
 *     hipDeviceSynchronize (the reference flags torch.cuda.synchronize() as
 *     harmful on this path, lmcache/storage_backend/local_backend.py:83-85);
 *   - return value: 0 = ok, negative = error (lmc_strerror); nothing throws;
 *   - re-entrant per context: calls on different streams may interleave; the
 *     context orders its internal workspace with events, not host syncs.
 *
 * Plane order everywhere: p = kv * L + layer (all K planes, then all V
 * planes) -- the order of the reference's encode_input / cdf tensors
 * (cachegen_encoder.py:284,290).
 */
#ifndef LMC_HIP_H
#define LMC_HIP_H

#include <stddef.h>
#include <stdint.h>

#include "lmc_format.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lmc_ctx lmc_ctx;
typedef void* lmc_stream_t; /* hipStream_t */
typedef void* lmc_event_t;  /* hipEvent_t  */

#define LMC_OK 0
#define LMC_ERR_INVALID (-1)     /* bad argument / unsupported geometry            */
#define LMC_ERR_HIP (-2)         /* a HIP runtime call failed (see lmc_last_hip_error) */
#define LMC_ERR_NOMEM (-3)
#define LMC_ERR_DEVICE_FLAG (-4) /* a kernel reported an error (lmc_device_status)  */

const char* lmc_strerror(int code);
/* hipError_t of the last failing HIP call made by this library on this thread. */
int lmc_last_hip_error(void);
/* ABI version of this header. */
int lmc_abi_version(void);
#define LMC_ABI_VERSION 6

/* ------------------------------------------------------------------ */
/* KV addressing                                                       */
/* ------------------------------------------------------------------ */
/*
 * Where the element (layer l, kv, token t, head h, dim d) of a KV cache
 * lives.  One descriptor covers every layout the reference's engine and the
 * (external) vLLM connector hand over:
 *   - chunk blob  [L,2,T,H,D]  "vllm" fmt          (cache_engine.py:137-138)
 *   - chunk blob  [L,2,H,T,D]  "huggingface" fmt   (cache_engine.py:139-140)
 *   - the KVCache tuple of per-layer (K,V) tensors passed to
 *     LMCacheEngine.store (cache_engine.py:230-236) -> plane_ptrs
 *   - vLLM paged blocks addressed through slot_mapping
 *     (docs/source/developer_tutorial/LLM_Engine.rst:91-122)
 *
 *   addr = plane_base(l,kv) + tok_off(t) + h*stride_head + d        [elements]
 *   plane_base = plane_ptrs ? plane_ptrs[2*l+kv] : base + l*stride_layer + kv*stride_kv
 *   tok_off(t) = slot_mapping ? (s / block_size)*stride_block + (s % block_size)*stride_token,
 *                               s = slot_mapping[t]
 *                             : t*stride_token
 * d is contiguous.  A plane has a multiple of 8 channels (num_heads * head_size % 8 == 0).  Layouts the ENCODERS read
 * (lmc_quantize, lmc_encode_chunks, lmc_store_*) are read with vectors of 8 channels -- 16 bytes for the 16-bit dtypes, 8 bytes
 * for fp8 -- : base aligned to one vector (16 B; fp8: 8 B),
 * stride_layer / stride_kv / stride_token / stride_block multiples of 8 elements, and either head_size % 8 == 0 with
 * stride_head % 8 == 0, or stride_head == head_size (the heads of a token row back to back -- the vllm chunk, the
 * per-layer [T,H,D] tensors, NBHD blocks -- where any head_size will do).  The DECODERS' destination and both sides of
 * lmc_copy_kv take any strides and any head_size (lmc_copy_kv copies element-wise when a side is not vector-readable:
 * the way to bring such a range into a chunk the encoders take; lmcache_amd's codec does that by itself).
 * "Any strides" of a DECODE destination ends where the decoder's 32-bit store offsets do.  With E = element bytes (2 or
 * 1), row = ((H-1)*stride_head + D)*E (a token row, first channel to last) and row_step = stride_token*E:
 *   stride_head >= 0 and stride_token >= 0;
 *   without a slot_mapping   (chunk_tokens-1)*row_step + row <= 0xfffffff0   (the rows of one chunk, the last one's last
 *                            channel included, lie within the store's range of the chunk's first row);
 *   with a slot_mapping      row <= 0xfffffff0, and 7*row_step + row <= 0xfffffff0 while row_step < 2^28.
 * Every decode and load entry point returns LMC_ERR_INVALID beyond that, before anything is queued.  (Planes, blocks and
 * chunks may lie any distance apart: those offsets are 64-bit.)
 *
 * paged_kind = LMC_PAGED_ROWS (0) is all of the above: a token's head is a row of D contiguous elements.
 * paged_kind = LMC_PAGED_SPLIT (1) is the cache of vLLM's ROCm paged-attention kernels (paged_attention_rocm,
 * paged_attention_v1 / v2; PagedAttention.split_kv_cache): key_cache [num_blocks, H, D/x, block_size, x] with
 * x = 16 / element bytes (8 for bf16 / fp16, 16 for fp8), value_cache [num_blocks, H, D, block_size].  slot_mapping and
 * block_size are required, head_size % x == 0, stride_token is ignored; the plane bases are found as above, K planes
 * (kv = 0) are x-split, V planes token-innermost.  With s = slot_mapping[t], b = s / block_size, w = s % block_size:
 *   K addr = plane_base(l,0) + b*stride_block + h*stride_head + (d / x)*(block_size*x) + w*x + d % x      [elements]
 *   V addr = plane_base(l,1) + b*stride_block + h*stride_head + d*block_size + w
 * (a dense cache: stride_head = D*block_size, stride_block = H*D*block_size).  A token's channels are not contiguous
 * there.  Who takes such a layout:
 *   - lmc_copy_kv, as its source or as its destination (not both; the other side is any LMC_PAGED_ROWS layout):
 *     k_copy_split.h; the scatter_dst of an lmc_range_post, as a destination;
 *   - as a DECODE DESTINATION, the four entry points behind a serving engine's retrieve: lmc_decode_chunks_layers,
 *     lmc_decode_chunks_schedule, lmc_load_chunks and lmc_load_pack (k_decode.h stores into the split blocks: a lane's
 *     head / granule / element is its 32-bit offset, a token its block, 64-bit, plus its slot's step).  Its 32-bit
 *     offsets end at   stride_head >= 0  and  ((H-1)*stride_head + D*block_size)*E + 7*16 <= 0xfffffff0;
 *     beyond that LMC_ERR_INVALID before anything is queued (blocks and planes may lie any distance apart).
 *     For LMC_MODEL_FIXED blobs, lmc_decode_chunks_fixed_split_schedule (16-bit elements; k_fixed.h: a K token's granule
 *     by one 16-byte store, a V oct that is eight consecutive slots of a block from slot % 8 == 0 on by one 16-byte store
 *     per channel, anything else element by element), under the same rule for the 32-bit offsets.
 *   - NOT lmc_decode_chunks: it is the replacement of the reference's from_bytes, whose caller wants a tensor of rows.
 *   - as an ENCODE SOURCE, lmc_encode_chunks_split and the stores (lmc_store_chunks, lmc_store_pack,
 *     lmc_store_pack_parts): k_quantize.h reads the split blocks in place (a V oct whose tokens are eight consecutive
 *     slots of a block, from slot % 8 == 0 on, as 16-byte runs of one channel; a K token's granules where they lie;
 *     anything else element by element), then k_cdf_encode -- never the fused kernel, so a pack store is one part.
 *     Planes of at most 1024 channels (H * D), stride_head >= 0 and ((H-1)*stride_head + D*block_size)*E <= 0xfffffff0;
 *     beyond that LMC_ERR_INVALID before anything is queued.  lmc_encode_chunks_fixed_split reads it the same way
 *     (k_fixed.h, one kernel) under the same limits, for 16-bit elements.
 *   - NOT lmc_encode_chunks and lmc_quantize: they stand for the reference's to_bytes / torch_quant_vectorized, whose
 *     caller holds a tensor of rows.  NOT lmc_encode_chunks_fixed and lmc_decode_chunks_fixed_schedule either: their
 *     _split twins are the ones that take it.
 *   - lmc_rope_shift_split (16-bit elements): the keys re-rotated in the split blocks themselves, under the decoders'
 *     rule for the 32-bit offsets; NOT lmc_rope_shift, which rotates rows.
 * Every other entry point -- lmc_rope_shift among them -- reads and writes rows and returns LMC_ERR_INVALID for it: bring
 * the range into a chunk with lmc_copy_kv first, as for any layout the encoders cannot read.  Any other paged_kind is
 * LMC_ERR_INVALID; a caller that zeroes the struct gets LMC_PAGED_ROWS.
 */
#define LMC_PAGED_ROWS 0
#define LMC_PAGED_SPLIT 1
typedef struct lmc_kv_layout {
  int32_t dtype;      /* LMC_DTYPE_BF16 / FP16 / FP8_E4M3 / FP8_E5M2 (elements of 2 or 1 bytes; strides count elements) */
  int32_t num_layers; /* L */
  int32_t num_heads;  /* H (KV heads held by this rank) */
  int32_t head_size;  /* D */
  const void* base;
  const void* const* plane_ptrs; /* device array [2L] of device pointers, or NULL */
  int64_t stride_layer;
  int64_t stride_kv;
  int64_t stride_token;
  int64_t stride_head;
  const int64_t* slot_mapping; /* device [ntokens] or NULL */
  int32_t block_size;
  int32_t paged_kind; /* LMC_PAGED_ROWS / LMC_PAGED_SPLIT (this word was padding, zero, before) */
  int64_t stride_block;
} lmc_kv_layout;

/* ------------------------------------------------------------------ */
/* context                                                             */
/* ------------------------------------------------------------------ */
/* Replaces the per-serializer device state of CacheGenSerializer /
 * CacheGenDeserializer.__init__ (cachegen_encoder.py:330-350,
 * cachegen_decoder.py:110-140: bins tensors, reusable output buffer). */
int lmc_ctx_create(int device, lmc_ctx** out);
int lmc_ctx_destroy(lmc_ctx* ctx);
/* Pre-size the encode workspace (symbols + padded stream scratch) for up to
 * max_chunks chunks of chunk_tokens tokens.  Optional: lmc_encode_chunks grows
 * it on demand (growth allocates, i.e. may stall that one call). */
int lmc_ctx_reserve(lmc_ctx* ctx, int L, int H, int D, int chunk_tokens, int max_chunks);
/* Status bits a kernel can raise (0 = ok).  A call that is given a `job_status` word reports into THAT
 * word (device-accessible uint32, e.g. pinned host memory, zeroed by the caller; valid once the call's
 * work has completed: after an event / stream sync by the caller), so that concurrent jobs never see each
 * other's failures; with job_status == NULL the bits go to the context's sticky word below. */
#define LMC_STATUS_STREAM_OVERFLOW 1u /* encode: a group stream outgrew its scratch slot (cannot happen) */
#define LMC_STATUS_BAD_HEADER 2u      /* decode: header / geometry / section offsets inconsistent */
#define LMC_STATUS_BAD_STREAM 4u      /* decode: directory out of bounds, words left over, final state wrong */
#define LMC_STATUS_LOOKBACK_TIMEOUT 8u
#define LMC_STATUS_BAD_SCALES 16u     /* decode: a plane's scales do not match their checksum (lmc_format.h: scsum) */
#define LMC_STATUS_HOST_ARENA_FULL 32u /* lmc_store_chunks: the pinned arena cannot take the job's blobs */
#define LMC_STATUS_BAD_POSITION 64u  /* rope shift: a token's |delta| is outside the table; that token is left as it was */
/* A decode that raises any bit leaves the destination rows of the blobs concerned UNDEFINED (some of a plane's
 * waves may have stored before another wave saw the damage: BAD_SCALES is found by the plane's first wave only,
 * BAD_STREAM at the end of a stream).  A caller that decodes into live storage -- the paged entry points -- must
 * treat those tokens as not retrieved; lmcache_amd's engine turns every non-zero status into a miss. */
/* The context's sticky status word.  `clear` resets it. */
int lmc_device_status(lmc_ctx* ctx, int clear);

/* Geometry limits of this build: 2L <= LMC_MAX_PLANES planes, C = H*D <= LMC_MAX_CHANNELS channels per
 * plane (4096 = a 32-head x 128 MHA model; every BASELINE.json config fits), C a multiple of 8,
 * chunks of 1 .. 65535 tokens.  Outside them the entry points return LMC_ERR_INVALID. */
#define LMC_MAX_PLANES 256
#define LMC_MAX_CHANNELS 4096
#define LMC_FUSED_MAX_CHANNELS 1024 /* widest plane the fused encode kernel takes (k_fused.h) */

/* Which kernels lmc_encode_chunks launches.  The fused kernel (one workgroup quantises, codes and places a
 * run of whole planes of a chunk: k_fused.h) covers the 256-token chunks of planes of up to
 * LMC_FUSED_MAX_CHANNELS channels; wider planes, other chunk lengths and a ragged last chunk take
 * k_quantize + k_cdf_encode whatever the setting.
 *   AUTO (default)  fused when the job has more (chunk, plane) pairs than the chip has workgroup slots
 *                   (4 per CU), where it is the faster of the two;
 *   TWO_KERNELS     never fused;     FUSED  fused for any job size.
 * The blobs are byte-identical either way; the switch exists for A/B timing and for the parity tests. */
#define LMC_ENCODE_PATH_AUTO 0
#define LMC_ENCODE_PATH_TWO_KERNELS 1
#define LMC_ENCODE_PATH_FUSED 2
int lmc_ctx_set_encode_path(lmc_ctx* ctx, int path);

/* Into how many slices a layer's launch of a fixed-width layer-wise job (lmc_encode_layers_begin_fixed, which reads
 * this) cuts each plane of a chunk; additive in ABI 6.  A slice is a run of whole passes of k_fixed_encode's eight
 * waves over the plane's row octs (8, 16 or 32 octs a pass for planes of more than 256, more than 128, at most 128
 * channels), so n is clipped to the passes of a whole chunk's plane.
 *   n >= 1  that many;    0 (default)  the smallest power of two that gives a layer's launch (2 planes x nchunks x
 *                                      slices workgroups) a workgroup per CU, else as many as there are passes.
 * The blobs do not depend on it; the switch exists for A/B timing and for the tests.  n < 0: LMC_ERR_INVALID. */
int lmc_ctx_set_fixed_layer_slices(lmc_ctx* ctx, int n);

/* Per-kernel timing of the NEXT lmc_encode_chunks / lmc_decode_chunks calls:
 * when enabled the call brackets each of its kernels with hipEvents on the
 * caller's stream.  lmc_ctx_profile_read (after the caller has synchronised
 * that stream) returns the durations in ms of the last profiled call, in
 * launch order (encode: k_encode_fused, or k_quantize, k_cdf_encode [which also compacts the streams
 * into the blob]; decode: k_decode; lmc_encode_chunks_fixed: k_fixed_encode; lmc_decode_chunks_fixed_schedule:
 * k_fixed_decode of the last range) and the number of entries written (<= cap). */
int lmc_ctx_profile(lmc_ctx* ctx, int enable);
int lmc_ctx_profile_read(lmc_ctx* ctx, float* ms_out, int cap);

/* ------------------------------------------------------------------ */
/* encode side                                                         */
/* ------------------------------------------------------------------ */
/*
 * Quantise tokens [tok_begin, tok_begin+ntok) of `src`.
 * Replaces torch_quant_vectorized applied to K and V + the torch.cat that
 * builds encode_input (cachegen_encoder.py:40-61, 278-285).
 *   bins_h   host int32 [2L], plane order (key_bins ++ value_bins,
 *            cachegen_encoder.py:339-350)
 *   sym_out  int8  [2L][ntok][C]   (= encode_input)
 *   scale_out u16  [2L][ntok]      raw bits of src dtype (= max_tensors_key ++ max_tensors_value); fp8 src: of the
 *                                  bf16 image of the max
 */
int lmc_quantize(lmc_ctx* ctx, const lmc_kv_layout* src, int32_t tok_begin, int32_t ntok,
                 const int32_t* bins_h, int8_t* sym_out, uint16_t* scale_out, lmc_stream_t stream);

/*
 * Replaces torchac_cuda.calculate_cdf(sym, max_bins) (call sites
 * cachegen_encoder.py:287-289): per-(plane,channel) histogram over tokens ->
 * 16-bit strictly increasing CDF.
 *   sym int8 [P][T][C], cdf_out u16 [P][C][max_bins+1]; max_bins must be 32.
 */
int lmc_calculate_cdf(lmc_ctx* ctx, const int8_t* sym, int32_t P, int32_t T, int32_t C, int32_t max_bins,
                      uint16_t* cdf_out, lmc_stream_t stream);

/*
 * Fused encode of consecutive token chunks: quantise + CDF + entropy-encode +
 * compaction + container, one blob per chunk.  Replaces, per chunk,
 * LMCacheEngine._slice_kv_at (cache_engine.py:131-161) +
 * CacheGenSerializer.to_bytes -> encode_function -> encode_ntokens/
 * torchac_cuda.encode_fast_new -> collect_bytes -> CacheGenGPUEncoderOutput
 * (cachegen_encoder.py:225-325, 352-389), minus the pickle/D2H which is
 * lmc_memcpy_async's job.
 *   chunk i covers tokens [tok_begin + i*chunk_tokens, min(+chunk_tokens, tok_end))
 *   blobs    device arena; blob i is written at blobs + i*blob_stride;
 *            blob_stride >= lmc_blob_bound(L, chunk_tokens, H, D), multiple of 16
 *   sizes    device-accessible uint32 [nchunks] (device or pinned host memory):
 *            receives total_bytes of each blob
 *   job_status  see LMC_STATUS_* above (may be NULL)
 */
int lmc_encode_chunks(lmc_ctx* ctx, const lmc_kv_layout* src, int32_t tok_begin, int32_t tok_end,
                      int32_t chunk_tokens, const int32_t* bins_h, void* blobs, uint64_t blob_stride,
                      uint32_t* sizes, uint32_t* job_status, lmc_stream_t stream);

/*
 * lmc_encode_chunks for any source lmc_encode_chunks takes AND an LMC_PAGED_SPLIT one (see lmc_kv_layout): the cache of
 * vLLM's ROCm paged-attention kernels is read in place, no staged chunk and no lmc_copy_kv in front.  The blobs are
 * byte for byte those lmc_encode_chunks writes from the gathered chunk.  A split source always takes k_quantize +
 * k_cdf_encode, whatever lmc_ctx_set_encode_path says; with more than 1024 channels per plane it is LMC_ERR_INVALID and
 * nothing is launched.  Any other source: exactly lmc_encode_chunks.
 */
int lmc_encode_chunks_split(lmc_ctx* ctx, const lmc_kv_layout* src, int32_t tok_begin, int32_t tok_end,
                            int32_t chunk_tokens, const int32_t* bins_h, void* blobs, uint64_t blob_stride,
                            uint32_t* sizes, uint32_t* job_status, lmc_stream_t stream);

/*
 * lmc_encode_chunks with the blobs written in the FIXED-WIDTH model (lmc_format.h: LMC_MODEL_FIXED; additive in ABI 6;
 * csrc/k_fixed.h): the same quantisation, scales and checksums, every symbol at 4 or 5 bits and no entropy coder -- for
 * blobs that stay in HBM, where the coder's bytes buy nothing.  One launch, one pass over the source.  Arguments and
 * refusals are lmc_encode_chunks' (an LMC_PAGED_SPLIT source is LMC_ERR_INVALID here: lmc_encode_chunks_fixed_split
 * takes it), and so is blob_stride >= lmc_blob_bound: a fixed-width blob never outgrows the coded models' slot.  fp8 KV
 * is LMC_ERR_INVALID.  sizes[i] receives lmc_fixed_blob_bytes of chunk i, a function of the geometry and the bins alone.
 */
int lmc_encode_chunks_fixed(lmc_ctx* ctx, const lmc_kv_layout* src, int32_t tok_begin, int32_t tok_end,
                            int32_t chunk_tokens, const int32_t* bins_h, void* blobs, uint64_t blob_stride,
                            uint32_t* sizes, uint32_t* job_status, lmc_stream_t stream);

/*
 * lmc_encode_chunks_fixed for any source it takes AND a 16-bit LMC_PAGED_SPLIT one (additive in ABI 6; what
 * lmc_encode_chunks_split is to lmc_encode_chunks): the cache is read in place by k_fixed_encode's split instances, no
 * staged chunk and no lmc_copy_kv in front, and the blobs are byte for byte those lmc_encode_chunks_fixed writes from the
 * gathered chunk.  Only slots of the job's own tokens are read.  A split source with more than 1024 channels per plane,
 * stride_head < 0 or ((H-1)*stride_head + D*block_size)*E > 0xfffffff0, or fp8 elements, is LMC_ERR_INVALID and nothing
 * is launched.  Any other source: exactly lmc_encode_chunks_fixed.
 */
int lmc_encode_chunks_fixed_split(lmc_ctx* ctx, const lmc_kv_layout* src, int32_t tok_begin, int32_t tok_end,
                                  int32_t chunk_tokens, const int32_t* bins_h, void* blobs, uint64_t blob_stride,
                                  uint32_t* sizes, uint32_t* job_status, lmc_stream_t stream);

/*
 * The same encode issued LAYER BY LAYER (additive in ABI 6; csrc/k_layers.h).  Replaces the store of the reference, which
 * serialises every chunk after the whole forward pass (cache_engine.py:268-282), and the per-layer gather of the paged
 * cache that a connector runs in front of it (docs/source/developer_tutorial/LLM_Engine.rst:91-122): layer l's planes
 * l and L + l are quantised and entropy-coded the moment layer l has written its KV, and one pass at HBM speed finishes
 * the blobs.  After lmc_encode_layers_finish every blob and size word is byte for byte what lmc_encode_chunks (or, for an
 * LMC_PAGED_SPLIT source, lmc_encode_chunks_split) writes for the same source, token range, chunk length and bins; a size
 * word stays 0 until then.
 *   lmc_encode_layers_begin   arguments and refusals of lmc_encode_chunks_split; `src` is the full layout, every layer's
 *                             planes (only their contents arrive layer by layer) and must stay valid, with whatever it
 *                             points to, until finish or abort.  Queues nothing.  Returns LMC_OK and the job, or
 *                             LMC_NOT_LAYERWISE (positive, no job): the arguments are fine but the job is not eligible --
 *                             eligible are jobs whose every chunk, a ragged last one included, has 2 .. 256 tokens and
 *                             whose planes have at most 1024 channels; the caller encodes in one piece instead.
 *                             The job owns its look-back granules, ticket counter, two-plane symbol workspace and V
 *                             region: it takes neither of the context's encode workspaces nor its store arena, so a job
 *                             that spans a forward pass makes no other store wait.
 *   lmc_encode_layer          quantise and code layer `layer` on `stream`.  Layers come in ascending order from 0; a
 *                             repeated, skipped or out-of-range layer is LMC_ERR_INVALID with nothing queued.  The
 *                             calls of one job are ordered by the caller: one stream, or events between them.
 *   lmc_encode_layers_finish  k_layers_finish on `stream` behind layer L - 1 (LMC_ERR_INVALID before that, nothing
 *                             queued); the job handle is gone afterwards, its buffers are reused behind the launch.
 *   lmc_encode_layers_abort   gives the job up at any point: its buffers are reused behind what it has queued.
 */
#define LMC_NOT_LAYERWISE 1
typedef struct lmc_layer_job lmc_layer_job;
int lmc_encode_layers_begin(lmc_ctx* ctx, const lmc_kv_layout* src, int32_t tok_begin, int32_t tok_end,
                            int32_t chunk_tokens, const int32_t* bins_h, void* blobs, uint64_t blob_stride,
                            uint32_t* sizes, uint32_t* job_status, lmc_layer_job** job_out);
/*
 * The layer-wise form of lmc_encode_chunks_fixed_split (additive in ABI 6; csrc/k_fixed.h): the same lmc_layer_job, tagged
 * with its model -- lmc_encode_layer, lmc_encode_layers_finish and lmc_encode_layers_abort take it as they take the coded
 * job, with the same ordering rules and the same LMC_ERR_INVALID for a repeated, skipped or out-of-range layer or an early
 * finish, nothing queued.  Arguments and refusals are lmc_encode_chunks_fixed_split's (fp8 KV and blob_stride <
 * lmc_blob_bound are LMC_ERR_INVALID); LMC_NOT_LAYERWISE only for planes of more than 1024 channels: every chunk length
 * of the one-piece call is eligible, a ragged last chunk of one token included.
 * A fixed-width stream's place is a function of (bins, T) alone, so there is no placement chain, no V region and no
 * move at the end: lmc_encode_layer is ONE launch of k_fixed_encode over planes `layer` and L + `layer`, each plane of a
 * chunk cut into slices (lmc_ctx_set_fixed_layer_slices) so that a launch of few chunks still fills the chip; the
 * workgroups store streams and scales where they belong and their partial check sums into the job's own workspace
 * ([nchunks][2L][slices][G + 1] dwords, plain stores, nothing zeroed in front).  lmc_encode_layers_finish is
 * k_fixed_layers_finish: it sums the partials and writes each stream's 16-byte tail and directory entry, the planes'
 * scale checksums, header, bins, pads and the size word.  sizes[i] is written 0 by layer 0's launch and
 * lmc_fixed_blob_bytes by the finish; afterwards bytes [0, sizes[i]) of every blob are byte for byte what
 * lmc_encode_chunks_fixed / _fixed_split writes and nothing beyond them is touched.  The job takes neither of the
 * context's encode workspaces.
 */
int lmc_encode_layers_begin_fixed(lmc_ctx* ctx, const lmc_kv_layout* src, int32_t tok_begin, int32_t tok_end,
                                  int32_t chunk_tokens, const int32_t* bins_h, void* blobs, uint64_t blob_stride,
                                  uint32_t* sizes, uint32_t* job_status, lmc_layer_job** job_out);
int lmc_encode_layer(lmc_ctx* ctx, lmc_layer_job* job, int32_t layer, lmc_stream_t stream);
int lmc_encode_layers_finish(lmc_ctx* ctx, lmc_layer_job* job, lmc_stream_t stream);
int lmc_encode_layers_abort(lmc_ctx* ctx, lmc_layer_job* job);

/* ------------------------------------------------------------------ */
/* decode side                                                         */
/* ------------------------------------------------------------------ */
/*
 * Fused decode of nchunks blobs straight into the destination layout:
 * entropy-decode + dequantise + cast + scatter.  Replaces, per chunk,
 * CacheGenDeserializer.from_bytes -> decode_function_gpu -> decode_chunk /
 * torchac_cuda.decode_fast_prefsum -> do_dequantize -> stack/reshape/permute/
 * .to(16-bit) (cachegen_decoder.py:24-35, 51-106, 142-202) and the engine's
 * torch.cat over chunks (cache_engine.py:362-368).
 *   blob i is read from blobs + i*blob_stride (device memory)
 *   token t of chunk i is written to dst token  dst_tok0 + i*chunk_tokens + t;
 *   tokens that land below 0 are dropped (the "drop extra tokens in the first
 *   chunk" rule of retrieve(), cache_engine.py:360-365: pass dst_tok0 = -skip)
 *   dst->dtype selects the output type (bf16 for "vllm", fp16 for
 *   "huggingface": cachegen_decoder.py:190-200)
 * dst is a LMC_PAGED_ROWS layout.  This call alone among the decode entry points returns LMC_ERR_INVALID for an
 * LMC_PAGED_SPLIT destination: it stands for from_bytes, which returns a tensor; a paged-attention cache is filled through
 * lmc_decode_chunks_layers / _schedule, lmc_load_chunks or lmc_load_pack (see lmc_kv_layout).
 */
int lmc_decode_chunks(lmc_ctx* ctx, const void* blobs, uint64_t blob_stride, int32_t nchunks,
                      const lmc_kv_layout* dst, int32_t dst_tok0, int32_t chunk_tokens, uint32_t* job_status,
                      lmc_stream_t stream);

/*
 * The same decode for a RANGE OF LAYERS of blobs that lie anywhere in device memory: the launch handles the K and V
 * planes of layers [layer_begin, layer_begin + layer_count) of every chunk.  A retrieve cut into one launch per
 * layer range (an event after each) hands layer 0's KV to the model after 1/L of the decode instead of all of it
 * -- the streams of a plane are independent and the blob's stream directory ({beg, end} per stream) gives random access to them.  Stands
 * where the reference decodes and concatenates the whole context before the first layer can run
 * (cache_engine.py:339-381; the connector writes layer by layer afterwards, LLM_Engine.rst:101-122).
 *   blob_ptrs       device array [nchunks] of device pointers, blob i at blob_ptrs[i] (16-byte aligned)
 *   max_blob_bytes  upper bound of the blobs' sizes (a blob whose header claims more is rejected)
 */
int lmc_decode_chunks_layers(lmc_ctx* ctx, const void* const* blob_ptrs, uint64_t max_blob_bytes, int32_t nchunks,
                             const lmc_kv_layout* dst, int32_t dst_tok0, int32_t chunk_tokens, int32_t layer_begin,
                             int32_t layer_count, uint32_t* job_status, lmc_stream_t stream);

/*
 * ... and a whole SCHEDULE of such launches in one call (round 6): range i covers layers
 * [layer_ends[i - 1], layer_ends[i]) (layer_ends[-1] = 0, ascending, the last entry = num_layers), each launch is
 * followed by hipEventRecord(events[i]) on `stream`.  What engine.retrieve_layerwise() issued as one C call and one
 * event per range from Python (0.26 ms of host time in front of the first kernel of a warm 16 k prefix) -- the host
 * side of cache_engine.py:293-381 for the HBM-resident tier.  events may be NULL (no events), or hold NULL entries.
 */
int lmc_decode_chunks_schedule(lmc_ctx* ctx, const void* const* blob_ptrs, uint64_t max_blob_bytes, int32_t nchunks,
                               const lmc_kv_layout* dst, int32_t dst_tok0, int32_t chunk_tokens, int32_t nranges,
                               const int32_t* layer_ends_h, const lmc_event_t* events_h, uint32_t* job_status,
                               lmc_stream_t stream);

/*
 * What is done to each layer range of a decode job AFTER its decode launch and BEFORE its event (lmc_decode_chunks_schedule_post,
 * lmc_load_pack_post): the event of a range then says "decoded, re-rotated and in its final place".  Stands where
 * engine.retrieve_into_paged() queues one lmc_rope_shift and, for a staged "NHDB" retrieve, one lmc_copy_kv over ALL
 * layers behind the whole decode, so that the model waits for the last layer: here the same work is cut by the job's
 * ranges and the attention of layer l waits for its own range only (a vLLM v1 connector's wait_for_layer_load(l)).
 *   `dst` below is the job's decode destination; the post-op works on the layer window [l0, l0 + nl) of the layouts
 *   cos_sin .. deltas  a rotation as lmc_rope_shift takes it (cos_sin NULL: none); deltas[i] belongs to token tok_begin + i
 *   tok_begin, ntok    the tokens of `dst` this job filled (the caller knows: dst_tok0, the chunks, the first-chunk trim)
 *   scatter_dst        NULL, or an LMC_PAGED_SPLIT cache: `dst` is a staged chunk of rows, and token tok_begin + i of the
 *                      range's layers is scattered to token scatter_tok0 + i of scatter_dst (lmc_copy_kv's scatter)
 * Per range:  rotation -- lmc_rope_shift's kernels in place on the window of `dst` (rows);  scatter -- lmc_copy_kv's
 * scatter of the window;  both -- the rotation of the staged window, then its scatter, two launches (a scatter that
 * rotates the keys on their way was built and measured: slower than the two, profiles/paged_layerwise.md).  Neither: nothing.
 * ONE more form, every condition required: `dst` is LMC_PAGED_SPLIT, cos_sin is set, scatter_dst describes the SAME cache
 * as `dst` (every field of the two structs equal) and scatter_tok0 == tok_begin.  It says that the range's final place is
 * where the decoder put it and the rotation is done there: per range ONE lmc_rope_shift_split launch on the range's layer
 * window of `dst`, between its decode and its event; nothing is copied.  It is held against lmc_rope_shift_split's rules.
 * (Both sides split was refused before this form existed, so no valid call changed its meaning; a rotation of a split
 * `dst` with scatter_dst NULL, or with a scatter_dst that differs from `dst` in any field, or with
 * scatter_tok0 != tok_begin, stays LMC_ERR_INVALID.)
 * The whole post-op is held against lmc_rope_shift's and lmc_copy_kv's rules before anything of the job is queued
 * (LMC_ERR_INVALID): a rotation of an LMC_PAGED_SPLIT `dst`, of fp8, a scatter_dst that is not LMC_PAGED_SPLIT or differs
 * from `dst` in geometry or dtype, ntok < 1, ...  A per-token |delta| outside the table is reported as lmc_rope_shift
 * reports it with job_status NULL: LMC_STATUS_BAD_POSITION in the context's sticky word, that token copied unrotated (the
 * job's own word stays the verdict on its blobs).
 * The struct and everything it points to on the host is read during the call only.
 */
typedef struct lmc_range_post {
  const float* cos_sin; int32_t table_rows, rot_dim, is_neox, delta; const int32_t* deltas;
  int32_t tok_begin, ntok;
  const lmc_kv_layout* scatter_dst;
  int32_t scatter_tok0;
} lmc_range_post;
/* lmc_decode_chunks_schedule with `post` done to every range between its launch and its event; post NULL IS
 * lmc_decode_chunks_schedule (one body).  A split `dst` takes the in-place rotation form of lmc_range_post (`dst` named
 * as its own scatter_dst): decoded into the split blocks, then lmc_rope_shift_split per range. */
int lmc_decode_chunks_schedule_post(lmc_ctx* ctx, const void* const* blob_ptrs, uint64_t max_blob_bytes, int32_t nchunks,
                                    const lmc_kv_layout* dst, int32_t dst_tok0, int32_t chunk_tokens, int32_t nranges,
                                    const int32_t* layer_ends_h, const lmc_event_t* events_h, uint32_t* job_status,
                                    lmc_stream_t stream, const lmc_range_post* post);

/*
 * lmc_decode_chunks_schedule_post for LMC_MODEL_FIXED blobs (k_fixed_decode; one body with it, only the launch differs).
 * post NULL is the plain schedule; one range that ends at num_layers is the one-piece decode.  Every byte a section's
 * address depends on is checked before the section is read, and nothing is read past max_blob_bytes: magic, version,
 * geometry against `dst`, model == LMC_MODEL_FIXED, the totals and the directory entry of every stream decoded against
 * the layout the bins give (LMC_STATUS_BAD_HEADER -- a coded blob handed to this call is one, as a fixed-width blob is to
 * the coded models' decoders).  A stream whose check word does not match is LMC_STATUS_BAD_STREAM, scales that do not
 * match scsum LMC_STATUS_BAD_SCALES; the destination is undefined then, as for the coded models.
 * `dst` is 16-bit rows (LMC_PAGED_ROWS, with or without a slot mapping): an LMC_PAGED_SPLIT or fp8 destination is
 * LMC_ERR_INVALID with nothing queued -- here an "NHDB" cache is filled through a staged chunk and post->scatter_dst;
 * lmc_decode_chunks_fixed_split_schedule decodes straight into it.
 */
int lmc_decode_chunks_fixed_schedule(lmc_ctx* ctx, const void* const* blob_ptrs, uint64_t max_blob_bytes, int32_t nchunks,
                                     const lmc_kv_layout* dst, int32_t dst_tok0, int32_t chunk_tokens, int32_t nranges,
                                     const int32_t* layer_ends_h, const lmc_event_t* events_h, const lmc_range_post* post,
                                     uint32_t* job_status, lmc_stream_t stream);

/*
 * lmc_decode_chunks_fixed_schedule for any destination it takes (one body: exactly that call) AND a 16-bit
 * LMC_PAGED_SPLIT one (additive in ABI 6): k_fixed_decode's split instances store into the cache of vLLM's ROCm
 * paged-attention kernels, per range and with the ranges' events as there, no staged chunk and no scatter behind.  The
 * validation is the same and comes before every read; only slots of the call's own tokens are written (a token in front
 * of dst_tok0 + ... = 0 or past the blob's count is neither written nor looked up in slot_mapping).  The decoded bits
 * are those the row decode leaves in a chunk.  The split destination's 32-bit offsets follow the rule stated at
 * lmc_kv_layout for the coded decoders (LMC_ERR_INVALID beyond it, as for fp8), and `post` follows
 * lmc_decode_chunks_schedule_post: a rotation of a split `dst` is LMC_ERR_INVALID unless the post names `dst` as its
 * own scatter_dst (the in-place form of lmc_range_post: lmc_rope_shift_split per range, in front of the range's event).
 */
int lmc_decode_chunks_fixed_split_schedule(lmc_ctx* ctx, const void* const* blob_ptrs, uint64_t max_blob_bytes,
                                           int32_t nchunks, const lmc_kv_layout* dst, int32_t dst_tok0, int32_t chunk_tokens,
                                           int32_t nranges, const int32_t* layer_ends_h, const lmc_event_t* events_h,
                                           const lmc_range_post* post, uint32_t* job_status, lmc_stream_t stream);

/*
 * A WINDOW OF HEADS out of every blob (additive in ABI 6): KV stored under one tensor-parallel degree, retrieved under
 * another.  The blobs have src_heads heads; heads [src_head_begin, src_head_begin + nheads) of every blob are written to
 * heads [dst_head_begin, dst_head_begin + nheads) of `dst`, whose num_heads is ITS OWN (a TP = 8 rank takes one eighth of
 * a TP = 1 blob; a TP = 2 rank fills its destination from four TP = 8 blob sets with four calls).  The streams of a plane
 * are independent per 64-channel group and the directory gives random access to them (lmc_format.h), so a launch reads
 * only the streams of the groups the window touches -- the random access lmc_decode_chunks_layers uses along the layers,
 * along the heads.  A channel that shares a group with the window but lies outside it is decoded and not stored.
 *   dst->num_heads   the destination's head count;  dst->head_size must be the blobs' D (header word 6)
 *   win              required.  LMC_ERR_INVALID, nothing queued: win NULL, src_heads < 1, nheads < 1, a window outside
 *                    [0, src_heads) or outside [0, dst->num_heads), src_heads * D not a multiple of 8 or above
 *                    LMC_MAX_CHANNELS, and whatever the twin refuses for `dst`
 * Everything else is the twin's -- lmc_decode_chunks_schedule for the coded models (rows, paged rows, LMC_PAGED_SPLIT;
 * 16-bit and fp8 elements), lmc_decode_chunks_fixed_split_schedule for LMC_MODEL_FIXED blobs (16-bit rows, paged rows,
 * LMC_PAGED_SPLIT): blobs behind a pointer table, layer ranges with their events, the validation in front of every read.
 * The decoders' 32-bit offset rule (lmc_kv_layout) is held against dst's own num_heads.  A blob whose header does not say
 * num_heads == src_heads and head_size == dst->head_size is LMC_STATUS_BAD_HEADER; the scales of a plane are checked by
 * the first group the window touches (LMC_STATUS_BAD_SCALES), the streams that are read by their own waves
 * (LMC_STATUS_BAD_STREAM) -- damage in a stream outside the window's groups is not seen, it is not read.
 * Only bytes of heads [dst_head_begin, dst_head_begin + nheads) of the call's own tokens are written.
 * There is no `post`: a rotation or a scatter acts on all heads of `dst`, and a destination is typically filled by several
 * window calls -- the caller queues lmc_rope_shift / lmc_copy_kv once, behind the last of them.
 * A window that is the whole blob (src_heads == dst->num_heads, begins 0) launches exactly what the twin launches.
 */
typedef struct lmc_head_window {
  int32_t src_heads;       /* H of the blobs (their header's num_heads)            */
  int32_t src_head_begin;  /* first head taken out of every blob                    */
  int32_t nheads;          /* heads taken                                           */
  int32_t dst_head_begin;  /* head of dst that src_head_begin lands on              */
} lmc_head_window;
int lmc_decode_chunks_heads_schedule(lmc_ctx* ctx, const void* const* blob_ptrs, uint64_t max_blob_bytes, int32_t nchunks,
                                     const lmc_kv_layout* dst, int32_t dst_tok0, int32_t chunk_tokens, int32_t nranges,
                                     const int32_t* layer_ends_h, const lmc_event_t* events_h, const lmc_head_window* win,
                                     uint32_t* job_status, lmc_stream_t stream);
/* ... the same for LMC_MODEL_FIXED blobs (k_fixed_decode; one body with the call above). */
int lmc_decode_chunks_fixed_heads_schedule(lmc_ctx* ctx, const void* const* blob_ptrs, uint64_t max_blob_bytes,
                                           int32_t nchunks, const lmc_kv_layout* dst, int32_t dst_tok0, int32_t chunk_tokens,
                                           int32_t nranges, const int32_t* layer_ends_h, const lmc_event_t* events_h,
                                           const lmc_head_window* win, uint32_t* job_status, lmc_stream_t stream);

/* Entropy-decode only (debug / parity): blob -> sym_out int8 [P][T][C].
 * Stands where torchac_cuda.decode_fast_prefsum stands (cachegen_decoder.py:65-66). */
int lmc_decode_symbols(lmc_ctx* ctx, const void* blob, int32_t L, int32_t H, int32_t D, int8_t* sym_out,
                       lmc_stream_t stream);

/* ------------------------------------------------------------------ */
/* lossless gather / scatter (raw chunks)                              */
/* ------------------------------------------------------------------ */
/*
 * Copy tokens [tok_begin, +ntok) between an arbitrary KV layout and a
 * contiguous chunk.  Replaces _tuple_kv_to_blob + _slice_kv_at
 * (cache_engine.py:98-161) on the store side, torch.cat + _blob_to_tuple_kv
 * (cache_engine.py:120-129, 362-368) on the retrieve side, and the external
 * connector's slot_mapping gather / reshape_and_cache_flash scatter
 * (LLM_Engine.rst:91-122).  Both layouts share L, H, D and dtype.
 * dst token index = dst_tok0 + (t - tok_begin).
 * One side (not both) may be LMC_PAGED_SPLIT: the gather from / scatter into vLLM's ROCm paged-attention cache.
 */
int lmc_copy_kv(lmc_ctx* ctx, const lmc_kv_layout* src, int32_t tok_begin, int32_t ntok,
                const lmc_kv_layout* dst, int32_t dst_tok0, lmc_stream_t stream);

/* ------------------------------------------------------------------ */
/* RoPE shift: stored keys to new positions                            */
/* ------------------------------------------------------------------ */
/*
 * Re-rotate, IN PLACE, the keys of tokens [tok_begin, +ntok) of `kv` by a position difference: a segment that was
 * prefilled on its own carries the rotary embedding of positions 0 .. n-1, and placed at offset p in a later prompt
 * (BASELINE.json configs[4]) every key needs R(p) applied first -- RoPE is a rotation group, R(new) = R(new - old) R(old),
 * so the difference and the model's own table suffice.  Stands where the external connector gathers K by slot mapping,
 * applies rotary_emb in torch and scatters K back (three passes and a temporary per layer): one pass over the K planes
 * (k_rope.h), queued behind the decode / copy that filled them, on the same stream, with no host wait.
 *   touches   the K planes (kv = 0) of ALL layers, the given tokens, channels [0, rot_dim) of every head; V planes,
 *             channels >= rot_dim, other tokens and other slots are not written at all
 *   cos_sin   device fp32 [table_rows][rot_dim]: row r = cos(r f_i) for i < rot_dim / 2, then sin(r f_i) -- the layout of
 *             vLLM's cos_sin_cache widened to fp32; any scaling (llama-3, YaRN, ...) is whatever the caller baked in
 *   delta     token tok_begin + i is shifted by d = deltas ? deltas[i] : delta; deltas: device int32 [ntok] or NULL
 *   is_neox   != 0: x1 = channel i, x2 = channel i + rot_dim / 2 (NeoX);  0: x1 = channel 2i, x2 = channel 2i + 1 (GPT-J)
 * With c = row |d| cos and s = sign(d) * row |d| sin:  o1 = x1 c - x2 s,  o2 = x2 c + x1 s, every product and sum rounded
 * to fp32 by itself, then one round-to-nearest-even cast to the layout's dtype.  (The shifted key has then been rounded
 * to 16 bits twice: when it was stored and now.)
 * LMC_ERR_INVALID, with nothing launched: a layout the decoders would refuse; LMC_PAGED_SPLIT (no split addressing here: lmc_rope_shift_split
 * below rotates such a cache in place, or shift the chunk before lmc_copy_kv scatters it); an fp8 dtype (rotating fp8 would round the key to 3 or 2 mantissa bits a
 * second time: not offered); rot_dim odd, < 2 or > head_size; table_rows < 1; a uniform |delta| >= table_rows; ntok < 1,
 * tok_begin < 0, a NULL table; ntok * num_heads * rot_dim / 2 >= 2^31 (split the range).
 * A per-token |deltas[i]| >= table_rows leaves that token untouched and raises LMC_STATUS_BAD_POSITION in job_status (or
 * in the context's sticky word when job_status is NULL), the way the decoders report.
 * Two tokens of the range mapped to one slot: undefined, as for the scatter.  Rows on 16-byte boundaries with
 * head_size % 8 == 0, whole 8-channel vectors per pair half (NeoX: rot_dim % 16 == 0, GPT-J: rot_dim % 8 == 0) and a
 * 16-byte aligned table are rotated with 16-byte accesses; anything else one pair per thread (correct, not fast).
 */
int lmc_rope_shift(lmc_ctx* ctx, const lmc_kv_layout* kv, int32_t tok_begin, int32_t ntok, const float* cos_sin,
                   int32_t table_rows, int32_t rot_dim, int32_t is_neox, int32_t delta, const int32_t* deltas,
                   uint32_t* job_status, lmc_stream_t stream);

/*
 * lmc_rope_shift IN an LMC_PAGED_SPLIT cache (additive in ABI 6; k_rope.h: k_rope_split_vec / k_rope_split_elem): the keys
 * of tokens [tok_begin, +ntok) are re-rotated where the decoder stored them, in the split blocks of vLLM's ROCm
 * paged-attention kernels -- behind a DIRECT decode (lmc_decode_chunks_schedule, lmc_decode_chunks_fixed_split_schedule,
 * lmc_load_pack, a scatter by lmc_copy_kv) there is no staged chunk of rows to rotate first.  The NeoX partners of a pair
 * lie in granules j and j + rot_dim/16 of one (block, head, slot), the GPT-J partners inside one granule.
 *   `kv` must be LMC_PAGED_SPLIT with 16-bit elements (bf16 / fp16); every other argument, the arithmetic, the status
 *   bit and every refusal are lmc_rope_shift's.  LMC_ERR_INVALID with nothing launched as well for: a rows layout
 *   (lmc_rope_shift takes that), a split layout beyond the 32-bit offsets stated at lmc_kv_layout for the decoders, and
 *   ntok * num_heads * (work items of a head) >= 2^31.
 *   touches   channels [0, rot_dim) of the K planes at the slots of the named tokens; V planes, other slots and channels
 *             >= rot_dim are not written at all
 *   A window of layers is a layout of that many layers (plane_ptrs moved by two pointers per layer, or base by
 *   stride_layer): what lmc_range_post does per range.
 * 16-byte accesses (two loads, eight pairs, two stores per NeoX item; consecutive lanes take consecutive tokens, which
 * in a block-ordered mapping are adjacent granules) where the K planes stand on 16-byte boundaries, stride_block and
 * stride_head are multiples of 8 elements, the table is 16-byte aligned and rot_dim % 16 == 0 (NeoX) or % 8 == 0 (GPT-J);
 * anything else one pair per thread (correct, not fast).
 */
int lmc_rope_shift_split(lmc_ctx* ctx, const lmc_kv_layout* kv, int32_t tok_begin, int32_t ntok, const float* cos_sin,
                         int32_t table_rows, int32_t rot_dim, int32_t is_neox, int32_t delta, const int32_t* deltas,
                         uint32_t* job_status, lmc_stream_t stream);

/* ------------------------------------------------------------------ */
/* CacheBlend token selection: KV deviation and top-k                  */
/* ------------------------------------------------------------------ */
/*
 * The selection step of CacheBlend (BASELINE.json configs[4]; additive in ABI 6; csrc/k_blend.h): segments that were
 * prefilled on their own sit in the paged cache (retrieve + lmc_rope_shift), the model recomputes ONE check layer over all
 * tokens, and the tokens whose fresh K/V deviates most from what the cache holds are the ones it recomputes in the deeper
 * layers.  Replaces nothing in the reference v0.1.2 (it has no blending); stands where a connector-side CacheBlend executor
 * gathers the cached layer by slot mapping in torch, subtracts, squares, sums over (head, channel), runs torch.topk (tie
 * order unspecified) and sorts -- a gather per cache layout, three element-wise passes with temporaries the size of the
 * layer's KV -- in the TTFT path of every blended request.
 *
 * lmc_kv_deviation: for token i in [0, ntok)
 *     dev_k[i] = sum over (h, d) of (K_a(a_layer, a_tok0 + i, h, d) - K_b(b_layer, b_tok0 + i, h, d))^2
 *     dev_v[i] = the same sum over the V planes
 *   dev_k, dev_v   device fp32 [ntok]; either may be NULL (that plane is skipped), not both
 *   Tokens are addressed through each layout's own slot_mapping and strides, exactly as lmc_copy_kv addresses its two
 *   sides, and the layouts follow lmc_copy_kv's rules: any strides, any LMC_PAGED_ROWS layout, at most one side
 *   LMC_PAGED_SPLIT; num_heads, head_size and dtype equal on both sides -- num_layers may differ (`a` is typically the
 *   model's fresh [T,H,D] pair of one layer, `b` the whole cache).  bf16 and fp16 only: fp8 is refused as lmc_rope_shift
 *   refuses it (a blended fp8 cache cannot be position-shifted in the first place).
 *   LMC_ERR_INVALID, nothing launched and nothing written: a layout lmc_copy_kv would refuse, a mismatch of H, D or dtype,
 *   fp8, both sides split, a layer out of range, ntok < 1, a negative token offset, both outputs NULL.
 *   Both KV sides are only read.  Elements are widened exactly to fp32; difference, square and sum are fp32.  No float
 *   atomics: for given layouts and shapes the order of the additions is fixed by the code, so a token's sum is the same
 *   bits on every run.  One plain store per token and plane.
 *
 * lmc_select_topk: the min(k, n) tokens with the largest key, key = bits(dev[i]) & 0x7fffffff compared as unsigned -- the
 *   float order of the non-negative values lmc_kv_deviation writes, with NaN above +inf (a token whose KV holds a NaN is
 *   recomputed first).  Ties go to the lower index.
 *   dev       device fp32 [n]
 *   idx_out   device int32: receives min(k, n) indices in ASCENDING order (the order the model recomputes in); nothing
 *             beyond them is written
 *   k comes from the host: no count to read back, no host wait, no allocation.  1 <= n <= 2^20 and k >= 0 (k == 0 writes
 *   nothing and launches nothing); anything else is LMC_ERR_INVALID.  Deterministic.
 * The two calls stay apart on purpose: under tensor parallelism a rank sees its own heads only, and the connector must
 * all-reduce `dev` across the ranks before it selects, or the ranks pick different tokens.
 */
int lmc_kv_deviation(lmc_ctx* ctx, const lmc_kv_layout* a, int32_t a_layer, int32_t a_tok0, const lmc_kv_layout* b,
                     int32_t b_layer, int32_t b_tok0, int32_t ntok, float* dev_k, float* dev_v, lmc_stream_t stream);
int lmc_select_topk(lmc_ctx* ctx, const float* dev, int32_t n, int32_t k, int32_t* idx_out, lmc_stream_t stream);

/* ------------------------------------------------------------------ */
/* host DRAM offload plumbing                                          */
/* ------------------------------------------------------------------ */
/* Pinned, device-accessible host memory (hipHostMalloc).  Replaces the
 * pageable kv_chunk.to("cpu") of LMCLocalBackend.put_blocking and its stubbed
 * pin-memory path (local_backend.py:50,82-100). */
int lmc_pinned_alloc(size_t bytes, void** out_h);
int lmc_pinned_free(void* ptr_h);
/* hipMemcpyAsync on `stream`; kind: 0 = D2H, 1 = H2D, 2 = D2D. */
int lmc_memcpy_async(void* dst, const void* src, size_t bytes, int kind, lmc_stream_t stream);

/*
 * The store leg in ONE call: encode the chunks (as lmc_encode_chunks does, into an arena the context owns) and move
 * every blob, at its exact size, into a pinned host arena -- with no host wait anywhere: the sizes are read on the GPU
 * by the copy kernel (k_offload.h), which also writes them, and the blobs' offsets, to pinned words for later.
 * Stands where LMCLocalBackend.put_blocking / put_nonblocking stand (local_backend.py:82-100): `.to("cpu")` behind a
 * device synchronisation.  A long job leaves in a few parts: the copy of part k (on a stream of the context) runs
 * beside the encode of part k + 1; `stream` is done when everything has landed.
 *   host_arena_h   pinned, device-mapped (lmc_pinned_alloc), host_cap bytes
 *   offsets_h      pinned uint64 [nchunks + 1]: blob i lies at host_arena_h + offsets_h[i]; [nchunks] = bytes used
 *   sizes_h        pinned uint32 [nchunks]: its size (0 and LMC_STATUS_HOST_ARENA_FULL if it did not fit)
 *   job_status     pinned status word of this job (may be NULL: the context's sticky word)
 * All three arrays are valid once `stream` has completed.
 */
int lmc_store_chunks(lmc_ctx* ctx, const lmc_kv_layout* src, int32_t tok_begin, int32_t tok_end, int32_t chunk_tokens,
                     const int32_t* bins_h, void* host_arena_h, uint64_t host_cap, uint64_t* offsets_h,
                     uint32_t* sizes_h, uint32_t* job_status, lmc_stream_t stream);

/*
 * The retrieve leg in ONE call, cut by layers: blobs in pinned host memory -> decoded KV in `dst`.  The blobs' headers
 * are checked by the CPU where they lie (pinned host memory: no GPU work, no wait), every blob goes over PCIe as one
 * hipMemcpyAsync (two copy streams of the context), and behind the transfer the decode runs as one launch per range of
 * `layers_per_range` layers (lmc_decode_chunks_layers) on `stream`, each followed by its event: the caller's model
 * starts on the first layers while the later ranges still decode.  (Per-range transfers -- the K run and the V run of
 * every blob, per range -- were measured slower than whole blobs: many short copies, see lmc_api.hip.)  Stands where
 * LMCLocalBackend.get + CacheGenDeserializer.from_bytes + the engine's torch.cat stand (local_backend.py:128-144,
 * cache_engine.py:339-381): whole chunks to the GPU one `.to("cuda")` at a time, then everything decoded and
 * concatenated, then the first layer can run.
 *   host_blob_ptrs_h  host array [nchunks] of pinned blob addresses (16-byte aligned); read during the call only
 *   sizes_h           host array [nchunks] of their sizes; read during the call only
 *   range_events      NULL, or [ceil(L / layers_per_range)] events: event r is recorded on `stream` behind the decode
 *                     of range r (the KV of its layers is complete once it has fired)
 *   layers_per_range  0 = all layers in one range
 * Returns LMC_ERR_INVALID, with nothing queued at all, if a blob's header does not check out (the stream directory is
 * checked by the decoder: LMC_STATUS_BAD_STREAM in the job's status word).
 * The blobs themselves must stay where they are until `stream` has completed.
 */
int lmc_load_chunks(lmc_ctx* ctx, const void* const* host_blob_ptrs_h, const uint32_t* sizes_h, int32_t nchunks,
                    const lmc_kv_layout* dst, int32_t dst_tok0, int32_t chunk_tokens, int32_t layers_per_range,
                    lmc_event_t* range_events, uint32_t* job_status, lmc_stream_t stream);

/*
 * Packs: the plane-major form of the pinned host tier (lmc_format.h, "pack").  lmc_store_pack is lmc_store_chunks with
 * the job's blobs written TRANSPOSED into one pinned region -- static sections of every chunk, then the streams ordered
 * (plane, chunk): K planes of every layer, then V planes -- so that lmc_load_pack moves the streams of a range of layers
 * as TWO hipMemcpyAsync (their K planes, their V planes) and the
 * model's first layers run while the later ranges are still crossing PCIe.  That is the order the consumer needs and
 * the reference cannot produce: its chunks arrive whole, one `.to("cuda")` each (local_backend.py:128-144), and
 * nothing can be decoded before the last one (cache_engine.py:339-381).
 *
 * lmc_store_pack: encode [tok_begin, tok_end) of `src` and write the pack to pack_h (pinned, device-mapped, pack_cap
 *   bytes; lmc_pack_bound is the worst case, a Llama-3-8B context needs about a quarter of it) without any host wait.
 *   sizes_h: pinned uint32 [nchunks], the blob sizes (0 = that chunk's encode failed).  Valid once `stream` has completed:
 *   the pack header's total_bytes (0 and LMC_STATUS_HOST_ARENA_FULL if the pack did not fit or a chunk failed).
 *   WHERE pack_h points decides who pays: mapped pinned HOST memory makes the call complete by itself (no host wait at
 *   all), but its copy kernel then posts PCIe writes from 64 workgroups for ~10 ms per 16 k context, and a bandwidth-bound
 *   kernel running beside it (a decode step) was measured 4.3x slower for that time -- the form for an otherwise idle
 *   GPU.  DEVICE memory (pack_h and sizes_h both device-accessible) builds the pack in HBM in ~0.3 ms; the caller reads
 *   total_bytes from the 256-byte header and moves the pack with DMA copies, which leave concurrent kernels alone
 *   (1.03x): what lmcache_amd's engine does (CacheGenDeviceCodec.store_pack).
 * lmc_pack_info: check a pack's header and offset table (host only), return the header.
 * lmc_pack_extract: chunk `chunk` of a pack as the blob lmc_encode_chunks wrote, byte for byte (host only: the
 *   one-chunk path of the backend, and how the tests pin a pack to the oracle).
 * lmc_load_pack: chunks [chunk_begin, chunk_begin + nchunks) of the pack (nchunks 0 = all that follow chunk_begin) ->
 *   decoded KV in `dst`, chunk chunk_begin + i at tokens dst_tok0 + i * chunk_tokens.  Offset table and static slots go first, then per range of `layers_per_range` layers
 *   (0 = all in one) the streams -- two copies per range for the whole pack, one per (layer, K/V) for a run of its
 *   chunks -- each followed by the range's decode on `stream` and, if given, range_events[r].  The pack must stay where it
 *   is until `stream` has completed.  LMC_ERR_INVALID, with nothing queued, if the pack does not check out.
 */
int lmc_store_pack(lmc_ctx* ctx, const lmc_kv_layout* src, int32_t tok_begin, int32_t tok_end, int32_t chunk_tokens,
                   const int32_t* bins_h, void* pack_h, uint64_t pack_cap, uint32_t* sizes_h, uint32_t* job_status,
                   lmc_stream_t stream);
/*
 * lmc_store_pack with the encode launched in `nparts` ranges of planes, each range packed as soon as it is coded
 * (round 6): after part r the streams region holds part r's segments at their final offsets, part_info_h[2 r] =
 * the part's offset in the streams region, part_info_h[2 r + 1] = its bytes, and
 * part_events[r] is recorded on `stream` -- the caller moves [off_streams + offset, + bytes) to host memory with a
 * DMA copy while the later planes are still being encoded (CacheGenDeviceCodec.store_pack / finish_pack: a 16 k
 * store completes when its last PCIe byte lands, where lmc_store_pack + one copy of the finished pack waits for the
 * whole encode first).  Header, offset table and static slots ([0, off_streams)) are final after the LAST part.
 * A part of 0 bytes is no verdict on the pack: a part that is not the last packs the planes coded so far BUT the newest
 * one (whose end its successor writes), so a first range of a single plane ships nothing, and the parts of a pack that
 * did not fit read 0 bytes too.  Failure is the job's status word (LMC_STATUS_HOST_ARENA_FULL) and a header that is
 * not a pack's (magic 0, total_bytes 0), both valid after the last part.
 * pack_d must be DEVICE memory (a kernel that posts PCIe writes between the encode's parts would stall them);
 * part_info_h: pinned uint64 [2 nparts]; part_events: [nparts] events or NULL.  A job that cannot be split (a ragged
 * last chunk, a job too small for the fused encode) runs as ONE part: part_info_h[1 .. ) read {0, 0} and the
 * events of the unused parts are recorded behind the only one.  nparts <= 16.
 */
int lmc_store_pack_parts(lmc_ctx* ctx, const lmc_kv_layout* src, int32_t tok_begin, int32_t tok_end, int32_t chunk_tokens,
                         const int32_t* bins_h, void* pack_d, uint64_t pack_cap, uint32_t* sizes_h, int32_t nparts,
                         uint64_t* part_info_h, const lmc_event_t* part_events, uint32_t* job_status, lmc_stream_t stream);
int lmc_pack_info(const void* pack_h, uint64_t nbytes, lmc_pack_header* out);
int lmc_pack_extract(const void* pack_h, uint64_t nbytes, int32_t chunk, void* blob_out, uint64_t cap, uint32_t* size_out);
int lmc_load_pack(lmc_ctx* ctx, const void* pack_h, uint64_t pack_bytes, int32_t chunk_begin, int32_t nchunks,
                  const lmc_kv_layout* dst, int32_t dst_tok0, int32_t layers_per_range, lmc_event_t* range_events,
                  uint32_t* job_status, lmc_stream_t stream);
/* lmc_load_pack with `post` (lmc_range_post, above) done to every range between its decode and range_events[r]: the
 * pinned tier's layer-by-layer retrieve into a paged cache.  post NULL IS lmc_load_pack (one body); a post-op that does
 * not check out is LMC_ERR_INVALID with nothing queued, like a pack that does not.  A split `dst` takes the in-place
 * rotation form of lmc_range_post (`dst` named as its own scatter_dst): lmc_rope_shift_split per range. */
int lmc_load_pack_post(lmc_ctx* ctx, const void* pack_h, uint64_t pack_bytes, int32_t chunk_begin, int32_t nchunks,
                       const lmc_kv_layout* dst, int32_t dst_tok0, int32_t layers_per_range, lmc_event_t* range_events,
                       uint32_t* job_status, lmc_stream_t stream, const lmc_range_post* post);

/*
 * Moving encoded chunks BETWEEN the two local tiers without re-encoding them (bounded tiers: the HBM tier demotes its
 * coldest store group to the pinned tier, a pinned group that is hit again is promoted back).
 *
 * lmc_pack_blobs -- the demotion leg: n already-encoded v6 blobs that lie ANYWHERE in device memory -> one v3 pack in
 *   DEVICE memory, byte for byte the pack lmc_store_pack writes for the same chunks.  No encode, no host wait: the scan
 *   and the copy of one "last" part, both on `stream` (the store path's kernels over a pointer table instead of
 *   base + stride).
 *   blob_ptrs    device array [nchunks] of blob addresses, each 16-byte aligned
 *   blob_bytes   device-accessible uint32 [nchunks]: the room each pointer may be read for (0 = no blob there).  It
 *                stands where the arena stride and the size words stand on the store path: the read bound, and the
 *                test that the chunk was encoded
 *   ntokens      tokens of all chunks together (every chunk chunk_tokens long but, possibly, the last)
 *   A bad header, a blob shorter than its header claims, or a pack that does not fit pack_cap: LMC_STATUS_HOST_ARENA_FULL
 *   in the job's word and a header that is not a pack's (magic 0, total_bytes 0), as lmc_store_pack fails a pack.
 *   The caller knows every blob's size, so it knows the pack's: off_streams + the sum of the blobs' stream_bytes; it
 *   moves the finished pack to pinned memory with DMA copies of that size (never a kernel that stores over PCIe).
 * lmc_unpack_blobs -- the promotion leg, the inverse: chunks [chunk_begin, chunk_begin + nchunks) of a pack in pinned
 *   host memory -> the blobs lmc_encode_chunks wrote, byte for byte, chunk chunk_begin + i at blob_ptrs_h[i] (device
 *   memory, 16-byte aligned, blob_caps_h[i] bytes of room; both arrays are read during the call only).  The host checks
 *   the pack first (LMC_ERR_INVALID with nothing queued, like lmc_load_pack); offset table, static slots and the wanted
 *   segments cross PCIe as DMA copies on the context's copy streams into its load staging, and a kernel on `stream`
 *   writes every static slot's [0, off_streams) and every segment to its place in the blob (the place of plane p comes
 *   from the slot's own stream directory).  A blob that would outgrow its room, or a static slot whose header or
 *   directory does not match the pack's table: LMC_STATUS_BAD_HEADER, and nothing is written for that chunk.
 * lmc_pack_chunk_bytes -- host only: the size lmc_pack_extract would report for chunk `chunk`, without extracting
 *   (how the caller sizes the destinations of lmc_unpack_blobs).
 */
int lmc_pack_blobs(lmc_ctx* ctx, const void* const* blob_ptrs, const uint32_t* blob_bytes, int32_t nchunks, int32_t L,
                   int32_t H, int32_t D, int32_t chunk_tokens, uint32_t ntokens, void* pack_d, uint64_t pack_cap,
                   uint32_t* job_status, lmc_stream_t stream);
int lmc_unpack_blobs(lmc_ctx* ctx, const void* pack_h, uint64_t pack_bytes, int32_t chunk_begin, int32_t nchunks,
                     void* const* blob_ptrs_h, const uint32_t* blob_caps_h, uint32_t* job_status, lmc_stream_t stream);
int lmc_pack_chunk_bytes(const void* pack_h, uint64_t nbytes, int32_t chunk, uint32_t* size_out);

/*
 * lmc_transcode_fixed -- the fixed-width tier's way to a pack: n LMC_MODEL_FIXED blobs that lie ANYWHERE in device memory
 *   -> the blobs lmc_encode_chunks would have written from the KV they were stored from, byte for byte and with equal
 *   size words, without that KV.  Replaces nothing in the reference (it has no second coder model).  Two kernels on
 *   `stream`: k_fixed_expand re-addresses the fixed streams into the symbol workspace, copies the scales and clears the
 *   job's words -- what k_quantize leaves -- and the coder launch of the two-kernel encode follows, chosen as
 *   lmc_encode_chunks chooses it (counts-only or general, ragged last chunk and one-token tail included).  Never the
 *   fused kernel, whatever lmc_ctx_set_encode_path says.  The workspace is the encode jobs' (two, by stream).
 *   blob_ptrs    device array [nchunks] of blob addresses, each 16-byte aligned
 *   blob_bytes   device-accessible uint32 [nchunks]: the room each pointer may be read for (0 = no blob there)
 *   L, H, D, dtype   the geometry and the 16-bit KV dtype the blobs were stored with (no fp8: the fixed tier has none);
 *                    planes of up to LMC_MAX_CHANNELS channels
 *   ntokens      tokens of all chunks together (every chunk chunk_tokens long but, possibly, the last)
 *   bins_h       host int32 [2 L]: must be the bins the blobs hold
 *   blobs_out, blob_stride, sizes, job_status   as lmc_encode_chunks takes them (blob_stride >= lmc_blob_bound, both
 *                    16-byte aligned); header word 23 of the new blobs is 0
 *   Refusals are lmc_encode_chunks's: LMC_ERR_INVALID with nothing queued.  On the device a blob is held against
 *   everything lmc_decode_chunks_fixed_schedule holds it against, in its order, and against the call (L, H, D, dtype,
 *   the chunk's length, the bins): LMC_STATUS_BAD_HEADER / BAD_STREAM / BAD_SCALES in the job's word, no read outside
 *   blob_bytes[i], and the chunk's output is no blob of its KV (the other chunks of the job are not touched by that).
 */
int lmc_transcode_fixed(lmc_ctx* ctx, const void* const* blob_ptrs, const uint32_t* blob_bytes, int32_t nchunks, int32_t L,
                        int32_t H, int32_t D, int32_t dtype, int32_t chunk_tokens, uint32_t ntokens, const int32_t* bins_h,
                        void* blobs_out, uint64_t blob_stride, uint32_t* sizes, uint32_t* job_status, lmc_stream_t stream);

/*
 * lmc_transcode_to_fixed -- the way back, a demoted fixed-width group's promotion: n entropy-coded blobs (LMC_MODEL_COUNTS
 *   or LMC_MODEL_CDF16) that lie ANYWHERE in device memory -> the LMC_MODEL_FIXED blobs lmc_encode_chunks_fixed would have
 *   written from the KV they were stored from, byte for byte, without that KV:
 *       lmc_transcode_to_fixed(lmc_encode_chunks(x)) == lmc_encode_chunks_fixed(x)
 *   over every byte of [0, lmc_fixed_blob_bytes), pads included.  Replaces nothing in the reference (it has no second
 *   coder model).  ONE launch on `stream`: the rANS decoder with a fixed-width sink (k_decode.h, DEC_SINK_FIXED) -- the
 *   two formats share the stream geometry, so the wave that decodes a coded stream writes one fixed-width stream, a plane's
 *   first wave copies the scales, the chunk's first wave writes header, bins and pads.  No workspace (neither KV nor
 *   symbols are staged), no host wait.
 *   blob_ptrs    device array [nchunks] of blob addresses, each 16-byte aligned
 *   blob_bytes   device-accessible uint32 [nchunks]: the room each pointer may be read for (0 = no blob there)
 *   L, H, D, dtype   the geometry and the 16-bit KV dtype the blobs were stored with (no fp8: the fixed tier has none);
 *                    planes of up to LMC_MAX_CHANNELS channels
 *   ntokens      tokens of all chunks together (every chunk chunk_tokens long but, possibly, the last)
 *   bins_h       host int32 [2 L]: must be the bins the blobs hold
 *   out_ptrs     device array [nchunks]: where chunk i's fixed-width blob goes, 16-byte aligned, anywhere
 *   out_bytes    device-accessible uint32 [nchunks]: the room there, >= lmc_fixed_blob_bytes for the chunk's length
 *   Refusals are lmc_transcode_fixed's: LMC_ERR_INVALID with nothing queued (geometry, dtype, bins, a fixed-width blob of
 *   2^32 bytes or more, 2^31 streams or more).  On the device a blob is held against everything lmc_decode_chunks holds it
 *   against, in its order, and against the call: pointer, alignment and room before the header is read, total_bytes
 *   against blob_bytes[i], L / H / D / dtype / the chunk's length, the bins, a coded model (an LMC_MODEL_FIXED input is a
 *   bad header), header word 23 == 0, and the output's pointer and room: LMC_STATUS_BAD_HEADER, and nothing is written for
 *   that stream.  LMC_STATUS_BAD_SCALES / BAD_STREAM are known only once scales or stream have been consumed: that
 *   chunk's output is then unspecified, but nothing is written outside its [out_ptrs[i], + lmc_fixed_blob_bytes), and the
 *   other chunks of the job are not touched by it.
 */
int lmc_transcode_to_fixed(lmc_ctx* ctx, const void* const* blob_ptrs, const uint32_t* blob_bytes, int32_t nchunks,
                           int32_t L, int32_t H, int32_t D, int32_t dtype, int32_t chunk_tokens, uint32_t ntokens,
                           const int32_t* bins_h, void* const* out_ptrs, const uint32_t* out_bytes,
                           uint32_t* job_status, lmc_stream_t stream);

int lmc_stream_create(lmc_stream_t* out);
int lmc_stream_destroy(lmc_stream_t s);
int lmc_stream_synchronize(lmc_stream_t s);
int lmc_stream_wait_event(lmc_stream_t s, lmc_event_t e);
int lmc_event_create(lmc_event_t* out, int timing);
int lmc_event_destroy(lmc_event_t e);
int lmc_event_record(lmc_event_t e, lmc_stream_t s);
int lmc_event_synchronize(lmc_event_t e);
/* 1 = complete, 0 = pending, negative = error */
int lmc_event_query(lmc_event_t e);
int lmc_event_elapsed_ms(lmc_event_t start, lmc_event_t stop, float* ms);

/* Host-side blob header check/parse (no GPU).  Stands where
 * CacheGenEncoderOutput.from_bytes is used to inspect a blob
 * (tests/test_serde.py:60-62).  A kv_dtype other than 0, LMC_DTYPE_FP8_E4M3 or LMC_DTYPE_FP8_E5M2, or an fp8 kv_dtype on a
 * blob whose dtype is not bf16, is refused like any other damaged header.  Only the 128 header bytes are read (callers
 * hand over the header of a blob that lies in device memory, with its length), so of an LMC_MODEL_FIXED blob this call
 * checks what the header alone can say (the totals against each other and against the smallest and largest layout);
 * lmc_fixed_blob_info takes the WHOLE blob (nbytes readable bytes), accepts LMC_MODEL_FIXED only, and also holds the
 * bins, total_bytes and every directory entry against the layout the bins give (lmc_fixed_stream_bytes). */
int lmc_blob_info(const void* blob_h, size_t nbytes, lmc_blob_header* out);
int lmc_fixed_blob_info(const void* blob_h, size_t nbytes, lmc_blob_header* out);

#ifdef __cplusplus
}
#endif
#endif /* LMC_HIP_H */
