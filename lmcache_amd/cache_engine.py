"""LMCacheEngine -- the drop-in boundary.

Same public surface as the reference's lmcache/cache_engine.py:
  LMCacheEngine(config, metadata)                                        :18-35
  .store(tokens, kv_tensors_raw, skip_existing=True, blocking=True)      :230-287
  .retrieve(tokens, mask=None) -> (KVCache | (), ret_mask)               :293-381
  .close()                                                               :383
  LMCacheEngineBuilder.get_or_create / get / destroy                     :387-436

What stays Python, bit-exact with the reference: token chunking (:68-84), the
SHA-256 prefix-hash chain (:58-66, :86-96), key construction (:37-44), the
skip-existing scan (:183-208), the prefix-only / suffix-mask retrieve rules
(:323-357, :379).

What moved into HIP: the three full-size copies of store()
(_tuple_kv_to_blob :98-118, _slice_kv_at :131-161) and the concat of
retrieve() (:362-368) are gone -- chunks are gathered from / scattered to the
caller's per-layer tensors by the kernels (put_kv_range / get_kv_range), or by
one lmc_copy_kv pass per chunk for backends that only speak chunk tensors.
"""
import hashlib
import os
import time
from typing import Dict, Iterable, List, Optional, Tuple, Union

import torch

from lmcache_amd import native, resharding
from lmcache_amd.config import LMCacheEngineConfig, LMCacheEngineMetadata
from lmcache_amd.logging import init_logger
from lmcache_amd.rope import RopeShift
from lmcache_amd.storage_backend import CreateStorageBackend
from lmcache_amd.utils import CacheEngineKey, KVCache, _lmcache_nvtx_annotate

logger = init_logger(__name__)


def _token_dim(fmt: str) -> int:
    if fmt == "vllm":
        return 0
    if fmt == "huggingface":
        return 1
    raise ValueError(f"Invalid format: {fmt}")


class LMCacheEngine:
    def __init__(self, config: LMCacheEngineConfig, metadata: LMCacheEngineMetadata):
        self.config = config
        self.metadata = metadata
        self.chunk_size = config.chunk_size
        self.save_decode_cache = config.save_decode_cache
        self.engine_ = CreateStorageBackend(config, metadata)
        # retrieve_into_paged(direct=True, rope=...) on an "NHDB" cache: decode into the split blocks and re-rotate the keys
        # there (lmc_rope_shift_split) where LMCACHE_AMD_SPLIT_ROPE=1 is set (read here, once); the default keeps what the
        # tiers have always done with that call -- the coded tiers raise, the fixed-width tier stages
        self.split_rope = os.environ.get("LMCACHE_AMD_SPLIT_ROPE", "0") == "1"
        logger.debug("Current storage backend type %s", type(self.engine_))

    # ------------------------------------------------------------------ index (pure Python)
    def _make_key(self, chunk_hash: str, fmt: str, shard: Optional[Tuple[int, int]] = None) -> CacheEngineKey:
        """shard: (world_size, worker_id) of the store that wrote the chunk, where that is not this engine's own."""
        m = self.metadata
        ws, wid = (m.world_size, m.worker_id) if shard is None else shard
        return CacheEngineKey(fmt, m.model_name, ws, wid, chunk_hash)

    def _num_tokens_in_kv(self, kv_tensors: Union[KVCache, torch.Tensor], fmt: str) -> int:
        return kv_tensors[0][0].shape[_token_dim(fmt)]

    def _get_init_hash(self) -> str:
        return ""

    def _hash(self, tokens: torch.Tensor, prefix_hash: str) -> str:
        # the token bytes are dtype dependent (int64 little-endian for the usual LongTensor)
        return hashlib.sha256(prefix_hash.encode("ascii") + tokens.cpu().numpy().tobytes()).hexdigest()

    def _chunk_tokens(self, tokens: torch.Tensor) -> Iterable[torch.Tensor]:
        for start in range(0, len(tokens), self.chunk_size):
            yield tokens[start:start + self.chunk_size]

    def _prefix_hash(self, token_chunks: Iterable[torch.Tensor], num_skip_chunk: Optional[int] = 0) -> List[str]:
        running = self._get_init_hash()
        out = []
        for chunk in token_chunks:
            running = self._hash(chunk, running)
            out.append(running)
        return out[num_skip_chunk:]

    def _prefix_hashes_of(self, tokens: torch.Tensor, num_skip_chunk: int = 0) -> List[str]:
        """_prefix_hash(_chunk_tokens(tokens), num_skip_chunk) with one device-to-host conversion for the whole
        token tensor and no per-chunk copies (the same digests: the hash input is the chunk's bytes either way) --
        this runs in front of every store / retrieve, 64 chunks for a 16 k context.

        The chain of the LAST call is kept (token bytes + digests): a serving engine looks the same prompt up, retrieves
        it and stores it, and the next turn of a conversation extends it -- the chunks whose bytes equal the kept ones
        (a memcmp of 2 KB per chunk, ~10x cheaper than its SHA-256) take their digests from there, and the chain
        resumes at the first chunk that differs.  Same digests by construction: digest k is a function of bytes
        [0, end of chunk k) alone."""
        buf = tokens.detach().cpu().contiguous().numpy().tobytes()  # (bytes: slices of it compare by memcmp)
        step = self.chunk_size * tokens.element_size()
        running = self._get_init_hash()
        out: List[str] = []
        kept = getattr(self, "_hash_chain", None)
        start = 0
        if kept is not None and kept[0] == step:
            kbuf, khashes = kept[1], kept[2]
            n = min(len(buf), len(kbuf))
            whole = n // step  # (a shorter last chunk hashes different bytes: only whole chunks are compared)
            if whole and buf[:whole * step] == kbuf[:whole * step]:
                same = whole
            else:
                same = 0
                while same < whole and buf[same * step:(same + 1) * step] == kbuf[same * step:(same + 1) * step]:
                    same += 1
            if same:
                out = list(khashes[:same])
                running = out[-1]
                start = same * step
        for pos in range(start, len(buf), step):
            h = hashlib.sha256(running.encode("ascii"))
            h.update(buf[pos:pos + step])
            running = h.hexdigest()
            out.append(running)
        self._hash_chain = (step, buf, list(out))
        return out[num_skip_chunk:]

    def _first_missing_chunk(self, chunk_hashes: List[str], fmt: str) -> Optional[int]:
        """Index of the first chunk the backend does not hold (None: all present) -- the
        skip-existing scan of _make_chunks_skip_existing (:192-202)."""
        for idx, h in enumerate(chunk_hashes):
            if not self.engine_.contains(self._make_key(h, fmt)):
                return idx
        return None

    @staticmethod
    def plan_retrieve(num_tokens: int, chunk_size: int, mask_false_prefix: int, hit_chunks: int):
        """Pure arithmetic of retrieve() (:323-329, :360-365, :379): given how many leading tokens the
        mask skips and how many consecutive chunks (after the skipped whole chunks) hit, return
        (num_skip_chunk, extra_token_len, retrieved_token_count)."""
        num_skip_chunk = mask_false_prefix // chunk_size
        extra = mask_false_prefix - num_skip_chunk * chunk_size
        if hit_chunks == 0:
            return num_skip_chunk, extra, 0
        covered_end = min((num_skip_chunk + hit_chunks) * chunk_size, num_tokens)
        return num_skip_chunk, extra, covered_end - mask_false_prefix

    # ------------------------------------------------------------------ data movement helpers
    def _as_cuda_kv(self, kv: KVCache) -> KVCache:
        if all(k.is_cuda and v.is_cuda for k, v in kv):
            return kv
        return tuple((k.cuda(), v.cuda()) for k, v in kv)

    def _blob_to_tuple_kv(self, blob: torch.Tensor) -> KVCache:
        # (one unbind per layer: layer[0], layer[1] are two indexing calls each -- 64 of them in front of a 32-layer model)
        return tuple(tuple(layer.unbind(0)) for layer in blob.unbind(0))

    # ------------------------------------------------------------------ store
    @_lmcache_nvtx_annotate
    @torch.no_grad()
    def store(self, tokens: torch.Tensor, kv_tensors_raw: KVCache, skip_existing=True, blocking=True) -> None:
        """tokens [seq_len]; kv_tensors_raw: per layer (K, V), [T,H,D] ("vllm") or [H,T,D] ("huggingface")."""
        fmt = self.metadata.fmt
        assert len(tokens.shape) == 1, f"Invalid shape of tokens: {tokens.shape}"
        assert len(kv_tensors_raw) > 0, "Empty kv_tensors"
        assert len(tokens) == self._num_tokens_in_kv(kv_tensors_raw, fmt), \
            "Number of tokens in the kv cache does not match the input tokens"
        self._store_from(tokens, lambda: native.KVLayout.from_kv_tuple(self._as_cuda_kv(kv_tensors_raw), fmt),
                         skip_existing, blocking)

    @_lmcache_nvtx_annotate
    @torch.no_grad()
    def store_paged(self, tokens: torch.Tensor, kv_caches, slot_mapping: torch.Tensor, block_size: int,
                    layout: str = "NBHD", skip_existing=True, blocking=True, direct: bool = False) -> None:
        """store() for a serving engine's PAGED KV cache -- what the external vLLM connector does around
        store() (`lmcache_store_kv`: gather the rows of every layer's cache by slot_mapping into [T,H,D], then
        store; docs/source/developer_tutorial/LLM_Engine.rst:91-122), without the gather copy: the kernels
        read the blocks where they lie.
          kv_caches     per layer a tensor [2, num_blocks, block_size, H, D] (layout "NBHD", vLLM's flash layout)
                        or [2, num_blocks, H, block_size, D] ("NHBD", BASELINE.json's north star), bf16 / fp16
                        or, layout "NHDB", the cache of vLLM's ROCm paged-attention kernels: [2, num_blocks, H, D,
                        block_size] (a view of vLLM's [2, num_blocks, block_size * H * D]) or the (key_cache,
                        value_cache) pair of PagedAttention.split_kv_cache (native.KVLayout.paged); bf16 / fp16 / fp8
          slot_mapping  int64 [len(tokens)]: token t lives in slot slot_mapping[t] = block * block_size + offset
        The engine's fmt must be "vllm" (chunks are keyed and laid out [L,2,T,H,D]).
        An "NHDB" cache has no token rows: by default every tier first brings the range into a vllm chunk on the device
        with one lmc_copy_kv (k_copy_split.h) -- the codec's staging of any layout the row encoders cannot read, the raw
        tiers' own gather -- instead of the connector's torch gather of every layer.
          direct  True: the CacheGen tiers hand an "NHDB" cache to the encoder as it is -- k_quantize reads the split
                  blocks (lmc_encode_chunks_split, lmc_store_pack_parts; k_quantize.h), no staging chunk of the size of
                  the raw KV is allocated and no lmc_copy_kv is launched.  Such a job is coded by k_quantize +
                  k_cdf_encode, never by the fused kernel, and on the pinned tier its pack leaves as one part, without the
                  overlap of the part copies with the encode: it buys memory first, time only
                  where profiles/paged_split_encode.md says so.  Planes of more than 1024 channels (H * D) are staged all
                  the same.  It means nothing for "NBHD" / "NHBD", which are read in place anyway, and nothing for the raw
                  tiers and the chunk-tensor backends, whose gather IS the store.  The stored bytes are the same.
                  The fixed-width HBM tier (local_serde="cachegen-fixed") reads the split blocks with its one kernel
                  (lmc_encode_chunks_fixed_split; k_fixed.h) under the same 1024-channel limit: no gather there either,
                  and on block-ordered slots less time as well (profiles/fixed_model.md)."""
        self._check_paged_store(tokens, kv_caches, slot_mapping)
        self._store_from(tokens, lambda: native.KVLayout.paged(kv_caches, slot_mapping, block_size, layout),
                         skip_existing, blocking, direct=direct and layout == "NHDB")

    @_lmcache_nvtx_annotate
    @torch.no_grad()
    def store_paged_layerwise(self, tokens: torch.Tensor, kv_caches, slot_mapping: torch.Tensor, block_size: int,
                              layout: str = "NBHD", skip_existing=True, direct: bool = False) -> "LayerwiseStore":
        """store_paged() whose encode is issued layer by layer WHILE the forward pass fills the cache: call this before the
        step (the cache tensors exist; only their contents arrive layer by layer), `save_layer(l)` on the model's stream
        right behind layer l's cache write, `finish()` behind the last layer -- the `save_kv_layer` / `wait_for_save`
        hooks of a vLLM v1 connector.  Replaces the reference's store behind the forward pass
        (cache_engine.py:268-282) and the connector's per-layer gather in front of it
        (docs/source/developer_tutorial/LLM_Engine.rst:91-122).  Arguments are store_paged's.
        Hashing, skip_existing and the keys are resolved HERE, from the tokens alone: with everything present every
        method of the returned LayerwiseStore is a no-op; with a stored prefix only the missing chunks' token range is
        encoded and published.
        Layer-wise (LayerwiseStore.layerwise): the two CacheGen tiers of the local backend, chunks of 2 .. 256 tokens
        (the ragged last one included), planes of at most 1024 channels, layouts "NBHD" / "NHBD", and "NHDB" with
        direct=True (the split blocks are read per layer).  save_layer(l) then quantises and entropy-codes layer l's two
        planes on a side stream of the job -- never on the model's -- and layer_event(l) fires once layer l's KV has been
        read; finish() is one pass at HBM speed plus the tier's copies, and leaves what store_paged leaves: the same keys,
        byte for byte the same blobs (and the same pack on the pinned tier).
        The fixed-width HBM tier (local_serde="cachegen-fixed") is layer-wise where LMCACHE_AMD_FIXED_LAYERWISE=1 was set
        when the engine was built (lmc_encode_layers_begin_fixed; k_fixed.h): the same layouts -- "NHDB" with direct=True
        -- and planes, chunks of any length the tier stores; save_layer(l) is one sliced launch of its one kernel, finish()
        a few words per stream.  Without the switch it falls back, as it always has.
        Everything else FALLS BACK: the raw tiers, remote, hybrid and chunk-tensor backends, a job the layer-wise encoder
        does not take, and an "NHDB" cache without `direct` -- it has no token rows to read per layer, and its staging
        gather needs every layer.  save_layer is then a no-op, layer_event(l) is None (nothing has been read: the cache
        must keep every layer until finish), and finish() runs today's store_paged path for the keys resolved here.
        That is correct, not layer-wise -- the rule retrieve_into_paged_layerwise states for its side; logged once."""
        self._check_paged_store(tokens, kv_caches, slot_mapping)
        fmt, cs, ntok = self.metadata.fmt, self.chunk_size, len(tokens)
        plan = self._plan_store(tokens, skip_existing)
        if plan is None:
            return LayerwiseStore(self, None, [], None, 0, 0, False)
        first, keys = plan
        direct = direct and layout == "NHDB"
        src = native.KVLayout.paged(kv_caches, slot_mapping, block_size, layout)
        put = None
        if layout != "NHDB" or direct:
            begin = getattr(self.engine_, "begin_put_kv_layers", None)
            if begin is not None and getattr(self.engine_, "supports_kv_layout", False):
                put = begin(keys, src, fmt, first * cs, ntok, cs)
        if put is None and not getattr(self, "_layerwise_fallback_logged", False):
            self._layerwise_fallback_logged = True
            logger.info("store_paged_layerwise: no layer-wise path for this backend / job: storing in one piece at finish() "
                        "(logged once)")
        return LayerwiseStore(self, put, keys, src, first * cs, ntok, direct)

    def _check_paged_store(self, tokens: torch.Tensor, kv_caches, slot_mapping: torch.Tensor) -> None:
        assert self.metadata.fmt == "vllm", "paged KV is a vLLM layout"
        assert len(tokens.shape) == 1, f"Invalid shape of tokens: {tokens.shape}"
        assert len(kv_caches) > 0, "Empty kv_caches"
        assert len(tokens) == slot_mapping.numel(), "one slot per token"

    def _plan_store(self, tokens: torch.Tensor, skip_existing: bool) -> Optional[Tuple[int, List[CacheEngineKey]]]:
        """Hashes, the skip-existing scan and the keys of a store -> (first chunk to store, its keys on), None: all present."""
        fmt = self.metadata.fmt
        chunk_hashes = self._prefix_hashes_of(tokens)
        first = self._first_missing_chunk(chunk_hashes, fmt) if skip_existing else 0
        if first is None:
            return None
        return first, [self._make_key(h, fmt) for h in chunk_hashes[first:]]

    def _put_range(self, keys, src: native.KVLayout, t0: int, t1: int, blocking: bool, direct: bool) -> int:
        """Tokens [t0, t1) of `src` under `keys`: read in place by a backend that takes a layout, else gathered -> chunks stored."""
        fmt, kw = self.metadata.fmt, {"direct": True} if direct else {}
        if getattr(self.engine_, "supports_kv_layout", False):
            return self.engine_.put_kv_range(keys, src, fmt, t0, t1, self.chunk_size, blocking=blocking, **kw)
        return self.engine_.batched_put(self._gather_chunks(keys, src, fmt, t0, t1), blocking=blocking)

    def _store_from(self, tokens: torch.Tensor, make_src, skip_existing: bool, blocking: bool, direct: bool = False) -> None:
        t_start = time.perf_counter()
        plan = self._plan_store(tokens, skip_existing)
        if plan is None:
            logger.info("Stored/updated 0 chunks (all present)")
            return
        first, keys = plan
        src = make_src()
        t_plan = time.perf_counter()
        n = self._put_range(keys, src, first * self.chunk_size, len(tokens), blocking, direct)
        logger.info("Stored/updated %d chunks, total time %.4fs, planning %.4fs", n,
                    time.perf_counter() - t_start, t_plan - t_start)

    def _gather_chunks(self, keys, src: native.KVLayout, fmt: str, tok_begin: int, tok_end: int):
        """(key, contiguous chunk tensor) pairs for chunk-tensor backends: one lmc_copy_kv pass per chunk
        instead of stack + permute + split + contiguous (:98-118, :141-150)."""
        ctx = native.get_context(src.device.index)
        dt = native.torch_dtype(src.dtype)
        for i, key in enumerate(keys):
            t0 = tok_begin + i * self.chunk_size
            T = min(self.chunk_size, tok_end - t0)
            shape = (src.L, 2, T, src.H, src.D) if fmt == "vllm" else (src.L, 2, src.H, T, src.D)
            chunk = torch.empty(shape, dtype=dt, device=src.device)
            ctx.copy_kv(src, t0, T, native.KVLayout.from_chunk(chunk, fmt), 0)
            yield key, chunk

    # ------------------------------------------------------------------ retrieve
    @_lmcache_nvtx_annotate
    @torch.no_grad()
    def retrieve(self, tokens: torch.Tensor, mask: Optional[torch.Tensor] = None, **resharding) -> Tuple[KVCache, torch.Tensor]:
        """Prefix hits only; `mask` (suffix mask) marks the tokens whose KV is wanted.
        Returns (per-layer (K, V) tuple or (), ret_mask).
        The named parameters are the reference's (tests/test_dropin_api.py holds this mirror to its signature); the one
        keyword taken beyond them is stored_world_size: Optional[int] = None (anything else: TypeError):
        retrieve(tokens, mask, stored_world_size=W) is stored_at(W).retrieve(tokens, mask) -- see stored_at."""
        stored_world_size = resharding.pop("stored_world_size", None)
        if resharding:
            raise TypeError(f"retrieve() got an unexpected keyword argument {next(iter(resharding))!r}")
        if stored_world_size is not None:
            return self.stored_at(stored_world_size).retrieve(tokens, mask)
        target = _DenseTarget(self.metadata.fmt)
        got, ret_mask = self._retrieve_into(tokens, mask, target.make_dst)
        if got == 0:
            return (), ret_mask
        ret = self._blob_to_tuple_kv(target.head(got))
        assert ret[0][0].shape[_token_dim(self.metadata.fmt)] == got
        return ret, ret_mask

    @_lmcache_nvtx_annotate
    @torch.no_grad()
    def retrieve_into_paged(self, tokens: torch.Tensor, kv_caches, slot_mapping: torch.Tensor, block_size: int,
                            layout: str = "NBHD", mask: Optional[torch.Tensor] = None,
                            rope: Optional[RopeShift] = None, direct: bool = False) -> torch.Tensor:
        """retrieve() straight into a serving engine's PAGED KV cache: the decoded (or copied) KV of token t is
        written to slot slot_mapping[t] of every layer's cache -- the connector's `lmcache_retrieve_kv` +
        reshape_and_cache_flash scatter (LLM_Engine.rst:101-122) fused into the decode kernel's store.  Slots
        need not be contiguous or ordered (CacheBlend-style placement of a non-prefix segment, BASELINE
        configs[4]).  Returns ret_mask (True where KV was written); the caches of tokens outside it are untouched.
          slot_mapping  int64 [len(tokens)] (entries of tokens the mask skips are ignored)
        layout "NHDB" (the cache of vLLM's ROCm paged-attention kernels, see store_paged) is by default STAGED, the same
        way for every tier.  The hit chunks are decoded (or copied) into a
        contiguous [L,2,nret,H,D] chunk on the current stream, as retrieve() fills its own blob, and one lmc_copy_kv on
        that stream scatters tokens 0 .. got-1 into the cache (k_copy_split.h); nothing is launched when nothing was
        retrieved.  Costs: device memory the size of the retrieved KV for the duration of the call, and one more pass
        over it.  A side effect: a stored chunk that fails to decode never touches the live
        cache, because the miss is decided before the scatter.
          direct  True: an "NHDB" cache is written the way "NBHD" / "NHBD" are -- the decoder stores into the split blocks
                  themselves (k_decode.h, DEC_PAGED_SPLIT; the raw tiers scatter each stored chunk with lmc_copy_kv): no
                  staged chunk, no second pass, no device memory for the duration of the call.  The price is the side
                  effect above: a stored chunk that fails to decode is a miss in ret_mask, but the slots of the call's
                  tokens may hold garbage by then, as for the row layouts.  With a row layout the keyword changes
                  nothing.  Not with `rope` (ValueError before anything is queued): lmc_rope_shift has no split
                  addressing, and the staged chunk is where the keys are rotated.  The fixed-width HBM tier
                  (local_serde="cachegen-fixed") decodes into the split blocks the same way
                  (lmc_decode_chunks_fixed_split_schedule); asked for `direct` WITH `rope` it does not raise but takes
                  the staged path (logged once).
                  Where LMCACHE_AMD_SPLIT_ROPE=1 was set when the engine was built (engine.split_rope), `direct` WITH
                  `rope` is honoured by every tier that honours `direct` -- the coded HBM tier, the fixed-width tier,
                  pinned packs and blobs, the raw tiers' per-chunk scatter: the KV goes straight into the split blocks
                  and ONE lmc_rope_shift_split (k_rope.h: k_rope_split_*) behind it re-rotates the keys there.  No
                  staged chunk; when everything has completed the caches hold, bit for bit, what the staged call
                  leaves.  The side effect of `direct` stays: a blob that fails to decode is a miss, nothing is
                  rotated, and the call's slots may hold garbage.
          rope  a lmcache_amd.rope.RopeShift: the keys of the retrieved tokens are re-rotated to new positions on the way
                (a segment that was prefilled on its own and is placed at offset p: delta = p; a per-token delta tensor
                has one entry per token of `tokens`).  One lmc_rope_shift (k_rope.h) on the current stream behind the
                decode or copy launches: on the paged cache itself for "NBHD" / "NHBD", on the staged chunk BEFORE the
                scatter for "NHDB".  Nothing is launched on a miss.  The cache must be bf16 / fp16 and rope.rot_dim at
                most its head size (ValueError before anything is queued).  A per-token delta outside the table leaves
                that token's keys as stored and raises LMC_STATUS_BAD_POSITION in the context's status word (a delta
                tensor that lives on the CPU is checked here instead: ValueError).  A cos_sin that is not a contiguous
                device fp32 table once moved to the cache's device is refused when the destination is made (ValueError
                of native.RangePost), before the decode is queued.
        On stored_at(W) -- the chunks were stored under another tensor-parallel degree -- the cache is still this rank's
        own (its head count); the rotation and the staged scatter are queued ONCE, behind the last source's window.  With
        direct=True the known caveat holds: slots of a miss may hold garbage."""
        target = _PagedTarget(self, tokens, kv_caches, slot_mapping, block_size, layout, mask, rope, direct)
        # (without jobs_out no decode job takes the post-ops: _retrieve_into queues them itself, native.RangePost.apply
        # over tokens [0, got) behind the last write, and only when the retrieve did not miss)
        return self._retrieve_into(tokens, mask, target.make_dst, post=target.post)[1]

    def stored_at(self, stored_world_size: Optional[int]) -> "LMCacheEngine":
        """This engine as it RETRIEVES chunks that an instance of another tensor-parallel degree stored: a view on the same
        backend (same configuration and metadata; close the engine, not its views) whose retrieve() and
        retrieve_into_paged() -- their signatures are the engine's, which tests/test_split_decode_host.py and
        tests/test_paged_layerwise_host.py pin -- read across degrees:

            engine.stored_at(1).retrieve_into_paged(tokens, kv_caches, slot_mapping, block_size, layout)

        The keys are made with (stored_world_size, source rank) for every stored shard this rank's KV heads come from
        (resharding.head_sources: contiguous head shards), a chunk is a hit only when ALL its shards are there (the usable
        prefix is the minimum over the sources), and every source decodes its window of heads into the one destination,
        whose head count is H_stored * stored_world_size / world_size.  None, or the engine's own world size: the engine
        itself, today's path untouched.
        ValueError, nothing queued: a backend without the window decode (the raw tiers, chunk-tensor backends) here; head
        counts the two degrees do not divide once the stored geometry is known; retrieve_layerwise and
        retrieve_into_paged_layerwise of a view (a window of heads has no per-range post-op)."""
        if stored_world_size is None or int(stored_world_size) == self.metadata.world_size:
            return self
        if int(stored_world_size) < 1:
            raise ValueError(f"stored_world_size must be a positive tensor-parallel degree, not {stored_world_size!r}")
        if not (getattr(self.engine_, "supports_kv_layout", False) and getattr(self.engine_, "supports_head_window", False)):
            raise ValueError("stored_world_size: this backend cannot take a window of heads out of a stored chunk (the "
                             "CacheGen tiers of the local backend and the remote backends with remote_serde='cachegen' can)")
        view = LMCacheEngine.__new__(LMCacheEngine)
        view.__dict__.update({k: v for k, v in self.__dict__.items() if k not in ("_hash_chain", "_key_memo")})
        view._stored_ws = int(stored_world_size)
        return view

    def _refuse_layerwise_view(self, what: str) -> None:
        if getattr(self, "_stored_ws", None) is not None:
            raise ValueError(f"{what} across tensor-parallel degrees is not built: a window of heads has no per-range "
                             "post-op; use the one-piece call")

    def _direct_retrieve(self, direct: bool, layout: str, rope: Optional[RopeShift] = None) -> bool:
        """`direct` as the backend honours it.  The fixed-width HBM tier (local_serde="cachegen-fixed") decodes straight
        into an "NHDB" cache (lmc_decode_chunks_fixed_split_schedule); asked for that together with a `rope` it does not
        raise as the coded tiers do but takes the staged path, where the keys are rotated (logged once).  With
        LMCACHE_AMD_SPLIT_ROPE=1 (self.split_rope) every tier honours it: the keys are rotated in the split blocks."""
        if getattr(self, "split_rope", False):
            return direct
        if direct and layout == "NHDB" and rope is not None and getattr(self.engine_, "model", None) == "fixed":
            if not getattr(self, "_fixed_direct_logged", False):
                self._fixed_direct_logged = True
                logger.info("retrieve_into_paged(direct=True) with rope on the fixed-width tier: the keys are re-rotated in "
                            "the staged chunk, so the \"NHDB\" cache is filled through it (logged once)")
            return False
        return direct

    @staticmethod
    def _check_rope(rope: RopeShift, kv_caches, layout: str, ntokens: int) -> None:
        """What retrieve_into_paged refuses of a RopeShift before anything is queued (ValueError)."""
        first = kv_caches[0]
        if layout == "NHDB":  # [2, num_blocks, H, D, block_size], or the (key_cache, value_cache [num_blocks, H, D, block_size]) pair
            pair = isinstance(first, (tuple, list))
            ref = first[1] if pair else first
            D = ref.shape[2] if pair else ref.shape[3]
        else:
            ref, D = first, first.shape[-1]
        if ref.dtype not in (torch.bfloat16, torch.float16):
            raise ValueError(f"rope: a {ref.dtype} cache cannot be shifted (rotating fp8 keys would round them to 3 or 2 "
                             "mantissa bits a second time); only bfloat16 / float16 caches are")
        if rope.rot_dim > D:
            raise ValueError(f"rope: rot_dim {rope.rot_dim} is larger than the cache's head size {D}")
        if isinstance(rope.delta, torch.Tensor):
            if rope.delta.numel() != ntokens:
                raise ValueError(f"rope: a per-token delta needs one entry per token of the call: {rope.delta.numel()} "
                                 f"for {ntokens} tokens")
            if not rope.delta.is_cuda and ntokens and int(rope.delta.abs().max()) >= rope.table_rows:
                raise ValueError(f"rope: a per-token delta is outside the table of {rope.table_rows} rows")

    @_lmcache_nvtx_annotate
    @torch.no_grad()
    def retrieve_layerwise(self, tokens: torch.Tensor, mask: Optional[torch.Tensor] = None,
                           layers_per_launch=1) -> "LayerwiseRetrieval":
        """retrieve() that does not make the model wait for the last layer: the KV tuple is returned at once and
        `layer_events` says when each range of layers is complete -- [(first layer after the range, event), ...] in
        layer order; the attention of layer l runs after `wait_layer(l)` (a stream-side wait).  With an HBM-resident
        CacheGen tier (local_device="cuda", local_serde="cachegen") the decode of layer l+1 then hides behind the
        model's layer l and a warm prefix costs the model almost nothing (bench.py: ttft_proxy).  Backends that
        cannot cut their retrieve by layer return one event that covers everything.  Call finish() before
        trusting the KV for good: it waits for the decode and raises if a stored blob was corrupt.
        layers_per_launch: a range size, or a schedule of range sizes whose last entry repeats, e.g. (2, 6, 24).
        On a stored_at() view: ValueError, nothing queued."""
        self._refuse_layerwise_view("retrieve_layerwise")
        target, jobs = _DenseTarget(self.metadata.fmt), []
        got, ret_mask = self._retrieve_into(tokens, mask, target.make_dst, layers_per_launch=layers_per_launch, jobs_out=jobs)
        if got == 0:
            return LayerwiseRetrieval((), ret_mask, [], [])
        blob = target.head(got)
        event_sets = self._event_sets(jobs, target.L, blob.device)
        # (the per-layer (K, V) views are made when `kv` is first read: 33 tensor calls that need not stand between the
        # launches above and the caller's first wait_layer)
        return LayerwiseRetrieval(lambda: self._blob_to_tuple_kv(blob), ret_mask, event_sets[-1], jobs, event_sets)

    @_lmcache_nvtx_annotate
    @torch.no_grad()
    def retrieve_into_paged_layerwise(self, tokens: torch.Tensor, kv_caches, slot_mapping: torch.Tensor, block_size: int,
                                      layout: str = "NBHD", mask: Optional[torch.Tensor] = None,
                                      rope: Optional[RopeShift] = None, direct: bool = False,
                                      layers_per_launch=1) -> "LayerwiseRetrieval":
        """retrieve_into_paged() that does not make the model wait for the last layer -- the two halves of a warm prefix's
        TTFT together: the KV goes straight into the serving engine's paged cache, as retrieve_into_paged writes it, and
        the call returns at once with an event per range of layers, as retrieve_layerwise does.  The shape of a vLLM v1
        connector: start_load_kv() calls this once, wait_for_layer_load(l) is `r.wait_layer(l)` in front of every
        attention layer.  Arguments, layouts and refusals are retrieve_into_paged's (`direct`
        with `rope` on "NHDB": ValueError before anything is queued); layers_per_launch is retrieve_layerwise's.
        Returns a LayerwiseRetrieval whose `kv` is () -- the KV is in the cache -- and whose ret_mask is
        retrieve_into_paged's.  A miss launches nothing: an all-False mask, no events.
        The events: after wait_layer(l, s), work on stream s sees layer l's K and V in the cache in their FINAL state --
        decoded, re-rotated (`rope`), and for a staged "NHDB" retrieve scattered into the split blocks.  What
        retrieve_into_paged queues behind the whole decode (one lmc_rope_shift, one lmc_copy_kv, over all layers) is done
        here per range, between the range's decode and its event, by the C call that launches the range (include/lmc_hip.h,
        lmc_range_post); for "NHDB" with `rope` that is the rotation of the range's staged keys, then their scatter.
        When everything has completed, every cache
        tensor holds, bit for bit, what retrieve_into_paged with the same arguments leaves.
        Staged "NHDB" (direct=False) keeps ONE staged chunk of the retrieved size; the returned object holds it until
        finish().  direct=True sets no scatter: the decoder writes the split blocks.  direct=True with `rope` on "NHDB"
        (LMCACHE_AMD_SPLIT_ROPE=1 when the engine was built; ValueError or the staged path otherwise, as for
        retrieve_into_paged): each range is decoded into the split blocks and its keys are re-rotated there, one
        lmc_rope_shift_split per range in front of the range's event (the in-place form of lmc_range_post); no staged chunk.
        A blob that fails to decode may leave garbage in the call's slots, as for every `direct` retrieve.
        Tiers: the HBM-resident CacheGen tier and the pinned tier's packs are cut by layers as above.  Pinned blobs that
        are no pack (a store of one chunk, LMCACHE_AMD_PINNED_PACKS=0) cross PCIe whole, then decode range by range with
        the post-ops in front of the events: layer 0 waits for that transfer.  The raw tiers and remote backends queue
        everything, then the post-ops for all layers behind it, and ONE event covers every layer: correct, not layer-wise.
        Call finish() before trusting the cache for good: it waits for the decode and raises NativeError if a stored
        blob was corrupt -- the slots of the call's tokens may hold garbage then, as for retrieve_into_paged(direct=True).
        On a stored_at() view: ValueError, nothing queued."""
        self._refuse_layerwise_view("retrieve_into_paged_layerwise")
        target, jobs = _PagedTarget(self, tokens, kv_caches, slot_mapping, block_size, layout, mask, rope, direct), []
        got, ret_mask = self._retrieve_into(tokens, mask, target.make_dst, layers_per_launch=layers_per_launch, jobs_out=jobs,
                                            post=target.post)
        if got == 0:
            return LayerwiseRetrieval((), ret_mask, [], [])
        event_sets = self._event_sets(jobs, target.L, target.device)
        return LayerwiseRetrieval((), ret_mask, event_sets[-1], jobs, event_sets, hold=target.hold)

    @staticmethod
    def _event_sets(jobs: list, L: int, device) -> list:
        """The events of a layer-wise retrieve: one list of (first layer after the range, event) per decode job.  A retrieve
        that spans several stores is several runs (local_backend.get_kv_range), i.e. several jobs, and layer l is complete
        when EVERY job's range that holds l is (round 4 kept only the last job's events and was right only because all
        jobs share a stream)."""
        event_sets = [list(job.layer_events) for _, job in jobs if job is not None and job.layer_events]
        if not event_sets or len(event_sets) < len(jobs):
            # some run of the retrieve (or all of it) carries no per-layer events -- a backend that finished or queued its
            # part in one piece: ONE event recorded now on the current stream, behind everything _retrieve_into queued,
            # covers those runs for every layer (wait_layer used to skip them, which was right only while
            # every run shared this stream AND stood in front of the other runs' events)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(device))
            event_sets.append([(L, ev)])
        return event_sets

    def _retrieve_into(self, tokens: torch.Tensor, mask: Optional[torch.Tensor], make_dst,
                       layers_per_launch: Optional[int] = None, jobs_out: Optional[list] = None,
                       post=None) -> Tuple[int, torch.Tensor]:
        """The body of retrieve(): prefix probe, the first-chunk trim of a suffix mask, then every hit chunk
        written to destination tokens 0 .. got-1 of the layout make_dst(nret, L, H, D, dtype, device) returns.
        -> (got = tokens written, ret_mask).
        post: a callable, asked after make_dst, for the native.RangePost of this retrieve (or None).  The CacheGen tiers
        take it into their decode jobs (get_kv_range(post=...)); behind any other backend it is queued here (`pending`),
        for all layers, once everything has been written.
        A stored_at() view -- chunks stored under another tensor-parallel degree -- takes _retrieve_resharded."""
        if getattr(self, "_stored_ws", None) is not None:
            assert jobs_out is None and not layers_per_launch
            return self._retrieve_resharded(tokens, mask, make_dst, post, self._stored_ws)
        t_start = time.perf_counter()
        fmt = self.metadata.fmt
        cs = self.chunk_size
        ret_mask = torch.ones_like(tokens, dtype=torch.bool)
        num_skip_tok = 0
        if mask is not None:
            num_skip_tok = int(len(mask) - int(torch.sum(mask)))
        num_skip_chunk = num_skip_tok // cs
        if num_skip_tok:
            ret_mask[:num_skip_tok] = False
        chunk_hashes = self._prefix_hashes_of(tokens, num_skip_chunk)
        # the key objects of the last few hash chains are kept (the chain's last digest names the whole chain): a warm
        # prefix is looked up, retrieved and stored with the same 64 keys (round 6: host time in front of the first launch)
        memo = getattr(self, "_key_memo", None)
        if memo is None:
            memo = self._key_memo = {}
        mk = (fmt, chunk_hashes[-1], len(chunk_hashes)) if chunk_hashes else None
        keys = memo.get(mk)
        if keys is None:
            keys = [self._make_key(h, fmt) for h in chunk_hashes]
            if mk is not None:
                if len(memo) >= 4:
                    memo.pop(next(iter(memo)))
                memo[mk] = keys
        dev = torch.device("cuda", torch.cuda.current_device())
        pending = None  # the RangePost this function itself still has to queue, behind everything else

        def miss():
            ret_mask[:] = False
            return 0, ret_mask

        if getattr(self.engine_, "supports_kv_layout", False):
            count = getattr(self.engine_, "contains_prefix", None)
            if count is not None:
                hits = count(keys)  # the same scan inside the backend: one call instead of one per key
            else:
                hits = 0
                for k in keys:
                    if not self.engine_.contains(k):
                        break
                    hits += 1
            _, extra, nret = self.plan_retrieve(len(tokens), cs, num_skip_tok, hits)
            if hits == 0 or nret <= 0:
                return miss()
            try:
                shape0, dtype = self.engine_.chunk_meta(keys[0])
            except KeyError:  # gone since `contains`: a miss
                return miss()
            L = shape0[0]
            H, D = (shape0[3], shape0[4]) if fmt == "vllm" else (shape0[2], shape0[4])
            dst = make_dst(nret, L, H, D, dtype, dev)
            pending = post() if post is not None else None
            try:
                if jobs_out is not None and getattr(self.engine_, "mode", None) in ("hbm-cachegen", "cachegen"):
                    kw = {} if pending is None else {"post": pending}
                    pending = None  # (the decode jobs do it, range by range)
                    got = self.engine_.get_kv_range(keys if hits == len(keys) else keys[:hits], dst, fmt, -extra, cs,
                                                    layers_per_launch=layers_per_launch, jobs_out=jobs_out, **kw)
                else:
                    got = self.engine_.get_kv_range(keys if hits == len(keys) else keys[:hits], dst, fmt, -extra, cs)
            except native.NativeError:
                # a stored blob that does not decode must never reach the model as KV: the whole lookup is a miss
                logger.exception("retrieve: a cached chunk failed to decode; treated as a miss")
                got = 0
            got = hits if got is None else got
            if got < hits:  # some chunks went missing after `contains`: keep the prefix that arrived
                hits = got
                _, extra, nret = self.plan_retrieve(len(tokens), cs, num_skip_tok, hits)
                if hits == 0 or nret <= 0:
                    return miss()
        else:
            chunks = []
            for chunk in self.engine_.batched_get(iter(keys)):
                if chunk is None:
                    break
                chunks.append(chunk)
            hits = len(chunks)
            _, extra, nret = self.plan_retrieve(len(tokens), cs, num_skip_tok, hits)
            if hits == 0 or nret <= 0:
                return miss()
            c0 = chunks[0]
            L = c0.shape[0]
            H, D = (c0.shape[3], c0.shape[4]) if fmt == "vllm" else (c0.shape[2], c0.shape[4])
            dst = make_dst(nret, L, H, D, c0.dtype, c0.device)
            pending = post() if post is not None else None
            ctx = native.get_context(c0.device.index)
            pos = -extra
            for c in chunks:  # scatter every chunk into its slice (replaces slice + torch.cat, :360-368)
                T = c.shape[2] if fmt == "vllm" else c.shape[3]
                skip = max(0, -pos)
                if skip < T:
                    ctx.copy_kv(native.KVLayout.from_chunk(c, fmt), skip, T - skip, dst, pos + skip)
                pos += T
        if pending is not None:  # (only reached behind a retrieve that wrote its nret tokens: every miss has returned)
            with torch.cuda.device(dst.device):
                pending.apply(native.get_context(dst.device.index), dst, 0, nret)
        if num_skip_tok + nret < len(ret_mask):
            ret_mask[num_skip_tok + nret:] = False
        logger.info("Retrieved %d chunks (%d tokens in total) -- elapsed time %.4f", hits, nret,
                    time.perf_counter() - t_start)
        return nret, ret_mask

    def _retrieve_resharded(self, tokens: torch.Tensor, mask: Optional[torch.Tensor], make_dst, post,
                            stored_ws: int) -> Tuple[int, torch.Tensor]:
        """_retrieve_into for chunks stored at tensor-parallel degree `stored_ws` (another than the engine's own): the
        same prefix probe, first-chunk trim and ret_mask, with every hit chunk assembled from the stored shards this
        rank's heads come from -- one get_kv_range(heads=...) per source into the one destination, the post-op queued
        once behind the last."""
        t_start = time.perf_counter()
        fmt, cs, m = self.metadata.fmt, self.chunk_size, self.metadata
        ret_mask = torch.ones_like(tokens, dtype=torch.bool)
        num_skip_tok = 0 if mask is None else int(len(mask) - int(torch.sum(mask)))
        num_skip_chunk = num_skip_tok // cs
        if num_skip_tok:
            ret_mask[:num_skip_tok] = False
        chunk_hashes = self._prefix_hashes_of(tokens, num_skip_chunk)

        def miss():
            ret_mask[:] = False
            return 0, ret_mask

        def keys_of(src_rank: int) -> List[CacheEngineKey]:
            return [self._make_key(h, fmt, (stored_ws, src_rank)) for h in chunk_hashes]

        def prefix(keys) -> int:
            count = getattr(self.engine_, "contains_prefix", None)
            if count is not None:
                return count(keys)
            hits = 0
            for k in keys:
                if not self.engine_.contains(k):
                    break
                hits += 1
            return hits

        # The geometry comes from the first source's first chunk; which rank that is does not depend on the head count
        # (contiguous shards: rank floor(worker_id * stored_ws / world_size) holds this rank's first head).
        first_rank = (m.worker_id * stored_ws) // m.world_size
        first_keys = keys_of(first_rank)
        if not first_keys or prefix(first_keys[:1]) == 0:
            return miss()
        try:
            shape0, dtype = self.engine_.chunk_meta(first_keys[0])
        except KeyError:  # gone since `contains`: a miss
            return miss()
        L = shape0[0]
        H_src, D = (shape0[3], shape0[4]) if fmt == "vllm" else (shape0[2], shape0[4])
        # (ValueError -- nothing has been queued yet -- where the two degrees do not both divide the model's KV heads)
        sources = resharding.head_sources(H_src * stored_ws, m.world_size, m.worker_id, stored_ws)
        H = H_src * stored_ws // m.world_size
        src_keys = [first_keys if s == first_rank else keys_of(s) for s, _, _, _ in sources]
        hits = min(prefix(keys) for keys in src_keys)  # a chunk counts only when all its shards are there
        _, extra, nret = self.plan_retrieve(len(tokens), cs, num_skip_tok, hits)
        if hits == 0 or nret <= 0:
            return miss()
        dev = torch.device("cuda", torch.cuda.current_device())
        dst = make_dst(nret, L, H, D, dtype, dev)
        pending = post() if post is not None else None
        try:
            for keys, (_, src_begin, nheads, dst_begin) in zip(src_keys, sources):
                got = self.engine_.get_kv_range(keys[:hits], dst, fmt, -extra, cs,
                                                heads=native.HeadWindow(H_src, src_begin, nheads, dst_begin))
                hits = min(hits, hits if got is None else got)  # a shard that delivers fewer chunks shrinks the result
                if hits == 0:
                    break
        except native.NativeError:
            logger.exception("retrieve: a cached chunk failed to decode; treated as a miss")
            hits = 0
        _, extra, nret = self.plan_retrieve(len(tokens), cs, num_skip_tok, hits)
        if hits == 0 or nret <= 0:
            return miss()
        if pending is not None:  # once, behind the last source's window: it acts on every head of dst
            with torch.cuda.device(dst.device):
                pending.apply(native.get_context(dst.device.index), dst, 0, nret)
        if num_skip_tok + nret < len(ret_mask):
            ret_mask[num_skip_tok + nret:] = False
        logger.info("Retrieved %d chunks (%d tokens in total) from %d shards stored at TP = %d -- elapsed time %.4f", hits,
                    nret, len(sources), stored_ws, time.perf_counter() - t_start)
        return nret, ret_mask

    def close(self):
        self.engine_.close()


class _DenseTarget:
    """Where retrieve and retrieve_layerwise write: a blob of the engine's format, made once the geometry is known."""

    def __init__(self, fmt: str):
        self.fmt, self.blob, self.L = fmt, None, None

    def make_dst(self, nret, L, H, D, dtype, dev) -> native.KVLayout:
        shape = (L, 2, nret, H, D) if self.fmt == "vllm" else (L, 2, H, nret, D)
        self.blob, self.L = torch.empty(shape, dtype=dtype, device=dev), L
        return native.KVLayout.from_chunk(self.blob, self.fmt)

    def head(self, got: int) -> torch.Tensor:
        return self.blob.narrow(2 if self.fmt == "vllm" else 3, 0, got)


class _PagedTarget:
    """Where retrieve_into_paged and retrieve_into_paged_layerwise write.  Constructing it is what both refuse before
    anything is queued; make_dst is _retrieve_into's destination -- the paged cache itself, or for a staged "NHDB" retrieve
    a [L,2,nret,H,D] chunk of rows -- and post() the native.RangePost that finishes it (the rotation of `rope`, the scatter
    of the staged chunk), None when there is nothing to do."""

    def __init__(self, engine: "LMCacheEngine", tokens, kv_caches, slot_mapping, block_size: int, layout: str, mask, rope, direct):
        assert engine.metadata.fmt == "vllm", "paged KV is a vLLM layout"
        assert len(tokens) == slot_mapping.numel(), "one slot per token"
        self.num_skip_tok = 0 if mask is None else int(len(mask) - int(torch.sum(mask)))
        direct = engine._direct_retrieve(direct, layout, rope)
        if rope is not None:
            if direct and layout == "NHDB" and not getattr(engine, "split_rope", False):
                raise ValueError("direct=True with rope: the keys are re-rotated in the staged chunk (lmc_rope_shift does "
                                 "not address an \"NHDB\" cache); use the staged retrieve")
            engine._check_rope(rope, kv_caches, layout, len(tokens))
        self._cache = (kv_caches, slot_mapping, block_size, layout)
        self.ntokens, self.rope, self.staged = len(tokens), rope, layout == "NHDB" and not direct
        self.L = self.device = self._post = None
        self.hold = (None, None)  # what a caller that returns before the kernels have run keeps alive

    def make_dst(self, nret, L, H, D, dtype, dev) -> native.KVLayout:
        kv_caches, slot_mapping, block_size, layout = self._cache
        skip, rope = self.num_skip_tok, self.rope
        dst = native.KVLayout.paged(kv_caches, slot_mapping[skip:skip + nret], block_size, layout)
        assert dst.L == L and native.torch_dtype(dst.dtype) == dtype, "cache geometry / dtype differs from the stored chunks"
        assert layout != "NHDB" or (dst.H, dst.D) == (H, D), "cache geometry differs from the stored chunks"
        self.L, self.device = L, dst.device
        rows, chunk = dst, None  # where the tokens lie as rows
        if self.staged:
            chunk = torch.empty((L, 2, nret, H, D), dtype=dtype, device=dst.device)
            rows = native.KVLayout.from_chunk(chunk, "vllm")
        if self.staged or rope is not None:
            self._post = native.RangePost(
                cos_sin=None if rope is None else rope.cos_sin.to(dst.device),
                rot_dim=0 if rope is None else rope.rot_dim, is_neox=rope is None or rope.is_neox,
                delta=0 if rope is None or isinstance(rope.delta, torch.Tensor) else rope.delta,
                deltas=None if rope is None else rope.deltas_for(skip, nret, self.ntokens, dst.device),
                # (a split cache that is filled directly names ITSELF: the keys are rotated where the decoder put them,
                # native.RangePost.in_place / the in-place form of lmc_range_post)
                scatter_dst=dst if self.staged or (rope is not None and layout == "NHDB") else None)
        self.hold = (chunk, self._post)
        return rows

    def post(self) -> Optional[native.RangePost]:
        return self._post


class LayerwiseStore:
    """What store_paged_layerwise returns.  `layerwise`: the encode runs per layer (else: in one piece at finish, or --
    nothing to store -- never); `nchunks`: chunks that will be stored."""

    def __init__(self, engine: "LMCacheEngine", put, keys, src, tok_begin: int, tok_end: int, direct: bool):
        self._engine, self._put, self._keys, self._src = engine, put, keys, src
        self._range, self._direct = (tok_begin, tok_end), direct
        self._done = False

    @property
    def layerwise(self) -> bool:
        return self._put is not None

    @property
    def nchunks(self) -> int:
        return len(self._keys)

    def save_layer(self, layer: int) -> None:
        """Layer `layer`'s K and V are in the cache as far as the CURRENT stream is concerned: encode them (on the job's
        side stream, behind an event recorded here).  Layers in ascending order from 0."""
        if self._put is not None:
            self._put.encode_layer(layer)

    def layer_event(self, layer: int):
        """The event behind which layer `layer`'s KV has been read and its cache may be overwritten; None when the store is
        not layer-wise (nothing is read before finish) or there is nothing to store."""
        return self._put.layer_event(layer) if self._put is not None else None

    def finish(self, blocking: bool = True) -> int:
        """Behind the last layer: finish the blobs and hand them to the tier (blocking=False: the tier's copies and the
        publishing run on the backend's worker thread; backend.drain() waits for them).  -> chunks stored."""
        if self._done or not self._keys:
            return 0
        self._done = True
        eng, (t0, t1) = self._engine, self._range
        if self._put is not None:
            n = self._put.finish(blocking=blocking)
        else:
            n = eng._put_range(self._keys, self._src, t0, t1, blocking, self._direct)
        self._src = None
        return n


class LayerwiseRetrieval:
    """What retrieve_layerwise and retrieve_into_paged_layerwise return: the KV tuple (being filled layer by layer; () when
    the KV goes into a paged cache), ret_mask, and the events."""

    def __init__(self, kv, ret_mask, layer_events, jobs, event_sets=None, hold=None):
        # `layer_events` is the LAST run's list only (kept for callers of rounds 2-4): a retrieve that spans several
        # stores has one list per run, and layer l is complete when every run's range that holds l is -- use wait_layer()
        self._kv, self.ret_mask, self.layer_events, self._jobs = kv, ret_mask, layer_events, jobs
        self._event_sets = event_sets if event_sets is not None else ([layer_events] if layer_events else [])
        self._hold = hold  # retrieve_into_paged_layerwise: the staged chunk and what the post-ops read, until finish()

    @property
    def kv(self):
        """The per-layer (K, V) tuple (being filled layer by layer); () on a miss."""
        if callable(self._kv):
            self._kv = self._kv()
        return self._kv

    def wait_layer(self, layer: int, stream: Optional[torch.cuda.Stream] = None) -> None:
        """Make `stream` (default: the current one) wait until the KV of `layer` is complete.  No host wait."""
        if not self.layer_events:
            return
        st = stream or torch.cuda.current_stream()

        def wait(ev):  # a torch event, or a native.NativeEvent recorded by lmc_load_chunks
            if hasattr(ev, "handle"):
                ev.wait(st.cuda_stream)
            else:
                st.wait_event(ev)

        for events in self._event_sets:  # every decode job of the retrieve: the range of ITS events that holds `layer`
            for end, ev in events:
                if layer < end:
                    wait(ev)
                    break
            else:
                wait(events[-1][1])

    def finish(self) -> None:
        """Host-side completion: waits for the decode and raises NativeError if a blob did not check out."""
        jobs, self._jobs = self._jobs, []
        try:
            for codec, job in jobs:
                codec.finish_decode(job)
            if self._hold is not None and not jobs and self.layer_events:
                self.layer_events[-1][1].synchronize()  # a backend without jobs: its one event
        finally:
            self._hold = None


class LMCacheEngineBuilder:
    """Per-process registry of engines by instance id (cache_engine.py:387-436)."""
    _instances: Dict[str, LMCacheEngine] = {}
    _cfgs: Dict[str, LMCacheEngineConfig] = {}
    _metadatas: Dict[str, LMCacheEngineMetadata] = {}

    @classmethod
    def get_or_create(cls, instance_id: str, config: LMCacheEngineConfig,
                      metadata: LMCacheEngineMetadata) -> LMCacheEngine:
        if instance_id in cls._instances:
            if cls._cfgs[instance_id] != config or cls._metadatas[instance_id] != metadata:
                raise ValueError(f"Instance {instance_id} already exists with a different configuration or metadata.")
            return cls._instances[instance_id]
        engine = LMCacheEngine(config, metadata)
        cls._instances[instance_id] = engine
        cls._cfgs[instance_id] = config
        cls._metadatas[instance_id] = metadata
        return engine

    @classmethod
    def get(cls, instance_id: str) -> Optional[LMCacheEngine]:
        return cls._instances.get(instance_id)

    @classmethod
    def destroy(cls, instance_id: str) -> None:
        engine = cls._instances.pop(instance_id, None)
        if engine is not None:
            engine.close()
        cls._cfgs.pop(instance_id, None)
        cls._metadatas.pop(instance_id, None)
