"""Which stored shards a tensor-parallel rank reads when the KV was stored under another tensor-parallel degree.

A stored chunk belongs to one TP shard: its key carries (world_size, worker_id) and its blob holds that rank's KV heads.
With contiguous head shards -- rank r of W owns KV heads [r * total / W, (r + 1) * total / W) -- the heads of a rank of
one degree are a union of head WINDOWS of ranks of another degree; the decoders take such a window out of a blob
(native.HeadWindow, lmc_decode_chunks_heads_schedule).  Pure arithmetic, no device.
"""
from typing import List, Tuple


def head_sources(total_kv_heads: int, world_size: int, worker_id: int, src_world_size: int) -> List[Tuple[int, int, int, int]]:
    """The shards of a store made at tensor-parallel degree `src_world_size` that rank `worker_id` of `world_size` reads
    -> [(src_worker_id, src_head_begin, nheads, dst_head_begin), ...] in ascending source rank (= ascending destination
    head): heads [src_head_begin, + nheads) of source rank src_worker_id's blobs are heads [dst_head_begin, + nheads) of
    this rank.  Every head of the rank is covered exactly once.
    ValueError unless both degrees divide total_kv_heads: replicated KV heads (a TP degree above the KV head count) have
    no contiguous-shard description."""
    for name, v in (("total_kv_heads", total_kv_heads), ("world_size", world_size), ("src_world_size", src_world_size)):
        if int(v) != v or v < 1:
            raise ValueError(f"{name} must be a positive integer, not {v!r}")
    if not 0 <= worker_id < world_size:
        raise ValueError(f"worker_id {worker_id} is outside [0, {world_size})")
    if total_kv_heads % world_size or total_kv_heads % src_world_size:
        raise ValueError(f"{total_kv_heads} KV heads are not divisible by both tensor-parallel degrees ({world_size} and "
                         f"{src_world_size}): replicated KV heads are not resharded")
    per_dst, per_src = total_kv_heads // world_size, total_kv_heads // src_world_size
    lo, hi = worker_id * per_dst, (worker_id + 1) * per_dst  # this rank's heads, in the model's numbering
    out = []
    for s in range(lo // per_src, (hi - 1) // per_src + 1):
        a, b = max(lo, s * per_src), min(hi, (s + 1) * per_src)
        out.append((s, a - s * per_src, b - a, a - lo))
    return out
