"""CacheBlend token selection: which tokens of a blended prompt the model recomputes.

Segments that were prefilled on their own are retrieved into the paged cache at their new positions
(retrieve_into_paged(..., rope=RopeShift(...)), lmcache_amd/rope.py).  That alone ignores the attention between the
segments.  CacheBlend repairs it cheaply: the model recomputes ONE check layer over all tokens, the fresh K/V of every
token is compared with what the cache holds for it, and only the small share of tokens that deviate most is recomputed
in the deeper layers (BASELINE.json configs[4]).  The two steps are two C calls (include/lmc_hip.h, csrc/k_blend.h):

    lmc_kv_deviation   dev[t] = sum over (head, channel) of (fresh - cached)^2, fp32, read in place from the model's
                       [T, H, D] tensors and from the paged cache in any layout retrieve_into_paged fills
    lmc_select_topk    the k tokens with the largest deviation, NaN first, ties to the lower index, ascending

    fresh_k, fresh_v = model.layers[check].kv(hidden)            # [T, H, D], the check layer recomputed
    todo = select_recompute(fresh_k, fresh_v, kv_caches, check, slot_mapping, block_size, "NHDB", ratio=0.15, mask=ret_mask)

Both run on the current stream with no host wait; nothing is allocated but the outputs.  They are functions, not engine
methods: they use nothing of an engine.  Under tensor parallelism every rank sees its own heads only: all-reduce the
result of kv_deviation across the ranks and call select_tokens on the sum, or the ranks pick different tokens.
"""
import math
from typing import Optional, Tuple

import torch

from lmcache_amd import native

_PLANES = ("k", "v", "kv")
_LAYOUTS = ("NBHD", "NHBD", "NHDB")


def _cache_geometry(cache, layout: str) -> Tuple[torch.Tensor, int, int, int]:
    """(a tensor of the layer's cache, H, D, block size) of one entry of kv_caches in `layout`."""
    if layout == "NHDB" and isinstance(cache, (tuple, list)):
        if len(cache) != 2 or cache[1].dim() != 4:
            raise ValueError("NHDB pair: (key_cache [num_blocks, H, D/x, block_size, x], value_cache [num_blocks, H, D, block_size])")
        _, H, D, bs = cache[1].shape
        return cache[1], H, D, bs
    if not isinstance(cache, torch.Tensor) or cache.dim() != 5 or cache.shape[0] != 2:
        raise ValueError(f"a layer cache is a tensor [2, num_blocks, ...] of five dimensions in layout {layout}")
    if layout == "NBHD":
        _, _, bs, H, D = cache.shape
    elif layout == "NHBD":
        _, _, H, bs, D = cache.shape
    else:
        _, _, H, D, bs = cache.shape
    return cache, H, D, bs


def _check(fresh_k, fresh_v, kv_caches, layer, slot_mapping, block_size, layout, planes) -> int:
    """Everything kv_deviation refuses, before anything is queued (ValueError).  -> the number of tokens."""
    if planes not in _PLANES:
        raise ValueError(f"planes must be one of {_PLANES}, got {planes!r}")
    if layout not in _LAYOUTS:
        raise ValueError(f"layout must be one of {_LAYOUTS}, got {layout!r}")
    for name, t in (("fresh_k", fresh_k), ("fresh_v", fresh_v)):
        if not isinstance(t, torch.Tensor) or t.dim() != 3:
            raise ValueError(f"{name} must be a tensor [T, H, D]")
    if fresh_k.shape != fresh_v.shape or fresh_k.dtype != fresh_v.dtype or fresh_k.device != fresh_v.device:
        raise ValueError("fresh_k and fresh_v must share shape, dtype and device")
    if fresh_k.dtype not in (torch.bfloat16, torch.float16):
        raise ValueError(f"fresh K/V of {fresh_k.dtype}: only bfloat16 / float16 KV is compared")
    T, H, D = fresh_k.shape
    if T < 1:
        raise ValueError("no tokens")
    if not len(kv_caches) or not (isinstance(layer, int) and 0 <= layer < len(kv_caches)):
        raise ValueError(f"layer {layer!r} of a cache of {len(kv_caches)} layers")
    ref, cH, cD, bs = _cache_geometry(kv_caches[layer], layout)
    if ref.dtype not in (torch.bfloat16, torch.float16):
        raise ValueError(f"a {ref.dtype} cache cannot be blended (fp8 and uint8 caches cannot be position-shifted in the first "
                         "place); only bfloat16 / float16 caches are")
    if ref.dtype != fresh_k.dtype:
        raise ValueError(f"the cache is {ref.dtype}, the fresh K/V {fresh_k.dtype}")
    if (cH, cD) != (H, D):
        raise ValueError(f"the cache holds heads of {cH} x {cD}, the fresh K/V {H} x {D}")
    if bs != block_size:
        raise ValueError(f"the cache's blocks hold {bs} slots, block_size is {block_size}")
    if ref.device != fresh_k.device:
        raise ValueError(f"the cache lives on {ref.device}, the fresh K/V on {fresh_k.device}")
    if not isinstance(slot_mapping, torch.Tensor) or slot_mapping.dim() != 1 or slot_mapping.numel() != T or \
            slot_mapping.is_floating_point() or slot_mapping.dtype == torch.bool:
        raise ValueError(f"slot_mapping must be an integer tensor with one entry per token ({T})")
    return T


def _check_ratio(ratio) -> None:
    if not (isinstance(ratio, (int, float)) and 0.0 < ratio <= 1.0):
        raise ValueError(f"ratio must lie in (0, 1], got {ratio!r}")


def recompute_count(ratio: float, n: int) -> int:
    """k = ceil(ratio * n) for n >= 1 tokens: at least one, at most all.  (A product that is an integer but for the
    rounding of `ratio` -- 6 / 40 * 40 -- is taken as that integer.)"""
    _check_ratio(ratio)
    x = ratio * n
    k = round(x) if abs(x - round(x)) <= 1e-9 * n else math.ceil(x)
    return max(1, min(n, int(k)))


def _runs(mask_cpu: torch.Tensor):
    """The runs [begin, end) of True entries of a CPU bool vector."""
    m = mask_cpu.to(torch.int8)
    edge = torch.diff(m, prepend=m.new_zeros(1), append=m.new_zeros(1))
    return list(zip(torch.nonzero(edge == 1).flatten().tolist(), torch.nonzero(edge == -1).flatten().tolist()))


def _deviation(fresh_k, fresh_v, kv_caches, layer, slot_mapping, block_size, layout, planes, runs, n) -> torch.Tensor:
    """dev [n] of the tokens of `runs` (n in all), run after run."""
    ctx = native.get_context(fresh_k.device.index)
    a = native.KVLayout.from_kv_tuple(((fresh_k, fresh_v),), "vllm")
    b = native.KVLayout.paged(kv_caches, slot_mapping, block_size, layout)
    dev_k = torch.empty(n, dtype=torch.float32, device=fresh_k.device) if "k" in planes else None
    dev_v = torch.empty(n, dtype=torch.float32, device=fresh_k.device) if "v" in planes else None
    at = 0
    for begin, end in runs:
        ctx.kv_deviation(a, 0, begin, b, layer, begin, end - begin, None if dev_k is None else dev_k[at:],
                         None if dev_v is None else dev_v[at:])
        at += end - begin
    if planes == "kv":
        return dev_k + dev_v
    return dev_k if planes == "k" else dev_v


@torch.no_grad()
def kv_deviation(fresh_k: torch.Tensor, fresh_v: torch.Tensor, kv_caches, layer: int, slot_mapping: torch.Tensor,
                 block_size: int, layout: str = "NBHD", planes: str = "v") -> torch.Tensor:
    """float32 [T]: per token, the squared distance between the fresh and the cached KV of layer `layer`.
      fresh_k, fresh_v   the model's [T, H, D] tensors of that layer (bf16 / fp16, head dimension contiguous); read in
                         place (native.KVLayout.from_kv_tuple), never copied
      kv_caches, slot_mapping, block_size, layout   what retrieve_into_paged takes (native.KVLayout.paged): "NBHD", "NHBD"
                         or "NHDB"; token t is compared with slot slot_mapping[t]
      planes             "v" (the deviation CacheBlend uses), "k", or "kv": the fp32 sum of the two
    ValueError before anything is queued: shapes, dtypes or devices that do not match, an fp8 or uint8 cache."""
    T = _check(fresh_k, fresh_v, kv_caches, layer, slot_mapping, block_size, layout, planes)
    return _deviation(fresh_k, fresh_v, kv_caches, layer, slot_mapping, block_size, layout, planes, [(0, T)], T)


@torch.no_grad()
def select_tokens(dev: torch.Tensor, k: int) -> torch.Tensor:
    """int32 [min(k, T)]: the tokens with the largest deviation, in ascending order.  NaN counts as the largest value (a
    token whose KV holds one is recomputed first), ties go to the lower index: the same tokens on every run and rank."""
    if not isinstance(dev, torch.Tensor) or dev.dim() != 1 or dev.dtype != torch.float32 or dev.numel() < 1:
        raise ValueError("dev must be a float32 vector with one entry per token")
    if not isinstance(k, int) or k < 0:
        raise ValueError(f"k must be a non-negative integer, got {k!r}")
    if dev.numel() > 1 << 20:
        raise ValueError(f"{dev.numel()} tokens: lmc_select_topk takes up to 2^20")
    dev = dev.contiguous()
    out = torch.empty(min(k, dev.numel()), dtype=torch.int32, device=dev.device)
    if out.numel():
        native.get_context(dev.device.index).select_topk(dev, k, out)
    return out


@torch.no_grad()
def select_recompute(fresh_k: torch.Tensor, fresh_v: torch.Tensor, kv_caches, layer: int, slot_mapping: torch.Tensor,
                     block_size: int, layout: str = "NBHD", planes: str = "v", ratio: float = 0.15,
                     mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int32, ascending: the ceil(ratio * n) tokens to recompute among the n tokens where `mask` is True (all T without
    one).  Pass the ret_mask of the retrieves: a token that was not retrieved is the caller's to recompute anyway, its
    slot is never looked up and it cannot be selected.  The indices are indices into the call's tokens.  A mask is read
    on the host (ret_mask lives there); its runs of True become one lmc_kv_deviation each.
    ValueError before anything is queued: whatever kv_deviation refuses, a ratio outside (0, 1], a mask that is not a
    bool vector of T entries or that is False everywhere."""
    T = _check(fresh_k, fresh_v, kv_caches, layer, slot_mapping, block_size, layout, planes)
    _check_ratio(ratio)
    if mask is None:
        runs, n, pos = [(0, T)], T, None
    else:
        if not isinstance(mask, torch.Tensor) or mask.dim() != 1 or mask.dtype != torch.bool or mask.numel() != T:
            raise ValueError(f"mask must be a bool vector with one entry per token ({T})")
        mask_cpu = mask.cpu()
        n = int(mask_cpu.sum())
        if n == 0:
            raise ValueError("mask is False everywhere: no token to select from")
        runs = _runs(mask_cpu)
        pos = None if n == T else torch.nonzero(mask_cpu).flatten().to(dtype=torch.int32).to(fresh_k.device)
    dev = _deviation(fresh_k, fresh_v, kv_caches, layer, slot_mapping, block_size, layout, planes, runs, n)
    picked = select_tokens(dev, recompute_count(ratio, n))
    return picked if pos is None else pos[picked.long()]
