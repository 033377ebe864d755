"""RoPE shift: what retrieve_into_paged needs to hand a model keys at NEW positions.

A segment that was prefilled on its own (RAG / CacheBlend, BASELINE.json configs[4]) carries the rotary embedding of
positions 0 .. n-1.  Placed at offset p of a later prompt, every key has to be rotated by p positions first.  RoPE is a
rotation group, R(new) = R(new - old) R(old): the position DIFFERENCE and the model's own cos/sin table are enough, and
lmc_rope_shift (include/lmc_hip.h, csrc/k_rope.h) applies it in place in one pass over the K planes.

    rope = RopeShift.from_cos_sin_cache(model.rotary_emb.cos_sin_cache, is_neox=True, delta=p)
    engine.retrieve_into_paged(tokens, kv_caches, slot_mapping, block_size, layout, rope=rope)
"""
from dataclasses import dataclass
from typing import Union

import torch


@dataclass
class RopeShift:
    """cos_sin  device float32 [table_rows, rot_dim]: row r = cos(r f_i) for i < rot_dim / 2, then sin(r f_i) -- vLLM's
                cos_sin_cache widened to fp32; any scaling (llama-3, YaRN, ...) is whatever the model baked into it
       rot_dim  rotated channels of a head (the first rot_dim; partial rotary leaves the rest alone)
       is_neox  True: pairs (i, i + rot_dim / 2) (NeoX, Llama);  False: pairs (2i, 2i + 1) (GPT-J)
       delta    new position - stored position: an int for every token, or an int32 tensor with one entry per token of
                the retrieve call (entry t belongs to tokens[t]; |delta| must be a row of the table)"""
    cos_sin: torch.Tensor
    rot_dim: int
    is_neox: bool = True
    delta: Union[int, torch.Tensor] = 0

    def __post_init__(self):
        t = self.cos_sin
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype != torch.float32:
            raise ValueError("cos_sin must be a float32 tensor [table_rows, rot_dim] (from_cos_sin_cache widens a model's cache)")
        if t.shape[0] < 1 or t.shape[1] != self.rot_dim:
            raise ValueError(f"cos_sin is {tuple(t.shape)}: rot_dim = {self.rot_dim} columns and at least one row expected")
        if self.rot_dim < 2 or self.rot_dim % 2:
            raise ValueError(f"rot_dim must be even and at least 2, got {self.rot_dim}")
        if not t.is_contiguous():
            raise ValueError("cos_sin must be contiguous")
        if isinstance(self.delta, torch.Tensor):
            if self.delta.dtype != torch.int32 or self.delta.dim() != 1:
                raise ValueError("a per-token delta must be a one-dimensional int32 tensor")
        elif not isinstance(self.delta, int) or abs(self.delta) >= t.shape[0]:
            raise ValueError(f"delta {self.delta!r} is outside the table of {t.shape[0]} rows")

    @property
    def table_rows(self) -> int:
        return self.cos_sin.shape[0]

    @staticmethod
    def from_base(base: float, rot_dim: int, table_rows: int, device, is_neox: bool = True,
                  delta: Union[int, torch.Tensor] = 0) -> "RopeShift":
        """The table of vLLM's RotaryEmbedding._compute_cos_sin_cache, computed ON THE CPU in fp32 and then moved: cos on
        the GPU and on the CPU differ in the last bit, and the table must be the same on every machine."""
        if rot_dim < 2 or rot_dim % 2:
            raise ValueError(f"rot_dim must be even and at least 2, got {rot_dim}")
        if table_rows < 1:
            raise ValueError(f"table_rows must be at least 1, got {table_rows}")
        inv_freq = 1.0 / (base ** (torch.arange(0, rot_dim, 2, dtype=torch.float32) / rot_dim))
        freqs = torch.outer(torch.arange(table_rows, dtype=torch.float32), inv_freq)
        table = torch.cat((freqs.cos(), freqs.sin()), dim=-1)
        return RopeShift(table.to(device), rot_dim, is_neox, delta)

    @staticmethod
    def from_cos_sin_cache(cache: torch.Tensor, is_neox: bool = True, delta: Union[int, torch.Tensor] = 0) -> "RopeShift":
        """A model's rotary_emb.cos_sin_cache [max_position, rot_dim] of any float dtype, widened to fp32."""
        if not isinstance(cache, torch.Tensor) or cache.dim() != 2 or not cache.is_floating_point():
            raise ValueError("cos_sin_cache must be a floating-point tensor [max_position, rot_dim]")
        return RopeShift(cache.float().contiguous(), cache.shape[1], is_neox, delta)

    def deltas_for(self, first: int, count: int, total: int, device) -> Union[None, torch.Tensor]:
        """The per-token deltas of tokens [first, first + count) of a retrieve call of `total` tokens, as the device int32
        tensor lmc_rope_shift reads (None: one delta for all)."""
        if not isinstance(self.delta, torch.Tensor):
            return None
        if self.delta.numel() != total:
            raise ValueError(f"a per-token delta needs one entry per token of the call: {self.delta.numel()} for {total} tokens")
        return self.delta[first:first + count].to(device).contiguous()
