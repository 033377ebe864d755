// k_rope.h -- re-rotate stored keys to new positions, in place (RoPE shift).
//
// A key that was computed at position p_old carries R(p_old); placed at p_new it needs R(p_new) = R(p_new - p_old) R(p_old):
// one rotation by the position DIFFERENCE, taken from the model's own cos/sin table (vLLM's cos_sin_cache widened to
// fp32: row r = cos(r f_i) for i < rot/2, then sin(r f_i)).  Replaces the connector's gather-K / rotary / scatter-K in
// torch behind a retrieve of a segment that was prefilled on its own (BASELINE configs[4]): three passes and one
// temporary per layer become one pass over the K planes, read once and written once.  It is a kernel of its own and not
// part of k_decode: a decoder wave owns 64 adjacent channels, and the NeoX partners (i, i + rot/2) of a 128-wide head
// lie in two waves.
//
// The arithmetic, the same in all three kernels and in the CPU statement the tests hold them to (bit for bit): with
// d the token's delta, c = table[|d|][i], s = sign(d) table[|d|][rot/2 + i],
//     o1 = x1 c - x2 s,   o2 = x2 c + x1 s        every product and sum rounded to fp32 by itself, then ONE cast (RNE)
// NeoX: x1 = channel i, x2 = channel i + rot/2.  GPT-J: x1 = channel 2i, x2 = channel 2i + 1.
// A token whose |d| is not a row of the table is left as it was and raises LMC_STATUS_BAD_POSITION.
//
// Work is laid out (layer = blockIdx.y; token, head, piece of the head with the piece fastest), so that a wave of the
// vector kernels reads whole 128-byte runs of token rows.  Addressing is k_copy_kv's: chunks, the per-layer tuple and both
// paged row layouts come with lmc_plane_base / lmc_tok_off.
#pragma once
#include "lmc_device.h"

// 1 (default): the K vectors are loaded and stored with the non-temporal hint -- nothing is re-read.  Measured on a 16 k
// Llama-3-8B context against the plain form (0): contiguous chunk 0.372 against 0.416 ms, NHBD blocks 0.387 against 0.397
// (profiles/rope_shift.md; tools/probes/rope_shift_rates.py times either build).
#ifndef LMC_ROPE_NT
#define LMC_ROPE_NT 1
#endif

typedef float f32x4_t __attribute__((ext_vector_type(4)));

struct RopeArgs {
  KvAddr kv;
  const float* cos_sin;  // [table_rows][rot]
  const int* deltas;     // [ntok] per token, or null: `delta` for all
  u32* status;
  int tok_begin, ntok, rot, table_rows, delta, neox;
  u32 per_head;  // work items of one head: rot/16 (NeoX vectors), rot/8 (GPT-J vectors), rot/2 (element form)
  u32 nitems;    // of one layer: ntok * H * per_head (< 2^31: lmc_rope_shift refuses more)
};

// the table row and the sign of token t's delta; false: |delta| is outside the table
__device__ __forceinline__ bool rope_row(const RopeArgs& a, u32 t, u32& row, bool& neg) {
  const int d = a.deltas ? ((const LMC_GLOBAL int*)a.deltas)[t] : a.delta;
  neg = d < 0;
  row = neg ? 0u - (u32)d : (u32)d;
  return row < (u32)a.table_rows;
}

// (the intrinsics are never contracted into an fma, whatever the build's -ffp-contract says)
__device__ __forceinline__ void rope_pair(float x1, float x2, float c, float s, float& o1, float& o2) {
  o1 = __fsub_rn(__fmul_rn(x1, c), __fmul_rn(x2, s));
  o2 = __fadd_rn(__fmul_rn(x2, c), __fmul_rn(x1, s));
}

template <int DT>
__device__ __forceinline__ u32 rope_cast(float f) {
  return DT == LMC_DTYPE_BF16 ? f2bf16(f) : f2fp16(f);
}

__device__ __forceinline__ uint4 rope_ld(const u16* p) { return LMC_ROPE_NT ? ld_global_u4_nt(p) : ld_global_u4(p); }
__device__ __forceinline__ void rope_st(u16* p, uint4 v) {
#if LMC_ROPE_NT
  u32x4_t t;
  t.x = v.x; t.y = v.y; t.z = v.z; t.w = v.w;
  __builtin_nontemporal_store(t, reinterpret_cast<LMC_GLOBAL u32x4_t*>((LMC_GLOBAL u16*)p));
#else
  st_global_u4(p, v);
#endif
}

// The vector form: rows on 16-byte boundaries, head_size % 8 == 0, and a pair's two halves whole vectors of 8 channels.
//   NEOX   one work item = vector j and vector j + rot/16 of a head: two 16-byte loads, eight pairs, two 16-byte stores
//   GPT-J  one work item = one vector: four pairs
// cos / sin come as 16-byte fp32 vectors of the token's table row.  With one delta for the whole launch that row
// (rot floats, at most 1 KiB for a 256-wide head) is staged in LDS once per workgroup and read from there: half of the
// load instructions of an item would otherwise be global loads of the same few lines.  Per-token deltas read their rows
// from global memory (the table of a model is a few MiB: L2).
template <int DT, bool NEOX>
__global__ __launch_bounds__(256) void k_rope_vec(RopeArgs a) {
  extern __shared__ f32x4_t rope_row_lds[];  // [rot / 4], uniform delta only
  const u32 half4 = (u32)a.rot >> 3;        // 16-byte vectors of cos in front of the sin half of a row
  if (!a.deltas) {
    const u32 row = a.delta < 0 ? 0u - (u32)a.delta : (u32)a.delta;  // (in the table: checked by the host)
    const LMC_GLOBAL f32x4_t* g = (const LMC_GLOBAL f32x4_t*)(a.cos_sin + (size_t)row * a.rot);
    for (u32 i = threadIdx.x; i < 2 * half4; i += 256) rope_row_lds[i] = g[i];
    __syncthreads();
  }
  const u16* const plane = lmc_plane_base(a.kv, (int)blockIdx.y);  // the K plane of this layer (kv = 0)
  const u32 H = (u32)a.kv.H;
  for (u32 id = blockIdx.x * 256u + threadIdx.x; id < a.nitems; id += gridDim.x * 256u) {
    const u32 j = id % a.per_head;
    const u32 r = id / a.per_head;
    const u32 h = r % H, t = r / H;
    u32 row;
    bool neg;
    if (!rope_row(a, t, row, neg)) {
      if (j == 0 && h == 0) atomicOr(a.status, LMC_STATUS_BAD_POSITION);
      continue;
    }
    constexpr int NC = NEOX ? 2 : 1;  // 16-byte vectors of cos (and of sin) per item
    f32x4_t cv[NC], sv[NC];
    if (a.deltas) {
      const LMC_GLOBAL f32x4_t* g = (const LMC_GLOBAL f32x4_t*)(a.cos_sin + (size_t)row * a.rot);
#pragma unroll
      for (int k = 0; k < NC; k++) { cv[k] = g[NC * j + k]; sv[k] = g[half4 + NC * j + k]; }
    } else {
#pragma unroll
      for (int k = 0; k < NC; k++) { cv[k] = rope_row_lds[NC * j + k]; sv[k] = rope_row_lds[half4 + NC * j + k]; }
    }
    float c[4 * NC], s[4 * NC];
#pragma unroll
    for (int k = 0; k < NC; k++) {
      c[4 * k] = cv[k].x; c[4 * k + 1] = cv[k].y; c[4 * k + 2] = cv[k].z; c[4 * k + 3] = cv[k].w;
      s[4 * k] = sv[k].x; s[4 * k + 1] = sv[k].y; s[4 * k + 2] = sv[k].z; s[4 * k + 3] = sv[k].w;
    }
#pragma unroll
    for (int k = 0; k < 4 * NC; k++) s[k] = neg ? -s[k] : s[k];
    u16* const head = const_cast<u16*>(plane) + lmc_tok_off(a.kv, a.tok_begin + (int)t) + (long long)h * a.kv.stride_head;
    if constexpr (NEOX) {
      u16* const p1 = head + 8 * j;
      u16* const p2 = p1 + (a.rot >> 1);
      const uint4 v1 = rope_ld(p1), v2 = rope_ld(p2);
      const u32 w1[4] = {v1.x, v1.y, v1.z, v1.w}, w2[4] = {v2.x, v2.y, v2.z, v2.w};
      u32 q1[4], q2[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {  // word k: pairs 2k (low halves) and 2k + 1 (high halves) of this vector
        float a1, a2, b1, b2;
        rope_pair(h_lo<DT>(w1[k]), h_lo<DT>(w2[k]), c[2 * k], s[2 * k], a1, a2);
        rope_pair(h_hi<DT>(w1[k]), h_hi<DT>(w2[k]), c[2 * k + 1], s[2 * k + 1], b1, b2);
        q1[k] = rope_cast<DT>(a1) | (rope_cast<DT>(b1) << 16);
        q2[k] = rope_cast<DT>(a2) | (rope_cast<DT>(b2) << 16);
      }
      rope_st(p1, make_uint4(q1[0], q1[1], q1[2], q1[3]));
      rope_st(p2, make_uint4(q2[0], q2[1], q2[2], q2[3]));
    } else {
      u16* const p = head + 8 * j;
      const uint4 v = rope_ld(p);
      const u32 w[4] = {v.x, v.y, v.z, v.w};
      u32 q[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {  // word k IS pair 4j + k: x1 its low half, x2 its high half
        float o1, o2;
        rope_pair(h_lo<DT>(w[k]), h_hi<DT>(w[k]), c[k], s[k], o1, o2);
        q[k] = rope_cast<DT>(o1) | (rope_cast<DT>(o2) << 16);
      }
      rope_st(p, make_uint4(q[0], q[1], q[2], q[3]));
    }
  }
}

// The element form, one pair per thread: any strides, any head size, any even rot (a base that is not on a 16-byte
// boundary, rot/2 = 12, ...).  Correct, not fast, like k_copy_kv_elem.
template <int DT>
__global__ __launch_bounds__(256) void k_rope_elem(RopeArgs a) {
  const u16* const plane = lmc_plane_base(a.kv, (int)blockIdx.y);
  const u32 H = (u32)a.kv.H, half = (u32)a.rot >> 1;
  for (u32 id = blockIdx.x * 256u + threadIdx.x; id < a.nitems; id += gridDim.x * 256u) {
    const u32 i = id % half;
    const u32 r = id / half;
    const u32 h = r % H, t = r / H;
    u32 row;
    bool neg;
    if (!rope_row(a, t, row, neg)) {
      if (i == 0 && h == 0) atomicOr(a.status, LMC_STATUS_BAD_POSITION);
      continue;
    }
    const LMC_GLOBAL float* g = (const LMC_GLOBAL float*)(a.cos_sin + (size_t)row * a.rot);
    const float c = g[i];
    const float s = neg ? -g[half + i] : g[half + i];
    LMC_GLOBAL u16* const head = (LMC_GLOBAL u16*)(const_cast<u16*>(plane) + lmc_tok_off(a.kv, a.tok_begin + (int)t) +
                                                   (long long)h * a.kv.stride_head);
    LMC_GLOBAL u16* const p1 = head + (a.neox ? i : 2 * i);
    LMC_GLOBAL u16* const p2 = head + (a.neox ? i + half : 2 * i + 1);
    float o1, o2;
    rope_pair(h2f_rt(*p1, DT), h2f_rt(*p2, DT), c, s, o1, o2);
    *p1 = (u16)rope_cast<DT>(o1);
    *p2 = (u16)rope_cast<DT>(o2);
  }
}
