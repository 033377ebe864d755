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
// The arithmetic, the same in all kernels of this file and in the CPU statement the tests hold them to (bit for bit): with
// d the token's delta, c = table[|d|][i], s = sign(d) table[|d|][rot/2 + i],
//     o1 = x1 c - x2 s,   o2 = x2 c + x1 s        every product and sum rounded to fp32 by itself, then ONE cast (RNE)
// NeoX: x1 = channel i, x2 = channel i + rot/2.  GPT-J: x1 = channel 2i, x2 = channel 2i + 1.
// A token whose |d| is not a row of the table is left as it was and raises LMC_STATUS_BAD_POSITION.
//
// Work is laid out (layer = blockIdx.y; token, head, piece of the head with the piece fastest), so that a wave of the
// vector kernels reads whole 128-byte runs of token rows.  Addressing is k_copy_kv's: chunks, the per-layer tuple and both
// paged row layouts come with lmc_plane_base / lmc_tok_off.  (The LMC_PAGED_SPLIT cache has kernels of its own at the
// end of this file: other addressing, the opposite order.)
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

// ---- the same rotation IN an LMC_PAGED_SPLIT cache (include/lmc_hip.h: key_cache [num_blocks, H, D/8, block_size, 8]) ----
// Behind a decode that wrote the split blocks directly (lmc_rope_shift_split): no staged chunk of rows to rotate.  A
// token's head is D/8 granules of 8 channels (16 bytes), block_size * 8 elements apart; the same granule of the next slot
// of the block is the next 16 bytes.  The NeoX partners of a pair lie in granules j and j + rot/16 of one (block, head,
// slot), the GPT-J partners side by side in one granule -- so the vector items are k_rope_vec's, only found elsewhere:
//     element (t, h, d) = plane + block * stride_block + h * stride_head + (d / 8) * (block_size * 8) + w * 8 + d % 8
// with slot = slot_mapping[tok_begin + t], block = slot / block_size (its offset is 64-bit: blocks may lie any distance
// apart), w = slot % block_size; the rest is the lane's 32-bit part (the rule stated at lmc_kv_layout for the decoders,
// which the host holds the layout to).  The arithmetic is rope_row / rope_pair / rope_cast above, bit for bit.
//
// Work is laid out (layer = blockIdx.y; head, piece of the head, token with the TOKEN fastest): the opposite of
// k_rope_vec, because here it is the slots of a block that are adjacent -- consecutive lanes of a block-ordered mapping
// touch consecutive granules, 256-byte runs at block size 16.
//
// 1: the granules are loaded and stored with the non-temporal hint; 0 (default): plainly.  This pass reads what the
// decoder has just written, and k_rope_vec's answer (LMC_ROPE_NT = 1) does not carry over: measured on the 16 k
// Llama-3-8B context, against lmc_rope_shift on an NHBD cache in the same process, one delta 0.385 ms plain (ratio 0.96)
// against 0.400 with the hint (1.03), per-token deltas 0.840 (2.07) against 0.785 (1.98) -- the plain form wins the case
// the workload produces, a segment moved by one delta (profiles/rope_split.md; tools/probes/rope_split_rates.py times
// either build).
#ifndef LMC_ROPE_SPLIT_NT
#define LMC_ROPE_SPLIT_NT 0
#endif

// the block of token t (64-bit offset) and w * 8, the first element of its slot in a granule's row of slots
__device__ __forceinline__ u16* rope_split_block(const RopeArgs& a, const u16* plane, u32 t, u32& w8) {
  const u32 s = (u32)((const LMC_GLOBAL long long*)a.kv.slot_mapping)[(u32)a.tok_begin + t];
  const u32 bs = (u32)a.kv.block_size;
  const u32 b = s / bs;
  w8 = (s - b * bs) * 8u;
  return const_cast<u16*>(plane) + (long long)b * a.kv.stride_block;
}

// One granule.  `al`: the plane stands on a 16-byte boundary (the strides are whole granules: the host has looked) -- a
// plane that comes out of a pointer table is seen by the kernel only, and one that is off goes element by element.
__device__ __forceinline__ uint4 rope_split_ld(const u16* p, bool al) {
  if (al) return LMC_ROPE_SPLIT_NT ? ld_global_u4_nt(p) : ld_global_u4(p);
  const LMC_GLOBAL u16* q = (const LMC_GLOBAL u16*)p;
  u32 w[4];
#pragma unroll
  for (int k = 0; k < 4; k++) w[k] = (u32)q[2 * k] | ((u32)q[2 * k + 1] << 16);
  return make_uint4(w[0], w[1], w[2], w[3]);
}
__device__ __forceinline__ void rope_split_st(u16* p, uint4 v, bool al) {
  if (al) {
#if LMC_ROPE_SPLIT_NT
    u32x4_t t;
    t.x = v.x; t.y = v.y; t.z = v.z; t.w = v.w;
    __builtin_nontemporal_store(t, reinterpret_cast<LMC_GLOBAL u32x4_t*>((LMC_GLOBAL u16*)p));
#else
    st_global_u4(p, v);
#endif
    return;
  }
  const u32 w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int k = 0; k < 4; k++) { st_global_u16(p + 2 * k, (u16)w[k]); st_global_u16(p + 2 * k + 1, (u16)(w[k] >> 16)); }
}

// The vector form: strides of whole granules, a 16-byte aligned table and a pair's two halves whole granules.
//   NEOX   one work item = granule j and granule j + rot/16 of a (token, head): two 16-byte loads, eight pairs, two stores
//   GPT-J  one work item = one granule: four pairs inside it
// cos / sin as in k_rope_vec: the one row of a uniform delta from LDS, per-token rows from global memory.
template <int DT, bool NEOX>
__global__ __launch_bounds__(256) void k_rope_split_vec(RopeArgs a) {
  extern __shared__ f32x4_t rope_row_lds[];  // [rot / 4], uniform delta only
  const u32 half4 = (u32)a.rot >> 3;        // 16-byte vectors of cos in front of the sin half of a row
  if (!a.deltas) {
    const u32 row = a.delta < 0 ? 0u - (u32)a.delta : (u32)a.delta;  // (in the table: checked by the host)
    const LMC_GLOBAL f32x4_t* g = (const LMC_GLOBAL f32x4_t*)(a.cos_sin + (size_t)row * a.rot);
    for (u32 i = threadIdx.x; i < 2 * half4; i += 256) rope_row_lds[i] = g[i];
    __syncthreads();
  }
  const u16* const plane = lmc_plane_base(a.kv, (int)blockIdx.y);  // the K plane of this layer (kv = 0)
  const bool al = ((uintptr_t)plane & 15u) == 0u;
  const u32 ntok = (u32)a.ntok, gran = (u32)a.kv.block_size * 8u;  // elements from a granule to the next of a slot
  for (u32 id = blockIdx.x * 256u + threadIdx.x; id < a.nitems; id += gridDim.x * 256u) {
    const u32 t = id % ntok;
    const u32 r = id / ntok;
    const u32 j = r % a.per_head, h = r / a.per_head;
    u32 row;
    bool neg;
    if (!rope_row(a, t, row, neg)) {
      if (r == 0) atomicOr(a.status, LMC_STATUS_BAD_POSITION);
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
    u32 w8;
    u16* const blk = rope_split_block(a, plane, t, w8);
    const u32 head = h * (u32)a.kv.stride_head + w8;  // (32 bits: the host holds the layout to the decoders' rule)
    if constexpr (NEOX) {
      u16* const p1 = blk + (head + j * gran);
      u16* const p2 = p1 + ((u32)a.rot >> 4) * gran;
      const uint4 v1 = rope_split_ld(p1, al), v2 = rope_split_ld(p2, al);
      const u32 w1[4] = {v1.x, v1.y, v1.z, v1.w}, w2[4] = {v2.x, v2.y, v2.z, v2.w};
      u32 q1[4], q2[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {  // word k: pairs 2k (low halves) and 2k + 1 (high halves) of this granule
        float a1, a2, b1, b2;
        rope_pair(h_lo<DT>(w1[k]), h_lo<DT>(w2[k]), c[2 * k], s[2 * k], a1, a2);
        rope_pair(h_hi<DT>(w1[k]), h_hi<DT>(w2[k]), c[2 * k + 1], s[2 * k + 1], b1, b2);
        q1[k] = rope_cast<DT>(a1) | (rope_cast<DT>(b1) << 16);
        q2[k] = rope_cast<DT>(a2) | (rope_cast<DT>(b2) << 16);
      }
      rope_split_st(p1, make_uint4(q1[0], q1[1], q1[2], q1[3]), al);
      rope_split_st(p2, make_uint4(q2[0], q2[1], q2[2], q2[3]), al);
    } else {
      u16* const p = blk + (head + j * gran);
      const uint4 v = rope_split_ld(p, al);
      const u32 w[4] = {v.x, v.y, v.z, v.w};
      u32 q[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {  // word k IS pair 4j + k: x1 its low half, x2 its high half
        float o1, o2;
        rope_pair(h_lo<DT>(w[k]), h_hi<DT>(w[k]), c[k], s[k], o1, o2);
        q[k] = rope_cast<DT>(o1) | (rope_cast<DT>(o2) << 16);
      }
      rope_split_st(p, make_uint4(q[0], q[1], q[2], q[3]), al);
    }
  }
}

// The element form, one pair per thread: any strides, any table, any even rot (rot/2 = 12: the partners of a pair in the
// middle of two granules).  Correct, not fast, like k_rope_elem.
template <int DT>
__global__ __launch_bounds__(256) void k_rope_split_elem(RopeArgs a) {
  const u16* const plane = lmc_plane_base(a.kv, (int)blockIdx.y);
  const u32 ntok = (u32)a.ntok, half = (u32)a.rot >> 1, gran = (u32)a.kv.block_size * 8u;
  for (u32 id = blockIdx.x * 256u + threadIdx.x; id < a.nitems; id += gridDim.x * 256u) {
    const u32 t = id % ntok;
    const u32 r = id / ntok;
    const u32 i = r % half, h = r / half;
    u32 row;
    bool neg;
    if (!rope_row(a, t, row, neg)) {
      if (r == 0) atomicOr(a.status, LMC_STATUS_BAD_POSITION);
      continue;
    }
    const LMC_GLOBAL float* g = (const LMC_GLOBAL float*)(a.cos_sin + (size_t)row * a.rot);
    const float c = g[i];
    const float s = neg ? -g[half + i] : g[half + i];
    u32 w8;
    u16* const blk = rope_split_block(a, plane, t, w8);
    const u32 head = h * (u32)a.kv.stride_head + w8;
    const u32 d1 = a.neox ? i : 2 * i, d2 = a.neox ? i + half : 2 * i + 1;
    LMC_GLOBAL u16* const p1 = (LMC_GLOBAL u16*)(blk + (head + (d1 >> 3) * gran + (d1 & 7u)));
    LMC_GLOBAL u16* const p2 = (LMC_GLOBAL u16*)(blk + (head + (d2 >> 3) * gran + (d2 & 7u)));
    float o1, o2;
    rope_pair(h2f_rt(*p1, DT), h2f_rt(*p2, DT), c, s, o1, o2);
    *p1 = (u16)rope_cast<DT>(o1);
    *p2 = (u16)rope_cast<DT>(o2);
  }
}
