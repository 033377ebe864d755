// k_copy_split.h -- gather / scatter between vLLM's ROCm paged-attention cache layout (LMC_PAGED_SPLIT, include/lmc_hip.h)
// and any layout of rows (a chunk, per-layer tensors, NBHD / NHBD blocks).
//
// The split layout keeps, per block b and head h, one dense run of D * block_size elements:
//   K(b, h, d, w) = b * stride_block + h * stride_head + (d / X) * (block_size * X) + w * X + d % X     X = 16 / element bytes
//   V(b, h, d, w) = b * stride_block + h * stride_head + d * block_size + w
// so a token's channels are NOT contiguous: in K its 16-byte granules lie block_size * 16 bytes apart, in V every element
// lies block_size elements from the next.  On the row side the same data are block_size rows of D elements.
//
// Work item of ONE WAVE: (plane, head, tile of TT consecutive tokens of the range); TT = 32 / 16 / 8, the largest that
// divides block_size (the host's choice: a tile of a block-ordered mapping then is TT consecutive slots of one block, and
// for block_size 8 .. 32 the whole block).  The tiles are anchored at the slot of the range's first token (off0 = that
// slot % TT), so a range that begins in the middle of a block still has its later tiles on block boundaries; the lanes of
// the first and the last tile that have no token are masked.
//
// FAST tile (decided per tile from the slot values, wave-uniform: one ballot): every token of the tile sits at slot
// (first slot + its distance), the TT slots lie inside one block, both plane bases are on 16-byte boundaries and the host
// found every stride a multiple of X.  Then both sides move 16 bytes per lane and the permutation happens in an LDS
// image of the tile, TT * D elements = NV = TT * NG granules of 16 bytes (NG = D / X granules per row):
//   K  the granule is the unit: (g, w) <-> (w, g), no sub-vector shuffling.
//      gather:  split-side lanes (v -> g = v / TT, w = v % TT: runs of TT * 16 contiguous bytes) write their granule to
//               the ROW image at Pg(w, g); row-side lanes read position v linearly and own granule (w = v / NG,
//               g = (v % NG - rot(w)) mod NG) of the row: the NG lanes of a row still cover its D elements.
//      scatter: row-side lanes (v -> w = v / NG, g = v % NG) write to the SPLIT image at Ps(g, w); split-side lanes read
//               position v linearly and own (g = v / TT, w = (v % TT - g) mod TT).
//   V  an element transpose D x w <-> w x D over the ROW image in both directions: the split-side lane (v -> d = v / GPR,
//      part = v % GPR, GPR = TT / X granules per channel) holds X tokens of one channel and writes (gather) or reads
//      (scatter) them as X single elements at Pg(part * X + k, d / X) * X + d % X; the row-side lanes move whole granules
//      at their linear positions as for K.
// LDS banks (MI355X: 64 banks of 4 bytes; a ds_write_b128 is served in groups of 8 consecutive lanes over 32 banks, i.e.
// eight 16-byte slots, position mod 8; a ds_read_b128 in four groups of 16 lanes whose lane numbers are distinct mod 16,
// over 64 banks; 4-byte and narrower accesses in two groups of 32 lanes over 32 banks).  Every LINEAR phase is conflict
// free by construction: lane = position.  The PERMUTED phases use a rotation instead of padding, so that the image stays
// NV granules and the linear side stays linear:
//   Pg(w, g) = w * NG + (g + rot(w)) mod NG,   rot(w) = (NG even ? w : 0) + w / 8
//   Ps(g, w) = g * TT + (w + g) mod TT
// Eight consecutive lanes of a K write hold eight consecutive w (gather) or g (scatter) of one column: without the
// rotation their positions differ by multiples of NG (TT) and share a slot whenever that is a multiple of 8 -- an
// eight-way conflict for D = 128; with it they step by NG + 1 (odd) or TT + 1 and take eight different slots, except
// where the rotation wraps around the row inside the group: two runs of distinct slots, two-way at worst.  The w / 8 term
// separates the GPR parts of a V lane group (tokens 8 apart) the same way.  tools/probes/split_lds_banks.py enumerates
// the four permuted phases with these group rules for every D up to 512, both element sizes and TT 8 / 16 / 32: at most
// two-way everywhere from NG = 4 on (an NG of 3 is three-way in the K scatter), which is why the fast path asks for
// NG >= 4.  (For V's single-element WRITES two lanes on the two halves of one dword are counted as one address, as they
// are for reads.)
//
// Any other tile -- a token-random mapping, a run that breaks or crosses a block inside the tile, an unaligned base,
// a geometry the host ruled out -- is copied element by element from the same formulas: correct, slow.
// A scatter writes only elements of the slots it was given: K granules of valid tokens, V granules whose X tokens are
// all valid as 16 bytes and the others element by element.  The source is streamed once: non-temporal loads.
#pragma once
#include "lmc_device.h"

struct SplitCopyArgs {
  KvAddr sp, rw;  // the split side and the row side (which is source: the template's GATHER)
  int sp_tok0, rw_tok0, ntok;
  int P, ntiles;  // ntiles: an upper bound of the tiles the range touches (the last may be empty)
  int fast;       // host: strides of both sides are multiples of X, NG >= 4 and the image fits the LDS the launch asked for
};

#define SPLIT_WAVES 4
#define SPLIT_MAX_IMAGE 16384  // bytes of one wave's tile image

// e / R and e % R for wave-uniform 4 <= R <= 2048 and e < 2048 through one float multiply: the quotient is below 2^9, so
// the product is off by less than 2^9 * 2^-22 = 2^-13, and (e + 0.5) / R is never within 0.5 / R >= 2^-12 of an integer.
__device__ __forceinline__ void split_divmod(u32 e, u32 R, float rcpR, u32& q, u32& r) {
  q = (u32)(((float)e + 0.5f) * rcpR);
  r = e - q * R;
}
__device__ __forceinline__ u32 split_addmod(u32 x, u32 y, u32 R) {  // (x + y) mod R for x, y < R
  const u32 t = x + y;
  return t >= R ? t - R : t;
}
__device__ __forceinline__ u32 split_submod(u32 x, u32 y, u32 R) {  // (x - y) mod R for x, y < R
  return x >= y ? x - y : x + R - y;
}

template <typename E>
__device__ __forceinline__ E split_elem(const uint4& v, int k) {  // element k of a granule (k a compile-time constant after unrolling)
  const u32 w[4] = {v.x, v.y, v.z, v.w};
  if constexpr (sizeof(E) == 2) return (E)(w[k >> 1] >> (16 * (k & 1)));
  else return (E)(w[k >> 2] >> (8 * (k & 3)));
}
template <typename E>
__device__ __forceinline__ uint4 split_pack(const E* e) {
  uint4 o;
  if constexpr (sizeof(E) == 2) {
    o.x = e[0] | ((u32)e[1] << 16); o.y = e[2] | ((u32)e[3] << 16);
    o.z = e[4] | ((u32)e[5] << 16); o.w = e[6] | ((u32)e[7] << 16);
  } else {
    o.x = e[0] | ((u32)e[1] << 8) | ((u32)e[2] << 16) | ((u32)e[3] << 24);
    o.y = e[4] | ((u32)e[5] << 8) | ((u32)e[6] << 16) | ((u32)e[7] << 24);
    o.z = e[8] | ((u32)e[9] << 8) | ((u32)e[10] << 16) | ((u32)e[11] << 24);
    o.w = e[12] | ((u32)e[13] << 8) | ((u32)e[14] << 16) | ((u32)e[15] << 24);
  }
  return o;
}

// What a fast tile's lanes need, all wave-uniform but `roff` (lane l: the row offset of tile position l).
template <typename E>
struct SplitTile {
  const E* sp;   // split side at (block, head, slot w0 of the block): tile position 0
  const E* rw;   // row side at (plane, head): + roff of a position
  uint4* img;
  long long roff;
  int lo, hi;    // the tile positions that hold tokens of the range
  u32 NG, NV, bs;
  float rcpNG;
  bool rot_w;
  // rot(w) mod NG
  __device__ __forceinline__ u32 rotm(u32 w) const {
    u32 q, r;
    split_divmod((rot_w ? w : 0u) + (w >> 3), NG, rcpNG, q, r);
    return r;
  }
  __device__ __forceinline__ bool has(u32 w) const { return (int)w >= lo && (int)w < hi; }
};

// The row-side lanes: position v of the row image <-> granule g of row w, moved between the image and the rows.
template <typename E, bool TO_IMAGE, int TT>
__device__ __forceinline__ void split_rows_linear(const SplitTile<E>& t, int lane) {
  constexpr int X = 16 / (int)sizeof(E);
#pragma unroll 1
  for (u32 v0 = 0; v0 < t.NV; v0 += 256u) {
    uint4 val[4];
    bool on[4];
    const E* ptr[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const u32 v = v0 + 64u * u + (u32)lane;
      u32 w, c;
      split_divmod(v, t.NG, t.rcpNG, w, c);
      on[u] = v < t.NV && t.has(w);
      const long long ro = __shfl(t.roff, on[u] ? (int)w : 0);
      ptr[u] = t.rw + ro + (long long)split_submod(c, t.rotm(on[u] ? w : 0u), t.NG) * X;
      if (on[u]) val[u] = TO_IMAGE ? ld_global_u4_nt(reinterpret_cast<const u16*>(ptr[u])) : t.img[v];
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      if (!on[u]) continue;
      if constexpr (TO_IMAGE) t.img[v0 + 64u * u + (u32)lane] = val[u];
      else st_global_u4(reinterpret_cast<u16*>(const_cast<E*>(ptr[u])), val[u]);
    }
  }
}

// K, split-side lanes of a gather: granule (g = v / TT, w = v % TT) -> the row image at Pg(w, g).
template <typename E, int TT>
__device__ __forceinline__ void split_k_to_rows_image(const SplitTile<E>& t, int lane) {
  constexpr int X = 16 / (int)sizeof(E);
#pragma unroll 1
  for (u32 v0 = 0; v0 < t.NV; v0 += 256u) {
    uint4 val[4];
    bool on[4];
    u32 pos[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const u32 v = v0 + 64u * u + (u32)lane, g = v / TT, w = v % TT;
      on[u] = v < t.NV && t.has(w);
      pos[u] = w * t.NG + split_addmod(on[u] ? g : 0u, t.rotm(w), t.NG);
      if (on[u]) val[u] = ld_global_u4_nt(reinterpret_cast<const u16*>(t.sp + (long long)g * (t.bs * X) + w * X));
    }
#pragma unroll
    for (int u = 0; u < 4; u++)
      if (on[u]) t.img[pos[u]] = val[u];
  }
}

// K scatter.  Row-side lanes: granule (w = v / NG, g = v % NG) -> the split image at Ps(g, w); then the split-side lanes:
// position v = (g = v / TT, column (w + g) mod TT) -> the cache.
template <typename E, int TT>
__device__ __forceinline__ void split_k_rows_to_split_image(const SplitTile<E>& t, int lane) {
  constexpr int X = 16 / (int)sizeof(E);
#pragma unroll 1
  for (u32 v0 = 0; v0 < t.NV; v0 += 256u) {
    uint4 val[4];
    bool on[4];
    u32 pos[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const u32 v = v0 + 64u * u + (u32)lane;
      u32 w, g;
      split_divmod(v, t.NG, t.rcpNG, w, g);
      on[u] = v < t.NV && t.has(w);
      const long long ro = __shfl(t.roff, on[u] ? (int)w : 0);
      pos[u] = g * TT + ((w + g) & (u32)(TT - 1));
      if (on[u]) val[u] = ld_global_u4_nt(reinterpret_cast<const u16*>(t.rw + ro + (long long)g * X));
    }
#pragma unroll
    for (int u = 0; u < 4; u++)
      if (on[u]) t.img[pos[u]] = val[u];
  }
}
template <typename E, int TT>
__device__ __forceinline__ void split_k_from_split_image(const SplitTile<E>& t, int lane) {
  constexpr int X = 16 / (int)sizeof(E);
#pragma unroll 1
  for (u32 v0 = 0; v0 < t.NV; v0 += 256u) {
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const u32 v = v0 + 64u * u + (u32)lane, g = v / TT, w = ((v % TT) - g) & (u32)(TT - 1);
      if (v < t.NV && t.has(w))
        st_global_u4(reinterpret_cast<u16*>(const_cast<E*>(t.sp) + (long long)g * (t.bs * X) + w * X), t.img[v]);
    }
  }
}

// V, split-side lanes: granule (channel d = v / GPR, part = v % GPR) holds tokens part * X .. + X - 1 of channel d, which
// are the single elements Pg(part * X + k, d / X) * X + d % X of the row image.  rot(part * X + k) = A(part) + B(k) with
// B wave-uniform (k is unrolled): one division per granule.
template <typename E, bool GATHER, int TT>
__device__ __forceinline__ void split_v_elements(const SplitTile<E>& t, int lane) {
  constexpr int X = 16 / (int)sizeof(E);
  constexpr int GPR = TT / X > 0 ? TT / X : 1;
  constexpr int U = GATHER ? 4 : 2;
  E* const img_e = reinterpret_cast<E*>(t.img);
  u32 bm[X];
#pragma unroll
  for (int k = 0; k < X; k++) {
    u32 q;
    split_divmod((t.rot_w ? (u32)k : 0u) + ((u32)k >> 3), t.NG, t.rcpNG, q, bm[k]);
  }
#pragma unroll 1
  for (u32 v0 = 0; v0 < t.NV; v0 += 64u * U) {
    uint4 val[U];
    bool on[U];
    u32 col[U], d_[U], part_[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const u32 v = v0 + 64u * u + (u32)lane, d = v / GPR, part = v % GPR;
      const int t0 = (int)(part * X);
      on[u] = v < t.NV && t0 < t.hi && t0 + X > t.lo;
      u32 q, am;
      split_divmod((t.rot_w ? part * X : 0u) + part * (X / 8), t.NG, t.rcpNG, q, am);
      col[u] = split_addmod(on[u] ? d / X : 0u, am, t.NG);
      d_[u] = d; part_[u] = part;
      if constexpr (GATHER) {
        if (on[u]) val[u] = ld_global_u4_nt(reinterpret_cast<const u16*>(t.sp + (long long)d * t.bs + t0));
      }
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      if (!on[u]) continue;
      const u32 row0 = part_[u] * X, sub = d_[u] % X;
      if constexpr (GATHER) {
#pragma unroll
        for (int k = 0; k < X; k++) img_e[((row0 + k) * t.NG + split_addmod(col[u], bm[k], t.NG)) * X + sub] = split_elem<E>(val[u], k);
      } else {
        E e[X];
#pragma unroll
        for (int k = 0; k < X; k++) e[k] = img_e[((row0 + k) * t.NG + split_addmod(col[u], bm[k], t.NG)) * X + sub];
        E* const dp = const_cast<E*>(t.sp) + (long long)d_[u] * t.bs + row0;
        if ((int)row0 >= t.lo && (int)row0 + X <= t.hi) st_global_u4(reinterpret_cast<u16*>(dp), split_pack<E>(e));
        else {  // a granule that also holds slots of other sequences: the given slots only
#pragma unroll
          for (int k = 0; k < X; k++)
            if (t.has(row0 + k)) dp[k] = e[k];
        }
      }
    }
  }
}

template <typename E, bool GATHER, int TT>
__global__ __launch_bounds__(64 * SPLIT_WAVES) void k_copy_split(SplitCopyArgs a) {
  extern __shared__ uint4 split_lds[];
  constexpr int X = 16 / (int)sizeof(E);
  constexpr bool V_VEC = TT >= X;  // V: a tile's run of one channel is at least one granule
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int D = a.sp.D, H = a.sp.H;
  const u32 bs = (u32)a.sp.block_size;
  SplitTile<E> t;
  t.NG = (u32)D / X; t.NV = TT * t.NG; t.bs = bs;
  t.rcpNG = 1.0f / (float)t.NG;
  t.rot_w = (t.NG & 1u) == 0u;
  t.img = split_lds + (size_t)wv * t.NV;  // (only touched when a.fast)
  const int off0 = (int)((u32)a.sp.slot_mapping[a.sp_tok0] % (u32)TT);
  const long long nitems = (long long)a.P * a.ntiles * H;

  for (long long it = (long long)blockIdx.x * SPLIT_WAVES + wv; it < nitems; it += (long long)gridDim.x * SPLIT_WAVES) {
    const int h = (int)(it % H);
    const long long q = it / H;
    const int tile = (int)(q % a.ntiles), p = (int)(q / a.ntiles);
    const int r0 = tile * TT - off0;  // range token of tile position 0
    const int lo = r0 < 0 ? -r0 : 0, hi = a.ntok - r0 < TT ? a.ntok - r0 : TT;
    if (hi <= lo) continue;
    const bool is_k = p < a.sp.L;
    const E* const sp_base = lmc_plane_base<E>(a.sp, p) + (long long)h * a.sp.stride_head;
    const E* const rw_base = lmc_plane_base<E>(a.rw, p) + (long long)h * a.rw.stride_head;

    // lane l < TT: slot and row offset of tile position l
    const bool tv = lane >= lo && lane < hi;
    const u32 s = tv ? (u32)a.sp.slot_mapping[a.sp_tok0 + r0 + lane] : 0u;
    const long long roff = tv ? lmc_tok_off(a.rw, a.rw_tok0 + r0 + lane) : 0ll;
    const u32 s_first = (u32)__shfl((int)s, lo);
    const u32 slot0 = s_first - (u32)lo;  // slot of tile position 0 if the tile is one run
    const u32 blk = slot0 / bs, w0 = slot0 - blk * bs;
    bool fast = a.fast != 0 && s_first >= (u32)lo && w0 + (u32)TT <= bs &&
                ((((uintptr_t)sp_base) | ((uintptr_t)rw_base)) & 15u) == 0u &&
                __ballot(tv && s != slot0 + (u32)lane) == 0ull;
    if (!is_k) fast = fast && V_VEC && (w0 % X) == 0u && (bs % X) == 0u;

    if (fast) {
      t.sp = sp_base + (long long)blk * a.sp.stride_block + (is_k ? (long long)w0 * X : (long long)w0);
      t.rw = rw_base; t.roff = roff; t.lo = lo; t.hi = hi;
      if constexpr (GATHER) {
        if (is_k) split_k_to_rows_image<E, TT>(t, lane);
        else split_v_elements<E, true, TT>(t, lane);
        wave_lds_fence();
        split_rows_linear<E, false, TT>(t, lane);
      } else {
        if (is_k) split_k_rows_to_split_image<E, TT>(t, lane);
        else split_rows_linear<E, true, TT>(t, lane);
        wave_lds_fence();
        if (is_k) split_k_from_split_image<E, TT>(t, lane);
        else split_v_elements<E, false, TT>(t, lane);
      }
      wave_lds_fence();  // the next item's writes come after these reads
      continue;
    }

    // element path: lane = (tile position, channel), a token's slot and row from the lane that holds them
    const u32 ne = (u32)TT * (u32)D;
    for (u32 i0 = 0; i0 < ne; i0 += 64u) {
      const u32 i = i0 + (u32)lane;
      const bool in = i < ne;
      const u32 w = in ? i / (u32)D : 0u, d = i - (i / (u32)D) * (u32)D;
      const u32 sw = (u32)__shfl((int)s, (int)w);
      const long long ro = __shfl(roff, (int)w);
      if (!in || (int)w < lo || (int)w >= hi) continue;
      const u32 b = sw / bs, ws = sw - b * bs;
      const long long so = (long long)b * a.sp.stride_block +
                           (is_k ? (long long)(d / X) * (bs * X) + (long long)ws * X + d % X : (long long)d * bs + ws);
      if constexpr (GATHER) const_cast<E*>(rw_base)[ro + d] = sp_base[so];
      else const_cast<E*>(sp_base)[so] = rw_base[ro + d];
    }
  }
}
