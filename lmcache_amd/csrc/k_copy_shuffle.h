// k_copy_shuffle.h -- gather / scatter between AITER's shuffled paged KV cache (LMC_PAGED_SHUFFLE, include/lmc_hip.h)
// and any layout of rows (a chunk, per-layer tensors, NBHD / NHBD blocks).
//
// Per block b and head h the shuffled layout keeps one dense run of D * block_size elements, X = 16 / element bytes:
//   K(b, h, d, w) = b * stride_block + h * stride_head + (d / X) * (block_size * X) + w * X + d % X
//   V(b, h, d, w) = b * stride_block + h * stride_head + (w / X) * (D * X) + d * X + w % X
// K is byte for byte LMC_PAGED_SPLIT's key cache: its tiles go through k_copy_split.h's K functions, nothing of them is
// repeated here.  V is a sequence of [D][X] tiles, one per X consecutive slots: the 16-byte granule at element
// (w / X) * D * X + d * X holds channel d of X tokens, and TT consecutive slots from slot % X == 0 on are ONE run of
// TT * D contiguous elements (LMC_PAGED_SPLIT's value cache has 16-byte runs block_size elements apart there).
//
// Work item of ONE WAVE, as in k_copy_split.h: (plane, head, tile of TT consecutive tokens of the range); TT is the
// largest of 32 / 16 / 8 that divides block_size and is a multiple of X (the host's choice; block_size % X == 0 is the
// layout's rule, so there is one), the tiles anchored at the slot of the range's first token (off0 = that slot % TT).
//
// FAST tile (per tile, wave-uniform: one ballot): k_copy_split.h's conditions -- the tile is one run of slots inside one
// block, both plane bases on 16-byte boundaries, every stride a multiple of X (host) -- and for V a run that begins at
// slot % X == 0 (every tile of a block-ordered mapping does: slot % TT == 0).  Both sides move 16 bytes per lane and
// the [D][X] <-> [X][D] element transposition happens in the LDS ROW image of the tile that k_copy_split.h defines
// (NV = TT * NG granules, NG = D / X per row, row w's granule g at Pg(w, g) = w * NG + (g + rot(w)) mod NG):
//   cache side  lane = linear position: granule v of the run is channel d = v % D of token group part = v / D.  A wave
//               access covers 1 KB of contiguous cache; the loads are non-temporal.  The lane writes (gather) or reads
//               (scatter) its X tokens as X single elements of the image, element d % X of granule Pg(part * X + k, d / X).
//   row side    split_rows_linear: lane = image position, whole granules, NG lanes cover a row's D elements.
// LDS banks, under the rules k_copy_split.h states for MI355X (narrow accesses: two groups of 32 lanes over 32 banks).
// In the single-element phase the 32 lanes of a group hold 32 CONSECUTIVE channels of one token group (v % D), so for a
// given k they touch one image row: 32 consecutive elements of it, rotated as a whole by rot(w) granules -- 16 dwords
// (2-byte elements, two lanes a dword, which count as one address) or 8 (1-byte) that are consecutive modulo the row.
// Consecutive dwords lie in different banks; the wrap at the row's end can bring the run's tail onto banks of its head
// only when the row is no multiple of 32 dwords (D = 80: 40 dwords), and a group that crosses from one token group into
// the next (D % 32 != 0) touches two rows: two-way at worst in both cases, conflict free for D = 64 / 128 / 256.
// tools/probes/split_lds_banks.py enumerates this phase beside k_copy_split.h's four, for every D from NG = 4 up to 512,
// both element sizes and TT 8 / 16 / 32: conflict free for 164 of the 209 geometries, two-way for the other 45, never
// more (k_copy_split.h's V phase: 128 and 81).  The rotation is not needed by this phase; it is kept because it costs
// this phase nothing (whole granules move) and the K phases and split_rows_linear are shared as they are.  The linear
// phase is lane = position: conflict free.
//
// LDS, not registers: an 8 x 8 transpose across 8 lanes (DPP / ds_bpermute) leaves every lane with one granule of a
// DIFFERENT row -- per 8 lanes eight 16-byte row accesses stride_token apart -- where the image hands a row's D elements
// to NG neighbouring lanes (D = 128, bf16: 256 contiguous bytes per row).  The transpose itself is three exchange stages
// over a granule's four dwords plus the 16-bit repacking, against X narrow LDS accesses that are conflict free here, and
// for 1-byte elements it is 16 x 16 across 16 lanes.  The image also keeps the row side in common with the K planes.
//
// Any other tile -- random slots, a run that enters a block off a TT boundary, a ragged tile whose run is broken, an
// unaligned base, a geometry the host ruled out -- is copied element by element from the formulas: correct, slow.
// A scatter writes only elements of the slots it was given: a V granule whose X tokens are all in the range is stored
// as 16 bytes, any other element by element.  Block and plane offsets are 64-bit.
#pragma once
#include "k_copy_split.h"

// V, cache-side lanes of a fast tile: granule v = (part = v / D, d = v % D) at t.sp + v * X  <->  the single elements
// Pg(part * X + k, d / X) * X + d % X of the row image.  rot(part * X + k) = A(part) + B(k) as in split_v_elements.
template <typename E, bool GATHER, int TT>
__device__ __forceinline__ void shuffle_v_elements(const SplitTile<E>& t, u32 D, float rcpD, int lane) {
  constexpr int X = 16 / (int)sizeof(E);
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
    u32 col[U], sub[U], row0[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const u32 v = v0 + 64u * u + (u32)lane;
      u32 part, d;
      split_divmod(v, D, rcpD, part, d);  // (v < NV + 256 <= 2048, D >= 4 * X: split_divmod's range)
      const int t0 = (int)(part * X);
      on[u] = v < t.NV && t0 < t.hi && t0 + X > t.lo;
      u32 q, am;
      split_divmod((t.rot_w ? part * X : 0u) + part * (X / 8), t.NG, t.rcpNG, q, am);
      col[u] = split_addmod(on[u] ? d / X : 0u, am, t.NG);
      sub[u] = d % X; row0[u] = part * X;
      if constexpr (GATHER) {
        if (on[u]) val[u] = ld_global_u4_nt(reinterpret_cast<const u16*>(t.sp + (long long)v * X));
      }
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      if (!on[u]) continue;
      if constexpr (GATHER) {
#pragma unroll
        for (int k = 0; k < X; k++)
          img_e[((row0[u] + k) * t.NG + split_addmod(col[u], bm[k], t.NG)) * X + sub[u]] = split_elem<E>(val[u], k);
      } else {
        E e[X];
#pragma unroll
        for (int k = 0; k < X; k++) e[k] = img_e[((row0[u] + k) * t.NG + split_addmod(col[u], bm[k], t.NG)) * X + sub[u]];
        E* const dp = const_cast<E*>(t.sp) + (long long)(v0 + 64u * u + (u32)lane) * X;
        if ((int)row0[u] >= t.lo && (int)row0[u] + X <= t.hi) st_global_u4(reinterpret_cast<u16*>(dp), split_pack<E>(e));
        else {  // a granule that also holds slots of other sequences: the given slots only
#pragma unroll
          for (int k = 0; k < X; k++)
            if (t.has(row0[u] + k)) dp[k] = e[k];
        }
      }
    }
  }
}

// `a.sp` is the shuffled side.  TT % X == 0 (the host launches no other instance).
template <typename E, bool GATHER, int TT>
__global__ __launch_bounds__(64 * SPLIT_WAVES) void k_copy_shuffle(SplitCopyArgs a) {
  extern __shared__ uint4 split_lds[];
  constexpr int X = 16 / (int)sizeof(E);
  static_assert(TT % X == 0, "a tile is whole [D][X] groups");
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int D = a.sp.D, H = a.sp.H;
  const u32 bs = (u32)a.sp.block_size;
  const float rcpD = 1.0f / (float)D;
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
    const bool fast = a.fast != 0 && s_first >= (u32)lo && w0 + (u32)TT <= bs && (is_k || (w0 % X) == 0u) &&
                      ((((uintptr_t)sp_base) | ((uintptr_t)rw_base)) & 15u) == 0u &&
                      __ballot(tv && s != slot0 + (u32)lane) == 0ull;

    if (fast) {
      // K: the run's first granule of d / X = 0; V: the run's first [D][X] group
      t.sp = sp_base + (long long)blk * a.sp.stride_block + (is_k ? (long long)w0 * X : (long long)(w0 / X) * ((long long)D * X));
      t.rw = rw_base; t.roff = roff; t.lo = lo; t.hi = hi;
      if constexpr (GATHER) {
        if (is_k) split_k_to_rows_image<E, TT>(t, lane);
        else shuffle_v_elements<E, true, TT>(t, (u32)D, rcpD, lane);
        wave_lds_fence();
        split_rows_linear<E, false, TT>(t, lane);
      } else {
        if (is_k) split_k_rows_to_split_image<E, TT>(t, lane);
        else split_rows_linear<E, true, TT>(t, lane);
        wave_lds_fence();
        if (is_k) split_k_from_split_image<E, TT>(t, lane);
        else shuffle_v_elements<E, false, TT>(t, (u32)D, rcpD, lane);
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
                           (is_k ? (long long)(d / X) * (bs * X) + (long long)ws * X + d % X
                                 : (long long)(ws / X) * ((long long)D * X) + (long long)d * X + ws % X);
      if constexpr (GATHER) const_cast<E*>(rw_base)[ro + d] = sp_base[so];
      else const_cast<E*>(sp_base)[so] = rw_base[ro + d];
    }
  }
}
