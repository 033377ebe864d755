// k_blend.h -- CacheBlend token selection: per-token KV deviation between two layouts, and a deterministic top-k.
//
// Stands where a CacheBlend executor on the connector side gathers the cached KV of the check layer by slot mapping,
// subtracts the fresh KV, squares, sums over (head, channel), runs torch.topk (tie order unspecified) and sorts: a gather
// per cache layout, three element-wise passes with temporaries the size of the layer's KV, and a selection.  Here:
// one read of both sides (k_kv_deviation), one workgroup that selects (k_select_topk).  The reference has neither.
//
// k_kv_deviation: out[i] = sum over (h, d) of (A(a_tok0 + i, h, d) - B(b_tok0 + i, h, d))^2 for one plane of each side.
// Elements are widened exactly to fp32; difference, square and sum are fp32 (the square and the add may contract into one
// fma, which only removes a rounding).  No float atomics: a token belongs to one wave, its partial sums meet in the wave's
// lanes in an order the code fixes, and one lane stores the sum -- the same bits on every run.
//
// Two forms, an instance each (the host launches the tile form for a V plane with a split side, the group form otherwise):
//   GROUP form (any two layouts): LPT lanes share a token (LPT = the power of two that covers the plane's C / 8 runs of 8
//     channels, at most 64), a wave takes 64 / LPT consecutive tokens.  A lane loads run j of its token from both sides and
//     goes on to run j + LPT.  How a side hands over 8 channels (dev_ld8):
//       rows, vector-addressable (lmc_copy_kv's `vec` rule, plane base on a 16-byte boundary)   one 16-byte load
//       rows, anything else (odd strides, head_size % 8 with the heads apart, a base 2 bytes off) eight element loads
//       split K   the run is one x-granule of the token: one 16-byte load (strides multiples of 8, aligned base), else 8
//       split V   eight elements block_size apart
//     The LPT lanes fold their sums with xor-shuffles; lane 0 of the group stores.
//   TILE form (a V plane with one LMC_PAGED_SPLIT side): a wave takes a tile of 8 consecutive tokens, the tiles anchored at
//     the first token's slot % 8 as in k_copy_split.h, so that the tiles of a block-ordered mapping are eight consecutive
//     slots from slot % 8 == 0 on.  A whole tile that is such a run (k_fixed_decode's run condition) is read as the cache
//     holds it: lane = channel, ONE 16-byte load brings that channel of all eight tokens, the row side gives the same
//     eight values as eight 2-byte loads (64 lanes = 128 contiguous bytes of a token row each), and the lane keeps eight
//     sums, one per token.  They are folded by a reduce-scatter (4 + 2 + 1 exchanges halve what a lane holds, three more
//     finish a token: 10 exchanges for 8 tokens).  Any other tile -- the range's ragged ends, random slots, a run that
//     enters a block at offset 5, an unaligned base -- goes token by token through dev_ld8: correct, slow.
// A slot is read from slot_mapping only for a token of the range.  Plane, block and token offsets are 64-bit.
#pragma once
#include "lmc_device.h"

#define BLEND_WAVES 4

struct DevSide {
  KvAddr kv;
  int tok0, plane_k, plane_v;  // the two planes of the side's layer (p = kv * L + layer)
  int vec;                     // host: every stride lets the side be read 16 bytes at a time (the kernel adds the base)
  int split;                   // LMC_PAGED_SPLIT
};
struct DeviationArgs {
  DevSide a, b;
  int ntok, C;
  int lpt;          // GROUP form: lanes per token
  int ntiles;       // TILE form: an upper bound of the 8-token tiles the range touches
  int nplanes;      // grid.y
  int plane_kv[2];  // grid.y -> 0 (K) / 1 (V)
  float* out[2];    // dev_k, dev_v
};

// One side's plane as the lanes address it.
struct DevPlane {
  const u16* pb;
  long long stride_head, stride_block;
  u32 D, bs;
  bool vec, split, is_k;
};
__device__ __forceinline__ DevPlane dev_plane(const DevSide& s, int kv) {
  DevPlane p;
  p.pb = lmc_plane_base(s.kv, kv ? s.plane_v : s.plane_k);
  p.stride_head = s.kv.stride_head; p.stride_block = s.kv.stride_block;
  p.D = (u32)s.kv.D; p.bs = (u32)s.kv.block_size;
  p.split = s.split != 0; p.is_k = kv == 0;
  p.vec = s.vec != 0 && (((uintptr_t)p.pb) & 15u) == 0u;
  return p;
}
// Where token t of a side begins: rows -- its row; split -- its block, and w = its slot in the block.
__device__ __forceinline__ long long dev_tok(const DevSide& s, int t, u32& w) {
  if (!s.split) { w = 0; return lmc_tok_off(s.kv, t); }
  const u32 slot = (u32)s.kv.slot_mapping[t], bs = (u32)s.kv.block_size, b = slot / bs;
  w = slot - b * bs;
  return (long long)b * s.kv.stride_block;
}
__device__ __forceinline__ uint4 dev_pack8(const u32 (&e)[8]) {
  return make_uint4(e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16));
}
// Channels c0 .. c0 + 7 (c0 % 8 == 0) of the token at (toff, w).
__device__ __forceinline__ uint4 dev_ld8(const DevPlane& p, long long toff, u32 w, u32 c0) {
  u32 e[8];
  if (!p.split) {
    if (p.vec) {
      const u32 h = c0 / p.D, d = c0 - h * p.D;
      return ld_global_u4_nt(p.pb + toff + (long long)h * p.stride_head + d);
    }
#pragma unroll
    for (u32 k = 0; k < 8; k++) {
      const u32 c = c0 + k, h = c / p.D, d = c - h * p.D;
      e[k] = p.pb[toff + (long long)h * p.stride_head + d];
    }
    return dev_pack8(e);
  }
  const u32 h = c0 / p.D, d0 = c0 - h * p.D;  // head_size % 8 == 0: the run is one granule of one head
  const u16* q = p.pb + toff + (long long)h * p.stride_head;
  if (p.is_k) {
    q += (long long)(d0 >> 3) * (p.bs * 8u) + (long long)w * 8;
    if (p.vec) return ld_global_u4_nt(q);
#pragma unroll
    for (u32 k = 0; k < 8; k++) e[k] = q[k];
  } else {
    q += (long long)d0 * p.bs + w;
#pragma unroll
    for (u32 k = 0; k < 8; k++) e[k] = q[(long long)k * p.bs];
  }
  return dev_pack8(e);
}
template <int DT>
__device__ __forceinline__ float dev_sq(float acc, float x, float y) {
  const float d = x - y;
  return __builtin_fmaf(d, d, acc);
}
template <int DT>
__device__ __forceinline__ float dev_sq8(float acc, const uint4& x, const uint4& y) {
  const u32 xw[4] = {x.x, x.y, x.z, x.w}, yw[4] = {y.x, y.y, y.z, y.w};
#pragma unroll
  for (int k = 0; k < 4; k++) {
    acc = dev_sq<DT>(acc, h_lo<DT>(xw[k]), h_lo<DT>(yw[k]));
    acc = dev_sq<DT>(acc, h_hi<DT>(xw[k]), h_hi<DT>(yw[k]));
  }
  return acc;
}
__device__ __forceinline__ float dev_wave_sum(float v, int lanes) {  // over aligned groups of `lanes` lanes (a power of two)
  for (int off = lanes >> 1; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// TILE: the instance of a V plane with a split side; the other instance is the group form alone, which needs a third of
// the registers and so keeps twice the waves resident (a wave is a chain of dependent loads: occupancy is its rate).
template <int DT, bool TILE>
__global__ __launch_bounds__(64 * BLEND_WAVES) void k_kv_deviation(DeviationArgs g) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int kv = g.plane_kv[blockIdx.y];
  float* const out = g.out[kv];
  const DevPlane pa = dev_plane(g.a, kv), pb = dev_plane(g.b, kv);
  const u32 C8 = (u32)g.C >> 3;

  if constexpr (!TILE) {  // GROUP form
    const int lpt = g.lpt, tpw = 64 / lpt;
    const u32 j0 = (u32)(lane & (lpt - 1));
    const long long nitems = ((long long)g.ntok + tpw - 1) / tpw;
    for (long long it = (long long)blockIdx.x * BLEND_WAVES + wv; it < nitems; it += (long long)gridDim.x * BLEND_WAVES) {
      const long long t = it * tpw + lane / lpt;
      const bool on = t < g.ntok;
      float acc = 0.f;
      if (on) {
        u32 wa, wb;
        const long long oa = dev_tok(g.a, g.a.tok0 + (int)t, wa), ob = dev_tok(g.b, g.b.tok0 + (int)t, wb);
        for (u32 j = j0; j < C8; j += (u32)lpt) acc = dev_sq8<DT>(acc, dev_ld8(pa, oa, wa, j * 8u), dev_ld8(pb, ob, wb, j * 8u));
      }
      acc = dev_wave_sum(acc, lpt);
      if (on && j0 == 0u) out[t] = acc;
    }
  } else {
  // TILE form: the split side is b, the rows are a (the host swaps the sides if need be: (x - y)^2 = (y - x)^2 exactly)
  const DevSide& sp = g.b;
  const DevSide& rw = g.a;
  const DevPlane& psp = pb;
  const DevPlane& prw = pa;
  const u32 bs = psp.bs;
  const bool runs = psp.vec && (bs & 7u) == 0u;  // a run of eight slots from slot % 8 == 0 on is 16 aligned bytes of a channel
  const int off0 = (int)((u32)sp.kv.slot_mapping[sp.tok0] & 7u);
  for (long long it = (long long)blockIdx.x * BLEND_WAVES + wv; it < g.ntiles; it += (long long)gridDim.x * BLEND_WAVES) {
    const int r0 = (int)it * 8 - off0;  // range token of tile position 0
    const int lo = r0 < 0 ? -r0 : 0, hi = g.ntok - r0 < 8 ? g.ntok - r0 : 8;
    if (hi <= lo) continue;
    // lane l < 8: slot and row offset of tile position l
    const bool tv = lane >= lo && lane < hi;
    const u32 s = tv ? (u32)sp.kv.slot_mapping[sp.tok0 + r0 + lane] : 0u;
    const long long roff = tv ? lmc_tok_off(rw.kv, rw.tok0 + r0 + lane) : 0ll;
    const u32 s_first = (u32)__shfl((int)s, lo);
    const bool fast = runs && lo == 0 && hi == 8 && (s_first & 7u) == 0u && __ballot(tv && s != s_first + (u32)lane) == 0ull;
    if (fast) {
      const u32 blk = s_first / bs, w0 = s_first - blk * bs;
      const u16* const spt = psp.pb + (long long)blk * psp.stride_block + w0;
      long long ro[8];
#pragma unroll
      for (int k = 0; k < 8; k++) ro[k] = __shfl(roff, k);
      float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      for (u32 c = (u32)lane; c < (u32)g.C; c += 64u) {
        const u32 h = c / psp.D, d = c - h * psp.D;
        const uint4 v = ld_global_u4_nt(spt + (long long)h * psp.stride_head + (long long)d * bs);
        const u16* const rp = prw.pb + (long long)h * prw.stride_head + d;
        const u32 vw[4] = {v.x, v.y, v.z, v.w};
        u32 r[8];
#pragma unroll
        for (int k = 0; k < 8; k++) r[k] = rp[ro[k]];
#pragma unroll
        for (int k = 0; k < 4; k++) {
          acc[2 * k] = dev_sq<DT>(acc[2 * k], h_lo<DT>(vw[k]), h_lo<DT>(r[2 * k]));
          acc[2 * k + 1] = dev_sq<DT>(acc[2 * k + 1], h_hi<DT>(vw[k]), h_lo<DT>(r[2 * k + 1]));
        }
      }
      // reduce-scatter: lanes with bit 5 set keep tokens 4 .. 7, then bit 4 picks the pair, bit 3 the token
      const bool b5 = (lane & 32) != 0, b4 = (lane & 16) != 0, b3 = (lane & 8) != 0;
      float q[4], p2[2];
#pragma unroll
      for (int k = 0; k < 4; k++) q[k] = (b5 ? acc[4 + k] : acc[k]) + __shfl_xor(b5 ? acc[k] : acc[4 + k], 32);
#pragma unroll
      for (int k = 0; k < 2; k++) p2[k] = (b4 ? q[2 + k] : q[k]) + __shfl_xor(b4 ? q[k] : q[2 + k], 16);
      float tot = (b3 ? p2[1] : p2[0]) + __shfl_xor(b3 ? p2[0] : p2[1], 8);
      tot = dev_wave_sum(tot, 8);
      if ((lane & 7) == 0) out[r0 + ((lane >> 5) & 1) * 4 + ((lane >> 4) & 1) * 2 + ((lane >> 3) & 1)] = tot;
      continue;
    }
    for (int w = lo; w < hi; w++) {  // token by token, the wave's lanes over the runs of 8 channels
      const u32 sw = (u32)__shfl((int)s, w);
      const long long row = __shfl(roff, w);
      const u32 blk = sw / bs, ws = sw - blk * bs;
      const long long so = (long long)blk * psp.stride_block;
      float acc = 0.f;
      for (u32 j = (u32)lane; j < C8; j += 64u) acc = dev_sq8<DT>(acc, dev_ld8(psp, so, ws, j * 8u), dev_ld8(prw, row, 0u, j * 8u));
      acc = dev_wave_sum(acc, 64);
      if (lane == 0) out[r0 + w] = acc;
    }
  }
  }
}

// k_select_topk: the kk = min(k, n) indices with the largest key, key = bits(dev[i]) & 0x7fffffff compared as unsigned
// (the float order of non-negative values; NaN above +inf), ties to the lower index, written in ascending order.
// ONE workgroup.  Four passes of an 8-bit radix select, most significant digit first: a histogram in LDS (integer atomics:
// the counts do not depend on their order) of the keys that match the digits found so far, then wave 0 walks the 256
// bins from the top -- four bins a lane, a prefix sum over the lanes -- to the bin that holds the kk-th largest key and
// keeps how many keys are still wanted inside it.  After the last digit: the threshold key T and the quota of keys == T.
// A fifth pass in index order writes: a token is taken when key > T, or key == T and fewer than quota such keys precede
// it; its place is (keys > T before it) + min(keys == T before it, quota) -- ballots and lane ranks inside a wave, the
// waves' counts through LDS, the tiles' totals carried in a register.  Nothing is written beyond idx_out[kk - 1].
#define TOPK_THREADS 1024
#define TOPK_WAVES (TOPK_THREADS / 64)

struct TopkArgs {
  const float* dev;
  int* idx_out;
  u32 n, kk;  // 1 <= kk <= n
};

__global__ __launch_bounds__(TOPK_THREADS) void k_select_topk(TopkArgs a) {
  __shared__ u32 hist[256];
  __shared__ u32 wave_cnt[2][TOPK_WAVES][2];
  __shared__ u32 sh_prefix, sh_want;
  const u32 tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
  const u32* const keys = reinterpret_cast<const u32*>(a.dev);
  if (tid == 0) { sh_prefix = 0u; sh_want = a.kk; }

  for (int pass = 0; pass < 4; pass++) {
    const u32 shift = 24u - 8u * (u32)pass;
    const u32 himask = pass ? 0xffffffffu << (shift + 8u) : 0u;
    if (tid < 256u) hist[tid] = 0u;
    __syncthreads();
    const u32 prefix = sh_prefix;
    for (u32 i0 = 0; i0 < a.n; i0 += TOPK_THREADS) {
      const u32 i = i0 + tid;
      const u32 key = i < a.n ? keys[i] & 0x7fffffffu : 0u;
      const bool in = i < a.n && (key & himask) == prefix;
      const u32 digit = (key >> shift) & 255u;
      const u64 m = __ballot(in);
      if (m == 0ull) continue;
      // keys of one magnitude share their upper digits: a wave whose digits are all one bin adds its count once
      const u32 first = (u32)__builtin_amdgcn_readlane((int)digit, (int)__builtin_ctzll(m));
      if (__ballot(in && digit != first) == 0ull) {
        if (lane == 0u) atomicAdd(&hist[first], (u32)__builtin_popcountll(m));
      } else if (in) atomicAdd(&hist[digit], 1u);
    }
    __syncthreads();
    if (wv == 0u) {
      const u32 want = sh_want, top = 255u - 4u * lane;  // this lane's bins: top, top - 1, top - 2, top - 3
      u32 c[4];
#pragma unroll
      for (u32 j = 0; j < 4; j++) c[j] = hist[top - j];
      const u32 tot = c[0] + c[1] + c[2] + c[3];
      u32 inc = tot;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const u32 t = (u32)__shfl_up((int)inc, off);
        if ((int)lane >= off) inc += t;
      }
      const u32 exc = inc - tot;
      if (exc < want && want <= inc) {  // one lane: 1 <= want <= the keys that match
        u32 r = want - exc, bin = top;
#pragma unroll
        for (u32 j = 0; j < 3; j++)
          if (bin == top - j && r > c[j]) { r -= c[j]; bin = top - j - 1u; }
        sh_prefix = prefix | (bin << shift);
        sh_want = r;
      }
    }
    __syncthreads();
  }

  const u32 T = sh_prefix, quota = sh_want;
  u32 gt_base = 0u, eq_base = 0u;  // keys > T / == T in front of the tile
  u32 par = 0u;
  for (u32 i0 = 0; i0 < a.n; i0 += TOPK_THREADS, par ^= 1u) {
    const u32 i = i0 + tid;
    const u32 key = i < a.n ? keys[i] & 0x7fffffffu : 0u;
    const bool gt = i < a.n && key > T, eq = i < a.n && key == T;
    const u64 mg = __ballot(gt), me = __ballot(eq);
    if (lane == 0u) { wave_cnt[par][wv][0] = (u32)__builtin_popcountll(mg); wave_cnt[par][wv][1] = (u32)__builtin_popcountll(me); }
    __syncthreads();  // (the other parity's words were last read before the previous tile's barrier)
    u32 gt_w = 0u, eq_w = 0u, gt_t = 0u, eq_t = 0u;
#pragma unroll
    for (u32 w = 0; w < TOPK_WAVES; w++) {
      const u32 cg = wave_cnt[par][w][0], ce = wave_cnt[par][w][1];
      if (w < wv) { gt_w += cg; eq_w += ce; }
      gt_t += cg; eq_t += ce;
    }
    const u32 gt_before = gt_base + gt_w + lane_rank(mg), eq_before = eq_base + eq_w + lane_rank(me);
    if (gt || (eq && eq_before < quota)) a.idx_out[gt_before + (eq_before < quota ? eq_before : quota)] = (int)i;
    gt_base += gt_t; eq_base += eq_t;
  }
}
