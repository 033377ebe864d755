// k_quantize.h -- fused |x| row-max + quantise.
//
// Replaces _split_kv + torch_quant_vectorized + torch.cat
// (lmcache/storage_backend/serde/cachegen_encoder.py:40-61, 76-91, 278-285):
//   MAX = bins//2 - 1;  max1 = amax(|x|, channels);  factor = MAX / max1
//   q = round(x * factor + MAX).to(int8)
// in fp32 with separately rounded mul and add (-ffp-contract=off), IEEE
// division, round-half-even.
//
// Mapping: a task = one "row oct", 8 consecutive tokens of one plane, taken by the G lanes of a wave
// (G = 16/32/64 by channel count); each lane owns NITER runs of 8 consecutive channels (one 16-byte load
// per row per run), so a task keeps 8*NITER independent 16-byte loads in flight per lane (NITER <= 2).
// The row max is a packed-u16 integer max on |x| bit patterns (NaN > inf > finite, which is torch.amax's
// NaN propagation) reduced with xor-shuffles inside the G-lane group.
//
// Output, QUAD=true (pipeline): the symbol workspace of the coder, one region of TQ*C dwords per
// (chunk, plane), written with a lane-local transpose so that the coder later reads several tokens of its
// channel with one coalesced dword:
//   planes with > 17 bins  [quad][channel] u32, byte k = symbol of token 4*quad + k
//   planes with <= 17 bins [oct][channel] u32,  byte k = token 8*oct + k | token 8*oct + 4 + k << 4
// Output, QUAD=false (lmc_quantize parity entry): int8 [P][T][C].
#pragma once
#include "lmc_device.h"
#include "k_hist.h"

struct QuantArgs {
  KvAddr src;
  BinsArg bins;
  int tok_begin, tok_end, chunk_tokens, nchunks;
  int P, C, TQ;          // TQ = ceil(chunk_tokens / 4)
  long long sym_stride;  // QUAD: dwords between the workspace regions of consecutive (chunk, plane) pairs (>= TQ * C)
  int pc_limit;          // plane-chunks (chunk * P + plane) to quantise: nchunks * P
  u32* sym4;             // QUAD: symbol workspace, TQ*C dwords per (chunk, plane)
  int8_t* sym8;          // !QUAD: [P][T][C]
  u8* scale_base;        // scale of (chunk, p, t) at scale_base + chunk*scale_stride + 2*(p*Tc + t)
  long long scale_stride;
  unsigned long long* agg;  // the coder's look-back granules, zeroed here (saves a memset dispatch), or NULL
  long long agg_n;
  u32* sizes;               // ... and the job's size words [nchunks] (0 = "this chunk's encode did not finish"), or NULL
  // A launch over a SUBSET of the planes (k_layers.h: a layer of a layer-wise store is plane0 = l, plane_step = L, two
  // planes): grid row y takes plane plane0 + y * plane_step of every chunk.  Source, bins and the scales' place in the blob
  // stay addressed by that real plane; the symbol workspace holds the launch's planes only, region (chunk, y).  All zero:
  // every plane, plane y in row y -- what every launch was before these fields existed.
  int plane0, plane_step, nplanes;
};

typedef float f32x2_t __attribute__((ext_vector_type(2)));
// Regular rows (finite, non-zero max): |x * factor| <= MAX(1 + 2^-23), so z = x*factor + MAX lies in
// [-MAX 2^-23, 2 MAX + ...] and round-half-even gives 0 .. 2*MAX.  Two elements per instruction with the
// packed fp32 multiply and add (each rounded on its own: no FMA), and v_cvt_pk_u8_f32 does the RNE
// conversion, the clamp at 0 (-0.x -> 0) and the byte insertion in one op (probed on gfx950:
// tools/probes/cvt_pk_u8.hip -- RNE, saturating, NaN -> 0).  The three functions below, compiled with the library's
// flags, are held against round(fl(fl(x * factor) + MAX)) for every x of chosen rows -- rows picked so that a fused
// multiply-add or a factor one ulp off would show -- by tests/test_gpu_device_arith.py::test_quantise_step_*.
__device__ __forceinline__ f32x2_t quant_z2(float xlo, float xhi, f32x2_t factor2, f32x2_t maxf2) {
  f32x2_t x = {xlo, xhi};
  f32x2_t y = x * factor2;  // v_pk_mul_f32, rounded
  return y + maxf2;         // v_pk_add_f32, rounded separately (-ffp-contract=off)
}
__device__ __forceinline__ u32 quant_fast(float x, float factor, float maxf) {
  float y = x * factor;  // rounded
  float z = y + maxf;    // rounded separately (no FMA: -ffp-contract=off)
  return (u32)(int)__builtin_rintf(z);
}
// Special rows (max is 0 / denormal-tiny / inf / NaN): follow the reference's CPU float->int8
// conversion: NaN and |r| >= 2^31 give INT_MIN whose low byte is 0.
__device__ __forceinline__ u32 quant_special(float x, float factor, float maxf) {
  float y = x * factor;
  float z = y + maxf;
  float r = __builtin_rintf(z);
  return (__builtin_fabsf(r) < 2147483648.0f) ? ((u32)(int)r & 0xffu) : 0u;
}

// ---- an LMC_PAGED_SPLIT source (include/lmc_hip.h: the cache of vLLM's ROCm paged-attention kernels) -----------------
// The cache keeps, per block b and head h, one dense run of D * block_size elements (k_copy_split.h):
//   K(b, h, d, w) = b * stride_block + h * stride_head + ((d / X) * block_size + w) * X + d % X     X = 16 / element bytes
//   V(b, h, d, w) = b * stride_block + h * stride_head + d * block_size + w
// The block offset is 64-bit; everything inside a block fits 32 bits (lmc_api.hip: split_range_ok).
// K: a lane's 8 channels of a token are still one x-granule (fp8: half of one), only at another address -- the task
// keeps quantize_task's token-major registers, v[r][it] = token r.  V: 16 bytes (fp8: 8) are eight consecutive slots of
// ONE channel, which is what a workspace dword holds anyway, so the task loads channel-major, v[e][it] = the 8 tokens of
// channel c0[it] + e, and quantises without a transpose (the V form of quantize_task).  That needs the oct's tokens at
// slots s, s + 1, ... of one block with s % 8 == 0 and block_size % 8 == 0 (of a ragged oct: its tokens below Tc; the
// load still lies inside the block that the oct's first slot names), and both forms need the plane base and the block
// and head strides to keep the vector on its 16-byte (8-byte) boundary.  Anything else -- single tokens at random slots,
// a run that enters a block at offset 5 or breaks inside the oct, a base 2 bytes off -- is loaded element by element
// into the token-major registers.  Decided per task; a ballot sends the whole wave (G < 64: several octs) one way.
// Only slots of the job's own tokens are turned into addresses, and a token at or past Tc is zero in the registers.

// 8 elements p[0], p[step], ..., p[7 * step] as kv_ld8 would hold them
template <int DT>
__device__ __forceinline__ uint4 split_ld_elems(const typename KvElem<DT>::T* p, u32 step) {
  const LMC_GLOBAL typename KvElem<DT>::T* q = (const LMC_GLOBAL typename KvElem<DT>::T*)p;
  u32 e[8];
#pragma unroll
  for (int k = 0; k < 8; k++) e[k] = (u32)q[(u32)k * step];
  if constexpr (!lmc_dtype_fp8(DT)) return make_uint4(e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16));
  else return make_uint4(e[0] | (e[1] << 8) | (e[2] << 16) | (e[3] << 24), e[4] | (e[5] << 8) | (e[6] << 16) | (e[7] << 24), 0u, 0u);
}

// The loads of one row oct from a split source.  -> true: the V form (v[e][it]), false: token-major (v[r][it]).
template <int NITER, int DT>
__device__ __forceinline__ bool split_load_oct(const KvAddr& src, int p, int tok0, int Tc, int t_first, bool qvalid,
                                               const int (&c0)[NITER], const bool (&cval)[NITER], uint4 (&v)[8][NITER],
                                               bool (&tv)[8]) {
  typedef typename KvElem<DT>::T E;
  constexpr u32 X = 16 / (u32)sizeof(E);
  const bool is_v = p >= src.L;  // (wave-uniform, like everything of the plane)
  const E* const pbase = lmc_plane_base<E>(src, p);
  const u32 bs = (u32)src.block_size;
  const bool aligned = ((((uintptr_t)pbase) & (lmc_dtype_fp8(DT) ? 7u : 15u)) | (uintptr_t)((src.stride_block | src.stride_head) & 7)) == 0;
  u32 s[8];
#pragma unroll
  for (int r = 0; r < 8; r++) {
    tv[r] = qvalid && t_first + r < Tc;
    s[r] = tv[r] ? (u32)src.slot_mapping[tok0 + t_first + r] : 0u;
  }
  const u32 b0 = s[0] / bs, w0 = s[0] - b0 * bs;  // (the valid tokens of an oct are its first: tv[0] or none)
  // the lane's channel runs inside a block
  u32 in_k[NITER], in_v[NITER];
#pragma unroll
  for (int it = 0; it < NITER; it++) {
    const u32 h = (u32)c0[it] / (u32)src.D, d = (u32)c0[it] - h * (u32)src.D;
    const u32 hoff = h * (u32)src.stride_head;
    in_k[it] = hoff + (d / X) * (bs * X) + d % X;
    in_v[it] = hoff + d * bs;
  }
  if (is_v) {
    bool run = aligned && (w0 & 7u) == 0u && (bs & 7u) == 0u;
#pragma unroll
    for (int r = 1; r < 8; r++) run = run && (!tv[r] || s[r] == s[0] + (u32)r);
    if (__ballot(tv[0] && !run) == 0ull) {
      // tokens at or past Tc share the vector with the oct's own: cleared
      u32 msk[4];
      if constexpr (!lmc_dtype_fp8(DT)) {
#pragma unroll
        for (int j = 0; j < 4; j++) msk[j] = (tv[2 * j] ? 0xffffu : 0u) | (tv[2 * j + 1] ? 0xffff0000u : 0u);
      } else {
#pragma unroll
        for (int j = 0; j < 2; j++)
          msk[j] = (tv[4 * j] ? 0xffu : 0u) | (tv[4 * j + 1] ? 0xff00u : 0u) | (tv[4 * j + 2] ? 0xff0000u : 0u) | (tv[4 * j + 3] ? 0xff000000u : 0u);
        msk[2] = msk[3] = 0u;
      }
      const E* const blk = pbase + (long long)b0 * src.stride_block + w0;
#pragma unroll
      for (int it = 0; it < NITER; it++) {
#pragma unroll
        for (int e = 0; e < 8; e++) {
          if (tv[0] && cval[it]) {
            const uint4 u = kv_ld8<DT>(blk + (in_v[it] + (u32)e * bs));
            v[e][it] = make_uint4(u.x & msk[0], u.y & msk[1], u.z & msk[2], u.w & msk[3]);
          } else v[e][it] = make_uint4(0, 0, 0, 0);
        }
      }
      return true;
    }
  }
  // token-major: every token's own block and column -- without a division where the oct stays in the block of its first
  // token (wave-uniform: a ballot)
  bool same = true;
#pragma unroll
  for (int r = 1; r < 8; r++) same = same && (!tv[r] || s[r] - (s[0] - w0) < bs);
  auto load_tokens = [&](auto same_tag) {
#pragma unroll
    for (int r = 0; r < 8; r++) {
      const u32 br = decltype(same_tag)::value ? b0 : s[r] / bs;
      const u32 wr = decltype(same_tag)::value ? s[r] - (s[0] - w0) : s[r] - br * bs;
      const E* const tp = pbase + (long long)br * src.stride_block;
#pragma unroll
      for (int it = 0; it < NITER; it++) {
        if (!(tv[r] && cval[it])) v[r][it] = make_uint4(0, 0, 0, 0);
        else if (is_v) v[r][it] = split_ld_elems<DT>(tp + (in_v[it] + wr), bs);
        else if (aligned) v[r][it] = kv_ld8<DT>(tp + (in_k[it] + wr * X));
        else v[r][it] = split_ld_elems<DT>(tp + (in_k[it] + wr * X), 1u);
      }
    }
  };
  if (__ballot(!same) == 0ull) load_tokens(BoolTag<true>{});
  else load_tokens(BoolTag<false>{});
  return false;
}

// One task = 4 (row quad) or, NIB, 8 consecutive tokens starting at token t_first of plane p of one chunk,
// by the G lanes sl = 0..G-1.
//   sym_out     QUAD: the task's dwords, [channel]      sym8_plane  !QUAD: &sym8[p][0][0]
//   scale_out   &scales[chunk][p][t_first]
// QUAD output dword of channel c: byte k = symbol of token t_first + k.  NIB (planes whose symbols fit four
// bits: bins <= 17): byte k = symbol of token t_first + k | symbol of token t_first + 4 + k << 4, so the
// workspace round trip of most planes is half a byte per element.
// ROWS (4 or 2): rows loaded and reduced together -- 4 keeps 4*NITER 16-byte loads in flight per lane,
// 2 halves the registers.
// SPLIT > 1 (planes of more than 1024 channels, workspace output): SPLIT waves of the workgroup share the task, wave
// `slice` takes channels [slice, slice + 1) * NITER * 512, and the row maxima meet in `xmax` (LDS, [8][SPLIT]) behind
// ONE workgroup barrier per task -- a wave then holds 8 rows x 1024 channels (98 VGPRs, 4 waves per SIMD) where a
// whole 4096-channel row per wave costs 241 VGPRs and 2 waves per SIMD (C = 4096: 3.5 -> 4.3 TB/s).
// HIST (the fused encode's narrow planes, round 6): the task's symbols also go into the work item's histogram (k_hist.h)
// -- hist_lane4 = 4 * the task's virtual quantising lane, hist_it its virtual channel run (wave-uniform: a wave pass
// quantises row octs of ONE plane).
// NHDB: the source is an LMC_PAGED_SPLIT cache (split_load_oct above): the loads, and for a V oct on its fast path the
// max and the conversion in their channel-major form; from o[][][] on the task is the same.
// SINK (k_fixed.h, the fixed-width model): the task's symbols do not go to the workspace but to `sink`, in registers --
// sink.oct(c0, lo quad dwords, hi quad dwords) per channel run of a valid task, runs past C included (their dwords are 0),
// and sink.scale(token, bits) with every scale the task stores.  NoSink: the task as it always was.
struct NoSink {};
template <int G, int NITER, int DT, bool QUAD, bool NIB, int ROWS = 4, int NQ = NIB ? 2 : 1, int SPLIT = 1, bool HIST = false,
          bool NHDB = false, class SINK = NoSink>
__device__ __forceinline__ void quantize_task(const KvAddr& src, int p, int tok0, int Tc, int t_first, bool qvalid,
                                              bool q1valid, int C, float maxf, u32* sym_out, int8_t* sym8_plane,
                                              u16* scale_out, int sl, int slice = 0, u32* xmax = nullptr,
                                              u32 hist_lane4 = 0, int hist_it = 0, SINK* sink = nullptr) {
  constexpr bool HAS_SINK = !__is_same(SINK, NoSink);
  static_assert(!HAS_SINK || (QUAD && NQ == 2 && ROWS == 8 && !HIST), "a sink takes whole octs");
  static_assert(!HIST || (QUAD && NITER == 1 && NQ == 2 && SPLIT == 1), "the histogram rides on the fused kernel's narrow tasks");
  static_assert(SPLIT == 1 || (QUAD && ROWS == 4 * NQ), "a split task exchanges all its rows' maxima at once");
  static_assert(ROWS == 2 || ROWS == 4 || (ROWS == 8 && NQ == 2), "rows in flight: a power of two within the task");
  static_assert(QUAD || (!NIB && NQ == 1), "nibble packing and two-quad tasks are workspace formats");
  static_assert(!NIB || NQ == 2, "a nibble dword holds two row quads");
  static_assert(!NHDB || (QUAD && ROWS == 8 && SPLIT == 1 && !HIST), "a split source: whole octs into the workspace");
  // per-lane channel runs (row independent)
  long long coff[NITER];
  int c0[NITER];
  bool cval[NITER];
#pragma unroll
  for (int it = 0; it < NITER; it++) {
    c0[it] = ((slice * NITER + it) * G + sl) * 8;
    cval[it] = c0[it] < C;
    int h = c0[it] / src.D, d = c0[it] - h * src.D;
    coff[it] = (long long)h * src.stride_head + d;
  }
  const typename KvElem<DT>::T* pbase = lmc_plane_base<typename KvElem<DT>::T>(src, p);
  const f32x2_t maxf2 = {maxf, maxf};
  // QUAD: o[hq][it][e] byte r = symbol of (token t_first + 4 hq + r, channel c0[it] + e); bytes of tokens past
  // the end of a ragged chunk are never read by the coder, so they need no masking
  u32 o[NQ][NITER][8];
#pragma unroll
  for (int hq = 0; hq < NQ; hq++)
#pragma unroll
    for (int it = 0; it < NITER; it++)
#pragma unroll
      for (int e = 0; e < 8; e++) o[hq][it][e] = 0;

#pragma unroll
  for (int r0 = 0; r0 < 4 * NQ; r0 += ROWS) {
    uint4 v[ROWS][NITER];
    bool tv[ROWS];
    bool vform = false;  // NHDB, a V oct on its fast path: v[e][it] = the 8 tokens of channel c0[it] + e
    if constexpr (NHDB) {
      vform = split_load_oct<NITER, DT>(src, p, tok0, Tc, t_first, qvalid, c0, cval, v, tv);
    } else {
#pragma unroll
      for (int r = 0; r < ROWS; r++) {
        int t = t_first + r0 + r;
        tv[r] = qvalid && t < Tc;
        const typename KvElem<DT>::T* rowp = pbase + (tv[r] ? lmc_tok_off(src, tok0 + t) : 0);
#pragma unroll
        for (int it = 0; it < NITER; it++) {
          if (tv[r] && cval[it]) v[r][it] = kv_ld8<DT>(rowp + coff[it]);  // (non-temporal here: two-kernel path +0.5 %)
          else v[r][it] = make_uint4(0, 0, 0, 0);
        }
      }
    }

    // row |x| max on bit patterns, two rows per register through the xor-shuffle reduction
    u32 mrow[ROWS];
    if (!NHDB || !vform) {
#pragma unroll
      for (int r = 0; r < ROWS; r++) {
        u32 m = 0;
#pragma unroll
        for (int it = 0; it < NITER; it++) {
          m = kv_absmax8<DT>(m, v[r][it]);
        }
        mrow[r] = max(m & 0xffffu, m >> 16);
      }
#pragma unroll
      for (int r = 0; r < ROWS; r += 2) {
        u32 m2 = mrow[r] | (mrow[r + 1] << 16);
#pragma unroll
        for (int off = 1; off < G; off <<= 1) m2 = pk_max_u16(m2, (u32)__shfl_xor((int)m2, off));
        mrow[r] = m2 & 0xffffu;
        mrow[r + 1] = m2 >> 16;
      }
    } else if constexpr (NHDB) {
      // V form: the element-wise packed max over the lane's channels leaves the eight per-token maxima in 4 dwords --
      // 16-bit: dword j = tokens 2j | 2j + 1; fp8 (a byte per token, widened to the u16 lanes): tokens 0|2, 1|3, 4|6, 5|7
      u32 m4[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int it = 0; it < NITER; it++) {
#pragma unroll
        for (int e = 0; e < 8; e++) {
          const uint4& u = v[e][it];
          if constexpr (!lmc_dtype_fp8(DT)) {
            m4[0] = pk_max_u16(m4[0], u.x & 0x7fff7fffu);
            m4[1] = pk_max_u16(m4[1], u.y & 0x7fff7fffu);
            m4[2] = pk_max_u16(m4[2], u.z & 0x7fff7fffu);
            m4[3] = pk_max_u16(m4[3], u.w & 0x7fff7fffu);
          } else {
            m4[0] = pk_max_u16(m4[0], u.x & 0x007f007fu);
            m4[1] = pk_max_u16(m4[1], (u.x >> 8) & 0x007f007fu);
            m4[2] = pk_max_u16(m4[2], u.y & 0x007f007fu);
            m4[3] = pk_max_u16(m4[3], (u.y >> 8) & 0x007f007fu);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < 4; j++) {
#pragma unroll
        for (int off = 1; off < G; off <<= 1) m4[j] = pk_max_u16(m4[j], (u32)__shfl_xor((int)m4[j], off));
        constexpr bool B8 = lmc_dtype_fp8(DT);
        mrow[B8 ? 4 * (j >> 1) + (j & 1) : 2 * j] = m4[j] & 0xffffu;
        mrow[B8 ? 4 * (j >> 1) + (j & 1) + 2 : 2 * j + 1] = m4[j] >> 16;
      }
    }

    if constexpr (SPLIT > 1) {  // the row maxima of the SPLIT channel slices meet in LDS
      if (sl == 0) {
#pragma unroll
        for (int r = 0; r < ROWS; r++) xmax[r * SPLIT + slice] = mrow[r];
      }
      __syncthreads();
#pragma unroll
      for (int r = 0; r < ROWS; r++) {
        u32 m = 0;
#pragma unroll
        for (int k = 0; k < SPLIT; k++) m = max(m, xmax[r * SPLIT + k]);
        mrow[r] = m;
      }
    }
#pragma unroll
    for (int r = 0; r < ROWS; r++) mrow[r] = kv_max_scale<DT>(mrow[r]);  // (fp8: the max's bf16 image; else the max itself)
    // scales: first lane of the group (of the first slice)
    if (sl == 0 && slice == 0) {
#pragma unroll
      for (int r = 0; r < ROWS; r++)
        if (tv[r]) {
          scale_out[r0 + r] = (u16)mrow[r];
          if constexpr (HAS_SINK) sink->scale((u32)(t_first + r0 + r), mrow[r]);
        }
    }

    float factor[ROWS];
    bool special[ROWS];
    bool any_special = false;
#pragma unroll
    for (int r = 0; r < ROWS; r++) {
      float sf = h2f_rt(mrow[r], lmc_math_dtype(DT));
      factor[r] = maxf / sf;  // IEEE fp32 division
      special[r] = !(__builtin_fabsf(factor[r]) < __builtin_inff()) || !(sf < __builtin_inff());
      any_special |= special[r];
    }
    const bool slow = __ballot(any_special) != 0;  // wave-uniform and rare (zero / inf / NaN rows, ragged tails)
    // one symbol at a time; special rows follow the CPU float -> int8 conversion of the reference
    auto sym_of = [&](int r, float x) -> u32 {
      return (special[r] ? quant_special(x, factor[r], maxf) : quant_fast(x, factor[r], maxf)) & 0xffu;
    };

#pragma unroll
    for (int it = 0; it < NITER; it++) {
      if (!cval[it] || !qvalid) continue;
      if constexpr (NHDB) {
        if (vform) {
          // V form: dword j of channel e holds tokens 2j and 2j + 1 (kv_lo / kv_hi: for fp8 the byte pairs, in the same
          // order), each with its own row's factor, inserted at its token's byte of o[token / 4][it][e]
#pragma unroll
          for (int e = 0; e < 8; e++) {
            const u32 w[4] = {v[e][it].x, v[e][it].y, v[e][it].z, v[e][it].w};
#pragma unroll
            for (int j = 0; j < 4; j++) {
              const float xlo = kv_lo<DT>(w, j), xhi = kv_hi<DT>(w, j);
              if (!slow) {
                const f32x2_t f2 = {factor[2 * j], factor[2 * j + 1]};
                const f32x2_t z = quant_z2(xlo, xhi, f2, maxf2);
                o[j >> 1][it][e] = __builtin_amdgcn_cvt_pk_u8_f32(z.x, (2 * j) & 3, o[j >> 1][it][e]);
                o[j >> 1][it][e] = __builtin_amdgcn_cvt_pk_u8_f32(z.y, (2 * j + 1) & 3, o[j >> 1][it][e]);
              } else {
                o[j >> 1][it][e] |= (sym_of(2 * j, xlo) << (8 * ((2 * j) & 3))) | (sym_of(2 * j + 1, xhi) << (8 * ((2 * j + 1) & 3)));
              }
            }
          }
          continue;
        }
      }
      if (QUAD) {
#pragma unroll
        for (int r = 0; r < ROWS; r++) {
          const u32 w[4] = {v[r][it].x, v[r][it].y, v[r][it].z, v[r][it].w};
          if (!slow) {  // four chained byte-inserting conversions per output dword
            const f32x2_t f2 = {factor[r], factor[r]};
#pragma unroll
            for (int k = 0; k < 4; k++) {
              const f32x2_t z = quant_z2(kv_lo<DT>(w, k), kv_hi<DT>(w, k), f2, maxf2);
              o[(r0 + r) >> 2][it][2 * k] = __builtin_amdgcn_cvt_pk_u8_f32(z.x, (r0 + r) & 3, o[(r0 + r) >> 2][it][2 * k]);
              o[(r0 + r) >> 2][it][2 * k + 1] = __builtin_amdgcn_cvt_pk_u8_f32(z.y, (r0 + r) & 3, o[(r0 + r) >> 2][it][2 * k + 1]);
            }
          } else {
#pragma unroll
            for (int k = 0; k < 4; k++) {
              o[(r0 + r) >> 2][it][2 * k] |= sym_of(r, kv_lo<DT>(w, k)) << (8 * ((r0 + r) & 3));
              o[(r0 + r) >> 2][it][2 * k + 1] |= sym_of(r, kv_hi<DT>(w, k)) << (8 * ((r0 + r) & 3));
            }
          }
        }
      } else {  // int8 [P][T][C] output of lmc_quantize
#pragma unroll
        for (int r = 0; r < ROWS; r++) {
          if (!tv[r]) continue;
          const u32 w[4] = {v[r][it].x, v[r][it].y, v[r][it].z, v[r][it].w};
          u32 lo = 0, hi = 0;
#pragma unroll
          for (int k = 0; k < 2; k++) {
            lo |= (sym_of(r, kv_lo<DT>(w, k)) << (16 * k)) | (sym_of(r, kv_hi<DT>(w, k)) << (16 * k + 8));
            hi |= (sym_of(r, kv_lo<DT>(w, k + 2)) << (16 * k)) | (sym_of(r, kv_hi<DT>(w, k + 2)) << (16 * k + 8));
          }
          int8_t* dst = sym8_plane + ((long long)(t_first + r0 + r)) * C + c0[it];
          *reinterpret_cast<uint2*>(dst) = make_uint2(lo, hi);
        }
      }
    }
  }
  if constexpr (HAS_SINK) {
    if (qvalid) {
#pragma unroll
      for (int it = 0; it < NITER; it++) sink->oct(c0[it], o[0][it], o[1][it]);
    }
  } else if (QUAD && qvalid) {
#pragma unroll
    for (int it = 0; it < NITER; it++) {
      if (!cval[it]) continue;
      u32* dst = sym_out + c0[it];  // kernel-arg pointers: global already
      if (NIB) {
        u32 w[8];
#pragma unroll
        for (int e = 0; e < 8; e++) w[e] = o[0][it][e] | (o[NQ - 1][it][e] << 4);
        *reinterpret_cast<uint4*>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
        *reinterpret_cast<uint4*>(dst + 4) = make_uint4(w[4], w[5], w[6], w[7]);
        if constexpr (HIST) {
#pragma unroll
          for (int e = 0; e < 8; e++) o[0][it][e] = w[e];  // the histogram below counts the merged dwords
        }
      } else {
#pragma unroll
        for (int hq = 0; hq < NQ; hq++) {  // byte format: the task's row quads are adjacent [quad][channel] rows
          if (hq == 1 && !q1valid) continue;
          u32* d2 = dst + (long long)hq * C;
          *reinterpret_cast<uint4*>(d2) = make_uint4(o[hq][it][0], o[hq][it][1], o[hq][it][2], o[hq][it][3]);
          *reinterpret_cast<uint4*>(d2 + 4) = make_uint4(o[hq][it][4], o[hq][it][5], o[hq][it][6], o[hq][it][7]);
        }
      }
    }
  }
  if constexpr (HIST) {
    // rows of the oct that are tokens of the chunk (per lane group: the groups of a wave pass hold different octs); a byte
    // plane leaves token 0 out (its u8 counters must not reach 256: k_hist.h)
    const int nrow = (qvalid && cval[0]) ? min(8, Tc - t_first) : 0;
    const bool all8 = __ballot(nrow != 8) == 0;           // wave-uniform: every group holds a full oct (the usual case)
    const bool tok0_here = !NIB && __ballot(nrow > 0 && t_first == 0) != 0;  // wave-uniform: some group holds token 0
    u32 ad[2] = {hist_lane4, hist_lane4};
    auto add_all = [&](auto it_tag) {
      constexpr int IT = decltype(it_tag)::value;
      static_for<8>([&](auto e_tag) {
        constexpr int E = decltype(e_tag)::value;
        if (all8 && !tok0_here) {
          if constexpr (NIB) plane_hist_dword<true, IT, E, 0>(o[0][0][E], ad, [](int) { return true; });
          else {
            plane_hist_dword<false, IT, E, 0>(o[0][0][E], ad, [](int) { return true; });
            plane_hist_dword<false, IT, E, 1>(o[1][0][E], ad, [](int) { return true; });
          }
        } else {  // a partial or absent oct in some group, or token 0 of a byte plane: per-lane tests (exec-masked adds)
          auto counted = [&](int row) { return row < nrow && (NIB || t_first + row != 0); };
          if constexpr (NIB) plane_hist_dword<true, IT, E, 0>(o[0][0][E], ad, counted);
          else {
            plane_hist_dword<false, IT, E, 0>(o[0][0][E], ad, counted);
            plane_hist_dword<false, IT, E, 1>(o[1][0][E], ad, counted);
          }
        }
      });
    };
    if (hist_it) add_all(IntTag<1>{});  // (wave-uniform)
    else add_all(IntTag<0>{});
  }
}

// A wave (G = 64) or a G-lane group takes one row OCT: tokens 8*oct .. 8*oct + 7.  Planes with bins <= 17
// get the nibble-packed workspace format (one dword per channel for the oct), the others two row quads.
// grid = (ceil(TO / (4 * RPW)), P, chunks), TO = ceil(TQ / 2): plane and chunk come straight from the block
// index, and with G = 64 everything but the channel offset is wave-uniform and lives in SGPRs.
// NHDB: the instances that read an LMC_PAGED_SPLIT source (workspace form, up to 1024 channels); every other instance is
// what it was before they existed.
template <int G, int NITER, int DT, bool QUAD, int SPLIT = 1, bool NHDB = false>
__global__ __launch_bounds__(256) void k_quantize(QuantArgs a) {
  static_assert(SPLIT == 1 || (QUAD && G == LMC_WAVE && (SPLIT == 2 || SPLIT == 4)), "split tasks: whole waves, workspace output");
  static_assert(!NHDB || (QUAD && SPLIT == 1 && NITER <= 2), "a split source: the workspace form, planes of up to 1024 channels");
  constexpr int RPW = LMC_WAVE / G;  // tasks per wave
  __shared__ u32 xmax[SPLIT > 1 ? (4 / SPLIT) * 8 * SPLIT : 1];  // row maxima of the split tasks of this workgroup
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int sub = lane / G, sl = lane % G;
  const int p = a.plane0 + (int)blockIdx.y * (a.plane_step ? a.plane_step : 1), chunk = (int)blockIdx.z;
  if (QUAD && (a.agg || a.sizes)) {  // the launch has at least 256 threads per plane-chunk, a plane-chunk at most 64 granules
    const long long i = (((long long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 256 + threadIdx.x;
    if (a.agg && i < a.agg_n) a.agg[i] = 0ull;  // (a layer-wise job's granules live across its launches: zeroed once, by the host)
    if (a.sizes && i < a.nchunks) a.sizes[i] = 0u;
  }
  const int TO = (a.TQ + 1) >> 1;
  int oct = SPLIT > 1 ? ((int)blockIdx.x * 4 + wave) / SPLIT : ((int)blockIdx.x * 4 + wave) * RPW + sub;
  const int slice = SPLIT > 1 ? wave % SPLIT : 0;
  const bool ovalid = oct < TO && chunk * a.P + p < a.pc_limit;
  if (!ovalid) oct = 0;
  const int tok0 = a.tok_begin + chunk * a.chunk_tokens;
  const int Tc = min(a.chunk_tokens, a.tok_end - tok0);
  const int bins = (int)a.bins.b[p];
  const float maxf = (float)(bins / 2 - 1);
  u16* scale_out = reinterpret_cast<u16*>(a.scale_base + (long long)chunk * a.scale_stride) + ((long long)p * Tc + oct * 8);
  u32* sym_pc = QUAD ? a.sym4 + ((long long)chunk * gridDim.y + blockIdx.y) * a.sym_stride : nullptr;  // this plane-chunk's workspace (gridDim.y: the launch's planes)
  int8_t* sym8_plane = QUAD ? nullptr : a.sym8 + (long long)p * Tc * a.C;
  if constexpr (QUAD) {
    constexpr int ROWS = NITER <= 2 ? 8 : 4;  // 16-byte loads in flight per lane: ROWS * NITER
    u32* const sym_out = sym_pc + (long long)oct * (lmc_sym_nibbles(bins) ? 1 : 2) * a.C;
    const bool q1valid = 2 * oct + 1 < a.TQ;
    u32* const xm = xmax + (SPLIT > 1 ? (wave / SPLIT) * 8 * SPLIT : 0);  // this task's exchange slots
    if (lmc_sym_nibbles(bins))
      quantize_task<G, NITER, DT, true, true, ROWS, 2, SPLIT, false, NHDB>(a.src, p, tok0, Tc, oct * 8, ovalid, q1valid, a.C, maxf,
                                                                           sym_out, nullptr, scale_out, sl, slice, xm);
    else
      quantize_task<G, NITER, DT, true, false, ROWS, 2, SPLIT, false, NHDB>(a.src, p, tok0, Tc, oct * 8, ovalid, q1valid, a.C, maxf,
                                                                            sym_out, nullptr, scale_out, sl, slice, xm);
  } else {
#pragma unroll 1
    for (int hq = 0; hq < 2; hq++) {
      const int q = 2 * oct + hq;
      quantize_task<G, NITER, DT, false, false>(a.src, p, tok0, Tc, q * 4, ovalid && q < a.TQ, false, a.C, maxf, nullptr,
                                                sym8_plane, scale_out + 4 * hq, sl);
    }
  }
}
