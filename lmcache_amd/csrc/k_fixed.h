// k_fixed.h -- LMC_MODEL_FIXED (include/lmc_format.h): the CacheGen quantisation with every symbol stored at a fixed 4 or
// 5 bits and no entropy coder.  For the tier whose blobs stay in HBM: nothing crosses PCIe there, so the bytes the coder
// saves buy nothing and its token loop is the whole cost.  Quantiser, scales, dequantisation and casts are the coded
// models': a chunk decodes to the same bits whichever model stored it.
//
// k_fixed_encode -- one pass, source -> blob; the symbols never see a workspace.  A WORKGROUP OWNS A PLANE of a chunk: its
// waves walk the plane's row octs with k_quantize.h's quantize_task (same loads, row max, quant_z2 / quant_fast /
// quant_special, special-row rule), which hands each lane the eight nibble dwords of its 8 channels x 8 tokens in
// registers (FixedSink) instead of storing them to the workspace: two 16-byte stores into `lo`, and for a wide plane one
// 8-byte store into `hi`.  Why this mapping and not one atomic per (task, group): the check word of a stream and the
// plane's scsum are sums over the whole plane; with the plane in one workgroup they are summed on chip (LDS adds, integer:
// order-free, so deterministic) and stored once -- no pre-zeroed words, no memset dispatch in front, no global atomics
// (2 M single-lane atomics per 16 k context otherwise; cdna_hip_programming.md guideline 12: sum on chip what shares a
// destination).  The price is a grid of chunks x planes workgroups, which a job of a few chunks does not fill, and
// workgroups that live as long as a plane takes (FIXED_ENC_WAVES below).
// The workgroup of plane 0 also writes header, bins and pads; every workgroup its plane's directory entries and scsum.
//
// k_fixed_encode<..., LAYER = true> + k_fixed_layers_finish -- the layer-wise job (lmc_encode_layers_begin_fixed): a launch
// covers the two planes of one layer, which a workgroup per (plane, chunk) would leave at 2 x nchunks workgroups, so the
// work item there is (chunk, plane, SLICE): a run of whole passes of the plane's row octs.  Loads, `lo` / `hi` stores and
// scales are the one-piece kernel's.  The sums stay on chip per slice as above; check word and scsum are linear mod 2^32
// over absolute dword / token indices, so a slice's LDS sums are partials: stored once, plainly, into a slot of the job's
// workspace that only this workgroup writes, and added up by the finish kernel, which also writes what is per stream,
// per plane and per chunk.  Still no memset, no pre-zeroed word, no global atomic.
//
// k_fixed_decode -- a wave takes a stream and walks it in tiles of four octs (32 tokens): 16-byte loads of `lo` (lane =
// 4 channels of one oct) and a dword of `hi`, staged in 1.3 KiB of LDS and read back transposed -- lane = (8 channels,
// one token) -- so that every lane dequantises one 16-byte row vector per oct: t = ((q - C) / C) * max1 from k_decode.h's
// LUT construction, one RNE cast (fp16: two roundings, as there), one 16-byte store (element stores where the
// destination's rows are not vector-addressable).  The next tile's loads are in flight while this one is stored.  The
// check word is summed over exactly the dwords the wave loaded and compared at the end (BAD_STREAM), the plane's first
// wave checks scsum (BAD_SCALES); everything a section's address depends on is validated before the section is read
// (BAD_HEADER).  Block-ordered paged destinations take the same per-token path: a token's row is one slot_mapping load
// per lane and oct (k_decode.h's eight-row blocks were built around its scalar stores and are not needed here).
//
// LMC_PAGED_SPLIT ("NHDB", the cache of vLLM's ROCm paged-attention kernels: include/lmc_hip.h) on both sides, 16-bit
// elements.  k_fixed_encode<..., NHDB = true>: quantize_task's split source form (k_quantize.h, split_load_oct) with the
// same sink -- the loads differ, the blob does not; planes of up to 1024 channels (SPLIT == 1).
// k_fixed_decode<DT, DEC_PAGED_SPLIT>: a K plane goes through the same transpose, and the lane's 8 channels of a token are
// one x-granule (x = 8): the same 16-byte store at block * stride_block + h * stride_head + (d / 8) * (block_size * 8) +
// w * 8.  A V plane skips the transpose: AS LOADED, lane l holds `lo` dwords 4 l .. 4 l + 3 and `hi` dword l of the tile,
// i.e. every bit of channels 4 (l & 15) .. + 3 for the eight tokens of oct l >> 4, and eight consecutive slots of one
// channel are 16 contiguous bytes of the plane -- four 16-byte stores per lane where the oct's tokens lie at slots s ..
// s + 7 of one block, s % 8 == 0, all eight of them to be written, and base and strides keep the vector aligned (the
// encoder's V-form condition; a ballot sends the tile's four octs one way).  Any other oct -- a ragged tail, the
// first-chunk trim, a run that enters a block at offset 5 or breaks, single tokens at random slots, a base 2 bytes off --
// is stored element by element, live tokens only; a slot is read from slot_mapping only for a token that is written.
// The split stores carry no non-temporal hint: 16-byte pieces whose neighbours arrive later want L2 to merge them
// (k_decode.h, LMC_DEC_SPLIT_NT: 1.47 against 3.11 ms there).  A V store of 32 contiguous bytes per channel (two octs of
// a 16-slot block regrouped through LDS) was not built, so not compared.
//
// k_fixed_expand (at the end of this file) -- fixed-width blobs back into the symbol workspace, scales and job words that
// k_quantize leaves for the coder: the first kernel of lmc_transcode_fixed, the fixed-width tier's demotion.
#pragma once
#include "k_encode.h"
#include "k_quantize.h"
#include "k_decode.h"

__device__ __forceinline__ u32 fixed_stream_bytes_dev(u32 bins, u32 O) {  // lmc_fixed_stream_bytes
  return (bins <= LMC_FIXED_NARROW_BINS ? 256u : 320u) * O + LMC_FIXED_TAIL_BYTES;
}

struct FixedEncArgs {
  KvAddr src;
  EncodeArgs e;  // tok_begin .. nchunks, P, C, G, blobs, blob_stride, bins, sizes, L, H, D, dtype; plane0, plane_step
  // ---- a layer's launch of a layer-wise job (lmc_encode_layers_begin_fixed): the LAYER instances alone read these ----
  // grid = (planes of the launch, nchunks, slices): workgroup (x, chunk, z) quantises passes [z * slice_passes, + slice_passes)
  // of plane e.plane0 + x * e.plane_step and leaves its LDS sums -- NG check words and the scsum term, PARTIALS of the
  // plane's (both are sums mod 2^32 over the absolute dword / token index) -- at part[((chunk * P + p) * gridDim.z + z) *
  // (NG + 1)], plain stores, each slot written by exactly this workgroup (zeros by a slice that lies behind a ragged
  // chunk's last oct).  Tails, directory, scsum, the static sections and the size word are k_fixed_layers_finish's.
  u32* part;
  u32 slice_passes;
};

// What quantize_task hands over (k_quantize.h, SINK).  o0 / o1: byte r of dword e = symbol of (token 8 oct + r / + 4 + r,
// channel c0 + e).
typedef __attribute__((address_space(3))) u32 LdsU32;
struct FixedSink {
  u8* plane_streams;  // stream (p, 0)
  LdsU32* chk;        // LDS [NG]: the streams' check sums
  u32 ssize, O, NG, oct_i, scs;
  bool wide;
  __device__ __forceinline__ void scale(u32 t, u32 bits) { scs += (t + 1u) * (bits + 1u); }  // lmc_scale_checksum_term
  __device__ __forceinline__ void oct_store(int c0, const u32 (&o0)[8], const u32 (&o1)[8]) {
    if ((u32)c0 >= 64u * NG) return;  // (runs past C inside the last group store their zeros)
    const u32 g = (u32)c0 >> 6, l0 = (u32)c0 & 63u;
    u8* const sb = plane_streams + (size_t)g * ssize;
    const u32 i0 = oct_i * 64u + l0;
    u32 w[8], sum = 0;
#pragma unroll
    for (int e = 0; e < 8; e++) {
      w[e] = (o0[e] & 0x0f0f0f0fu) | ((o1[e] & 0x0f0f0f0fu) << 4);
      sum += (2u * (i0 + (u32)e) + 1u) * w[e];
    }
    LMC_GLOBAL u32x4_t* const lo = (LMC_GLOBAL u32x4_t*)(sb + 4u * (size_t)i0);
    lo[0] = u32x4_t{w[0], w[1], w[2], w[3]};
    lo[1] = u32x4_t{w[4], w[5], w[6], w[7]};
    if (wide) {
      // bit 4 of the four bytes of a dword -> four adjacent bits (the products' bit positions are all distinct: no carries)
      u32 h[2] = {0u, 0u};
#pragma unroll
      for (int e = 0; e < 8; e++) {
        const u32 b = ((((o0[e] >> 4) & 0x01010101u) * 0x01020408u) >> 24) | (((((o1[e] >> 4) & 0x01010101u) * 0x01020408u) >> 24) << 4);
        h[e >> 2] |= b << (8 * (e & 3));
      }
      const u32 j0 = 64u * O + oct_i * 16u + (l0 >> 2);
      sum += (2u * j0 + 1u) * h[0] + (2u * j0 + 3u) * h[1];
      *(LMC_GLOBAL u32x2_t*)(sb + 256u * (size_t)O + oct_i * 64u + l0) = u32x2_t{h[0], h[1]};
    }
    __hip_atomic_fetch_add(chk + g, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);  // ds_add_u32
  }
  __device__ __forceinline__ void oct(int c0, const u32 (&o0)[8], const u32 (&o1)[8]) { oct_store(c0, o0, o1); }
};

// grid = (P, nchunks), FIXED_ENC_WAVES waves.  G lanes per row oct, NITER channel runs per lane, SPLIT waves per oct of
// a plane of more than 1024 channels: k_quantize's workspace instances.
#ifndef FIXED_ENC_WAVES
#define FIXED_ENC_WAVES 8  // 8 waves walk a 256-token plane in 4 passes: measured against 4 waves (8 passes, workgroups that
                           // live twice as long) on a 16 k Llama-3-8B context, same box, alternating: 0.557 against 0.614 ms
#endif
// LAYER: the sliced launch over a layer's planes (FixedEncArgs).  A template flag and not run-time fields read by every
// instance: with the flag off the kernel is the code it was, and the one-piece encode of a 16 k context cannot be told
// from the parent library's (0.6344 / 0.6351 against 0.6346 / 0.6352 ms, alternating in one process).  The build with
// run-time fields came out 0.002 ms behind this one, though only across two runs of a comparison whose sides did not
// share a host path: profiles/fixed_layerwise_store.md has both.  Price: 16 instances, half a minute of compile.
template <int G, int NITER, int DT, int SPLIT, bool NHDB = false, bool LAYER = false>
__global__ __launch_bounds__(64 * FIXED_ENC_WAVES) void k_fixed_encode(FixedEncArgs a) {
  constexpr int NW = FIXED_ENC_WAVES;
  static_assert(!NHDB || SPLIT == 1, "a split source: planes of up to 1024 channels");
  static_assert(!LAYER || SPLIT == 1, "layer launches: planes of up to 1024 channels (the split tasks meet at barriers)");
  static_assert(SPLIT == 1 || (G == LMC_WAVE && NITER == 2 && (SPLIT == 2 || SPLIT == 4)), "split tasks: whole waves");
  constexpr int RPW = LMC_WAVE / G;
  constexpr int PER_PASS = SPLIT > 1 ? NW / SPLIT : NW * RPW;  // row octs a workgroup takes at a time
  __shared__ u32 xmax[SPLIT > 1 ? (NW / SPLIT) * 8 * SPLIT : 1];
  __shared__ u32 chk[LMC_MAX_CHANNELS / 64];
  __shared__ u32 scs_all;
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int sub = lane / G, sl = lane % G;
  const EncodeArgs& e = a.e;
  const int p = LAYER ? e.plane0 + (int)blockIdx.x * e.plane_step : (int)blockIdx.x, chunk = (int)blockIdx.y;
  const int tok0 = e.tok_begin + chunk * e.chunk_tokens;
  const int Tc = min(e.chunk_tokens, e.tok_end - tok0);
  const u32 O = ((u32)Tc + 7u) >> 3, NG = (u32)e.G;
  const int bins = (int)e.bins.b[p];
  const float maxf = (float)(bins / 2 - 1);
  u32 beg = 0, total = 0;  // this plane's first stream, the streams section (wave-uniform: scalar code)
  for (int q = 0; q < e.P; q++) {
    const u32 sz = NG * fixed_stream_bytes_dev((u32)e.bins.b[q], O);
    if (q < p) beg += sz;
    total += sz;
  }
  const u32 ssize = fixed_stream_bytes_dev((u32)bins, O);
  const BlobOff bo = lmc_blob_off((u32)e.P, (u32)Tc, NG);
  u8* const blob = e.blobs + (long long)chunk * e.blob_stride;
  if (tid < LMC_MAX_CHANNELS / 64) chk[tid] = 0u;
  if (tid == 0) scs_all = 0u;
  __syncthreads();

  FixedSink sink;
  sink.plane_streams = blob + bo.streams + beg;
  sink.chk = (LdsU32*)chk;
  sink.ssize = ssize; sink.O = O; sink.NG = NG; sink.oct_i = 0u; sink.scs = 0u;
  sink.wide = !lmc_sym_nibbles(bins);
  const int slice = SPLIT > 1 ? wave % SPLIT : 0;
  u32* const xm = xmax + (SPLIT > 1 ? (wave / SPLIT) * 8 * SPLIT : 0);
  const u32 npass = (O + PER_PASS - 1u) / PER_PASS;  // the same for every wave: the split tasks meet at barriers
  const u32 pass0 = LAYER ? blockIdx.z * a.slice_passes : 0u;  // a slice: a run of whole passes
  const u32 pass1 = LAYER ? min(npass, pass0 + a.slice_passes) : npass;
  for (u32 pass = pass0; pass < pass1; pass++) {
    int oct = SPLIT > 1 ? (int)pass * PER_PASS + wave / SPLIT : ((int)pass * NW + wave) * RPW + sub;
    const bool ovalid = (u32)oct < O;
    if (!ovalid) oct = 0;
    sink.oct_i = (u32)oct;
    u16* const scale_out = reinterpret_cast<u16*>(blob + bo.scales) + ((long long)p * Tc + oct * 8);
    if (lmc_sym_nibbles(bins))
      quantize_task<G, NITER, DT, true, true, 8, 2, SPLIT, false, NHDB, FixedSink>(a.src, p, tok0, Tc, oct * 8, ovalid, true, e.C, maxf,
                                                                                   nullptr, nullptr, scale_out, sl, slice, xm, 0u, 0, &sink);
    else
      quantize_task<G, NITER, DT, true, false, 8, 2, SPLIT, false, NHDB, FixedSink>(a.src, p, tok0, Tc, oct * 8, ovalid, true, e.C, maxf,
                                                                                    nullptr, nullptr, scale_out, sl, slice, xm, 0u, 0, &sink);
    if constexpr (SPLIT > 1) __syncthreads();  // the next pass writes the exchange slots this one has read
  }
  if (sink.scs) __hip_atomic_fetch_add((LdsU32*)&scs_all, sink.scs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  __syncthreads();
  if constexpr (LAYER) {  // a slice of a layer-wise job: its sums are partials, and the first layer's launch clears the size word
    u32* const out = a.part + (((size_t)chunk * (u32)e.P + (u32)p) * gridDim.z + blockIdx.z) * (NG + 1u);
    if ((u32)tid <= NG) out[tid] = (u32)tid < NG ? chk[tid] : scs_all;
    if (tid == 0 && e.sizes && blockIdx.x == 0 && blockIdx.z == 0) e.sizes[chunk] = 0u;
    return;
  }
  if ((u32)tid < NG) {  // tails and directory entries of the plane's streams
    u8* const sb = sink.plane_streams + (size_t)tid * ssize;
    *(LMC_GLOBAL u32x4_t*)(sb + ssize - LMC_FIXED_TAIL_BYTES) = u32x4_t{chk[tid], 0u, 0u, 0u};
    const u32 b0 = beg + (u32)tid * ssize;
    *(LMC_GLOBAL u32x2_t*)(blob + bo.gdir + 8u * ((u32)p * NG + (u32)tid)) = u32x2_t{b0, b0 + ssize};
  }
  if (tid == 0) reinterpret_cast<u32*>(blob + bo.scsum)[p] = scs_all;
  if (p == 0 && wave == NW - 1) {  // (the last wave: not the one that stores the tails)
    write_blob_static(blob, bo, e, (u32)Tc, total, lane);
    if (lane == 22) reinterpret_cast<u32*>(blob)[22] = LMC_MODEL_FIXED;  // (the lane that wrote the coded models' word)
    if (lane == 0 && e.sizes) e.sizes[chunk] = bo.streams + total;
  }
}

// ---- k_fixed_layers_finish: the tail of a layer-wise job, a workgroup per chunk ------------------------------------------
// Sums the slices' partials of every (plane, stream) and writes what k_fixed_encode writes behind its plane loop: the
// 16-byte tail {check, 0, 0, 0} and the directory entry of each stream, scsum[p], header, bins and pads, the model word
// and -- last, behind a barrier -- sizes[chunk].  P * (G + 1) * slices dwords read and a few tens of bytes per stream
// written: nothing of the streams or the scales moves.
struct FixedFinishArgs {
  EncodeArgs e;
  const u32* part;  // [nchunks][P][nslices][G + 1]
  u32 nslices;
};

#define FIXED_FIN_THREADS 256
__global__ __launch_bounds__(FIXED_FIN_THREADS) void k_fixed_layers_finish(FixedFinishArgs a) {
  __shared__ u32 pbeg[LMC_MAX_PLANES + 1];  // a plane's first stream in the streams section; [P]: the section's bytes
  const EncodeArgs& e = a.e;
  const int tid = (int)threadIdx.x, lane = tid & 63, chunk = (int)blockIdx.x;
  const int Tc = min(e.chunk_tokens, e.tok_end - (e.tok_begin + chunk * e.chunk_tokens));
  const u32 O = ((u32)Tc + 7u) >> 3, NG = (u32)e.G, P = (u32)e.P;
  const BlobOff bo = lmc_blob_off(P, (u32)Tc, NG);
  u8* const blob = e.blobs + (long long)chunk * e.blob_stride;
  for (u32 q = (u32)tid; q <= P; q += FIXED_FIN_THREADS) {
    u32 beg = 0;
    for (u32 r = 0; r < q; r++) beg += NG * fixed_stream_bytes_dev((u32)e.bins.b[r], O);
    pbeg[q] = beg;
  }
  __syncthreads();
  const u32 total = pbeg[P];
  for (u32 i = (u32)tid; i < P * (NG + 1u); i += FIXED_FIN_THREADS) {
    const u32 p = i / (NG + 1u), k = i - p * (NG + 1u);
    const u32* const in = a.part + ((size_t)chunk * P + p) * a.nslices * (NG + 1u) + k;
    u32 sum = 0;
    for (u32 s = 0; s < a.nslices; s++) sum += in[(size_t)s * (NG + 1u)];
    if (k < NG) {
      const u32 ssize = fixed_stream_bytes_dev((u32)e.bins.b[p], O);
      const u32 b0 = pbeg[p] + k * ssize;
      *(LMC_GLOBAL u32x4_t*)(blob + bo.streams + b0 + ssize - LMC_FIXED_TAIL_BYTES) = u32x4_t{sum, 0u, 0u, 0u};
      *(LMC_GLOBAL u32x2_t*)(blob + bo.gdir + 8u * (p * NG + k)) = u32x2_t{b0, b0 + ssize};
    } else {
      reinterpret_cast<u32*>(blob + bo.scsum)[p] = sum;
    }
  }
  if (tid >= FIXED_FIN_THREADS - 64) {  // the last wave
    write_blob_static(blob, bo, e, (u32)Tc, total, lane);
    if (lane == 22) reinterpret_cast<u32*>(blob)[22] = LMC_MODEL_FIXED;  // (the lane that wrote the coded models' word)
  }
  __syncthreads();
  if (tid == 0) e.sizes[chunk] = bo.streams + total;
}

struct FixedDecArgs {
  DecodeArgs d;
  int vec;  // the destination's rows take 16-byte stores of 8 channels (what the encoders ask of a source)
};

#define FIXED_DEC_WAVES 4
#define FIXED_DEC_WAVE_DWORDS (256 + 64 + 32 + 32)  // lo tile | hi tile | scales of the tile's tokens | LUT

template <int DT_OUT, int KIND>
__global__ __launch_bounds__(64 * FIXED_DEC_WAVES) void k_fixed_decode(FixedDecArgs fa) {
  static_assert(!lmc_dtype_fp8(DT_OUT), "16-bit elements");
  constexpr bool SPLIT = KIND == DEC_PAGED_SPLIT;
  __shared__ __attribute__((aligned(16))) u32 lds_all[FIXED_DEC_WAVES * FIXED_DEC_WAVE_DWORDS];
  const DecodeArgs& a = fa.d;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const u32 gid = blockIdx.x * (u32)FIXED_DEC_WAVES + (u32)wave;
  const int n = 2 * a.layer_count * a.wGw;  // streams of a chunk in this launch (wGw: the groups its head window touches)
  if (gid >= (u32)a.nchunks * (u32)n) return;
  u32* const lo_t = lds_all + wave * FIXED_DEC_WAVE_DWORDS;
  u32* const hi_t = lo_t + 256;
  float* const sc_t = reinterpret_cast<float*>(hi_t + 64);
  float* const lut = sc_t + 32;
  const int chunk = (int)(gid / (u32)n);
  const int r = (int)(gid - (u32)chunk * (u32)n);
  const int pidx = r / a.wGw, g = a.wg_lo + r - pidx * a.wGw;  // (a.C, a.G and the directory index are the blob's)
  const int p = pidx < a.layer_count ? a.layer_begin + pidx : (a.P >> 1) + a.layer_begin + pidx - a.layer_count;
  const u8* const blob = a.blob_ptrs ? (const u8*)uniform_ptr(a.blob_ptrs[chunk]) : a.blobs + (long long)chunk * a.blob_stride;
  auto fail = [&](u32 bit) { if (lane == 0) atomicOr(a.status, bit); };

  // ---- header (the host has seen to it that 128 bytes may be read) -----------------------------------------------------
  const u32 hv = ((const LMC_GLOBAL u32*)blob)[lane & 31];
  auto hdw = [&](int i) { return (u32)__builtin_amdgcn_readlane((int)hv, i); };
  const u32 T = hdw(4), src_dtype = hdw(2);
  const BlobOff bo = lmc_blob_off((u32)a.P, T, (u32)a.G);
  if (hdw(0) != LMC_BLOB_MAGIC || (hdw(1) & 0xffffu) != LMC_BLOB_VERSION || hdw(7) != (u32)a.C || T == 0u || T > 65535u ||
      T > (u32)a.chunk_tokens || hdw(8) != (u32)a.P || hdw(22) != LMC_MODEL_FIXED || hdw(15) != bo.streams ||
      (a.w_src_heads != 0 && (hdw(5) != (u32)a.w_src_heads || hdw(6) != (u32)a.dst.D)) ||  // a head window: the blob's heads
      (src_dtype != (u32)LMC_DTYPE_BF16 && src_dtype != (u32)LMC_DTYPE_FP16) ||
      (unsigned long long)hdw(15) + (unsigned long long)hdw(16) != (unsigned long long)hdw(17) ||
      (unsigned long long)hdw(17) > (unsigned long long)a.blob_stride) {
    return fail(LMC_ST_BAD_HEADER);
  }
  // ---- the layout the bins say (they lie in front of off_streams <= total_bytes <= the blob's room) -------------------
  const u32 O = (T + 7u) >> 3;
  u32 mine = 0, before = 0;
  bool bad = false;
  for (int q = lane; q < a.P; q += 64) {
    const u32 b = (u32)((const LMC_GLOBAL u8*)blob)[LMC_HEADER_BYTES + q];
    bad = bad || b < 4u || b > (u32)LMC_MAX_BINS;
    const u32 sz = (u32)a.G * fixed_stream_bytes_dev(b, O);
    mine += sz;
    if (q < p) before += sz;
  }
  const u32 total = wave_sum_u32(mine);
  const u32 pbeg = wave_sum_u32(before);
  const u32 bins_p = (u32)__builtin_amdgcn_readfirstlane((int)(u32)((const LMC_GLOBAL u8*)blob)[LMC_HEADER_BYTES + p]);
  const u32 ssize = fixed_stream_bytes_dev(bins_p, O);
  const u32 beg = pbeg + (u32)g * ssize;
  const u32x2_t gd = *(const LMC_GLOBAL u32x2_t*)(blob + bo.gdir + 8u * (u32)(p * a.G + g));
  if (__ballot(bad) != 0ull || total != hdw(16) || (u32)__builtin_amdgcn_readfirstlane((int)gd.x) != beg ||
      (u32)__builtin_amdgcn_readfirstlane((int)gd.y) != beg + ssize) {
    return fail(LMC_ST_BAD_HEADER);
  }
  const u8* const sbytes = blob + bo.streams + beg;  // beg + ssize <= total: inside the blob
  const bool wide = bins_p > LMC_FIXED_NARROW_BINS;  // (wave-uniform)

  const u16* const scl = reinterpret_cast<const u16*>(blob + bo.scales) + (long long)p * T;
  if (g == a.wg_lo) {  // the plane's first wave of the launch checks the scales (k_decode.h: the others do not wait for the verdict)
    const u32 want = (u32)__builtin_amdgcn_readfirstlane((int)((const LMC_GLOBAL u32*)(blob + bo.scsum))[p]);
    if (scale_checksum(scl, T, lane) != want) return fail(LMC_ST_BAD_SCALES);
  }
  if (lane < 32) {  // (q - C) / C, k_decode.h's table
    const float Cf = (float)((int)bins_p / 2 - 1);
    const float v = (float)lane - Cf;
    lut[lane] = v / Cf;
  }

  // ---- destination ---------------------------------------------------------------------------------------------------
  typedef typename KvElem<DT_OUT>::T E;
  // Head window (DecodeArgs): channels [wc_lo, wc_hi) of the blob are stored, head h as head h + wh_shift of dst.  There is
  // no dependency between lanes here, so a lane outside the window skips its stores; every lane still takes part in the
  // loads, which the stream's check word is summed over.  The window's edges are multiples of D: where D % 8 == 0 a lane's
  // 8 (V: 4) channels lie on one side of an edge and the 16-byte forms stay; otherwise the rows are not `vec` and the
  // element path asks channel by channel.
  const int cj = lane & 7, tj = lane >> 3;
  const int c0 = g * 64 + 8 * cj;
  auto in_win = [&](int c) { return c >= a.wc_lo && c < a.wc_hi; };  // (wc_hi <= C)
  const bool cok = (fa.vec || SPLIT) ? in_win(c0) : c0 < a.C;  // (element rows: per channel below; lmc_api.hip leaves `vec` off for a window of heads with D % 8 != 0)
  E* const pbase = const_cast<E*>(lmc_plane_base<E>(a.dst, p));
  const int h0s = c0 / a.dst.D, d0 = c0 - h0s * a.dst.D, h0 = h0s + a.wh_shift;
  const long long coff = (long long)h0 * a.dst.stride_head + d0;  // vec: the 8 channels are contiguous from here
  // LMC_PAGED_SPLIT (k_quantize.h has the two address forms): the block offset is 64-bit, the lane's part 32-bit (lmc_api.hip,
  // decode_dst_ok).  A key plane: the lane's 8 channels are one x-granule, x = 8 (head_size is whole granules).  A value
  // plane: the lane keeps what it loaded, the eight tokens of oct lane >> 4 for the four channels vc0 .. vc0 + 3 (one head:
  // head_size % 8 == 0), each channel's eight slots 16 contiguous bytes where the oct lies as the encoder's V form asks.
  const bool is_v = SPLIT && p >= a.dst.L;  // (wave-uniform)
  const u32 bs = (u32)a.dst.block_size;
  const bool aligned = SPLIT && ((((uintptr_t)pbase) & 15u) | (uintptr_t)((a.dst.stride_block | a.dst.stride_head) & 7)) == 0;
  const u32 k_in = (u32)h0 * (u32)a.dst.stride_head + ((u32)d0 >> 3) * (bs * 8u);
  const int vc0 = g * 64 + 4 * (lane & 15);
  const bool vcok = in_win(vc0);
  const int vhs = vc0 / a.dst.D, vh = vhs + a.wh_shift;
  const u32 v_in = (u32)vh * (u32)a.dst.stride_head + (u32)(vc0 - vhs * a.dst.D) * bs;
  const int tdst0 = a.dst_tok0 + chunk * a.chunk_tokens;
  const u32 sh = 8u * ((u32)tj & 3u) + 4u * ((u32)tj >> 2);

  const LMC_GLOBAL u32x4_t* const lo_g = (const LMC_GLOBAL u32x4_t*)sbytes;
  const LMC_GLOBAL u32* const hi_g = (const LMC_GLOBAL u32*)(sbytes + 256u * (size_t)O);
  const u32 ntile = (O + 3u) >> 2;
  u32 acc = 0;
  struct Tile { u32x4_t lo; u32 hi; u32 sc; };
  auto load_tile = [&](u32 tile) -> Tile {
    Tile t;
    const bool in = tile * 4u + ((u32)lane >> 4) < O;
    t.lo = in ? __builtin_nontemporal_load(lo_g + (tile * 64u + (u32)lane)) : u32x4_t{0u, 0u, 0u, 0u};
    t.hi = (wide && in) ? __builtin_nontemporal_load(hi_g + (tile * 64u + (u32)lane)) : 0u;
    const u32 tt = tile * 32u + (u32)lane;
    t.sc = (lane < 32 && tt < T) ? (u32)scl[tt] : 0u;
    return t;
  };
  Tile cur = load_tile(0);
  for (u32 tile = 0; tile < ntile; tile++) {
    {  // the check word over exactly what was loaded; then the tile goes to LDS as it lies in the stream
      const u32 i0 = tile * 256u + 4u * (u32)lane;
      acc += (2u * i0 + 1u) * cur.lo.x + (2u * i0 + 3u) * cur.lo.y + (2u * i0 + 5u) * cur.lo.z + (2u * i0 + 7u) * cur.lo.w;
      acc += (2u * (64u * O + tile * 64u + (u32)lane) + 1u) * cur.hi;
      if (!is_v) {
        *reinterpret_cast<u32x4_t*>(lo_t + 4 * lane) = cur.lo;
        hi_t[lane] = cur.hi;
      }
      if (lane < 32) sc_t[lane] = h2f_rt(cur.sc, (int)src_dtype);
    }
    wave_lds_fence();
    const Tile mine = cur;
    if (tile + 1u < ntile) cur = load_tile(tile + 1u);  // in flight while this tile is stored
    if constexpr (SPLIT) {
      if (is_v) {
        // the lane's oct: slots of its live tokens only (t < T, not trimmed), and nothing of a token that is not live
        const u32 oo = (u32)lane >> 4, t0 = (tile * 4u + oo) * 8u;
        bool live[8], all = vcok, any = false;
        u32 sl[8];
#pragma unroll
        for (int r = 0; r < 8; r++) {
          live[r] = vcok && t0 + (u32)r < T && tdst0 + (int)(t0 + (u32)r) >= 0;
          sl[r] = live[r] ? (u32)a.dst.slot_mapping[tdst0 + (int)(t0 + (u32)r)] : 0u;
          all = all && live[r];
          any = any || live[r];
        }
        const u32 b0 = sl[0] / bs, w0 = sl[0] - b0 * bs;
        bool run = all && aligned && (w0 & 7u) == 0u && (bs & 7u) == 0u;
#pragma unroll
        for (int r = 1; r < 8; r++) run = run && sl[r] == sl[0] + (u32)r;
        const u32 lw[4] = {mine.lo.x, mine.lo.y, mine.lo.z, mine.lo.w};
        u32 bits[4][8];
#pragma unroll
        for (int r = 0; r < 8; r++) {
          const float scale = sc_t[oo * 8u + (u32)r];
#pragma unroll
          for (int e = 0; e < 4; e++) {
            u32 q = (lw[e] >> (8u * ((u32)r & 3u) + 4u * ((u32)r >> 2))) & 15u;
            if (wide) q |= ((mine.hi >> (8u * (u32)e + (u32)r)) & 1u) << 4;
            float val = lut[q] * scale;
            if constexpr (DT_OUT == LMC_DTYPE_BF16) bits[e][r] = (u32)__builtin_bit_cast(unsigned short, (__bf16)val);
            else {
              asm volatile("" : "+v"(val));  // two roundings, as in the rows
              bits[e][r] = f2fp16(val);
            }
          }
        }
        if (__ballot(any && !run) == 0ull) {  // every oct of the tile that writes at all is a whole aligned run
          if (run) {
            LMC_GLOBAL u16* const blk = (LMC_GLOBAL u16*)(pbase + (long long)b0 * a.dst.stride_block);
#pragma unroll
            for (int e = 0; e < 4; e++)
              *(LMC_GLOBAL u32x4_t*)(blk + (v_in + (u32)e * bs + w0)) = u32x4_t{bits[e][0] | (bits[e][1] << 16), bits[e][2] | (bits[e][3] << 16),
                                                                               bits[e][4] | (bits[e][5] << 16), bits[e][6] | (bits[e][7] << 16)};
          }
        } else {
#pragma unroll
          for (int r = 0; r < 8; r++) {
            if (!live[r]) continue;
            const u32 br = sl[r] / bs, wr = sl[r] - br * bs;
            LMC_GLOBAL u16* const blk = (LMC_GLOBAL u16*)(pbase + (long long)br * a.dst.stride_block);
#pragma unroll
            for (int e = 0; e < 4; e++) blk[v_in + (u32)e * bs + wr] = (u16)bits[e][r];
          }
        }
        wave_lds_fence();  // the scales have been read
        continue;
      }
    }
    const u32 noct = min(4u, O - tile * 4u);
    for (u32 oo = 0; oo < noct; oo++) {
      const u32 t = (tile * 4u + oo) * 8u + (u32)tj;
      const int tdst = tdst0 + (int)t;
      const bool ok = cok && t < T && tdst >= 0;
      const u32x4_t wa = *reinterpret_cast<const u32x4_t*>(lo_t + oo * 64u + 8u * (u32)cj);
      const u32x4_t wb = *reinterpret_cast<const u32x4_t*>(lo_t + oo * 64u + 8u * (u32)cj + 4u);
      const u32x2_t hb = *reinterpret_cast<const u32x2_t*>(hi_t + oo * 16u + 2u * (u32)cj);
      const float scale = sc_t[oo * 8u + (u32)tj];
      const u32 w[8] = {wa.x, wa.y, wa.z, wa.w, wb.x, wb.y, wb.z, wb.w};
      u32 bits[8];
#pragma unroll
      for (int e = 0; e < 8; e++) {
        u32 q = (w[e] >> sh) & 15u;
        if (wide) q |= ((((e < 4 ? hb.x : hb.y) >> (8 * (e & 3))) >> (u32)tj) & 1u) << 4;
        float val = lut[q] * scale;
        if constexpr (DT_OUT == LMC_DTYPE_BF16) bits[e] = (u32)__builtin_bit_cast(unsigned short, (__bf16)val);
        else {
          asm volatile("" : "+v"(val));  // the product is rounded to fp32 first, to fp16 second (k_decode.h)
          bits[e] = f2fp16(val);
        }
      }
      if constexpr (SPLIT) {
        if (ok) {
          LMC_GLOBAL u16* const gp = (LMC_GLOBAL u16*)(pbase + dec_tok_off_split(a.dst, tdst, 8u)) + k_in;
          if (aligned) {
            *(LMC_GLOBAL u32x4_t*)gp = u32x4_t{bits[0] | (bits[1] << 16), bits[2] | (bits[3] << 16), bits[4] | (bits[5] << 16), bits[6] | (bits[7] << 16)};
          } else {
#pragma unroll
            for (int e = 0; e < 8; e++) gp[e] = (u16)bits[e];
          }
        }
      } else if (ok) {
        const long long toff = KIND == DEC_ROWS ? (long long)tdst * a.dst.stride_token : dec_tok_off(a.dst, tdst);
        if (fa.vec) {
          const u32x4_t v = {bits[0] | (bits[1] << 16), bits[2] | (bits[3] << 16), bits[4] | (bits[5] << 16), bits[6] | (bits[7] << 16)};
          __builtin_nontemporal_store(v, (LMC_GLOBAL u32x4_t*)(pbase + toff + coff));
        } else {
#pragma unroll
          for (int e = 0; e < 8; e++) {
            const int c = c0 + e, hs = c / a.dst.D, d = c - hs * a.dst.D;
            if (in_win(c)) *((LMC_GLOBAL u16*)(pbase + toff + (long long)(hs + a.wh_shift) * a.dst.stride_head + d)) = (u16)bits[e];
          }
        }
      }
    }
    wave_lds_fence();  // the tile has been read: the next one may take its place
  }
  const u32 got = wave_sum_u32(acc);
  const u32 tw = lane < 4 ? ((const LMC_GLOBAL u32*)(sbytes + ssize - LMC_FIXED_TAIL_BYTES))[lane] : 0u;
  if (__ballot(lane < 4 && tw != (lane == 0 ? got : 0u)) != 0ull) fail(LMC_ST_BAD_STREAM);
}

// ---- k_fixed_expand: fixed-width blobs -> what k_quantize<true> leaves for the same chunks ----------------------------
// The first kernel of lmc_transcode_fixed (lmc_api.hip): it stands where k_quantize stands in the two-kernel encode and
// k_cdf_encode runs behind it unchanged, so a fixed-width blob becomes the entropy-coded blob of the same KV without the
// KV.  Per (chunk, plane) it fills the symbol workspace, copies the plane's scales into the output blob, and clears the
// job's look-back granules and size words.
// Mapping: k_fixed_decode's -- a wave takes a stream and walks it in tiles of four octs, lane = (oct tile * 4 + lane / 16,
// channels 4 (lane & 15) .. + 3): one 16-byte non-temporal load of `lo`, a dword of `hi`, the next tile's loads in flight
// while this one is stored.  No LDS: the lane that loaded a dword owns every bit of its four channels for the oct.
//   narrow plane   the `lo` vector IS the workspace's four dwords of (oct, channels): one 16-byte store
//   wide plane     byte k of quad dword 2 oct + j = nibble of token 4 j + k | bit 4 from `hi`: two 16-byte stores
// Plain stores: the coder reads the workspace next (k_quantize's stores carry no hint either).  The SET of dwords written
// is quantize_task's: every oct below ceil(TQ / 2), those past the chunk's own (a ragged last chunk in a job of longer
// chunks) as zeros, and quad 2 oct + 1 only where it lies below TQ.  Bytes of tokens at or past T -- inside the last oct
// whatever the blob holds there, zeros in the octs behind it -- are never read by the coder (k_quantize.h says the same
// of its own), so they are not part of what the two kernels have to agree on.
// Validation: k_fixed_decode's checks in its order, plus what a transcode adds -- pointer and room before the header is
// read (lmc_pack_blobs's rule), L / H / D / dtype and T against the call's (the coder writes the new header from the
// call's), the blob's bins against the call's (the coder takes them from BinsArg).  A wave that fails sets the job's
// status word and stores ZEROS for its whole stream: the coder behind it must never meet bytes nobody wrote (a fresh
// workspace) or a symbol of 32 and more -- its histogram is [32][lane].
struct FixedExpandArgs {
  const u8* const* blob_ptrs;  // device [nchunks]: the fixed-width blob of chunk i
  const u32* blob_bytes;       // device [nchunks]: how far it may be read
  int tok_begin, tok_end, chunk_tokens, nchunks;
  int P, C, G, TQ;
  int L, H, D, dtype;
  u32* sym4;             // symbol workspace, region (chunk, plane) at (chunk * P + plane) * sym_stride
  long long sym_stride;
  u8* scale_base;        // QuantArgs: scale of (chunk, p, t) at scale_base + chunk * scale_stride + 2 * (p * Tc + t)
  long long scale_stride;
  unsigned long long* agg;  // QuantArgs: zeroed here, [agg_n]
  long long agg_n;
  u32* sizes;               // ... and the job's size words [nchunks]
  u32* status;
  BinsArg bins;
};

#define FIXED_EXP_WAVES 4

// bit r of the low four bits of n -> bit 0 of byte r (7 r + r = 8 r; the products' bit positions are all distinct)
__device__ __forceinline__ u32 fixed_spread4(u32 n) { return ((n & 15u) * 0x00204081u) & 0x01010101u; }

__global__ __launch_bounds__(64 * FIXED_EXP_WAVES) void k_fixed_expand(FixedExpandArgs a) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const u32 gid = blockIdx.x * (u32)FIXED_EXP_WAVES + (u32)wave;  // (the grid is below 2^30 workgroups: lmc_api.hip)
  const int n = a.P * a.G;  // streams of a chunk
  if ((unsigned long long)gid >= (unsigned long long)a.nchunks * (unsigned long long)n) return;
  if (lane == 0) {  // the job words k_quantize clears: a launch has a wave per granule
    if (a.agg && (long long)gid < a.agg_n) a.agg[gid] = 0ull;
    if (a.sizes && gid < (u32)a.nchunks) a.sizes[gid] = 0u;
  }
  const int chunk = (int)(gid / (u32)n);
  const int r = (int)(gid - (u32)chunk * (u32)n);
  const int p = r / a.G, g = r - p * a.G;
  const u32 Tc = (u32)min(a.chunk_tokens, a.tok_end - (a.tok_begin + chunk * a.chunk_tokens));
  const u32 TQ = (u32)a.TQ, TO = (TQ + 1u) >> 1;
  const bool wide = !lmc_sym_nibbles((int)a.bins.b[p]);  // (wave-uniform; the blob's bins are held against these below)
  u32* const ws = a.sym4 + ((long long)chunk * a.P + p) * a.sym_stride;
  const u32 c4 = (u32)g * 64u + 4u * ((u32)lane & 15u);
  const bool cok = c4 < (u32)a.C;
  const u32 ntile = (TO + 3u) >> 2;
  // the lane's oct of a tile into the workspace
  auto store_oct = [&](u32 o, const u32x4_t& lo, u32 hi) {
    if (!cok || o >= TO) return;
    if (!wide) {
      *(LMC_GLOBAL u32x4_t*)(ws + (size_t)o * (u32)a.C + c4) = lo;
      return;
    }
    const u32 w[4] = {lo.x, lo.y, lo.z, lo.w};
    u32 q0[4], q1[4];
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const u32 hb = hi >> (8 * e);
      q0[e] = (w[e] & 0x0f0f0f0fu) | (fixed_spread4(hb) << 4);
      q1[e] = ((w[e] >> 4) & 0x0f0f0f0fu) | (fixed_spread4(hb >> 4) << 4);
    }
    *(LMC_GLOBAL u32x4_t*)(ws + (size_t)(2u * o) * (u32)a.C + c4) = u32x4_t{q0[0], q0[1], q0[2], q0[3]};
    if (2u * o + 1u < TQ) *(LMC_GLOBAL u32x4_t*)(ws + (size_t)(2u * o + 1u) * (u32)a.C + c4) = u32x4_t{q1[0], q1[1], q1[2], q1[3]};
  };
  auto fail = [&](u32 bit) {
    if (lane == 0) atomicOr(a.status, bit);
    for (u32 tile = 0; tile < ntile; tile++) store_oct(tile * 4u + ((u32)lane >> 4), u32x4_t{0u, 0u, 0u, 0u}, 0u);
  };

  // ---- pointer and room, then the header ------------------------------------------------------------------------------
  const u8* const blob = (const u8*)uniform_ptr(a.blob_ptrs[chunk]);
  const u32 room = (u32)__builtin_amdgcn_readfirstlane((int)a.blob_bytes[chunk]);
  if (!blob || ((u64)(uintptr_t)blob & 15ull) || room < LMC_HEADER_BYTES) return fail(LMC_ST_BAD_HEADER);
  const u32 hv = ((const LMC_GLOBAL u32*)blob)[lane & 31];
  auto hdw = [&](int i) { return (u32)__builtin_amdgcn_readlane((int)hv, i); };
  const u32 T = hdw(4);
  const BlobOff bo = lmc_blob_off((u32)a.P, T, (u32)a.G);
  if (hdw(0) != LMC_BLOB_MAGIC || (hdw(1) & 0xffffu) != LMC_BLOB_VERSION || hdw(7) != (u32)a.C || T == 0u || T > 65535u ||
      T != Tc || hdw(8) != (u32)a.P || hdw(22) != LMC_MODEL_FIXED || hdw(15) != bo.streams || hdw(2) != (u32)a.dtype ||
      hdw(3) != (u32)a.L || hdw(5) != (u32)a.H || hdw(6) != (u32)a.D ||
      (unsigned long long)hdw(15) + (unsigned long long)hdw(16) != (unsigned long long)hdw(17) ||
      (unsigned long long)hdw(17) > (unsigned long long)room) {
    return fail(LMC_ST_BAD_HEADER);
  }
  // ---- the bins (they lie in front of off_streams <= total_bytes <= room): the call's, and the layout they give ---------
  const u32 O = (T + 7u) >> 3;
  const u32 bw = 4 * lane < a.P ? ((const LMC_GLOBAL u32*)(blob + LMC_HEADER_BYTES))[lane] : 0u;  // lane = four planes' bins
  bool bad = false;
  for (int j = 0; 4 * j < a.P; j++) {  // (wave-uniform: scalar loads of the call's, a readlane of the blob's)
    u32 want;
    __builtin_memcpy(&want, a.bins.b + 4 * j, 4);
    const u32 mask = a.P - 4 * j >= 4 ? 0xffffffffu : (1u << (8 * (a.P - 4 * j))) - 1u;
    bad = bad || (((u32)__builtin_amdgcn_readlane((int)bw, j) ^ want) & mask) != 0u;
  }
  u32 nwide = 0, nwide_before = 0;
  for (int q0 = 0; q0 < a.P; q0 += 64) {
    const int q = q0 + lane;
    const u32 b = ((u32)__shfl((int)bw, q >> 2) >> (8 * (q & 3))) & 0xffu;
    const u64 m = __ballot(q < a.P && b > LMC_FIXED_NARROW_BINS);
    const int below = p - q0;  // planes of this round that lie in front of p
    nwide += (u32)__builtin_popcountll(m);
    nwide_before += (u32)__builtin_popcountll(below >= 64 ? m : below <= 0 ? 0ull : m & ((1ull << below) - 1ull));
  }
  // lmc_fixed_stream_bytes summed: 256 O + 16 per stream, 64 O more per wide one (the host has seen to it that the
  // call's geometry and bins stay below 2^32)
  const u32 total = (u32)a.G * ((256u * O + LMC_FIXED_TAIL_BYTES) * (u32)a.P + 64u * O * nwide);
  const u32 pbeg = (u32)a.G * ((256u * O + LMC_FIXED_TAIL_BYTES) * (u32)p + 64u * O * nwide_before);
  const u32 ssize = (wide ? 320u : 256u) * O + LMC_FIXED_TAIL_BYTES;
  const u32 beg = pbeg + (u32)g * ssize;
  if (bad || total != hdw(16)) return fail(LMC_ST_BAD_HEADER);  // (the directory lies in front of off_streams too)
  const u32x2_t gd = *(const LMC_GLOBAL u32x2_t*)(blob + bo.gdir + 8u * (u32)(p * a.G + g));
  if ((u32)__builtin_amdgcn_readfirstlane((int)gd.x) != beg || (u32)__builtin_amdgcn_readfirstlane((int)gd.y) != beg + ssize)
    return fail(LMC_ST_BAD_HEADER);
  const u8* const sbytes = blob + bo.streams + beg;  // beg + ssize <= total: inside the blob

  if (g == 0) {  // the plane's first wave: the scales into the new blob, summed on the way
    const u16* const scl = reinterpret_cast<const u16*>(blob + bo.scales) + (size_t)p * T;
    u16* const out = reinterpret_cast<u16*>(a.scale_base + (long long)chunk * a.scale_stride) + (size_t)p * T;
    const u32 want = (u32)__builtin_amdgcn_readfirstlane((int)((const LMC_GLOBAL u32*)(blob + bo.scsum))[p]);
    u32 acc = 0;
    for (u32 t = (u32)lane; t < T; t += 64) {
      const u32 v = (u32)scl[t];
      acc += (t + 1u) * (v + 1u);  // lmc_scale_checksum_term
      out[t] = (u16)v;
    }
    if (wave_sum_u32(acc) != want) return fail(LMC_ST_BAD_SCALES);
  }

  // ---- the stream -------------------------------------------------------------------------------------------------------
  const LMC_GLOBAL u32x4_t* const lo_g = (const LMC_GLOBAL u32x4_t*)sbytes;
  const LMC_GLOBAL u32* const hi_g = (const LMC_GLOBAL u32*)(sbytes + 256u * (size_t)O);
  struct Tile { u32x4_t lo; u32 hi; };
  auto load_tile = [&](u32 tile) -> Tile {
    Tile t;
    const bool in = tile * 4u + ((u32)lane >> 4) < O;
    t.lo = in ? __builtin_nontemporal_load(lo_g + (tile * 64u + (u32)lane)) : u32x4_t{0u, 0u, 0u, 0u};
    t.hi = (wide && in) ? __builtin_nontemporal_load(hi_g + (tile * 64u + (u32)lane)) : 0u;
    return t;
  };
  u32 acc = 0;
  Tile cur = load_tile(0);
  for (u32 tile = 0; tile < ntile; tile++) {  // (O <= TO: the octs behind the chunk's own are stored as zeros)
    const Tile mine = cur;
    if (tile + 1u < ntile) cur = load_tile(tile + 1u);  // in flight while this tile is stored
    const u32 i0 = tile * 256u + 4u * (u32)lane;  // the check word over exactly what was loaded
    acc += (2u * i0 + 1u) * mine.lo.x + (2u * i0 + 3u) * mine.lo.y + (2u * i0 + 5u) * mine.lo.z + (2u * i0 + 7u) * mine.lo.w;
    acc += (2u * (64u * O + tile * 64u + (u32)lane) + 1u) * mine.hi;
    store_oct(tile * 4u + ((u32)lane >> 4), mine.lo, mine.hi);
  }
  const u32 got = wave_sum_u32(acc);
  const u32 tw = lane < 4 ? ((const LMC_GLOBAL u32*)(sbytes + ssize - LMC_FIXED_TAIL_BYTES))[lane] : 0u;
  if (__ballot(lane < 4 && tw != (lane == 0 ? got : 0u)) != 0ull) fail(LMC_ST_BAD_STREAM);
}
