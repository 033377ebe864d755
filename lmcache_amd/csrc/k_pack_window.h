// k_pack_window.h -- a head window retrieved from the pinned tier: only the window's streams of a pack cross PCIe.
//
// A head window (lmc_head_window) is a contiguous range of 64-channel groups wg_lo .. wg_lo + wGw - 1, and the streams of
// a plane lie in group order: the window of segment (plane, chunk) of a pack (lmc_format.h) is ONE contiguous run of
// bytes whose ends stand in the chunk's stream directory.  A 16 k context is 64 planes x 64 chunks = 4096 such runs of
// ~14 KB at one eighth of the heads: far too many for one hipMemcpyAsync each (~5 us of submission per copy), so
//
//   k_pack_window   a bounded grid of persistent workgroups walks the items (plane of the launch's range, chunk) and
//                   gathers each item's run out of the pack in MAPPED PINNED HOST memory into the context's load staging
//                   AT THE OFFSET THE BYTES HAVE IN THE PACK: k_decode's pack mode (seg_off / seg_streams / seg_n) then
//                   finds the window's streams where lmc_load_pack would have put them.  The rest of a segment is never
//                   written and never read.
//
// lmc_load_pack_heads (lmc_api.hip) has queued the DMA copies of the offset table and of the wanted chunks' static slots
// in front of the launch, on the same queue: directory and table are read from HBM, only stream bytes from the host.
//
// Every workgroup checks the WHOLE chunk before it reads one byte of the host pack for it (256 threads: a plane each) --
// unpack_chunk_ok's checks of the staged slot against the table, repeated here so that k_unpack stays the binary it is,
// and the window's own (it lies inside the plane's groups, its run inside the segment, on 16-byte boundaries).  A chunk
// that fails raises LMC_ST_BAD_HEADER once per launch and nothing of it is copied; its staged header is overwritten with
// one k_decode refuses, so that the decode behind the gather does not read the streams that were not written.
//
// The copy: a run is cut into 4 KiB pieces dealt round-robin to the workgroup's four waves; a wave has a piece's four
// 16-byte loads per lane in flight before its first store, so the four waves have 16 KiB -- a 14 KB run whole -- in
// flight over PCIe at once.  Loads and stores are non-temporal (the bytes are read once by k_decode, from HBM).
// Offsets into the pack are 64-bit.
#pragma once
#include "k_offload.h"

// Workgroups of a launch.  Bounded on purpose, not one per item: kernel-driven PCIe traffic from many workgroups slowed a
// concurrent decode step 4.3 x (lmc_hip.h, lmc_store_pack), and so does this kernel at the 64 workgroups k_pack_copy
// uses.  The gather's own time hardly depends on the grid from 16 workgroups up (16 x 16 KiB in flight cover the link's
// latency; 8 do not), what it does to a bandwidth-bound kernel beside it grows with every doubling: 16, the smallest
// grid at the DMA rate.  The sweep is in profiles/pack_window.md (-DPACK_WINDOW_WGS=n builds the others).
#ifndef PACK_WINDOW_WGS
#define PACK_WINDOW_WGS 16
#endif
#define PACK_WINDOW_PIECE16 256u  // 16-byte units of a piece: 4 KiB, four loads per lane of a wave

struct PackWindowArgs {
  const u8* pack_h;                  // the pack in mapped pinned host memory, by its device-visible address
  u8* stage;                         // load staging: table and static slots at their offsets in the pack; the runs go there too
  unsigned long long off_table, off_static, off_streams;  // of the pack (lmc_pack_header)
  unsigned long long streams_bytes;  // size of the pack's streams region (the host has checked it against the table)
  u32 static_stride;
  int n;                             // chunks of the pack
  int c0, m;                         // this job: chunks [c0, c0 + m)
  int L, G;
  u32 chunk_tokens;                  // of the pack: no chunk is longer
  int p0, np;                        // this launch: planes [p0, p0 + np)
  int wg_lo, wGw;                    // the window's groups
  u32* status;
};

// The window's run of plane p, relative to the chunk's streams section: [*wb, *we).  `gdir`: the chunk's directory,
// `pe` the plane's end (its successor's beg, or the section's size).
__device__ __forceinline__ void pack_window_run(const PackWindowArgs& a, const u32* gdir, int p, u32 pe, u32* wb, u32* we) {
  *wb = gdir[2 * (p * a.G + a.wg_lo)];
  *we = a.wg_lo + a.wGw < a.G ? gdir[2 * (p * a.G + a.wg_lo + a.wGw)] : pe;
}

// Does chunk c0 + j of the pack check out against its static slot, and the window against its directory?  Uniform over
// the workgroup (every thread returns the same answer).
__device__ __forceinline__ bool pack_window_chunk_ok(const PackWindowArgs& a, int j) {
  const int P = 2 * a.L;
  const u8* slot = a.stage + a.off_static + (unsigned long long)(a.c0 + j) * a.static_stride;
  const u32* hd = reinterpret_cast<const u32*>(slot);
  // the header: a v6 blob of the pack's geometry whose static sections fit the slot
  bool ok = hd[0] == LMC_BLOB_MAGIC && (hd[1] & 0xffffu) == LMC_BLOB_VERSION && hd[8] == (u32)P && hd[9] == (u32)a.G && hd[4] - 1u < a.chunk_tokens &&
            a.wg_lo >= 0 && a.wGw >= 1 && a.wg_lo + a.wGw <= a.G;
  const BlobOff bo = lmc_blob_off((u32)P, hd[4], (u32)a.G);  // the chunk's own length (a ragged last chunk is shorter)
  const u32 stream_bytes = hd[16];
  ok = ok && hd[14] == bo.gdir && hd[15] == bo.streams && bo.streams >= LMC_HEADER_BYTES && bo.streams <= a.static_stride &&
       (unsigned long long)bo.streams + stream_bytes <= 0xfffffff0ull && hd[17] == bo.streams + stream_bytes;
  // the directory against the pack's table, a plane per thread: plane p begins where the directory says, on a 16-byte
  // boundary, ends where its successor begins (the last one with the section), and has the length of its segment; the
  // window's run begins and ends inside it, on 16-byte boundaries
  int bad = 0;
  if (ok) {
    const u32* gdir = reinterpret_cast<const u32*>(slot + bo.gdir);
    const unsigned long long* table = reinterpret_cast<const unsigned long long*>(a.stage + a.off_table);
    for (int p = (int)threadIdx.x; p < P; p += 256) {
      const u32 s = gdir[2 * (p * a.G)];
      const u32 e = p + 1 < P ? gdir[2 * ((p + 1) * a.G)] : stream_bytes;
      const unsigned long long i = (unsigned long long)p * (unsigned long long)a.n + (unsigned long long)(a.c0 + j);
      const unsigned long long lo = table[i], hi = table[i + 1];
      u32 wb, we;
      pack_window_run(a, gdir, p, e, &wb, &we);
      bad |= (p == 0 && s != 0u) || e < s || e > stream_bytes || (s & 15u) || (e & 15u) || hi < lo || hi > a.streams_bytes ||
             hi - lo != (unsigned long long)(e - s) || wb < s || we < wb || we > e || (wb & 15u) || (we & 15u);
    }
  }
  return __syncthreads_or(bad || !ok) == 0;
}

// One piece of a run by one wave: lane l moves the 16-byte units l, l + 64, l + 128, l + 192 of [0, n16), n16 <= 256.
// The four loads are unconditional -- in the last piece of a run a unit past the end reads the piece's last unit again
// (n16 >= 1), inside the run -- so that all four are in flight before the first store whatever n16 is; the stores keep
// their bounds.
__device__ __forceinline__ void pack_window_piece(LMC_GLOBAL u32x4_t* d, const LMC_GLOBAL u32x4_t* s, u32 n16, u32 lane) {
  const u32 last = n16 - 1u;
  const u32x4_t v0 = __builtin_nontemporal_load(s + min(lane, last)), v1 = __builtin_nontemporal_load(s + min(lane + 64u, last)),
                v2 = __builtin_nontemporal_load(s + min(lane + 128u, last)), v3 = __builtin_nontemporal_load(s + min(lane + 192u, last));
  if (n16 == PACK_WINDOW_PIECE16) {  // (wave-uniform: a whole piece stores without waiting between its stores)
    __builtin_nontemporal_store(v0, d + lane); __builtin_nontemporal_store(v1, d + lane + 64u);
    __builtin_nontemporal_store(v2, d + lane + 128u); __builtin_nontemporal_store(v3, d + lane + 192u);
    return;
  }
  if (lane < n16) __builtin_nontemporal_store(v0, d + lane);
  if (lane + 64u < n16) __builtin_nontemporal_store(v1, d + lane + 64u);
  if (lane + 128u < n16) __builtin_nontemporal_store(v2, d + lane + 128u);
  if (lane + 192u < n16) __builtin_nontemporal_store(v3, d + lane + 192u);
}

// grid = (workgroups <= PACK_WINDOW_WGS), 256 threads: workgroup w takes items w, w + gridDim.x, ... of np * m;
// item = pl * m + j: plane p0 + pl of chunk c0 + j.  (With gridDim.x a multiple of m -- a run of up to 16 chunks -- a
// workgroup stays with one chunk and checks it once.  Chunk-major blocks of items, one check per chunk whatever m is,
// were measured: no faster, and harder on a kernel running beside it -- profiles/pack_window.md.)
__global__ __launch_bounds__(256) void k_pack_window(PackWindowArgs a) {
  const int P = 2 * a.L;
  const int items = a.np * a.m;
  const u32 wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  int seen_j = -1;
  bool seen_ok = false;
  for (int item = (int)blockIdx.x; item < items; item += (int)gridDim.x) {
    const int pl = item / a.m, j = item - pl * a.m, p = a.p0 + pl;
    if (j != seen_j) {
      seen_ok = pack_window_chunk_ok(a, j);
      seen_j = j;
    }
    u8* slot = a.stage + a.off_static + (unsigned long long)(a.c0 + j) * a.static_stride;
    if (!seen_ok) {
      if (pl == 0 && threadIdx.x == 0) {  // once per chunk and launch
        atomicOr(a.status, LMC_ST_BAD_HEADER);
        // the decode behind this launch must not read what was not gathered: k_decode refuses a header without the magic
        // (every workgroup that checks this chunk reaches this verdict, with or without the store)
        *reinterpret_cast<volatile u32*>(slot) = 0u;
      }
      continue;
    }
    const BlobOff bo = lmc_blob_off((u32)P, reinterpret_cast<const u32*>(slot)[4], (u32)a.G);
    const u32* gdir = reinterpret_cast<const u32*>(slot + bo.gdir);
    const u32 s = gdir[2 * (p * a.G)];
    const u32 e = p + 1 < P ? gdir[2 * ((p + 1) * a.G)] : reinterpret_cast<const u32*>(slot)[16];
    u32 wb, we;
    pack_window_run(a, gdir, p, e, &wb, &we);
    const unsigned long long* table = reinterpret_cast<const unsigned long long*>(a.stage + a.off_table);
    const unsigned long long lo = table[(unsigned long long)p * (unsigned long long)a.n + (unsigned long long)(a.c0 + j)];
    const unsigned long long at = a.off_streams + lo + (unsigned long long)(wb - s);  // of the run, in the pack and in the staging
    const LMC_GLOBAL u32x4_t* src = reinterpret_cast<const LMC_GLOBAL u32x4_t*>((const LMC_GLOBAL u8*)(a.pack_h + at));
    LMC_GLOBAL u32x4_t* dst = reinterpret_cast<LMC_GLOBAL u32x4_t*>((LMC_GLOBAL u8*)(a.stage + at));
    const u32 n16 = (we - wb) >> 4;
    for (u32 k = wave * PACK_WINDOW_PIECE16; k < n16; k += 4u * PACK_WINDOW_PIECE16)
      pack_window_piece(dst + k, src + k, min(n16 - k, PACK_WINDOW_PIECE16), lane);
  }
}
