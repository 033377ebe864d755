// k_repack.h -- the promotion leg of the bounded local tiers: a pack (lmc_format.h) back into the blobs it was made of.
//
// The demotion leg needs no kernel of its own: lmc_pack_blobs runs k_pack_scan / k_pack_copy (k_offload.h) over a
// pointer table.  This is the inverse.  lmc_unpack_blobs (lmc_api.hip) has staged the pack's offset table, the static
// slots of the wanted chunks and their segments in device memory AT THE OFFSETS THEY HAVE IN THE PACK (as lmc_load_pack
// does for the decoder), and
//
//   k_unpack   a fixed number of workgroups walk the items (chunk, what), what = the static slot or one of the 2 L
//              planes, and copy each to its place in the chunk's blob: the slot's [0, off_streams) to the blob's head,
//              segment (p, chunk) to off_streams + beg of stream (p, 0) -- the slot's own stream directory says where.
//
// Every workgroup checks the WHOLE chunk before it writes one byte of it (256 threads: a plane each): a blob is written
// completely or not at all, whichever workgroup gets to it first.  Plain HBM copy: 16-byte non-temporal accesses, four
// loads in flight per thread; offsets into the pack are 64-bit (segment offsets pass 2^32 long before a blob's do).
#pragma once
#include "k_offload.h"

struct UnpackArgs {
  const u8* pack;                    // device staging: table, static slots and segments at their offsets in the pack
  unsigned long long off_table, off_static, off_streams;  // of the pack (lmc_pack_header)
  unsigned long long streams_bytes;  // size of the pack's streams region (the host has checked it against the table)
  u32 static_stride;
  int n;                             // chunks of the pack
  int c0, m;                         // this job: chunks [c0, c0 + m)
  int L, G;
  u32 chunk_tokens;                  // of the pack: no chunk is longer
  u8* const* dst_ptrs;               // device [m]: where blob c0 + j goes (16-byte aligned)
  const u32* dst_caps;               // device [m]: its room
  u32* status;
};

// Does chunk c0 + j of the pack check out against its static slot and fit its destination?  Uniform over the workgroup
// (every thread returns the same answer); *streams_off = the blob's off_streams.
__device__ __forceinline__ bool unpack_chunk_ok(const UnpackArgs& a, int j, u32* streams_off) {
  const int P = 2 * a.L;
  const u8* slot = a.pack + a.off_static + (unsigned long long)(a.c0 + j) * a.static_stride;
  const u32* hd = reinterpret_cast<const u32*>(slot);
  u8* dst = a.dst_ptrs[j];
  // the header: a v6 blob of the pack's geometry whose static sections fit the slot and whose total fits the room
  bool ok = hd[0] == LMC_BLOB_MAGIC && (hd[1] & 0xffffu) == LMC_BLOB_VERSION && hd[8] == (u32)P && hd[9] == (u32)a.G && hd[4] - 1u < a.chunk_tokens &&
            dst != nullptr && !((unsigned long long)(uintptr_t)dst & 15ull);
  const BlobOff bo = lmc_blob_off((u32)P, hd[4], (u32)a.G);  // the chunk's own length (a ragged last chunk is shorter)
  const u32 stream_bytes = hd[16];
  ok = ok && hd[14] == bo.gdir && hd[15] == bo.streams && bo.streams >= LMC_HEADER_BYTES && bo.streams <= a.static_stride &&
       (unsigned long long)bo.streams + stream_bytes <= 0xfffffff0ull && hd[17] == bo.streams + stream_bytes &&
       hd[17] <= a.dst_caps[j];
  *streams_off = bo.streams;
  // the directory against the pack's table, a plane per thread: plane p begins where the directory says, on a 16-byte
  // boundary, ends where its successor begins (the last one with the section), and has the length of its segment
  int bad = 0;
  if (ok) {
    const u32* gdir = reinterpret_cast<const u32*>(slot + bo.gdir);
    const unsigned long long* table = reinterpret_cast<const unsigned long long*>(a.pack + a.off_table);
    for (int p = (int)threadIdx.x; p < P; p += 256) {
      const u32 s = gdir[2 * (p * a.G)];
      const u32 e = p + 1 < P ? gdir[2 * ((p + 1) * a.G)] : stream_bytes;
      const unsigned long long i = (unsigned long long)p * (unsigned long long)a.n + (unsigned long long)(a.c0 + j);
      const unsigned long long lo = table[i], hi = table[i + 1];
      bad |= (p == 0 && s != 0u) || e < s || e > stream_bytes || (s & 15u) || (e & 15u) || hi < lo || hi > a.streams_bytes ||
             hi - lo != (unsigned long long)(e - s);
    }
  }
  return __syncthreads_or(bad || !ok) == 0;
}

// grid = (workgroups), 256 threads: workgroup w takes items w, w + gridDim.x, ... of m * (2 L + 1); item = what * m + j,
// what == 2 L: the static slot
__global__ __launch_bounds__(256) void k_unpack(UnpackArgs a) {
  const int P = 2 * a.L;
  const int items = a.m * (P + 1);
  for (int item = (int)blockIdx.x; item < items; item += (int)gridDim.x) {
    const int what = item / a.m, j = item - what * a.m;
    u32 streams_off;
    if (!unpack_chunk_ok(a, j, &streams_off)) {
      if (what == P && threadIdx.x == 0) atomicOr(a.status, LMC_ST_BAD_HEADER);  // once per chunk
      continue;
    }
    const u8* slot = a.pack + a.off_static + (unsigned long long)(a.c0 + j) * a.static_stride;
    u8* dst = a.dst_ptrs[j];
    if (what == P) {
      pack_copy16<true>(reinterpret_cast<uint4*>(dst), reinterpret_cast<const uint4*>(slot), streams_off >> 4);
    } else {
      const BlobOff bo = lmc_blob_off((u32)P, reinterpret_cast<const u32*>(slot)[4], (u32)a.G);
      const u32 s = reinterpret_cast<const u32*>(slot + bo.gdir)[2 * (what * a.G)];
      const unsigned long long* table = reinterpret_cast<const unsigned long long*>(a.pack + a.off_table);
      const unsigned long long i = (unsigned long long)what * (unsigned long long)a.n + (unsigned long long)(a.c0 + j);
      const unsigned long long lo = table[i], len = table[i + 1] - lo;
      pack_copy16<true>(reinterpret_cast<uint4*>(dst + streams_off + s),
                        reinterpret_cast<const uint4*>(a.pack + a.off_streams + lo), (u32)(len >> 4));
    }
  }
}
