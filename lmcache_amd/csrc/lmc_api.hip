// lmc_api.hip -- C ABI (include/lmc_hip.h) over the gfx950 kernels.
//
// Host side only does argument checking, workspace management and kernel
// launches.  Nothing here synchronises the device; the workspace shared by
// successive encode calls is ordered with an event recorded after the last
// kernel of a job and waited on by the first kernel of the next one.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <functional>
#include <mutex>
#include <new>
#include <type_traits>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "../../include/lmc_hip.h"
#include "k_blend.h"
#include "k_copy.h"
#include "k_copy_split.h"
#include "k_decode.h"
#include "k_encode_counts.h"
#include "k_fixed.h"
#include "k_fused.h"
#include "k_layers.h"
#include "k_offload.h"
#include "k_quantize.h"
#include "k_repack.h"
#include "k_rope.h"

static thread_local int g_last_hip = 0;

#define HIP_TRY(expr)                      \
  do {                                     \
    hipError_t e__ = (expr);               \
    if (e__ != hipSuccess) {               \
      g_last_hip = (int)e__;               \
      return LMC_ERR_HIP;                  \
    }                                      \
  } while (0)

// A device buffer that only grows.  grow(need): at least `need` bytes -- the old block is freed first, then a block of
// `need` rounded up to 1 MiB is taken; whoever grows a buffer that queued kernels may still use waits for them first.
template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t bytes = 0;
  int grow(size_t need) {
    if (bytes >= need) return LMC_OK;
    if (p) { hipError_t e = hipFree(p); if (e != hipSuccess) { g_last_hip = (int)e; return LMC_ERR_HIP; } p = nullptr; bytes = 0; }
    need = (need + (size_t)(1 << 20)) & ~(size_t)((1 << 20) - 1);
    hipError_t e = hipMalloc(&p, need);
    if (e != hipSuccess) { g_last_hip = (int)e; return e == hipErrorOutOfMemory ? LMC_ERR_NOMEM : LMC_ERR_HIP; }
    bytes = need;
    return LMC_OK;
  }
  void free() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
};

// What a layer-wise encode job (lmc_encode_layers_*) owns from begin to finish: look-back granules that live across the
// job's launches, a ticket counter, the symbol workspace of ONE layer's two planes and the region its V streams wait in;
// a job of the fixed-width model (lmc_encode_layers_begin_fixed) the slices' partial sums alone.
// Kept by the context between jobs and handed to the next one behind `free_ev`.
struct lmc_layer_bufs {
  DevBuf<unsigned long long> agg;
  DevBuf<u32> sym4;
  DevBuf<u8> vregion;
  DevBuf<u32> part;  // k_fixed.h: [nchunks][P][slices][G + 1]
  template <typename F> void each_buf(F&& f) { f(agg); f(sym4); f(vregion); f(part); }
  u32* ticket = nullptr;
  hipEvent_t free_ev = nullptr;  // recorded behind the last launch of the job that had them last
  bool used = false;             // ... if any
  bool busy = false;             // a live job holds them
};

struct lmc_layer_job {
  lmc_ctx* ctx;
  lmc_layer_bufs* b;
  lmc_kv_layout src;
  BinsArg bins;
  int tok_begin, tok_end, chunk_tokens, nchunks;
  u8* blobs; uint64_t blob_stride;
  u32* sizes; u32* status;
  int chain_gran;            // granules of a plane: G / 8 (a granule per workgroup) or G (per wave)
  long long vstride;         // bytes of a chunk's slot in the V region
  bool fixed = false;        // LMC_MODEL_FIXED: k_fixed_encode per layer, k_fixed_layers_finish
  u32 slices = 1, slice_passes = 0;  // ... in `slices` workgroups per (chunk, plane) of `slice_passes` passes each
  int next_layer = 0;
  u32 tickets_drawn = 0;
  hipStream_t last_stream = nullptr;  // of the last launch that went out
  bool queued = false;
};

struct lmc_ctx {
  int device;
  std::mutex mu;
  std::vector<lmc_layer_bufs*> layer_pool;  // buffers of the layer-wise encode jobs, live or not
  // Encode workspaces.  An encode job owns a workspace from its first kernel to its last; the job that takes it next
  // waits (on its own stream) for the event behind that last kernel.  TWO of them, so that a worker thread's
  // non-blocking put and the engine thread's put (the reference's model: local_backend.py:41-45, 72-80) run side by side
  // on their two streams instead of one behind the other: a job takes the slot its stream used last, else an idle one
  // (the second is allocated when the first is found busy by another stream for the first time), else the first.
  struct Workspace {
    DevBuf<u32> sym4;               // symbols between the quantise stage and the coder
    DevBuf<u8> scratch;             // two-kernel path: the streams before they are placed
    DevBuf<unsigned long long> agg; // look-back granules of the in-kernel compaction
    template <typename F> void each_buf(F&& f) { f(sym4); f(scratch); f(agg); }
    hipEvent_t ws_free = nullptr;  // recorded after the last kernel that touches the workspace
    bool ws_used = false;
    hipStream_t last_stream = nullptr;
    u32* ticket = nullptr;     // device work-ticket counter of the coder launches (k_encode.h: EncodeArgs::ticket) ...
    u32 tickets_drawn = 0;     // ... and how many tickets the launches so far have drawn (mod 2^32): per workspace, since
                               // launches that share a counter must be ordered
  };
  Workspace ws[2];
  int num_cus = 256;
  int enc_path = LMC_ENCODE_PATH_AUTO;  // lmc_ctx_set_encode_path
  int fixed_slices = 0;                 // lmc_ctx_set_fixed_layer_slices
  int fused_pl = 0;                     // LMC_FUSED_PL at lmc_ctx_create (A/B switch of tools/probes: planes per work item of narrow planes; 0 = the built-in choice)
  u32 epoch = 0;                        // of the last fused launch (tags its look-back granules)
  DevBuf<unsigned long long> pack_table;  // device copy of a pack's offset table while it is written (lmc_store_pack)
  // store / load legs (lmc_store_chunks, lmc_load_chunks)
  DevBuf<u8> store_arena;  // blobs of the job being offloaded
  DevBuf<u8> load_slots;   // HBM slots the gather kernel fills
  template <typename F> void each_buf(F&& f) { f(pack_table); f(store_arena); f(load_slots); }
  hipStream_t copy_stream = nullptr, copy_stream2 = nullptr;  // the PCIe side of both legs (two DMA queues for the load)
  hipEvent_t store_free = nullptr, load_free = nullptr;  // the arena / the slots may be reused behind these
  bool store_used = false, load_used = false;
  hipEvent_t evpool[64] = {}; int evnext = 0;         // fork / join events of the two legs (round robin)
  u32* status_h = nullptr;  // pinned, device-accessible
  // optional per-kernel timing (lmc_ctx_profile)
  bool profile = false;
  hipEvent_t pev[8] = {};
  int pn = 0;  // events recorded by the last profiled call
};

// Record the next timing event of a profiled call (no-op when profiling is off).
static int prof_mark(lmc_ctx* c, hipStream_t s) {
  if (!c->profile) return LMC_OK;
  if (c->pn >= 8) return LMC_OK;
  if (!c->pev[c->pn]) HIP_TRY(hipEventCreate(&c->pev[c->pn]));
  HIP_TRY(hipEventRecord(c->pev[c->pn], s));
  c->pn++;
  return LMC_OK;
}

extern "C" {
#ifdef LMC_EXP_TIMELINE  // experiments only (not in include/lmc_hip.h): the fused kernel's phase time stamps
int lmc_debug_fused_timeline(void* host_out, size_t bytes) {
  return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_fused_timeline), bytes < sizeof(g_fused_timeline) ? bytes : sizeof(g_fused_timeline));
}
int lmc_debug_decode_timeline(void* host_out, size_t bytes) {
  return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_decode_timeline), bytes < sizeof(g_decode_timeline) ? bytes : sizeof(g_decode_timeline));
}
#endif

const char* lmc_strerror(int code) {
  switch (code) {
    case LMC_OK: return "ok";
    case LMC_NOT_LAYERWISE: return "not an error: the job is not eligible for the layer-wise encode";
    case LMC_ERR_INVALID: return "invalid argument or unsupported geometry";
    case LMC_ERR_HIP: return "HIP runtime error (see lmc_last_hip_error)";
    case LMC_ERR_NOMEM: return "out of memory";
    case LMC_ERR_DEVICE_FLAG: return "a kernel flagged an error (see lmc_device_status)";
    default: return "unknown error";
  }
}
int lmc_last_hip_error(void) { return g_last_hip; }
int lmc_abi_version(void) { return LMC_ABI_VERSION; }

int lmc_ctx_create(int device, lmc_ctx** out) {
  if (!out) return LMC_ERR_INVALID;
  HIP_TRY(hipSetDevice(device));
  lmc_ctx* c = new (std::nothrow) lmc_ctx();
  if (!c) return LMC_ERR_NOMEM;
  c->device = device;
  {
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && v > 0) c->num_cus = v;
    if (const char* e = getenv("LMC_FUSED_PL")) c->fused_pl = atoi(e);  // read ONCE: never in the encode path
  }
  hipError_t e = hipHostMalloc(&c->status_h, 64, hipHostMallocMapped | hipHostMallocPortable);
  if (e != hipSuccess) { g_last_hip = (int)e; delete c; return LMC_ERR_HIP; }
  memset(c->status_h, 0, 64);
  for (int k = 0; k < 2; k++) {
    e = hipEventCreateWithFlags(&c->ws[k].ws_free, hipEventDisableTiming);
    if (e != hipSuccess) { g_last_hip = (int)e; (void)hipHostFree(c->status_h); delete c; return LMC_ERR_HIP; }
  }
  *out = c;
  return LMC_OK;
}

int lmc_ctx_destroy(lmc_ctx* c) {
  if (!c) return LMC_OK;
  (void)hipSetDevice(c->device);
  const auto free_buf = [](auto& buf) { buf.free(); };
  for (lmc_ctx::Workspace& w : c->ws) {
    if (w.ws_used) (void)hipEventSynchronize(w.ws_free);
    w.each_buf(free_buf);
    if (w.ticket) (void)hipFree(w.ticket);
    if (w.ws_free) (void)hipEventDestroy(w.ws_free);
  }
  if (c->copy_stream) { (void)hipStreamSynchronize(c->copy_stream); (void)hipStreamDestroy(c->copy_stream); }
  if (c->copy_stream2) { (void)hipStreamSynchronize(c->copy_stream2); (void)hipStreamDestroy(c->copy_stream2); }
  c->each_buf(free_buf);
  if (c->store_free) (void)hipEventDestroy(c->store_free);
  if (c->load_free) (void)hipEventDestroy(c->load_free);
  for (lmc_layer_bufs* b : c->layer_pool) {  // (a job still live at this point is the caller's leak: its handle dangles)
    if (b->used) (void)hipEventSynchronize(b->free_ev);
    b->each_buf(free_buf);
    if (b->ticket) (void)hipFree(b->ticket);
    if (b->free_ev) (void)hipEventDestroy(b->free_ev);
    delete b;
  }
  for (int i = 0; i < 64; i++) if (c->evpool[i]) (void)hipEventDestroy(c->evpool[i]);
  for (int i = 0; i < 8; i++) if (c->pev[i]) (void)hipEventDestroy(c->pev[i]);
  if (c->status_h) (void)hipHostFree(c->status_h);
  delete c;
  return LMC_OK;
}

int lmc_ctx_profile(lmc_ctx* c, int enable) {
  if (!c) return LMC_ERR_INVALID;
  std::lock_guard<std::mutex> lk(c->mu);
  c->profile = enable != 0;
  c->pn = 0;
  return LMC_OK;
}

int lmc_ctx_profile_read(lmc_ctx* c, float* ms_out, int cap) {
  if (!c || !ms_out || cap < 1) return LMC_ERR_INVALID;
  std::lock_guard<std::mutex> lk(c->mu);
  int n = 0;
  for (int i = 0; i + 1 < c->pn && n < cap; i++, n++)
    HIP_TRY(hipEventElapsedTime(&ms_out[n], c->pev[i], c->pev[i + 1]));
  return n;
}

int lmc_ctx_set_encode_path(lmc_ctx* c, int path) {
  if (!c || path < LMC_ENCODE_PATH_AUTO || path > LMC_ENCODE_PATH_FUSED) return LMC_ERR_INVALID;
  std::lock_guard<std::mutex> lk(c->mu);
  c->enc_path = path;
  return LMC_OK;
}

int lmc_ctx_set_fixed_layer_slices(lmc_ctx* c, int n) {
  if (!c || n < 0) return LMC_ERR_INVALID;
  std::lock_guard<std::mutex> lk(c->mu);
  c->fixed_slices = n;
  return LMC_OK;
}

int lmc_device_status(lmc_ctx* c, int clear) {
  if (!c) return LMC_ERR_INVALID;
  int v = (int)__atomic_load_n(c->status_h, __ATOMIC_ACQUIRE);
  if (clear) __atomic_store_n(c->status_h, 0u, __ATOMIC_RELEASE);
  return v;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// `vec`: the layout is READ or WRITTEN with 16-byte vectors of 8 channels (the encoders, k_copy_kv): rows on 16-byte
// boundaries, and a vector must not leave its head -- head_size a multiple of 8, or the heads of a token row back to back
// (stride_head == head_size: the vllm chunk, the per-layer [T,H,D] tensors, NBHD paged blocks), where a vector that
// crosses a head boundary is still 8 consecutive elements.  !vec: element-wise access (the decoder's scatter, the
// element-wise copy): any strides.  Either way a plane has a multiple of 8 channels (the blob's geometry).
// `split`: the caller addresses LMC_PAGED_SPLIT itself (lmc_copy_kv, the decode entry points that decode_common lets and
// the encode entry points that encode_job_ok lets); everybody else reads and writes rows and must refuse such a layout
// rather than address it as rows.
static bool layout_ok(const lmc_kv_layout* l, bool vec = true, bool split = false) {
  if (!l) return false;
  if (l->paged_kind != LMC_PAGED_ROWS && l->paged_kind != LMC_PAGED_SPLIT) return false;
  if (l->paged_kind == LMC_PAGED_SPLIT) {
    if (!split || vec || !l->slot_mapping || l->block_size < 1) return false;
    if (l->head_size < 1 || l->head_size % (lmc_dtype_fp8(l->dtype) ? 16 : 8)) return false;  // whole x-granules
  }
  if (l->dtype != LMC_DTYPE_BF16 && l->dtype != LMC_DTYPE_FP16 && !lmc_dtype_fp8(l->dtype)) return false;
  if (l->num_layers < 1 || 2 * l->num_layers > LMC_MAX_PLANES) return false;
  if (l->num_heads < 1 || l->head_size < 1) return false;
  const long long C = (long long)l->num_heads * l->head_size;
  if (C < 8 || (C & 7) || C > LMC_MAX_CHANNELS) return false;
  if (!l->base && !l->plane_ptrs) return false;
  if (l->slot_mapping && l->block_size < 1) return false;
  if (!vec) return true;
  if (l->head_size & 7) {
    if (l->stride_head != l->head_size) return false;
  } else if (l->stride_head & 7) return false;
  if (l->stride_token & 7) return false;
  // (a vector is 8 elements: 16 bytes of a 16-bit dtype, 8 of fp8 -- the alignment of the base follows the vector)
  const uintptr_t vec_align = lmc_dtype_fp8(l->dtype) ? 7 : 15;
  if (!l->plane_ptrs && ((l->stride_layer & 7) || (l->stride_kv & 7) || ((uintptr_t)l->base & vec_align))) return false;
  if (l->slot_mapping && (l->stride_block & 7)) return false;
  return true;
}

// What k_decode's stores can address in a destination that layout_ok(dst, false) has passed (k_decode.h).  A stored
// element of E bytes (2, fp8: 1) leaves through a raw buffer descriptor of 0xfffffff0 records: address = base (a token
// row, 64-bit) + soffset (u32, scalar) + voffset (u32, the lane).  On gfx950 the range check covers the SUM, not voffset
// alone as k_decode.h's comment has it: the store is dropped unless soffset + voffset + E <= 0xfffffff0 (idle lanes are
// parked at voffset 0xfffffff8 for that reason).  tests/test_gpu_far_offsets.py holds this against the hardware: of a
// chunk whose last row reached past the range, exactly the bytes at soffset + voffset >= 0xfffffff0 were missing (of a
// head stride at the voffset-only limit, every row of a chunk but its first), and nothing was written anywhere else.
//   voffset = lane_off = (u32)((h * stride_head + d) * E), at most  row - E  with  row = ((H - 1) * stride_head + D) * E;
//   a negative or larger offset would be truncated to 32 bits: stride_head >= 0.
//   soffset: without a slot mapping the descriptor stays at the chunk's first stored row and soffset grows by
//   row_step = stride_token * E per token, u32 arithmetic, up to (rows stored - 1) * row_step with at most chunk_tokens
//   rows (the kernel refuses a longer blob).  With a slot mapping every row has a descriptor based at the row itself
//   (soffset 0), except on the block path -- taken only while row_step < 2^28 -- where the descriptor stands at the first
//   of eight rows and soffset reaches 7 * row_step.  stride_token >= 0 for every destination: one rule.
//       reach = slot_mapping ? (row_step < 2^28 ? 7 * row_step : 0) : (chunk_tokens - 1) * row_step
//       admitted:  stride_head >= 0,  stride_token >= 0,  reach + row <= 0xfffffff0
// (so a row always fits the range, and without a slot mapping a chunk's rows end within 4 GiB of its first row).
// LMC_PAGED_SPLIT (k_decode's DEC_PAGED_SPLIT): the descriptor stands at a block (64-bit: blocks and planes may lie any
// distance apart), voffset is the lane's head, granule / column and element, below
//       head = ((H - 1) * stride_head + D * block_size) * E,
// and soffset the slot's step within a run of eight: at most 7 * 16 bytes (a key plane; a value plane 7 * E).
//       admitted:  stride_head >= 0,  head + 7 * 16 <= 0xfffffff0
// Every entry point that launches k_decode with a destination asks this before anything is queued.
static bool decode_dst_ok(const lmc_kv_layout* d, long long chunk_tokens) {
  typedef __int128 wide;  // (the products of two 64-bit strides and counts)
  const wide E = lmc_dtype_fp8(d->dtype) ? 1 : 2;
  if (d->paged_kind == LMC_PAGED_SPLIT) {
    if (d->stride_head < 0) return false;
    return ((wide)(d->num_heads - 1) * d->stride_head + (wide)d->head_size * d->block_size) * E + 7 * 16 <= (wide)0xfffffff0ll;
  }
  if (d->stride_head < 0 || d->stride_token < 0) return false;
  const wide row = ((wide)(d->num_heads - 1) * d->stride_head + d->head_size) * E;
  const wide row_step = (wide)d->stride_token * E;
  const wide reach = d->slot_mapping ? (row_step < ((wide)1 << 28) ? 7 * row_step : (wide)0) : (wide)(chunk_tokens - 1) * row_step;
  return reach + row <= (wide)0xfffffff0ll;
}

static KvAddr to_addr(const lmc_kv_layout* l) {
  KvAddr a;
  a.base = (const u16*)l->base;
  a.plane_ptrs = (const u16* const*)l->plane_ptrs;
  a.slot_mapping = (const long long*)l->slot_mapping;
  a.stride_layer = l->stride_layer; a.stride_kv = l->stride_kv; a.stride_token = l->stride_token;
  a.stride_head = l->stride_head; a.stride_block = l->stride_block;
  a.block_size = l->block_size > 0 ? l->block_size : 1;
  a.L = l->num_layers; a.H = l->num_heads; a.D = l->head_size; a.dtype = l->dtype;
  return a;
}

static bool bins_ok(const int32_t* bins_h, int P, BinsArg* out) {
  if (!bins_h) return false;
  memset(out, 0, sizeof *out);
  for (int p = 0; p < P; p++) {
    // MAX = bins//2 - 1 >= 1 and symbols 0..2*MAX must fit the 32-entry CDF
    if (bins_h[p] < 4 || bins_h[p] > LMC_MAX_BINS) return false;
    out->b[p] = (u8)bins_h[p];
  }
  return true;
}

// ---- where a run-time value picks a kernel instance: f is a generic lambda that takes the value as a tag type ------------
// f(IntTag<V>) for the first of V, Vs... that equals v, else for the last of them.
template <int V, int... Vs, typename F>
static auto with_int(int v, F&& f) {
  if constexpr (sizeof...(Vs) == 0) return f(IntTag<V>{});
  else return v == V ? f(IntTag<V>{}) : with_int<Vs...>(v, f);
}
template <typename F>
static auto with_bool(bool b, F&& f) { return b ? f(BoolTag<true>{}) : f(BoolTag<false>{}); }
// The KV dtype code `dtype` (one that layout_ok has passed) for the kernels that have an instance per dtype ...
template <typename F>
static auto with_kv_dtype(int dtype, F&& f) {
  return with_int<LMC_DTYPE_BF16, LMC_DTYPE_FP16, LMC_DTYPE_FP8_E4M3, LMC_DTYPE_FP8_E5M2>(dtype, f);
}
// ... and for the ones that have 16-bit instances only (k_fixed_*, k_rope_*: their callers have refused fp8).  Never
// with_kv_dtype there: it would build fp8 instances nobody launches.
template <typename F>
static auto with_kv_dtype16(int dtype, F&& f) {
  return with_int<LMC_DTYPE_BF16, LMC_DTYPE_FP16>(dtype, f);
}
// How a destination's tokens are found (k_decode.h, KIND).
template <typename F>
static auto with_decode_kind(const lmc_kv_layout* dst, F&& f) {
  const int kind = dst->paged_kind == LMC_PAGED_SPLIT ? DEC_PAGED_SPLIT : dst->slot_mapping ? DEC_PAGED_ROWS : DEC_ROWS;
  return with_int<DEC_PAGED_SPLIT, DEC_PAGED_ROWS, DEC_ROWS>(kind, f);
}
// f(IntTag<G>, IntTag<NITER>) for a plane of C <= 1024 channels: G lanes take a row, NITER runs of 8 channels each (the
// rungs every plane-wide kernel has: k_quantize, k_encode_fused, k_fixed_encode).  false, and f not called: the plane is
// wider -- the caller has its own instances for that, or none.
template <typename F>
static bool with_plane_width(int C, F&& f) {
  if (C <= 128) f(IntTag<16>{}, IntTag<1>{});
  else if (C <= 256) f(IntTag<32>{}, IntTag<1>{});
  else if (C <= 512) f(IntTag<64>{}, IntTag<1>{});
  else if (C <= 1024) f(IntTag<64>{}, IntTag<2>{});
  else return false;
  return true;
}

// What k_quantize's loads can address in an LMC_PAGED_SPLIT source that layout_ok(src, false, true) has passed
// (k_quantize.h, split_load_oct): the block offset is 64-bit, everything inside a block -- head, granule or channel,
// column, element -- is added up in 32 bits, in elements, and stays below
//       head = (H - 1) * stride_head + D * block_size.
//       admitted:  stride_head >= 0,  head * E <= 0xfffffff0     (E = element bytes; the bound decode_dst_ok sets the stores)
static bool split_range_ok(const lmc_kv_layout* l) {
  typedef __int128 wide;
  if (l->stride_head < 0 || l->block_size < 1) return false;
  const wide E = lmc_dtype_fp8(l->dtype) ? 1 : 2;
  return ((wide)(l->num_heads - 1) * l->stride_head + (wide)l->head_size * l->block_size) * E <= (wide)0xfffffff0ll;
}

// What every encode job asks of its source and its token range (lmc_encode_chunks, and the stores in front of it before
// they take a buffer).  *nchunks: the job's chunks -- at most 65535, they ride on gridDim.z of k_quantize.
// `split_ok`: the entry point takes an LMC_PAGED_SPLIT source (lmc_encode_chunks_split and the stores; lmc_encode_chunks
// does not) -- the twin of decode_common's flag.  Such a source is asked what lmc_copy_kv asks of a split side (a slot
// mapping, block_size >= 1, whole x-granules), split_range_ok, and planes of at most 1024 channels.
static bool encode_job_ok(const lmc_ctx* c, const lmc_kv_layout* src, int32_t tok_begin, int32_t tok_end, int32_t chunk_tokens,
                          int* nchunks, bool split_ok = false) {
  const bool nhdb = src && src->paged_kind == LMC_PAGED_SPLIT;
  if (nhdb ? !(split_ok && layout_ok(src, false, true) && split_range_ok(src)) : !layout_ok(src)) return false;
  if (nhdb && (long long)src->num_heads * src->head_size > 1024) return false;  // k_quantize's split instances stop there
  if (!c || tok_begin < 0 || tok_end <= tok_begin || chunk_tokens < 1 || chunk_tokens > 65535) return false;
  *nchunks = (tok_end - tok_begin + chunk_tokens - 1) / chunk_tokens;
  return *nchunks <= 65535;
}

// ... and of the arena its blobs go to, a slot of `blob_stride` bytes per chunk, and of its bins (-> *bins): 16-byte slots
// that hold the largest blob of the geometry, a size word per chunk.  `fixed_blobs`: the job writes or reads fixed-width
// blobs, whose exact size must fit the header's 32-bit size words (the coded models' bound is blob_stride's: checked by
// whoever sized the arena).
static bool encode_dst_ok(const void* blobs, uint64_t blob_stride, const uint32_t* sizes, int L, int H, int D, int32_t chunk_tokens,
                          const int32_t* bins_h, bool fixed_blobs, BinsArg* bins) {
  if (!blobs || !sizes || ((uintptr_t)blobs & 15) || (blob_stride & 15)) return false;
  if (blob_stride < lmc_blob_bound((uint32_t)L, (uint32_t)chunk_tokens, (uint32_t)H, (uint32_t)D)) return false;
  if (!bins_ok(bins_h, 2 * L, bins)) return false;
  return !fixed_blobs || lmc_fixed_blob_bytes((uint32_t)L, (uint32_t)chunk_tokens, (uint32_t)H, (uint32_t)D, bins->b) <= 0xffffffffull;
}

// What a job over blobs of earlier stores asks of the geometry it is told (the transcodes, lmc_pack_blobs): `nchunks`
// chunks of L layers x H heads x D, planes of a multiple of 8 channels up to LMC_MAX_CHANNELS, and `ntokens` tokens that
// fill every chunk but, possibly, the last.
static bool chunk_geometry_ok(int32_t nchunks, int32_t L, int32_t H, int32_t D, int32_t chunk_tokens, uint32_t ntokens) {
  if (nchunks < 1 || nchunks > 65535 || L < 1 || 2 * L > LMC_MAX_PLANES || H < 1 || D < 1 || chunk_tokens < 1 || chunk_tokens > 65535)
    return false;
  const long long C = (long long)H * D;
  if (C < 8 || (C & 7) || C > LMC_MAX_CHANNELS) return false;
  return (uint64_t)ntokens <= (uint64_t)nchunks * (uint32_t)chunk_tokens && (uint64_t)ntokens > (uint64_t)(nchunks - 1) * (uint32_t)chunk_tokens;
}

// NHDB: the source is an LMC_PAGED_SPLIT cache (k_quantize.h: instances of their own, planes of up to 1024 channels)
template <int DT, bool QUAD, bool NHDB = false>
static int launch_quant_dt(const QuantArgs& a, hipStream_t s) {
  const int C = a.C;
  if (a.pc_limit < 1) return LMC_OK;
  const unsigned nz = (unsigned)((a.pc_limit + a.P - 1) / a.P);  // chunks that hold the plane-chunks to do
  const unsigned ny = (unsigned)(a.nplanes ? a.nplanes : a.P);   // planes of the launch (QuantArgs::plane0)
  // SPLIT > 1 (wide planes, workspace output): SPLIT waves share a row oct, 1024 channels each (k_quantize.h)
  const auto launch = [&](auto g, auto n, auto split) {
    constexpr int G = decltype(g)::value, N = decltype(n)::value, SPLIT = decltype(split)::value;
    const int per_wg = 4 * (64 / G) / SPLIT, TO = (a.TQ + 1) / 2;  // row octs per plane-chunk
    const dim3 grid((unsigned)((TO + per_wg - 1) / per_wg), ny, nz);
    hipLaunchKernelGGL((k_quantize<G, N, DT, QUAD, SPLIT, NHDB>), grid, dim3(256), 0, s, a);
  };
  const IntTag<64> g64;
  if (with_plane_width(C, [&](auto g, auto n) { launch(g, n, IntTag<1>{}); })) {
  } else if constexpr (NHDB) {
    return LMC_ERR_INVALID;
  } else if (C > 4096) {
    return LMC_ERR_INVALID;
  } else if (QUAD) {  // (a plain `if`, here and below: either QUAD builds both arms, as it always has -- the set of kernels stays)
    if (C <= 2048) launch(g64, IntTag<2>{}, IntTag<QUAD ? 2 : 1>{});
    else launch(g64, IntTag<2>{}, IntTag<QUAD ? 4 : 1>{});
  } else {
    if (C <= 2048) launch(g64, IntTag<4>{}, IntTag<1>{});
    else launch(g64, IntTag<8>{}, IntTag<1>{});
  }
  HIP_TRY(hipGetLastError());
  return LMC_OK;
}

template <bool QUAD>
static int launch_quant(const QuantArgs& a, hipStream_t s, bool nhdb = false) {
  return with_kv_dtype(a.src.dtype, [&](auto dt) {
    if constexpr (QUAD) {
      if (nhdb) return launch_quant_dt<decltype(dt)::value, true, true>(a, s);
    }
    return launch_quant_dt<decltype(dt)::value, QUAD>(a, s);
  });
}

// The slot of a blob in the arenas and slots of this file: lmc_blob_bound rounded up to 16 bytes.
static uint64_t blob_stride(int L, int chunk_tokens, int H, int D) {
  return (lmc_blob_bound((uint32_t)L, (uint32_t)chunk_tokens, (uint32_t)H, (uint32_t)D) + 15) & ~(uint64_t)15;
}

// The fused encode for a plane width (k_fused.h: lanes per quantise task, channel runs per lane, waves per row).
// C <= LMC_FUSED_MAX_CHANNELS = 1024 (encode_job's fused_fits): the common rungs are all the kernel has.
static void launch_fused(int C, dim3 grid, dim3 block, hipStream_t s, const FusedArgs& fa) {
  // a paged source with a block size that is a power of two (every one vLLM offers) has kernel instances of its own: the
  // tokens' slots by scalar loads (k_fused.h, fused_tok_off)
  const u32 bs = (u32)fa.src.block_size;
  with_kv_dtype(fa.src.dtype, [&](auto dt) {
    with_bool(fa.src.slot_mapping && bs != 0u && (bs & (bs - 1u)) == 0u, [&](auto psrc) {
      with_plane_width(C, [&](auto g, auto n) {
        hipLaunchKernelGGL((k_encode_fused<decltype(g)::value, decltype(n)::value, decltype(dt)::value, FUSED_WAVES, decltype(psrc)::value>),
                           grid, block, 0, s, fa);
      });
    });
  });
}

// caller holds ctx->mu.  The symbol workspace and the look-back granules of `max_chunks` chunks, stream scratch for
// `scratch_chunks` of them (only the general coder launch -- chunk lengths other than 256, a ragged last chunk -- codes
// into scratch slots; the fused kernel and the counts-only coder launch code straight into the blobs).
static int reserve_locked(lmc_ctx::Workspace* c, int L, int H, int D, int chunk_tokens, int max_chunks, int scratch_chunks) {
  const size_t P = 2 * (size_t)L, C = (size_t)H * D, G = (C + 63) / 64, TQ = ((size_t)chunk_tokens + 3) / 4;
  const size_t need_sym = (size_t)max_chunks * P * TQ * C * 4;
  const size_t need_scr = (size_t)scratch_chunks * P * G * lmc_group_cap_bytes((uint32_t)chunk_tokens);
  const size_t need_agg = (size_t)max_chunks * P * G * 8;
  if (need_sym <= c->sym4.bytes && need_scr <= c->scratch.bytes && need_agg <= c->agg.bytes)
    return LMC_OK;
  // growing frees memory that queued kernels may still use: wait for them (this call only)
  if (c->ws_used) HIP_TRY(hipEventSynchronize(c->ws_free));
  int rc;
  const size_t agg_before = c->agg.bytes;
  if ((rc = c->sym4.grow(need_sym)) || (rc = c->scratch.grow(need_scr)) || (rc = c->agg.grow(need_agg))) return rc;
  // fresh granules must not look like a published value of some epoch (k_fused.h)
  if (c->agg.bytes != agg_before) HIP_TRY(hipMemset(c->agg.p, 0, c->agg.bytes));
  return LMC_OK;
}

// ---- LMC_MODEL_FIXED (k_fixed.h): one launch, a workgroup per (plane, chunk); no workspace, so no context state beyond
// the profiling marks ------------------------------------------------------------------------------------------------
// NHDB: the source is an LMC_PAGED_SPLIT cache (k_quantize.h, split_load_oct): instances of their own, planes of up to
// 1024 channels (encode_job_ok)
// LAYER: a layer's launch of a layer-wise job (FixedEncArgs): e.nplanes planes of every chunk in `slices` workgroups each,
// instances of their own (16: the one-piece instances stay the code they were), planes of up to 1024 channels.
template <int DT, bool LAYER = false>
static int launch_fixed_encode(const FixedEncArgs& fa, hipStream_t s, bool nhdb, unsigned slices = 1) {
  const int C = fa.e.C;
  const dim3 grid((unsigned)(LAYER ? fa.e.nplanes : fa.e.P), (unsigned)fa.e.nchunks, slices), block(64 * FIXED_ENC_WAVES);
  const bool common = with_bool(nhdb, [&](auto split) {
    return with_plane_width(C, [&](auto g, auto n) {
      hipLaunchKernelGGL((k_fixed_encode<decltype(g)::value, decltype(n)::value, DT, 1, decltype(split)::value, LAYER>), grid, block, 0, s, fa);
    });
  });
  if (!common) {  // wider than 1024 channels: rows in one piece only, SPLIT waves to a row oct
    if constexpr (LAYER) return LMC_ERR_INVALID;
    else if (nhdb) return LMC_ERR_INVALID;
    else if (C <= 2048) hipLaunchKernelGGL((k_fixed_encode<64, 2, DT, 2>), grid, block, 0, s, fa);
    else hipLaunchKernelGGL((k_fixed_encode<64, 2, DT, 4>), grid, block, 0, s, fa);  // C <= LMC_MAX_CHANNELS: layout_ok
  }
  HIP_TRY(hipGetLastError());
  return LMC_OK;
}

extern "C" {

int lmc_ctx_reserve(lmc_ctx* c, int L, int H, int D, int chunk_tokens, int max_chunks) {
  if (!c || L < 1 || H < 1 || D < 1 || (H * (long long)D) % 8 || chunk_tokens < 1 || max_chunks < 1) return LMC_ERR_INVALID;
  HIP_TRY(hipSetDevice(c->device));
  std::lock_guard<std::mutex> lk(c->mu);
  return reserve_locked(&c->ws[0], L, H, D, chunk_tokens, max_chunks, max_chunks);
}

int lmc_quantize(lmc_ctx* c, const lmc_kv_layout* src, int32_t tok_begin, int32_t ntok, const int32_t* bins_h,
                 int8_t* sym_out, uint16_t* scale_out, lmc_stream_t stream) {
  if (!c || !layout_ok(src) || ntok < 1 || ntok > 65535 || tok_begin < 0 || !sym_out || !scale_out) return LMC_ERR_INVALID;
  QuantArgs a;
  memset(&a, 0, sizeof a);
  a.src = to_addr(src);
  a.P = 2 * src->num_layers;
  if (!bins_ok(bins_h, a.P, &a.bins)) return LMC_ERR_INVALID;
  a.C = src->num_heads * src->head_size;
  a.tok_begin = tok_begin; a.tok_end = tok_begin + ntok; a.chunk_tokens = ntok; a.nchunks = 1;
  a.TQ = (ntok + 3) / 4;
  a.pc_limit = a.P;
  a.sym8 = sym_out;
  a.scale_base = (u8*)scale_out; a.scale_stride = 0;
  HIP_TRY(hipSetDevice(c->device));
  return launch_quant<false>(a, (hipStream_t)stream);
}

int lmc_calculate_cdf(lmc_ctx* c, const int8_t* sym, int32_t P, int32_t T, int32_t C, int32_t max_bins,
                      uint16_t* cdf_out, lmc_stream_t stream) {
  if (!c || !sym || !cdf_out || P < 1 || T < 1 || T > 65535 || C < 8 || (C & 7) || max_bins != LMC_MAX_BINS)
    return LMC_ERR_INVALID;
  EncodeArgs a;
  memset(&a, 0, sizeof a);
  a.sym8 = sym;
  a.tok_begin = 0; a.tok_end = T; a.chunk_tokens = T; a.nchunks = 1;
  a.P = P; a.C = C; a.G = (C + 63) / 64; a.TQ = (T + 3) / 4;
  a.cdf_out = cdf_out;
  a.status = c->status_h;
  HIP_TRY(hipSetDevice(c->device));
  long long n = (long long)P * a.G;
  hipLaunchKernelGGL((k_cdf_encode<false, false>), dim3((unsigned)((n + ENC_WAVES - 1) / ENC_WAVES)), dim3(64 * ENC_WAVES), 0, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return LMC_OK;
}

// What stands in front of the coder in a job that has no KV to quantise: fixed-width blobs of earlier stores
// (lmc_transcode_fixed; k_fixed.h, k_fixed_expand).
struct FixedSrc {
  const void* const* blob_ptrs;  // device [nchunks]
  const uint32_t* blob_bytes;    // device [nchunks]
  int L, H, D, dtype;
};
typedef std::function<int(int, int, bool)> AfterPart;
// The encode job behind its source's own checks: the refusals every source shares, the workspace, the launches.  `src`: the
// KV that k_quantize or the fused kernel reads, or NULL and `fx`: k_fixed_expand in k_quantize's place -- always the two
// kernels, and behind the first one the job is the same job.
static int encode_job(lmc_ctx* c, const lmc_kv_layout* src, const FixedSrc* fx, int nchunks, int32_t tok_begin, int32_t tok_end,
                      int32_t chunk_tokens, const int32_t* bins_h, void* blobs, uint64_t blob_stride, uint32_t* sizes,
                      uint32_t* job_status, lmc_stream_t stream, int nparts, const AfterPart* after_part) {
  const int L = src ? src->num_layers : fx->L, H = src ? src->num_heads : fx->H, D = src ? src->head_size : fx->D;
  const int kv_dtype = src ? src->dtype : fx->dtype;
  const int P = 2 * L, C = H * D, G = (C + 63) / 64;  // (C <= LMC_MAX_CHANNELS: layout_ok)
  // an LMC_PAGED_SPLIT source (at most 1024 channels per plane: encode_job_ok): k_quantize's split instances, then
  // k_cdf_encode -- never the fused kernel, so the job is one part
  const bool nhdb = src && src->paged_kind == LMC_PAGED_SPLIT;
  BinsArg bins;
  // (fixed-width blobs READ here: of this geometry and these bins they stay below 2^32 bytes, as their encoder saw to --
  // k_fixed_expand's sums)
  if (!encode_dst_ok(blobs, blob_stride, sizes, L, H, D, chunk_tokens, bins_h, /*fixed_blobs=*/fx != nullptr, &bins)) return LMC_ERR_INVALID;
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)stream;

  std::lock_guard<std::mutex> lk(c->mu);
  bool split_done = false;  // the fused launch went out in plane ranges and after_part ran behind each
  // k_fused.h codes the 256-token chunks (the counts model) of every plane width: a work item is a run of whole planes
  // of one chunk -- 8 planes of <= 64 channels, 4 of <= 128, 2 of <= 256, else one
  const int nfull = (tok_end - tok_begin) / chunk_tokens;  // chunks of exactly chunk_tokens tokens; a ragged one may follow
  // (planes of more than 1024 channels: two kernels -- the fused form built for them in round 4 never won below eight
  // generations of workgroups and was removed, k_fused.h)
  // chunk lengths: the counts model (and with it the counts-only coder launch) codes 2 .. 256 tokens, the fused kernel
  // takes the job's full chunks of 32 .. 256 tokens (round 5; both were 256 only)
  const bool fused_fits = chunk_tokens >= 32 && chunk_tokens <= (int)LMC_COUNTS_T && nfull > 0 && C <= LMC_FUSED_MAX_CHANNELS;
  // planes per work item: narrow planes are grouped until an item has about eight streams -- one per wave (C = 128,
  // 80 layers, 128 chunks, measured: 4 planes = 8 streams per item 0.65 ms, 8 planes 0.68, 2 planes 0.80)
  int pl = C <= 256 ? (8 / G > 1 ? 8 / G : 1) : 1;
  if (c->fused_pl >= 1 && c->fused_pl * G <= 16 && C <= 256) pl = c->fused_pl;  // A/B switch (tools/probes), read at lmc_ctx_create
  const int ipc = (P + pl - 1) / pl;
  // AUTO: the fused kernel pays once its workgroups fill the slots of the chip (4 per CU): measured on MI355X with
  // 64 planes of 1024 channels, 4 / 8 / 12 / 16 / 32 / 64 chunks: fused / two-kernel time = 1.27 / 1.16 / 1.05 / 1.00 /
  // 0.91 / 0.90 (tools/probes/encode_ab.hip)
  const long long auto_min = 4ll * c->num_cus;
  const bool fused = !nhdb && !fx && fused_fits && (c->enc_path == LMC_ENCODE_PATH_FUSED ||
                                    (c->enc_path == LMC_ENCODE_PATH_AUTO && (long long)nfull * ipc >= auto_min));
  // chunks that go through the general coder launch (scratch slots): every chunk of a job whose chunks are longer than
  // 256 tokens or whose streams do not fill 8-wave workgroups, a ragged last chunk of a single token
  const int tail_tokens = (tok_end - tok_begin) - nfull * chunk_tokens;  // 0: no ragged chunk
  const bool counts_geometry = chunk_tokens <= (int)LMC_COUNTS_T && ((long long)P * G) % 8 == 0;
  const bool general_only = !counts_geometry || chunk_tokens < (int)LMC_COUNTS_T_MIN;
  const bool tail_general = tail_tokens > 0 && (general_only || tail_tokens < (int)LMC_COUNTS_T_MIN);
  const int scratch_chunks = general_only ? (fused ? nchunks - nfull : nchunks) : (tail_general ? 1 : 0);
  // which workspace: the one this stream used last (stream order alone keeps the jobs apart), else an idle one, else --
  // both busy with other streams' jobs -- the first, behind its job
  lmc_ctx::Workspace* w = nullptr;
  for (lmc_ctx::Workspace& k : c->ws)
    if (!w && k.ws_used && k.last_stream == s) w = &k;
  for (lmc_ctx::Workspace& k : c->ws) {
    if (w) break;
    if (!k.ws_used) { w = &k; break; }
    const hipError_t q = hipEventQuery(k.ws_free);
    if (q == hipSuccess) w = &k;
    else (void)hipGetLastError();  // hipErrorNotReady
  }
  if (!w) w = &c->ws[0];
  int rc = reserve_locked(w, L, H, D, chunk_tokens, nchunks, scratch_chunks);
  if (rc) return rc;
  if (w->ws_used) HIP_TRY(hipStreamWaitEvent(s, w->ws_free, 0));
  // (A size word of 0 says "this chunk's encode did not finish" to whoever reads the words next: the kernels clear the
  // job's words themselves -- k_quantize on the two-kernel path, in the fused kernel the workgroup that later writes the
  // size -- so that no stale word of an earlier job stands in for a size and no memset dispatch sits in front of a job.)

  const int TQ = (chunk_tokens + 3) / 4;
  const u32 cap = lmc_group_cap_bytes((uint32_t)chunk_tokens);  // scratch slot stride (and capacity)
  lmc_blob_header hl;
  lmc_blob_layout((uint32_t)L, (uint32_t)chunk_tokens, (uint32_t)H, (uint32_t)D, &hl);
  const long long PG = (long long)P * G;

  EncodeArgs ea;
  memset(&ea, 0, sizeof ea);
  ea.sym4 = w->sym4.p;
  ea.tok_begin = tok_begin; ea.tok_end = tok_end; ea.chunk_tokens = chunk_tokens; ea.nchunks = nchunks;
  ea.P = P; ea.C = C; ea.G = G; ea.TQ = TQ;
  ea.sym_stride = (long long)TQ * C;
  ea.blobs = (u8*)blobs; ea.blob_stride = (long long)blob_stride;
  ea.scratch = w->scratch.p; ea.cap = cap;
  ea.status = job_status ? job_status : c->status_h;
  ea.bins = bins;
  ea.agg = w->agg.p; ea.sizes = sizes;
  ea.L = L; ea.H = H; ea.D = D;
  ea.dtype = lmc_math_dtype(kv_dtype);  // the header's dtype word: an fp8 chunk is coded as its bf16 images (lmc_format.h)
  u8* const scale_base = (u8*)blobs + hl.off_scales;  // off_scales does not depend on T

  if (!w->ticket) {
    HIP_TRY(hipMalloc(&w->ticket, 64));
    HIP_TRY(hipMemsetAsync(w->ticket, 0, 64, s));  // ordered in front of the first launch that draws from it
    w->tickets_drawn = 0;
  }
  ea.ticket = w->ticket;
  c->pn = 0;
  // A launch that draws tickets and fails leaves the host's count and the device counter apart: both start over.
  auto tickets_reset = [&]() {
    (void)hipMemsetAsync(w->ticket, 0, 64, s);
    w->tickets_drawn = 0;
  };
  // the chunks [c0, c0 + n) of the job with the two kernels: k_quantize, then k_cdf_encode (CDF or counts table +
  // coder + in-kernel compaction of the streams into the blobs).  Measured alternatives that lost: HISTORY.md.
  auto two_kernels = [&](int c0, int n) -> int {
    EncodeArgs e2 = ea;
    e2.tok_begin = tok_begin + c0 * chunk_tokens; e2.nchunks = n;
    e2.sym4 = w->sym4.p + (size_t)c0 * P * (size_t)ea.sym_stride;
    e2.blobs = (u8*)blobs + (size_t)c0 * blob_stride;
    e2.scratch = w->scratch.p;  // (at most one launch of a job codes into scratch: its slots are counted from its first chunk)
    e2.agg = w->agg.p + (size_t)c0 * PG;
    e2.sizes = sizes + c0;
    int r;
    if ((r = prof_mark(c, s))) return r;
    if (fx) {  // the same workspace, scales and job words from the chunks' fixed-width blobs
      FixedExpandArgs xa;
      memset(&xa, 0, sizeof xa);
      xa.blob_ptrs = (const u8* const*)fx->blob_ptrs + c0; xa.blob_bytes = fx->blob_bytes + c0;
      xa.tok_begin = e2.tok_begin; xa.tok_end = tok_end; xa.chunk_tokens = chunk_tokens; xa.nchunks = n;
      xa.P = P; xa.C = C; xa.G = G; xa.TQ = TQ;
      xa.L = L; xa.H = H; xa.D = D; xa.dtype = kv_dtype;
      xa.sym4 = const_cast<u32*>(e2.sym4); xa.sym_stride = ea.sym_stride;
      xa.scale_base = scale_base + (size_t)c0 * blob_stride; xa.scale_stride = (long long)blob_stride;
      xa.agg = e2.agg; xa.agg_n = (long long)n * PG;
      xa.sizes = e2.sizes;
      xa.status = e2.status;
      xa.bins = bins;
      const long long nwaves = (long long)n * PG;  // a wave per stream
      hipLaunchKernelGGL(k_fixed_expand, dim3((unsigned)((nwaves + FIXED_EXP_WAVES - 1) / FIXED_EXP_WAVES)), dim3(64 * FIXED_EXP_WAVES), 0, s, xa);
      HIP_TRY(hipGetLastError());
    } else {
      QuantArgs qa;
      memset(&qa, 0, sizeof qa);
      qa.src = to_addr(src); qa.bins = bins;
      qa.tok_begin = e2.tok_begin; qa.tok_end = tok_end; qa.chunk_tokens = chunk_tokens; qa.nchunks = n;
      qa.P = P; qa.C = C; qa.TQ = TQ; qa.pc_limit = n * P; qa.sym_stride = ea.sym_stride;
      qa.sym4 = const_cast<u32*>(e2.sym4);
      qa.scale_base = scale_base + (size_t)c0 * blob_stride;
      qa.scale_stride = (long long)blob_stride;
      qa.agg = e2.agg; qa.agg_n = (long long)n * PG;  // zeroed by the quantiser: one dispatch less per job
      qa.sizes = e2.sizes;
      if ((r = launch_quant<true>(qa, s, nhdb))) return r;
    }
    if ((r = prof_mark(c, s))) return r;
    const long long ngroups = (long long)n * PG;
    // launches whose chunks all have 2 .. 256 tokens (a ragged last chunk included) take the counts-only coder: 8 waves
    // per workgroup, 32 waves per CU
    const int last_tokens = std::min(chunk_tokens, tok_end - (e2.tok_begin + (n - 1) * chunk_tokens));
    const bool counts_only = !general_only && last_tokens >= (int)LMC_COUNTS_T_MIN;
    const int nw = counts_only ? 8 : ENC_WAVES;
    const unsigned nwg = (unsigned)((ngroups + nw - 1) / nw);
    e2.ticket_base = w->tickets_drawn;
    if (counts_only) hipLaunchKernelGGL((k_cdf_encode<true, true, 8, true>), dim3(nwg), dim3(64 * 8), 0, s, e2);
    else hipLaunchKernelGGL((k_cdf_encode<true, true>), dim3(nwg), dim3(64 * ENC_WAVES), 0, s, e2);
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) { g_last_hip = (int)le; tickets_reset(); return LMC_ERR_HIP; }
    w->tickets_drawn += nwg;  // only a launch that went out has drawn
    if (lmc_dtype_fp8(kv_dtype)) {  // the coder wrote header word 23 as 0: the KV's dtype goes there
      hipLaunchKernelGGL(k_set_kv_dtype, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, e2.blobs, e2.blob_stride, n,
                         (u32)kv_dtype);
      HIP_TRY(hipGetLastError());
    }
    return prof_mark(c, s);
  };
  if (fused) {
    // One launch for the full chunks: a workgroup per (chunk, plane) quantises, then codes its streams into the blob.
    FusedArgs fa;
    memset(&fa, 0, sizeof fa);
    fa.src = to_addr(src); fa.e = ea;
    fa.e.nchunks = nfull;
    fa.e.tok_end = tok_begin + nfull * chunk_tokens;
    fa.scale_base = scale_base; fa.scale_stride = (long long)blob_stride;
    c->epoch = (c->epoch + 1u) & 0x3fffffffu;
    if (!c->epoch) c->epoch = 1u;
    fa.epoch = c->epoch;
    fa.pl = pl; fa.ipc = ipc;
    // items are plane-major across the chunks (item = it * nfull + chunk): a range of `it` is a range of planes of ALL
    // chunks.  One launch, or -- a store that packs and ships the planes as they are coded -- `nparts` of them.
    const int np = (after_part && nfull == nchunks && nparts > 1) ? std::min(nparts, ipc) : 1;
    split_done = np > 1;
    const dim3 block(64 * FUSED_WAVES);
    if ((rc = prof_mark(c, s))) return rc;
    for (int r = 0; r < np; r++) {
      const int it0 = (int)((long long)ipc * r / np), it1 = (int)((long long)ipc * (r + 1) / np);
      const dim3 grid((unsigned)((long long)nfull * (it1 - it0)));
      fa.item_base = (u32)((long long)it0 * nfull);
      fa.e.ticket_base = w->tickets_drawn;
      launch_fused(C, grid, block, s, fa);
      const hipError_t le = hipGetLastError();
      if (le != hipSuccess) { g_last_hip = (int)le; tickets_reset(); return LMC_ERR_HIP; }
      w->tickets_drawn += grid.x;
      if (np > 1 && (rc = (*after_part)(r, std::min(P, it1 * pl), r == np - 1))) return rc;
    }
    if ((rc = prof_mark(c, s))) return rc;
    if (nfull < nchunks && (rc = two_kernels(nfull, nchunks - nfull))) return rc;  // the ragged last chunk
  } else if (nfull > 0 && nfull < nchunks && !general_only && tail_general) {
    // the full chunks with the counts-only coder, a one-token last chunk with the general one
    if ((rc = two_kernels(0, nfull)) || (rc = two_kernels(nfull, nchunks - nfull))) return rc;
  } else {
    if ((rc = two_kernels(0, nchunks))) return rc;
  }

  if (after_part && !split_done && (rc = (*after_part)(0, P, true))) return rc;  // one part: everything is coded
  HIP_TRY(hipEventRecord(w->ws_free, s));
  w->ws_used = true;
  w->last_stream = s;
  return LMC_OK;
}

// lmc_encode_chunks, optionally launched in `nparts` ranges of PLANES (all chunks of the job): after part r,
// after_part(r, planes coded so far, last part?) runs with the context lock held (lmc_store_pack_parts packs the range
// there).  Only a job that takes the fused kernel for every chunk is split; any other job is one part.
static int encode_chunks_parts(lmc_ctx* c, const lmc_kv_layout* src, int32_t tok_begin, int32_t tok_end, int32_t chunk_tokens,
                               const int32_t* bins_h, void* blobs, uint64_t blob_stride, uint32_t* sizes, uint32_t* job_status,
                               lmc_stream_t stream, int nparts, const AfterPart* after_part, bool split_ok) {
  int nchunks;
  if (!encode_job_ok(c, src, tok_begin, tok_end, chunk_tokens, &nchunks, split_ok)) return LMC_ERR_INVALID;
  return encode_job(c, src, nullptr, nchunks, tok_begin, tok_end, chunk_tokens, bins_h, blobs, blob_stride, sizes, job_status, stream,
                    nparts, after_part);
}

int lmc_encode_chunks(lmc_ctx* c, const lmc_kv_layout* src, int32_t tok_begin, int32_t tok_end, int32_t chunk_tokens,
                      const int32_t* bins_h, void* blobs, uint64_t blob_stride, uint32_t* sizes, uint32_t* job_status,
                      lmc_stream_t stream) {
  return encode_chunks_parts(c, src, tok_begin, tok_end, chunk_tokens, bins_h, blobs, blob_stride, sizes, job_status, stream, 1,
                             nullptr, false);
}

// ... and from any source: an LMC_PAGED_SPLIT cache is read in place by k_quantize's split instances (never fused)
int lmc_encode_chunks_split(lmc_ctx* c, const lmc_kv_layout* src, int32_t tok_begin, int32_t tok_end, int32_t chunk_tokens,
                            const int32_t* bins_h, void* blobs, uint64_t blob_stride, uint32_t* sizes, uint32_t* job_status,
                            lmc_stream_t stream) {
  return encode_chunks_parts(c, src, tok_begin, tok_end, chunk_tokens, bins_h, blobs, blob_stride, sizes, job_status, stream, 1,
                             nullptr, true);
}

// Fixed-width blobs of earlier stores -> the entropy-coded blobs of the same KV: k_fixed_expand, then the coder launch
// lmc_encode_chunks would have made behind k_quantize (encode_job).  The blobs are read where they lie, through the pointer
// table; a chunk that does not check out sets the job's status word (its slot then holds the coded blob of a chunk of zero
// symbols, with a size word to match: the status word is the verdict, as for every job).
int lmc_transcode_fixed(lmc_ctx* c, const void* const* blob_ptrs, const uint32_t* blob_bytes, int32_t nchunks, int32_t L, int32_t H,
                        int32_t D, int32_t dtype, int32_t chunk_tokens, uint32_t ntokens, const int32_t* bins_h, void* blobs_out,
                        uint64_t blob_stride, uint32_t* sizes, uint32_t* job_status, lmc_stream_t stream) {
  // (token indices are 32-bit and signed; fixed-width blobs hold 16-bit KV)
  if (!c || !blob_ptrs || !blob_bytes || !chunk_geometry_ok(nchunks, L, H, D, chunk_tokens, ntokens) || ntokens > 0x7fffffffu ||
      (dtype != LMC_DTYPE_BF16 && dtype != LMC_DTYPE_FP16))
    return LMC_ERR_INVALID;
  const FixedSrc fx = {blob_ptrs, blob_bytes, L, H, D, dtype};
  return encode_job(c, nullptr, &fx, nchunks, 0, (int32_t)ntokens, chunk_tokens, bins_h, blobs_out, blob_stride, sizes, job_status, stream,
                    1, nullptr);
}

}  // extern "C"

// One body for the two fixed-width encodes.  `split_ok`: the entry point takes an LMC_PAGED_SPLIT source (encode_job_ok).
static int encode_fixed(lmc_ctx* c, const lmc_kv_layout* src, int32_t tok_begin, int32_t tok_end, int32_t chunk_tokens,
                        const int32_t* bins_h, void* blobs, uint64_t blob_stride, uint32_t* sizes, uint32_t* job_status,
                        lmc_stream_t stream, bool split_ok) {
  int nchunks;
  if (!encode_job_ok(c, src, tok_begin, tok_end, chunk_tokens, &nchunks, split_ok) || lmc_dtype_fp8(src->dtype)) return LMC_ERR_INVALID;
  const int L = src->num_layers, H = src->num_heads, D = src->head_size;
  FixedEncArgs fa;
  memset(&fa, 0, sizeof fa);
  if (!encode_dst_ok(blobs, blob_stride, sizes, L, H, D, chunk_tokens, bins_h, /*fixed_blobs=*/true, &fa.e.bins)) return LMC_ERR_INVALID;
  fa.src = to_addr(src);
  fa.e.tok_begin = tok_begin; fa.e.tok_end = tok_end; fa.e.chunk_tokens = chunk_tokens; fa.e.nchunks = nchunks;
  fa.e.P = 2 * L; fa.e.C = H * D; fa.e.G = (fa.e.C + 63) / 64;
  fa.e.blobs = (u8*)blobs; fa.e.blob_stride = (long long)blob_stride;
  fa.e.sizes = sizes;
  fa.e.status = job_status ? job_status : c->status_h;  // (nothing the kernel can report: kept for the shape of the job)
  fa.e.L = L; fa.e.H = H; fa.e.D = D; fa.e.dtype = src->dtype;
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)stream;
  std::lock_guard<std::mutex> lk(c->mu);  // (the profiling marks are the context's)
  c->pn = 0;
  int rc;
  if ((rc = prof_mark(c, s))) return rc;
  const bool nhdb = src->paged_kind == LMC_PAGED_SPLIT;
  if ((rc = with_kv_dtype16(src->dtype, [&](auto dt) { return launch_fixed_encode<decltype(dt)::value>(fa, s, nhdb); }))) return rc;
  return prof_mark(c, s);
}

extern "C" {

int lmc_encode_chunks_fixed(lmc_ctx* c, const lmc_kv_layout* src, int32_t tok_begin, int32_t tok_end, int32_t chunk_tokens,
                            const int32_t* bins_h, void* blobs, uint64_t blob_stride, uint32_t* sizes, uint32_t* job_status,
                            lmc_stream_t stream) {
  return encode_fixed(c, src, tok_begin, tok_end, chunk_tokens, bins_h, blobs, blob_stride, sizes, job_status, stream, false);
}

int lmc_encode_chunks_fixed_split(lmc_ctx* c, const lmc_kv_layout* src, int32_t tok_begin, int32_t tok_end, int32_t chunk_tokens,
                                  const int32_t* bins_h, void* blobs, uint64_t blob_stride, uint32_t* sizes, uint32_t* job_status,
                                  lmc_stream_t stream) {
  return encode_fixed(c, src, tok_begin, tok_end, chunk_tokens, bins_h, blobs, blob_stride, sizes, job_status, stream, true);
}

// ---- the layer-wise encode (include/lmc_hip.h; k_layers.h) ------------------------------------------------------------
static bool layer_job_ok(const lmc_ctx* c, const lmc_layer_job* j) { return c && j && j->ctx == c && j->b && j->b->busy; }

// caller holds ctx->mu: the job is gone; its buffers go back behind what it queued
static void layer_job_release(lmc_layer_job* j) {
  lmc_layer_bufs* b = j->b;
  if (j->queued && hipEventRecord(b->free_ev, j->last_stream) == hipSuccess) b->used = true;
  b->busy = false;
  delete j;
}

// One body for the two models' begin.  `fixed`: lmc_encode_layers_begin_fixed.
static int layers_begin(lmc_ctx* c, const lmc_kv_layout* src, int32_t tok_begin, int32_t tok_end, int32_t chunk_tokens,
                        const int32_t* bins_h, void* blobs, uint64_t blob_stride, uint32_t* sizes, uint32_t* job_status,
                        lmc_layer_job** job_out, bool fixed) {
  int nchunks;
  if (!job_out) return LMC_ERR_INVALID;
  *job_out = nullptr;
  if (!encode_job_ok(c, src, tok_begin, tok_end, chunk_tokens, &nchunks, true) || (fixed && lmc_dtype_fp8(src->dtype))) return LMC_ERR_INVALID;
  const int L = src->num_layers, H = src->num_heads, D = src->head_size;
  const int P = 2 * L, C = H * D, G = (C + 63) / 64;
  BinsArg bins;
  if (!encode_dst_ok(blobs, blob_stride, sizes, L, H, D, chunk_tokens, bins_h, fixed, &bins)) return LMC_ERR_INVALID;
  // (every refusal is made before this: a job that is refused is refused whether or not it is) eligible: the counts-only coder takes every chunk (2 .. 256 tokens, a ragged last one included) and k_quantize's
  // one-wave-per-oct instances every plane (at most 1024 channels); the fixed-width model has no coder: every chunk
  // length of the one-piece call, the same planes
  const int tail = (tok_end - tok_begin) % chunk_tokens;
  if (C > 1024 ||
      (!fixed && (chunk_tokens < (int)LMC_COUNTS_T_MIN || chunk_tokens > (int)LMC_COUNTS_T || (tail && tail < (int)LMC_COUNTS_T_MIN))))
    return LMC_NOT_LAYERWISE;
  HIP_TRY(hipSetDevice(c->device));
  const int gran = G % 8 == 0 ? G / 8 : G;
  const size_t TQ = ((size_t)chunk_tokens + 3) / 4;
  const size_t need_agg = fixed ? 0 : (size_t)nchunks * 2 * L * gran * 8;
  const size_t need_sym = fixed ? 0 : (size_t)nchunks * 2 * TQ * C * 4;
  const size_t vstride = ((size_t)L * G * lmc_group_cap_bytes((uint32_t)chunk_tokens) + 255) & ~(size_t)255;
  const size_t need_v = fixed ? 0 : (size_t)nchunks * vstride;

  std::lock_guard<std::mutex> lk(c->mu);
  // fixed-width: the passes of a whole chunk's plane (k_fixed_encode: 8 waves take 8, 16 or 32 row octs at a time) are
  // cut into `slices` runs of `slice_passes`: as many as lmc_ctx_set_fixed_layer_slices says, else the smallest power of
  // two that gives a layer's launch a workgroup per CU -- never more slices than passes, and no slice without a pass
  u32 slices = 1, slice_passes = 0;
  if (fixed) {
    const u32 per_pass = C <= 128 ? 32u : C <= 256 ? 16u : 8u;
    const u32 npass = (((u32)chunk_tokens + 7u) / 8u + per_pass - 1u) / per_pass;
    u32 want = (u32)c->fixed_slices;
    if (!want)
      for (want = 1; 2u * want <= npass && (unsigned long long)want * 2u * (u32)nchunks < (unsigned long long)c->num_cus;) want *= 2u;
    want = std::min(want, npass);
    slice_passes = (npass + want - 1u) / want;
    slices = (npass + slice_passes - 1u) / slice_passes;
  }
  const size_t need_part = fixed ? (size_t)nchunks * P * slices * (G + 1) * 4 : 0;
  const auto fits = [&](const lmc_layer_bufs* k) {
    return k->agg.bytes >= need_agg && k->sym4.bytes >= need_sym && k->vregion.bytes >= need_v && k->part.bytes >= need_part;
  };
  lmc_layer_bufs* b = nullptr;
  for (lmc_layer_bufs* k : c->layer_pool)  // idle buffers that are large enough, else any idle ones (grown below)
    if (!k->busy && fits(k)) { b = k; break; }
  for (lmc_layer_bufs* k : c->layer_pool)
    if (!b && !k->busy) b = k;
  if (!b) {
    b = new (std::nothrow) lmc_layer_bufs();
    if (!b) return LMC_ERR_NOMEM;
    hipError_t e = hipEventCreateWithFlags(&b->free_ev, hipEventDisableTiming);
    if (e == hipSuccess) e = hipMalloc(&b->ticket, 64);
    if (e != hipSuccess) {
      g_last_hip = (int)e;
      if (b->free_ev) (void)hipEventDestroy(b->free_ev);
      delete b;
      return LMC_ERR_HIP;
    }
    c->layer_pool.push_back(b);
  }
  if (!fits(b)) {
    // growing frees memory that the previous job's kernels may still use: wait for them (this call only)
    if (b->used) HIP_TRY(hipEventSynchronize(b->free_ev));
    int rc;
    if ((rc = b->agg.grow(need_agg)) || (rc = b->sym4.grow(need_sym)) || (rc = b->vregion.grow(need_v)) || (rc = b->part.grow(need_part))) return rc;
  }
  lmc_layer_job* j = new (std::nothrow) lmc_layer_job();
  if (!j) return LMC_ERR_NOMEM;
  j->ctx = c; j->b = b; j->src = *src; j->bins = bins;
  j->tok_begin = tok_begin; j->tok_end = tok_end; j->chunk_tokens = chunk_tokens; j->nchunks = nchunks;
  j->blobs = (u8*)blobs; j->blob_stride = blob_stride; j->sizes = sizes;
  j->status = job_status ? job_status : c->status_h;
  j->chain_gran = gran; j->vstride = (long long)vstride;
  j->fixed = fixed; j->slices = slices; j->slice_passes = slice_passes;
  b->busy = true;
  *job_out = j;
  return LMC_OK;
}

int lmc_encode_layers_begin(lmc_ctx* c, const lmc_kv_layout* src, int32_t tok_begin, int32_t tok_end, int32_t chunk_tokens,
                            const int32_t* bins_h, void* blobs, uint64_t blob_stride, uint32_t* sizes, uint32_t* job_status,
                            lmc_layer_job** job_out) {
  return layers_begin(c, src, tok_begin, tok_end, chunk_tokens, bins_h, blobs, blob_stride, sizes, job_status, job_out, false);
}

int lmc_encode_layers_begin_fixed(lmc_ctx* c, const lmc_kv_layout* src, int32_t tok_begin, int32_t tok_end, int32_t chunk_tokens,
                                  const int32_t* bins_h, void* blobs, uint64_t blob_stride, uint32_t* sizes, uint32_t* job_status,
                                  lmc_layer_job** job_out) {
  return layers_begin(c, src, tok_begin, tok_end, chunk_tokens, bins_h, blobs, blob_stride, sizes, job_status, job_out, true);
}

// the coder's view of the job (EncodeArgs of every launch but for its planes)
static EncodeArgs layer_encode_args(const lmc_layer_job* j) {
  const lmc_kv_layout* src = &j->src;
  EncodeArgs ea;
  memset(&ea, 0, sizeof ea);
  ea.sym4 = j->b->sym4.p;
  ea.tok_begin = j->tok_begin; ea.tok_end = j->tok_end; ea.chunk_tokens = j->chunk_tokens; ea.nchunks = j->nchunks;
  ea.L = src->num_layers; ea.H = src->num_heads; ea.D = src->head_size;
  ea.P = 2 * ea.L; ea.C = ea.H * ea.D; ea.G = (ea.C + 63) / 64; ea.TQ = (j->chunk_tokens + 3) / 4;
  ea.sym_stride = (long long)ea.TQ * ea.C;
  ea.blobs = j->blobs; ea.blob_stride = (long long)j->blob_stride;
  ea.status = j->status;
  ea.bins = j->bins;
  ea.agg = j->b->agg.p; ea.sizes = j->sizes;
  ea.dtype = lmc_math_dtype(src->dtype);
  ea.ticket = j->b->ticket;
  ea.chain_gran = j->chain_gran;
  ea.vregion = j->b->vregion.p; ea.vstride = j->vstride;
  return ea;
}

// One layer of a job, per model; the caller (lmc_encode_layer) has ordered `s` behind the buffers' previous job.
// Fixed-width: one launch -- planes `layer` and L + `layer` in slices; nothing to zero (k_fixed.h, FixedEncArgs).
static int encode_layer_fixed(lmc_layer_job* j, int layer, hipStream_t s) {
  FixedEncArgs fa;
  memset(&fa, 0, sizeof fa);
  fa.src = to_addr(&j->src);
  fa.e = layer_encode_args(j);
  fa.e.dtype = j->src.dtype;
  fa.e.sizes = layer == 0 ? j->sizes : nullptr;  // 0 = "this chunk's encode did not finish" until k_fixed_layers_finish
  fa.e.plane0 = layer; fa.e.plane_step = fa.e.L; fa.e.nplanes = 2;
  fa.part = j->b->part.p; fa.slice_passes = j->slice_passes;
  const bool nhdb = j->src.paged_kind == LMC_PAGED_SPLIT;
  return with_kv_dtype16(j->src.dtype, [&](auto dt) { return launch_fixed_encode<decltype(dt)::value, true>(fa, s, nhdb, j->slices); });
}
// Coded: k_quantize of the layer's two planes, then the counts-only coder over their streams.
static int encode_layer_coded(lmc_layer_job* j, int layer, hipStream_t s) {
  lmc_layer_bufs* b = j->b;
  EncodeArgs ea = layer_encode_args(j);
  const int L = ea.L;
  if (layer == 0) {
    // the job's first launch: granules and tickets start from zero ONCE -- the later layers' look-backs read the prefixes
    // this and every earlier layer leave
    HIP_TRY(hipMemsetAsync(b->agg.p, 0, (size_t)j->nchunks * 2 * L * j->chain_gran * 8, s));
    HIP_TRY(hipMemsetAsync(b->ticket, 0, 64, s));
    j->tickets_drawn = 0;
  }
  ea.plane0 = layer; ea.plane_step = L; ea.nplanes = 2;
  lmc_blob_header hl;
  lmc_blob_layout((uint32_t)L, (uint32_t)j->chunk_tokens, (uint32_t)ea.H, (uint32_t)ea.D, &hl);
  QuantArgs qa;
  memset(&qa, 0, sizeof qa);
  qa.src = to_addr(&j->src); qa.bins = j->bins;
  qa.tok_begin = j->tok_begin; qa.tok_end = j->tok_end; qa.chunk_tokens = j->chunk_tokens; qa.nchunks = j->nchunks;
  qa.P = ea.P; qa.C = ea.C; qa.TQ = ea.TQ; qa.pc_limit = j->nchunks * ea.P; qa.sym_stride = ea.sym_stride;
  qa.sym4 = b->sym4.p;
  qa.scale_base = j->blobs + hl.off_scales; qa.scale_stride = (long long)j->blob_stride;
  qa.sizes = layer == 0 ? j->sizes : nullptr;  // 0 = "this chunk's encode did not finish" until k_layers_finish
  qa.plane0 = layer; qa.plane_step = L; qa.nplanes = 2;
  const int rc = launch_quant<true>(qa, s, j->src.paged_kind == LMC_PAGED_SPLIT);
  if (rc) return rc;
  const long long ngroups = (long long)j->nchunks * 2 * ea.G;
  const unsigned nwg = (unsigned)((ngroups + 7) / 8);
  ea.ticket_base = j->tickets_drawn;
  hipLaunchKernelGGL((k_cdf_encode<true, true, 8, true>), dim3(nwg), dim3(64 * 8), 0, s, ea);
  HIP_TRY(hipGetLastError());
  j->tickets_drawn += nwg;
  return LMC_OK;
}

int lmc_encode_layer(lmc_ctx* c, lmc_layer_job* j, int32_t layer, lmc_stream_t stream) {
  if (!c) return LMC_ERR_INVALID;
  std::lock_guard<std::mutex> lk(c->mu);
  if (!layer_job_ok(c, j) || layer != j->next_layer || layer >= j->src.num_layers) return LMC_ERR_INVALID;
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)stream;
  if (layer == 0 && j->b->used) HIP_TRY(hipStreamWaitEvent(s, j->b->free_ev, 0));  // behind the buffers' previous job
  const int rc = j->fixed ? encode_layer_fixed(j, layer, s) : encode_layer_coded(j, layer, s);
  j->queued = true; j->last_stream = s;  // (a failed launch too: what went out before it is on that stream)
  if (rc) return rc;
  j->next_layer = layer + 1;
  return LMC_OK;
}

// The job's last launch, per model: the headers, sizes and -- coded -- the move of the V streams behind the K streams.
static void layers_finish_fixed(const lmc_layer_job* j, hipStream_t s) {
  FixedFinishArgs ff;
  memset(&ff, 0, sizeof ff);
  ff.e = layer_encode_args(j);
  ff.e.dtype = j->src.dtype;
  ff.part = j->b->part.p; ff.nslices = j->slices;
  hipLaunchKernelGGL(k_fixed_layers_finish, dim3((unsigned)j->nchunks), dim3(FIXED_FIN_THREADS), 0, s, ff);
}
static void layers_finish_coded(const lmc_layer_job* j, hipStream_t s) {
  LayersFinishArgs fa;
  memset(&fa, 0, sizeof fa);
  fa.e = layer_encode_args(j);
  fa.kv_dtype = lmc_dtype_fp8(j->src.dtype) ? (u32)j->src.dtype : 0u;
  // the move of a chunk's V streams in pieces of 16 KiB per pass of a workgroup
  const unsigned nx = (unsigned)std::min<long long>(64, std::max<long long>(1, j->vstride / (16 * 256 * 4)));
  hipLaunchKernelGGL(k_layers_finish, dim3(nx, (unsigned)j->nchunks), dim3(256), 0, s, fa);
}

int lmc_encode_layers_finish(lmc_ctx* c, lmc_layer_job* j, lmc_stream_t stream) {
  if (!c) return LMC_ERR_INVALID;
  std::lock_guard<std::mutex> lk(c->mu);
  if (!layer_job_ok(c, j) || j->next_layer != j->src.num_layers) return LMC_ERR_INVALID;
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)stream;
  if (j->fixed) layers_finish_fixed(j, s);
  else layers_finish_coded(j, s);
  HIP_TRY(hipGetLastError());  // (the job stays live: the caller aborts it)
  j->queued = true; j->last_stream = s;
  layer_job_release(j);
  return LMC_OK;
}

int lmc_encode_layers_abort(lmc_ctx* c, lmc_layer_job* j) {
  if (!c) return LMC_ERR_INVALID;
  std::lock_guard<std::mutex> lk(c->mu);
  if (!layer_job_ok(c, j)) return LMC_ERR_INVALID;
  (void)hipSetDevice(c->device);
  layer_job_release(j);
  return LMC_OK;
}

// A decode job's arguments in three steps, every refusal LMC_ERR_INVALID and none of them queues anything:
// decode_geometry -- `nchunks` blobs of L layers x H heads x D, every layer (the ranged launches narrow that);
static int decode_geometry(lmc_ctx* c, int nchunks, int L, int H, int D, uint32_t* job_status, DecodeArgs& a) {
  memset(&a, 0, sizeof a);
  if (!c || nchunks < 1) return LMC_ERR_INVALID;
  a.nchunks = nchunks; a.layer_count = L;
  a.P = 2 * L; a.C = H * D; a.G = (a.C + 63) / 64;
  a.wc_hi = a.C; a.wGw = a.G;  // the full head window (k_decode.h): every channel stored, every group launched
  // k_decode numbers its streams (chunk, plane, group) in 32 bits: 2^31 of them would be > 10^11 tokens in one call
  if ((long long)nchunks * a.P * a.G >= (1ll << 31)) return LMC_ERR_INVALID;
  a.status = job_status ? job_status : c->status_h;
  return LMC_OK;
}
// decode_common -- ... of the geometry of `dst`, into it from token dst_tok0 on: what every entry point with a
// destination asks of it (lmc_decode_symbols has none) before it looks at anything else of `dst`.  `split_ok`: the entry
// point takes an LMC_PAGED_SPLIT destination -- the four the engine's retrieve paths use; lmc_decode_chunks does not;
static int decode_common(lmc_ctx* c, int nchunks, const lmc_kv_layout* dst, int dst_tok0, long long chunk_tokens,
                         uint32_t* job_status, DecodeArgs& a, bool split_ok = false) {
  if (!layout_ok(dst, false, split_ok) || chunk_tokens < 1 || !decode_dst_ok(dst, chunk_tokens)) return LMC_ERR_INVALID;
  const int rc = decode_geometry(c, nchunks, dst->num_layers, dst->num_heads, dst->head_size, job_status, a);
  if (rc) return rc;
  a.dst = to_addr(dst); a.dst_tok0 = dst_tok0; a.chunk_tokens = (int)chunk_tokens;
  return LMC_OK;
}
// decode_blobs -- the caller's blobs, `stride` bytes apart from `blobs` on or, with blob_ptrs, each at its own address
// (`blobs` is only a non-null placeholder then).  The load paths decode from their own staging and set the two fields.
static bool decode_blobs(DecodeArgs& a, const void* blobs, uint64_t stride, const void* const* blob_ptrs = nullptr) {
  if (!blobs || ((uintptr_t)blobs & 15) || (stride & 15)) return false;
  a.blobs = (const u8*)blobs; a.blob_stride = (long long)stride; a.blob_ptrs = (const u8* const*)blob_ptrs;
  return true;
}

// k_decode for a destination: its dtype decides what a blob decodes to (any blob, any of the four), its kind how the
// tokens are found
static void launch_decode(const lmc_kv_layout* dst, dim3 grid, hipStream_t s, const DecodeArgs& a) {
  with_kv_dtype(dst->dtype, [&](auto dt) {
    with_decode_kind(dst, [&](auto kind) {
      hipLaunchKernelGGL((k_decode<DEC_SINK_KV, decltype(dt)::value, decltype(kind)::value>), grid, dim3(64 * DEC_WAVES), 0, s, a);
    });
  });
}

// One range of layers of a decode: k_decode over the streams of layers [l0, l0 + nl) of the job's chunks, then `ev`
// (if any) recorded behind it.  The lock is not needed for the launch itself: the load paths call this with c->mu held.
static int range_post(lmc_ctx* c, const lmc_kv_layout* dst, const lmc_range_post* post, int l0, int nl, hipStream_t s);
// k_fixed_decode (LMC_MODEL_FIXED blobs) for a 16-bit destination, rows or an LMC_PAGED_SPLIT cache: a wave per stream,
// FIXED_DEC_WAVES per workgroup
static void launch_fixed_decode(const lmc_kv_layout* dst, long long nstreams, hipStream_t s, const DecodeArgs& a) {
  FixedDecArgs fa;
  fa.d = a;
  fa.vec = layout_ok(dst) ? 1 : 0;  // rows that take 16-byte vectors of 8 channels: what the encoders ask of a source
  if (a.w_src_heads && (dst->head_size & 7)) fa.vec = 0;  // a head window moves heads: a vector must lie inside one (k_fixed.h)
  if (dst->paged_kind == LMC_PAGED_SPLIT) fa.vec = 0;  // (the kernel looks at the plane's own alignment: k_fixed.h)
  const dim3 grid((unsigned)((nstreams + FIXED_DEC_WAVES - 1) / FIXED_DEC_WAVES)), block(64 * FIXED_DEC_WAVES);
  with_kv_dtype16(dst->dtype, [&](auto dt) {
    with_decode_kind(dst, [&](auto kind) {
      hipLaunchKernelGGL((k_fixed_decode<decltype(dt)::value, decltype(kind)::value>), grid, block, 0, s, fa);
    });
  });
}

static int decode_range_locked(DecodeArgs& a, const lmc_kv_layout* dst, int l0, int nl, hipStream_t s, lmc_event_t ev,
                               lmc_ctx* c = nullptr, const lmc_range_post* post = nullptr, bool fixed = false) {
  a.layer_begin = l0; a.layer_count = nl;
  const long long n = (long long)a.nchunks * 2 * nl * a.wGw;  // (wGw == G but for a head window: the groups it touches)
  const dim3 grid((unsigned)((n + DEC_WAVES - 1) / DEC_WAVES));
  if (fixed) launch_fixed_decode(dst, n, s, a);
  else launch_decode(dst, grid, s, a);
  HIP_TRY(hipGetLastError());
  if (post) {  // (none of its launches needs the lock)
    const int rc = range_post(c, dst, post, l0, nl, s);
    if (rc) return rc;
  }
  if (ev) HIP_TRY(hipEventRecord((hipEvent_t)ev, s));
  return LMC_OK;
}

// The same for the decode entry points, which do not hold the lock: taken here, and the launch bracketed by the
// profiling marks (the range's event follows the second mark).
static int decode_range(lmc_ctx* c, DecodeArgs& a, const lmc_kv_layout* dst, int l0, int nl, hipStream_t s, lmc_event_t ev,
                        const lmc_range_post* post = nullptr, bool fixed = false) {
  int rc;
  {
    std::lock_guard<std::mutex> lk(c->mu);
    c->pn = 0;
    if ((rc = prof_mark(c, s))) return rc;
    if ((rc = decode_range_locked(a, dst, l0, nl, s, nullptr, nullptr, nullptr, fixed))) return rc;
    if ((rc = prof_mark(c, s))) return rc;
  }
  if (post && (rc = range_post(c, dst, post, l0, nl, s))) return rc;
  if (ev) HIP_TRY(hipEventRecord((hipEvent_t)ev, s));
  return LMC_OK;
}

int lmc_decode_chunks(lmc_ctx* c, const void* blobs, uint64_t blob_stride, int32_t nchunks, const lmc_kv_layout* dst,
                      int32_t dst_tok0, int32_t chunk_tokens, uint32_t* job_status, lmc_stream_t stream) {
  DecodeArgs a;
  const int rc = decode_common(c, nchunks, dst, dst_tok0, chunk_tokens, job_status, a);
  if (rc) return rc;
  if (!decode_blobs(a, blobs, blob_stride)) return LMC_ERR_INVALID;
  HIP_TRY(hipSetDevice(c->device));
  return decode_range(c, a, dst, 0, dst->num_layers, (hipStream_t)stream, nullptr);
}

int lmc_decode_chunks_layers(lmc_ctx* c, const void* const* blob_ptrs, uint64_t max_blob_bytes, int32_t nchunks,
                             const lmc_kv_layout* dst, int32_t dst_tok0, int32_t chunk_tokens, int32_t layer_begin,
                             int32_t layer_count, uint32_t* job_status, lmc_stream_t stream) {
  DecodeArgs a;
  const int rc = decode_common(c, nchunks, dst, dst_tok0, chunk_tokens, job_status, a, true);
  if (rc) return rc;
  if (!decode_blobs(a, blob_ptrs, (max_blob_bytes + 15) & ~(uint64_t)15, blob_ptrs) || layer_begin < 0 || layer_count < 1 ||
      layer_begin + layer_count > dst->num_layers)
    return LMC_ERR_INVALID;
  HIP_TRY(hipSetDevice(c->device));
  return decode_range(c, a, dst, layer_begin, layer_count, (hipStream_t)stream, nullptr);
}

static bool post_ok(const lmc_kv_layout* dst, const lmc_range_post* post);

// One body for the two schedules: the coded models' k_decode, or -- `fixed` -- k_fixed_decode for LMC_MODEL_FIXED blobs,
// which fills 16-bit rows and -- `fixed_split`: lmc_decode_chunks_fixed_split_schedule -- a 16-bit LMC_PAGED_SPLIT cache
// (lmc_decode_chunks_fixed_schedule keeps refusing one: such a cache is filled through a staged chunk and
// post->scatter_dst there).
// `win` (lmc_decode_chunks_*_heads_schedule; NULL: none, the launches are the ones they were): the blobs have win->src_heads
// heads of dst->head_size, and heads [src_head_begin, + nheads) of every blob go to heads [dst_head_begin, ...) of `dst`,
// which keeps its own head count.  Everything asked of `dst` -- the 32-bit offset rule included -- is asked of dst's own
// geometry by decode_common; the blob's C and G and the window's channels and groups replace what it derived from dst.
static int decode_schedule(lmc_ctx* c, const void* const* blob_ptrs, uint64_t max_blob_bytes, int32_t nchunks,
                           const lmc_kv_layout* dst, int32_t dst_tok0, int32_t chunk_tokens, int32_t nranges,
                           const int32_t* layer_ends_h, const lmc_event_t* events_h, uint32_t* job_status,
                           lmc_stream_t stream, const lmc_range_post* post, bool fixed, bool fixed_split = false,
                           const lmc_head_window* win = nullptr) {
  DecodeArgs a;
  int rc = decode_common(c, nchunks, dst, dst_tok0, chunk_tokens, job_status, a, !fixed || fixed_split);
  if (rc) return rc;
  if (win) {
    const long long D = dst->head_size, Cs = (long long)win->src_heads * D;
    if (win->src_heads < 1 || win->nheads < 1 || win->src_head_begin < 0 || win->dst_head_begin < 0 ||
        (long long)win->src_head_begin + win->nheads > win->src_heads ||
        (long long)win->dst_head_begin + win->nheads > dst->num_heads || (Cs & 7) || Cs > LMC_MAX_CHANNELS)
      return LMC_ERR_INVALID;
    a.C = (int)Cs; a.G = (a.C + 63) / 64;
    if ((long long)nchunks * a.P * a.G >= (1ll << 31)) return LMC_ERR_INVALID;  // decode_geometry's bound, on the blob's groups
    a.wc_lo = win->src_head_begin * (int)D; a.wc_hi = a.wc_lo + win->nheads * (int)D;
    a.wg_lo = a.wc_lo / 64; a.wGw = (a.wc_hi - 1) / 64 - a.wg_lo + 1;
    a.wh_shift = win->dst_head_begin - win->src_head_begin;
    a.w_src_heads = win->src_heads;
  }
  if (fixed && (lmc_dtype_fp8(dst->dtype) || max_blob_bytes < LMC_HEADER_BYTES)) return LMC_ERR_INVALID;
  if (!decode_blobs(a, blob_ptrs, (max_blob_bytes + 15) & ~(uint64_t)15, blob_ptrs) || nranges < 1 || !layer_ends_h)
    return LMC_ERR_INVALID;
  if (fixed) a.blob_stride = (long long)max_blob_bytes;  // the read bound itself: k_fixed_decode reads nothing speculatively
  for (int i = 0, prev = 0; i < nranges; prev = layer_ends_h[i], i++)  // the whole schedule is checked before anything is launched
    if (layer_ends_h[i] <= prev || layer_ends_h[i] > dst->num_layers) return LMC_ERR_INVALID;
  if (layer_ends_h[nranges - 1] != dst->num_layers || !post_ok(dst, post)) return LMC_ERR_INVALID;
  HIP_TRY(hipSetDevice(c->device));
  for (int i = 0, prev = 0; i < nranges; prev = layer_ends_h[i], i++)
    if ((rc = decode_range(c, a, dst, prev, layer_ends_h[i] - prev, (hipStream_t)stream, events_h ? events_h[i] : nullptr, post, fixed)))
      return rc;
  return LMC_OK;
}

int lmc_decode_chunks_schedule_post(lmc_ctx* c, const void* const* blob_ptrs, uint64_t max_blob_bytes, int32_t nchunks,
                                    const lmc_kv_layout* dst, int32_t dst_tok0, int32_t chunk_tokens, int32_t nranges,
                                    const int32_t* layer_ends_h, const lmc_event_t* events_h, uint32_t* job_status,
                                    lmc_stream_t stream, const lmc_range_post* post) {
  return decode_schedule(c, blob_ptrs, max_blob_bytes, nchunks, dst, dst_tok0, chunk_tokens, nranges, layer_ends_h, events_h,
                         job_status, stream, post, false);
}

int lmc_decode_chunks_fixed_schedule(lmc_ctx* c, const void* const* blob_ptrs, uint64_t max_blob_bytes, int32_t nchunks,
                                     const lmc_kv_layout* dst, int32_t dst_tok0, int32_t chunk_tokens, int32_t nranges,
                                     const int32_t* layer_ends_h, const lmc_event_t* events_h, const lmc_range_post* post,
                                     uint32_t* job_status, lmc_stream_t stream) {
  return decode_schedule(c, blob_ptrs, max_blob_bytes, nchunks, dst, dst_tok0, chunk_tokens, nranges, layer_ends_h, events_h,
                         job_status, stream, post, true);
}

int lmc_decode_chunks_fixed_split_schedule(lmc_ctx* c, const void* const* blob_ptrs, uint64_t max_blob_bytes, int32_t nchunks,
                                           const lmc_kv_layout* dst, int32_t dst_tok0, int32_t chunk_tokens, int32_t nranges,
                                           const int32_t* layer_ends_h, const lmc_event_t* events_h, const lmc_range_post* post,
                                           uint32_t* job_status, lmc_stream_t stream) {
  return decode_schedule(c, blob_ptrs, max_blob_bytes, nchunks, dst, dst_tok0, chunk_tokens, nranges, layer_ends_h, events_h,
                         job_status, stream, post, true, true);
}

int lmc_decode_chunks_heads_schedule(lmc_ctx* c, const void* const* blob_ptrs, uint64_t max_blob_bytes, int32_t nchunks,
                                     const lmc_kv_layout* dst, int32_t dst_tok0, int32_t chunk_tokens, int32_t nranges,
                                     const int32_t* layer_ends_h, const lmc_event_t* events_h, const lmc_head_window* win,
                                     uint32_t* job_status, lmc_stream_t stream) {
  if (!win) return LMC_ERR_INVALID;
  return decode_schedule(c, blob_ptrs, max_blob_bytes, nchunks, dst, dst_tok0, chunk_tokens, nranges, layer_ends_h, events_h,
                         job_status, stream, nullptr, false, false, win);
}

int lmc_decode_chunks_fixed_heads_schedule(lmc_ctx* c, const void* const* blob_ptrs, uint64_t max_blob_bytes, int32_t nchunks,
                                           const lmc_kv_layout* dst, int32_t dst_tok0, int32_t chunk_tokens, int32_t nranges,
                                           const int32_t* layer_ends_h, const lmc_event_t* events_h, const lmc_head_window* win,
                                           uint32_t* job_status, lmc_stream_t stream) {
  if (!win) return LMC_ERR_INVALID;
  return decode_schedule(c, blob_ptrs, max_blob_bytes, nchunks, dst, dst_tok0, chunk_tokens, nranges, layer_ends_h, events_h,
                         job_status, stream, nullptr, true, true, win);
}

int lmc_decode_chunks_schedule(lmc_ctx* c, const void* const* blob_ptrs, uint64_t max_blob_bytes, int32_t nchunks,
                               const lmc_kv_layout* dst, int32_t dst_tok0, int32_t chunk_tokens, int32_t nranges,
                               const int32_t* layer_ends_h, const lmc_event_t* events_h, uint32_t* job_status,
                               lmc_stream_t stream) {
  return lmc_decode_chunks_schedule_post(c, blob_ptrs, max_blob_bytes, nchunks, dst, dst_tok0, chunk_tokens, nranges, layer_ends_h,
                                         events_h, job_status, stream, nullptr);
}

int lmc_decode_symbols(lmc_ctx* c, const void* blob, int32_t L, int32_t H, int32_t D, int8_t* sym_out,
                       lmc_stream_t stream) {
  if (!sym_out || L < 1 || H < 1 || D < 1 || (H * (long long)D) % 8) return LMC_ERR_INVALID;
  DecodeArgs a;
  const int rc = decode_geometry(c, 1, L, H, D, nullptr, a);
  if (rc) return rc;
  if (!decode_blobs(a, blob, 0)) return LMC_ERR_INVALID;
  a.sym_out = sym_out;
  HIP_TRY(hipSetDevice(c->device));
  const long long n = (long long)a.P * a.G;  // every layer (decode_geometry set the full range)
  hipLaunchKernelGGL((k_decode<DEC_SINK_SYM, LMC_DTYPE_BF16, DEC_ROWS>), dim3((unsigned)((n + DEC_WAVES - 1) / DEC_WAVES)), dim3(64 * DEC_WAVES), 0, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return LMC_OK;
}

// Entropy-coded blobs of earlier stores -> the fixed-width blobs of the same KV: ONE launch of the rANS decoder with its
// fixed-width sink (k_decode.h, DEC_SINK_FIXED), a wave per stream over all layers.  No workspace (neither the KV nor the
// symbols are staged) and no host wait.  The refusals are lmc_transcode_fixed's.
int lmc_transcode_to_fixed(lmc_ctx* c, const void* const* blob_ptrs, const uint32_t* blob_bytes, int32_t nchunks, int32_t L, int32_t H,
                           int32_t D, int32_t dtype, int32_t chunk_tokens, uint32_t ntokens, const int32_t* bins_h,
                           void* const* out_ptrs, const uint32_t* out_bytes, uint32_t* job_status, lmc_stream_t stream) {
  if (!c || !blob_ptrs || !blob_bytes || !out_ptrs || !out_bytes || !chunk_geometry_ok(nchunks, L, H, D, chunk_tokens, ntokens) ||
      ntokens > 0x7fffffffu || (dtype != LMC_DTYPE_BF16 && dtype != LMC_DTYPE_FP16))
    return LMC_ERR_INVALID;
  DecodeArgs a;
  if (decode_geometry(c, nchunks, L, H, D, job_status, a)) return LMC_ERR_INVALID;  // (2^31 streams or more)
  if (!bins_ok(bins_h, 2 * L, &a.bins)) return LMC_ERR_INVALID;
  // the header's size words, and the kernel's sums of stream sizes, are 32 bits
  if (lmc_fixed_blob_bytes((uint32_t)L, (uint32_t)chunk_tokens, (uint32_t)H, (uint32_t)D, a.bins.b) > 0xffffffffull) return LMC_ERR_INVALID;
  a.blob_ptrs = (const u8* const*)blob_ptrs; a.blob_bytes = blob_bytes;
  a.out_ptrs = (u8* const*)out_ptrs; a.out_bytes = out_bytes;
  a.chunk_tokens = chunk_tokens; a.tok_end = (int)ntokens;
  a.L = L; a.H = H; a.D = D; a.dtype = dtype;
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)stream;
  std::lock_guard<std::mutex> lk(c->mu);  // (the profiling marks are the context's)
  c->pn = 0;
  int rc;
  if ((rc = prof_mark(c, s))) return rc;
  const long long n = (long long)nchunks * a.P * a.G;  // every layer (decode_geometry set the full range)
  hipLaunchKernelGGL((k_decode<DEC_SINK_FIXED, LMC_DTYPE_BF16, DEC_ROWS>), dim3((unsigned)((n + DEC_WAVES - 1) / DEC_WAVES)), dim3(64 * DEC_WAVES), 0, s, a);
  HIP_TRY(hipGetLastError());
  return prof_mark(c, s);
}

}  // extern "C"

// One side of lmc_copy_kv is LMC_PAGED_SPLIT (k_copy_split.h): a wave per (plane, head, tile of TT tokens).
static int copy_split(lmc_ctx* c, const lmc_kv_layout* src, int32_t tok_begin, int32_t ntok, const lmc_kv_layout* dst,
                      int32_t dst_tok0, hipStream_t stream) {
  const bool gather = src->paged_kind == LMC_PAGED_SPLIT;
  const lmc_kv_layout* sp = gather ? src : dst;
  const lmc_kv_layout* rw = gather ? dst : src;
  const bool b8 = lmc_dtype_fp8(sp->dtype);
  const int X = b8 ? 16 : 8;  // elements of a 16-byte granule
  const int tt = sp->block_size % 32 == 0 ? 32 : sp->block_size % 16 == 0 ? 16 : 8;
  SplitCopyArgs a;
  memset(&a, 0, sizeof a);
  a.sp = to_addr(sp); a.rw = to_addr(rw);
  a.sp_tok0 = gather ? tok_begin : dst_tok0; a.rw_tok0 = gather ? dst_tok0 : tok_begin; a.ntok = ntok;
  a.P = 2 * sp->num_layers;
  a.ntiles = (int)(((long long)ntok + 2 * tt - 2) / tt);  // the first tile may begin tt - 1 positions in front of the range
  const size_t image = (size_t)tt * sp->head_size * (b8 ? 1 : 2);
  auto mult = [X](int64_t v) { return v % X == 0; };
  a.fast = sp->head_size / X >= 4 && image <= SPLIT_MAX_IMAGE && mult(sp->stride_block) && mult(sp->stride_head) &&
           (sp->plane_ptrs || (mult(sp->stride_layer) && mult(sp->stride_kv))) && mult(rw->stride_token) &&
           mult(rw->stride_head) && (!rw->slot_mapping || mult(rw->stride_block)) &&
           (rw->plane_ptrs || (mult(rw->stride_layer) && mult(rw->stride_kv)));
  HIP_TRY(hipSetDevice(c->device));
  const long long items = (long long)a.P * a.ntiles * sp->num_heads;
  long long blocks = (items + SPLIT_WAVES - 1) / SPLIT_WAVES;
  if (blocks > 8LL * c->num_cus) blocks = 8LL * c->num_cus;  // grid-stride beyond eight workgroups per CU
  const size_t lds = a.fast ? SPLIT_WAVES * image : 0;
  with_bool(b8, [&](auto e8) {
    with_bool(gather, [&](auto g) {
      with_int<32, 16, 8>(tt, [&](auto t) {
        using E = std::conditional_t<decltype(e8)::value, u8, u16>;
        hipLaunchKernelGGL((k_copy_split<E, decltype(g)::value, decltype(t)::value>), dim3((unsigned)blocks), dim3(64 * SPLIT_WAVES), lds, stream, a);
      });
    });
  });
  HIP_TRY(hipGetLastError());
  return LMC_OK;
}

// What lmc_copy_kv asks of its two layouts and its range (every refusal LMC_ERR_INVALID, nothing launched).
static bool copy_kv_ok(const lmc_kv_layout* src, int32_t tok_begin, int32_t ntok, const lmc_kv_layout* dst, int32_t dst_tok0) {
  if (!layout_ok(src, false, true) || !layout_ok(dst, false, true) || ntok < 1 || tok_begin < 0 || dst_tok0 < 0) return false;
  if (src->num_layers != dst->num_layers || src->num_heads != dst->num_heads || src->head_size != dst->head_size ||
      src->dtype != dst->dtype)
    return false;
  return !(src->paged_kind == LMC_PAGED_SPLIT && dst->paged_kind == LMC_PAGED_SPLIT);  // one side is rows
}

// A rotation as lmc_rope_shift takes it.
struct RopeSpec {
  const float* cos_sin;
  int32_t table_rows, rot_dim, is_neox, delta;
  const int32_t* deltas;
};
// 16-byte accesses to the table and whole 8-channel vectors per pair half (k_rope_vec)
static bool rope_vec_ok(const RopeSpec& r) {
  return r.rot_dim % (r.is_neox ? 16 : 8) == 0 && ((uintptr_t)r.cos_sin & 15) == 0;
}
// The access form is chosen as lmc_copy_kv chooses `vec`; -> the work items of one head
static bool rope_vec(const lmc_kv_layout* kv, const RopeSpec& r) { return layout_ok(kv) && kv->head_size % 8 == 0 && rope_vec_ok(r); }
static int rope_per_head(const lmc_kv_layout* kv, const RopeSpec& r) {
  return rope_vec(kv, r) ? r.rot_dim / (r.is_neox ? 16 : 8) : r.rot_dim / 2;
}
// ... and what lmc_rope_shift asks of it, of the rows it rotates and of their range.
static bool rope_ok(const lmc_kv_layout* kv, int32_t tok_begin, int32_t ntok, const RopeSpec& r) {
  if (!layout_ok(kv, false) || lmc_dtype_fp8(kv->dtype) || ntok < 1 || tok_begin < 0 || !r.cos_sin || r.table_rows < 1) return false;
  if (r.rot_dim < 2 || (r.rot_dim & 1) || r.rot_dim > kv->head_size) return false;
  if (!r.deltas && (r.delta <= -r.table_rows || r.delta >= r.table_rows)) return false;
  // the work items of one layer: the kernels index them with 32 bits
  return (long long)ntok * kv->num_heads * rope_per_head(kv, r) < (1ll << 31);
}

// Re-rotate the keys of tokens [tok_begin, +ntok) by a position difference, in place (k_rope.h).  The access form is
// chosen as lmc_copy_kv chooses `vec`: 16-byte vectors where the rows, the head and the pair halves are whole vectors
// (and the table's rows are), one pair per thread for everything else.
static void launch_rope(int dtype, bool vec, bool neox, dim3 grid, size_t lds, hipStream_t s, const RopeArgs& a) {
  with_kv_dtype16(dtype, [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    if (!vec) hipLaunchKernelGGL((k_rope_elem<DT>), grid, dim3(256), 0, s, a);
    else with_bool(neox, [&](auto nx) { hipLaunchKernelGGL((k_rope_vec<DT, decltype(nx)::value>), grid, dim3(256), lds, s, a); });
  });
}

// lmc_rope_shift behind its checks (rope_ok).
static int rope_launch(lmc_ctx* c, const lmc_kv_layout* kv, int32_t tok_begin, int32_t ntok, const RopeSpec& r,
                       uint32_t* job_status, hipStream_t stream) {
  const bool neox = r.is_neox != 0;
  const int rot_dim = r.rot_dim;
  const bool vec = rope_vec(kv, r);
  RopeArgs a;
  memset(&a, 0, sizeof a);
  a.kv = to_addr(kv);
  a.cos_sin = r.cos_sin; a.deltas = r.deltas; a.status = job_status ? job_status : c->status_h;
  a.tok_begin = tok_begin; a.ntok = ntok; a.rot = rot_dim; a.table_rows = r.table_rows; a.delta = r.delta; a.neox = neox;
  a.per_head = (u32)rope_per_head(kv, r);
  const long long nitems = (long long)ntok * kv->num_heads * a.per_head;  // of one layer (< 2^31: rope_ok)
  a.nitems = (u32)nitems;
  HIP_TRY(hipSetDevice(c->device));
  long long blocks = (nitems + 255) / 256;
  const long long cap = std::max(1ll, 64ll * c->num_cus / kv->num_layers);  // grid-stride beyond 64 blocks per CU
  if (blocks > cap) blocks = cap;
  const dim3 grid((unsigned)blocks, (unsigned)kv->num_layers);
  const size_t lds = vec && !r.deltas ? (size_t)rot_dim * sizeof(float) : 0;  // the one table row of a uniform delta
  launch_rope(kv->dtype, vec, neox, grid, lds, stream, a);
  HIP_TRY(hipGetLastError());
  return LMC_OK;
}

// ---- the same rotation in an LMC_PAGED_SPLIT cache (lmc_rope_shift_split; k_rope.h: k_rope_split_*) -------------------
// 16-byte accesses: every stride the kernel adds to a plane a whole granule, and what rope_vec_ok asks of the table and
// of rot_dim.  A plane that comes out of a pointer table is looked at by the kernel (k_rope_split_vec goes element by
// element through one that is off a 16-byte boundary).
static bool rope_split_vec(const lmc_kv_layout* kv, const RopeSpec& r) {
  if (!rope_vec_ok(r) || (kv->stride_block & 7) || (kv->stride_head & 7)) return false;
  return kv->plane_ptrs || (!(kv->stride_layer & 7) && ((uintptr_t)kv->base & 15) == 0);
}
static int rope_split_per_head(const lmc_kv_layout* kv, const RopeSpec& r) {
  return rope_split_vec(kv, r) ? r.rot_dim / (r.is_neox ? 16 : 8) : r.rot_dim / 2;
}
// What lmc_rope_shift_split asks: rope_ok's rules for a 16-bit split cache, whose 32-bit offsets follow the decoders' rule.
static bool rope_split_ok(const lmc_kv_layout* kv, int32_t tok_begin, int32_t ntok, const RopeSpec& r) {
  if (!layout_ok(kv, false, true) || kv->paged_kind != LMC_PAGED_SPLIT || lmc_dtype_fp8(kv->dtype) || !decode_dst_ok(kv, 0))
    return false;
  if (ntok < 1 || tok_begin < 0 || (long long)tok_begin + ntok > INT32_MAX || !r.cos_sin || r.table_rows < 1) return false;
  if (r.rot_dim < 2 || (r.rot_dim & 1) || r.rot_dim > kv->head_size) return false;
  if (!r.deltas && (r.delta <= -r.table_rows || r.delta >= r.table_rows)) return false;
  return (long long)ntok * kv->num_heads * rope_split_per_head(kv, r) < (1ll << 31);
}
// lmc_rope_shift_split behind its checks (rope_split_ok); the grid is rope_launch's.
static int rope_split_launch(lmc_ctx* c, const lmc_kv_layout* kv, int32_t tok_begin, int32_t ntok, const RopeSpec& r,
                             uint32_t* job_status, hipStream_t stream) {
  const bool neox = r.is_neox != 0, vec = rope_split_vec(kv, r);
  RopeArgs a;
  memset(&a, 0, sizeof a);
  a.kv = to_addr(kv);
  a.cos_sin = r.cos_sin; a.deltas = r.deltas; a.status = job_status ? job_status : c->status_h;
  a.tok_begin = tok_begin; a.ntok = ntok; a.rot = r.rot_dim; a.table_rows = r.table_rows; a.delta = r.delta; a.neox = neox;
  a.per_head = (u32)rope_split_per_head(kv, r);
  const long long nitems = (long long)ntok * kv->num_heads * a.per_head;  // of one layer (< 2^31: rope_split_ok)
  a.nitems = (u32)nitems;
  HIP_TRY(hipSetDevice(c->device));
  long long blocks = (nitems + 255) / 256;
  const long long cap = std::max(1ll, 64ll * c->num_cus / kv->num_layers);  // grid-stride beyond 64 blocks per CU
  if (blocks > cap) blocks = cap;
  const dim3 grid((unsigned)blocks, (unsigned)kv->num_layers);
  const size_t lds = vec && !r.deltas ? (size_t)r.rot_dim * sizeof(float) : 0;  // the one table row of a uniform delta
  with_kv_dtype16(kv->dtype, [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    if (!vec) hipLaunchKernelGGL((k_rope_split_elem<DT>), grid, dim3(256), 0, stream, a);
    else with_bool(neox, [&](auto nx) { hipLaunchKernelGGL((k_rope_split_vec<DT, decltype(nx)::value>), grid, dim3(256), lds, stream, a); });
  });
  HIP_TRY(hipGetLastError());
  return LMC_OK;
}

// ---- the post-op of a layer range (lmc_range_post): between a range's decode and its event --------------------------
// Layers [l0, l0 + nl) of a layout as a layout of nl layers: the plane table is layer-major (lmc_plane_base), so the
// window is a pointer into it, or the base moved by l0 layer strides.  The rope and copy kernels need nothing else.
static lmc_kv_layout layer_window(const lmc_kv_layout* l, int l0, int nl) {
  lmc_kv_layout w = *l;
  if (w.plane_ptrs) w.plane_ptrs += 2 * l0;
  else w.base = (const u8*)w.base + (long long)l0 * w.stride_layer * (lmc_dtype_fp8(w.dtype) ? 1 : 2);
  w.num_layers = nl;
  return w;
}
static RopeSpec post_rope(const lmc_range_post* p) {
  const RopeSpec r = {p->cos_sin, p->table_rows, p->rot_dim, p->is_neox, p->delta, p->deltas};
  return r;
}
// The whole post-op against lmc_copy_kv's and lmc_rope_shift's rules, before anything of the job is queued.
// A rotation of a split `dst` that names ITSELF as the scatter target: the range's final place is where the decoder put
// it, and the keys are rotated there (lmc_rope_shift_split per range; nothing is copied).  scatter_dst must describe the
// same cache, every field equal, and token i of it be token i of `dst`.
static bool post_in_place(const lmc_kv_layout* dst, const lmc_range_post* p) {
  const lmc_kv_layout* s = p->scatter_dst;
  if (!dst || dst->paged_kind != LMC_PAGED_SPLIT || !p->cos_sin || !s || p->scatter_tok0 != p->tok_begin) return false;
  return s->dtype == dst->dtype && s->num_layers == dst->num_layers && s->num_heads == dst->num_heads &&
         s->head_size == dst->head_size && s->base == dst->base && s->plane_ptrs == dst->plane_ptrs &&
         s->stride_layer == dst->stride_layer && s->stride_kv == dst->stride_kv && s->stride_token == dst->stride_token &&
         s->stride_head == dst->stride_head && s->slot_mapping == dst->slot_mapping && s->block_size == dst->block_size &&
         s->paged_kind == dst->paged_kind && s->stride_block == dst->stride_block;
}
static bool post_ok(const lmc_kv_layout* dst, const lmc_range_post* p) {
  if (!p || (!p->cos_sin && !p->scatter_dst)) return true;
  if (post_in_place(dst, p)) return rope_split_ok(dst, p->tok_begin, p->ntok, post_rope(p));
  if (p->scatter_dst && (p->scatter_dst->paged_kind != LMC_PAGED_SPLIT ||
                         !copy_kv_ok(dst, p->tok_begin, p->ntok, p->scatter_dst, p->scatter_tok0)))
    return false;
  return !p->cos_sin || rope_ok(dst, p->tok_begin, p->ntok, post_rope(p));  // (a split `dst` has no rows to rotate: refused)
}
// A bad position is reported where lmc_rope_shift reports it for the one-shot retrieve: the context's sticky word (the
// job's own word says whether its blobs decoded).
static int range_post(lmc_ctx* c, const lmc_kv_layout* dst, const lmc_range_post* p, int l0, int nl, hipStream_t s) {
  if (!p->cos_sin && !p->scatter_dst) return LMC_OK;
  const lmc_kv_layout rows = layer_window(dst, l0, nl);
  if (post_in_place(dst, p)) return rope_split_launch(c, &rows, p->tok_begin, p->ntok, post_rope(p), nullptr, s);  // (`rows`: the split window)
  if (!p->scatter_dst) return rope_launch(c, &rows, p->tok_begin, p->ntok, post_rope(p), nullptr, s);
  // rotation and scatter: the staged rows are rotated in place, then scattered (a scatter that rotates on the way was built
  // and measured slower than these two launches: profiles/paged_layerwise.md)
  if (p->cos_sin) {
    const int rc = rope_launch(c, &rows, p->tok_begin, p->ntok, post_rope(p), nullptr, s);
    if (rc) return rc;
  }
  const lmc_kv_layout split = layer_window(p->scatter_dst, l0, nl);
  return copy_split(c, &rows, p->tok_begin, p->ntok, &split, p->scatter_tok0, s);
}

extern "C" {

int lmc_copy_kv(lmc_ctx* c, const lmc_kv_layout* src, int32_t tok_begin, int32_t ntok, const lmc_kv_layout* dst,
                int32_t dst_tok0, lmc_stream_t stream) {
  if (!c || !copy_kv_ok(src, tok_begin, ntok, dst, dst_tok0)) return LMC_ERR_INVALID;
  if (src->paged_kind == LMC_PAGED_SPLIT || dst->paged_kind == LMC_PAGED_SPLIT)
    return copy_split(c, src, tok_begin, ntok, dst, dst_tok0, (hipStream_t)stream);
  const bool vec = layout_ok(src) && layout_ok(dst);  // else one element per thread (any strides, any head_size)
  CopyArgs a;
  memset(&a, 0, sizeof a);
  a.src = to_addr(src); a.dst = to_addr(dst);
  a.tok_begin = tok_begin; a.ntok = ntok; a.dst_tok0 = dst_tok0;
  a.P = 2 * src->num_layers; a.C = src->num_heads * src->head_size;
  a.nvec = (long long)a.P * ntok * (vec ? a.C / 8 : a.C);
  HIP_TRY(hipSetDevice(c->device));
  long long blocks = (a.nvec + 255) / 256;
  if (blocks > 256LL * 64) blocks = 256LL * 64;  // grid-stride beyond 64 blocks per CU
  if (lmc_dtype_fp8(src->dtype)) {  // 1-byte elements
    if (vec) hipLaunchKernelGGL(k_copy_kv_b8, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(k_copy_kv_elem_b8, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
  } else if (vec) hipLaunchKernelGGL(k_copy_kv, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(k_copy_kv_elem, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return LMC_OK;
}

int lmc_rope_shift(lmc_ctx* c, const lmc_kv_layout* kv, int32_t tok_begin, int32_t ntok, const float* cos_sin,
                   int32_t table_rows, int32_t rot_dim, int32_t is_neox, int32_t delta, const int32_t* deltas,
                   uint32_t* job_status, lmc_stream_t stream) {
  const RopeSpec r = {cos_sin, table_rows, rot_dim, is_neox, delta, deltas};
  if (!c || !rope_ok(kv, tok_begin, ntok, r)) return LMC_ERR_INVALID;
  return rope_launch(c, kv, tok_begin, ntok, r, job_status, (hipStream_t)stream);
}

int lmc_rope_shift_split(lmc_ctx* c, const lmc_kv_layout* kv, int32_t tok_begin, int32_t ntok, const float* cos_sin,
                         int32_t table_rows, int32_t rot_dim, int32_t is_neox, int32_t delta, const int32_t* deltas,
                         uint32_t* job_status, lmc_stream_t stream) {
  const RopeSpec r = {cos_sin, table_rows, rot_dim, is_neox, delta, deltas};
  if (!c || !rope_split_ok(kv, tok_begin, ntok, r)) return LMC_ERR_INVALID;
  return rope_split_launch(c, kv, tok_begin, ntok, r, job_status, (hipStream_t)stream);
}

}  // extern "C"

// ---- CacheBlend token selection (k_blend.h) -------------------------------------------------------------------------
// What lmc_kv_deviation asks of its two layouts and its range: lmc_copy_kv's rules with the layer count free, 16-bit
// elements only (every refusal LMC_ERR_INVALID, nothing launched).
static bool deviation_ok(const lmc_kv_layout* a, int32_t a_layer, int32_t a_tok0, const lmc_kv_layout* b, int32_t b_layer,
                         int32_t b_tok0, int32_t ntok, const float* dev_k, const float* dev_v) {
  if (!layout_ok(a, false, true) || !layout_ok(b, false, true) || ntok < 1 || a_tok0 < 0 || b_tok0 < 0) return false;
  if (a->num_heads != b->num_heads || a->head_size != b->head_size || a->dtype != b->dtype || lmc_dtype_fp8(a->dtype)) return false;
  if (a->paged_kind == LMC_PAGED_SPLIT && b->paged_kind == LMC_PAGED_SPLIT) return false;  // one side is rows
  if (a_layer < 0 || a_layer >= a->num_layers || b_layer < 0 || b_layer >= b->num_layers) return false;
  if ((long long)a_tok0 + ntok > INT32_MAX || (long long)b_tok0 + ntok > INT32_MAX) return false;
  return dev_k || dev_v;
}
// One side of the comparison: its layer's two planes, and whether its strides let it be read 16 bytes at a time -- rows:
// lmc_copy_kv's `vec` rule; split: every stride a whole granule (the kernel looks at the plane base itself).
static DevSide deviation_side(const lmc_kv_layout* l, int32_t layer, int32_t tok0) {
  DevSide s;
  memset(&s, 0, sizeof s);
  s.kv = to_addr(l);
  s.tok0 = tok0; s.plane_k = layer; s.plane_v = l->num_layers + layer;
  s.split = l->paged_kind == LMC_PAGED_SPLIT;
  auto mult = [](int64_t v) { return v % 8 == 0; };
  s.vec = s.split ? mult(l->stride_block) && mult(l->stride_head) && (l->plane_ptrs || (mult(l->stride_layer) && mult(l->stride_kv)))
                  : layout_ok(l);
  return s;
}

extern "C" {

int lmc_kv_deviation(lmc_ctx* c, const lmc_kv_layout* a, int32_t a_layer, int32_t a_tok0, const lmc_kv_layout* b,
                     int32_t b_layer, int32_t b_tok0, int32_t ntok, float* dev_k, float* dev_v, lmc_stream_t stream) {
  if (!c || !deviation_ok(a, a_layer, a_tok0, b, b_layer, b_tok0, ntok, dev_k, dev_v)) return LMC_ERR_INVALID;
  DeviationArgs g;
  memset(&g, 0, sizeof g);
  // the kernel's tile form wants the split side second: the squared difference does not care
  const bool swap = a->paged_kind == LMC_PAGED_SPLIT;
  g.a = swap ? deviation_side(b, b_layer, b_tok0) : deviation_side(a, a_layer, a_tok0);
  g.b = swap ? deviation_side(a, a_layer, a_tok0) : deviation_side(b, b_layer, b_tok0);
  g.ntok = ntok; g.C = a->num_heads * a->head_size;
  g.lpt = 1;
  while (g.lpt < g.C / 8 && g.lpt < 64) g.lpt <<= 1;
  g.ntiles = (int)(((long long)ntok + 14) / 8);  // the first tile may begin 7 positions in front of the range
  g.out[0] = dev_k; g.out[1] = dev_v;
  if (dev_k) g.plane_kv[g.nplanes++] = 0;
  if (dev_v) g.plane_kv[g.nplanes++] = 1;
  HIP_TRY(hipSetDevice(c->device));
  // a wave of the group form takes 64 / lpt tokens, a wave of the tile form a tile; grid-stride beyond 32 workgroups per CU
  auto launch = [&](bool tile, long long items) {
    long long blocks = (items + BLEND_WAVES - 1) / BLEND_WAVES;
    if (blocks > 32LL * c->num_cus) blocks = 32LL * c->num_cus;
    with_kv_dtype16(a->dtype, [&](auto dt) {
      with_bool(tile, [&](auto tl) {
        hipLaunchKernelGGL((k_kv_deviation<decltype(dt)::value, decltype(tl)::value>), dim3((unsigned)blocks, (unsigned)g.nplanes),
                           dim3(64 * BLEND_WAVES), 0, (hipStream_t)stream, g);
      });
    });
  };
  const long long tpw = 64 / g.lpt, groups = (ntok + tpw - 1) / tpw;
  if (!g.b.split) launch(false, groups);  // both planes in one launch
  else {  // a split side: the K plane in the group form, the V plane in the tile form, a launch each
    const int want_k = dev_k != nullptr, want_v = dev_v != nullptr;
    g.nplanes = 1;
    if (want_k) { g.plane_kv[0] = 0; launch(false, groups); }
    if (want_v) { g.plane_kv[0] = 1; launch(true, g.ntiles); }
  }
  HIP_TRY(hipGetLastError());
  return LMC_OK;
}

int lmc_select_topk(lmc_ctx* c, const float* dev, int32_t n, int32_t k, int32_t* idx_out, lmc_stream_t stream) {
  if (!c || !dev || n < 1 || n > (1 << 20) || k < 0 || (k > 0 && !idx_out)) return LMC_ERR_INVALID;
  if (k == 0) return LMC_OK;  // nothing to write
  TopkArgs t;
  t.dev = dev; t.idx_out = idx_out; t.n = (u32)n; t.kk = (u32)(k < n ? k : n);
  HIP_TRY(hipSetDevice(c->device));
  hipLaunchKernelGGL(k_select_topk, dim3(1), dim3(TOPK_THREADS), 0, (hipStream_t)stream, t);
  HIP_TRY(hipGetLastError());
  return LMC_OK;
}

// ---- host DRAM offload plumbing ---------------------------------------------
int lmc_pinned_alloc(size_t bytes, void** out_h) {
  if (!out_h || bytes == 0) return LMC_ERR_INVALID;
  hipError_t e = hipHostMalloc(out_h, bytes, hipHostMallocMapped | hipHostMallocPortable);
  if (e != hipSuccess) { g_last_hip = (int)e; return e == hipErrorOutOfMemory ? LMC_ERR_NOMEM : LMC_ERR_HIP; }
  return LMC_OK;
}
int lmc_pinned_free(void* p) { if (p) HIP_TRY(hipHostFree(p)); return LMC_OK; }

int lmc_memcpy_async(void* dst, const void* src, size_t bytes, int kind, lmc_stream_t stream) {
  if (!dst || !src) return LMC_ERR_INVALID;
  if (bytes == 0) return LMC_OK;
  hipMemcpyKind k = kind == 0 ? hipMemcpyDeviceToHost : kind == 1 ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
  if (kind < 0 || kind > 2) return LMC_ERR_INVALID;
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, k, (hipStream_t)stream));
  return LMC_OK;
}

int lmc_stream_create(lmc_stream_t* out) {
  if (!out) return LMC_ERR_INVALID;
  hipStream_t s;
  HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  *out = (lmc_stream_t)s;
  return LMC_OK;
}
int lmc_stream_destroy(lmc_stream_t s) { HIP_TRY(hipStreamDestroy((hipStream_t)s)); return LMC_OK; }
int lmc_stream_synchronize(lmc_stream_t s) { HIP_TRY(hipStreamSynchronize((hipStream_t)s)); return LMC_OK; }
int lmc_stream_wait_event(lmc_stream_t s, lmc_event_t e) { HIP_TRY(hipStreamWaitEvent((hipStream_t)s, (hipEvent_t)e, 0)); return LMC_OK; }
int lmc_event_create(lmc_event_t* out, int timing) {
  if (!out) return LMC_ERR_INVALID;
  hipEvent_t e;
  HIP_TRY(hipEventCreateWithFlags(&e, timing ? hipEventDefault : hipEventDisableTiming));
  *out = (lmc_event_t)e;
  return LMC_OK;
}
int lmc_event_destroy(lmc_event_t e) { HIP_TRY(hipEventDestroy((hipEvent_t)e)); return LMC_OK; }
int lmc_event_record(lmc_event_t e, lmc_stream_t s) { HIP_TRY(hipEventRecord((hipEvent_t)e, (hipStream_t)s)); return LMC_OK; }
int lmc_event_synchronize(lmc_event_t e) { HIP_TRY(hipEventSynchronize((hipEvent_t)e)); return LMC_OK; }
int lmc_event_query(lmc_event_t e) {
  hipError_t r = hipEventQuery((hipEvent_t)e);
  if (r == hipSuccess) return 1;
  if (r == hipErrorNotReady) return 0;
  g_last_hip = (int)r;
  return LMC_ERR_HIP;
}
int lmc_event_elapsed_ms(lmc_event_t a, lmc_event_t b, float* ms) {
  if (!ms) return LMC_ERR_INVALID;
  HIP_TRY(hipEventElapsedTime(ms, (hipEvent_t)a, (hipEvent_t)b));
  return LMC_OK;
}

// ---- store / load legs ------------------------------------------------------------------------------------
int lmc_blob_info(const void* blob_h, size_t nbytes, lmc_blob_header* out);
static int legs_init(lmc_ctx* c) {  // caller holds c->mu
  if (!c->copy_stream) HIP_TRY(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
  if (!c->store_free) HIP_TRY(hipEventCreateWithFlags(&c->store_free, hipEventDisableTiming));
  if (!c->load_free) HIP_TRY(hipEventCreateWithFlags(&c->load_free, hipEventDisableTiming));
  return LMC_OK;
}
static int next_event(lmc_ctx* c, hipEvent_t* out) {  // caller holds c->mu; 64 events in rotation: a call uses <= 34
  hipEvent_t& e = c->evpool[c->evnext];
  c->evnext = (c->evnext + 1) % 64;
  if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  *out = e;
  return LMC_OK;
}

// caller holds c->mu: `later` runs behind what `first` has queued so far (an event from the rotation)
static int stream_follows(lmc_ctx* c, hipStream_t later, hipStream_t first) {
  int rc;
  hipEvent_t ev;
  if ((rc = next_event(c, &ev))) return rc;
  HIP_TRY(hipEventRecord(ev, first));
  HIP_TRY(hipStreamWaitEvent(later, ev, 0));
  return LMC_OK;
}
// Takes c->mu.  The store arena of at least arena_bytes (and the pack table of table_bytes) for a job on `s`: the host
// waits for the previous job's copies only when a buffer must grow, the stream always does.
static int store_acquire(lmc_ctx* c, hipStream_t s, size_t arena_bytes, size_t table_bytes) {
  int rc;
  std::lock_guard<std::mutex> lk(c->mu);
  if ((rc = legs_init(c))) return rc;
  if (c->store_arena.bytes < arena_bytes || c->pack_table.bytes < table_bytes) {
    if (c->store_used) HIP_TRY(hipEventSynchronize(c->store_free));  // growing frees the buffers: this call only
    if ((rc = c->store_arena.grow(arena_bytes)) || (rc = c->pack_table.grow(table_bytes))) return rc;
  }
  if (c->store_used) HIP_TRY(hipStreamWaitEvent(s, c->store_free, 0));  // the previous job's copies have read the arena
  return LMC_OK;
}
// caller holds c->mu: the next job may take the arena and the table behind what `last` has queued so far
static int store_release(lmc_ctx* c, hipStream_t last) {
  HIP_TRY(hipEventRecord(c->store_free, last));
  c->store_used = true;
  return LMC_OK;
}
// The load side, caller holds c->mu.  The load staging (c->load_slots) of at least `bytes` for a job that copies into it
// on `queues` (1 or 2) copy queues -> cs[]: the host waits for the previous load only when the staging must grow, the
// queues always do, before their first copy (its decodes have read the staging).
static int load_acquire(lmc_ctx* c, size_t bytes, int queues, hipStream_t cs[2]) {
  int rc;
  if ((rc = legs_init(c))) return rc;
  if (queues > 1 && !c->copy_stream2) HIP_TRY(hipStreamCreateWithFlags(&c->copy_stream2, hipStreamNonBlocking));
  if (c->load_slots.bytes < bytes) {
    if (c->load_used) HIP_TRY(hipEventSynchronize(c->load_free));
    if ((rc = c->load_slots.grow(bytes))) return rc;
  }
  cs[0] = c->copy_stream; cs[1] = c->copy_stream2;
  for (int q = 0; q < queues && c->load_used; q++) HIP_TRY(hipStreamWaitEvent(cs[q], c->load_free, 0));
  return LMC_OK;
}
// ... and behind the job's last reader of the staging, on `s`
static int load_release(lmc_ctx* c, hipStream_t s) {
  HIP_TRY(hipEventRecord(c->load_free, s));
  c->load_used = true;
  return LMC_OK;
}

int lmc_store_chunks(lmc_ctx* c, const lmc_kv_layout* src, int32_t tok_begin, int32_t tok_end, int32_t chunk_tokens,
                     const int32_t* bins_h, void* host_arena_h, uint64_t host_cap, uint64_t* offsets_h,
                     uint32_t* sizes_h, uint32_t* job_status, lmc_stream_t stream) {
  int nchunks;
  if (!encode_job_ok(c, src, tok_begin, tok_end, chunk_tokens, &nchunks, true) || !host_arena_h || ((uintptr_t)host_arena_h & 15) ||
      !offsets_h || !sizes_h)
    return LMC_ERR_INVALID;
  const uint64_t stride = blob_stride(src->num_layers, chunk_tokens, src->num_heads, src->head_size);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)stream;
  int rc;
  if ((rc = store_acquire(c, s, (size_t)nchunks * stride, 0))) return rc;
  // a long job leaves in parts: the copy of part k runs on the context's copy stream beside the encode of part k + 1
  const int nparts = nchunks >= 16 ? 4 : 1, per = (nchunks + nparts - 1) / nparts;
  uint32_t* st = job_status ? job_status : c->status_h;
  for (int c0 = 0; c0 < nchunks; c0 += per) {
    const int c1 = c0 + per < nchunks ? c0 + per : nchunks;
    const int t1 = tok_begin + c1 * chunk_tokens < tok_end ? tok_begin + c1 * chunk_tokens : tok_end;
    if ((rc = encode_chunks_parts(c, src, tok_begin + c0 * chunk_tokens, t1, chunk_tokens, bins_h, c->store_arena.p + (size_t)c0 * stride,
                                  stride, sizes_h + c0, job_status, stream, 1, nullptr, true)))
      return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    if ((rc = stream_follows(c, c->copy_stream, s))) return rc;
    OffloadArgs oa;
    memset(&oa, 0, sizeof oa);
    oa.blobs = c->store_arena.p; oa.stride = (long long)stride; oa.sizes_d = sizes_h; oa.nchunks = nchunks; oa.chunk0 = c0;
    oa.host = (u8*)host_arena_h; oa.cap = host_cap; oa.offsets_h = (unsigned long long*)offsets_h; oa.sizes_h = sizes_h;
    oa.status = st;
    hipLaunchKernelGGL(k_offload, dim3(8, (unsigned)(c1 - c0)), dim3(256), 0, c->copy_stream, oa);
    HIP_TRY(hipGetLastError());
  }
  std::lock_guard<std::mutex> lk(c->mu);
  if ((rc = store_release(c, c->copy_stream))) return rc;
  HIP_TRY(hipStreamWaitEvent(s, c->store_free, 0));  // the caller's stream is done when the blobs have landed
  return LMC_OK;
}

// Host-side view of a blob that lies in pinned host memory: checked header + section offsets (lmc_blob_info's
// checks, without the copy-out).
static bool host_blob_ok(const u8* b, uint32_t size, int L, int H, int D, uint32_t max_bytes, lmc_blob_header* h) {
  if (size < sizeof(lmc_blob_header) || ((uintptr_t)b & 15)) return false;
  memcpy(h, b, sizeof *h);
  if (lmc_blob_info(b, size, h) != LMC_OK) return false;
  return h->num_layers == (uint32_t)L && h->num_heads == (uint32_t)H && h->head_size == (uint32_t)D &&
         h->total_bytes == size && h->total_bytes <= max_bytes;
}

int lmc_load_chunks(lmc_ctx* c, const void* const* host_blob_ptrs_h, const uint32_t* sizes_h, int32_t nchunks,
                    const lmc_kv_layout* dst, int32_t dst_tok0, int32_t chunk_tokens, int32_t layers_per_range,
                    lmc_event_t* range_events, uint32_t* job_status, lmc_stream_t stream) {
  if (!host_blob_ptrs_h || !sizes_h || layers_per_range < 0) return LMC_ERR_INVALID;
  DecodeArgs da;
  int rc = decode_common(c, nchunks, dst, dst_tok0, chunk_tokens, job_status, da, true);
  if (rc) return rc;
  const int L = dst->num_layers, H = dst->num_heads, D = dst->head_size;
  const uint64_t stride = blob_stride(L, chunk_tokens, H, D);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)stream;
  const int step = layers_per_range > 0 && layers_per_range < L ? layers_per_range : L;
  std::lock_guard<std::mutex> lk(c->mu);
  hipStream_t cs[2];  // two DMA queues (tools/probes/d2h_streams.py)
  if ((rc = load_acquire(c, (size_t)nchunks * stride, 2, cs))) return rc;
  // The blobs lie in pinned HOST memory: their headers are checked right here, by the CPU (a blob that does not check
  // out fails the call before anything is queued), and every blob travels as ONE hipMemcpyAsync, alternating between
  // two DMA queues.  Layer-range-major copies (the K run and the V run of every chunk, per range) were built first and
  // measured: 576 copies of ~0.9 MB for four ranges cost 14.0 ms per 16 k context against 9.8 ms for these 64 whole
  // blobs (~5 us of submission per copy, and the DMA engines lose rate on short transfers) -- more than the overlap
  // of the first ranges' decode with the later ranges' transfer can give back (<= 0.75 ms: the decode of a 16 k
  // context is 1.0 ms in all).  So the transfer stays chunk-major and the ranges are separate decode launches behind
  // it: range r is ready 9.8 ms + (r + 1) x 1.0 ms / ranges after the call, the model can start on layer 0 while the
  // later ranges still decode, and the whole context is there after 10.8 ms.
  for (int i = 0; i < nchunks; i++) {
    lmc_blob_header h;
    if (!host_blob_ok((const u8*)host_blob_ptrs_h[i], sizes_h[i], L, H, D, (uint32_t)(stride > 0xffffffffull ? 0xffffffffu : stride), &h))
      return LMC_ERR_INVALID;
  }
  for (int i = 0; i < nchunks; i++)
    HIP_TRY(hipMemcpyAsync(c->load_slots.p + (size_t)i * stride, host_blob_ptrs_h[i], (sizes_h[i] + 15u) & ~15u,
                           hipMemcpyHostToDevice, cs[i & 1]));
  for (int q = 0; q < 2; q++)  // the decodes wait for both queues
    if ((rc = stream_follows(c, s, cs[q]))) return rc;
  da.blobs = c->load_slots.p; da.blob_stride = (long long)stride;
  int r = 0;
  for (int l0 = 0; l0 < L; l0 += step, r++) {
    const int n = l0 + step <= L ? step : L - l0;
    if ((rc = decode_range_locked(da, dst, l0, n, s, range_events ? range_events[r] : nullptr))) return rc;
  }
  return load_release(c, s);
}

// ---- packs (lmc_format.h): the layer-major form of the pinned host tier ---------------------------------------------
// lmc_store_pack and lmc_store_pack_parts.  nparts == 0: the pack kernels run on the context's copy stream behind the
// whole encode (pack_h may be mapped host memory: their PCIe writes then stall nobody's encode); nparts >= 1: the
// encode goes out in plane ranges and each range is packed on `stream` right behind the launch that coded it.
static int store_pack_impl(lmc_ctx* c, const lmc_kv_layout* src, int32_t tok_begin, int32_t tok_end, int32_t chunk_tokens,
                           const int32_t* bins_h, void* pack_h, uint64_t pack_cap, uint32_t* sizes_h, int32_t nparts,
                           uint64_t* part_info_h, const lmc_event_t* part_events, uint32_t* job_status, lmc_stream_t stream) {
  int nchunks;
  if (!encode_job_ok(c, src, tok_begin, tok_end, chunk_tokens, &nchunks, true) || !pack_h || ((uintptr_t)pack_h & 15) || !sizes_h ||
      nparts < 0 || nparts > 16 || (nparts > 0 && !part_info_h))
    return LMC_ERR_INVALID;
  const int L = src->num_layers, P = 2 * L;
  BinsArg bins;  // (checked here, before the arena is taken; the encode makes its own copy)
  if ((long long)P * nchunks > (1ll << 22) || !bins_ok(bins_h, P, &bins)) return LMC_ERR_INVALID;
  PackArgs pa;
  memset(&pa, 0, sizeof pa);
  lmc_pack_layout((uint32_t)nchunks, (uint32_t)L, (uint32_t)chunk_tokens, (uint32_t)src->num_heads, (uint32_t)src->head_size, &pa.hdr);
  pa.hdr.ntokens = (uint32_t)(tok_end - tok_begin);
  if (pa.hdr.off_streams > pack_cap) return LMC_ERR_INVALID;
  const uint64_t stride = blob_stride(L, chunk_tokens, src->num_heads, src->head_size);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)stream;
  int rc;
  const size_t table_bytes = 8 * ((size_t)P * nchunks + 2);  // the table, and the running total of the parts
  if ((rc = store_acquire(c, s, (size_t)nchunks * stride, table_bytes))) return rc;
  pa.blobs = c->store_arena.p; pa.stride = (long long)stride; pa.sizes_d = sizes_h;
  pa.n = nchunks; pa.L = L; pa.G = (int)pa.hdr.ngroups;
  pa.host = (u8*)pack_h; pa.cap = pack_cap; pa.table_d = c->pack_table.p;
  pa.status = job_status ? job_status : c->status_h;
  const auto pack_range = [](const PackArgs& q, hipStream_t on) -> int {  // planes [q.p_begin, q.p_end) of the arena's blobs
    hipLaunchKernelGGL(k_pack_scan<false>, dim3(1), dim3(256), 0, on, q);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_pack_copy<false>, dim3(64), dim3(256), 0, on, q);  // PCIe-bound: 64 workgroups fill the link
    HIP_TRY(hipGetLastError());
    return LMC_OK;
  };
  if (nparts == 0) {
    // the whole job is encoded (1 ms per 16 k tokens) before the first byte leaves: the pack kernels on the copy stream
    if ((rc = encode_chunks_parts(c, src, tok_begin, tok_end, chunk_tokens, bins_h, c->store_arena.p, stride, sizes_h, job_status, stream,
                                  1, nullptr, true)))
      return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    if ((rc = stream_follows(c, c->copy_stream, s))) return rc;
    pa.p_begin = 0; pa.p_end = P; pa.last = 1; pa.part_h = nullptr;
    if ((rc = pack_range(pa, c->copy_stream))) return rc;
    if ((rc = store_release(c, c->copy_stream))) return rc;
    HIP_TRY(hipStreamWaitEvent(s, c->store_free, 0));  // the caller's stream is done when the pack has landed
    return LMC_OK;
  }
  // ---- in parts: plane range r is packed on `stream` behind the launch that coded it.  A plane's end is the `beg` its
  // successor's first stream writes, so a part that is not the last packs the planes coded so far BUT the newest one,
  // which rides with the next part (1 / 64 of the data at Llama-3-8B's 64 planes).
  for (int r = 0; r < nparts; r++) part_info_h[2 * r] = part_info_h[2 * r + 1] = 0;  // (pinned host words: plain stores)
  int packed = 0, parts_out = 0;
  const AfterPart after = [&](int r, int coded, bool last) -> int {
    (void)r;
    const int upto = last ? P : coded - 1;
    if (upto > packed || last) {
      PackArgs q = pa;
      q.p_begin = packed; q.p_end = upto; q.last = last ? 1 : 0;
      q.part_h = (unsigned long long*)(part_info_h + 2 * parts_out);
      const int prc = pack_range(q, s);
      if (prc) return prc;
      packed = upto;
    }
    if (part_events && part_events[parts_out]) HIP_TRY(hipEventRecord((hipEvent_t)part_events[parts_out], s));
    parts_out++;
    return LMC_OK;
  };
  if ((rc = encode_chunks_parts(c, src, tok_begin, tok_end, chunk_tokens, bins_h, c->store_arena.p, stride, sizes_h, job_status,
                                stream, nparts, &after, true)))
    return rc;
  std::lock_guard<std::mutex> lk(c->mu);
  for (; parts_out < nparts; parts_out++)  // a job that could not be split: the unused parts' events fire behind the only one
    if (part_events && part_events[parts_out]) HIP_TRY(hipEventRecord((hipEvent_t)part_events[parts_out], s));
  return store_release(c, s);
}

int lmc_store_pack(lmc_ctx* c, const lmc_kv_layout* src, int32_t tok_begin, int32_t tok_end, int32_t chunk_tokens,
                   const int32_t* bins_h, void* pack_h, uint64_t pack_cap, uint32_t* sizes_h, uint32_t* job_status,
                   lmc_stream_t stream) {
  return store_pack_impl(c, src, tok_begin, tok_end, chunk_tokens, bins_h, pack_h, pack_cap, sizes_h, 0, nullptr, nullptr,
                         job_status, stream);
}

int lmc_store_pack_parts(lmc_ctx* c, const lmc_kv_layout* src, int32_t tok_begin, int32_t tok_end, int32_t chunk_tokens,
                         const int32_t* bins_h, void* pack_d, uint64_t pack_cap, uint32_t* sizes_h, int32_t nparts,
                         uint64_t* part_info_h, const lmc_event_t* part_events, uint32_t* job_status, lmc_stream_t stream) {
  if (nparts < 1) return LMC_ERR_INVALID;
  return store_pack_impl(c, src, tok_begin, tok_end, chunk_tokens, bins_h, pack_d, pack_cap, sizes_h, nparts, part_info_h,
                         part_events, job_status, stream);
}

// Host-side check of a pack that lies in (pinned) host memory.
static bool pack_ok(const u8* b, uint64_t nbytes, lmc_pack_header* h) {
  if (!b || ((uintptr_t)b & 15) || nbytes < LMC_PACK_HEADER_BYTES) return false;
  memcpy(h, b, sizeof *h);
  if (h->magic != LMC_PACK_MAGIC || h->version != LMC_PACK_VERSION || h->header_bytes != LMC_PACK_HEADER_BYTES) return false;
  if (h->nchunks < 1 || h->nchunks > 65535 || h->num_layers < 1 || h->num_layers > LMC_MAX_PLANES / 2 || h->num_heads == 0 ||
      h->head_size == 0 || h->chunk_tokens < 1 || h->chunk_tokens > 65535 || (h->static_stride & 15) ||
      h->static_stride < sizeof(lmc_blob_header))
    return false;
  const uint64_t N = 2ull * h->num_layers * h->nchunks;
  if (h->off_table != LMC_PACK_HEADER_BYTES || h->off_static != lmc_r16_64(h->off_table + 8 * (N + 1)) ||
      h->off_streams != h->off_static + (uint64_t)h->nchunks * h->static_stride || h->total_bytes > nbytes ||
      h->total_bytes < h->off_streams)
    return false;
  const uint64_t* t = (const uint64_t*)(b + h->off_table);
  if (t[0] != 0 || t[N] != h->total_bytes - h->off_streams) return false;
  for (uint64_t i = 0; i < N; i++)
    if (t[i + 1] < t[i] || (t[i] & 15)) return false;
  return true;
}

int lmc_pack_info(const void* pack_h, uint64_t nbytes, lmc_pack_header* out) {
  lmc_pack_header h;
  if (!out || !pack_ok((const u8*)pack_h, nbytes, &h)) return LMC_ERR_INVALID;
  *out = h;
  return LMC_OK;
}

// Chunk `chunk` of a checked pack as the blob it was packed from: the checks of its static slot (the head of the blob:
// its header says how long the head and the whole blob are) and the walk over its segments, which must add up to the
// blob.  blob_out, if given, receives the blob (`cap` bytes of room).  Returns the blob's size, or 0: the pack holds no
// such blob (or it does not fit).
static uint32_t pack_chunk_walk(const u8* b, const lmc_pack_header& h, uint32_t chunk, u8* blob_out, uint64_t cap) {
  const u8* st = b + h.off_static + (uint64_t)chunk * h.static_stride;
  lmc_blob_header bh;
  memcpy(&bh, st, sizeof bh);
  if (bh.magic != LMC_BLOB_MAGIC || bh.off_streams > h.static_stride || bh.off_streams < sizeof bh ||
      bh.total_bytes != bh.off_streams + bh.stream_bytes || (blob_out && bh.total_bytes > cap) || bh.num_layers != h.num_layers)
    return 0;
  if (blob_out) memcpy(blob_out, st, bh.off_streams);
  const uint64_t* t = (const uint64_t*)(b + h.off_table);
  uint64_t at = bh.off_streams;
  for (uint32_t p = 0; p < 2 * h.num_layers; p++) {  // plane order of the blob and of the pack: K planes of every layer, then V planes
    const uint64_t i = (uint64_t)p * h.nchunks + chunk;
    const uint64_t len = t[i + 1] - t[i];
    if (at + len > bh.total_bytes) return 0;
    if (blob_out) memcpy(blob_out + at, b + h.off_streams + t[i], len);
    at += len;
  }
  return at == bh.total_bytes ? bh.total_bytes : 0;
}

int lmc_pack_extract(const void* pack_h, uint64_t nbytes, int32_t chunk, void* blob_out, uint64_t cap, uint32_t* size_out) {
  lmc_pack_header h;
  const u8* b = (const u8*)pack_h;
  if (!pack_ok(b, nbytes, &h) || chunk < 0 || (uint32_t)chunk >= h.nchunks || !blob_out || !size_out) return LMC_ERR_INVALID;
  const uint32_t size = pack_chunk_walk(b, h, (uint32_t)chunk, (u8*)blob_out, cap);
  if (!size) return LMC_ERR_INVALID;
  *size_out = size;
  return LMC_OK;
}

int lmc_load_pack_post(lmc_ctx* c, const void* pack_h, uint64_t pack_bytes, int32_t chunk_begin, int32_t nchunks,
                       const lmc_kv_layout* dst, int32_t dst_tok0, int32_t layers_per_range, lmc_event_t* range_events,
                       uint32_t* job_status, lmc_stream_t stream, const lmc_range_post* post) {
  lmc_pack_header h;
  if (layers_per_range < 0 || nchunks < 0 || chunk_begin < 0 || !pack_ok((const u8*)pack_h, pack_bytes, &h) ||
      (uint32_t)chunk_begin >= h.nchunks || (uint32_t)nchunks > h.nchunks - (uint32_t)chunk_begin)
    return LMC_ERR_INVALID;
  const int n = (int)h.nchunks, c0 = chunk_begin, m = nchunks ? nchunks : n - c0;  // chunks c0 .. c0 + m of the pack
  DecodeArgs da;
  int rc = decode_common(c, m, dst, dst_tok0, (long long)h.chunk_tokens, job_status, da, true);
  if (rc) return rc;
  const int L = dst->num_layers, H = dst->num_heads, D = dst->head_size;
  if ((uint32_t)L != h.num_layers || (uint32_t)H != h.num_heads || (uint32_t)D != h.head_size || !post_ok(dst, post))
    return LMC_ERR_INVALID;
  const u8* b = (const u8*)pack_h;
  const uint64_t* t = (const uint64_t*)(b + h.off_table);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)stream;
  const int step = layers_per_range > 0 && layers_per_range < L ? layers_per_range : L;
  std::lock_guard<std::mutex> lk(c->mu);
  hipStream_t queues[2];
  if ((rc = load_acquire(c, (size_t)h.total_bytes, 1, queues))) return rc;
  hipStream_t cs = queues[0];  // ONE queue: the ranges must arrive in layer order
  // the device copy keeps the pack's offsets: table, static slots and segments land where they lie in the pack
  u8* dev = c->load_slots.p;
  HIP_TRY(hipMemcpyAsync(dev + h.off_table, b + h.off_table, 8 * (2 * (size_t)L * n + 1), hipMemcpyHostToDevice, cs));
  HIP_TRY(hipMemcpyAsync(dev + h.off_static + (size_t)c0 * h.static_stride, b + h.off_static + (size_t)c0 * h.static_stride,
                         (size_t)m * h.static_stride, hipMemcpyHostToDevice, cs));
  da.blobs = dev + h.off_static + (size_t)c0 * h.static_stride; da.blob_stride = (long long)h.static_stride;  // (the static slots)
  da.seg_off = (const unsigned long long*)(dev + h.off_table) + c0; da.seg_streams = dev + h.off_streams; da.seg_n = n;
  int r = 0;
  for (int l0 = 0; l0 < L; l0 += step, r++) {
    const int nl = l0 + step <= L ? step : L - l0;
    // the streams of layers l0 .. l0 + nl: one contiguous region when the whole pack is wanted, else one run of the
    // m chunks per (layer, kv)
    // (pack v3, plane order: the K planes of the range are one contiguous region, its V planes another)
    for (int kv = 0; kv < 2; kv++) {
      const int p0 = kv * L + l0;
      if (m == n) {
        const uint64_t lo = t[(uint64_t)p0 * n], hi = t[(uint64_t)(p0 + nl) * n];
        if (hi > lo) HIP_TRY(hipMemcpyAsync(dev + h.off_streams + lo, b + h.off_streams + lo, hi - lo, hipMemcpyHostToDevice, cs));
      } else {
        for (int p = p0; p < p0 + nl; p++) {
          const uint64_t lo = t[(uint64_t)p * n + c0], hi = t[(uint64_t)p * n + c0 + m];
          if (hi > lo) HIP_TRY(hipMemcpyAsync(dev + h.off_streams + lo, b + h.off_streams + lo, hi - lo, hipMemcpyHostToDevice, cs));
        }
      }
    }
    if ((rc = stream_follows(c, s, cs))) return rc;
    if ((rc = decode_range_locked(da, dst, l0, nl, s, range_events ? range_events[r] : nullptr, c, post))) return rc;
  }
  return load_release(c, s);
}

int lmc_load_pack(lmc_ctx* c, const void* pack_h, uint64_t pack_bytes, int32_t chunk_begin, int32_t nchunks,
                  const lmc_kv_layout* dst, int32_t dst_tok0, int32_t layers_per_range, lmc_event_t* range_events,
                  uint32_t* job_status, lmc_stream_t stream) {
  return lmc_load_pack_post(c, pack_h, pack_bytes, chunk_begin, nchunks, dst, dst_tok0, layers_per_range, range_events, job_status,
                            stream, nullptr);
}

// ---- bounded tiers: blobs of earlier stores -> a pack (demotion), a pack -> blobs (promotion) ------------------------
int lmc_pack_blobs(lmc_ctx* c, const void* const* blob_ptrs, const uint32_t* blob_bytes, int32_t nchunks, int32_t L, int32_t H,
                   int32_t D, int32_t chunk_tokens, uint32_t ntokens, void* pack_d, uint64_t pack_cap, uint32_t* job_status,
                   lmc_stream_t stream) {
  // (P * nchunks: lmc_store_pack's bound on a pack's table)
  if (!c || !blob_ptrs || !blob_bytes || !pack_d || ((uintptr_t)pack_d & 15) || !chunk_geometry_ok(nchunks, L, H, D, chunk_tokens, ntokens) ||
      2ll * L * nchunks > (1ll << 22))
    return LMC_ERR_INVALID;
  const int P = 2 * L;
  PackArgs pa;
  memset(&pa, 0, sizeof pa);
  lmc_pack_layout((uint32_t)nchunks, (uint32_t)L, (uint32_t)chunk_tokens, (uint32_t)H, (uint32_t)D, &pa.hdr);
  pa.hdr.ntokens = ntokens;
  if (pa.hdr.off_streams > pack_cap) return LMC_ERR_INVALID;
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)stream;
  int rc;
  // the offset table's device copy is the store path's (c->pack_table): taken like a store takes it, behind the copies of
  // the previous job (no arena is needed: the blobs are read where they lie)
  if ((rc = store_acquire(c, s, 0, 8 * ((size_t)P * nchunks + 2)))) return rc;
  pa.blob_ptrs = (const u8* const*)blob_ptrs; pa.blob_bytes = blob_bytes;
  pa.n = nchunks; pa.L = L; pa.G = (int)pa.hdr.ngroups;
  pa.host = (u8*)pack_d; pa.cap = pack_cap; pa.table_d = c->pack_table.p;
  pa.status = job_status ? job_status : c->status_h;
  pa.p_begin = 0; pa.p_end = P; pa.last = 1; pa.part_h = nullptr;
  std::lock_guard<std::mutex> lk(c->mu);
  c->pn = 0;
  if ((rc = prof_mark(c, s))) return rc;
  hipLaunchKernelGGL(k_pack_scan<true>, dim3(1), dim3(256), 0, s, pa);
  HIP_TRY(hipGetLastError());
  // HBM to HBM: as many workgroups as there are items to walk, up to one per CU
  const int items = (P + 1) * nchunks;
  hipLaunchKernelGGL(k_pack_copy<true>, dim3((unsigned)std::max(1, std::min(items, c->num_cus))), dim3(256), 0, s, pa);
  HIP_TRY(hipGetLastError());
  if ((rc = prof_mark(c, s))) return rc;
  return store_release(c, s);  // the next job may rewrite the table behind this
}

int lmc_pack_chunk_bytes(const void* pack_h, uint64_t nbytes, int32_t chunk, uint32_t* size_out) {
  lmc_pack_header h;
  const u8* b = (const u8*)pack_h;
  if (!pack_ok(b, nbytes, &h) || chunk < 0 || (uint32_t)chunk >= h.nchunks || !size_out) return LMC_ERR_INVALID;
  const uint32_t size = pack_chunk_walk(b, h, (uint32_t)chunk, nullptr, 0);  // lmc_pack_extract's checks and walk, without the copies
  if (!size) return LMC_ERR_INVALID;
  *size_out = size;
  return LMC_OK;
}

int lmc_unpack_blobs(lmc_ctx* c, const void* pack_h, uint64_t pack_bytes, int32_t chunk_begin, int32_t nchunks,
                     void* const* blob_ptrs_h, const uint32_t* blob_caps_h, uint32_t* job_status, lmc_stream_t stream) {
  lmc_pack_header h;
  if (!c || !blob_ptrs_h || !blob_caps_h || nchunks < 1 || chunk_begin < 0 || !pack_ok((const u8*)pack_h, pack_bytes, &h))
    return LMC_ERR_INVALID;
  if ((uint32_t)chunk_begin >= h.nchunks || (uint32_t)nchunks > h.nchunks - (uint32_t)chunk_begin) return LMC_ERR_INVALID;
  {  // the kernel computes section offsets from the pack's geometry words: they must be a geometry's
    const uint64_t C = (uint64_t)h.num_heads * h.head_size;
    if (C < 8 || (C & 7) || C > LMC_MAX_CHANNELS) return LMC_ERR_INVALID;
    lmc_pack_header ref;
    lmc_pack_layout(h.nchunks, h.num_layers, h.chunk_tokens, h.num_heads, h.head_size, &ref);
    if (h.ngroups != ref.ngroups || h.static_stride != ref.static_stride) return LMC_ERR_INVALID;
  }
  for (int i = 0; i < nchunks; i++)
    if (!blob_ptrs_h[i] || ((uintptr_t)blob_ptrs_h[i] & 15)) return LMC_ERR_INVALID;
  const int n = (int)h.nchunks, c0 = chunk_begin, m = nchunks, L = (int)h.num_layers, P = 2 * L;
  const u8* b = (const u8*)pack_h;
  const uint64_t* t = (const uint64_t*)(b + h.off_table);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)stream;
  int rc;
  std::lock_guard<std::mutex> lk(c->mu);
  // the load staging holds the pack at its own offsets (as for lmc_load_pack), and behind it the destinations' addresses
  // and their room
  const size_t meta_off = (size_t)lmc_r16_64(h.total_bytes), caps_off = meta_off + (size_t)lmc_r16_64(8 * (uint64_t)m);
  const size_t need = caps_off + (size_t)lmc_r16_64(4 * (uint64_t)m);
  hipStream_t cs[2];  // the order of arrival does not matter here: two DMA queues
  if ((rc = load_acquire(c, need, 2, cs))) return rc;
  u8* dev = c->load_slots.p;
  // (the two arrays are the caller's pageable memory: hipMemcpyAsync has read them when it returns)
  HIP_TRY(hipMemcpyAsync(dev + meta_off, blob_ptrs_h, 8 * (size_t)m, hipMemcpyHostToDevice, cs[0]));
  HIP_TRY(hipMemcpyAsync(dev + caps_off, blob_caps_h, 4 * (size_t)m, hipMemcpyHostToDevice, cs[0]));
  HIP_TRY(hipMemcpyAsync(dev + h.off_table, b + h.off_table, 8 * ((size_t)P * n + 1), hipMemcpyHostToDevice, cs[0]));
  HIP_TRY(hipMemcpyAsync(dev + h.off_static + (size_t)c0 * h.static_stride, b + h.off_static + (size_t)c0 * h.static_stride,
                         (size_t)m * h.static_stride, hipMemcpyHostToDevice, cs[1]));
  if (m == n) {  // the whole streams region, a half per queue
    const uint64_t all = t[(uint64_t)P * n], half = (all / 2) & ~(uint64_t)15;
    if (half) HIP_TRY(hipMemcpyAsync(dev + h.off_streams, b + h.off_streams, half, hipMemcpyHostToDevice, cs[0]));
    if (all > half) HIP_TRY(hipMemcpyAsync(dev + h.off_streams + half, b + h.off_streams + half, all - half, hipMemcpyHostToDevice, cs[1]));
  } else {
    for (int p = 0; p < P; p++) {  // a run of the m chunks per plane
      const uint64_t lo = t[(uint64_t)p * n + c0], hi = t[(uint64_t)p * n + c0 + m];
      if (hi > lo) HIP_TRY(hipMemcpyAsync(dev + h.off_streams + lo, b + h.off_streams + lo, hi - lo, hipMemcpyHostToDevice, cs[p & 1]));
    }
  }
  for (int q = 0; q < 2; q++)
    if ((rc = stream_follows(c, s, cs[q]))) return rc;
  UnpackArgs ua;
  memset(&ua, 0, sizeof ua);
  ua.pack = dev; ua.off_table = h.off_table; ua.off_static = h.off_static; ua.off_streams = h.off_streams;
  ua.streams_bytes = h.total_bytes - h.off_streams; ua.static_stride = h.static_stride;
  ua.n = n; ua.c0 = c0; ua.m = m; ua.L = L; ua.G = (int)h.ngroups; ua.chunk_tokens = h.chunk_tokens;
  ua.dst_ptrs = (u8* const*)(dev + meta_off); ua.dst_caps = (const u32*)(dev + caps_off);
  ua.status = job_status ? job_status : c->status_h;
  c->pn = 0;
  if ((rc = prof_mark(c, s))) return rc;
  const int items = (P + 1) * m;
  hipLaunchKernelGGL(k_unpack, dim3((unsigned)std::max(1, std::min(items, c->num_cus))), dim3(256), 0, s, ua);
  HIP_TRY(hipGetLastError());
  if ((rc = prof_mark(c, s))) return rc;
  return load_release(c, s);
}

int lmc_blob_info(const void* blob_h, size_t nbytes, lmc_blob_header* out) {
  if (!blob_h || !out || nbytes < sizeof(lmc_blob_header)) return LMC_ERR_INVALID;
  lmc_blob_header h;
  memcpy(&h, blob_h, sizeof h);
  if (h.magic != LMC_BLOB_MAGIC || h.version != LMC_BLOB_VERSION || h.header_bytes != LMC_HEADER_BYTES) return LMC_ERR_INVALID;
  if (h.num_layers == 0 || h.ntokens == 0 || h.num_heads == 0 || h.head_size == 0) return LMC_ERR_INVALID;
  const bool fixed = h.model == LMC_MODEL_FIXED;  // (lmc_model_valid is about the coded models)
  if (h.num_layers > LMC_MAX_PLANES / 2 || h.ntokens > 65535u || !(fixed ? lmc_fixed_valid(h.ntokens) : lmc_model_valid(h.model, h.ntokens)))
    return LMC_ERR_INVALID;
  if ((uint64_t)h.num_heads * h.head_size > LMC_MAX_CHANNELS) return LMC_ERR_INVALID;
  lmc_blob_header ref;
  memset(&ref, 0, sizeof ref);
  lmc_blob_layout(h.num_layers, h.ntokens, h.num_heads, h.head_size, &ref);
  if (h.nchannels != ref.nchannels || h.nplanes != ref.nplanes || h.ngroups != ref.ngroups || h.lp != ref.lp ||
      h.off_bins != ref.off_bins || h.off_scales != ref.off_scales || h.off_scsum != ref.off_scsum ||
      h.off_gdir != ref.off_gdir || h.off_streams != ref.off_streams)
    return LMC_ERR_INVALID;
  if (h.total_bytes != h.off_streams + h.stream_bytes || h.total_bytes > nbytes) return LMC_ERR_INVALID;
  if (h.kv_dtype != 0u && !((h.kv_dtype == LMC_DTYPE_FP8_E4M3 || h.kv_dtype == LMC_DTYPE_FP8_E5M2) && h.dtype == LMC_DTYPE_BF16))
    return LMC_ERR_INVALID;
  if (fixed) {
    // (this call may be handed the header alone, with the blob's length: what the header can say is checked here, the
    // bins and the directory by lmc_fixed_blob_info)
    const uint64_t n = (uint64_t)h.nplanes * h.ngroups;
    if (h.kv_dtype != 0u || (uint64_t)h.stream_bytes < n * lmc_fixed_stream_bytes(4u, h.ntokens) ||
        (uint64_t)h.stream_bytes > n * lmc_fixed_stream_bytes(LMC_MAX_BINS, h.ntokens))
      return LMC_ERR_INVALID;
  }
  *out = h;
  return LMC_OK;
}

int lmc_fixed_blob_info(const void* blob_h, size_t nbytes, lmc_blob_header* out) {
  lmc_blob_header h;
  const int rc = lmc_blob_info(blob_h, nbytes, &h);
  if (rc) return rc;
  if (h.model != LMC_MODEL_FIXED || !out) return LMC_ERR_INVALID;
  // totals and directory are functions of (bins, T): held against the computed layout (total_bytes <= nbytes: lmc_blob_info)
  const uint8_t* const b = (const uint8_t*)blob_h;
  for (uint32_t p = 0; p < h.nplanes; p++)
    if (b[h.off_bins + p] < 4u || b[h.off_bins + p] > LMC_MAX_BINS) return LMC_ERR_INVALID;
  if ((uint64_t)h.total_bytes != lmc_fixed_blob_bytes(h.num_layers, h.ntokens, h.num_heads, h.head_size, b + h.off_bins))
    return LMC_ERR_INVALID;
  uint32_t beg = 0;
  for (uint32_t p = 0; p < h.nplanes; p++) {
    const uint32_t sz = lmc_fixed_stream_bytes(b[h.off_bins + p], h.ntokens);
    for (uint32_t g = 0; g < h.ngroups; g++, beg += sz) {
      uint32_t gd[2];
      memcpy(gd, b + h.off_gdir + 8u * (p * h.ngroups + g), sizeof gd);
      if (gd[0] != beg || gd[1] != beg + sz) return LMC_ERR_INVALID;
    }
  }
  *out = h;
  return LMC_OK;
}

}  // extern "C"
