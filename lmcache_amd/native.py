"""ctypes binding of liblmc_hip.so (include/lmc_hip.h) -- the only door from the
Python host side into the HIP hot path.

There is NO CPU fallback: if the library is missing or was not built for this
box the import-time loader raises, and every product entry point fails loudly.
torch is used only as plumbing (device memory, streams); torch types never
cross the C ABI -- tensors are passed as raw device pointers.
"""
import ctypes
import os
import subprocess
import sys
import threading
from typing import NamedTuple, Optional, Sequence, Tuple

import torch  # must be imported before the .so so that a single libamdhip64 (torch's) is loaded

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
# LMCACHE_AMD_SO: an alternative build of the same library (A/B timing of experimental kernels: tools/probes)
SO_PATH = os.environ.get("LMCACHE_AMD_SO") or os.path.join(CSRC, "liblmc_hip.so")
INCLUDE = os.path.join(os.path.dirname(_HERE), "include")

BF16, FP16 = 0, 1
FP8_E4M3, FP8_E5M2 = 2, 3  # OCP fp8 (torch.float8_e4m3fn / float8_e5m2): stored as the bf16 blob of their images
LANES, MAX_BINS, LP = 64, 32, 33
HEADER_BYTES = 128
BLOB_MAGIC = 0x31434D4C

HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-strict-aliasing",
               "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-Wl,-rpath,/opt/rocm/lib"]


def build(force: bool = False) -> str:
    """Compile lmcache_amd/csrc/lmc_api.hip for gfx950 with hipcc, in-tree."""
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h"))]
    srcs += [os.path.join(INCLUDE, f) for f in os.listdir(INCLUDE)]
    newest = max(os.path.getmtime(s) for s in srcs)
    # (kernel_resources.json is a by-product, never a reason to rebuild: a prebuilt or read-only install, or a box
    # without hipcc, loads an up-to-date library as it is -- ADVICE r05; the test that reads the file skips without it)
    if force or not os.path.exists(SO_PATH) or os.path.getmtime(SO_PATH) < newest:
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        # -Rpass-analysis=kernel-resource-usage: the register / scratch / LDS figures of every kernel come out of the SAME
        # compile as remarks; they are kept beside the library (kernel_resources.json) so that a test can hold the hot
        # kernels' ScratchSize against what DESIGN.md says (round 4's commit log said "without spills" about a kernel
        # that spilled 68 bytes)
        cmd = [hipcc] + HIPCC_FLAGS + ["-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "lmc_api.hip"), "-o", SO_PATH]
        proc = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
        if proc.returncode != 0:
            sys.stderr.write(proc.stderr)
            raise subprocess.CalledProcessError(proc.returncode, cmd)
        # a diagnostic is several lines (the caret, the notes): all of them, without the resource remarks
        if "warning:" in proc.stderr or "error:" in proc.stderr:
            sys.stderr.write("\n".join(l for l in proc.stderr.splitlines() if "[-Rpass-analysis=kernel-resource-usage]" not in l) + "\n")
        _write_kernel_resources(proc.stderr)
        _check_decoder_registers()
        _check_fixed_registers()
    return SO_PATH


def _check_fixed_registers() -> None:
    """k_fixed_encode's instances -- the one-piece encode's and the LAYER ones of the sliced per-layer launches (k_fixed.h,
    FixedEncArgs) -- and k_fixed_layers_finish must not spill: a build in which one of them uses scratch is refused here,
    as the decoder's is above."""
    import json
    res = json.load(open(RESOURCES_PATH))
    bad = {k: v.get("ScratchSize") for k, v in res.items()
           if ("k_fixed_encode" in k or "k_fixed_layers_finish" in k) and v.get("ScratchSize") != 0}
    if bad:
        try:
            os.remove(SO_PATH)
        except OSError:
            pass
        raise RuntimeError(f"k_fixed_encode / k_fixed_layers_finish must not use scratch (k_fixed.h); got {bad}")


def _check_decoder_registers() -> None:
    """k_decode keeps the word ring's in-flight block in AGPR a0 WITHOUT telling the compiler (k_decode.h,
    LMC_DEC_A0_CLOBBER): that is only sound while the kernel has exactly 60 VGPRs and no AGPRs of the compiler's own --
    a0 is then physical register 60 of a 64-register allocation.  A build that comes out differently is refused here,
    loudly, instead of decoding with a register that belongs to another wave."""
    import json
    res = json.load(open(RESOURCES_PATH))
    bad = {k: (v.get("VGPRs"), v.get("AGPRs")) for k, v in res.items()
           if "k_decode" in k and (v.get("VGPRs") != 60 or v.get("AGPRs") != 0)}
    if bad:
        try:
            os.remove(SO_PATH)
        except OSError:
            pass
        raise RuntimeError(f"k_decode must compile to 60 VGPRs / 0 AGPRs (hidden a0, see k_decode.h); got {bad}")


RESOURCES_PATH = os.path.join(CSRC, "kernel_resources.json")


def _write_kernel_resources(remarks: str) -> None:
    import json
    import re
    table, cur = {}, None
    for line in remarks.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = table.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill|"
                      r"LDS Size \[bytes/block\]): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).split(" [")[0]] = int(m.group(2))
    demangled = {}
    try:
        out = subprocess.run(["c++filt"] + list(table), stdout=subprocess.PIPE, text=True).stdout.split("\n")
        demangled = dict(zip(table, out))
    except Exception:
        pass
    with open(RESOURCES_PATH, "w") as f:
        json.dump({demangled.get(k, k): v for k, v in sorted(table.items())}, f, indent=1)


class KvLayoutStruct(ctypes.Structure):
    _fields_ = [("dtype", ctypes.c_int32), ("num_layers", ctypes.c_int32), ("num_heads", ctypes.c_int32),
                ("head_size", ctypes.c_int32), ("base", ctypes.c_void_p), ("plane_ptrs", ctypes.c_void_p),
                ("stride_layer", ctypes.c_int64), ("stride_kv", ctypes.c_int64), ("stride_token", ctypes.c_int64),
                ("stride_head", ctypes.c_int64), ("slot_mapping", ctypes.c_void_p), ("block_size", ctypes.c_int32),
                ("paged_kind", ctypes.c_int32), ("stride_block", ctypes.c_int64)]


PAGED_ROWS, PAGED_SPLIT = 0, 1  # LMC_PAGED_*: lmc_kv_layout.paged_kind


class RangePostStruct(ctypes.Structure):
    """lmc_range_post (include/lmc_hip.h): what is done to each layer range of a decode job before its event."""
    _fields_ = [("cos_sin", ctypes.c_void_p), ("table_rows", ctypes.c_int32), ("rot_dim", ctypes.c_int32),
                ("is_neox", ctypes.c_int32), ("delta", ctypes.c_int32), ("deltas", ctypes.c_void_p),
                ("tok_begin", ctypes.c_int32), ("ntok", ctypes.c_int32), ("scatter_dst", ctypes.POINTER(KvLayoutStruct)),
                ("scatter_tok0", ctypes.c_int32)]


class HeadWindowStruct(ctypes.Structure):
    """lmc_head_window (include/lmc_hip.h): the heads a decode takes out of every blob, and where they land in dst."""
    _fields_ = [("src_heads", ctypes.c_int32), ("src_head_begin", ctypes.c_int32), ("nheads", ctypes.c_int32),
                ("dst_head_begin", ctypes.c_int32)]


class HeadWindow(NamedTuple):
    """Heads [src_head_begin, src_head_begin + nheads) of blobs that have src_heads heads -> heads [dst_head_begin, ...)
    of a destination with a head count of its own: KV stored under another tensor-parallel degree (resharding.py)."""
    src_heads: int
    src_head_begin: int
    nheads: int
    dst_head_begin: int

    def struct(self) -> HeadWindowStruct:
        return HeadWindowStruct(int(self.src_heads), int(self.src_head_begin), int(self.nheads), int(self.dst_head_begin))


class BlobHeader(ctypes.Structure):
    _fields_ = [("magic", ctypes.c_uint32), ("version", ctypes.c_uint16), ("header_bytes", ctypes.c_uint16),
                ("dtype", ctypes.c_uint32), ("num_layers", ctypes.c_uint32), ("ntokens", ctypes.c_uint32),
                ("num_heads", ctypes.c_uint32), ("head_size", ctypes.c_uint32), ("nchannels", ctypes.c_uint32),
                ("nplanes", ctypes.c_uint32), ("ngroups", ctypes.c_uint32), ("lp", ctypes.c_uint32),
                ("off_bins", ctypes.c_uint32), ("off_scales", ctypes.c_uint32), ("zero13", ctypes.c_uint32),
                ("off_gdir", ctypes.c_uint32), ("off_streams", ctypes.c_uint32), ("stream_bytes", ctypes.c_uint32),
                ("total_bytes", ctypes.c_uint32), ("zero18", ctypes.c_uint32 * 3),
                ("off_scsum", ctypes.c_uint32), ("model", ctypes.c_uint32), ("kv_dtype", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32 * 8)]


class PackHeader(ctypes.Structure):
    _fields_ = [("magic", ctypes.c_uint32), ("version", ctypes.c_uint32), ("header_bytes", ctypes.c_uint32),
                ("nchunks", ctypes.c_uint32), ("num_layers", ctypes.c_uint32), ("num_heads", ctypes.c_uint32),
                ("head_size", ctypes.c_uint32), ("chunk_tokens", ctypes.c_uint32), ("ngroups", ctypes.c_uint32),
                ("static_stride", ctypes.c_uint32), ("ntokens", ctypes.c_uint32), ("reserved0", ctypes.c_uint32),
                ("off_table", ctypes.c_uint64), ("off_static", ctypes.c_uint64), ("off_streams", ctypes.c_uint64),
                ("total_bytes", ctypes.c_uint64), ("reserved", ctypes.c_uint32 * 44)]


# name -> (restype, argtypes); every symbol include/lmc_hip.h declares
_vp, _i32, _u64, _sz = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint64, ctypes.c_size_t
_PL = ctypes.POINTER(KvLayoutStruct)
SYMBOLS = {
    "lmc_strerror": (ctypes.c_char_p, [ctypes.c_int]),
    "lmc_last_hip_error": (ctypes.c_int, []),
    "lmc_abi_version": (ctypes.c_int, []),
    "lmc_ctx_create": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(_vp)]),
    "lmc_ctx_destroy": (ctypes.c_int, [_vp]),
    "lmc_ctx_reserve": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "lmc_device_status": (ctypes.c_int, [_vp, ctypes.c_int]),
    "lmc_ctx_set_encode_path": (ctypes.c_int, [_vp, ctypes.c_int]),
    "lmc_ctx_set_fixed_layer_slices": (ctypes.c_int, [_vp, ctypes.c_int]),
    "lmc_ctx_profile": (ctypes.c_int, [_vp, ctypes.c_int]),
    "lmc_ctx_profile_read": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_float), ctypes.c_int]),
    "lmc_quantize": (ctypes.c_int, [_vp, _PL, _i32, _i32, _vp, _vp, _vp, _vp]),
    "lmc_calculate_cdf": (ctypes.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp]),
    "lmc_encode_chunks": (ctypes.c_int, [_vp, _PL, _i32, _i32, _i32, _vp, _vp, _u64, _vp, _vp, _vp]),
    "lmc_encode_chunks_split": (ctypes.c_int, [_vp, _PL, _i32, _i32, _i32, _vp, _vp, _u64, _vp, _vp, _vp]),
    "lmc_encode_chunks_fixed": (ctypes.c_int, [_vp, _PL, _i32, _i32, _i32, _vp, _vp, _u64, _vp, _vp, _vp]),
    "lmc_encode_chunks_fixed_split": (ctypes.c_int, [_vp, _PL, _i32, _i32, _i32, _vp, _vp, _u64, _vp, _vp, _vp]),
    "lmc_encode_layers_begin": (ctypes.c_int, [_vp, _PL, _i32, _i32, _i32, _vp, _vp, _u64, _vp, _vp, ctypes.POINTER(_vp)]),
    "lmc_encode_layers_begin_fixed": (ctypes.c_int, [_vp, _PL, _i32, _i32, _i32, _vp, _vp, _u64, _vp, _vp, ctypes.POINTER(_vp)]),
    "lmc_encode_layer": (ctypes.c_int, [_vp, _vp, _i32, _vp]),
    "lmc_encode_layers_finish": (ctypes.c_int, [_vp, _vp, _vp]),
    "lmc_encode_layers_abort": (ctypes.c_int, [_vp, _vp]),
    "lmc_decode_chunks": (ctypes.c_int, [_vp, _vp, _u64, _i32, _PL, _i32, _i32, _vp, _vp]),
    "lmc_decode_chunks_layers": (ctypes.c_int, [_vp, _vp, _u64, _i32, _PL, _i32, _i32, _i32, _i32, _vp, _vp]),
    "lmc_decode_chunks_schedule": (ctypes.c_int, [_vp, _vp, _u64, _i32, _PL, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "lmc_decode_chunks_schedule_post": (ctypes.c_int, [_vp, _vp, _u64, _i32, _PL, _i32, _i32, _i32, _vp, _vp, _vp, _vp,
                                                       ctypes.POINTER(RangePostStruct)]),
    "lmc_decode_chunks_fixed_schedule": (ctypes.c_int, [_vp, _vp, _u64, _i32, _PL, _i32, _i32, _i32, _vp, _vp,
                                                        ctypes.POINTER(RangePostStruct), _vp, _vp]),
    "lmc_decode_chunks_fixed_split_schedule": (ctypes.c_int, [_vp, _vp, _u64, _i32, _PL, _i32, _i32, _i32, _vp, _vp,
                                                              ctypes.POINTER(RangePostStruct), _vp, _vp]),
    "lmc_decode_chunks_heads_schedule": (ctypes.c_int, [_vp, _vp, _u64, _i32, _PL, _i32, _i32, _i32, _vp, _vp,
                                                        ctypes.POINTER(HeadWindowStruct), _vp, _vp]),
    "lmc_decode_chunks_fixed_heads_schedule": (ctypes.c_int, [_vp, _vp, _u64, _i32, _PL, _i32, _i32, _i32, _vp, _vp,
                                                              ctypes.POINTER(HeadWindowStruct), _vp, _vp]),
    "lmc_decode_symbols": (ctypes.c_int, [_vp, _vp, _i32, _i32, _i32, _vp, _vp]),
    "lmc_store_chunks": (ctypes.c_int, [_vp, _PL, _i32, _i32, _i32, _vp, _vp, _u64, _vp, _vp, _vp, _vp]),
    "lmc_load_chunks": (ctypes.c_int, [_vp, _vp, _vp, _i32, _PL, _i32, _i32, _i32, _vp, _vp, _vp]),
    "lmc_store_pack": (ctypes.c_int, [_vp, _PL, _i32, _i32, _i32, _vp, _vp, _u64, _vp, _vp, _vp]),
    "lmc_store_pack_parts": (ctypes.c_int, [_vp, _PL, _i32, _i32, _i32, _vp, _vp, _u64, _vp, _i32, _vp, _vp, _vp, _vp]),
    "lmc_pack_info": (ctypes.c_int, [_vp, _u64, ctypes.POINTER(PackHeader)]),
    "lmc_pack_extract": (ctypes.c_int, [_vp, _u64, _i32, _vp, _u64, _vp]),
    "lmc_load_pack": (ctypes.c_int, [_vp, _vp, _u64, _i32, _i32, _PL, _i32, _i32, _vp, _vp, _vp]),
    "lmc_load_pack_post": (ctypes.c_int, [_vp, _vp, _u64, _i32, _i32, _PL, _i32, _i32, _vp, _vp, _vp,
                                          ctypes.POINTER(RangePostStruct)]),
    "lmc_pack_blobs": (ctypes.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, ctypes.c_uint32, _vp, _u64, _vp, _vp]),
    "lmc_transcode_fixed": (ctypes.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, ctypes.c_uint32, _vp, _vp, _u64, _vp, _vp,
                                           _vp]),
    "lmc_transcode_to_fixed": (ctypes.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, ctypes.c_uint32, _vp, _vp, _vp, _vp,
                                              _vp]),
    "lmc_unpack_blobs": (ctypes.c_int, [_vp, _vp, _u64, _i32, _i32, _vp, _vp, _vp, _vp]),
    "lmc_pack_chunk_bytes": (ctypes.c_int, [_vp, _u64, _i32, ctypes.POINTER(ctypes.c_uint32)]),
    "lmc_copy_kv": (ctypes.c_int, [_vp, _PL, _i32, _i32, _PL, _i32, _vp]),
    "lmc_rope_shift": (ctypes.c_int, [_vp, _PL, _i32, _i32, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "lmc_rope_shift_split": (ctypes.c_int, [_vp, _PL, _i32, _i32, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "lmc_kv_deviation": (ctypes.c_int, [_vp, _PL, _i32, _i32, _PL, _i32, _i32, _i32, _vp, _vp, _vp]),
    "lmc_select_topk": (ctypes.c_int, [_vp, _vp, _i32, _i32, _vp, _vp]),
    "lmc_pinned_alloc": (ctypes.c_int, [_sz, ctypes.POINTER(_vp)]),
    "lmc_pinned_free": (ctypes.c_int, [_vp]),
    "lmc_memcpy_async": (ctypes.c_int, [_vp, _vp, _sz, ctypes.c_int, _vp]),
    "lmc_stream_create": (ctypes.c_int, [ctypes.POINTER(_vp)]),
    "lmc_stream_destroy": (ctypes.c_int, [_vp]),
    "lmc_stream_synchronize": (ctypes.c_int, [_vp]),
    "lmc_stream_wait_event": (ctypes.c_int, [_vp, _vp]),
    "lmc_event_create": (ctypes.c_int, [ctypes.POINTER(_vp), ctypes.c_int]),
    "lmc_event_destroy": (ctypes.c_int, [_vp]),
    "lmc_event_record": (ctypes.c_int, [_vp, _vp]),
    "lmc_event_synchronize": (ctypes.c_int, [_vp]),
    "lmc_event_query": (ctypes.c_int, [_vp]),
    "lmc_event_elapsed_ms": (ctypes.c_int, [_vp, _vp, ctypes.POINTER(ctypes.c_float)]),
    "lmc_blob_info": (ctypes.c_int, [_vp, _sz, ctypes.POINTER(BlobHeader)]),
    "lmc_fixed_blob_info": (ctypes.c_int, [_vp, _sz, ctypes.POINTER(BlobHeader)]),
}

# where the lmc_range_post pointer stands among the last three arguments of the symbols that take one ("status, stream,
# post" or "post, status, stream"): read off the argument types above.  The head-window schedules carry their
# lmc_head_window pointer in the same place ("win, status, stream") and take no post: one slot table for both.
_RP, _HW = ctypes.POINTER(RangePostStruct), ctypes.POINTER(HeadWindowStruct)
_POST_SLOT = {name: args.index(t) - (len(args) - 3) for name, (_, args) in SYMBOLS.items() for t in (_RP, _HW) if t in args}

ENCODE_PATHS = {"auto": 0, "two_kernels": 1, "fused": 2}  # LMC_ENCODE_PATH_*
ERR_INVALID = -1      # LMC_ERR_INVALID
NOT_LAYERWISE = 1     # LMC_NOT_LAYERWISE: lmc_encode_layers_begin found the job not eligible (no error, no job)

_lib = None
_lib_lock = threading.Lock()


class NativeError(RuntimeError):
    pass


def lib() -> ctypes.CDLL:
    """Load liblmc_hip.so (built in-tree by build()).  Raises if absent: there is no fallback path."""
    global _lib
    with _lib_lock:
        if _lib is None:
            if not os.path.exists(SO_PATH):
                raise NativeError(
                    f"{SO_PATH} is missing: the MI355X HIP extension has not been built "
                    f"(run `python -c 'import __graft_entry__ as g; g.build()'`). lmcache_amd has no CPU fallback.")
            L = ctypes.CDLL(SO_PATH)
            for name, (res, args) in SYMBOLS.items():
                fn = getattr(L, name)  # AttributeError if the ABI and this binding drift apart
                fn.restype, fn.argtypes = res, args
            if L.lmc_abi_version() != 6:
                raise NativeError("liblmc_hip.so ABI version mismatch; rebuild")
            _lib = L
    return _lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        L = lib()
        msg = L.lmc_strerror(rc).decode()
        raise NativeError(f"{what or 'lmc call'} failed: {msg} (rc={rc}, hip={L.lmc_last_hip_error()})")


_CODES = {torch.bfloat16: BF16, torch.float16: FP16, torch.float8_e4m3fn: FP8_E4M3, torch.float8_e5m2: FP8_E5M2}
_DTYPES = {v: k for k, v in _CODES.items()}


def dtype_code(dt: torch.dtype) -> int:
    code = _CODES.get(dt)
    if code is not None:
        return code
    if dt == torch.uint8:
        raise ValueError("KV dtype torch.uint8: an fp8 cache allocated as bytes (vLLM does that) has to be passed as "
                         "its fp8 view, e.g. kv_cache.view(torch.float8_e4m3fn) (or torch.float8_e5m2); the view copies nothing")
    if dt in (getattr(torch, "float8_e4m3fnuz", None), getattr(torch, "float8_e5m2fnuz", None)):
        raise ValueError(f"KV dtype {dt} is an MI300 (fnuz) fp8 format; gfx950 caches use the OCP formats "
                         "torch.float8_e4m3fn / torch.float8_e5m2")
    raise ValueError(f"KV dtype must be bfloat16, float16, float8_e4m3fn or float8_e5m2, got {dt} "
                     "(float32 KV is not supported: convert it to bfloat16)")


def torch_dtype(code: int) -> torch.dtype:
    return _DTYPES[int(code)]


def elem_bytes(code: int) -> int:
    """Bytes of one KV element of dtype code `code`."""
    return 1 if int(code) in (FP8_E4M3, FP8_E5M2) else 2


def stored_dtype(h) -> torch.dtype:
    """The dtype a blob's KV was stored in (its header's kv_dtype, else its dtype): what the engine retrieves."""
    return torch_dtype(int(h.kv_dtype) or int(h.dtype))


def pack_info(pack_ptr: int, nbytes: int) -> PackHeader:
    """Checked header of a pack in host memory (lmc_pack_info); raises NativeError if it does not check out."""
    h = PackHeader()
    check(lib().lmc_pack_info(pack_ptr, nbytes, ctypes.byref(h)), "lmc_pack_info")
    return h


def pack_extract(pack_ptr: int, nbytes: int, chunk: int) -> bytes:
    """Chunk `chunk` of a pack as the blob lmc_encode_chunks wrote (lmc_pack_extract)."""
    h = pack_info(pack_ptr, nbytes)
    cap = blob_bound(h.num_layers, h.chunk_tokens, h.num_heads, h.head_size)
    buf = ctypes.create_string_buffer(cap)
    size = ctypes.c_uint32(0)
    check(lib().lmc_pack_extract(pack_ptr, nbytes, chunk, buf, cap, ctypes.byref(size)), "lmc_pack_extract")
    return buf.raw[:size.value]


def pack_chunk_bytes(pack_ptr: int, nbytes: int, chunk: int) -> int:
    """Size of chunk `chunk` of a pack as a blob (lmc_pack_chunk_bytes): what pack_extract would return, not extracted."""
    size = ctypes.c_uint32(0)
    check(lib().lmc_pack_chunk_bytes(pack_ptr, nbytes, chunk, ctypes.byref(size)), "lmc_pack_chunk_bytes")
    return int(size.value)


def pack_bound(n: int, L: int, chunk_tokens: int, H: int, D: int) -> int:
    """lmc_pack_bound (lmc_format.h): worst-case bytes of a pack of n chunks."""
    G = (H * D + LANES - 1) // LANES
    static = r16(blob_static_bytes(L, chunk_tokens, H, D))
    return r16(256 + 8 * (2 * L * n + 1)) + n * static + n * 2 * L * G * group_cap_bytes(chunk_tokens)


def pack_off_streams(n: int, L: int, chunk_tokens: int, H: int, D: int) -> int:
    """lmc_pack_layout's off_streams: where the segments of a pack of n chunks begin (header, offset table, static slots in front)."""
    return r16(256 + 8 * (2 * L * n + 1)) + n * r16(blob_static_bytes(L, chunk_tokens, H, D))


def r16(x: int) -> int:
    return (x + 15) & ~15


def group_cap_bytes(T: int) -> int:
    """lmc_group_cap_bytes: the largest head (31 symbols, every width at its maximum) + words and states."""
    stored = 255 if T == 256 else T
    return r16(32 + 8 * 31 * stored.bit_length()) + r16(LANES * (T + 8))


def blob_static_bytes(L: int, T: int, H: int, D: int) -> int:
    """Bytes in front of the streams section (lmc_blob_layout): header, bins, scales, their checksums, the stream
    directory."""
    C, P = H * D, 2 * L
    G = (C + LANES - 1) // LANES
    off = HEADER_BYTES + r16(P)
    off += r16(2 * P * T)
    off += r16(4 * P)
    off += r16(8 * P * G)
    return off


def blob_bound(L: int, T: int, H: int, D: int) -> int:
    """Worst-case blob size (lmc_blob_bound in include/lmc_format.h)."""
    C, P = H * D, 2 * L
    G = (C + LANES - 1) // LANES
    return blob_static_bytes(L, T, H, D) + P * G * group_cap_bytes(T)


MODEL_CDF16, MODEL_COUNTS, MODEL_FIXED = 0, 1, 2  # LMC_MODEL_*: the header's `model` word
FIXED_NARROW_BINS = 17                            # LMC_FIXED_NARROW_BINS


def fixed_stream_bytes(bins: int, T: int) -> int:
    """lmc_fixed_stream_bytes: one group stream of the fixed-width model (lo, hi of a wide plane, tail)."""
    return (256 if bins <= FIXED_NARROW_BINS else 320) * ((T + 7) // 8) + 16


def fixed_blob_bytes(L: int, T: int, H: int, D: int, bins: Sequence[int]) -> int:
    """lmc_fixed_blob_bytes: the exact size of an LMC_MODEL_FIXED blob; bins: the per-plane bins [2 L]."""
    assert len(bins) == 2 * L
    G = (H * D + LANES - 1) // LANES
    return blob_static_bytes(L, T, H, D) + G * sum(fixed_stream_bytes(int(b), T) for b in bins)


def current_stream_ptr(device=None) -> int:
    return torch.cuda.current_stream(device).cuda_stream


class _PointerTables:
    """Device copies of plane-pointer tables (lmc_kv_layout.plane_ptrs), keyed by the pointers themselves.

    A serving engine hands the same per-layer KV tensors to every store()/retrieve(), so the table of a call
    is almost always one uploaded before: no copy, no host wait.  A table seen for the first time goes through
    pinned staging on a PRIVATE copy stream and the host waits for that 2 KiB copy alone (~20 us) -- never for
    the work queued on the caller's stream (the reference's own note on this path: "synchronize is harmful",
    local_backend.py:83-90) -- so the table is complete before a kernel on ANY stream can be launched with it."""
    MAX_CACHED = 4096   # 2 KiB each; when full the cache is dropped after a device synchronise (once in a blue moon)

    def __init__(self):
        self._lock = threading.Lock()
        self._cache = {}     # (device index, ptrs tuple) -> device int64 tensor
        self._stage = None   # PinnedBuffer, 2 KiB
        self._streams = {}   # device index -> private copy stream

    def get(self, ptrs: Sequence[int], device: torch.device) -> torch.Tensor:
        key = (device.index, tuple(ptrs))
        with self._lock:
            t = self._cache.get(key)
            if t is not None:
                return t
            n = len(ptrs)
            assert n <= 256, "at most 256 planes"
            if self._stage is None:
                self._stage = PinnedBuffer(2048)
            self._stage.tensor[:8 * n].view(torch.int64).copy_(torch.tensor(ptrs, dtype=torch.int64))
            with torch.cuda.device(device):
                st = self._streams.get(device.index)
                if st is None:
                    st = self._streams[device.index] = torch.cuda.Stream(device=device)
                if len(self._cache) >= self.MAX_CACHED:
                    torch.cuda.synchronize(device)  # nobody reads the old tables any more
                    self._cache.clear()
                with torch.cuda.stream(st):  # the block belongs to the private stream: nothing else is queued on it
                    t = torch.empty(n, dtype=torch.int64, device=device)
                memcpy_async(t.data_ptr(), self._stage.ptr, 8 * n, "h2d", st.cuda_stream)
                st.synchronize()  # this copy only
            self._cache[key] = t
            return t


_pointer_tables = _PointerTables()


def pointer_table(ptrs: Sequence[int], device: torch.device) -> torch.Tensor:
    """Device int64 array holding `ptrs` (cached by content: see _PointerTables)."""
    return _pointer_tables.get(ptrs, device)


def _layout_struct(dt: torch.dtype, L: int, H: int, D: int, stride_token: int, stride_head: int, base: Optional[int] = None,
                   stride_layer: int = 0, stride_kv: int = 0, plane_ptrs: Optional[int] = None,
                   slot_mapping: Optional[int] = None, block_size: int = 0, stride_block: int = 0,
                   paged_kind: int = PAGED_ROWS) -> KvLayoutStruct:
    """A filled lmc_kv_layout: the planes are addressed from `base` with layer / kv strides or through the device table
    `plane_ptrs`, the tokens directly or (paged) through `slot_mapping` in blocks of `block_size`; `paged_kind`
    PAGED_SPLIT: the blocks are those of vLLM's ROCm paged-attention kernels (include/lmc_hip.h)."""
    s = KvLayoutStruct()
    s.dtype = dtype_code(dt)
    s.num_layers, s.num_heads, s.head_size = L, H, D
    s.base, s.plane_ptrs = base, plane_ptrs
    s.stride_layer, s.stride_kv, s.stride_token, s.stride_head = stride_layer, stride_kv, stride_token, stride_head
    s.slot_mapping, s.block_size, s.stride_block = slot_mapping, block_size, stride_block
    s.paged_kind = paged_kind
    return s


class KVLayout:
    """Python owner of a lmc_kv_layout; keeps the tensors it points into alive."""

    def __init__(self, struct: KvLayoutStruct, keep: Sequence, ntokens: int, device: torch.device):
        self.struct = struct
        self._keep = list(keep)
        self.ntokens = ntokens
        self.device = device

    @property
    def L(self):
        return self.struct.num_layers

    @property
    def H(self):
        return self.struct.num_heads

    @property
    def D(self):
        return self.struct.head_size

    @property
    def dtype(self):
        return self.struct.dtype

    def layers(self, l0: int, nl: int) -> "KVLayout":
        """Layers [l0, l0 + nl) of this layout as a layout of nl layers (the window the C side cuts for the post-op of a
        layer range -- layer_window() in lmc_api.hip is the same arithmetic, and tests/test_gpu_range_post.py holds
        a rotation of this window against the C side's): the plane table is layer-major, so the window is a pointer into
        it, or the base moved by l0 layer strides.  Shares everything this layout keeps alive."""
        if not (0 <= l0 and nl >= 1 and l0 + nl <= self.L):
            raise ValueError(f"layers [{l0}, {l0 + nl}) of a layout of {self.L}")
        s = KvLayoutStruct.from_buffer_copy(self.struct)
        if s.plane_ptrs:
            s.plane_ptrs += 16 * l0  # two 8-byte pointers per layer
        else:
            s.base += l0 * s.stride_layer * elem_bytes(s.dtype)
        s.num_layers = nl
        return KVLayout(s, self._keep, self.ntokens, self.device)

    def vector_readable(self) -> bool:
        """Whether the encoders can read this layout with their 16-byte vectors of 8 channels (the rule of layout_ok in
        lmc_api.hip / include/lmc_hip.h): rows on 16-byte boundaries, strides multiples of 8 elements, and head_size a
        multiple of 8 unless the heads of a token row lie back to back.  The decoders and lmc_copy_kv take any layout.
        A PAGED_SPLIT layout ("NHDB") has no rows at all: lmc_copy_kv reads and writes it, the decoders behind the
        engine's retrieve paths (decode_chunks_layers / _schedule, load_chunks, load_pack) write it, nobody else takes it."""
        s = self.struct
        if s.paged_kind != PAGED_ROWS:
            return False
        if s.head_size % 8:
            if s.stride_head != s.head_size:
                return False
        elif s.stride_head % 8:
            return False
        if s.stride_token % 8 or (s.slot_mapping and s.stride_block % 8):
            return False
        vec = 8 * elem_bytes(s.dtype)  # a vector of 8 channels: 16 bytes, fp8 8
        if s.plane_ptrs:
            return all(x.data_ptr() % vec == 0 for x in self._keep if isinstance(x, torch.Tensor) and x.dtype in _CODES)
        return s.stride_layer % 8 == 0 and s.stride_kv % 8 == 0 and (s.base or 0) % vec == 0

    @staticmethod
    def from_chunk(t: torch.Tensor, fmt: str) -> "KVLayout":
        """A chunk blob: [L,2,T,H,D] for "vllm", [L,2,H,T,D] for "huggingface"
        (cache_engine.py:137-140).  Any strides are fine (permuted views included) as long as
        the head dimension is contiguous; what the ENCODERS read must also be vector_readable()."""
        assert t.is_cuda and t.dim() == 5 and t.shape[1] == 2, f"bad chunk shape {tuple(t.shape)}"
        st = t.stride()
        if fmt == "vllm":
            L, _, T, H, D = t.shape
            stride_token, stride_head = st[2], st[3]
        elif fmt == "huggingface":
            L, _, H, T, D = t.shape
            stride_token, stride_head = st[3], st[2]
        else:
            raise ValueError(f"Invalid format: {fmt}")
        if st[4] != 1:
            raise ValueError("head dimension must be contiguous")
        s = _layout_struct(t.dtype, L, H, D, stride_token, stride_head, base=t.data_ptr(), stride_layer=st[0], stride_kv=st[1])
        return KVLayout(s, [t], T, t.device)

    @staticmethod
    def from_kv_tuple(kv, fmt: str) -> "KVLayout":
        """The KVCache nested tuple handed to LMCacheEngine.store (cache_engine.py:230-236):
        per layer (K, V), each [T,H,D] ("vllm") or [H,T,D] ("huggingface").  No stacking copy:
        the kernels read every plane through a pointer table."""
        k0 = kv[0][0]
        assert k0.is_cuda and k0.dim() == 3
        st = k0.stride()
        if st[2] != 1:
            raise ValueError("head dimension must be contiguous")
        ptrs = []
        keep = []
        for k, v in kv:
            for x in (k, v):
                if x.shape != k0.shape or x.stride() != st or x.dtype != k0.dtype or x.device != k0.device:
                    raise ValueError("all K/V tensors must share shape, strides, dtype and device")
                ptrs.append(x.data_ptr())
                keep.append(x)
        table = _pointer_tables.get(ptrs, k0.device)
        if fmt == "vllm":
            T, H, D = k0.shape
            stride_token, stride_head = st[0], st[1]
        elif fmt == "huggingface":
            H, T, D = k0.shape
            stride_token, stride_head = st[1], st[0]
        else:
            raise ValueError(f"Invalid format: {fmt}")
        s = _layout_struct(k0.dtype, len(kv), H, D, stride_token, stride_head, plane_ptrs=table.data_ptr())
        return KVLayout(s, keep + [table], T, k0.device)

    @staticmethod
    def paged(kv_caches, slot_mapping: torch.Tensor, block_size: int, layout: str = "NBHD") -> "KVLayout":
        """vLLM paged KV: per layer a tensor [2, num_blocks, ...] addressed through slot_mapping
        (LLM_Engine.rst:91-122).  layout "NBHD" = [num_blocks, block_size, H, D] (flash layout),
        "NHBD" = [num_blocks, H, block_size, D] (BASELINE.json north star), "NHDB" = the cache of vLLM's ROCm
        paged-attention kernels (_paged_split below)."""
        if layout == "NHDB":
            return KVLayout._paged_split(kv_caches, slot_mapping, block_size)
        c0 = kv_caches[0]
        assert c0.is_cuda and c0.dim() == 5 and c0.shape[0] == 2
        st = c0.stride()
        ptrs, keep = [], []
        for c in kv_caches:
            if c.shape != c0.shape or c.stride() != st or c.dtype != c0.dtype:
                raise ValueError("all layer caches must share shape, strides and dtype")
            ptrs += [c[0].data_ptr(), c[1].data_ptr()]
            keep.append(c)
        table = _pointer_tables.get(ptrs, c0.device)
        sm = slot_mapping.to(device=c0.device, dtype=torch.int64).contiguous()
        if layout == "NBHD":
            _, _, bs, H, D = c0.shape
            stride_token, stride_head = st[2], st[3]
        elif layout == "NHBD":
            _, _, H, bs, D = c0.shape
            stride_token, stride_head = st[3], st[2]
        else:
            raise ValueError(layout)
        assert bs == block_size and st[4] == 1
        s = _layout_struct(c0.dtype, len(kv_caches), H, D, stride_token, stride_head, plane_ptrs=table.data_ptr(),
                           slot_mapping=sm.data_ptr(), block_size=block_size, stride_block=st[1])
        return KVLayout(s, keep + [table, sm], sm.numel(), c0.device)

    @staticmethod
    def _paged_split(kv_caches, slot_mapping: torch.Tensor, block_size: int) -> "KVLayout":
        """layout "NHDB": the cache that paged_attention_rocm and paged_attention_v1 / v2 read, as
        PagedAttention.split_kv_cache views it.  With x = 16 / element bytes (8 for bf16 / fp16, 16 for fp8), per layer
          - one tensor [2, num_blocks, H, D, block_size]: a copy-free .view of vLLM's [2, num_blocks, block_size * H * D];
            index 1 IS the value cache, index 0 holds the keys in the x-split order of the next form, or
          - the pair (key_cache [num_blocks, H, D / x, block_size, x], value_cache [num_blocks, H, D, block_size]).
        A token's channels are not contiguous there (K: x-element granules block_size * x apart, V: every element
        block_size apart), so the layout is not vector_readable(): the encoders cannot read it.  lmc_copy_kv gathers from and
        scatters into it (k_copy_split.h), and the decoders store into it (k_decode.h, DEC_PAGED_SPLIT) -- all of them but
        decode_chunks, whose callers want a tensor."""
        first = kv_caches[0]
        pair = isinstance(first, (tuple, list))
        v0 = first[1] if pair else first
        if not v0.is_cuda:
            raise ValueError("the paged KV cache must live on the GPU")
        x = 16 // elem_bytes(dtype_code(v0.dtype))  # (a uint8 cache is refused here: pass its fp8 view)
        planes = []  # per layer (K base, V base, H, D, block size, (stride_block, stride_head, inner strides...) of K and of V)
        for c in kv_caches:
            if pair:
                k, v = c
                if k.dim() != 5 or v.dim() != 4:
                    raise ValueError(f"NHDB pair: key_cache [num_blocks, H, D/x, block_size, x] and value_cache [num_blocks, H, D, "
                                     f"block_size] expected, got {tuple(k.shape)} and {tuple(v.shape)}")
                nb, H, D, bs = v.shape
                if tuple(k.shape) != (nb, H, D // x, bs, x) or D % x:
                    raise ValueError(f"NHDB pair: key_cache {tuple(k.shape)} is not [num_blocks, H, D/x, block_size, x] of "
                                     f"value_cache {tuple(v.shape)} with x = {x} (head_size % x must be 0)")
                ks, vs = k.stride(), v.stride()
                dense = ks[2:] == (bs * x, x, 1) and vs[2:] == (bs, 1)
                outer = (ks[0], ks[1]) if (ks[0], ks[1]) == (vs[0], vs[1]) else None
            else:
                if c.dim() != 5 or c.shape[0] != 2:
                    raise ValueError(f"NHDB: a layer cache is [2, num_blocks, H, D, block_size], got {tuple(c.shape)}")
                _, nb, H, D, bs = c.shape
                k, v = c[0], c[1]
                cs = c.stride()
                dense = cs[3:] == (bs, 1)
                outer = (cs[1], cs[2])
            if k.dtype != v0.dtype or v.dtype != v0.dtype or k.device != v0.device or v.device != v0.device:
                raise ValueError("all layer caches must share dtype and device")
            if bs != block_size:
                raise ValueError(f"NHDB: the cache's blocks hold {bs} slots, block_size is {block_size}")
            if D % x:
                raise ValueError(f"NHDB: head_size {D} is no multiple of x = {x} (16 bytes of {v0.dtype}): the key cache "
                                 "splits a head into x-element granules")
            if not dense:
                raise ValueError("NHDB: the inner dimensions of a block's head (D/x, block_size, x for keys; D, block_size "
                                 "for values) must be dense")
            if outer is None:
                raise ValueError("NHDB pair: key_cache and value_cache must share their block and head strides")
            planes.append((k, v, H, D, outer))
        _, _, H, D, (stride_block, stride_head) = planes[0]
        if any(pl[2:] != planes[0][2:] for pl in planes):
            raise ValueError("all layer caches must share shape and strides")
        ptrs, keep = [], []
        for k, v, *_ in planes:
            ptrs += [k.data_ptr(), v.data_ptr()]
            keep += [k, v]
        table = _pointer_tables.get(ptrs, v0.device)
        sm = slot_mapping.to(device=v0.device, dtype=torch.int64).contiguous()
        s = _layout_struct(v0.dtype, len(planes), H, D, 0, stride_head, plane_ptrs=table.data_ptr(), slot_mapping=sm.data_ptr(),
                           block_size=block_size, stride_block=stride_block, paged_kind=PAGED_SPLIT)
        return KVLayout(s, keep + [table, sm], sm.numel(), v0.device)


class RangePost:
    """Python owner of what becomes one lmc_range_post per decode job: a rotation as Context.rope_shift takes it and / or
    the LMC_PAGED_SPLIT cache the decode destination (then a staged chunk of rows) is scattered into.  Written in the
    decode destination's tokens: deltas[t] belongs to destination token t, and destination token t goes to token
    scatter_tok0 + t of scatter_dst.  A rotation whose scatter_dst is the (PAGED_SPLIT) decode destination ITSELF, with
    scatter_tok0 0, is the in-place form: the decoder wrote the split blocks and the keys are rotated there
    (lmc_rope_shift_split), nothing is copied.  Keeps the tensors the kernels read alive."""

    def __init__(self, cos_sin: Optional[torch.Tensor] = None, rot_dim: int = 0, is_neox: bool = True, delta: int = 0,
                 deltas: Optional[torch.Tensor] = None, scatter_dst: Optional["KVLayout"] = None, scatter_tok0: int = 0):
        if cos_sin is not None:
            Context._check_rope_args(cos_sin, rot_dim, deltas, None)
        self.cos_sin, self.rot_dim, self.is_neox, self.delta, self.deltas = cos_sin, int(rot_dim), bool(is_neox), int(delta), deltas
        self.scatter_dst, self.scatter_tok0 = scatter_dst, int(scatter_tok0)

    @staticmethod
    def window(dst: "KVLayout", dst_tok0: int, nchunks: int, chunk_tokens: int) -> Tuple[int, int]:
        """(first token, tokens) of `dst` that a decode job of nchunks chunks from dst_tok0 on fills: tokens below 0 are
        dropped, and the last chunk ends with the destination."""
        t0 = max(0, dst_tok0)
        return t0, min(dst.ntokens, dst_tok0 + nchunks * chunk_tokens) - t0

    def in_place(self, dst: "KVLayout") -> bool:
        """Whether this post rotates a PAGED_SPLIT `dst` where it lies: a rotation whose scatter target is `dst` itself
        (the same cache, every field of the two lmc_kv_layout equal, token for token)."""
        s = self.scatter_dst
        return (self.cos_sin is not None and s is not None and self.scatter_tok0 == 0
                and dst.struct.paged_kind == PAGED_SPLIT and (s is dst or bytes(s.struct) == bytes(dst.struct)))

    def struct(self, tok_begin: int, ntok: int) -> RangePostStruct:
        """The lmc_range_post of the job that fills destination tokens [tok_begin, +ntok): filled per call, nothing kept."""
        p = RangePostStruct()
        if self.cos_sin is not None:
            p.cos_sin, p.table_rows, p.rot_dim = self.cos_sin.data_ptr(), self.cos_sin.shape[0], self.rot_dim
            p.is_neox, p.delta = 1 if self.is_neox else 0, self.delta
            if self.deltas is not None:
                p.deltas = self.deltas.data_ptr() + 4 * tok_begin
        p.tok_begin, p.ntok = tok_begin, ntok
        if self.scatter_dst is not None:
            p.scatter_dst = ctypes.pointer(self.scatter_dst.struct)
            p.scatter_tok0 = self.scatter_tok0 + tok_begin
        return p

    def apply(self, ctx: "Context", dst: "KVLayout", tok_begin: int, ntok: int) -> None:
        """The same work from Python, for ALL layers of destination tokens [tok_begin, +ntok), on the current stream:
        lmc_rope_shift on the rows, then lmc_copy_kv into scatter_dst.  For retrieve_into_paged, and for the tiers whose
        decode is not cut by the C side.  A PAGED_SPLIT `dst` that the post names as its own scatter target (the in-place
        form of lmc_range_post) was filled where it is: lmc_rope_shift_split there, and nothing is copied."""
        if self.in_place(dst):
            ctx.rope_shift_split(dst, tok_begin, ntok, self.cos_sin, self.rot_dim, self.is_neox, delta=self.delta,
                                 deltas=None if self.deltas is None else self.deltas[tok_begin:tok_begin + ntok])
            return
        if self.cos_sin is not None:
            ctx.rope_shift(dst, tok_begin, ntok, self.cos_sin, self.rot_dim, self.is_neox, delta=self.delta,
                           deltas=None if self.deltas is None else self.deltas[tok_begin:tok_begin + ntok])
        if self.scatter_dst is not None:
            ctx.copy_kv(dst, tok_begin, ntok, self.scatter_dst, self.scatter_tok0 + tok_begin)


class PinnedBuffer:
    """hipHostMalloc'ed host memory (lmc_pinned_alloc) exposed as a uint8 torch tensor view."""

    def __init__(self, nbytes: int):
        p = ctypes.c_void_p()
        check(lib().lmc_pinned_alloc(nbytes, ctypes.byref(p)), "lmc_pinned_alloc")
        self.ptr = p.value
        self.nbytes = nbytes
        self._arr = (ctypes.c_uint8 * nbytes).from_address(self.ptr)
        self.tensor = torch.frombuffer(self._arr, dtype=torch.uint8)

    def free(self):
        if self.ptr:
            self.tensor = None
            self._arr = None
            lib().lmc_pinned_free(ctypes.c_void_p(self.ptr))
            self.ptr = 0

    def __del__(self):
        # at interpreter shutdown the HIP runtime may already be gone: leave the pages to the OS then
        try:
            if not sys.is_finalizing():
                self.free()
        except Exception:
            pass


class NativeEvent:
    """A hipEvent_t of the C ABI (lmc_event_*): what lmc_load_chunks records behind every range of layers.  Has the
    two methods the Python side needs of an event: synchronize() (host) and wait(stream) (stream-side)."""

    def __init__(self, timing: bool = False):
        h = ctypes.c_void_p()
        check(lib().lmc_event_create(ctypes.byref(h), 1 if timing else 0), "lmc_event_create")
        self.handle = h

    def synchronize(self) -> None:
        check(lib().lmc_event_synchronize(self.handle), "lmc_event_synchronize")

    def wait(self, stream_ptr: int) -> None:
        check(lib().lmc_stream_wait_event(stream_ptr, self.handle), "lmc_stream_wait_event")

    def query(self) -> bool:
        return lib().lmc_event_query(self.handle) == 1

    def __del__(self):
        try:
            if self.handle and not sys.is_finalizing():
                lib().lmc_event_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


class Context:
    """Owner of one lmc_ctx (per device).  Thread-safe: the C side serialises workspace use."""

    def __init__(self, device: Optional[int] = None):
        if not torch.cuda.is_available():
            raise NativeError("lmcache_amd needs an MI355X (torch.cuda.is_available() is False); no CPU fallback")
        self.device = torch.cuda.current_device() if device is None else int(device)
        h = ctypes.c_void_p()
        check(lib().lmc_ctx_create(self.device, ctypes.byref(h)), "lmc_ctx_create")
        self.handle = h

    def close(self):
        if self.handle:
            lib().lmc_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            if not sys.is_finalizing():
                self.close()
        except Exception:
            pass

    def status(self, clear: bool = False) -> int:
        return lib().lmc_device_status(self.handle, 1 if clear else 0)

    def raise_on_status(self, what: str):
        st = self.status(clear=True)
        if st:
            raise NativeError(f"{what}: {describe_status(st)}")

    def set_encode_path(self, path: str) -> None:
        """Which kernels encode_chunks launches: "auto" (default), "two_kernels" (k_quantize + k_cdf_encode) or
        "fused" (k_encode_fused: whole 256-token chunks of any plane width).  Blobs are byte-identical either way (include/lmc_hip.h)."""
        check(lib().lmc_ctx_set_encode_path(self.handle, ENCODE_PATHS[path]), "lmc_ctx_set_encode_path")

    def profile(self, enable: bool) -> None:
        check(lib().lmc_ctx_profile(self.handle, 1 if enable else 0), "lmc_ctx_profile")

    def profile_read(self):
        """Per-kernel ms of the last profiled call (caller must have synchronised the stream)."""
        buf = (ctypes.c_float * 8)()
        n = lib().lmc_ctx_profile_read(self.handle, buf, 8)
        if n < 0:
            check(n, "lmc_ctx_profile_read")
        return [float(buf[i]) for i in range(n)]

    def reserve(self, L, H, D, chunk_tokens, max_chunks):
        check(lib().lmc_ctx_reserve(self.handle, L, H, D, chunk_tokens, max_chunks), "lmc_ctx_reserve")

    @staticmethod
    def _bins(bins: Sequence[int]):
        arr = (ctypes.c_int32 * len(bins))(*[int(b) for b in bins])
        return arr

    def _call(self, name: str, device, stream: Optional[int], *args) -> None:
        """The C-ABI call `name`(ctx, *args, stream), checked; stream None: the current stream of `device`."""
        st = current_stream_ptr(device) if stream is None else stream
        check(getattr(lib(), name)(self.handle, *args, st), name)

    @staticmethod
    def _nchunks(tok_begin: int, tok_end: int, chunk_tokens: int) -> int:
        return (tok_end - tok_begin + chunk_tokens - 1) // chunk_tokens

    def quantize(self, src: KVLayout, tok_begin: int, ntok: int, bins, stream: Optional[int] = None
                 ) -> Tuple[torch.Tensor, torch.Tensor]:
        P, C = 2 * src.L, src.H * src.D
        sym = torch.empty((P, ntok, C), dtype=torch.int8, device=src.device)
        scale = torch.empty((P, ntok), dtype=torch.int16, device=src.device)
        self._call("lmc_quantize", src.device, stream, ctypes.byref(src.struct), tok_begin, ntok, self._bins(bins),
                   sym.data_ptr(), scale.data_ptr())
        return sym, scale

    def calculate_cdf(self, sym: torch.Tensor, max_bins: int = MAX_BINS, stream: Optional[int] = None) -> torch.Tensor:
        assert sym.is_cuda and sym.dtype == torch.int8 and sym.is_contiguous() and sym.dim() == 3
        P, T, C = sym.shape
        out = torch.empty((P, C, max_bins + 1), dtype=torch.int16, device=sym.device)
        self._call("lmc_calculate_cdf", sym.device, stream, sym.data_ptr(), P, T, C, max_bins, out.data_ptr())
        return out

    def _encode_job(self, symbol: str, src, tok_begin: int, tok_end: int, chunk_tokens: int, bins, blobs_ptr: int,
                    blob_stride: int, sizes_ptr: int, stream: Optional[int], status_ptr: Optional[int], device=None) -> int:
        """The marshalling of the lmc_encode_chunks* exports and lmc_store_pack (one argument list) -> the job's chunks.
        `src`: the KVLayout the job reads; or, for lmc_transcode_fixed, which reads blobs instead, the tuple of its own
        leading arguments (with `device`) -- behind the source the argument list is the same."""
        if isinstance(src, KVLayout):
            head, device = (ctypes.byref(src.struct), tok_begin, tok_end, chunk_tokens), src.device
        else:
            head = tuple(src)
        self._call(symbol, device, stream, *head, self._bins(bins), blobs_ptr, blob_stride, sizes_ptr, status_ptr)
        return self._nchunks(tok_begin, tok_end, chunk_tokens)

    def encode_chunks(self, src: KVLayout, tok_begin: int, tok_end: int, chunk_tokens: int, bins,
                      blobs_ptr: int, blob_stride: int, sizes_ptr: int, stream: Optional[int] = None,
                      status_ptr: Optional[int] = None) -> int:
        """status_ptr: device-accessible uint32 (pinned host) that receives THIS job's LMC_STATUS_* bits
        (None: the context's sticky word)."""
        return self._encode_job("lmc_encode_chunks", src, tok_begin, tok_end, chunk_tokens, bins, blobs_ptr, blob_stride,
                                sizes_ptr, stream, status_ptr)

    def encode_chunks_split(self, src: KVLayout, tok_begin: int, tok_end: int, chunk_tokens: int, bins,
                            blobs_ptr: int, blob_stride: int, sizes_ptr: int, stream: Optional[int] = None,
                            status_ptr: Optional[int] = None) -> int:
        """encode_chunks for any source it takes and a PAGED_SPLIT ("NHDB") one, read in place (lmc_encode_chunks_split)."""
        return self._encode_job("lmc_encode_chunks_split", src, tok_begin, tok_end, chunk_tokens, bins, blobs_ptr, blob_stride,
                                sizes_ptr, stream, status_ptr)

    def encode_chunks_fixed(self, src: KVLayout, tok_begin: int, tok_end: int, chunk_tokens: int, bins,
                            blobs_ptr: int, blob_stride: int, sizes_ptr: int, stream: Optional[int] = None,
                            status_ptr: Optional[int] = None) -> int:
        """encode_chunks with the blobs in the fixed-width model (lmc_encode_chunks_fixed): sizes are fixed_blob_bytes."""
        return self._encode_job("lmc_encode_chunks_fixed", src, tok_begin, tok_end, chunk_tokens, bins, blobs_ptr, blob_stride,
                                sizes_ptr, stream, status_ptr)

    def encode_chunks_fixed_split(self, src: KVLayout, tok_begin: int, tok_end: int, chunk_tokens: int, bins,
                                  blobs_ptr: int, blob_stride: int, sizes_ptr: int, stream: Optional[int] = None,
                                  status_ptr: Optional[int] = None) -> int:
        """encode_chunks_fixed for any source it takes and a 16-bit PAGED_SPLIT ("NHDB") one of up to 1024 channels per
        plane, read in place (lmc_encode_chunks_fixed_split)."""
        return self._encode_job("lmc_encode_chunks_fixed_split", src, tok_begin, tok_end, chunk_tokens, bins, blobs_ptr,
                                blob_stride, sizes_ptr, stream, status_ptr)

    def encode_layers_begin(self, src: KVLayout, tok_begin: int, tok_end: int, chunk_tokens: int, bins,
                            blobs_ptr: int, blob_stride: int, sizes_ptr: int, status_ptr: Optional[int] = None
                            ) -> Optional["LayerEncodeHandle"]:
        """lmc_encode_layers_begin: the layer-wise form of encode_chunks_split -> the job's handle, or None when the job
        is not eligible (LMC_NOT_LAYERWISE: the caller encodes in one piece).  `src` is kept alive by the handle."""
        h = ctypes.c_void_p()
        return self._layers_begin("lmc_encode_layers_begin", src, tok_begin, tok_end, chunk_tokens, bins, blobs_ptr, blob_stride,
                                  sizes_ptr, status_ptr)

    def encode_layers_begin_fixed(self, src: KVLayout, tok_begin: int, tok_end: int, chunk_tokens: int, bins,
                                  blobs_ptr: int, blob_stride: int, sizes_ptr: int, status_ptr: Optional[int] = None
                                  ) -> Optional["LayerEncodeHandle"]:
        """lmc_encode_layers_begin_fixed: the layer-wise form of encode_chunks_fixed_split -> the same handle as
        encode_layers_begin's, or None for planes of more than 1024 channels."""
        return self._layers_begin("lmc_encode_layers_begin_fixed", src, tok_begin, tok_end, chunk_tokens, bins, blobs_ptr,
                                  blob_stride, sizes_ptr, status_ptr)

    def _layers_begin(self, symbol: str, src: KVLayout, tok_begin: int, tok_end: int, chunk_tokens: int, bins,
                      blobs_ptr: int, blob_stride: int, sizes_ptr: int, status_ptr: Optional[int]) -> Optional["LayerEncodeHandle"]:
        h = ctypes.c_void_p()
        rc = getattr(lib(), symbol)(self.handle, ctypes.byref(src.struct), tok_begin, tok_end, chunk_tokens,
                                    self._bins(bins), blobs_ptr, blob_stride, sizes_ptr, status_ptr, ctypes.byref(h))
        if rc == NOT_LAYERWISE:
            return None
        check(rc, symbol)
        return LayerEncodeHandle(self, h, src)

    def set_fixed_layer_slices(self, n: int) -> None:
        """lmc_ctx_set_fixed_layer_slices: slices per plane of a chunk in the layer launches of the fixed-width layer-wise
        jobs begun from now on; 0: the library's own rule.  Blobs do not depend on it."""
        check(lib().lmc_ctx_set_fixed_layer_slices(self.handle, int(n)), "lmc_ctx_set_fixed_layer_slices")

    def decode_chunks(self, blobs_ptr: int, blob_stride: int, nchunks: int, dst: KVLayout, dst_tok0: int,
                      chunk_tokens: int, stream: Optional[int] = None, status_ptr: Optional[int] = None) -> None:
        self._call("lmc_decode_chunks", dst.device, stream, blobs_ptr, blob_stride, nchunks, ctypes.byref(dst.struct),
                   dst_tok0, chunk_tokens, status_ptr)

    def decode_chunks_layers(self, blob_ptrs: int, max_blob_bytes: int, nchunks: int, dst: KVLayout, dst_tok0: int,
                             chunk_tokens: int, layer_begin: int, layer_count: int, stream: Optional[int] = None,
                             status_ptr: Optional[int] = None) -> None:
        """Decode layers [layer_begin, +layer_count) of blobs addressed through a device pointer table."""
        self._call("lmc_decode_chunks_layers", dst.device, stream, blob_ptrs, max_blob_bytes, nchunks,
                   ctypes.byref(dst.struct), dst_tok0, chunk_tokens, layer_begin, layer_count, status_ptr)

    def _call_post(self, symbol: str, device, stream: Optional[int], status_ptr: Optional[int], post, *args) -> None:
        """_call for the symbols that end in status, stream and -- some -- a post pointer, in the order `symbol` declares them."""
        tail = [status_ptr, current_stream_ptr(device) if stream is None else stream]
        if symbol in _POST_SLOT:
            tail.insert(_POST_SLOT[symbol], None if post is None else ctypes.byref(post))
        else:
            assert post is None, f"{symbol} takes no lmc_range_post"
        check(getattr(lib(), symbol)(self.handle, *args, *tail), symbol)

    def _schedule(self, symbol: str, blob_ptrs: int, max_blob_bytes: int, nchunks: int, dst: KVLayout, dst_tok0: int,
                  chunk_tokens: int, layer_ends, events, post, stream: Optional[int], status_ptr: Optional[int]) -> None:
        """The marshalling of the lmc_decode_chunks*_schedule* exports; layer_ends / events as decode_chunks_schedule.
        `post`: the struct the symbol takes in its slot -- a RangePostStruct, or the head-window calls' HeadWindowStruct."""
        n = len(layer_ends)
        ends = layer_ends if isinstance(layer_ends, ctypes.Array) else (ctypes.c_int32 * n)(*layer_ends)
        evs = events if events is None or isinstance(events, ctypes.Array) else (ctypes.c_void_p * n)(*[e.handle for e in events])
        self._call_post(symbol, dst.device, stream, status_ptr, post, blob_ptrs, max_blob_bytes, nchunks,
                        ctypes.byref(dst.struct), dst_tok0, chunk_tokens, n, ends, evs)

    def decode_chunks_schedule(self, blob_ptrs: int, max_blob_bytes: int, nchunks: int, dst: KVLayout, dst_tok0: int,
                               chunk_tokens: int, layer_ends, events, stream: Optional[int] = None,
                               status_ptr: Optional[int] = None) -> None:
        """lmc_decode_chunks_schedule: one launch per range of layers [layer_ends[i - 1], layer_ends[i]) and one event
        record behind each (events: NativeEvent objects), in ONE call.  layer_ends / events may be prebuilt ctypes arrays
        (a cached retrieval plan passes the same ones every time)."""
        self._schedule("lmc_decode_chunks_schedule", blob_ptrs, max_blob_bytes, nchunks, dst, dst_tok0, chunk_tokens,
                       layer_ends, events, None, stream, status_ptr)

    def decode_chunks_schedule_post(self, blob_ptrs: int, max_blob_bytes: int, nchunks: int, dst: KVLayout, dst_tok0: int,
                                    chunk_tokens: int, layer_ends, events, post: Optional[RangePostStruct],
                                    stream: Optional[int] = None, status_ptr: Optional[int] = None) -> None:
        """lmc_decode_chunks_schedule_post: decode_chunks_schedule with `post` (RangePost.struct) done to every range
        between its launch and its event, still ONE call.  post None is decode_chunks_schedule."""
        self._schedule("lmc_decode_chunks_schedule_post", blob_ptrs, max_blob_bytes, nchunks, dst, dst_tok0, chunk_tokens,
                       layer_ends, events, post, stream, status_ptr)

    def decode_chunks_fixed_schedule(self, blob_ptrs: int, max_blob_bytes: int, nchunks: int, dst: KVLayout, dst_tok0: int,
                                     chunk_tokens: int, layer_ends, events, post: Optional[RangePostStruct] = None,
                                     stream: Optional[int] = None, status_ptr: Optional[int] = None) -> None:
        """lmc_decode_chunks_fixed_schedule: decode_chunks_schedule_post for LMC_MODEL_FIXED blobs (post None: no post-op)."""
        self._schedule("lmc_decode_chunks_fixed_schedule", blob_ptrs, max_blob_bytes, nchunks, dst, dst_tok0, chunk_tokens,
                       layer_ends, events, post, stream, status_ptr)

    def decode_chunks_fixed_split_schedule(self, blob_ptrs: int, max_blob_bytes: int, nchunks: int, dst: KVLayout,
                                           dst_tok0: int, chunk_tokens: int, layer_ends, events,
                                           post: Optional[RangePostStruct] = None, stream: Optional[int] = None,
                                           status_ptr: Optional[int] = None) -> None:
        """lmc_decode_chunks_fixed_split_schedule: decode_chunks_fixed_schedule for any destination it takes and a 16-bit
        PAGED_SPLIT ("NHDB") one, stored into in place."""
        self._schedule("lmc_decode_chunks_fixed_split_schedule", blob_ptrs, max_blob_bytes, nchunks, dst, dst_tok0,
                       chunk_tokens, layer_ends, events, post, stream, status_ptr)

    def decode_chunks_heads_schedule(self, blob_ptrs: int, max_blob_bytes: int, nchunks: int, dst: KVLayout, dst_tok0: int,
                                     chunk_tokens: int, layer_ends, events, heads: HeadWindow, stream: Optional[int] = None,
                                     status_ptr: Optional[int] = None) -> None:
        """lmc_decode_chunks_heads_schedule: decode_chunks_schedule of a window of heads of blobs that have heads.src_heads
        heads, into heads [heads.dst_head_begin, ...) of `dst` (its own head count).  No post: see include/lmc_hip.h."""
        self._schedule("lmc_decode_chunks_heads_schedule", blob_ptrs, max_blob_bytes, nchunks, dst, dst_tok0, chunk_tokens,
                       layer_ends, events, None if heads is None else HeadWindow(*heads).struct(), stream, status_ptr)

    def decode_chunks_fixed_heads_schedule(self, blob_ptrs: int, max_blob_bytes: int, nchunks: int, dst: KVLayout,
                                           dst_tok0: int, chunk_tokens: int, layer_ends, events, heads: HeadWindow,
                                           stream: Optional[int] = None, status_ptr: Optional[int] = None) -> None:
        """lmc_decode_chunks_fixed_heads_schedule: the same for LMC_MODEL_FIXED blobs (rows or a 16-bit PAGED_SPLIT cache)."""
        self._schedule("lmc_decode_chunks_fixed_heads_schedule", blob_ptrs, max_blob_bytes, nchunks, dst, dst_tok0,
                       chunk_tokens, layer_ends, events, None if heads is None else HeadWindow(*heads).struct(), stream,
                       status_ptr)

    def store_chunks(self, src: KVLayout, tok_begin: int, tok_end: int, chunk_tokens: int, bins, host_arena_ptr: int,
                     host_cap: int, offsets_ptr: int, sizes_ptr: int, stream: Optional[int] = None,
                     status_ptr: Optional[int] = None) -> int:
        """lmc_store_chunks: encode + exact-size copies into a pinned arena, no host wait.  offsets_ptr / sizes_ptr:
        pinned uint64 [n + 1] / uint32 [n], valid once `stream` has completed."""
        self._call("lmc_store_chunks", src.device, stream, ctypes.byref(src.struct), tok_begin, tok_end, chunk_tokens,
                   self._bins(bins), host_arena_ptr, host_cap, offsets_ptr, sizes_ptr, status_ptr)
        return self._nchunks(tok_begin, tok_end, chunk_tokens)

    def load_chunks(self, host_ptrs_ptr: int, sizes_ptr: int, nchunks: int, dst: KVLayout, dst_tok0: int,
                    chunk_tokens: int, layers_per_range: int = 0, range_events_ptr: Optional[int] = None,
                    stream: Optional[int] = None, status_ptr: Optional[int] = None) -> None:
        """lmc_load_chunks: blobs in pinned host memory -> decoded KV, gathered and decoded layer range by layer range."""
        self._call("lmc_load_chunks", dst.device, stream, host_ptrs_ptr, sizes_ptr, nchunks, ctypes.byref(dst.struct),
                   dst_tok0, chunk_tokens, layers_per_range, range_events_ptr, status_ptr)

    def store_pack(self, src: KVLayout, tok_begin: int, tok_end: int, chunk_tokens: int, bins, pack_ptr: int, pack_cap: int,
                   sizes_ptr: int, stream: Optional[int] = None, status_ptr: Optional[int] = None) -> int:
        """lmc_store_pack: encode + the job's blobs transposed plane-major into one region, no host wait."""
        return self._encode_job("lmc_store_pack", src, tok_begin, tok_end, chunk_tokens, bins, pack_ptr, pack_cap, sizes_ptr,
                                stream, status_ptr)

    def store_pack_parts(self, src: KVLayout, tok_begin: int, tok_end: int, chunk_tokens: int, bins, pack_ptr: int,
                         pack_cap: int, sizes_ptr: int, nparts: int, part_info_ptr: int, part_events,
                         stream: Optional[int] = None, status_ptr: Optional[int] = None) -> int:
        """lmc_store_pack_parts: the encode in `nparts` plane ranges, each packed into the DEVICE region at pack_ptr as soon
        as it is coded; part_info_ptr: pinned uint64 [2 nparts] ({offset in the streams region, bytes} per part);
        part_events: NativeEvent per part (recorded behind the part's pack kernels)."""
        evs = None if part_events is None else (ctypes.c_void_p * nparts)(*[e.handle for e in part_events])
        self._call("lmc_store_pack_parts", src.device, stream, ctypes.byref(src.struct), tok_begin, tok_end, chunk_tokens,
                   self._bins(bins), pack_ptr, pack_cap, sizes_ptr, nparts, part_info_ptr, evs, status_ptr)
        return self._nchunks(tok_begin, tok_end, chunk_tokens)

    def load_pack(self, pack_ptr: int, pack_bytes: int, chunk_begin: int, nchunks: int, dst: KVLayout, dst_tok0: int,
                  layers_per_range: int = 0, range_events_ptr: Optional[int] = None, stream: Optional[int] = None,
                  status_ptr: Optional[int] = None) -> None:
        """lmc_load_pack: chunks [chunk_begin, chunk_begin + nchunks) (nchunks 0 = all that follow) of a pack in pinned
        host memory -> decoded KV, one transfer and one decode per range of layers."""
        self._call_post("lmc_load_pack", dst.device, stream, status_ptr, None, pack_ptr, pack_bytes, chunk_begin, nchunks,
                        ctypes.byref(dst.struct), dst_tok0, layers_per_range, range_events_ptr)

    def load_pack_post(self, pack_ptr: int, pack_bytes: int, chunk_begin: int, nchunks: int, dst: KVLayout, dst_tok0: int,
                       layers_per_range: int, range_events_ptr: Optional[int], post: Optional[RangePostStruct],
                       stream: Optional[int] = None, status_ptr: Optional[int] = None) -> None:
        """lmc_load_pack_post: load_pack with `post` (RangePost.struct) done to every range between its decode and its event."""
        self._call_post("lmc_load_pack_post", dst.device, stream, status_ptr, post, pack_ptr, pack_bytes, chunk_begin, nchunks,
                        ctypes.byref(dst.struct), dst_tok0, layers_per_range, range_events_ptr)

    def pack_blobs(self, blob_ptrs: int, blob_bytes_ptr: int, nchunks: int, L: int, H: int, D: int, chunk_tokens: int,
                   ntokens: int, pack_ptr: int, pack_cap: int, device, stream: Optional[int] = None,
                   status_ptr: Optional[int] = None) -> None:
        """lmc_pack_blobs: nchunks encoded blobs anywhere in device memory (blob_ptrs: device int64 [n]; blob_bytes_ptr:
        device-accessible uint32 [n], the room of each) -> one pack in the DEVICE region at pack_ptr.  No encode."""
        self._call("lmc_pack_blobs", device, stream, blob_ptrs, blob_bytes_ptr, nchunks, L, H, D, chunk_tokens, ntokens,
                   pack_ptr, pack_cap, status_ptr)

    def transcode_fixed(self, blob_ptrs: int, blob_bytes_ptr: int, nchunks: int, L: int, H: int, D: int, dtype: int,
                        chunk_tokens: int, ntokens: int, bins, blobs_ptr: int, blob_stride: int, sizes_ptr: int, device,
                        stream: Optional[int] = None, status_ptr: Optional[int] = None) -> int:
        """lmc_transcode_fixed: nchunks fixed-width blobs anywhere in device memory (blob_ptrs: device int64 [n];
        blob_bytes_ptr: device-accessible uint32 [n], the room of each) -> the blobs encode_chunks would have written from
        the same KV, at blobs_ptr + i * blob_stride, sizes at sizes_ptr.  `dtype`: dtype_code of the stored KV."""
        n = self._encode_job("lmc_transcode_fixed", (blob_ptrs, blob_bytes_ptr, nchunks, L, H, D, dtype, chunk_tokens, ntokens),
                             0, ntokens, chunk_tokens, bins, blobs_ptr, blob_stride, sizes_ptr, stream, status_ptr, device=device)
        assert n == nchunks, "ntokens does not make nchunks chunks"
        return n

    def transcode_to_fixed(self, blob_ptrs: int, blob_bytes_ptr: int, nchunks: int, L: int, H: int, D: int, dtype: int,
                           chunk_tokens: int, ntokens: int, bins, out_ptrs: int, out_bytes_ptr: int, device,
                           stream: Optional[int] = None, status_ptr: Optional[int] = None) -> int:
        """lmc_transcode_to_fixed, transcode_fixed's inverse: nchunks entropy-coded blobs anywhere in device memory
        (blob_ptrs: device int64 [n]; blob_bytes_ptr: device-accessible uint32 [n], the room of each) -> the blobs
        encode_chunks_fixed would have written from the same KV, chunk i at the device address out_ptrs[i] (device int64
        [n]; out_bytes_ptr: device-accessible uint32 [n], the room there, at least fixed_blob_bytes of the chunk's length).
        One launch, no workspace.  `dtype`: dtype_code of the stored KV."""
        assert self._nchunks(0, ntokens, chunk_tokens) == nchunks, "ntokens does not make nchunks chunks"
        self._call("lmc_transcode_to_fixed", device, stream, blob_ptrs, blob_bytes_ptr, nchunks, L, H, D, dtype, chunk_tokens,
                   ntokens, self._bins(bins), out_ptrs, out_bytes_ptr, status_ptr)
        return nchunks

    def unpack_blobs(self, pack_ptr: int, pack_bytes: int, chunk_begin: int, nchunks: int, dst_ptrs: Sequence[int],
                     dst_caps: Sequence[int], device, stream: Optional[int] = None, status_ptr: Optional[int] = None) -> None:
        """lmc_unpack_blobs: chunks [chunk_begin, +nchunks) of a pack in pinned host memory -> the blobs they were made
        of, chunk chunk_begin + i at device address dst_ptrs[i] (dst_caps[i] bytes of room)."""
        ptrs = (ctypes.c_void_p * nchunks)(*[int(p) for p in dst_ptrs])
        caps = (ctypes.c_uint32 * nchunks)(*[int(c) for c in dst_caps])
        self._call("lmc_unpack_blobs", device, stream, pack_ptr, pack_bytes, chunk_begin, nchunks, ptrs, caps, status_ptr)

    def decode_symbols(self, blob: torch.Tensor, L: int, H: int, D: int, T: int, stream: Optional[int] = None
                       ) -> torch.Tensor:
        sym = torch.empty((2 * L, T, H * D), dtype=torch.int8, device=blob.device)
        self._call("lmc_decode_symbols", blob.device, stream, blob.data_ptr(), L, H, D, sym.data_ptr())
        return sym

    def copy_kv(self, src: KVLayout, tok_begin: int, ntok: int, dst: KVLayout, dst_tok0: int,
                stream: Optional[int] = None) -> None:
        self._call("lmc_copy_kv", src.device, stream, ctypes.byref(src.struct), tok_begin, ntok, ctypes.byref(dst.struct),
                   dst_tok0)


    def rope_shift(self, layout: KVLayout, tok_begin: int, ntok: int, cos_sin: torch.Tensor, rot_dim: int,
                   is_neox: bool = True, delta: int = 0, deltas: Optional[torch.Tensor] = None,
                   job_status: Optional[int] = None, stream: Optional[int] = None) -> None:
        """lmc_rope_shift: the keys of tokens [tok_begin, +ntok) of `layout` re-rotated in place by `delta` positions (or
        by deltas[i] for token tok_begin + i: device int32 [ntok]).  cos_sin: device fp32 [table_rows, rot_dim], the
        model's cos_sin_cache (lmcache_amd.rope.RopeShift builds or widens one).  job_status: pinned word that receives
        LMC_STATUS_BAD_POSITION for a per-token delta outside the table (None: the context's sticky word)."""
        self._check_rope_args(cos_sin, rot_dim, deltas, ntok)
        self._call("lmc_rope_shift", layout.device, stream, ctypes.byref(layout.struct), tok_begin, ntok, cos_sin.data_ptr(),
                   cos_sin.shape[0], rot_dim, 1 if is_neox else 0, int(delta), None if deltas is None else deltas.data_ptr(),
                   job_status)

    def rope_shift_split(self, layout: KVLayout, tok_begin: int, ntok: int, cos_sin: torch.Tensor, rot_dim: int,
                         is_neox: bool = True, delta: int = 0, deltas: Optional[torch.Tensor] = None,
                         job_status: Optional[int] = None, stream: Optional[int] = None) -> None:
        """lmc_rope_shift_split: rope_shift for a PAGED_SPLIT ("NHDB") layout of bf16 / fp16 -- the keys are re-rotated in
        the split blocks themselves, behind a decode that stored into them directly.  Arguments as rope_shift's; a rows
        layout is refused here (NativeError) as a split one is there."""
        self._check_rope_args(cos_sin, rot_dim, deltas, ntok)
        self._call("lmc_rope_shift_split", layout.device, stream, ctypes.byref(layout.struct), tok_begin, ntok,
                   cos_sin.data_ptr(), cos_sin.shape[0], rot_dim, 1 if is_neox else 0, int(delta),
                   None if deltas is None else deltas.data_ptr(), job_status)

    def kv_deviation(self, a: KVLayout, a_layer: int, a_tok0: int, b: KVLayout, b_layer: int, b_tok0: int, ntok: int,
                     dev_k: Optional[torch.Tensor] = None, dev_v: Optional[torch.Tensor] = None,
                     stream: Optional[int] = None) -> None:
        """lmc_kv_deviation: dev_k[i] / dev_v[i] = the squared distance, summed over heads and channels in fp32, between
        the K / V of token a_tok0 + i of layer a_layer of `a` and token b_tok0 + i of layer b_layer of `b`.  dev_k, dev_v:
        contiguous device float32 tensors of at least ntok entries; either may be None (that plane is skipped)."""
        for name, t in (("dev_k", dev_k), ("dev_v", dev_v)):
            if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() >= ntok):
                raise ValueError(f"{name} must be a contiguous device float32 tensor of at least ntok = {ntok} entries")
        self._call("lmc_kv_deviation", a.device, stream, ctypes.byref(a.struct), a_layer, a_tok0, ctypes.byref(b.struct), b_layer,
                   b_tok0, ntok, None if dev_k is None else dev_k.data_ptr(), None if dev_v is None else dev_v.data_ptr())

    def select_topk(self, dev: torch.Tensor, k: int, idx_out: torch.Tensor, stream: Optional[int] = None) -> int:
        """lmc_select_topk: the min(k, n) entries of `dev` (device float32 [n]) with the largest magnitude bits, NaN above
        +inf, ties to the lower index -> their indices in ascending order in idx_out (device int32, at least min(k, n)
        entries).  Returns min(k, n); nothing is read back."""
        n = dev.numel()
        kk = min(int(k), n)
        if not (dev.is_cuda and dev.dtype == torch.float32 and dev.is_contiguous()):
            raise ValueError("dev must be a contiguous device float32 tensor")
        if not (idx_out.is_cuda and idx_out.dtype == torch.int32 and idx_out.is_contiguous() and idx_out.numel() >= max(kk, 0)):
            raise ValueError(f"idx_out must be a contiguous device int32 tensor of at least min(k, n) = {kk} entries")
        self._call("lmc_select_topk", dev.device, stream, dev.data_ptr(), n, int(k), idx_out.data_ptr())
        return kk

    @staticmethod
    def _check_rope_args(cos_sin: torch.Tensor, rot_dim: int, deltas: Optional[torch.Tensor], ntok: Optional[int]) -> None:
        if not (cos_sin.is_cuda and cos_sin.dtype == torch.float32 and cos_sin.dim() == 2 and cos_sin.is_contiguous()
                and cos_sin.shape[1] == rot_dim):
            raise ValueError(f"cos_sin must be a contiguous device float32 [table_rows, rot_dim = {rot_dim}] tensor")
        if deltas is not None and not (deltas.is_cuda and deltas.dtype == torch.int32 and deltas.is_contiguous()
                                       and (ntok is None or deltas.numel() == ntok)):
            raise ValueError(f"deltas must be a contiguous device int32 tensor of ntok = {ntok} entries")


class LayerEncodeHandle:
    """A live lmc_layer_job of either coder model: encode_layer(l) for l = 0 .. L-1 in order, then finish() -- or abort() at any point.  The raw
    return codes are available (`*_rc`) for callers that test the refusals; the plain methods raise NativeError."""

    def __init__(self, ctx: "Context", handle, src: KVLayout):
        self.ctx, self.handle, self.src = ctx, handle, src

    def encode_layer_rc(self, layer: int, stream: Optional[int] = None) -> int:
        st = current_stream_ptr(self.src.device) if stream is None else stream
        return lib().lmc_encode_layer(self.ctx.handle, self.handle, layer, st)

    def encode_layer(self, layer: int, stream: Optional[int] = None) -> None:
        check(self.encode_layer_rc(layer, stream), "lmc_encode_layer")

    def finish_rc(self, stream: Optional[int] = None) -> int:
        st = current_stream_ptr(self.src.device) if stream is None else stream
        rc = lib().lmc_encode_layers_finish(self.ctx.handle, self.handle, st)
        if rc == 0:
            self.handle = None  # the job is gone
        return rc

    def finish(self, stream: Optional[int] = None) -> None:
        check(self.finish_rc(stream), "lmc_encode_layers_finish")

    def abort(self) -> None:
        if self.handle is not None:
            h, self.handle = self.handle, None
            check(lib().lmc_encode_layers_abort(self.ctx.handle, h), "lmc_encode_layers_abort")

    def __del__(self):
        try:
            if self.handle is not None and self.ctx.handle and not sys.is_finalizing():
                self.abort()
        except Exception:
            pass


def describe_status(st: int) -> str:
    names = [(1, "stream overflow"), (2, "bad blob header"), (4, "bad stream"), (8, "look-back timeout"), (16, "scale checksum mismatch"),
             (32, "host arena full"), (64, "rope delta outside the table")]
    return f"device status 0x{st:x} (" + ", ".join(n for b, n in names if st & b) + ")"


class StatusWords:
    """Pool of pinned uint32 words a job's kernels report their LMC_STATUS_* bits into (one word per job, so
    concurrent jobs never see each other's failures).  The pool grows by a block when every word is out: a caller
    that forgets jobs (their words come back when the job objects are collected) never breaks the cache."""
    BLOCK = 256

    def __init__(self, n: int = 256):
        self._blocks = []   # (PinnedBuffer, int32 view); word i lives in block i // BLOCK
        self._free = []
        self._lock = threading.Lock()
        self._grow()

    def _grow(self) -> None:
        buf = PinnedBuffer(4 * self.BLOCK)
        base = len(self._blocks) * self.BLOCK
        self._blocks.append((buf, buf.tensor.view(torch.int32)))
        self._free.extend(range(base + self.BLOCK - 1, base - 1, -1))

    def acquire(self) -> int:
        with self._lock:
            if not self._free:
                self._grow()
            i = self._free.pop()
            self._blocks[i // self.BLOCK][1][i % self.BLOCK] = 0
        return i

    def ptr(self, i: int) -> int:
        return self._blocks[i // self.BLOCK][0].ptr + 4 * (i % self.BLOCK)

    def read_release(self, i: int) -> int:
        """Value of word i (the job's work must have completed) and return it to the pool."""
        with self._lock:
            buf, words = self._blocks[i // self.BLOCK]
            # (a job collected together with its pool -- the codec of a finished process or test module -- may be
            # finalised after the pool's pinned block has been freed: there is no word to read any more)
            if not buf.ptr:
                return 0
            self._free.append(i)
            return int(words[i % self.BLOCK]) & 0xffffffff

    def close(self) -> None:
        """Free the pinned blocks (the work of every job must have completed).  A word that is still out reads 0 from
        then on, and a pool that is used again starts on a fresh block."""
        with self._lock:
            for buf, _ in self._blocks:
                buf.free()
            self._free = []


def memcpy_async(dst_ptr: int, src_ptr: int, nbytes: int, kind: str, stream: int) -> None:
    k = {"d2h": 0, "h2d": 1, "d2d": 2}[kind]
    check(lib().lmc_memcpy_async(dst_ptr, src_ptr, nbytes, k, stream), "lmc_memcpy_async")


def blob_info(blob: bytes, total_len: Optional[int] = None) -> BlobHeader:
    """Parse + validate a blob header on the host (lmc_blob_info).  `blob` may be just the first 128 bytes
    when the blob's length is passed as total_len (a blob that lives in device memory)."""
    h = BlobHeader()
    if len(blob) < HEADER_BYTES:
        raise NativeError("blob shorter than its header")
    buf = (ctypes.c_uint8 * HEADER_BYTES).from_buffer_copy(bytes(blob[:HEADER_BYTES]))
    rc = lib().lmc_blob_info(buf, len(blob) if total_len is None else total_len, ctypes.byref(h))
    check(rc, "lmc_blob_info")
    if h.model == MODEL_FIXED and total_len is None:
        # the whole blob is here: its bins, totals and stream directory against the computed layout (lmc_fixed_blob_info)
        full = (ctypes.c_uint8 * len(blob)).from_buffer_copy(bytes(blob))
        check(lib().lmc_fixed_blob_info(full, len(blob), ctypes.byref(h)), "lmc_fixed_blob_info")
    return h


_ctx_lock = threading.Lock()
_ctxs = {}


def get_context(device: Optional[int] = None) -> Context:
    """Per-device singleton context."""
    dev = torch.cuda.current_device() if device is None else int(device)
    with _ctx_lock:
        if dev not in _ctxs:
            _ctxs[dev] = Context(dev)
        return _ctxs[dev]
