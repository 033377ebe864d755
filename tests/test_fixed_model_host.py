"""LMC_MODEL_FIXED without a GPU: the format's arithmetic (include/lmc_format.h), the numpy reference of its bytes
(tests/fixed_model.py), the C ABI's new exports, lmc_blob_info on a fixed-width blob, and the configuration rule."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from lmcache_amd import native
from lmcache_amd.config import LMCacheEngineConfig
from tests import fixed_model as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lmc_encode_chunks_fixed", "lmc_decode_chunks_fixed_schedule", "lmc_fixed_blob_info")


@pytest.fixture(scope="module")
def fmt_lib(tmp_path_factory):
    """The inline helpers of include/lmc_format.h themselves, compiled into a small C library."""
    d = tmp_path_factory.mktemp("fixedfmt")
    src = d / "f.c"
    src.write_text('#include "lmc_format.h"\n'
                   "unsigned sb(unsigned bins, unsigned T) { return lmc_fixed_stream_bytes(bins, T); }\n"
                   "unsigned long long bb(unsigned L, unsigned T, unsigned H, unsigned D, const unsigned char* b) "
                   "{ return lmc_fixed_blob_bytes(L, T, H, D, b); }\n"
                   "unsigned long long bound(unsigned L, unsigned T, unsigned H, unsigned D) { return lmc_blob_bound(L, T, H, D); }\n"
                   "int valid(unsigned T) { return lmc_fixed_valid(T); }\n"
                   "int coded_valid(unsigned m, unsigned T) { return lmc_model_valid(m, T); }\n"
                   "unsigned coded_for(unsigned T) { return lmc_model_for(T); }\n")
    so = d / "f.so"
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-O1", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(so)])
    lib = ctypes.CDLL(str(so))
    lib.sb.restype = ctypes.c_uint
    lib.bb.restype = lib.bound.restype = ctypes.c_uint64
    lib.bb.argtypes = [ctypes.c_uint] * 4 + [ctypes.c_char_p]
    return lib


def test_header_declares_the_new_exports_at_abi_6_and_the_library_has_them():
    text = open(os.path.join(ROOT, "include", "lmc_hip.h")).read()
    assert re.search(r"#define LMC_ABI_VERSION 6\b", text)
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, text), name
        assert name in native.SYMBOLS
    assert re.search(r"#define LMC_MODEL_FIXED 2u", open(os.path.join(ROOT, "include", "lmc_format.h")).read())
    lib = native.lib()
    assert lib.lmc_abi_version() == 6
    for name in NEW:
        assert getattr(lib, name) is not None


def test_format_helpers_match_the_numpy_layout(fmt_lib):
    for T in (1, 7, 8, 9, 100, 255, 256, 257, 300, 65535):
        assert fmt_lib.valid(T)
        for bins in (4, 16, 17, 18, 31, 32):
            assert fmt_lib.sb(bins, T) == fm.stream_bytes(bins, T) == native.fixed_stream_bytes(bins, T)
    assert not fmt_lib.valid(0) and not fmt_lib.valid(65536)
    # the coded models' own rules are as they were: model 2 is none of theirs
    assert not fmt_lib.coded_valid(2, 256) and fmt_lib.coded_for(256) == 1 and fmt_lib.coded_for(300) == 0
    rng = np.random.default_rng(3)
    for L, T, H, D in ((1, 1, 1, 8), (2, 20, 3, 40), (3, 300, 2, 64), (32, 256, 8, 128)):
        bins = rng.choice([32, 18, 17, 16, 4], size=2 * L).astype(np.uint8)
        want = fm.blob_bytes(L, T, H, D, bins)
        assert fmt_lib.bb(L, T, H, D, bins.tobytes()) == want == native.fixed_blob_bytes(L, T, H, D, bins.tolist())


def test_fixed_blob_never_outgrows_the_coded_models_slot(fmt_lib):
    for C in (8, 120, 1024, 4096):
        for T in range(1, 301):
            for bins in (17, 18):  # the widest narrow plane, the narrowest wide one: both plane kinds
                b = bytes([bins, bins])
                assert fmt_lib.bb(1, T, 1, C, b) <= fmt_lib.bound(1, T, 1, C), (C, T, bins)
            assert fmt_lib.bb(1, T, 1, C, bytes([32, 32])) <= fmt_lib.bound(1, T, 1, C), (C, T)


def test_llama3_8b_chunk_size(oracle, fmt_lib):
    bins, L = oracle.cachegen_bins("meta-llama/Llama-3.1-8B-Instruct")
    assert native.fixed_blob_bytes(L, 256, 8, 128, bins.tolist()) == 8839616
    assert fmt_lib.bb(L, 256, 8, 128, bins.astype(np.uint8).tobytes()) == 8839616
    raw = L * 2 * 256 * 1024 * 2
    assert round(raw / 8839616, 2) == 3.80


def _chunk(rng, L, T, C, dtype_code):
    x = rng.standard_normal((L, 2, T, C)).astype(np.float32) * np.exp(rng.standard_normal(C)).astype(np.float32)
    import torch
    t = torch.from_numpy(x).to(torch.bfloat16 if dtype_code == 0 else torch.float16)
    return t.view(torch.int16).numpy().view(np.uint16)


@pytest.mark.parametrize("shape", [(1, 1, 1, 8), (2, 20, 3, 40), (1, 100, 2, 64)])
def test_numpy_pack_round_trips_to_the_oracle(oracle, shape):
    L, T, H, D = shape
    rng = np.random.default_rng(T)
    for code in (oracle.BF16, oracle.FP16):
        bins = np.array([32, 18, 17, 16, 4, 32][:2 * L] if L > 1 else [18, 17], np.int32)
        kv = _chunk(rng, L, T, H * D, code)
        blob = fm.encode_blob(oracle, kv, code, H, D, bins)
        assert len(blob) == fm.blob_bytes(L, T, H, D, bins)
        sym, scale = oracle.quantize(kv, code, bins)
        assert int(sym.max()) <= 2 * (int(bins.max()) // 2 - 1) and int(sym.min()) >= 0
        assert np.array_equal(fm.unpack_symbols(blob), sym)
        for out in (oracle.BF16, oracle.FP16):
            assert np.array_equal(fm.decode_blob(oracle, blob, out), oracle.dequantize(sym, scale, code, bins, out))
        # ... and to what the coded blob of the same chunk decodes to
        assert np.array_equal(fm.decode_blob(oracle, blob, code), oracle.decode_blob(oracle.encode_blob(kv, code, H, D, bins), code))


def test_a_change_of_any_single_dword_changes_the_check_word():
    rng = np.random.default_rng(11)
    w = rng.integers(0, 1 << 32, size=400, dtype=np.uint64)
    base = fm.check_word(w)
    for i in range(len(w)):
        for delta in (1, 1 << 31, int(rng.integers(1, 1 << 32))):
            v = w.copy()
            v[i] = (int(v[i]) + delta) & 0xffffffff
            assert fm.check_word(v) != base, (i, delta)  # (2 i + 1) is odd: (2 i + 1) * delta != 0 mod 2^32


def test_config_takes_cachegen_fixed_with_cuda_only(tmp_path):
    cfg = LMCacheEngineConfig.from_legacy(chunk_size=16, backend="cuda", persist_path=None)
    ok = LMCacheEngineConfig(16, "cuda", None, None, False, False, "cachegen-fixed")
    assert ok.local_serde == "cachegen-fixed" and cfg.local_device == "cuda"
    with pytest.raises(ValueError, match="PCIe"):
        LMCacheEngineConfig(16, "cpu", None, None, False, False, "cachegen-fixed")
    with pytest.raises(ValueError, match="cuda"):
        LMCacheEngineConfig(16, str(tmp_path) + "/", None, None, False, False, "cachegen-fixed")
    y = tmp_path / "c.yaml"
    y.write_text("chunk_size: 16\nlocal_device: cpu\nlocal_serde: cachegen-fixed\n")
    with pytest.raises(ValueError, match="PCIe"):
        LMCacheEngineConfig.from_file(str(y))
    y.write_text("chunk_size: 16\nlocal_device: cuda\nlocal_serde: cachegen-fixed\n")
    assert LMCacheEngineConfig.from_file(str(y)).local_serde == "cachegen-fixed"


def test_blob_info_on_a_numpy_made_blob(oracle):
    from lmcache_amd.storage_backend.serde.cachegen_basics import CacheGenGPUEncoderOutput
    L, T, H, D = 2, 20, 3, 40
    bins = np.array([32, 17, 18, 4], np.int32)
    kv = _chunk(np.random.default_rng(5), L, T, H * D, oracle.BF16)
    blob = fm.encode_blob(oracle, kv, oracle.BF16, H, D, bins)
    h = native.blob_info(blob)
    assert (h.model, h.num_layers, h.ntokens, h.num_heads, h.head_size, h.total_bytes) == (2, L, T, H, D, len(blob))
    out = CacheGenGPUEncoderOutput.from_bytes(blob)
    assert out.bins == bins.tolist() and out.num_heads == H and out.head_size == D and out.ntokens == T
    _, scale = oracle.quantize(kv, oracle.BF16, bins)
    assert np.array_equal(out.max_tensors_key.view(__import__("torch").int16).numpy().view(np.uint16)[..., 0], scale[:L])
    assert out.max_tensors_value.shape == (L, T, 1)
    for name in ("cdf", "data_chunks"):
        with pytest.raises(ValueError, match="fixed-width"):
            getattr(out, name)

    def patched(off, value):
        b = bytearray(blob)
        b[off:off + 4] = int(value).to_bytes(4, "little")
        return bytes(b)
    hd = fm.header(blob)
    for bad in (patched(4 * fm.W_TOTAL, len(blob) - 16), patched(4 * fm.W_STREAM_BYTES, int(hd[fm.W_STREAM_BYTES]) + 16),
                patched(int(hd[fm.W_OFF_GDIR]) + 8, 16), patched(int(hd[fm.W_OFF_GDIR]) + 4, 0), patched(4 * fm.W_MODEL, 3),
                blob[:len(blob) - 16]):
        with pytest.raises(native.NativeError):
            native.blob_info(bad)
    # a bins byte that changes a plane's kind moves every stream behind it: refused
    b = bytearray(blob)
    b[int(hd[fm.W_OFF_BINS]) + 1] = 18
    with pytest.raises(native.NativeError):
        native.blob_info(bytes(b))
