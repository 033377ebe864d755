"""fp8 KV (OCP float8_e4m3fn / float8_e5m2) on the host side: dtype codes, refused inputs, the header's kv_dtype word,
the serde view of an fp8 blob, the raw tiers' byte arithmetic and the decoder's fp32 -> fp8 rounding (k_fp8.h).  No GPU.

An fp8 chunk is stored as the blob of its bf16 images with header word 23 (kv_dtype) set to the fp8 code
(include/lmc_format.h); these tests build such blobs by patching that word into oracle blobs of the images."""
import ctypes
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP8 = [torch.float8_e4m3fn, torch.float8_e5m2]


def _patched(blob: bytes, word23: int) -> bytes:
    return blob[:92] + struct.pack("<I", word23) + blob[96:]


def _oracle_blob(oracle, kv16, H, D, bins):
    bits, code = oracle.torch_to_bits(kv16)
    return oracle.encode_blob(bits, code, H, D, np.array(bins, np.int32))


def test_dtype_codes_round_trip():
    from lmcache_amd import native
    assert (native.FP8_E4M3, native.FP8_E5M2) == (2, 3)
    for dt, code in [(torch.bfloat16, 0), (torch.float16, 1), (torch.float8_e4m3fn, 2), (torch.float8_e5m2, 3)]:
        assert native.dtype_code(dt) == code
        assert native.torch_dtype(code) == dt
        assert native.elem_bytes(code) == dt.itemsize
    hdr = open(os.path.join(ROOT, "include", "lmc_format.h")).read()
    assert "#define LMC_DTYPE_FP8_E4M3 2" in hdr and "#define LMC_DTYPE_FP8_E5M2 3" in hdr


@pytest.mark.parametrize("dt,hint", [
    (torch.uint8, "view(torch.float8_e4m3fn)"),
    (torch.float8_e4m3fnuz, "fnuz"),
    (torch.float8_e5m2fnuz, "fnuz"),
    (torch.float32, "float32"),
])
def test_refused_kv_dtypes_say_what_to_do(dt, hint):
    from lmcache_amd import native
    with pytest.raises(ValueError, match=hint.replace("(", r"\(").replace(")", r"\)")):
        native.dtype_code(dt)


def test_blob_info_kv_dtype_word(oracle):
    from lmcache_amd import native
    torch.manual_seed(3)
    L, T, H, D = 2, 24, 2, 64
    x = (torch.randn(L, 2, T, H * D) * 4).to(torch.float8_e4m3fn)
    blob = _oracle_blob(oracle, x.to(torch.bfloat16), H, D, [32, 16, 16, 32])
    assert native.blob_info(blob).kv_dtype == 0  # every blob written so far: word 23 is 0
    for code, dt in [(2, torch.float8_e4m3fn), (3, torch.float8_e5m2)]:
        h = native.blob_info(_patched(blob, code))
        assert h.kv_dtype == code and h.dtype == native.BF16
        assert native.stored_dtype(h) == dt
    for bad in (1, 4, 7, 0x100):
        with pytest.raises(native.NativeError):
            native.blob_info(_patched(blob, bad))
    fp16_blob = _oracle_blob(oracle, torch.randn(L, 2, T, H * D).to(torch.float16), H, D, [32, 16, 16, 32])
    assert native.blob_info(fp16_blob).kv_dtype == 0
    with pytest.raises(native.NativeError):  # fp8 kv_dtype needs bf16 scales
        native.blob_info(_patched(fp16_blob, 2))


@pytest.mark.parametrize("dt", FP8, ids=["e4m3", "e5m2"])
def test_serde_view_of_an_fp8_blob(oracle, dt):
    from lmcache_amd import native
    from lmcache_amd.storage_backend.serde.cachegen_basics import CacheGenEncoderOutput
    torch.manual_seed(4)
    L, T, H, D = 2, 40, 4, 32
    x = (torch.randn(L, 2, T, H * D) * 3).to(dt)
    u = x.to(torch.bfloat16)
    bins = [32, 16, 16, 32]
    blob = _patched(_oracle_blob(oracle, u, H, D, bins), native.dtype_code(dt))
    out = CacheGenEncoderOutput.from_bytes(blob)
    assert out.dtype == dt
    scale = u.float().abs().amax(dim=-1, keepdim=True)  # [L, 2, T, 1]
    kmax, vmax = out.max_tensors_key, out.max_tensors_value
    assert kmax.dtype == dt and vmax.dtype == dt
    assert torch.equal(kmax.view(torch.uint8), scale[:, 0].to(dt).view(torch.uint8))
    assert torch.equal(vmax.view(torch.uint8), scale[:, 1].to(dt).view(torch.uint8))
    assert out.bins == bins


def test_retrieve_spec_follows_kv_dtype(oracle):
    from lmcache_amd import native
    from lmcache_amd.storage_backend.serde.cachegen_decoder import output_spec, retrieve_spec
    L, T, H, D = 1, 16, 1, 64
    blob = _oracle_blob(oracle, torch.randn(L, 2, T, H * D).to(torch.bfloat16), H, D, [32, 32])
    for fmt in ("vllm", "huggingface"):
        assert retrieve_spec(fmt, native.blob_info(blob)) == output_spec(fmt, L, T, H, D)
        for dt in FP8:
            shape, got = retrieve_spec(fmt, native.blob_info(_patched(blob, native.dtype_code(dt))))
            assert shape == output_spec(fmt, L, T, H, D)[0] and got == dt


def test_cachegen_tier_dtype_rule():
    from lmcache_amd.storage_backend.local_backend import _coded_dtype
    assert _coded_dtype("vllm", torch.float16) == torch.bfloat16  # the reference's rule, unchanged
    assert _coded_dtype("huggingface", torch.bfloat16) == torch.float16
    for dt in FP8:
        assert _coded_dtype("vllm", dt) == dt and _coded_dtype("huggingface", dt) == dt


def test_fp8_header_field_layout():
    from lmcache_amd import native
    assert ctypes.sizeof(native.BlobHeader) == 128
    assert native.BlobHeader.kv_dtype.offset == 92


def _vector_readable(dt, base, **strides):
    from lmcache_amd import native
    s = native.KvLayoutStruct()
    s.dtype = native.dtype_code(dt)
    s.num_layers, s.num_heads, s.head_size = 2, 2, 64
    s.base = base
    s.stride_layer, s.stride_kv, s.stride_token, s.stride_head = strides.get("layer", 2 * 2 * 8 * 128), 8 * 128, 128, 64
    return native.KVLayout(s, [], 8, torch.device("cpu")).vector_readable()


def test_vector_rule_for_fp8_is_eight_bytes():
    # 8 channels per vector: 16 bytes of a 16-bit dtype, 8 bytes of fp8
    assert _vector_readable(torch.float8_e4m3fn, 0x1008)
    assert not _vector_readable(torch.float8_e4m3fn, 0x1004)
    assert not _vector_readable(torch.bfloat16, 0x1008)
    assert _vector_readable(torch.bfloat16, 0x1010)
    assert not _vector_readable(torch.float8_e5m2, 0x1000, layer=2 * 2 * 8 * 128 + 4)


def _compile_fp8_rounding(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src = tmp_path / "fp8_round.cpp"
    src.write_text('#include "%s"\n'
                   'extern "C" void cvt(const float* x, unsigned char* o4, unsigned char* o5, long n) {\n'
                   '  for (long i = 0; i < n; i++) { o4[i] = (unsigned char)lmc_f32_to_fp8<2>(x[i]);'
                   ' o5[i] = (unsigned char)lmc_f32_to_fp8<3>(x[i]); }\n}\n'
                   % os.path.join(ROOT, "lmcache_amd", "csrc", "k_fp8.h"))
    so = tmp_path / "fp8_round.so"
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-shared", "-fPIC", str(src), "-o", str(so)])
    return ctypes.CDLL(str(so))


def test_decoder_fp8_rounding_is_torchs(tmp_path):
    """k_fp8.h's lmc_f32_to_fp8 (the decoder's fp32 -> fp8 cast) against torch's CPU cast: every fp32 exponent with
    random and edge mantissas, both signs, and the values around every fp8 rounding boundary.  NaN by NaN-ness."""
    lib = _compile_fp8_rounding(tmp_path)
    rng = np.random.default_rng(0)
    e = np.repeat(np.arange(256, dtype=np.uint32), 4096)
    m = rng.integers(0, 1 << 23, e.size, dtype=np.uint32)
    m[::4096] = 0
    m[1::4096] = (1 << 23) - 1
    s = rng.integers(0, 2, e.size, dtype=np.uint32)
    u = [(s << 31) | (e << 23) | m]
    # the midpoints between neighbouring fp8 values (ties) and one fp32 ulp either side, for both formats
    for dt in FP8:
        v = torch.arange(256, dtype=torch.int32).to(torch.uint8).view(dt).float().numpy()
        v = np.unique(v[np.isfinite(v)])
        mid = ((v[:-1].astype(np.float64) + v[1:]) / 2).astype(np.float32)
        for d in (-1, 0, 1):
            w = (mid.view(np.uint32).astype(np.int64) + d).astype(np.uint32)
            u += [w, w ^ np.uint32(0x80000000)]
    u = np.concatenate(u)
    x = u.view(np.float32)
    o4, o5 = np.empty(x.size, np.uint8), np.empty(x.size, np.uint8)
    lib.cvt(x.ctypes.data_as(ctypes.c_void_p), o4.ctypes.data_as(ctypes.c_void_p), o5.ctypes.data_as(ctypes.c_void_p),
            ctypes.c_long(x.size))
    xt = torch.from_numpy(x)
    r4 = xt.to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    r5 = xt.to(torch.float8_e5m2).view(torch.uint8).numpy()
    nan4, nan5 = (r4 & 0x7f) == 0x7f, (r5 & 0x7f) > 0x7c
    assert np.array_equal(o4[~nan4], r4[~nan4]) and (o4[nan4] == 0x7f).all()
    assert np.array_equal(o5[~nan5], r5[~nan5]) and (o5[nan5] == 0x7f).all()
    assert (o5[r5 == 0x7c] == 0x7c).all() and (o5[r5 == 0xfc] == 0xfc).all()  # e5m2 +-inf bit for bit
