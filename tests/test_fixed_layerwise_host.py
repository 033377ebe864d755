"""The fixed-width layer-by-layer store's surface, without a GPU: the two C exports at ABI 6, their bindings, the Python
signatures, the switch INTEGRATION.md names, and that the new kernel and the sliced instances use no scratch."""
import inspect
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ["lmc_encode_layers_begin_fixed", "lmc_ctx_set_fixed_layer_slices"]


def _code():
    hdr = open(os.path.join(ROOT, "include", "lmc_hip.h")).read()
    return hdr, re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def _params(code, name):
    return [" ".join(p.split()) for p in re.search(r"\bint " + name + r"\s*\(([^)]*)\)", code).group(1).split(",")]


def test_the_header_declares_both_exports_at_abi_6_and_the_library_exports_them():
    from lmcache_amd import native
    hdr, code = _code()
    assert re.search(r"#define LMC_ABI_VERSION 6\b", hdr), "no new ABI version: the exports are additive"
    for name in EXPORTS:
        assert re.search(r"\bint " + name + r"\s*\(", code), name
        assert name in native.SYMBOLS, name
    # begin_fixed's argument list is lmc_encode_layers_begin's, word for word
    assert _params(code, "lmc_encode_layers_begin_fixed") == _params(code, "lmc_encode_layers_begin")
    assert native.SYMBOLS["lmc_encode_layers_begin_fixed"] == native.SYMBOLS["lmc_encode_layers_begin"]
    assert _params(code, "lmc_ctx_set_fixed_layer_slices") == ["lmc_ctx* ctx", "int n"]
    native.build()
    lib = native.lib()
    out = subprocess.check_output(["nm", "-D", "--defined-only", native.SO_PATH], text=True)
    assert set(EXPORTS) <= set(re.findall(r" T (lmc_[a-z0-9_]+)", out))
    assert lib.lmc_abi_version() == 6
    # a call without a context is refused before anything else happens
    assert lib.lmc_encode_layers_begin_fixed(None, None, 0, 1, 1, None, None, 0, None, None, None) == native.ERR_INVALID
    assert lib.lmc_ctx_set_fixed_layer_slices(None, 2) == native.ERR_INVALID


def test_the_python_signatures():
    from lmcache_amd import native
    from lmcache_amd.storage_backend.serde.cachegen_device import CacheGenDeviceCodec
    want = list(inspect.signature(CacheGenDeviceCodec.encode_layers).parameters)
    assert want == ["self", "src", "tok_begin", "tok_end", "chunk_tokens", "bins"]
    assert list(inspect.signature(CacheGenDeviceCodec.encode_layers_fixed).parameters) == want
    assert list(inspect.signature(native.Context.encode_layers_begin_fixed).parameters) == \
        list(inspect.signature(native.Context.encode_layers_begin).parameters)
    assert list(inspect.signature(native.Context.set_fixed_layer_slices).parameters) == ["self", "n"]


def test_the_documents_name_the_switch():
    for doc in ("INTEGRATION.md", "README.md"):
        assert "LMCACHE_AMD_FIXED_LAYERWISE" in open(os.path.join(ROOT, doc)).read(), doc
    src = open(os.path.join(ROOT, "lmcache_amd", "storage_backend", "local_backend.py")).read()
    assert re.search(r"self\.fixed_layerwise = .*LMCACHE_AMD_FIXED_LAYERWISE", src)


def test_the_fixed_width_encoder_and_its_finish_kernel_use_no_scratch():
    """native.build() refuses a build in which they do (native._check_fixed_registers); held here against the remarks of
    the build that produced the library."""
    from lmcache_amd import native
    native.build()
    if not os.path.exists(native.RESOURCES_PATH):
        pytest.skip("the library was not compiled here (prebuilt): no kernel_resources.json")
    res = json.load(open(native.RESOURCES_PATH))
    enc = {k: v for k, v in res.items() if "k_fixed_encode" in k}
    fin = {k: v for k, v in res.items() if "k_fixed_layers_finish" in k}
    # 20 one-piece instances as before, 16 LAYER ones (2 dtypes x 4 plane widths x rows / NHDB), one finish kernel
    assert len(enc) == 36 and len(fin) == 1, (len(enc), len(fin))
    for name, v in {**enc, **fin}.items():
        assert v["ScratchSize"] == 0, (name, v)
    native._check_fixed_registers()
