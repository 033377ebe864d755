"""The layer-by-layer store's surface, without a GPU: the four C exports at ABI 6, the Python signatures, the names the
connector snippet of INTEGRATION.md uses, and that the product does not lean on the oracle."""
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ["lmc_encode_layers_begin", "lmc_encode_layer", "lmc_encode_layers_finish", "lmc_encode_layers_abort"]


def _header():
    return open(os.path.join(ROOT, "include", "lmc_hip.h")).read()


def test_the_header_declares_the_four_exports_at_abi_6_and_the_library_exports_them():
    from lmcache_amd import native
    hdr = _header()
    assert re.search(r"#define LMC_ABI_VERSION 6\b", hdr), "no new ABI version: the exports are additive"
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in EXPORTS:
        assert re.search(r"\bint " + name + r"\s*\(", code), name
        assert name in native.SYMBOLS, name
    # the arguments of begin are lmc_encode_chunks_split's, with the job in the stream's place
    def params(name):
        return [p.strip() for p in re.search(r"\bint " + name + r"\s*\(([^)]*)\)", code).group(1).split(",")]
    split, begin = params("lmc_encode_chunks_split"), params("lmc_encode_layers_begin")
    assert begin[:-1] == split[:-1] and begin[-1].startswith("lmc_layer_job**")
    m = re.search(r"#define LMC_NOT_LAYERWISE (\d+)", hdr)
    assert m and int(m.group(1)) > 0 and int(m.group(1)) == native.NOT_LAYERWISE, "a positive code of its own"
    assert native.SYMBOLS["lmc_encode_layers_begin"][1][:-1] == native.SYMBOLS["lmc_encode_chunks_split"][1][:-1]
    native.build()
    lib = native.lib()
    out = subprocess.check_output(["nm", "-D", "--defined-only", native.SO_PATH], text=True)
    exported = set(re.findall(r" T (lmc_[a-z0-9_]+)", out))
    assert set(EXPORTS) <= exported
    assert lib.lmc_abi_version() == 6
    assert b"layer-wise" in lib.lmc_strerror(native.NOT_LAYERWISE)
    # a call without a context or a job is refused before anything else happens
    assert lib.lmc_encode_layer(None, None, 0, None) == native.ERR_INVALID
    assert lib.lmc_encode_layers_finish(None, None, None) == native.ERR_INVALID
    assert lib.lmc_encode_layers_abort(None, None) == native.ERR_INVALID


def _defaults(fn):
    return {k: v.default for k, v in inspect.signature(fn).parameters.items() if v.default is not inspect.Parameter.empty}


def test_the_python_signatures():
    from lmcache_amd.cache_engine import LayerwiseStore, LMCacheEngine
    from lmcache_amd.storage_backend.abstract_backend import LMCBackendInterface
    from lmcache_amd.storage_backend.local_backend import LMCLocalBackend
    from lmcache_amd.storage_backend.serde.cachegen_device import CacheGenDeviceCodec, EncodeJob, LayerwiseEncodeJob
    sig = inspect.signature(LMCacheEngine.store_paged_layerwise)
    assert list(sig.parameters) == ["self", "tokens", "kv_caches", "slot_mapping", "block_size", "layout", "skip_existing", "direct"]
    assert _defaults(LMCacheEngine.store_paged_layerwise) == {"layout": "NBHD", "skip_existing": True, "direct": False}
    for cls in (LMCLocalBackend, LMCBackendInterface):
        assert list(inspect.signature(cls.begin_put_kv_layers).parameters) == \
            ["self", "keys", "src", "fmt", "tok_begin", "tok_end", "chunk_tokens"]
    assert _defaults(LayerwiseStore.finish) == {"blocking": True}
    for name in ("save_layer", "layer_event", "finish"):
        assert callable(getattr(LayerwiseStore, name))
    assert issubclass(LayerwiseEncodeJob, EncodeJob), "after finish() the job IS an EncodeJob"
    assert list(inspect.signature(CacheGenDeviceCodec.encode_layers).parameters) == \
        ["self", "src", "tok_begin", "tok_end", "chunk_tokens", "bins"]
    # the existing entry points keep their signatures
    assert list(inspect.signature(LMCacheEngine.store_paged).parameters) == \
        ["self", "tokens", "kv_caches", "slot_mapping", "block_size", "layout", "skip_existing", "blocking", "direct"]
    assert list(inspect.signature(LMCLocalBackend.put_kv_range).parameters) == \
        ["self", "keys", "src", "fmt", "tok_begin", "tok_end", "chunk_tokens", "blocking", "direct"]
    # backends without a layer-wise path say None (the engine then stores in one piece at finish)
    assert LMCBackendInterface.begin_put_kv_layers(object(), [], None, "vllm", 0, 0, 256) is None


def test_the_connector_snippet_of_integration_md_names_what_exists():
    from lmcache_amd.cache_engine import LayerwiseRetrieval, LayerwiseStore, LMCacheEngine
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "store_paged_layerwise(" in doc and hasattr(LMCacheEngine, "store_paged_layerwise")
    for hook, call in (("save_kv_layer", "self._save.save_layer(i)"), ("wait_for_save", "self._save.finish(blocking=False)")):
        assert re.search(r"\|\s*`" + hook + r"`\s*\|\s*`" + re.escape(call) + r"`\s*\|", doc), hook
    for name in re.findall(r"self\._save\.(\w+)\(", doc):
        assert hasattr(LayerwiseStore, name), name
    for name in re.findall(r"self\._load\.(\w+)\(", doc):
        assert hasattr(LayerwiseRetrieval, name), name


def test_the_product_does_not_import_the_oracle():
    bad = []
    for base, _, files in os.walk(os.path.join(ROOT, "lmcache_amd")):
        for fn in files:
            if fn.endswith((".py", ".h", ".hip")):
                src = open(os.path.join(base, fn), errors="replace").read()
                if re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M) or "lmc_oracle" in src:
                    bad.append(fn)
    assert not bad, bad
