"""The fixed-width model on an "NHDB" cache (lmc_encode_chunks_fixed_split, lmc_decode_chunks_fixed_split_schedule) as far
as it shows without a GPU: the declarations, the exports, the bindings, and the configuration rule, which does not move."""
import inspect
import os
import re

import pytest

from lmcache_amd import native
from lmcache_amd.config import LMCacheEngineConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWINS = {"lmc_encode_chunks_fixed_split": "lmc_encode_chunks_fixed",
         "lmc_decode_chunks_fixed_split_schedule": "lmc_decode_chunks_fixed_schedule"}


def _params(hdr, name):
    m = re.search(r"\bint %s\(([^;]*)\);" % name, hdr)
    assert m, name
    return re.sub(r"\s+", " ", m.group(1)).strip()


def test_the_header_declares_the_two_exports_with_their_row_twins_signatures_at_abi_6():
    hdr = open(os.path.join(ROOT, "include", "lmc_hip.h")).read()
    assert re.search(r"#define LMC_ABI_VERSION 6\b", hdr)
    for new, twin in TWINS.items():
        assert _params(hdr, new) == _params(hdr, twin), new
        assert native.SYMBOLS[new] == native.SYMBOLS[twin], new


def test_the_library_exports_them_at_abi_6():
    native.build()
    lib = native.lib()
    assert lib.lmc_abi_version() == 6
    for new in TWINS:
        assert getattr(lib, new) is not None, new


def test_the_context_methods_have_the_parameter_order_of_their_row_twins():
    for new, twin in (("encode_chunks_fixed_split", "encode_chunks_fixed"),
                      ("decode_chunks_fixed_split_schedule", "decode_chunks_fixed_schedule")):
        a = inspect.signature(getattr(native.Context, new)).parameters
        b = inspect.signature(getattr(native.Context, twin)).parameters
        assert list(a) == list(b), new
        assert [p.default for p in a.values()] == [p.default for p in b.values()], new


def test_local_backend_config_rules_are_unchanged(tmp_path):
    ok = LMCacheEngineConfig(16, "cuda", None, None, False, False, "cachegen-fixed")
    assert ok.local_serde == "cachegen-fixed"
    with pytest.raises(ValueError, match="PCIe"):
        LMCacheEngineConfig(16, "cpu", None, None, False, False, "cachegen-fixed")
    with pytest.raises(ValueError, match="cuda"):
        LMCacheEngineConfig(16, str(tmp_path) + "/", None, None, False, False, "cachegen-fixed")
    from lmcache_amd.cache_engine import LMCacheEngine
    for name in ("store_paged", "retrieve_into_paged", "retrieve_into_paged_layerwise"):
        assert inspect.signature(getattr(LMCacheEngine, name)).parameters["direct"].default is False, name
