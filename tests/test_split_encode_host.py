"""The split-source encode (lmc_encode_chunks_split, store_paged(direct=)) as far as it shows without a GPU."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_store_paged_takes_direct_as_its_last_keyword_default_false():
    from lmcache_amd.cache_engine import LMCacheEngine
    params = list(inspect.signature(LMCacheEngine.store_paged).parameters.values())
    assert params[-1].name == "direct" and params[-1].default is False
    # the mirror of retrieve_into_paged(direct=)
    assert inspect.signature(LMCacheEngine.retrieve_into_paged).parameters["direct"].default is False


def test_the_entry_point_is_declared_and_bound():
    from lmcache_amd import native
    hdr = open(os.path.join(ROOT, "include", "lmc_hip.h")).read()
    decl = re.search(r"int lmc_encode_chunks_split\(([^;]*)\);", hdr)
    same = re.search(r"int lmc_encode_chunks\(([^;]*)\);", hdr)
    assert decl and same and re.sub(r"\s+", " ", decl.group(1)) == re.sub(r"\s+", " ", same.group(1))
    assert "lmc_encode_chunks_split" in native.SYMBOLS
    assert native.SYMBOLS["lmc_encode_chunks_split"] == native.SYMBOLS["lmc_encode_chunks"]
    assert re.search(r"#define LMC_ABI_VERSION 6\b", hdr)


def test_the_library_exports_it_at_abi_6():
    from lmcache_amd import native
    native.build()
    lib = native.lib()
    assert lib.lmc_abi_version() == 6
    assert hasattr(lib, "lmc_encode_chunks_split")
