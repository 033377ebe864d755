"""lmc_decode_chunks_fixed_rope_schedule on the host: the export as include/lmc_hip.h declares it and native.py binds it,
and where the engine reads LMCACHE_AMD_FUSED_ROPE.  No GPU and no library."""
from lmcache_amd import native
from tests.test_binding_dispatch_host import _header_params
from tests.test_rope_split_host import _engine


def test_the_export_takes_the_arguments_of_the_split_schedule():
    params = _header_params("lmc_decode_chunks_fixed_rope_schedule")
    assert params == _header_params("lmc_decode_chunks_fixed_split_schedule")
    assert native.SYMBOLS["lmc_decode_chunks_fixed_rope_schedule"] == native.SYMBOLS["lmc_decode_chunks_fixed_split_schedule"]
    assert native._POST_SLOT["lmc_decode_chunks_fixed_rope_schedule"] == native._POST_SLOT["lmc_decode_chunks_fixed_split_schedule"]


def test_the_switch_is_read_at_construction_and_is_off_by_default(monkeypatch):
    monkeypatch.delenv("LMCACHE_AMD_FUSED_ROPE", raising=False)
    off = _engine(monkeypatch)
    monkeypatch.setenv("LMCACHE_AMD_FUSED_ROPE", "1")
    on = _engine(monkeypatch)
    monkeypatch.delenv("LMCACHE_AMD_FUSED_ROPE")
    assert (off.fused_rope, on.fused_rope) == (False, True)

    class Fixed:
        model = "fixed"

    class Rope:
        rot_dim, is_neox = 64, True
    # only the fixed-width tier, only its own engine (no stored_at view), only a head size the kernel serves
    assert not on._fused_rope_tier() and not on._fused_direct(True, "NHDB", Rope(), 64)
    on.engine_ = off.engine_ = Fixed()
    assert on._fused_rope_tier() and not off._fused_rope_tier()
    assert on._direct_retrieve(True, "NHDB", Rope(), 64) is True and on._direct_retrieve(True, "NHDB", Rope(), 96) is False
    assert off._direct_retrieve(True, "NHDB", Rope(), 64) is False
    on._stored_ws = 2
    assert not on._fused_rope_tier()
