"""lmc_kv_layout.paged_kind (include/lmc_hip.h) took the place of the struct's padding word: the struct keeps its size and
every other field its offset, and the ABI version does not move -- a caller that zeroes the struct sees no change."""
import ctypes

from lmcache_amd import native


def test_kv_layout_struct_keeps_its_size_and_offsets():
    S = native.KvLayoutStruct
    assert ctypes.sizeof(S) == 88
    assert S.block_size.offset == 72
    assert S.paged_kind.offset == 76 and S.paged_kind.size == 4
    assert S.stride_block.offset == 80
    # the fields in front of them, as include/lmc_hip.h lays them out
    assert [getattr(S, f).offset for f in ("dtype", "num_layers", "num_heads", "head_size", "base", "plane_ptrs", "stride_layer",
                                           "stride_kv", "stride_token", "stride_head", "slot_mapping")] == \
        [0, 4, 8, 12, 16, 24, 32, 40, 48, 56, 64]
    assert S().paged_kind == native.PAGED_ROWS == 0 and native.PAGED_SPLIT == 1


def test_abi_version_is_still_6():
    assert native.lib().lmc_abi_version() == 6
