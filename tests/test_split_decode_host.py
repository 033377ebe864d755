"""The host side of tests/test_gpu_split_decode.py, without a GPU.

The decoder addresses an LMC_PAGED_SPLIT destination with a 64-bit block base, a 32-bit lane offset (head, granule /
column, element) and a 32-bit scalar offset (the slot's step inside a run of eight, at most 7 * 16 bytes); the store's
range check covers their SUM (lmc_api.hip: decode_dst_ok).  The rule is restated here and held against limits worked
out by hand, as tests/test_far_offsets_host.py does for rows."""
import inspect

import pytest

DESC_RANGE = 0xfffffff0


def split_decode_dst_ok(H, D, bs, stride_head, E):
    """lmc_api.hip: decode_dst_ok for paged_kind == LMC_PAGED_SPLIT (strides in elements, E = element bytes)."""
    return stride_head >= 0 and ((H - 1) * stride_head + D * bs) * E + 7 * 16 <= DESC_RANGE


# (H, D, bs, E, the largest stride_head admitted), by hand:
#   E = 2: (H-1)*sh + D*bs <= (4294967280 - 112) / 2 = 2147483584;   E = 1: (H-1)*sh + D*bs <= 4294967168
LIMITS = [
    (2, 128, 16, 2, 2147483584 - 2048),            # 2147481536
    (2, 128, 16, 1, 4294967168 - 2048),            # 4294965120
    (8, 128, 16, 2, 306783076),                    # 7 * 306783076 = 2147481532 <= 2147481536 < 7 * 306783077
    (8, 128, 16, 1, 613566445),                    # 7 * 613566445 = 4294965115 <= 4294965120 < 7 * 613566446
    (2, 64, 32, 2, 2147483584 - 2048),
    (2, 80, 16, 1, 4294967168 - 1280),
]


@pytest.mark.parametrize("H,D,bs,E,limit", LIMITS)
def test_the_split_range_rule_against_hand_computed_limits(H, D, bs, E, limit):
    assert split_decode_dst_ok(H, D, bs, limit, E)
    assert not split_decode_dst_ok(H, D, bs, limit + 1, E)
    assert split_decode_dst_ok(H, D, bs, D * bs, E)  # the dense cache
    assert split_decode_dst_ok(H, D, bs, 0, E) and not split_decode_dst_ok(H, D, bs, -1, E)
    # at the limit the last byte a lane can name plus the largest scalar offset ends inside the range, one stride later not
    last = ((H - 1) * limit + D * bs) * E  # one past the last element of the last head
    assert last + 112 <= DESC_RANGE < last + (H - 1) * E + 112


def test_one_head_is_limited_by_the_block_alone():
    """H = 1: stride_head plays no part; D * block_size must fit.  E = 2, D = 128: bs <= 2147483584 / 128 = 16777215.5."""
    assert split_decode_dst_ok(1, 128, 16777215, 1 << 40, 2)
    assert not split_decode_dst_ok(1, 128, 16777216, 0, 2)
    assert split_decode_dst_ok(1, 128, 33554431, 0, 1) and not split_decode_dst_ok(1, 128, 33554432, 0, 1)


def test_the_rule_as_the_library_source_states_it():
    """The C side carries the same three numbers: the range, seven steps of 16 bytes, and D * block_size per head."""
    import os
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lmcache_amd", "csrc", "lmc_api.hip")).read()
    body = src[src.index("static bool decode_dst_ok("):]
    body = body[:body.index("\n}\n")]
    assert "LMC_PAGED_SPLIT" in body and "7 * 16" in body and "0xfffffff0" in body and "d->head_size * d->block_size" in body


def test_direct_is_the_last_keyword_and_defaults_to_false():
    from lmcache_amd.cache_engine import LMCacheEngine
    params = list(inspect.signature(LMCacheEngine.retrieve_into_paged).parameters.values())
    assert params[-1].name == "direct" and params[-1].default is False
    assert [p.name for p in params[-3:]] == ["mask", "rope", "direct"]
