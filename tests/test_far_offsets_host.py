"""The integer side of tests/test_gpu_far_offsets.py, without a GPU (helpers: tests/far_offsets.py).

  1. The safety property of every layout the GPU tests use (far_offsets.REGISTRY, refused layouts included): each address,
     also with one of its offsets reduced mod 2^32 or sign-extended from 32 bits, lies inside the arena -- so a kernel
     that narrows an offset misplaces data where the arena check finds it and does not fault a shared machine.
  2. The tables do reach both sides of 2^31 and 2^32 bytes, and for 1-byte elements of 2^31 and 2^32 elements.
  3. The specs' offset arithmetic is torch's own indexing of the same as_strided views (a small CPU stand-in).
  4. The arena checker passes on correct placement and names the offsets when a row lands one block low or is dropped."""
import numpy as np
import pytest
import torch

from tests import far_offsets as fo

P31, P32 = 1 << 31, 1 << 32


# ------------------------------------------------------------------ 1. safety
@pytest.mark.parametrize("name", sorted(fo.REGISTRY))
def test_every_address_stays_inside_the_arena_with_one_offset_narrowed(name):
    assert fo.unsafe_addresses(fo.REGISTRY[name]) == []


def test_the_safety_check_can_fail():
    """Without the 2 GiB guard in front a sign-extended block offset leaves the arena; without the room behind, a true one."""
    spec = fo.REGISTRY["NBHD_e2_bs16_runs"]
    low = fo.unsafe_addresses(spec.with_("no_guard", base=64), fo.ARENA_BYTES - fo.GUARD)
    assert low and all("sign-extended" in b for b in low) and any("block offset" in b for b in low)
    assert any(": true:" in b for b in fo.unsafe_addresses(spec, fo.GUARD + 4 * fo.GIB))


def test_every_plane_base_is_the_guards_end_give_or_take_a_few_kib():
    for spec in fo.REGISTRY.values():
        assert 0 <= spec.base - fo.GUARD <= 128 * 1024, spec.name
    assert fo.ARENA_BYTES == 2 * fo.GIB + 4 * fo.GIB + 256 * (1 << 20) and fo.ARENA_BYTES % fo.SLAB == 0


# ------------------------------------------------------------------ 2. the tables reach what they are for
def _plane_relative(spec):
    """Byte offsets from the plane base of the first and the last byte of every piece."""
    if isinstance(spec, fo.SplitSpec):
        off = spec.element_offsets()[0, 0] - spec.base - spec.plane_off[0]
        return off.reshape(-1), off.reshape(-1) + spec.esz - 1
    off = spec.row_offsets()[0, 0] - spec.base - spec.plane_off[0]
    return off.reshape(-1), off.reshape(-1) + spec.D * spec.esz - 1


@pytest.mark.parametrize("name", [n for n in sorted(fo.REGISTRY) if n[:4] in ("NBHD", "NHBD", "NHDB")])  # (not the limit layouts)
def test_paged_tables_reach_both_sides_of_2_31_and_2_32(name):
    spec = fo.REGISTRY[name]
    first, last = _plane_relative(spec)
    assert first.min() == 0
    for edge in (P31, P32):
        below, above = last[last < edge], first[first >= edge]
        assert edge - below.max() <= fo.STRIDE_BLOCK, "the block that ends at the edge"
        assert above.min() == edge, "the block that starts there"
    assert first.max() // fo.STRIDE_BLOCK == fo.NUM_BLOCKS - 1, "the arena's last block"
    assert spec.base + (fo.NUM_BLOCKS + 1) * fo.STRIDE_BLOCK > fo.ARENA_BYTES, "... behind which no further block fits"
    # in ELEMENTS: a byte is an element for fp8; 16-bit elements pass 2^31 (at 2^32 bytes) but 2^32 needs an 8 GiB plane
    fe, le = first // spec.esz, last // spec.esz
    edges = (P31, P32) if spec.esz == 1 else (P31,)
    for edge in edges:
        assert (le < edge).any() and (fe >= edge).any()
    if spec.esz == 2:
        assert le.max() < P32
    # a block of the mapping is used by the tokens the mapping gives it, all of them far apart or not: both block sizes
    assert len(np.unique(spec.slots // spec.bs)) == (fo.T + spec.bs - 1) // spec.bs


@pytest.mark.parametrize("esz", [1, 2])
def test_dense_views_and_limit_layouts_reach_past_2_32(esz):
    for kind in ("vllm", "huggingface"):
        spec = fo.REGISTRY[f"dense_{kind}_e{esz}"]
        assert spec.plane_off[2] > P31 > spec.plane_off[1] and spec.plane_off[3] > P32
    # the limits: the scalar offset of a chunk's last row plus the row itself against the descriptor's range
    head = fo.REGISTRY[f"head_stride_limit_e{esz}_over0"]
    assert (fo.CS - 1) * head.stride_token + fo.row_span(head) == fo.DESC_RANGE and head.stride_head > P32 - (1 << 16)
    tok = fo.REGISTRY[f"token_stride_limit_e{esz}_over0"]
    assert (fo.T - 1) * tok.stride_token + fo.row_span(tok) <= fo.DESC_RANGE < (fo.T - 1) * (tok.stride_token + esz) + fo.row_span(tok)
    assert 39 * (1 << 20) < tok.stride_token < 41 * (1 << 20)
    paged = fo.REGISTRY[f"paged_head_stride_limit_e{esz}_over0"]
    assert 7 * paged.stride_token + fo.row_span(paged) == fo.DESC_RANGE and paged.stride_token < (1 << 28)


def test_the_guards_inequalities_on_the_specs():
    for name, spec in fo.REGISTRY.items():
        refused = name.startswith("negative") or name.endswith("over1")
        assert fo.decode_dst_ok(spec, spec.chunk) == (not refused), name


def test_mappings_take_the_paths_they_are_named_for():
    """runs: every aligned group of eight tokens of a 40-token chunk is eight consecutive slots of one block when the
    block size is 16 (the decoder's block path, the split copy's fast tiles); swapped or block size 12: some group of
    every chunk is not."""
    def groups_are_runs(slots, bs):
        ok = []
        for c0 in range(0, fo.T, fo.CS):
            n = min(fo.CS, fo.T - c0)
            g = slots[c0:c0 + n // 8 * 8].reshape(-1, 8)
            ok.append(bool(((g - g[:, :1] == np.arange(8)).all(1) & (g[:, 0] // bs == g[:, 7] // bs)).all()))
        return ok
    assert groups_are_runs(fo.slot_table(16, False), 16) == [True, True, True]
    assert groups_are_runs(fo.slot_table(16, True), 16) == [False, False, False]
    assert groups_are_runs(fo.slot_table(12, False), 12) == [False, False, False]
    assert groups_are_runs(fo.slot_table(12, True), 12) == [False, False, False]


# ------------------------------------------------------------------ 3. and 4. a small stand-in on the CPU
SMALL_ARENA, SMALL_WINDOW, SMALL_SLAB = 1 << 20, 256, 1 << 16
SL, SH, SD, ST, SBS = 2, 2, 8, 20, 4
SMALL_BLOCKS = [7, 3, 11, 12, 5]


def _small(kind, esz):
    base = 4096 + 64
    if kind in ("NBHD", "NHBD", "NHDB"):
        slots = fo.slot_table(SBS, True, ST, SMALL_BLOCKS)
        planes = [p * 256 for p in range(2 * SL)]
        if kind == "NHDB":
            return fo.SplitSpec("small_split", kind, esz, base, planes, 0, 16 * SBS * esz, slots, SBS, 1024, ST, SL, SH, 16)
        st, sh = (SH * SD * esz, SD * esz) if kind == "NBHD" else (SD * esz, SBS * SD * esz)
        return fo.RowsSpec("small_" + kind, kind, esz, base, planes, st, sh, slots, SBS, 1024, ST, SL, SH, SD)
    planes = [p * 200000 for p in range(2 * SL)]
    st, sh = (SH * SD * esz, SD * esz) if kind == "vllm" else (SD * esz, ST * SD * esz)
    return fo.RowsSpec("small_" + kind, kind, esz, base, planes, st, sh, None, 0, 0, ST, SL, SH, SD)


def _fresh():
    return torch.full((SMALL_ARENA,), fo.FILL, dtype=torch.uint8)


def _check(arena, spec, data, **kw):
    return fo.check_arena(arena, *spec.pieces(data, **kw), what=spec.name, window=SMALL_WINDOW, slab=SMALL_SLAB)


def _torch_scatter(spec, arena, dt, x, tok, layers):
    """x [l, 2, t, H, D] into tokens `tok` of layers `layers` by torch indexing of the spec's views."""
    views = spec.views(arena, dt)
    esz = spec.esz
    if spec.kind in ("vllm", "huggingface"):
        dst = views if spec.kind == "vllm" else views.permute(0, 1, 3, 2, 4)
        dst[layers, :, tok] = x
        return
    blk, off = torch.from_numpy(spec.slots[tok] // spec.bs), torch.from_numpy(spec.slots[tok] % spec.bs)
    for c, xl in zip(views[layers], x):
        for kv in range(2):
            if spec.kind == "NBHD":
                c[kv, blk, off] = xl[kv]
            elif spec.kind == "NHBD":
                c[kv, blk, :, off] = xl[kv]
            elif kv == 1:  # value_cache [num_blocks, H, D, block_size]
                c[1, blk, :, :, off] = xl[1]
            else:          # key_cache = cache[0].view(num_blocks, H, D / x, block_size, x)
                xg = 16 // esz
                kc = c[0].view(c.shape[1], spec.H, spec.D // xg, spec.bs, xg)
                kc[blk, :, :, off, :] = xl[0].reshape(-1, spec.H, spec.D // xg, xg)


@pytest.mark.parametrize("esz", [1, 2])
@pytest.mark.parametrize("kind", ["NBHD", "NHBD", "vllm", "huggingface", "NHDB"])
def test_spec_offsets_are_torch_indexing_of_the_views(kind, esz):
    spec = _small(kind, esz)
    assert fo.unsafe_addresses(spec, SMALL_ARENA) == []
    dt = torch.uint8 if esz == 1 else torch.int16
    g = torch.Generator().manual_seed(7)
    x = torch.randint(1, 100, (spec.L, 2, spec.ntok, spec.H, spec.D), generator=g).to(dt)
    arena = _fresh()
    _torch_scatter(spec, arena, dt, x, slice(None), slice(None))
    _check(arena, spec, fo.to_bytes(x))
    # a sub-range of tokens of one layer, as the GPU tests select them
    sub = _fresh()
    _torch_scatter(spec, sub, dt, x[1:, :, 3:9], slice(3, 9), slice(1, 2))
    starts = _check(sub, spec, fo.to_bytes(x[1:, :, 3:9]), tok=slice(3, 9), layers=slice(1, 2))
    fo.restore_windows(sub, starts, window=SMALL_WINDOW)
    assert fo.count_stray_words(sub, slab=SMALL_SLAB) == 0


def test_checker_passes_on_correct_placement_and_restores():
    spec = _small("NBHD", 2)
    x = torch.arange(spec.L * 2 * spec.ntok * spec.H * spec.D, dtype=torch.int16).reshape(spec.L, 2, spec.ntok, spec.H, spec.D) + 1
    arena = _fresh()
    starts, img = fo.expected_windows(*spec.pieces(fo.to_bytes(x)), window=SMALL_WINDOW)
    fo.write_windows(arena, starts, img, SMALL_WINDOW)
    assert np.array_equal(_check(arena, spec, fo.to_bytes(x)), starts)
    fo.restore_windows(arena, starts, window=SMALL_WINDOW)
    assert fo.count_stray_words(arena, slab=SMALL_SLAB) == 0 and fo.first_stray(arena, [], window=SMALL_WINDOW, slab=SMALL_SLAB) is None
    # nothing expected at all (a refused call): passes on the untouched arena, names the offset of anything written
    none = (np.zeros(0, np.int64), np.zeros((0, 1), np.uint8))
    assert len(fo.check_arena(arena, *none, window=SMALL_WINDOW, slab=SMALL_SLAB)) == 0
    arena[777] = 1
    with pytest.raises(AssertionError, match="first stray byte at arena offset 0x309"):
        fo.check_arena(arena, *none, window=SMALL_WINDOW, slab=SMALL_SLAB)


def _placed_with(spec, x, move):
    """The arena with x placed by spec, the row of (layer 1, V, token 2, head 1) handled by move(offsets, index)."""
    off, data = spec.pieces(fo.to_bytes(x))
    i = int(np.ravel_multi_index((1, 1, 2, 1), (spec.L, 2, spec.ntok, spec.H)))
    true = int(off[i])
    off, data = move(off.copy(), data, i)
    arena = _fresh()
    for o, d in zip(off.tolist(), data):
        arena[o:o + len(d)] = torch.from_numpy(d.copy())
    return arena, true


def test_checker_names_the_offsets_of_a_row_one_block_low():
    spec = _small("NBHD", 2)
    x = torch.full((spec.L, 2, spec.ntok, spec.H, spec.D), 0x1234, dtype=torch.int16)

    def low(off, data, i):
        off[i] -= spec.stride_block  # token 2 lives in block 7; block 6 is nobody's
        return off, data
    arena, true = _placed_with(spec, x, low)
    with pytest.raises(AssertionError) as e:
        _check(arena, spec, fo.to_bytes(x))
    msg = str(e.value)
    assert f"arena offset {true:#x}: an expected byte is missing" in msg
    assert f"first stray byte at arena offset {true - spec.stride_block:#x}" in msg and "2 8-byte words" in msg


def test_checker_tells_a_dropped_row_and_a_wrapped_one():
    spec = _small("NBHD", 2)
    x = torch.full((spec.L, 2, spec.ntok, spec.H, spec.D), 0x1234, dtype=torch.int16)

    def drop(off, data, i):
        keep = np.arange(len(off)) != i
        return off[keep], data[keep]
    arena, true = _placed_with(spec, x, drop)
    with pytest.raises(AssertionError) as e:
        _check(arena, spec, fo.to_bytes(x))
    assert f"arena offset {true:#x}: an expected byte is missing" in str(e.value) and "the store was dropped" in str(e.value)
    # a stray byte alone, inside an expected window and outside all of them
    ok, _ = _placed_with(spec, x, lambda off, data, i: (off, data))
    _check(ok, spec, fo.to_bytes(x))
    beside = true - (true - spec.base) % 256 + 130  # behind the plane's 128 bytes of the block, in the same window
    ok[beside] = 0
    with pytest.raises(AssertionError, match=f"arena offset {beside:#x}: a byte beside the expected rows was written"):
        _check(ok, spec, fo.to_bytes(x))
    ok[beside] = fo.FILL
    ok[SMALL_ARENA - 5] = 0
    with pytest.raises(AssertionError, match=f"first stray byte at arena offset {SMALL_ARENA - 5:#x}"):
        _check(ok, spec, fo.to_bytes(x))
