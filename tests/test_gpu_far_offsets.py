"""The kernels' addressing past 2 GiB and 4 GiB from a plane's base (helpers and the layouts: tests/far_offsets.py).

One uint8 arena of 2 GiB (guard) + 4 GiB + 256 MiB is allocated once, filled with 0xA5, and every layout of this module is
a torch.as_strided view of it whose plane bases lie just behind the guard: paged caches whose used blocks sit at byte
offsets 0, on both sides of 2^31 and of 2^32 and at the arena's end, dense chunks whose planes lie 1.4 GiB apart, and the
widest head and token strides the decoder admits.  Every comparison is bit-exact against what the suite already trusts
(oracle.encode_blob / decode_blob, the fp8 tests' CPU formula, the rope tests' CPU formula, the bytes themselves for
copies), and after every call that writes, the arena is checked as a whole: the expected rows hold the expected bits and
every other byte still holds the fill pattern (far_offsets.check_arena names the first stray offset).  Only the touched
4 KiB windows are restored afterwards.

Which path a case takes follows from the mapping's shape (tests/test_far_offsets_host.py asserts the shapes): block size
16 in block-ordered runs gives the decoder's eight-token block path for bf16 -> bf16 / fp8 and the split copy's fast LDS
tiles; the swapped mappings and block size 12 give the one-token path (and lmc_tok_off's / dec_tok_off's division branch)
and the element path; a power-of-two block size under set_encode_path("fused") is k_encode_fused's PSRC instance, 12 the
generic one.

What the module found when it was written: the decoder's raw buffer stores are range-checked on scalar offset + lane
offset together (k_decode.h assumes the lane offset alone), so a destination whose head stride or whose chunk of rows
reached the descriptor's 0xfffffff0 only by that sum lost exactly the bytes behind it, silently.  The host now refuses
such destinations (lmc_api.hip: decode_dst_ok) and the limit tests at the end decode bit-exact AT the sum's limit.

Not covered: ELEMENT offsets above 2^32 of a 16-bit dtype need an 8 GiB plane; fp8, where an element is a byte, covers the
element-count crossings of 2^31 and 2^32 (16-bit elements cross 2^31 at 2^32 bytes here)."""
import ctypes

import numpy as np
import pytest
import torch

from lmcache_amd import native
from lmcache_amd.cache_engine import LMCacheEngine
from lmcache_amd.rope import RopeShift
from tests import far_offsets as fo
from tests.test_gpu_engine import dumb_metadata, generate_tokens, make_cfg
from tests.test_gpu_fp8 import _formula, _oracle_blob
from tests.test_gpu_parity import default_bins
from tests.test_rope_host import cpu_shift

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
L, H, D, T, CS = fo.L, fo.H, fo.D, fo.T, fo.CS
BINS = default_bins(L)
BF16, FP16, E4M3 = torch.bfloat16, torch.float16, torch.float8_e4m3fn
NAMES = {BF16: "bf16", FP16: "fp16", E4M3: "e4m3"}
MAPPINGS = [(16, False), (16, True), (12, False), (12, True)]
MAP_IDS = ["bs16_runs", "bs16_swapped", "bs12_runs", "bs12_swapped"]
INVALID = -1  # LMC_ERR_INVALID
ROPE_ROWS = 64


def _spec(s):
    assert fo.REGISTRY[s.name] is not None, "only layouts whose safety test_far_offsets_host.py has checked"
    return fo.REGISTRY[s.name]


# ------------------------------------------------------------------ the arena
@pytest.fixture(scope="module")
def arena():
    native.build()
    free, need = torch.cuda.mem_get_info()[0], fo.ARENA_BYTES + 4 * fo.GIB
    if free < need:
        pytest.skip(f"far-offset arena: {free} bytes of device memory are free, {need} are needed "
                    f"(the arena's {fo.ARENA_BYTES} + 4 GiB)")
    a = torch.full((fo.ARENA_BYTES,), fo.FILL, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    yield a
    del a
    torch.cuda.empty_cache()


class Far:
    """The arena and the windows a test has touched."""

    def __init__(self, arena):
        self.arena, self.touched = arena, []

    def layout(self, spec, dt, ntok=None):
        spec = _spec(spec)
        views = spec.views(self.arena, dt)
        if spec.paged:
            slots = torch.from_numpy(spec.slots[:ntok]).to(DEV)
            return native.KVLayout.paged(views, slots, spec.bs, spec.kind)
        return native.KVLayout.from_chunk(views, spec.kind)

    def place(self, spec, data, **sel):
        starts, img = fo.expected_windows(*_spec(spec).pieces(data, **sel))
        fo.write_windows(self.arena, starts, img)
        self.touched.append(starts)

    def check(self, what, *pairs):
        """pairs: (spec, data) or (spec, data, selection dict): together, everything the arena may hold."""
        torch.cuda.synchronize()
        offs, rows = [], []
        for spec, data, *sel in pairs:
            o, d = _spec(spec).pieces(data, **(sel[0] if sel else {}))
            byte = (o[:, None] + np.arange(d.shape[1], dtype=np.int64)).reshape(-1)
            offs.append(byte)
            rows.append(d.reshape(-1))
        if not pairs:
            offs, rows = [np.zeros(0, np.int64)], [np.zeros(0, np.uint8)]
        self.touched.append(fo.check_arena(self.arena, np.concatenate(offs), np.concatenate(rows).reshape(-1, 1), what))

    def restore(self):
        for starts in self.touched:
            fo.restore_windows(self.arena, starts)
        self.touched = []


@pytest.fixture
def far(arena):
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:  # a device fault is sticky: nothing more of this module may run on the device
        pytest.exit(f"the device reported an error before this test: {e}", returncode=3)
    f = Far(arena)
    yield f
    torch.cuda.synchronize()
    f.restore()
    if fo.count_stray_words(arena):  # a failed test must not fail the next one
        arena.fill_(fo.FILL)
    native.get_context(0).status(clear=True)


@pytest.fixture(scope="module")
def ctx():
    native.build()
    return native.get_context(0)


# ------------------------------------------------------------------ references, computed once and never written
_refs = {}


def _ref(oracle, dt):
    """The logical KV [L, 2, T, H, D] of dtype dt (CPU), its bytes, and the oracle's blobs of its chunks of CS tokens."""
    if dt not in _refs:
        g = torch.Generator().manual_seed(1000 + list(NAMES).index(dt))
        x = (torch.randn((L, 2, T, H, D), generator=g) * 4).clamp(-400, 400).to(dt)
        blobs = []
        for t0 in range(0, T, CS):
            part = x[:, :, t0:t0 + CS].reshape(L, 2, -1, H * D)
            if dt == E4M3:
                blobs.append(_oracle_blob(oracle, part, H, D, BINS))
            else:
                bits, code = oracle.torch_to_bits(part)
                blobs.append(oracle.encode_blob(bits, code, H, D, np.array(BINS, np.int32)))
        _refs[dt] = dict(x=x, bytes=fo.to_bytes(x), blobs=blobs)
    return _refs[dt]


_decoded, _device_blobs = {}, {}


def _decoded_bytes(oracle, src, dst, chunk=CS):
    """What the blobs of _ref(src) (or its one blob of T tokens) decode to in dtype dst: bytes [L, 2, T, H, D * esz]."""
    key = (src, dst, chunk)
    if key not in _decoded:
        ref = _ref(oracle, src)
        blobs = ref["blobs"] if chunk == CS else _one_blob(oracle, src)
        parts = []
        for i, b in enumerate(blobs):
            if dst == E4M3:
                part = ref["x"][:, :, i * chunk:(i + 1) * chunk].reshape(L, 2, -1, H * D)
                parts.append(_formula(oracle, part, BINS, dst).view(torch.uint8).numpy())
            else:
                code = oracle.BF16 if dst == BF16 else oracle.FP16
                parts.append(oracle.decode_blob(b, code).view(np.uint8))
        _decoded[key] = np.ascontiguousarray(np.concatenate(parts, axis=2)).reshape(L, 2, T, H, -1)
    return _decoded[key]


def _one_blob(oracle, dt):
    bits, code = oracle.torch_to_bits(_ref(oracle, dt)["x"].reshape(L, 2, T, H * D))
    return [oracle.encode_blob(bits, code, H, D, np.array(BINS, np.int32))]


def _blobs_on_device(oracle, dt, chunk=CS):
    """(device tensor, stride, pointer table) of the oracle's blobs, uploaded once."""
    key = (dt, chunk)
    if key not in _device_blobs:
        blobs = _ref(oracle, dt)["blobs"] if chunk == CS else _one_blob(oracle, dt)
        stride = native.r16(native.blob_bound(L, chunk, H, D))
        host = np.zeros(len(blobs) * stride, np.uint8)
        for i, b in enumerate(blobs):
            host[i * stride:i * stride + len(b)] = np.frombuffer(b, np.uint8)
        dev = torch.from_numpy(host).to(DEV)
        table = native.pointer_table([dev.data_ptr() + i * stride for i in range(len(blobs))], torch.device(DEV))
        _device_blobs[key] = (dev, stride, table, len(blobs))
    return _device_blobs[key]


def _encode(ctx, layout, path):
    stride = native.r16(native.blob_bound(L, CS, H, D))
    n = (T + CS - 1) // CS
    blobs = torch.zeros(n * stride, dtype=torch.uint8, device=DEV)
    sizes = torch.zeros(n, dtype=torch.int32, device=DEV)
    ctx.set_encode_path(path)
    try:
        ctx.encode_chunks(layout, 0, T, CS, BINS, blobs.data_ptr(), stride, sizes.data_ptr())
        torch.cuda.synchronize()
    finally:
        ctx.set_encode_path("auto")
    ctx.raise_on_status(f"encode ({path})")
    sz, host = sizes.cpu().tolist(), blobs.cpu().numpy()
    return [host[i * stride:i * stride + sz[i]].tobytes() for i in range(n)]


def _esz(dt):
    return dt.itemsize


def _decode_three_ways(oracle, ctx, far, spec, src, dst):
    """lmc_decode_chunks of all tokens, with a trimmed first chunk (dst_tok0 = -3), and lmc_decode_chunks_layers of layer 1:
    after each the arena holds the oracle's decode at the layout's rows and the fill pattern everywhere else."""
    dev, stride, table, n = _blobs_on_device(oracle, src)
    want = _decoded_bytes(oracle, src, dst)
    what = f"{spec.name} {NAMES[src]}->{NAMES[dst]}"
    ctx.decode_chunks(dev.data_ptr(), stride, n, far.layout(spec, dst), 0, CS)
    far.check(what, (spec, want))
    ctx.raise_on_status(what)
    far.restore()
    ctx.decode_chunks(dev.data_ptr(), stride, n, far.layout(spec, dst, T - 3), -3, CS)
    far.check(what + ", first chunk trimmed by 3", (spec, want[:, :, 3:], dict(tok=slice(0, T - 3))))
    ctx.raise_on_status(what)
    far.restore()
    ctx.decode_chunks_layers(table.data_ptr(), stride, n, far.layout(spec, dst), 0, CS, 1, 1)
    far.check(what + ", layer 1 only", (spec, want[1:2], dict(layers=slice(1, 2))))
    ctx.raise_on_status(what)


def test_the_arena_check_sees_a_wrapped_row_and_a_stray_byte_anywhere(oracle, far):
    """The checker on the device arena itself: the rows of the arena's last block written 2^32 bytes low (nobody's block)
    are named as missing here and stray there, and one byte at the arena's very end is found."""
    spec = _spec(fo.paged_rows("NBHD", 2, 16, False))
    data = _ref(oracle, BF16)["bytes"]
    off, rows = spec.pieces(data)
    wrapped = np.where(off - spec.base >= (fo.NUM_BLOCKS - 1) * fo.STRIDE_BLOCK, off - (1 << 32), off)
    assert 0 < (wrapped != off).sum() < len(off)
    starts, img = fo.expected_windows(wrapped, rows)
    fo.write_windows(far.arena, starts, img)
    far.touched.append(starts)
    first_high = int(off[wrapped != off].min())
    with pytest.raises(AssertionError) as e:
        far.check("wrapped", (spec, data))
    assert f"arena offset {first_high:#x}: an expected byte is missing" in str(e.value)
    assert f"first stray byte at arena offset {first_high - (1 << 32):#x} = an expected window's address minus 2^32" in str(e.value)
    far.restore()
    far.check("clean again")
    far.arena[fo.ARENA_BYTES - 1] = 0
    with pytest.raises(AssertionError, match=f"first stray byte at arena offset {fo.ARENA_BYTES - 1:#x}"):
        far.check("one byte at the end")
    far.arena[fo.ARENA_BYTES - 1] = fo.FILL
    far.check("clean again")


# ------------------------------------------------------------------ the codec on far paged rows
@pytest.mark.parametrize("mapping", MAPPINGS, ids=MAP_IDS)
@pytest.mark.parametrize("dt", [BF16, FP16, E4M3], ids=["bf16", "fp16", "e4m3"])
@pytest.mark.parametrize("kind", ["NBHD", "NHBD"])
def test_encode_from_far_paged_rows(oracle, ctx, far, kind, dt, mapping):
    spec = fo.paged_rows(kind, _esz(dt), *mapping)
    ref = _ref(oracle, dt)
    far.place(spec, ref["bytes"])
    layout = far.layout(spec, dt)
    assert layout.vector_readable()
    for path in ("two_kernels", "fused"):
        for i, (got, want) in enumerate(zip(_encode(ctx, layout, path), ref["blobs"])):
            assert got == want, f"{spec.name} {path}: blob of chunk {i} differs from the oracle's blob of the gathered rows"
    far.check(spec.name + ": the encoders write nothing", (spec, ref["bytes"]))


@pytest.mark.parametrize("mapping", MAPPINGS, ids=MAP_IDS)
@pytest.mark.parametrize("src,dst", [(BF16, BF16), (BF16, FP16), (BF16, E4M3), (FP16, FP16)],
                         ids=["bf16_bf16", "bf16_fp16", "bf16_e4m3", "fp16_fp16"])
@pytest.mark.parametrize("kind", ["NBHD", "NHBD"])
def test_decode_into_far_paged_rows(oracle, ctx, far, kind, src, dst, mapping):
    _decode_three_ways(oracle, ctx, far, fo.paged_rows(kind, _esz(dst), *mapping), src, dst)


# ------------------------------------------------------------------ dense chunks whose planes lie 1.4 GiB apart
@pytest.mark.parametrize("dt", [BF16, E4M3], ids=["bf16", "e4m3"])
def test_encode_from_a_dense_view_with_far_planes(oracle, ctx, far, dt):
    spec = fo.dense("vllm", _esz(dt))
    ref = _ref(oracle, dt)
    far.place(spec, ref["bytes"])
    layout = far.layout(spec, dt)
    assert layout.vector_readable() and layout.struct.stride_layer * _esz(dt) == 2 * fo.PLANE_FAR
    for path in ("two_kernels", "fused"):
        assert _encode(ctx, layout, path) == ref["blobs"], f"{spec.name} {path}"
    far.check(spec.name + ": the encoders write nothing", (spec, ref["bytes"]))


@pytest.mark.parametrize("kind,src,dst", [("vllm", BF16, BF16), ("vllm", BF16, E4M3), ("vllm", FP16, FP16),
                                          ("huggingface", BF16, BF16), ("huggingface", BF16, FP16), ("huggingface", BF16, E4M3)],
                         ids=lambda v: v if isinstance(v, str) else NAMES[v])
def test_decode_into_a_dense_view_with_far_planes(oracle, ctx, far, kind, src, dst):
    _decode_three_ways(oracle, ctx, far, fo.dense(kind, _esz(dst)), src, dst)


# ------------------------------------------------------------------ lmc_copy_kv
def _near_chunk(dt, g, aligned):
    """A small ordinary vllm chunk of random bit patterns; not aligned: 2 bytes off a 16-byte boundary (element kernels)."""
    n = L * 2 * T * H * D
    skip = 2 // _esz(dt)
    flat = torch.randint(0, 256, ((n + 16) * _esz(dt),), generator=g, dtype=torch.uint8).view(dt).to(DEV)
    chunk = (flat[:n] if aligned else flat[skip:skip + n]).view(L, 2, T, H, D)
    assert chunk.data_ptr() % 16 == (0 if aligned else 2)
    return chunk


FAR_SIDES = [("NBHD", 16, True), ("NHBD", 12, False), ("vllm",)]


@pytest.mark.parametrize("side", FAR_SIDES, ids=["NBHD_bs16_swapped", "NHBD_bs12_runs", "dense_vllm"])
@pytest.mark.parametrize("kernel", ["k_copy_kv", "k_copy_kv_elem", "k_copy_kv_b8", "k_copy_kv_elem_b8"])
def test_copy_kv_with_the_far_side_as_source_and_as_destination(ctx, far, kernel, side):
    dt = E4M3 if kernel.endswith("b8") else BF16
    vec = "elem" not in kernel
    spec = fo.dense(side[0], _esz(dt)) if len(side) == 1 else fo.paged_rows(side[0], _esz(dt), side[1], side[2])
    g = torch.Generator().manual_seed(len(kernel))
    data = _near_chunk(dt, g, True).cpu()
    far.place(spec, fo.to_bytes(data))
    layout = far.layout(spec, dt)
    near = _near_chunk(dt, g, vec)
    near_layout = native.KVLayout.from_chunk(near, "vllm")
    # lmc_copy_kv takes the vector kernel exactly when both sides are vector-readable
    assert layout.vector_readable() and near_layout.vector_readable() == vec
    ctx.copy_kv(layout, 0, T, near_layout, 0)
    far.check(f"{kernel} from {spec.name}: the source keeps its bytes", (spec, fo.to_bytes(data)))
    assert np.array_equal(fo.to_bytes(near), fo.to_bytes(data)), f"{kernel} from {spec.name}"
    far.restore()
    fresh = _near_chunk(dt, g, vec)
    ctx.copy_kv(native.KVLayout.from_chunk(fresh, "vllm"), 0, T, layout, 0)
    far.check(f"{kernel} into {spec.name}", (spec, fo.to_bytes(fresh)))


@pytest.mark.parametrize("swapped", [False, True], ids=["runs_fast_tiles", "swapped_element_path"])
@pytest.mark.parametrize("dt", [BF16, E4M3], ids=["bf16", "e4m3"])
def test_copy_split_gathers_from_and_scatters_into_a_far_nhdb_cache(ctx, far, dt, swapped):
    spec = fo.paged_split(_esz(dt), swapped)
    g = torch.Generator().manual_seed(40 + swapped)
    data = _near_chunk(dt, g, True).cpu()
    far.place(spec, fo.to_bytes(data))
    layout = far.layout(spec, dt)
    assert layout.struct.paged_kind == native.PAGED_SPLIT and layout.struct.stride_block * _esz(dt) == fo.STRIDE_BLOCK
    near = torch.zeros((L, 2, T, H, D), dtype=torch.uint8, device=DEV).view(dt) if dt == E4M3 else torch.zeros((L, 2, T, H, D), dtype=dt, device=DEV)
    ctx.copy_kv(layout, 0, T, native.KVLayout.from_chunk(near, "vllm"), 0)
    far.check(f"gather from {spec.name}: the source keeps its bytes", (spec, fo.to_bytes(data)))
    assert np.array_equal(fo.to_bytes(near), fo.to_bytes(data)), f"gather from {spec.name} (K and V planes)"
    far.restore()
    fresh = _near_chunk(dt, g, True)
    ctx.copy_kv(native.KVLayout.from_chunk(fresh, "vllm"), 0, T, layout, 0)
    far.check(f"scatter into {spec.name}", (spec, fo.to_bytes(fresh)))


# ------------------------------------------------------------------ lmc_rope_shift in place
_tables = {}


def _table(rot):
    if rot not in _tables:
        t = RopeShift.from_base(10000.0, rot, ROPE_ROWS, DEV).cos_sin
        _tables[rot] = (t, t.cpu())
    return _tables[rot]


@pytest.mark.parametrize("rot", [64, 24], ids=["vector_form", "element_form"])
@pytest.mark.parametrize("side", FAR_SIDES, ids=["NBHD_bs16_swapped", "NHBD_bs12_runs", "dense_vllm"])
@pytest.mark.parametrize("dt", [BF16, FP16], ids=["bf16", "fp16"])
def test_rope_shift_in_place_on_far_rows(oracle, ctx, far, dt, side, rot):
    """rot 64 (NeoX, whole 16-byte vectors) is k_rope_vec, rot 24 k_rope_elem; one uniform delta, then per-token deltas on
    what the first left.  V and the channels behind rot keep their bits."""
    spec = fo.dense(side[0], 2) if len(side) == 1 else fo.paged_rows(side[0], 2, side[1], side[2])
    x = _ref(oracle, dt)["x"].clone()
    far.place(spec, fo.to_bytes(x))
    layout = far.layout(spec, dt)
    table, table_cpu = _table(rot)
    ctx.rope_shift(layout, 0, T, table, rot, True, delta=-9)
    x[:, 0] = cpu_shift(x[:, 0], table_cpu, torch.full((T,), -9), rot, True)
    far.check(f"{spec.name} rot {rot}: uniform delta", (spec, fo.to_bytes(x)))
    deltas = torch.randint(-(ROPE_ROWS - 1), ROPE_ROWS, (T,), generator=torch.Generator().manual_seed(rot), dtype=torch.int32)
    ctx.rope_shift(layout, 0, T, table, rot, True, deltas=deltas.to(DEV))
    x[:, 0] = cpu_shift(x[:, 0], table_cpu, deltas, rot, True)
    far.check(f"{spec.name} rot {rot}: per-token deltas", (spec, fo.to_bytes(x)))
    assert ctx.status(clear=True) == 0


# ------------------------------------------------------------------ the engine on far caches
def _small_rows(x, slots, bs):
    """An ordinary NBHD cache of nine blocks that holds x [L, 2, T, H, D] at `slots`."""
    caches = [torch.zeros((2, len(fo.BLOCKS), bs, H, D), dtype=x.dtype, device=DEV) for _ in range(L)]
    for c, xl in zip(caches, x.to(DEV)):
        c[:, slots // bs, slots % bs] = xl
    return caches


@pytest.mark.parametrize("with_rope", [False, True], ids=["plain", "rope"])
def test_engine_store_paged_and_retrieve_into_paged_on_far_caches(oracle, far, with_rope):
    """store_paged from far NBHD rows and retrieve_into_paged into far NHBD rows of another mapping (cachegen-host) leave
    in the arena exactly what the same two calls leave in small ordinary caches that hold the same rows."""
    bs, dt = 16, BF16
    src, dst = fo.paged_rows("NBHD", 2, bs, False), fo.paged_rows("NHBD", 2, bs, True)
    x = _ref(oracle, dt)["x"]
    tokens = generate_tokens(T, DEV)
    # the small twins: block BLOCKS[i] of the far mapping is block i here
    rank = {b: i for i, b in enumerate(fo.BLOCKS)}
    small = lambda spec: torch.tensor([rank[int(s) // bs] * bs + int(s) % bs for s in spec.slots], device=DEV)
    rope = RopeShift.from_base(10000.0, D, 128, DEV, delta=37) if with_rope else None
    e_far = LMCacheEngine(make_cfg("cachegen-host", CS), dumb_metadata("vllm", "Llama-3-8B"))
    e_small = LMCacheEngine(make_cfg("cachegen-host", CS), dumb_metadata("vllm", "Llama-3-8B"))
    try:
        far.place(src, fo.to_bytes(x))
        e_far.store_paged(tokens, src.views(far.arena, dt), torch.from_numpy(src.slots).to(DEV), bs, "NBHD")
        far.check("store_paged reads only", (src, fo.to_bytes(x)))
        far.restore()
        e_small.store_paged(tokens, _small_rows(x, small(src), bs), small(src), bs, "NBHD")
        twin = [torch.zeros((2, len(fo.BLOCKS), H, bs, D), dtype=dt, device=DEV) for _ in range(L)]
        m_small = e_small.retrieve_into_paged(tokens, twin, small(dst), bs, "NHBD", rope=rope)
        m_far = e_far.retrieve_into_paged(tokens, dst.views(far.arena, dt), torch.from_numpy(dst.slots).to(DEV), bs, "NHBD", rope=rope)
        torch.cuda.synchronize()
        assert torch.equal(m_far, m_small) and bool(m_far.all())
        sl = small(dst)
        got = torch.stack([c[:, sl // bs, :, sl % bs].permute(1, 0, 2, 3) for c in twin])  # [L, 2, T, H, D]
        assert bool(got.ne(0).any()) and not np.array_equal(fo.to_bytes(got), fo.to_bytes(x))  # retrieved, and lossy
        far.check("retrieve_into_paged" + (" with rope" if with_rope else ""), (dst, fo.to_bytes(got)))
        assert native.get_context(0).status(clear=True) == 0
    finally:
        e_far.close()
        e_small.close()


# ------------------------------------------------------------------ the decoder's 32-bit store offsets: the host's guard
def _struct(arena, spec, dt):
    """The lmc_kv_layout of a dense spec, written field by field (strides that torch.as_strided refuses included)."""
    e = spec.esz
    s = native.KvLayoutStruct()
    s.dtype, s.num_layers, s.num_heads, s.head_size = native.dtype_code(dt), spec.L, spec.H, spec.D
    s.base = arena.data_ptr() + spec.base
    sl, skv = int(spec.plane_off[2] - spec.plane_off[0]), int(spec.plane_off[1] - spec.plane_off[0])
    s.stride_layer, s.stride_kv, s.stride_token, s.stride_head = sl // e, skv // e, spec.stride_token // e, spec.stride_head // e
    return s


LIMITS = {"head": fo.head_stride_limit, "token": fo.token_stride_limit, "paged_head": fo.paged_head_stride_limit}


@pytest.mark.parametrize("dst", [BF16, E4M3], ids=["bf16", "e4m3"])
@pytest.mark.parametrize("limit", list(LIMITS))
def test_the_largest_admitted_strides_decode_bit_exact(oracle, ctx, far, limit, dst):
    """The store's range covers scalar offset + lane offset (lmc_api.hip: decode_dst_ok).  head: H = 2, the last channel of
    the second head of a chunk's LAST row ends exactly at the range; token: T = 104 rows of one chunk, the last row ending
    as far out as the range reaches; paged_head: the same for the eighth row of the paged block path.  All are views the
    binding builds, and all decode bit-exact (bf16 and fp8 take the eight-token path, whose scalar offset is the largest)."""
    spec = LIMITS[limit](_esz(dst))
    assert fo.decode_dst_ok(spec, spec.chunk) and not fo.decode_dst_ok(LIMITS[limit](_esz(dst), 1), spec.chunk)
    dev, stride, _, n = _blobs_on_device(oracle, BF16, spec.chunk)
    layout = far.layout(spec, dst)
    if not spec.paged:
        made, want = layout.struct, _struct(far.arena, spec, dst)
        assert (made.base, made.stride_layer, made.stride_kv, made.stride_token, made.stride_head) == \
            (want.base, want.stride_layer, want.stride_kv, want.stride_token, want.stride_head)
    ctx.decode_chunks(dev.data_ptr(), stride, n, layout, 0, spec.chunk)
    far.check(spec.name, (spec, _decoded_bytes(oracle, BF16, dst, spec.chunk)))
    ctx.raise_on_status(spec.name)


def _pinned(data: bytes):
    buf = native.PinnedBuffer(native.r16(len(data)))
    ctypes.memmove(buf.ptr, data, len(data))
    return buf


def _decode_entry_points(oracle, ctx, chunk):
    """The five entry points that launch k_decode with a destination (the layer-wise load is lmc_load_chunks /
    lmc_load_pack with layers_per_range), each as rc = call(layout struct), on valid blobs of chunk length `chunk`."""
    lib, ref = native.lib(), ctypes.byref
    st = native.current_stream_ptr(torch.device(DEV))
    dev, stride, table, n = _blobs_on_device(oracle, BF16, chunk)
    blobs = _ref(oracle, BF16)["blobs"] if chunk == CS else _one_blob(oracle, BF16)
    host = [_pinned(b) for b in blobs]
    ptrs = (ctypes.c_void_p * n)(*[h.ptr for h in host])
    sizes = (ctypes.c_uint32 * n)(*[len(b) for b in blobs])
    pack_bytes = oracle.pack_from_blobs(blobs, chunk)
    pack = _pinned(pack_bytes)
    ends = (ctypes.c_int32 * 2)(1, L)
    calls = {
        "lmc_decode_chunks": lambda s: lib.lmc_decode_chunks(ctx.handle, dev.data_ptr(), stride, n, ref(s), 0, chunk, None, st),
        "lmc_decode_chunks_layers": lambda s: lib.lmc_decode_chunks_layers(ctx.handle, table.data_ptr(), stride, n, ref(s), 0, chunk,
                                                                          0, L, None, st),
        "lmc_decode_chunks_schedule": lambda s: lib.lmc_decode_chunks_schedule(ctx.handle, table.data_ptr(), stride, n, ref(s), 0, chunk,
                                                                              2, ends, None, None, st),
        "lmc_load_chunks": lambda s: lib.lmc_load_chunks(ctx.handle, ptrs, sizes, n, ref(s), 0, chunk, 0, None, None, st),
        "lmc_load_chunks (layer-wise)": lambda s: lib.lmc_load_chunks(ctx.handle, ptrs, sizes, n, ref(s), 0, chunk, 1, None, None, st),
        "lmc_load_pack": lambda s: lib.lmc_load_pack(ctx.handle, pack.ptr, len(pack_bytes), 0, 0, ref(s), 0, 0, None, None, st),
        "lmc_load_pack (layer-wise)": lambda s: lib.lmc_load_pack(ctx.handle, pack.ptr, len(pack_bytes), 0, 0, ref(s), 0, 1, None, None, st),
    }
    return calls, host + [pack]


@pytest.mark.parametrize("limit", list(LIMITS))
def test_every_decode_entry_point_admits_the_limit_and_refuses_the_first_value_behind_it(oracle, ctx, far, limit):
    """At the limit every entry point decodes bit-exact; one element more of stride, or a negative stride, and each returns
    LMC_ERR_INVALID, launches nothing and leaves the arena's fill intact."""
    ok, over = LIMITS[limit](2, 0), LIMITS[limit](2, 1)
    neg = fo.negative_stride("token" if limit == "token" else "head")
    alive = []

    def struct(spec):
        if not spec.paged:
            return _struct(far.arena, _spec(spec), BF16)
        alive.append(far.layout(spec, BF16))
        return alive[-1].struct

    calls, keep = _decode_entry_points(oracle, ctx, ok.chunk)
    try:
        want = _decoded_bytes(oracle, BF16, BF16, ok.chunk)
        for name, call in calls.items():
            assert call(struct(ok)) == 0, name
            far.check(f"{name} at the {limit} stride limit", (ok, want))
            far.restore()
        small_calls, keep2 = (calls, []) if ok.chunk == CS else _decode_entry_points(oracle, ctx, CS)
        keep += keep2
        for name, call in calls.items():
            assert call(struct(over)) == INVALID, f"{name}: first refused {limit} stride"
        for name, call in small_calls.items():  # (the negative strides are chunks of CS tokens)
            assert call(struct(neg)) == INVALID, f"{name}: negative stride"
        if ok.paged:  # a negative stride is refused with a slot mapping too
            for field in ("stride_token", "stride_head"):
                s = native.KvLayoutStruct.from_buffer_copy(struct(ok))
                setattr(s, field, -getattr(s, field))
                assert calls["lmc_decode_chunks"](s) == INVALID, field
        far.check(f"refused {limit} strides launch nothing")
        assert ctx.status(clear=True) == 0
    finally:
        torch.cuda.synchronize()
        for b in keep:
            b.free()
