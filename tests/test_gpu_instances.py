"""One small parity case per kernel instance that lmc_api.hip picks from a plane width, a dtype or a source / destination
kind: k_quantize, k_encode_fused, k_fixed_encode, k_decode, k_fixed_decode.

The host picks the instance (with_plane_width, with_kv_dtype / with_kv_dtype16, with_decode_kind, with_bool, with_int); a
plane sent to the wrong rung drops or repeats channels, a dtype sent to its neighbour's instance decodes to other bits.
Every case goes through the public entry point that reaches its instance and compares BYTES with the CPU oracle
(oracle.encode_blob / oracle.quantize / oracle.decode_blob; fixed-width blobs: tests/fixed_model.py).  There is no
tolerance anywhere.

Shapes are the smallest at which the pick can go wrong: one layer, 32 + 5 tokens in chunks of 32 (a full chunk, which the
fused kernel takes, and a ragged one), a nibble and a wide plane, randn data with a zero row and the row's largest values
in its LAST 8 channels (a dropped vector changes the scale of the whole row), and plane widths at both ends of every rung:
8, 128 | 136, 256 | 264, 512 | 520, 1024 and, where the entry point takes wide planes, 1032, 2048 | 2056, 4096.  Where a
layout does not admit a width (an fp8 NHDB cache needs head_size % 16 == 0) the next one it admits stands in.  Arenas and
destinations are canary-filled and compared whole.

MATRIX (below, data) names for every instance the cases that launch it; tests/test_instance_inventory_host.py holds it
against the build's instance list without a GPU, so an instance added without a case fails there.  UNREACHABLE lists the
instances the library holds and no call can launch, each with the line of lmc_api.hip that builds it."""
import ctypes
import struct

import numpy as np
import pytest
import torch

from lmcache_amd import native
from tests import fixed_model as fm
from tests.test_gpu_paged_split import _ibits, _torch_gather, _torch_scatter

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CS, NTOK, BS = 32, 37, 16
POISON, GUARD = 0xA5, 256
DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}
CODE = {"bf16": 0, "fp16": 1, "e4m3": 2, "e5m2": 3}  # include/lmc_format.h: LMC_DTYPE_*
DT16, DT_ALL = ["bf16", "fp16"], ["bf16", "fp16", "e4m3", "e5m2"]
FMAX = {"e4m3": 448.0, "e5m2": 57344.0}
WIDE_BINS, NIBBLE_BINS = [32, 20, 24], [16, 12, 17]  # 5-bit and 4-bit symbols (tests/fixed_model.py: NARROW_BINS)
KINDS = ["rows", "paged", "split"]  # k_decode.h: DEC_ROWS, DEC_PAGED_ROWS, DEC_PAGED_SPLIT

# (G lanes per row, NITER channel runs per lane) of with_plane_width and the widths at the rung's two ends ...
RUNGS = [((16, 1), (8, 128)), ((32, 1), (136, 256)), ((64, 1), (264, 512)), ((64, 2), (520, 1024))]
# ... the wide planes of lmc_quantize (NITER 4 / 8) and of the two-kernel and fixed-width encodes (SPLIT 2 / 4 waves per oct)
WIDE_WIDTHS = [(1032, 2048), (2056, 4096)]
FP8_SPLIT_WIDTHS = [(16, 128), (144, 256), (272, 512), (528, 1024)]  # an fp8 NHDB cache: head_size % 16 == 0
HD = {8: (1, 8), 16: (1, 16), 128: (2, 64), 136: (17, 8), 144: (9, 16), 256: (2, 128), 264: (3, 88), 272: (17, 16),
      512: (4, 128), 520: (5, 104), 528: (3, 176), 1024: (8, 128), 1032: (3, 344), 2048: (16, 128), 2056: (257, 8),
      4096: (32, 128)}
# the layer-wise fixed-width job: tokens of one pass of a plane per rung (k_fixed_encode: 8 waves take 32, 16 or 8 row octs)
PASS_TOKENS = [256, 128, 64, 64]

MATRIX = {}  # (family, template arguments) -> [case ids]
UNREACHABLE = {  # instance -> the line of lmcache_amd/csrc/lmc_api.hip that builds it (launch_quant_dt, instantiated with QUAD = true)
    **{("k_quantize", (64, 4, dt, True, 1, False)): "if (C <= 2048) launch(g64, IntTag<4>{}, IntTag<1>{});" for dt in range(4)},
    **{("k_quantize", (64, 8, dt, True, 1, False)): "else launch(g64, IntTag<8>{}, IntTag<1>{});" for dt in range(4)},
}


def _case(cid, values, *instances):
    """A pytest.param with id `cid` that is entered in MATRIX under every instance it launches."""
    for inst in instances:
        MATRIX.setdefault(inst, []).append(cid)
    return pytest.param(*values, id=cid)


def _rung_cases(prefix, rungs, dts, inst):
    return [_case(f"{prefix}-G{g}N{n}-C{w[0]}_{w[1]}-{dt}", (w, dt), inst(g, n, k, CODE[dt]))
            for k, ((g, n), w) in enumerate(rungs) for dt in dts]


ALL_RUNGS = RUNGS + [((64, 4), WIDE_WIDTHS[0]), ((64, 8), WIDE_WIDTHS[1])]
QUANT = _rung_cases("quantize", ALL_RUNGS, DT_ALL, lambda g, n, k, dt: ("k_quantize", (g, n, dt, False, 1, False)))
# QUAD = true: a wide plane is NITER 2 with SPLIT 2 / 4 waves to a row oct
SPLIT_RUNGS = RUNGS + [((64, 2), WIDE_WIDTHS[0]), ((64, 2), WIDE_WIDTHS[1])]
TWO_KERNEL = _rung_cases("two_kernel", SPLIT_RUNGS, DT_ALL,
                         lambda g, n, k, dt: ("k_quantize", (g, n, dt, True, (1, 1, 1, 1, 2, 4)[k], False)))
NHDB_ENCODE = [_case(f"nhdb-G{g}N{n}-{dt}", ((FP8_SPLIT_WIDTHS[k] if CODE[dt] >= 2 else w), dt),
                     ("k_quantize", (g, n, CODE[dt], True, 1, True)))
               for k, ((g, n), w) in enumerate(RUNGS) for dt in DT_ALL]
FUSED = [_case(f"fused-G{g}N{n}-C{w[0]}_{w[1]}-{dt}-{src}", (w, dt, src),
               ("k_encode_fused", (g, n, CODE[dt], 8, src == "paged16")))
         for (g, n), w in RUNGS for dt in DT_ALL for src in ("rows", "paged16")]
FUSED_BS12 = [_case("fused-paged12-C136-bf16", (136, "bf16"), ("k_encode_fused", (32, 1, 0, 8, False)))]
FIXED = _rung_cases("fixed", SPLIT_RUNGS, DT16,
                    lambda g, n, k, dt: ("k_fixed_encode", (g, n, dt, (1, 1, 1, 1, 2, 4)[k], False, False)))
FIXED_SPLIT = _rung_cases("fixed_nhdb", RUNGS, DT16, lambda g, n, k, dt: ("k_fixed_encode", (g, n, dt, 1, True, False)))
LAYERWISE = [_case(f"layerwise-G{g}N{n}-C{w[0]}_{w[1]}-{dt}-{src}", (k, w, dt, src),
                   ("k_fixed_encode", (g, n, CODE[dt], 1, src == "nhdb", True)))
             for k, ((g, n), w) in enumerate(RUNGS) for dt in DT16 for src in ("rows", "nhdb")]
DECODE = [_case(f"decode-{dt}-{kind}", (dt, kind), ("k_decode", (0, CODE[dt], KINDS.index(kind)))) for dt in DT_ALL for kind in KINDS]
# (the two sinks that are no KV have one instance each and a test of their own, entered under the test's name)
MATRIX[("k_decode", (1, 0, 0))] = ["test_decode_symbols_sink_equals_the_oracles_symbols"]
MATRIX[("k_decode", (2, 0, 0))] = ["test_decode_fixed_sink_equals_the_model"]
FIXED_DECODE = [_case(f"fixed_decode-{dt}-{kind}", (dt, kind), ("k_fixed_decode", (CODE[dt], KINDS.index(kind))))
                for dt in DT16 for kind in KINDS]


# ------------------------------------------------------------------ data, sources, references
@pytest.fixture(scope="module")
def ctx():
    native.build()
    c = native.get_context(0)
    yield c
    c.set_encode_path("auto")
    c.set_fixed_layer_slices(0)


def _bins(C, dt, nl=1):
    """A nibble plane beside a wide one, which of them the keys get and their symbol counts walking with the case."""
    i = C // 8 + CODE[dt]
    pair = [WIDE_BINS[i % 3], NIBBLE_BINS[(i // 3) % 3]]
    return [pair[(i + p) % 2] for p in range(2 * nl)]


def _kv(C, dt, ntok=NTOK, nl=1):
    """[nl, 2, ntok, H, D] of dt (CPU): randn, token 3 all zero, every row's last 8 channels three times as large."""
    H, D = HD[C]
    g = torch.Generator().manual_seed(16 * C + CODE[dt])
    x = torch.randn((nl, 2, ntok, C), generator=g)
    x[..., C - 8:] *= 3.0
    x[:, :, 3] = 0
    if dt in FMAX:
        x = x.clamp(-FMAX[dt], FMAX[dt])
    return x.to(DT[dt]).reshape(nl, 2, ntok, H, D)


def _bits(oracle, x):
    """(uint16 [L, 2, T, C], dtype code) of what the encoders code of x [L, 2, T, H, D]: an fp8 chunk is coded as its bf16
    images (include/lmc_format.h)."""
    v = x.reshape(x.shape[0], 2, x.shape[2], -1)
    return oracle.torch_to_bits(v.to(torch.bfloat16) if v.dtype.itemsize == 1 else v)


def _coded_refs(oracle, x, bins, cs=CS):
    """The oracle's coded blob of every chunk of x; an fp8 chunk's header word 23 holds the fp8 code."""
    H, D = x.shape[3], x.shape[4]
    out = []
    for t0 in range(0, x.shape[2], cs):
        bits, code = _bits(oracle, x[:, :, t0:t0 + cs])
        b = oracle.encode_blob(bits, code, H, D, np.array(bins, np.int32))
        if x.dtype.itemsize == 1:
            b = b[:92] + struct.pack("<I", native.dtype_code(x.dtype)) + b[96:]
        out.append(b)
    return out


def _fixed_refs(oracle, x, bins, cs=CS):
    H, D = x.shape[3], x.shape[4]
    out = []
    for t0 in range(0, x.shape[2], cs):
        bits, code = _bits(oracle, x[:, :, t0:t0 + cs])
        out.append(fm.encode_blob(oracle, bits, code, H, D, np.array(bins, np.int32)))
    return out


def _canary(shape, dt):
    """A tensor of dt whose every byte is 0x5A (a finite value in all four formats)."""
    return torch.full(shape, 0x5A5A if dt.itemsize == 2 else 0x5A, dtype=torch.int16 if dt.itemsize == 2 else torch.uint8).view(dt)


def _slots(ntok, nb, bs, seed):
    return torch.randperm(nb * bs, generator=torch.Generator().manual_seed(seed))[:ntok]


def _rows_src(x):
    return native.KVLayout.from_chunk(x.to(DEV), "vllm"), x


def _paged_rows_src(x, bs):
    """x in an NBHD paged cache at random slots -> (layout, the chunk gathered back on the host)."""
    nl, _, T, H, D = x.shape
    nb = (T + bs - 1) // bs + 2
    slots = _slots(T, nb, bs, T + H)
    caches = [_canary((2, nb, bs, H, D), x.dtype) for _ in range(nl)]
    for l in range(nl):
        _ibits(caches[l])[:, slots // bs, slots % bs] = _ibits(x[l])
    back = torch.stack([_ibits(c)[:, slots // bs, slots % bs] for c in caches]).view(x.dtype)
    return native.KVLayout.paged([c.to(DEV) for c in caches], slots.to(DEV), bs, "NBHD"), back


def _nhdb_src(x, bs=BS):
    """x in an NHDB cache (LMC_PAGED_SPLIT) at random slots -> (layout, the chunk gathered on the host by torch indexing)."""
    nl, _, T, H, D = x.shape
    nb = (T + bs - 1) // bs + 2
    slots = _slots(T, nb, bs, T + D)
    caches = [_canary((2, nb, H, D, bs), x.dtype) for _ in range(nl)]
    _torch_scatter(caches, _ibits(x), slots, bs)
    back = _torch_gather(caches, slots, bs).view(x.dtype).contiguous()
    return native.KVLayout.paged([c.to(DEV) for c in caches], slots.to(DEV), bs, "NHDB"), back


class _Arena:
    """The blob arena of one encode job, 0xA5 everywhere and GUARD bytes longer than its slots, and its size words."""

    def __init__(self, nl, H, D, cs, ntok):
        self.n = (ntok + cs - 1) // cs
        self.stride = native.r16(native.blob_bound(nl, cs, H, D))
        self.blobs = torch.full((self.n * self.stride + GUARD,), POISON, dtype=torch.uint8, device=DEV)
        self.sizes = torch.full((self.n,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
        self.table = torch.tensor([self.blobs.data_ptr() + i * self.stride for i in range(self.n)], dtype=torch.int64).to(DEV)

    def read(self, pad16):
        """-> the blobs' bytes.  Nothing behind a blob's end was written: from its size on (a coded blob, pad16: from its
        size rounded up to 16, what the coder's zero fill owns) to the end of its slot, and the guard behind the slots."""
        torch.cuda.synchronize()
        sz, host = self.sizes.cpu().tolist(), self.blobs.cpu().numpy()
        assert (host[self.n * self.stride:] == POISON).all(), "bytes behind the arena's slots were written"
        out = []
        for i in range(self.n):
            assert 0 < sz[i] <= self.stride, (i, sz[i])
            end = native.r16(sz[i]) if pad16 else sz[i]
            assert (host[i * self.stride + end:(i + 1) * self.stride] == POISON).all(), f"chunk {i}: bytes behind the blob were written"
            out.append(host[i * self.stride:i * self.stride + sz[i]].tobytes())
        return out


def _encode(ctx, fn, layout, bins, ntok=NTOK, cs=CS, coded=True):
    a = _Arena(layout.L, layout.H, layout.D, cs, ntok)
    fn(layout, 0, ntok, cs, bins, a.blobs.data_ptr(), a.stride, a.sizes.data_ptr())
    blobs = a.read(pad16=coded)
    ctx.raise_on_status("encode")
    return blobs, a


def _same_blobs(got, want, what):
    assert [len(b) for b in got] == [len(b) for b in want], what
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{what}: chunk {i} differs from the reference"


# ------------------------------------------------------------------ k_quantize
@pytest.mark.parametrize("widths,dt", QUANT)
def test_quantize_symbols_and_scales_equal_the_oracle(ctx, oracle, widths, dt):
    """lmc_quantize (QUAD = false): six rungs, NITER 4 / 8 for the wide planes."""
    for C in widths:
        x = _kv(C, dt)
        layout, _ = _rows_src(x)
        bins = _bins(C, dt)
        n_sym, n_scale = 2 * NTOK * C, 2 * NTOK
        sym = torch.full((n_sym + GUARD,), 0x5A, dtype=torch.int8, device=DEV)
        scale = torch.full((n_scale + GUARD,), 0x5A5A, dtype=torch.int16, device=DEV)
        ctx._call("lmc_quantize", layout.device, None, ctypes.byref(layout.struct), 0, NTOK, ctx._bins(bins), sym.data_ptr(), scale.data_ptr())
        torch.cuda.synchronize()
        ctx.raise_on_status("quantize")
        bits, code = _bits(oracle, x)
        want_sym, want_scale = oracle.quantize(bits, code, np.array(bins, np.int32))
        sym_h, scale_h = sym.cpu().numpy(), scale.cpu().numpy().view(np.uint16)
        assert np.array_equal(sym_h[:n_sym].reshape(2, NTOK, C), want_sym), f"C={C}: symbols"
        assert np.array_equal(scale_h[:n_scale].reshape(2, NTOK), want_scale), f"C={C}: scales"
        assert (sym_h[n_sym:] == 0x5A).all() and (scale_h[n_scale:] == 0x5A5A).all(), f"C={C}: written behind the outputs"


@pytest.mark.parametrize("widths,dt", TWO_KERNEL)
def test_two_kernel_encode_equals_the_oracle(ctx, oracle, widths, dt):
    """lmc_encode_chunks on the two-kernel path (QUAD = true): SPLIT 2 / 4 waves share a row oct of a wide plane."""
    ctx.set_encode_path("two_kernels")
    try:
        for C in widths:
            x = _kv(C, dt)
            bins = _bins(C, dt)
            blobs, _ = _encode(ctx, ctx.encode_chunks, _rows_src(x)[0], bins)
            _same_blobs(blobs, _coded_refs(oracle, x, bins), f"C={C}")
    finally:
        ctx.set_encode_path("auto")


@pytest.mark.parametrize("widths,dt", NHDB_ENCODE)
def test_nhdb_encode_equals_the_oracle_of_the_gathered_chunk(ctx, oracle, widths, dt):
    """lmc_encode_chunks_split from an LMC_PAGED_SPLIT cache: k_quantize's NHDB instances."""
    for C in widths:
        x = _kv(C, dt)
        bins = _bins(C, dt)
        layout, chunk = _nhdb_src(x)
        assert layout.struct.paged_kind == native.PAGED_SPLIT and torch.equal(_ibits(chunk), _ibits(x))
        blobs, _ = _encode(ctx, ctx.encode_chunks_split, layout, bins)
        _same_blobs(blobs, _coded_refs(oracle, chunk, bins), f"C={C}")


# ------------------------------------------------------------------ k_encode_fused
def _fused(ctx, oracle, layout, chunk, bins, what):
    ctx.set_encode_path("fused")
    try:
        blobs, _ = _encode(ctx, ctx.encode_chunks, layout, bins)
    finally:
        ctx.set_encode_path("auto")
    _same_blobs(blobs, _coded_refs(oracle, chunk, bins), what)


@pytest.mark.parametrize("widths,dt,src", FUSED)
def test_fused_encode_equals_the_oracle(ctx, oracle, widths, dt, src):
    """The full chunk through k_encode_fused (the ragged one takes the two kernels): contiguous rows, and a paged-rows
    source whose block size is a power of two, which has instances of its own."""
    for C in widths:
        x = _kv(C, dt)
        layout, chunk = _rows_src(x) if src == "rows" else _paged_rows_src(x, 16)
        assert torch.equal(_ibits(chunk), _ibits(x))
        _fused(ctx, oracle, layout, chunk, _bins(C, dt), f"C={C} {src}")


@pytest.mark.parametrize("C,dt", FUSED_BS12)
def test_fused_encode_from_a_paged_source_whose_block_size_is_no_power_of_two(ctx, oracle, C, dt):
    """12 slots per block: not the power-of-two instances (their shifts would address other rows), the same bytes."""
    x = _kv(C, dt)
    layout, chunk = _paged_rows_src(x, 12)
    assert layout.struct.block_size == 12 and torch.equal(_ibits(chunk), _ibits(x))
    _fused(ctx, oracle, layout, chunk, _bins(C, dt), "block size 12")


# ------------------------------------------------------------------ k_fixed_encode
@pytest.mark.parametrize("widths,dt", FIXED)
def test_fixed_encode_equals_the_model(ctx, oracle, widths, dt):
    """lmc_encode_chunks_fixed: six rungs, SPLIT 2 / 4 for the wide planes."""
    for C in widths:
        x = _kv(C, dt)
        bins = _bins(C, dt)
        blobs, _ = _encode(ctx, ctx.encode_chunks_fixed, _rows_src(x)[0], bins, coded=False)
        _same_blobs(blobs, _fixed_refs(oracle, x, bins), f"C={C}")


@pytest.mark.parametrize("widths,dt", FIXED_SPLIT)
def test_fixed_encode_from_the_nhdb_cache_equals_the_model(ctx, oracle, widths, dt):
    for C in widths:
        x = _kv(C, dt)
        bins = _bins(C, dt)
        layout, chunk = _nhdb_src(x)
        assert torch.equal(_ibits(chunk), _ibits(x))
        blobs, _ = _encode(ctx, ctx.encode_chunks_fixed_split, layout, bins, coded=False)
        _same_blobs(blobs, _fixed_refs(oracle, chunk, bins), f"C={C}")


@pytest.mark.parametrize("rung,widths,dt,src", LAYERWISE)
def test_layerwise_fixed_job_equals_the_one_piece_encode_and_the_model(ctx, oracle, rung, widths, dt, src):
    """lmc_encode_layers_begin_fixed, one lmc_encode_layer per layer, finish: the LAYER instances, in 1, 2 and 4 slices.
    A chunk has four passes of its rung (three whole ones and two row octs), so every slice count is real; the last chunk
    has two passes (one and a row oct): fewer than four slices, the last two of them empty."""
    nl, per = 2, PASS_TOKENS[rung]
    cs = 3 * per + 9
    ntok = cs + per + 3
    for C in widths:
        H, D = HD[C]
        x = _kv(C, dt, ntok, nl)
        bins = _bins(C, dt, nl)
        layout, chunk = _rows_src(x) if src == "rows" else _nhdb_src(x)
        assert torch.equal(_ibits(chunk), _ibits(x))
        one, _ = _encode(ctx, ctx.encode_chunks_fixed_split, layout, bins, ntok, cs, coded=False)
        _same_blobs(one, _fixed_refs(oracle, chunk, bins, cs), f"C={C}: one piece vs the model")
        st = torch.cuda.current_stream().cuda_stream
        for S in (1, 2, 4):
            ctx.set_fixed_layer_slices(S)
            try:
                a = _Arena(nl, H, D, cs, ntok)
                h = ctx.encode_layers_begin_fixed(layout, 0, ntok, cs, bins, a.blobs.data_ptr(), a.stride, a.sizes.data_ptr())
                assert h is not None, "planes of up to 1024 channels are eligible"
                for l in range(nl):
                    h.encode_layer(l, st)
                h.finish(st)
                blobs = a.read(pad16=False)
                ctx.raise_on_status("layer-wise")
            finally:
                ctx.set_fixed_layer_slices(0)
            _same_blobs(blobs, one, f"C={C} S={S}: layer-wise vs one piece")


# ------------------------------------------------------------------ k_decode, k_fixed_decode
DEC_C = 128  # H = 2, D = 64: an fp8 NHDB destination takes it


class _Stored:
    """NTOK tokens of bf16 KV of DEC_C channels encoded once, coded or fixed-width: the arena, the reference blobs it was
    held against, and the source."""

    def __init__(self, ctx, oracle, fixed):
        self.x = _kv(DEC_C, "bf16")
        self.bins = _bins(DEC_C, "bf16")
        self.H, self.D = HD[DEC_C]
        fn = ctx.encode_chunks_fixed if fixed else ctx.encode_chunks
        blobs, self.arena = _encode(ctx, fn, _rows_src(self.x)[0], self.bins, coded=not fixed)
        self.refs = (_fixed_refs if fixed else _coded_refs)(oracle, self.x, self.bins)
        _same_blobs(blobs, self.refs, "the stored blobs")


@pytest.fixture(scope="module")
def coded(ctx, oracle):
    return _Stored(ctx, oracle, fixed=False)


@pytest.fixture(scope="module")
def fixed(ctx, oracle):
    return _Stored(ctx, oracle, fixed=True)


def _fp8_decode(oracle, blob, dt):
    """The decode of a blob into an fp8 destination (include/lmc_format.h): the fp32 dequantisation (s - C) / C * max of the
    blob's symbols and scales, three separately rounded operations, then ONE cast -- torch's, on the CPU.  -> uint8 [L, 2, T, C]."""
    h = oracle.parse_header(blob)
    P, T, C = h["nplanes"], h["ntokens"], h["nchannels"]
    sym = oracle.decode_blob_symbols(blob)
    bins = np.frombuffer(blob, np.uint8, P, h["off_bins"]).astype(np.int32)
    scale = np.frombuffer(blob, "<u2", P * T, h["off_scales"]).reshape(P, T).copy()
    sc = oracle.bits_to_torch(scale, h["dtype"]).float().reshape(P, T, 1)
    cc = torch.tensor([b // 2 - 1 for b in bins], dtype=torch.float32).reshape(-1, 1, 1)
    t = (torch.from_numpy(sym.astype(np.int16)).float() - cc) / cc * sc
    return t.reshape(2, P // 2, T, C).permute(1, 0, 2, 3).to(dt).contiguous().view(torch.uint8)


def _decoded(oracle, st, dt, fixed):
    """What the blobs of `st` decode to in dt: the integer view [1, 2, NTOK, H, D] (CPU)."""
    tdt = DT[dt]
    if tdt.itemsize == 1:
        parts = [_fp8_decode(oracle, b, tdt) for b in st.refs]
    else:
        code = oracle.BF16 if dt == "bf16" else oracle.FP16
        dec = [fm.decode_blob(oracle, b, code) if fixed else oracle.decode_blob(b, code) for b in st.refs]
        parts = [torch.from_numpy(d.view(np.int16)) for d in dec]
    return torch.cat(parts, dim=2).reshape(1, 2, NTOK, st.H, st.D)


def _destination(kind, want, tdt, H, D):
    """(layout, the tensors it writes, what they must hold afterwards): canary everywhere the decode does not own."""
    if kind == "rows":
        dst = _canary((1, 2, NTOK + 3, H, D), tdt)
        expect = dst.clone()
        _ibits(expect)[:, :, :NTOK] = want
        dst = dst.to(DEV)
        return native.KVLayout.from_chunk(dst, "vllm"), [dst], [expect]
    nb = (NTOK + BS - 1) // BS + 2
    slots = _slots(NTOK, nb, BS, 7 + KINDS.index(kind))
    if kind == "paged":
        dst = _canary((2, nb, BS, H, D), tdt)
        expect = dst.clone()
        _ibits(expect)[:, slots // BS, slots % BS] = want[0]
        layout_name = "NBHD"
    else:
        dst = _canary((2, nb, H, D, BS), tdt)
        expect = dst.clone()
        _torch_scatter([expect], want, slots, BS)
        layout_name = "NHDB"
    dst = dst.to(DEV)
    return native.KVLayout.paged([dst], slots.to(DEV), BS, layout_name), [dst], [expect]


def _whole(tensors, expect, what):
    torch.cuda.synchronize()
    for t, e in zip(tensors, expect):
        assert torch.equal(_ibits(t).cpu(), _ibits(e)), what


@pytest.mark.parametrize("dt,kind", DECODE)
def test_decode_into_every_dtype_and_kind_equals_the_oracles_decode(ctx, oracle, coded, dt, kind):
    want = _decoded(oracle, coded, dt, fixed=False)
    layout, dst, expect = _destination(kind, want, DT[dt], coded.H, coded.D)
    a = coded.arena
    ctx.decode_chunks_layers(a.table.data_ptr(), a.stride, a.n, layout, 0, CS, 0, 1)
    _whole(dst, expect, f"{dt} {kind}")
    ctx.raise_on_status("decode")


def test_decode_symbols_sink_equals_the_oracles_symbols(ctx, oracle, coded):
    a = coded.arena
    for i, t0 in enumerate(range(0, NTOK, CS)):
        T = min(CS, NTOK - t0)
        n = 2 * T * DEC_C
        sym = torch.full((n + GUARD,), 0x5A, dtype=torch.int8, device=DEV)
        ctx._call("lmc_decode_symbols", torch.device(DEV), None, a.blobs.data_ptr() + i * a.stride, 1, coded.H, coded.D, sym.data_ptr())
        torch.cuda.synchronize()
        ctx.raise_on_status("decode_symbols")
        bits, code = _bits(oracle, coded.x[:, :, t0:t0 + T])
        want, _ = oracle.quantize(bits, code, np.array(coded.bins, np.int32))
        got = sym.cpu().numpy()
        assert np.array_equal(got[:n].reshape(2, T, DEC_C), want), f"chunk {i}"
        assert (got[n:] == 0x5A).all(), f"chunk {i}: written behind the symbols"


def test_decode_fixed_sink_equals_the_model(ctx, oracle, coded, fixed):
    """lmc_transcode_to_fixed: the coded blobs -> the fixed-width blobs of the same KV."""
    a = coded.arena
    out = _Arena(1, coded.H, coded.D, CS, NTOK)
    nbytes = torch.tensor([len(b) for b in coded.refs], dtype=torch.int32, device=DEV)
    room = torch.tensor([len(b) for b in fixed.refs], dtype=torch.int32, device=DEV)
    ctx.transcode_to_fixed(a.table.data_ptr(), nbytes.data_ptr(), a.n, 1, coded.H, coded.D, CODE["bf16"], CS, NTOK, coded.bins,
                           out.table.data_ptr(), room.data_ptr(), torch.device(DEV))
    torch.cuda.synchronize()
    ctx.raise_on_status("transcode_to_fixed")
    host = out.blobs.cpu().numpy()
    for i, want in enumerate(fixed.refs):
        slot = host[i * out.stride:(i + 1) * out.stride]
        assert slot[:len(want)].tobytes() == want, f"chunk {i}"
        assert (slot[len(want):] == POISON).all(), f"chunk {i}: bytes behind the blob were written"
    assert (host[out.n * out.stride:] == POISON).all()


@pytest.mark.parametrize("dt,kind", FIXED_DECODE)
def test_fixed_decode_into_every_dtype_and_kind_equals_the_model(ctx, oracle, fixed, dt, kind):
    want = _decoded(oracle, fixed, dt, fixed=True)
    layout, dst, expect = _destination(kind, want, DT[dt], fixed.H, fixed.D)
    a = fixed.arena
    ctx.decode_chunks_fixed_split_schedule(a.table.data_ptr(), a.stride, a.n, layout, 0, CS, [1], None)
    _whole(dst, expect, f"{dt} {kind}")
    ctx.raise_on_status("fixed decode")
