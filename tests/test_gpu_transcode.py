"""lmc_transcode_fixed on the GPU: fixed-width blobs -> the entropy-coded blobs of the same KV.

The central property has no tolerance: lmc_transcode_fixed(lmc_encode_chunks_fixed(x)) == lmc_encode_chunks(x), byte for
byte and with equal size words, for the same KV and bins.  The right-hand side is held against the oracle by the rest of
the suite (and once here).  Input blobs lie scattered in a canary-filled pool, in shuffled order; the output slots have
guard bytes behind each of them and the whole output region is compared with the region lmc_encode_chunks filled from the
same canary -- k_cdf_encode writes a stream's allocation and nothing behind the blob's size (its copy and zero_fill end
with the allocation), so bytes past sizes[i] are the canary in both.

The symbol workspace is the context's and outlives a call: a job takes the workspace its stream used last, so a transcode
straight behind the reference encode would find k_quantize's own -- correct -- symbols of the same chunks at the same
addresses, and a k_fixed_expand that stored nothing would pass.  Every transcode here therefore runs behind `dirty`: a
two-kernel lmc_encode_chunks of FOREIGN data with the same geometry and every chunk full, on the same stream, so that
every dword the coder can read holds another job's symbols until k_fixed_expand has written it."""
import os

import numpy as np
import pytest
import torch

from lmcache_amd import native
from tests import fixed_model as fm

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BAD_HEADER, BAD_STREAM, BAD_SCALES = 2, 4, 16
CANARY, GUARD = 0xC3, 32
BINS = [16, 32, 17, 18]  # L = 2: narrow, wide, narrow (the last narrow count), wide (the first wide one)


@pytest.fixture(scope="module")
def ctx():
    native.lib()
    return native.get_context(0)


def make_kv(L, T, H, D, dtype, seed, kind="randn"):
    g = torch.Generator().manual_seed(seed)
    if kind == "rand":
        return (torch.rand(L, 2, T, H, D, generator=g) - 0.25).to(dtype)
    x = torch.randn(L, 2, T, H, D, generator=g) * torch.exp(1.5 * torch.randn(H * D, generator=g)).reshape(H, D)
    return x.to(dtype)


def nchunks_of(n, cs):
    return (n + cs - 1) // cs


def encode(ctx, kv_d, cs, bins, fixed, stride=None, stream=None):
    """-> (region [n * stride] prefilled with the canary, sizes list, stride)."""
    L, _, n, H, D = kv_d.shape
    stride = stride or native.r16(native.blob_bound(L, cs, H, D)) + GUARD
    m = nchunks_of(n, cs)
    region = torch.full((m * stride,), CANARY, dtype=torch.uint8, device=DEV)
    sizes = torch.zeros(m, dtype=torch.int32, device=DEV)
    call = ctx.encode_chunks_fixed if fixed else ctx.encode_chunks
    call(native.KVLayout.from_chunk(kv_d, "vllm"), 0, n, cs, bins, region.data_ptr(), stride, sizes.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    assert ctx.status(clear=True) == 0
    return region, sizes.cpu().tolist(), stride


def dirty(ctx, L, H, D, cs, nchunks, dtype, bins, stream=None):
    """Fill the symbol workspace this stream's next job takes with the symbols of foreign data (module docstring): the same
    L, H, D, chunk length and chunk count -- the same regions at the same addresses -- every chunk full, k_quantize always."""
    g = torch.Generator().manual_seed(977 + nchunks + cs)
    # (a wide spread of magnitudes and signs: every symbol value of every plane occurs, none of it related to the test's data)
    x = (torch.randn(L, 2, nchunks * cs, H, D, generator=g) * torch.exp(2.0 * torch.randn(H, D, generator=g))).to(dtype).to(DEV)
    stride = native.r16(native.blob_bound(L, cs, H, D))
    junk = torch.empty(nchunks * stride, dtype=torch.uint8, device=DEV)
    sizes = torch.zeros(nchunks, dtype=torch.int32, device=DEV)
    ctx.set_encode_path("two_kernels")
    try:
        ctx.encode_chunks(native.KVLayout.from_chunk(x, "vllm"), 0, nchunks * cs, cs, bins, junk.data_ptr(), stride, sizes.data_ptr(),
                          stream=stream)
    finally:
        ctx.set_encode_path("auto")
    return junk, sizes, x  # (kept alive by the caller until the stream has run them)


def scatter(blobs, seed=0):
    """Blobs (bytes) at 16-byte-aligned places of one canary-filled pool, in shuffled order, canary on both sides of each
    -> (pool, [uint8 views])."""
    order = np.random.default_rng(seed).permutation(len(blobs))
    at, place = 48, {}
    for i in order:
        place[int(i)] = at
        at += native.r16(len(blobs[i])) + 16 * (1 + int(i) % 3)
    pool = torch.full((at + 48,), CANARY, dtype=torch.uint8)
    for i, b in enumerate(blobs):
        pool[place[i]:place[i] + len(b)] = torch.from_numpy(np.frombuffer(b, np.uint8).copy())
    pool = pool.to(DEV)
    views = [pool[place[i]:place[i] + len(b)] for i, b in enumerate(blobs)]
    assert all(v.data_ptr() % 16 == 0 for v in views)
    return pool, views


def transcode(ctx, views, geometry, dtype, cs, ntokens, bins, stride, room=None, stream=None):
    """Behind a `dirty` of the same geometry on the same stream -> (output region prefilled with the canary, sizes list,
    status word)."""
    L, H, D = geometry
    n = len(views)
    keep = dirty(ctx, L, H, D, cs, n, dtype, bins, stream=stream)
    table = torch.tensor([v.data_ptr() for v in views], dtype=torch.int64, device=DEV)
    nbytes = torch.tensor(room if room is not None else [v.numel() for v in views], dtype=torch.int32, device=DEV)
    out = torch.full((n * stride,), CANARY, dtype=torch.uint8, device=DEV)
    sizes = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    ctx.transcode_fixed(table.data_ptr(), nbytes.data_ptr(), n, L, H, D, native.dtype_code(dtype), cs, ntokens, bins, out.data_ptr(),
                        stride, sizes.data_ptr(), torch.device(DEV), stream=stream)
    torch.cuda.synchronize()
    del keep
    return out, sizes.cpu().tolist(), ctx.status(clear=True)


def fixed_blobs(ctx, kv_d, cs, bins):
    region, sizes, stride = encode(ctx, kv_d, cs, bins, fixed=True)
    host = region.cpu().numpy()
    return [host[i * stride:i * stride + sizes[i]].tobytes() for i in range(len(sizes))]


def check_equal(ctx, kv, cs, bins, oracle=None, seed=0):
    """The central property for one job; -> (coded region, sizes, stride, fixed views)."""
    L, _, n, H, D = kv.shape
    kv_d = kv.to(DEV)
    blobs = fixed_blobs(ctx, kv_d, cs, bins)
    pool, views = scatter(blobs, seed)
    pool0 = pool.clone()
    ref, ref_sizes, stride = encode(ctx, kv_d, cs, bins, fixed=False)
    out, sizes, st = transcode(ctx, views, (L, H, D), kv.dtype, cs, n, bins, stride)
    assert st == 0
    assert sizes == ref_sizes
    assert torch.equal(out, ref), "the transcoded region differs from the encoded one (blobs, slot tails or guards)"
    assert torch.equal(pool, pool0), "the transcode wrote to its input"
    for i, nb in enumerate(sizes):  # what the coder leaves behind a blob: nothing
        assert bool((out[i * stride + native.r16(nb):(i + 1) * stride] == CANARY).all()), i
    if oracle is not None:
        host = out.cpu().numpy()
        for i, nb in enumerate(sizes):
            c = kv[:, :, i * cs:(i + 1) * cs].contiguous()
            b, code = oracle.torch_to_bits(c.reshape(L, 2, c.shape[2], H * D))
            assert host[i * stride:i * stride + nb].tobytes() == oracle.encode_blob(b, code, H, D, np.array(bins, np.int32)), i
    return out, sizes, stride, views


# (H, D, chunk_tokens, tokens, dtype, data): L = 2 throughout
CASES = [
    (2, 64, 256, 2 * 256, torch.bfloat16, "randn"),      # C = 128: P G = 8, the counts-only coder
    (2, 64, 32, 3 * 32, torch.bfloat16, "rand"),
    (2, 64, 16, 3 * 16, torch.float16, "randn"),
    (2, 64, 256, 256 + 5, torch.bfloat16, "randn"),      # a ragged last chunk of 5 tokens
    (2, 64, 256, 256 + 1, torch.float16, "randn"),       # a one-token last chunk: CDF16, the general coder for the tail only
    (2, 64, 257, 257 + 100, torch.bfloat16, "randn"),    # T > 256: CDF16 throughout
    (2, 64, 32, 32 + 13, torch.bfloat16, "rand"),        # tails that are no multiple of 8 or 4
    (2, 64, 32, 32 + 30, torch.float16, "rand"),
    (3, 64, 256, 256 + 5, torch.bfloat16, "randn"),      # C = 192: P G = 12, the general coder launch with scratch slots
    (3, 64, 64, 2 * 64, torch.float16, "rand"),
    (1, 72, 64, 2 * 64 + 13, torch.bfloat16, "randn"),   # C = 72: the last group is partly empty
    (16, 128, 32, 32, torch.bfloat16, "randn"),          # C = 2048: past k_fixed_encode's split-source limit, not this kernel's
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "H%dD%dcs%dn%d-%s-%s" % (c[0], c[1], c[2], c[3], str(c[4]).split(".")[-1], c[5]))
def test_transcoded_blobs_equal_the_encoded_ones(ctx, case):
    H, D, cs, n, dtype, kind = case
    kv = make_kv(2, n, H, D, dtype, seed=n + H, kind=kind)
    check_equal(ctx, kv, cs, BINS, seed=n)


def test_the_chain_is_closed_against_the_oracle(ctx, oracle):
    kv = make_kv(2, 64 + 13, 2, 64, torch.bfloat16, seed=5)
    check_equal(ctx, kv, 64, BINS, oracle=oracle)


def test_edge_rows_round_trip(ctx, golden_dir):
    z = np.load(os.path.join(golden_dir, "quant_edge.npz"))
    x = torch.from_numpy(z["x"].view(np.int16)).view(torch.bfloat16)  # [2, T, 64]: zero / inf / NaN / denormal rows among them
    Lk, T, C = x.shape
    kv = torch.stack([x, x], dim=1).reshape(Lk, 2, T, 1, C)
    for bins in ([int(v) for v in z["bins"].tolist()] * 2, BINS[:2 * Lk]):
        check_equal(ctx, kv, T, bins)


def test_the_comparison_can_fail(ctx):
    a = make_kv(2, 64, 2, 64, torch.bfloat16, seed=1)
    b = make_kv(2, 64, 2, 64, torch.bfloat16, seed=2)
    pool, views = scatter(fixed_blobs(ctx, a.to(DEV), 64, BINS))
    ref, ref_sizes, stride = encode(ctx, b.to(DEV), 64, BINS, fixed=False)
    out, sizes, st = transcode(ctx, views, (2, 2, 64), a.dtype, 64, 64, BINS, stride)
    assert st == 0 and not torch.equal(out, ref)
    # ... and by the symbols alone: B with A's scales row for row (a row max of A's, the rest of the row smaller) differs from
    # A in its symbols only -- the streams sections must differ, the scales sections must not
    c = (b.float() * 0.25).clamp(-1, 1)
    amax = a.float().abs().amax(dim=(3, 4), keepdim=True)
    c = c * amax
    c[:, :, :, 0, 0] = amax[:, :, :, 0, 0]
    c = c.to(torch.bfloat16)
    ref_c, sizes_c, _ = encode(ctx, c.to(DEV), 64, BINS, fixed=False)
    h = native.blob_info(bytes(out[:128].cpu().numpy()), sizes[0])
    sc = slice(int(h.off_scales), int(h.off_scales) + 2 * 4 * 64)
    assert torch.equal(out[sc], ref_c[sc]), "the two chunks were meant to share their scales"
    assert not torch.equal(out[int(h.off_streams):sizes[0]], ref_c[int(h.off_streams):sizes[0]])


def test_decode_parity(ctx):
    L, H, D, cs, n = 2, 3, 64, 64, 64 + 30
    kv = make_kv(L, n, H, D, torch.bfloat16, seed=9)
    out, sizes, stride, views = check_equal(ctx, kv, cs, BINS)
    a = torch.zeros(L, 2, n, H, D, dtype=torch.bfloat16, device=DEV)
    b = torch.zeros_like(a)
    ctx.decode_chunks(out.data_ptr(), stride, len(sizes), native.KVLayout.from_chunk(a, "vllm"), 0, cs)
    table = torch.tensor([v.data_ptr() for v in views], dtype=torch.int64, device=DEV)
    ctx.decode_chunks_fixed_schedule(table.data_ptr(), max(v.numel() for v in views), len(views), native.KVLayout.from_chunk(b, "vllm"),
                                     0, cs, [L], None)
    torch.cuda.synchronize()
    assert ctx.status(clear=True) == 0
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


def _damaged(blob, what):
    """-> (bytes, the status bit a transcode must report)."""
    b = bytearray(blob)
    h = fm.header(blob)
    u32 = lambda at: int(np.frombuffer(bytes(b[at:at + 4]), "<u4")[0])

    def put32(at, v):
        b[at:at + 4] = np.array([v & 0xffffffff], "<u4").tobytes()
    if what == "lo":
        at = fm.stream_spans(blob)[1][0] + 8
        put32(at, u32(at) ^ 0x10)
        return bytes(b), BAD_STREAM
    if what == "scale":
        at = int(h[fm.W_OFF_SCALES]) + 2 * 3
        b[at] ^= 1
        return bytes(b), BAD_SCALES
    if what == "model":
        put32(4 * fm.W_MODEL, 1)  # LMC_MODEL_COUNTS
    elif what == "T":
        put32(4 * fm.W_T, int(h[fm.W_T]) - 1)
    elif what == "gdir":
        at = int(h[fm.W_OFF_GDIR]) + 8 * 2
        put32(at, u32(at) + 16)
    elif what == "bins":
        at = int(h[fm.W_OFF_BINS])
        assert b[at] == 16
        b[at] = 17  # (still a narrow plane: every total stays what it was -- only the bins differ from the call's)
    return bytes(b), BAD_HEADER


@pytest.mark.parametrize("what", ["lo", "scale", "model", "T", "gdir", "bins", "room0"])
def test_a_damaged_blob_is_flagged_and_its_neighbour_still_comes_out_right(ctx, what):
    L, H, D, cs, n = 2, 2, 64, 32, 64
    kv = make_kv(L, n, H, D, torch.bfloat16, seed=21)
    kv_d = kv.to(DEV)
    blobs = fixed_blobs(ctx, kv_d, cs, BINS)
    ref, ref_sizes, stride = encode(ctx, kv_d, cs, BINS, fixed=False)
    room = None
    if what == "room0":
        bad, want = blobs[0], BAD_HEADER
        room = [0, len(blobs[1])]
    else:
        bad, want = _damaged(blobs[0], what)
    pool, views = scatter([bad, blobs[1]])
    pool0 = pool.clone()
    out, sizes, st = transcode(ctx, views, (L, H, D), kv.dtype, cs, n, BINS, stride, room=room)
    assert st == want
    assert torch.equal(pool, pool0)
    assert sizes[1] == ref_sizes[1] and torch.equal(out[stride:], ref[stride:]), "the good chunk beside the bad one"
    assert bool((out[stride - GUARD:stride] == CANARY).all())


def test_refusals_queue_nothing(ctx):
    L, H, D, cs, n = 2, 2, 64, 32, 64
    kv_d = make_kv(L, n, H, D, torch.bfloat16, seed=3).to(DEV)
    pool, views = scatter(fixed_blobs(ctx, kv_d, cs, BINS))
    bound = native.r16(native.blob_bound(L, cs, H, D))
    table = torch.tensor([v.data_ptr() for v in views], dtype=torch.int64, device=DEV)
    nbytes = torch.tensor([v.numel() for v in views], dtype=torch.int32, device=DEV)
    out = torch.full((2 * bound + 16,), CANARY, dtype=torch.uint8, device=DEV)
    sizes = torch.full((2,), -1, dtype=torch.int32, device=DEV)
    bins = native.Context._bins(BINS)
    bf16 = native.dtype_code(torch.bfloat16)

    def call(nchunks=2, dtype=bf16, out_ptr=out.data_ptr(), stride=bound):
        return native.lib().lmc_transcode_fixed(ctx.handle, table.data_ptr(), nbytes.data_ptr(), nchunks, L, H, D, dtype, cs, n, bins,
                                                out_ptr, stride, sizes.data_ptr(), None, native.current_stream_ptr(torch.device(DEV)))
    assert call(stride=bound - 16) == native.ERR_INVALID
    assert call(out_ptr=out.data_ptr() + 8) == native.ERR_INVALID
    assert call(dtype=native.FP8_E4M3) == native.ERR_INVALID
    assert call(nchunks=0) == native.ERR_INVALID
    assert call(nchunks=-1) == native.ERR_INVALID
    torch.cuda.synchronize()
    assert bool((out == CANARY).all()) and sizes.cpu().tolist() == [-1, -1] and ctx.status(clear=True) == 0
    assert call() == 0  # (the same arguments, unspoilt, are a job)
    torch.cuda.synchronize()
    assert ctx.status(clear=True) == 0 and min(sizes.cpu().tolist()) > 0


def test_two_transcodes_on_two_streams(ctx):
    L, H, D, cs, n = 2, 2, 64, 256, 512
    kvs = [make_kv(L, n, H, D, torch.bfloat16, seed=40 + i) for i in range(2)]
    jobs = []
    for kv in kvs:
        kv_d = kv.to(DEV)
        ref, ref_sizes, stride = encode(ctx, kv_d, cs, BINS, fixed=False)
        pool, views = scatter(fixed_blobs(ctx, kv_d, cs, BINS))
        table = torch.tensor([v.data_ptr() for v in views], dtype=torch.int64, device=DEV)
        nbytes = torch.tensor([v.numel() for v in views], dtype=torch.int32, device=DEV)
        out = torch.full((len(views) * stride,), CANARY, dtype=torch.uint8, device=DEV)
        sizes = torch.full((len(views),), -1, dtype=torch.int32, device=DEV)
        jobs.append((ref, ref_sizes, stride, pool, views, table, nbytes, out, sizes, torch.cuda.Stream(device=DEV)))
    torch.cuda.synchronize()
    for _ in range(2):  # (the second round finds both workspaces taken)
        keep = [dirty(ctx, L, H, D, cs, len(j[4]), torch.bfloat16, BINS, stream=j[9].cuda_stream) for j in jobs]
        for ref, ref_sizes, stride, pool, views, table, nbytes, out, sizes, s in jobs:
            ctx.transcode_fixed(table.data_ptr(), nbytes.data_ptr(), len(views), L, H, D, native.dtype_code(torch.bfloat16), cs, n, BINS,
                                out.data_ptr(), stride, sizes.data_ptr(), torch.device(DEV), stream=s.cuda_stream)
    torch.cuda.synchronize()
    assert ctx.status(clear=True) == 0
    for ref, ref_sizes, stride, pool, views, table, nbytes, out, sizes, s in jobs:
        assert sizes.cpu().tolist() == ref_sizes and torch.equal(out, ref)
