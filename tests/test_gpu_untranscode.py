"""lmc_transcode_to_fixed on the GPU: entropy-coded blobs -> the fixed-width blobs of the same KV.

The central property has no tolerance: lmc_transcode_to_fixed(lmc_encode_chunks(x)) == lmc_encode_chunks_fixed(x), byte for
byte, for the same KV and bins.  The coded input blobs lie scattered in a canary-filled pool, in shuffled order; every
output slot has guard bytes behind it, and the whole output region is compared with the region lmc_encode_chunks_fixed
filled from the same canary: every byte of every blob, pads included, and nothing behind a blob's end.  The kernel has no
workspace, so nothing of an earlier job can stand in for its output: the canary is all a store that did not happen leaves.
Geometries, data and helpers are tests/test_gpu_transcode.py's (the other direction)."""
import os

import numpy as np
import pytest
import torch

from lmcache_amd import native
from tests import fixed_model as fm
from tests.test_gpu_transcode import (BAD_HEADER, BAD_SCALES, BAD_STREAM, BINS, CANARY, CASES, DEV, GUARD, encode, make_kv, scatter,
                                      transcode)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    native.lib()
    return native.get_context(0)


def coded_blobs(ctx, kv_d, cs, bins):
    region, sizes, stride = encode(ctx, kv_d, cs, bins, fixed=False)
    host = region.cpu().numpy()
    return [host[i * stride:i * stride + sizes[i]].tobytes() for i in range(len(sizes))]


def untranscode(ctx, views, geometry, dtype, cs, ntokens, bins, stride, room=None, out_room=None, ptrs=None, stream=None):
    """-> (output region of len(views) slots of `stride` bytes prefilled with the canary, status word).  room / out_room:
    what the call is told it may read / write per chunk (default: the blob's length / the slot without its guard)."""
    L, H, D = geometry
    n = len(views)
    out = torch.full((n * stride,), CANARY, dtype=torch.uint8, device=DEV)
    table = torch.tensor(ptrs if ptrs is not None else [v.data_ptr() for v in views], dtype=torch.int64, device=DEV)
    nbytes = torch.tensor(room if room is not None else [v.numel() for v in views], dtype=torch.int32, device=DEV)
    outs = torch.tensor([out.data_ptr() + i * stride for i in range(n)], dtype=torch.int64, device=DEV)
    obytes = torch.tensor(out_room if out_room is not None else [stride - GUARD] * n, dtype=torch.int32, device=DEV)
    ctx.transcode_to_fixed(table.data_ptr(), nbytes.data_ptr(), n, L, H, D, native.dtype_code(dtype), cs, ntokens, bins,
                           outs.data_ptr(), obytes.data_ptr(), torch.device(DEV), stream=stream)
    torch.cuda.synchronize()
    return out, ctx.status(clear=True)


def check_equal(ctx, kv, cs, bins, oracle=None, seed=0):
    """The central property for one job; -> (fixed-width region, its blobs' sizes, stride, coded views, their pool)."""
    L, _, n, H, D = kv.shape
    kv_d = kv.to(DEV)
    pool, views = scatter(coded_blobs(ctx, kv_d, cs, bins), seed)
    pool0 = pool.clone()
    ref, ref_sizes, stride = encode(ctx, kv_d, cs, bins, fixed=True)
    out, st = untranscode(ctx, views, (L, H, D), kv.dtype, cs, n, bins, stride)
    assert st == 0
    for i, nb in enumerate(ref_sizes):
        assert nb == native.fixed_blob_bytes(L, min(cs, n - i * cs), H, D, bins)
        assert bool((ref[i * stride + nb:(i + 1) * stride] == CANARY).all()), i  # (the reference writes its blob and no more)
    assert torch.equal(out, ref), "the transcoded region differs from the encoded one (blobs, pads or guards)"
    assert torch.equal(pool, pool0), "the transcode wrote to its input"
    if oracle is not None:
        host = out.cpu().numpy()
        for i, nb in enumerate(ref_sizes):
            c = kv[:, :, i * cs:(i + 1) * cs].contiguous()
            b, code = oracle.torch_to_bits(c.reshape(L, 2, c.shape[2], H * D))
            assert host[i * stride:i * stride + nb].tobytes() == fm.encode_blob(oracle, b, code, H, D, bins), i
    return out, ref_sizes, stride, views, pool


@pytest.mark.parametrize("case", CASES, ids=lambda c: "H%dD%dcs%dn%d-%s-%s" % (c[0], c[1], c[2], c[3], str(c[4]).split(".")[-1], c[5]))
def test_transcoded_blobs_equal_the_fixed_width_encode(ctx, case):
    H, D, cs, n, dtype, kind = case
    kv = make_kv(2, n, H, D, dtype, seed=n + H, kind=kind)
    check_equal(ctx, kv, cs, BINS, seed=n)


def test_the_chain_is_closed_against_the_oracle(ctx, oracle):
    kv = make_kv(2, 64 + 13, 2, 64, torch.bfloat16, seed=5)
    check_equal(ctx, kv, 64, BINS, oracle=oracle)


def test_the_two_transcodes_are_inverses(ctx):
    """lmc_transcode_fixed(lmc_transcode_to_fixed(b)) == b for coded b."""
    L, H, D, cs, n = 2, 3, 64, 32, 2 * 32 + 13
    kv = make_kv(L, n, H, D, torch.float16, seed=17)
    out, sizes, stride, views, pool = check_equal(ctx, kv, cs, BINS)
    fixed_views = [out[i * stride:i * stride + nb] for i, nb in enumerate(sizes)]
    ref, ref_sizes, cstride = encode(ctx, kv.to(DEV), cs, BINS, fixed=False)
    back, back_sizes, st = transcode(ctx, fixed_views, (L, H, D), kv.dtype, cs, n, BINS, cstride)
    assert st == 0 and back_sizes == ref_sizes == [v.numel() for v in views]
    assert torch.equal(back, ref)
    for i, v in enumerate(views):
        assert torch.equal(back[i * cstride:i * cstride + v.numel()], v), i


def test_edge_rows(ctx, golden_dir):
    z = np.load(os.path.join(golden_dir, "quant_edge.npz"))
    x = torch.from_numpy(z["x"].view(np.int16)).view(torch.bfloat16)  # [2, T, 64]: zero / inf / NaN / denormal rows among them
    Lk, T, C = x.shape
    kv = torch.stack([x, x], dim=1).reshape(Lk, 2, T, 1, C)
    for bins in ([int(v) for v in z["bins"].tolist()] * 2, BINS[:2 * Lk]):
        check_equal(ctx, kv, T, bins)


def test_the_comparison_can_fail(ctx):
    a = make_kv(2, 64, 2, 64, torch.bfloat16, seed=1)
    b = make_kv(2, 64, 2, 64, torch.bfloat16, seed=2)
    pool, views = scatter(coded_blobs(ctx, a.to(DEV), 64, BINS))
    ref, ref_sizes, stride = encode(ctx, b.to(DEV), 64, BINS, fixed=True)
    out, st = untranscode(ctx, views, (2, 2, 64), a.dtype, 64, 64, BINS, stride)
    assert st == 0 and not torch.equal(out, ref)
    ref_a, _, _ = encode(ctx, a.to(DEV), 64, BINS, fixed=True)
    assert torch.equal(out, ref_a)


def test_decode_parity(ctx):
    """lmc_decode_chunks_fixed_schedule of the output is bit-equal to lmc_decode_chunks of the input."""
    L, H, D, cs, n = 2, 3, 64, 64, 64 + 30
    for dtype in (torch.bfloat16, torch.float16):
        kv = make_kv(L, n, H, D, dtype, seed=9)
        kv_d = kv.to(DEV)
        coded, csizes, cstride = encode(ctx, kv_d, cs, BINS, fixed=False)
        out, sizes, stride, views, pool = check_equal(ctx, kv, cs, BINS)
        a = torch.zeros(L, 2, n, H, D, dtype=dtype, device=DEV)
        b = torch.zeros_like(a)
        ctx.decode_chunks(coded.data_ptr(), cstride, len(csizes), native.KVLayout.from_chunk(a, "vllm"), 0, cs)
        table = torch.tensor([out.data_ptr() + i * stride for i in range(len(sizes))], dtype=torch.int64, device=DEV)
        ctx.decode_chunks_fixed_schedule(table.data_ptr(), max(sizes), len(sizes), native.KVLayout.from_chunk(b, "vllm"), 0, cs, [L], None)
        torch.cuda.synchronize()
        assert ctx.status(clear=True) == 0
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))
        assert bool(a.view(torch.int16).any())


def _damaged(blob, what):
    """A coded blob with one thing wrong -> (bytes, the status bit a transcode must report)."""
    b = bytearray(blob)
    h = fm.header(blob)
    u32 = lambda at: int(np.frombuffer(bytes(b[at:at + 4]), "<u4")[0])

    def put32(at, v):
        b[at:at + 4] = np.array([v & 0xffffffff], "<u4").tobytes()
    if what == "stream":  # a byte of the final states of stream 1 (the last 256 bytes of a stream)
        end = u32(int(h[fm.W_OFF_GDIR]) + 8 * 1 + 4)
        b[int(h[fm.W_OFF_STREAMS]) + end - 100] ^= 0x10
        return bytes(b), BAD_STREAM
    if what == "scale":
        b[int(h[fm.W_OFF_SCALES]) + 2 * 3] ^= 1
        return bytes(b), BAD_SCALES
    if what == "magic":
        put32(0, u32(0) ^ 1)
    elif what == "model-fixed":
        put32(4 * fm.W_MODEL, fm.MODEL_FIXED)
    elif what == "kv_dtype":
        put32(4 * 23, native.FP8_E4M3)
    elif what == "dtype":
        put32(4 * 2, u32(4 * 2) ^ 1)
    elif what == "L":
        put32(4 * 3, u32(4 * 3) + 1)
    elif what == "T":
        put32(4 * fm.W_T, int(h[fm.W_T]) - 1)
    elif what == "HD":  # the same C = H D, other heads
        put32(4 * 5, u32(4 * 5) * 2)
        put32(4 * 6, u32(4 * 6) // 2)
    elif what == "C":
        put32(4 * fm.W_C, int(h[fm.W_C]) + 8)
    elif what == "total":
        put32(4 * fm.W_TOTAL, int(h[fm.W_TOTAL]) + 16)
    elif what == "bins":
        at = int(h[fm.W_OFF_BINS])
        assert b[at] == 16
        b[at] = 17  # (a plane of the same width class: only the bins differ from the call's)
    else:
        raise KeyError(what)
    return bytes(b), BAD_HEADER


DAMAGE = ["stream", "scale", "magic", "model-fixed", "kv_dtype", "dtype", "L", "T", "HD", "C", "total", "bins",
          "room-1", "room0", "null", "unaligned", "out-1", "out-null"]


@pytest.mark.parametrize("what", DAMAGE)
def test_a_damaged_blob_is_flagged_and_its_neighbour_still_comes_out_right(ctx, what):
    L, H, D, cs, n = 2, 2, 64, 32, 64
    kv = make_kv(L, n, H, D, torch.bfloat16, seed=21)
    kv_d = kv.to(DEV)
    blobs = coded_blobs(ctx, kv_d, cs, BINS)
    ref, ref_sizes, stride = encode(ctx, kv_d, cs, BINS, fixed=True)
    room = out_room = ptrs = None
    bad, want = blobs[0], BAD_HEADER
    if what == "room-1":
        room = [len(blobs[0]) - 1, len(blobs[1])]
    elif what == "room0":
        room = [0, len(blobs[1])]
    elif what == "out-1":
        out_room = [ref_sizes[0] - 1, ref_sizes[1]]
    elif what == "out-null":
        out_room = [0, ref_sizes[1]]
    elif what not in ("null", "unaligned"):
        bad, want = _damaged(blobs[0], what)
    pool, views = scatter([bad, blobs[1]])
    if what == "null":
        ptrs = [0, views[1].data_ptr()]
    elif what == "unaligned":
        ptrs = [views[0].data_ptr() + 8, views[1].data_ptr()]
    pool0 = pool.clone()
    out, st = untranscode(ctx, views, (L, H, D), kv.dtype, cs, n, BINS, stride, room=room, out_room=out_room, ptrs=ptrs)
    assert st == want
    assert torch.equal(pool, pool0)
    assert torch.equal(out[stride:], ref[stride:]), "the good chunk beside the bad one"
    # nothing outside the damaged chunk's own output span; a header that fails writes nothing at all.  (Scales and stream
    # are judged once they have been consumed: the span's contents are unspecified then.)
    assert bool((out[ref_sizes[0]:stride] == CANARY).all())
    if want == BAD_HEADER:
        assert bool((out[:stride] == CANARY).all())


def test_refusals_queue_nothing(ctx):
    L, H, D, cs, n = 2, 2, 64, 32, 64
    kv_d = make_kv(L, n, H, D, torch.bfloat16, seed=3).to(DEV)
    pool, views = scatter(coded_blobs(ctx, kv_d, cs, BINS))
    ref, ref_sizes, stride = encode(ctx, kv_d, cs, BINS, fixed=True)
    table = torch.tensor([v.data_ptr() for v in views], dtype=torch.int64, device=DEV)
    nbytes = torch.tensor([v.numel() for v in views], dtype=torch.int32, device=DEV)
    out = torch.full((2 * stride,), CANARY, dtype=torch.uint8, device=DEV)
    outs = torch.tensor([out.data_ptr(), out.data_ptr() + stride], dtype=torch.int64, device=DEV)
    obytes = torch.tensor([stride - GUARD] * 2, dtype=torch.int32, device=DEV)
    bf16 = native.dtype_code(torch.bfloat16)

    def call(nchunks=2, dtype=bf16, H=H, D=D, bins=BINS, ntokens=n, out_ptrs=outs.data_ptr()):
        return native.lib().lmc_transcode_to_fixed(ctx.handle, table.data_ptr(), nbytes.data_ptr(), nchunks, L, H, D, dtype, cs, ntokens,
                                                   native.Context._bins(bins), out_ptrs, obytes.data_ptr(), None,
                                                   native.current_stream_ptr(torch.device(DEV)))
    assert call(dtype=native.FP8_E4M3) == native.ERR_INVALID
    assert call(nchunks=0) == native.ERR_INVALID
    assert call(nchunks=-1) == native.ERR_INVALID
    assert call(ntokens=n + 1) == native.ERR_INVALID       # more tokens than two chunks hold
    assert call(ntokens=cs) == native.ERR_INVALID          # ... and no more than one holds
    assert call(H=2, D=63) == native.ERR_INVALID           # C is no multiple of 8
    assert call(H=64, D=128) == native.ERR_INVALID         # planes above LMC_MAX_CHANNELS channels
    assert call(bins=[16, 32, 17, 3]) == native.ERR_INVALID
    assert call(bins=[16, 32, 17, 64]) == native.ERR_INVALID
    assert call(out_ptrs=None) == native.ERR_INVALID
    torch.cuda.synchronize()
    assert bool((out == CANARY).all()) and ctx.status(clear=True) == 0
    assert call() == 0  # (the same arguments, unspoilt, are a job)
    torch.cuda.synchronize()
    assert ctx.status(clear=True) == 0 and torch.equal(out, ref)


def test_two_jobs_on_two_streams(ctx):
    L, H, D, cs, n = 2, 2, 64, 256, 512
    jobs = []
    for i in range(2):
        kv_d = make_kv(L, n, H, D, torch.bfloat16, seed=40 + i).to(DEV)
        ref, ref_sizes, stride = encode(ctx, kv_d, cs, BINS, fixed=True)
        pool, views = scatter(coded_blobs(ctx, kv_d, cs, BINS), seed=i)
        m = len(views)
        table = torch.tensor([v.data_ptr() for v in views], dtype=torch.int64, device=DEV)
        nbytes = torch.tensor([v.numel() for v in views], dtype=torch.int32, device=DEV)
        out = torch.full((m * stride,), CANARY, dtype=torch.uint8, device=DEV)
        outs = torch.tensor([out.data_ptr() + k * stride for k in range(m)], dtype=torch.int64, device=DEV)
        obytes = torch.tensor([stride - GUARD] * m, dtype=torch.int32, device=DEV)
        jobs.append((ref, pool, table, nbytes, out, outs, obytes, torch.cuda.Stream(device=DEV), m))
    torch.cuda.synchronize()
    for ref, pool, table, nbytes, out, outs, obytes, s, m in jobs:
        ctx.transcode_to_fixed(table.data_ptr(), nbytes.data_ptr(), m, L, H, D, native.dtype_code(torch.bfloat16), cs, n, BINS,
                               outs.data_ptr(), obytes.data_ptr(), torch.device(DEV), stream=s.cuda_stream)
    torch.cuda.synchronize()
    assert ctx.status(clear=True) == 0
    for ref, pool, table, nbytes, out, outs, obytes, s, m in jobs:
        assert torch.equal(out, ref)
