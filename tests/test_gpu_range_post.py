"""The post-op entry points of the C ABI on the GPU (include/lmc_hip.h, lmc_range_post): the post = NULL form of
lmc_decode_chunks_schedule_post against lmc_decode_chunks_schedule, a post-op that does not check out, and the layer
window (native.KVLayout.layers) that the C side cuts for a range.  Every comparison is on integer views, bit for bit."""
import pytest
import torch

from lmcache_amd import native
from tests.test_gpu_rope_shift import NTOK, ROWS, _finite_keys, _ibits, _random_bits, _table

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def ctx():
    native.build()
    return native.get_context(0)


def test_schedule_post_with_a_null_post_is_the_schedule(ctx):
    """lmc_decode_chunks_schedule_post(post = NULL) and lmc_decode_chunks_schedule on the same blobs: the same bytes."""
    Lb, T, H, D, cs = 3, 64, 2, 64, 32
    g = torch.Generator().manual_seed(5)
    kv = torch.randn((Lb, 2, T, H, D), generator=g).to(torch.bfloat16).to(DEV)
    n = T // cs
    stride = native.r16(native.blob_bound(Lb, cs, H, D))
    blobs = torch.zeros(n * stride, dtype=torch.uint8, device=DEV)
    sizes = torch.zeros(n, dtype=torch.int32, device=DEV)
    ctx.encode_chunks(native.KVLayout.from_chunk(kv, "vllm"), 0, T, cs, [32, 32, 32, 16, 16, 16], blobs.data_ptr(), stride,
                      sizes.data_ptr())
    table = torch.tensor([blobs.data_ptr() + i * stride for i in range(n)], dtype=torch.int64).to(DEV)
    outs = [torch.zeros_like(kv) for _ in range(3)]
    dsts = [native.KVLayout.from_chunk(o, "vllm") for o in outs]
    ctx.decode_chunks_schedule(table.data_ptr(), stride, n, dsts[0], 0, cs, [1, 3], None)
    ctx.decode_chunks_schedule_post(table.data_ptr(), stride, n, dsts[1], 0, cs, [1, 3], None, None)
    evs = [native.NativeEvent() for _ in range(2)]
    ctx.decode_chunks_schedule_post(table.data_ptr(), stride, n, dsts[2], 0, cs, [1, 3], evs, native.RangePost().struct(0, T))
    evs[-1].synchronize()
    torch.cuda.synchronize()
    ctx.raise_on_status("decode")
    assert float(outs[0].float().abs().max()) > 0
    assert torch.equal(_ibits(outs[0]), _ibits(outs[1])) and torch.equal(_ibits(outs[0]), _ibits(outs[2]))
    # a post-op that does not check out is refused before anything is queued: a uniform delta outside the table, a scatter into rows
    bad = native.RangePost(cos_sin=_table(64)[0], rot_dim=64, delta=ROWS)
    with pytest.raises(native.NativeError):
        ctx.decode_chunks_schedule_post(table.data_ptr(), stride, n, dsts[1], 0, cs, [1, 3], None, bad.struct(0, T))
    rows_scatter = native.RangePost(scatter_dst=dsts[2])
    with pytest.raises(native.NativeError):
        ctx.decode_chunks_schedule_post(table.data_ptr(), stride, n, dsts[1], 0, cs, [1, 3], None, rows_scatter.struct(0, T))
    torch.cuda.synchronize()
    assert torch.equal(_ibits(outs[0]), _ibits(outs[1])) and ctx.status(clear=True) == 0


def test_layer_window_rotates_its_layers_only(ctx):
    """KVLayout.layers(l0, nl) is the window the C side cuts for a range's post-op: a rotation of the window of a chunk
    and of a plane-table layout leaves what the rotation of the whole layout leaves in those layers, and nothing elsewhere."""
    H, D, rot, Lw = 2, 64, 64, 3
    g = torch.Generator().manual_seed(41)
    table, _ = _table(rot)
    deltas = torch.randint(-(ROWS - 1), ROWS, (NTOK,), generator=g, dtype=torch.int32).to(DEV)
    chunk = _random_bits((Lw, 2, NTOK, H, D), torch.bfloat16, g)
    chunk[:, 0] = _finite_keys((Lw, NTOK, H, D), torch.bfloat16, g)
    for form in ("base", "plane_table"):
        whole, part = chunk.to(DEV), chunk.to(DEV)

        def layout(t):
            if form == "base":
                return native.KVLayout.from_chunk(t, "vllm")
            return native.KVLayout.from_kv_tuple(tuple((t[l, 0], t[l, 1]) for l in range(Lw)), "vllm")
        ctx.rope_shift(layout(whole), 0, NTOK, table, rot, True, deltas=deltas)
        ctx.rope_shift(layout(part).layers(1, 2), 0, NTOK, table, rot, True, deltas=deltas)
        torch.cuda.synchronize()
        assert torch.equal(_ibits(part[1:]), _ibits(whole[1:])), form
        assert torch.equal(_ibits(part[0].cpu()), _ibits(chunk[0])), form
        assert not torch.equal(_ibits(part[1].cpu()), _ibits(chunk[1])), form
    assert ctx.status(clear=True) == 0
