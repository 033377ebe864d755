"""The serial part of a fused-encode work item (k_fused.h: the ticket with the table copy and the histogram's zero fill
under it and one barrier for all three; the scales' checksum, token 0 of a byte plane and the look-back between quantise
and coding): whole blobs, their sizes and the status word of the fused kernel against the two-kernel path and the oracle,
at the smallest shapes that reach each of those lines.  Jobs this small are far below the threshold at which AUTO picks
the fused kernel, so the path is forced, as tests/test_gpu_parity.py does."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def nat():
    from lmcache_amd import native
    native.lib()
    return native


@pytest.fixture(scope="module")
def ctx(nat):
    return nat.get_context(0)


def kv_bins(L):
    """32 bins on every K plane, 16 on every V plane: byte counters and nibble counters in one job -- and, for narrow
    planes, side by side in one work item."""
    return [32] * L + [16] * L


def encode(nat, ctx, path, layout, tok_end, cs, bins):
    """-> (blobs as bytes, sizes, status word) of one job through the launch path `path`."""
    L, H, D = layout.L, layout.H, layout.D
    stride = nat.r16(nat.blob_bound(L, cs, H, D))
    n = (tok_end + cs - 1) // cs
    blobs = torch.zeros(n * stride, dtype=torch.uint8, device=DEV)
    sizes = torch.zeros(n, dtype=torch.int32, device=DEV)
    ctx.set_encode_path(path)
    try:
        ctx.encode_chunks(layout, 0, tok_end, cs, bins, blobs.data_ptr(), stride, sizes.data_ptr())
        torch.cuda.synchronize()
    finally:
        ctx.set_encode_path("auto")
    status = ctx.status(clear=True)
    sz = sizes.cpu().tolist()
    host = blobs.cpu().numpy()
    return [host[i * stride:i * stride + sz[i]].tobytes() for i in range(n)], sz, status


def check_job(nat, ctx, oracle, kv, layout, cs, bins, tag):
    """kv [L, 2, T, H, D] on the host is what `layout` holds: both paths' blobs, sizes and status against the oracle."""
    L, _, Ttot, H, D = kv.shape
    fused, fsz, fst = encode(nat, ctx, "fused", layout, Ttot, cs, bins)
    two, tsz, tst = encode(nat, ctx, "two_kernels", layout, Ttot, cs, bins)
    assert fst == 0 and tst == 0, f"{tag}: status fused {fst}, two kernels {tst}"
    n = (Ttot + cs - 1) // cs
    assert len(fused) == len(two) == n, tag
    assert fsz == tsz, f"{tag}: sizes {fsz} vs {tsz}"
    for i in range(n):
        t0, t1 = i * cs, min(Ttot, (i + 1) * cs)
        b, code = oracle.torch_to_bits(kv[:, :, t0:t1].reshape(L, 2, t1 - t0, H * D))
        ref = oracle.encode_blob(b, code, H, D, np.array(bins, np.int32))
        assert fsz[i] == len(ref), f"{tag}: size of chunk {i}"
        assert two[i] == ref, f"{tag}: two-kernel path, chunk {i}"
        assert fused[i] == ref, f"{tag}: fused path, chunk {i}"
        hdr = nat.blob_info(fused[i])
        # the section this file is about: one checksum word per plane behind the scales
        assert fused[i][hdr.off_scsum:hdr.off_scsum + 8 * L] == ref[hdr.off_scsum:hdr.off_scsum + 8 * L], f"{tag}: scsum, chunk {i}"


GEOMETRIES = [
    # L, H, D: what the shape reaches
    (1, 8, 128),  # C = 1024: two channel runs per lane, no absent channels (the FULL quantise variant)
    (1, 4, 128),  # C = 512: one channel run per lane
    (1, 3, 128),  # C = 384: lanes without channels
    (1, 2, 128),  # C = 256: narrow planes, the K and the V plane in ONE work item (quantize_task, two octs per wave pass)
    (2, 1, 128),  # C = 128: four planes in one work item, four octs per wave pass
]


@pytest.mark.parametrize("cs", [256, 32, 40], ids=lambda c: f"cs{c}")
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("geo", GEOMETRIES, ids=lambda g: f"L{g[0]}C{g[1] * g[2]}")
def test_geometries_bins_and_chunk_lengths(nat, ctx, oracle, geo, dtype, cs):
    """Two chunks of 256 / 32 / 40 tokens (40: a last oct with absent rows) per geometry and dtype."""
    L, H, D = geo
    g = torch.Generator().manual_seed(1000 * H + cs)
    kv = torch.randn(L, 2, 2 * cs, H, D, generator=g).to(dtype)
    lay = nat.KVLayout.from_chunk(kv.to(DEV), "vllm")
    check_job(nat, ctx, oracle, kv, lay, cs, kv_bins(L), f"L{L} H{H} D{D} cs{cs}")


def test_lookbacks_across_many_workgroups(nat, ctx, oracle):
    """16 chunks x 8 planes = 128 work items: every look-back but a chunk's first reads granules other workgroups wrote,
    most of them while those are still running."""
    L, H, D, cs, n = 4, 4, 128, 32, 16
    g = torch.Generator().manual_seed(16)
    kv = torch.randn(L, 2, n * cs, H, D, generator=g).to(torch.bfloat16)
    lay = nat.KVLayout.from_chunk(kv.to(DEV), "vllm")
    check_job(nat, ctx, oracle, kv, lay, cs, kv_bins(L), "128 items")


@pytest.mark.parametrize("H", [8, 2], ids=["C1024", "C256_two_planes_per_item"])
def test_special_rows_and_constant_channels(nat, ctx, oracle, H):
    """All-zero, inf and NaN rows, each at token 0 of a chunk and elsewhere, in byte planes (K, 32 bins: token 0 is left
    out of the counters and added back by pass 1) and nibble planes (V); a channel constant over a chunk (its counter reads
    255: nothing is added back) and one constant everywhere except token 0."""
    L, D, cs, T = 2, 128, 256, 512
    g = torch.Generator().manual_seed(50 + H)
    x = torch.randn(L, 2, T, H, D, generator=g)
    big = x.abs().amax(dim=(-1, -2))           # [L, 2, T]
    x[:, :, :, 0, 5] = 0.0                      # constant over every chunk (the middle symbol)
    x[:, :, :, 0, 6] = 0.0                      # ... except token 0 of every chunk, which carries the row max
    x[:, :, 0::cs, 0, 6] = big[:, :, 0::cs]
    x[:, :, :, H - 1, 9] = -big                 # symbol 0 every token
    x[0, 0, 0] = 0.0                            # zero row: token 0, byte plane
    x[0, 0, 100] = 0.0                          # ... elsewhere
    x[0, 1, cs] = 0.0                           # ... token 0 of the second chunk, nibble plane
    x[0, 1, cs + 9] = 0.0
    x[1, 0, 0, 0, 3] = float("inf")             # inf row: token 0, byte plane
    x[1, 0, 77, H - 1, 100] = float("-inf")
    x[1, 1, 0, 0, 0] = float("inf")             # ... nibble plane
    x[1, 1, 300, 0, 64] = float("inf")
    x[0, 0, cs, 0, 7] = float("nan")            # NaN row: token 0 of the second chunk, byte plane
    x[0, 0, cs + 50, H - 1, 1] = float("nan")
    x[1, 1, cs, 0, 2] = float("nan")            # ... nibble plane
    x[1, 1, cs + 200, 0, 2] = float("nan")
    kv = x.to(torch.bfloat16)
    lay = nat.KVLayout.from_chunk(kv.to(DEV), "vllm")
    check_job(nat, ctx, oracle, kv, lay, cs, kv_bins(L), f"special rows, H{H}")


def test_paged_source_with_a_power_of_two_block_size(nat, ctx, oracle):
    """The kernel instance of a paged source whose block size is a power of two (slots by scalar loads)."""
    L, T, H, D, bs, nb, cs = 1, 512, 8, 128, 16, 35, 256
    g = torch.Generator().manual_seed(31)
    caches = [torch.randn((2, nb, bs, H, D), generator=g).to(torch.bfloat16).to(DEV) for _ in range(L)]
    slots = torch.randperm(nb * bs, generator=g)[:T]
    lay = nat.KVLayout.paged(caches, slots, bs, "NBHD")
    dense = torch.zeros(L, 2, T, H, D, dtype=torch.bfloat16)
    blk, w = slots // bs, slots % bs
    for l in range(L):
        dense[l] = caches[l].cpu()[:, blk, w]
    check_job(nat, ctx, oracle, dense, lay, cs, kv_bins(L), "paged source")
