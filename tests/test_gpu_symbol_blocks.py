"""The coder's symbol-block loads (k_encode_counts.h: sym_blocks_of -- a wave-uniform buffer descriptor over the stream's
plane-chunk region of the workspace, the lane's channel in the vector offset, the dword row in the scalar offset; a lane
without a channel and a row behind the chunk's last one read 0 by the descriptor's range, not under an exec mask).

Both launch paths, forced: "fused" (k_encode_fused: pass 2's loop, and for planes of 120 channels pass 1's loop too) and
"two_kernels" (k_cdf_encode<.., 8, true>: both loops).  One layer = two planes, bins [16, 32] and [32, 16]: both loop
variants (four dwords per 32-token block of a nibble plane, eight of a byte plane), each as the first and as the second
stream of a wave.  Chunk lengths: 32 = one block (the loop's prefetch guard is never true), 64 = two blocks, 40 = a
partial block in front of one whole block, 256.  Channels: 1024; 520 = 8 full groups and one of 8 active lanes (the
other 56 lanes read nothing); 120 = narrow planes, a last group of 56.  Inputs: uniform noise, and the same with the K
plane constant (every channel equal: single-symbol tables under the new loads).

Every blob is byte-identical to the CPU oracle's and to the other path's, the encode's status is 0, and the decoded KV
lies within the quantiser's bound |x^ - x| <= max1 / (2 M) + max1 2^-7 per token row and plane (bench.py: shape_rate's
round-trip check)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NCHUNKS = 2
SHAPES = [(8, 128), (5, 104), (3, 40)]  # H, D: 1024, 520 and 120 channels
CHUNKS = [32, 64, 40, 256]
BINS = [(16, 32), (32, 16)]


@pytest.fixture(scope="module")
def nat():
    from lmcache_amd import native
    native.lib()
    return native


@pytest.fixture(scope="module")
def ctx(nat):
    return nat.get_context(0)


def make_kv(H, D, T, dtype, kind):
    g = torch.Generator().manual_seed(1000 * H + T)
    kv = torch.rand(1, 2, NCHUNKS * T, H, D, generator=g)
    if kind == "const_plane":
        kv[0, 0] = 0.625
    return kv.to(dtype)


def encode(nat, ctx, path, kv_dev, T, bins):
    _, _, ntok, H, D = kv_dev.shape
    stride = nat.r16(nat.blob_bound(1, T, H, D))
    n = ntok // T
    arena = torch.zeros(n * stride, dtype=torch.uint8, device=DEV)
    sizes = torch.zeros(n, dtype=torch.int32, device=DEV)
    ctx.set_encode_path(path)
    try:
        ctx.encode_chunks(nat.KVLayout.from_chunk(kv_dev, "vllm"), 0, ntok, T, list(bins), arena.data_ptr(), stride, sizes.data_ptr())
        torch.cuda.synchronize()
    finally:
        ctx.set_encode_path("auto")
    assert ctx.status(clear=True) == 0, f"{path}: encode status"
    sz = sizes.cpu().tolist()
    host = arena.cpu().numpy()
    return [host[i * stride:i * stride + sz[i]].tobytes() for i in range(n)], arena, stride


@pytest.mark.parametrize("kind", ["rand", "const_plane"])
@pytest.mark.parametrize("T", CHUNKS)
@pytest.mark.parametrize("bins", BINS, ids=lambda b: f"bins{b[0]}_{b[1]}")
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("hd", SHAPES, ids=lambda s: f"C{s[0] * s[1]}")
def test_symbol_blocks_blobs_equal_oracle_on_both_paths(nat, ctx, oracle, hd, dtype, bins, T, kind):
    H, D = hd
    kv = make_kv(H, D, T, dtype, kind)
    kv_dev = kv.to(DEV)
    refs = []
    for i in range(NCHUNKS):
        b, code = oracle.torch_to_bits(kv[:, :, i * T:(i + 1) * T].reshape(1, 2, T, H * D))
        refs.append(oracle.encode_blob(b, code, H, D, np.array(bins, np.int32)))
    got = {}
    for path in ("fused", "two_kernels"):
        blobs, arena, stride = encode(nat, ctx, path, kv_dev, T, bins)
        got[path] = blobs
        for i in range(NCHUNKS):
            assert len(blobs[i]) == len(refs[i]), f"{path}: chunk {i}: size"
            assert blobs[i] == refs[i], f"{path}: chunk {i}: bytes"
        out = torch.zeros_like(kv_dev)
        ctx.decode_chunks(arena.data_ptr(), stride, NCHUNKS, nat.KVLayout.from_chunk(out, "vllm"), 0, T)
        torch.cuda.synchronize()
        assert ctx.status(clear=True) == 0, f"{path}: decode status"
        y = out.cpu().float()
        for kvi in range(2):
            x = kv[0, kvi].float()
            mx = x.abs().amax(dim=(1, 2), keepdim=True)
            m = bins[kvi] // 2 - 1
            assert bool(((y[0, kvi] - x).abs() <= mx / (2 * m) + mx * 2.0 ** -7).all()), f"{path}: plane {kvi}: round trip"
    assert got["fused"] == got["two_kernels"]
