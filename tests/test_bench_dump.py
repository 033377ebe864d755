"""bench.py --dump-outputs: what the timed step computed, written as float arrays that two builds can be compared by --
the same blobs give the same files, whatever lies in the arena's slack, and a changed byte shows."""
import os

import numpy as np
import pytest
import torch

import bench

NAMES = ("sizes", "blob_checksums", "blob_sample")


def _dump(path, blobs, sizes, stride, n):
    bench.dump_outputs(str(path), blobs, sizes, stride, n)
    return {k: np.load(os.path.join(str(path), k + ".npy")) for k in NAMES}


def test_dump_outputs_exact_deterministic_and_blind_to_slack(tmp_path):
    stride = 4096
    blobs = torch.randint(0, 256, (3 * stride,), generator=torch.Generator().manual_seed(0), dtype=torch.uint8)
    sizes = torch.tensor([4000, 17, 0], dtype=torch.int32)
    a = _dump(tmp_path / "a", blobs, sizes, stride, 3)
    for k in NAMES:
        assert a[k].dtype in (np.float32, np.float64), k
    assert a["sizes"].tolist() == [4000.0, 17.0, 0.0]
    assert a["blob_sample"].shape == (3, bench.DUMP_SAMPLE_BYTES)
    b0 = blobs[:4000].numpy().astype(np.int64)
    assert a["blob_checksums"][0].tolist() == [float(b0.sum()), float((b0 * (np.arange(4000) % 65521 + 1)).sum())]
    assert np.array_equal(a["blob_sample"][0, :256], b0[:256])
    assert set(a["blob_sample"][1].astype(np.int64)) <= set(blobs[stride:stride + 17].tolist())
    assert not a["blob_sample"][2].any() and not a["blob_checksums"][2].any()

    slack = blobs.clone()
    slack[4000:stride] = 7          # bytes after a blob's size are not output
    slack[stride + 17:2 * stride] = 9
    b = _dump(tmp_path / "b", slack, sizes, stride, 3)
    for k in NAMES:
        assert np.array_equal(a[k], b[k]), k

    flipped = blobs.clone()
    flipped[stride + 5] ^= 1
    c = _dump(tmp_path / "c", flipped, sizes, stride, 3)
    assert not np.array_equal(a["blob_checksums"], c["blob_checksums"])


def test_dump_outputs_fit_the_budget_at_the_bench_shape():
    n = bench.CTX // bench.CHUNK
    assert n * bench.DUMP_SAMPLE_BYTES * 4 + n * 2 * 8 + n * 8 <= 64 << 20


def test_profile_legs_belong_to_full():
    with pytest.raises(SystemExit):
        bench.main(["--profile-legs"])
