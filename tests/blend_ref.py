"""Numpy statements of lmc_kv_deviation and lmc_select_topk (include/lmc_hip.h), shared by tests/test_blend_host.py and
tests/test_gpu_blend.py.

Both work on the LOGICAL view of a KV cache, [L, 2, T, H, D] -- the view the layout helpers of
tests/test_gpu_rope_shift.py (_mapping, _random_bits) place into chunks, tuples and paged blocks -- so that a reference
never knows where a layout keeps a token."""
import numpy as np
import torch


def logical(t: torch.Tensor) -> np.ndarray:
    """A 16-bit float tensor as float64 (exact)."""
    return t.detach().cpu().to(torch.float64).numpy()


def deviation_ref(A, a_layer, a_tok0, B, b_layer, b_tok0, ntok, kv):
    """dev[i] = sum over (h, d) of (A[a_layer, kv, a_tok0 + i] - B[b_layer, kv, b_tok0 + i])^2 for logical views
    A [La, 2, Ta, H, D] and B [Lb, 2, Tb, H, D] (float64 arrays): in int64 when every value involved is an integer (the
    sum is then exact and any order of additions must give it), in float64 otherwise."""
    a = np.asarray(A)[a_layer, kv, a_tok0:a_tok0 + ntok].reshape(ntok, -1)
    b = np.asarray(B)[b_layer, kv, b_tok0:b_tok0 + ntok].reshape(ntok, -1)
    assert a.shape == b.shape and a.shape[0] == ntok
    finite = np.isfinite(a).all() and np.isfinite(b).all()
    if finite and np.array_equal(a, np.rint(a)) and np.array_equal(b, np.rint(b)):
        d = a.astype(np.int64) - b.astype(np.int64)
        return (d * d).sum(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        d = a.astype(np.float64) - b.astype(np.float64)
        return (d * d).sum(axis=1)


def topk_keys(dev) -> np.ndarray:
    """The selection key of every entry: the fp32 bit pattern without its sign, as an unsigned integer."""
    return (np.ascontiguousarray(dev, np.float32).view(np.uint32) & np.uint32(0x7fffffff)).astype(np.int64)


def topk_ref(dev, k: int) -> np.ndarray:
    """The min(k, n) indices with the largest key, ties to the lower index, ascending: a stable ordering by (-key, index),
    its first entries, sorted."""
    key = topk_keys(dev)
    n = len(key)
    order = np.lexsort((np.arange(n), -key))  # last key is the primary one
    return np.sort(order[:max(0, min(k, n))]).astype(np.int32)
