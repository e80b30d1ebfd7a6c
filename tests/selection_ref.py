"""Exact references for the kernels that produce INDICES (top-k of the decode, the kNN graph of DGCNNAttn), in numpy / fp64.

One rule for both: a stable sort by (value descending, flat index ascending) - among equal values the lower index comes first.
That is the rule gd4d_nms_free_decode_fwd ("lowest flat indices win") and gd4d_knn_farthest_fwd ("ties to the lower column")
state in their sources.  tests/test_selection_ref_cpu.py checks these functions against torch.topk without a GPU."""
import numpy as np


def topk_stable(values, k):
    """values: 1-D array-like.  Indices (int64) of the k largest entries: value descending, ties by ascending index."""
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    if not 0 < k <= v.size:
        raise ValueError(f'k = {k} out of range for {v.size} values')
    return np.argsort(-v, kind='stable')[:k].astype(np.int64)


def sq_dists(x):
    """x (B, N, C) -> fp64 squared euclidean distances (B, N, N), summed as differences (no |a|^2 + |b|^2 - 2ab cancellation)."""
    x = np.asarray(x, dtype=np.float64)
    out = np.empty((x.shape[0], x.shape[1], x.shape[1]), dtype=np.float64)
    for b in range(x.shape[0]):
        for i in range(x.shape[1]):
            e = x[b] - x[b, i]
            out[b, i] = np.einsum('nc,nc->n', e, e)
    return out


def knn_farthest_ref(x, k):
    """x (B, N, C) -> (B, N, k) int64: per row the k FARTHEST rows of the same sample (DGCNNAttn's choice), by fp64 squared
    distance, ties by ascending column."""
    d = sq_dists(x)
    if not 0 < k <= d.shape[-1]:
        raise ValueError(f'k = {k} out of range for {d.shape[-1]} rows')
    return np.argsort(-d, axis=-1, kind='stable')[..., :k].astype(np.int64)
