"""tests/selection_ref.py (the exact references of the GPU selection tests) against torch.topk on tie-free inputs, and its tie
rule on hand-written cases.  No GPU."""
import numpy as np
import pytest
import torch

from selection_ref import knn_farthest_ref, sq_dists, topk_stable


@pytest.mark.parametrize('n,k', [(1, 1), (7, 3), (310, 300), (9010, 1024), (4096, 4096)])
def test_topk_stable_equals_torch_topk_without_ties(n, k):
    g = torch.Generator().manual_seed(n + k)
    v = torch.randperm(n, generator=g).double() * 0.25 - 3.0          # distinct by construction
    want = torch.topk(v, k, largest=True, sorted=True).indices
    got = topk_stable(v.numpy(), k)
    assert got.dtype == np.int64 and got.shape == (k,)
    assert np.array_equal(got, want.numpy())


def test_topk_stable_tie_rule():
    #            0    1    2    3    4    5    6    7
    v = [1.0, 3.0, 1.0, 3.0, 0.5, 3.0, 1.0, -2.0]
    assert topk_stable(v, 8).tolist() == [1, 3, 5, 0, 2, 6, 4, 7]
    assert topk_stable(v, 2).tolist() == [1, 3]                       # the tie class is cut: lowest indices
    assert topk_stable(v, 4).tolist() == [1, 3, 5, 0]
    assert topk_stable(np.zeros(5), 3).tolist() == [0, 1, 2]
    assert topk_stable([0.0, -0.0, 0.0], 3).tolist() == [0, 1, 2]     # signed zeros are equal
    assert topk_stable(np.float32([0.5, 0.5, 1.0]), 2).tolist() == [2, 0]
    for bad in (0, 9):
        with pytest.raises(ValueError):
            topk_stable(v, bad)


@pytest.mark.parametrize('b,n,c,k', [(1, 1, 4, 1), (2, 70, 256, 16), (1, 65, 4, 65), (3, 200, 12, 16)])
def test_knn_farthest_ref_equals_cdist_topk_without_ties(b, n, c, k):
    g = torch.Generator().manual_seed(100 * n + c)
    x = torch.randn(b, n, c, generator=g)
    xd = x.double()
    dist = torch.cdist(xd, xd, compute_mode='donot_use_mm_for_euclid_dist')
    d2 = sq_dists(x.numpy())
    off = ~np.eye(n, dtype=bool)
    # tie-free: any two distances of a row differ by far more than the rounding of either evaluation
    srt = np.sort(d2, axis=-1)
    assert n < 3 or float(np.diff(srt, axis=-1)[..., 1:].min()) > 1e-9
    np.testing.assert_allclose(np.sqrt(d2)[:, off], dist.numpy()[:, off], rtol=1e-12, atol=0)
    want = torch.topk(dist, k, dim=-1, largest=True, sorted=True).indices
    got = knn_farthest_ref(x.numpy(), k)
    assert got.dtype == np.int64 and got.shape == (b, n, k)
    assert np.array_equal(got, want.numpy())


def test_knn_farthest_ref_tie_rule():
    # four corners of a square and its centre, twice (rows 5..9 duplicate rows 0..4), padded to 4 channels
    pts = [[0, 0], [2, 0], [0, 2], [2, 2], [1, 1]]
    x = np.zeros((1, 10, 4))
    x[0, :5, :2] = pts
    x[0, 5:, :2] = pts
    idx = knn_farthest_ref(x, 10)[0]
    # from corner 0: the opposite corner (rows 3, 8: d2 = 8), the adjacent corners (1, 2, 6, 7: 4), the centres (4, 9: 2),
    # itself and its duplicate (0, 5: 0) - inside each class ascending
    assert idx[0].tolist() == [3, 8, 1, 2, 6, 7, 4, 9, 0, 5]
    assert idx[5].tolist() == idx[0].tolist()                         # the duplicate row sees the same distances
    # from the centre: every corner at d2 = 2, then the two centres
    assert idx[4].tolist() == [0, 1, 2, 3, 5, 6, 7, 8, 4, 9]
    assert knn_farthest_ref(x, 3)[0, 4].tolist() == [0, 1, 2]
    # all rows identical: every distance 0, the first k columns
    same = np.ones((2, 6, 4))
    assert np.array_equal(knn_farthest_ref(same, 4), np.broadcast_to(np.arange(4), (2, 6, 4)))
    with pytest.raises(ValueError):
        knn_farthest_ref(same, 7)
