"""gd4d_knn_farthest_fwd / gd4d_edge_conv_max_fwd called directly: the kNN graph against an exact fp64 reference (tests/selection_ref.py,
checked without a GPU by tests/test_selection_ref_cpu.py), the edge convolution against its formula in fp64 under a derived
rounding bound.  GPU only."""
import numpy as np
import pytest
import torch

from selection_ref import knn_farthest_ref, sq_dists

pytestmark = pytest.mark.gpu


def _lattice(b, n, c, seed):
    """Integer coordinates in [-8, 8]: with C <= 256 every squared distance is an integer <= 256 * 16^2 = 65536, exact in fp32
    whatever the order of the fused multiply-adds - equal distances are true ties on the device as well."""
    assert c <= 256
    return torch.randint(-8, 9, (b, n, c), generator=torch.Generator().manual_seed(seed)).float()


def _knn(x, k):
    from graph_detr4d_amd import ops
    idx = ops.knn_farthest_fwd(x.cuda(), k)
    assert idx.dtype == torch.int32 and idx.shape == (*x.shape[:2], k)
    return idx.cpu().long()


@pytest.mark.parametrize('b,n,c,k', [
    (1, 1, 4, 1),              # smallest
    (1, 63, 4, 16),            # one lane short of a wave
    (1, 64, 8, 16),            # exactly one wave, one slot
    (1, 65, 4, 65),            # K = N: the row itself comes last; a second slot in lane 0 only
    (3, 70, 256, 16),          # batched
    (2, 900, 256, 16),         # the workload's
    (1, 2048, 4, 16),          # all 32 slots of every lane
    (1, 1000, 12, 1000),       # K = N, large
])
def test_knn_exact_on_a_lattice(b, n, c, k):
    x = _lattice(b, n, c, 7 * n + c)
    want = knn_farthest_ref(x.numpy(), k)
    if c == 4:                                     # few channels on a 17-point lattice: the case really has ties inside the top k
        d = np.take_along_axis(sq_dists(x.numpy()), want, axis=-1)
        assert n < 2 or bool((d[..., 1:] == d[..., :-1]).any())
    assert torch.equal(_knn(x, k), torch.from_numpy(want))


def test_knn_duplicated_and_identical_rows():
    x = _lattice(2, 70, 8, 3)
    x[0, 40:50] = x[0, 3]                          # ten copies of one row: equal columns in every row's distances
    x[1, 69] = x[1, 0]
    x[1, 64] = x[1, 1]                             # a tie between slot 0 of one lane and slot 1 of another
    assert torch.equal(_knn(x, 16), torch.from_numpy(knn_farthest_ref(x.numpy(), 16)))
    assert torch.equal(_knn(x, 70), torch.from_numpy(knn_farthest_ref(x.numpy(), 70)))
    same = torch.full((2, 130, 12), 3.0)           # every distance 0: the first K columns, in order
    assert torch.equal(_knn(same, 100), torch.arange(100).expand(2, 130, 100))


def test_knn_errors():
    from graph_detr4d_amd import ops
    from graph_detr4d_amd._lib import Gd4dError
    with pytest.raises(Gd4dError):
        ops.knn_farthest_fwd(torch.zeros(1, 2049, 4).cuda(), 16)          # more than 32 slots per lane
    with pytest.raises(Gd4dError):
        ops.knn_farthest_fwd(torch.zeros(1, 70, 6).cuda(), 16)            # C % 4 != 0
    with pytest.raises(Gd4dError):
        ops.knn_farthest_fwd(torch.zeros(1, 70, 8).cuda(), 71)            # K = N + 1


def test_knn_batch_isolation():
    """A B = 3 call equals the three B = 1 calls bit for bit, and no index leaves [0, N) (an index into another sample would)."""
    b, n, c, k = 3, 130, 64, 16
    x = torch.randn(b, n, c, generator=torch.Generator().manual_seed(9))
    x[1] *= 100.0                                  # samples of very different scale: a row of another sample would win
    together = _knn(x, k)
    assert int(together.min()) >= 0 and int(together.max()) < n
    for s in range(b):
        assert torch.equal(together[s:s + 1], _knn(x[s:s + 1].contiguous(), k))


def _swapped_rows(idx, d64, c):
    """Rows of idx (N, K) that differ from the fp64 order, after checking that every difference is one fp32 may make.
    An fp32 sum of C squares of fp32 differences carries a relative error of at most gamma = (C + 2) 2^-24 (one rounding per
    difference and square, C accumulations), so two columns whose computed order differs from the fp64 one are at most
    2 gamma max(d) apart in fp64.  Derived, not measured."""
    n, k = idx.shape
    want = np.argsort(-d64, axis=-1, kind='stable')[:, :k]
    gamma = (c + 2) * 2.0 ** -24
    got_d, want_d = np.take_along_axis(d64, idx, -1), np.take_along_axis(d64, want, -1)
    cap = 2.0 * gamma * d64.max(axis=-1, keepdims=True)
    differs = idx != want
    assert bool((np.abs(got_d - want_d)[differs] <= np.broadcast_to(cap, idx.shape)[differs]).all()), 'a swap beyond the fp32 rounding bound'
    assert all(len(set(r)) == k for r in idx.tolist()), 'a column chosen twice'
    return int(differs.any(axis=-1).sum())


def test_knn_floats_swap_only_within_rounding():
    b, n, c, k = 1, 900, 256, 16
    x = torch.randn(b, n, c, generator=torch.Generator().manual_seed(4))
    d64 = sq_dists(x.numpy())[0]
    # the seed is usable: a plain fp32 evaluation of the same distances on the CPU stays inside the cap
    xf = x[0].numpy()
    d32 = np.stack([np.square(xf - xf[i]).sum(axis=-1, dtype=np.float32) for i in range(n)])
    cpu_idx = np.argsort(-d32.astype(np.float64), axis=-1, kind='stable')[:, :k]
    cpu_rows = _swapped_rows(cpu_idx, d64, c)
    gpu_rows = _swapped_rows(_knn(x, k)[0].numpy(), d64, c)
    print(f'rows with a swap inside the bound: numpy fp32 {cpu_rows}, device {gpu_rows} of {n}')
    assert cpu_rows <= 0.02 * n
    assert gpu_rows <= 0.02 * n


# ---------------------------------------------------------------------------------------------------------------------
# gd4d_edge_conv_max_fwd: out[b, n, c] = max_k relu((a[b, idx[b, n, k], c] + b_self[b, n, c]) * scale[c] + shift[c])
# ---------------------------------------------------------------------------------------------------------------------
def _edge_reference(ab, idx, scale, shift):
    """fp64 value and the per-element bound 3 * 2^-24 * (|(a + b) scale| + |shift|): three fp32 roundings (the add, the multiply,
    the add of the shift; two when the last two fuse), each at most 2^-24 of a magnitude no larger than |(a + b) scale| + |shift|.
    ReLU and max are 1-Lipschitz: the bound of the output is the largest bound among its K candidates.  Derived."""
    b, n, c2 = ab.shape
    c = c2 // 2
    a, bs = ab[..., :c].double(), ab[..., c:].double()
    sc, sh = scale.double(), shift.double()
    out, bound = torch.empty(b, n, c, dtype=torch.float64), torch.empty(b, n, c, dtype=torch.float64)
    for s in range(b):
        for lo in range(0, n, 64):                                   # (chunks of rows: K = N = 900 stays small)
            prod = (a[s][idx[s, lo:lo + 64]] + bs[s, lo:lo + 64, None, :]) * sc          # (rows, K, C)
            out[s, lo:lo + 64] = (prod + sh).clamp(min=0).amax(dim=1)
            bound[s, lo:lo + 64] = (3.0 * 2.0 ** -24 * (prod.abs() + sh.abs())).amax(dim=1)
    return out, bound


def _edge_inputs(n, c, seed, b=2):
    g = torch.Generator().manual_seed(seed)
    ab = torch.randn(b, n, 2 * c, generator=g) * 2.0
    scale = torch.randn(c, generator=g)                              # both signs
    scale[0] = -abs(scale[0]) - 0.5
    shift = torch.randn(c, generator=g)
    return ab, scale, shift


def _edge(ab, idx, scale, shift):
    from graph_detr4d_amd import ops
    out = ops.edge_conv_max_fwd(ab.cuda(), idx.int().cuda(), scale.cuda(), shift.cuda()).cpu()
    assert out.shape == (*ab.shape[:2], ab.shape[2] // 2) and out.dtype == torch.float32
    return out


def _check_edge(ab, idx, scale, shift):
    got = _edge(ab, idx, scale, shift)
    want, bound = _edge_reference(ab, idx, scale, shift)
    excess = (got.double() - want).abs() - bound
    assert bool((excess <= 0).all()), f'largest excess over the bound {float(excess.max()):.3e} at {np.unravel_index(int(excess.argmax()), excess.shape)}'
    assert bool((got >= 0).all())
    return got


@pytest.mark.parametrize('n,k,c', [
    (1, 1, 4),                 # smallest; K = N
    (70, 1, 64),               # K = 1
    (70, 16, 256),             # one full trip of the channel loop
    (70, 70, 260),             # K = N; a second, partial trip (one lane)
    (70, 16, 512),             # two full trips
    (900, 16, 256),            # the workload's
    (900, 16, 260),
    (900, 1, 512),
    (900, 900, 4),             # K = N, large; one lane of the wave active
])
def test_edge_conv_max_matches_fp64(n, k, c):
    ab, scale, shift = _edge_inputs(n, c, 50 * n + c + k)
    x = torch.randn(2, n, 8, generator=torch.Generator().manual_seed(n + k))
    idx = _knn(x, k)                                                 # the graph the module feeds it
    assert int(idx.min()) >= 0 and int(idx.max()) < n
    _check_edge(ab, idx, scale, shift)


@pytest.mark.parametrize('n,k,c', [(70, 16, 260), (900, 16, 256)])
def test_edge_conv_max_adversarial_indices_and_all_negative(n, k, c):
    ab, scale, shift = _edge_inputs(n, c, 11 * n + c)
    for fill in (n - 1, 0):                                          # every neighbour the last / the first row of the sample
        _check_edge(ab, torch.full((2, n, k), fill, dtype=torch.int64), scale, shift)
    # sample 1's answer must come from sample 1's rows: the same indices on a sample 1000 x larger
    ab[1] *= 1000.0
    idx = torch.randint(0, n, (2, n, k), generator=torch.Generator().manual_seed(5))
    _check_edge(ab, idx, scale, shift)
    # a shift so negative that every candidate is below zero: ReLU gives exactly 0 everywhere
    got = _edge(ab, idx, scale, torch.full((c,), -1e8))
    assert torch.equal(got, torch.zeros_like(got))
