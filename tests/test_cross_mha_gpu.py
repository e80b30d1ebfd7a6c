"""gd4d_cross_mha_fwd / gd4d_cross_mha_pack_kv (PETR's global cross-attention core) against fp64 on the full tensor.

Tolerances are those of tests/test_dense_gpu.py::test_mha_core_matches_fp64 for split-bf16 arithmetic with fp32 accumulation (here
six bf16 MFMAs for the scores, three for P V): max < 1e-4 and median < 5e-6, lse max < 1e-4, asserted in every case.  The fp64 reference is tests/petr_ref.py (torch ops in
float64, on the device); every case prints its figures before it asserts."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import petr_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
H, C = 8, 256


def _inputs(lq, lk, b, seed=None, packed=True):
    g = torch.Generator().manual_seed(1000 * lq + lk + b if seed is None else seed)
    q = torch.randn(lq, b, C, generator=g).to(DEV)
    kvp = torch.randn(lk, b, 2 * C, generator=g).to(DEV)
    if packed:                                   # the two halves of one projection buffer, as the module hands them over
        return q, kvp[..., :C], kvp[..., C:]
    return q, kvp[..., :C].contiguous(), kvp[..., C:].contiguous()


def _random_mask(lk, b, seed, p=0.3):
    g = torch.Generator().manual_seed(seed)
    m = torch.rand(b, lk, generator=g) < p       # differs per batch
    m[:, int(torch.randint(0, lk, (1,), generator=g))] = False      # (never a fully masked row here)
    return m.to(DEV)


def _within(out, lse, ref, ref_lse):
    """The three bounds, on whatever part of the tensors is handed in; prints the figures first."""
    err = (out.double() - ref).abs()
    e_max, e_med, e_lse = float(err.max()), float(err.median()), float((lse.double() - ref_lse).abs().max())
    print(f'max {e_max:.2e}  median {e_med:.2e}  lse {e_lse:.2e}')
    assert torch.isfinite(out).all() and torch.isfinite(lse).all()
    assert e_max < 1e-4
    assert e_med < 5e-6
    assert e_lse < 1e-4


def _check(q, k, v, mask=None, kv=None, **plan):
    """Pack (unless the planes are given), run, compare the full tensor with fp64."""
    from graph_detr4d_amd import ops
    if kv is None:
        kv = ops.cross_mha_pack_kv(k, v)
    out, lse = ops.cross_mha_fwd(q, kv, H, key_padding_mask=mask, want_lse=True, **plan)
    _within(out, lse, *R.core(q, k, v, H, mask))
    return out, lse


@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('lq,lk,b', [(1, 1, 1), (17, 33, 2), (65, 95, 1), (64, 31, 2), (900, 1000, 1), (64, 12000, 1)])
def test_core_matches_fp64(lq, lk, b, masked):
    q, k, v = _inputs(lq, lk, b)
    _check(q, k, v, _random_mask(lk, b, lq + lk) if masked else None)


@pytest.mark.parametrize('plan', [dict(q_tile=32), dict(q_tile=32, splits=5), dict(splits=2), dict(splits=64)])
def test_every_tile_and_split_the_export_takes(plan):
    """The 32-query tile, forced splits, and more splits than the 3 key steps (empty splits contribute (m = -inf, l = 0, O = 0))."""
    q, k, v = _inputs(65, 95, 2, packed=False)
    _check(q, k, v, _random_mask(95, 2, 5), **plan)
    _check(q, k, v, None, **plan)


@pytest.fixture(scope='module')
def merge_case():
    """(65, 4096, 2): 2 query blocks x 8 key splits of 16 steps - 4 steps per wave - per (batch, head)."""
    from graph_detr4d_amd import ops
    lq, lk, b = 65, 4096, 2
    plan = ops.cross_mha_plan(lq, lk, b, H)
    assert plan.splits >= 3 and all((last - first) // 32 >= 8 for first, last in plan.ranges)
    return _inputs(lq, lk, b) + (plan,)


@pytest.mark.parametrize('which', ['first_split', 'last_split', 'one_survivor', 'one_wave'])
def test_masks_that_hit_the_merge_paths(merge_case, which):
    q, k, v, plan = merge_case
    lk, b = k.shape[0], k.shape[1]
    mask = torch.zeros(b, lk, dtype=torch.bool)
    if which == 'first_split':
        mask[0, plan.ranges[0][0]:plan.ranges[0][1]] = True
        mask[1, plan.ranges[1][0]:plan.ranges[1][1]] = True
    elif which == 'last_split':
        mask[:, plan.ranges[-1][0]:plan.ranges[-1][1]] = True
    elif which == 'one_survivor':                    # every key but one, the survivor in the last step (another one per batch)
        mask[:] = True
        mask[0, lk - 3] = False
        mask[1, lk - 32] = False
    else:                                            # wave 2's steps of split 1 (it takes every fourth step from the split's third)
        first, last = plan.ranges[1]
        for step in range(first // 32 + 2, last // 32, 4):
            mask[:, 32 * step:32 * step + 32] = True
        mask[1, plan.ranges[1][0]:plan.ranges[1][1]] = True          # batch 1: the whole split, every wave of it
    out, _ = _check(q, k, v, mask.to(DEV))
    if which == 'one_survivor':                      # the output is the survivor's value row: hi + lo holds it to 2^-16 relative
        assert float((out[:, 0] - v[lk - 3, 0]).abs().max()) <= 2.0 ** -16 * float(v[lk - 3, 0].abs().max())
        assert float((out[:, 1] - v[lk - 32, 1]).abs().max()) <= 2.0 ** -16 * float(v[lk - 32, 1].abs().max())


@pytest.mark.parametrize('where', ['first_step', 'last_step_of_last_split'])
def test_spiked_key_forces_the_rescale(merge_case, where):
    """One K row is a multiple of query 0's own row, per head, so that its score is 57 for that query: more than 50 above every
    other key's (asserted).  In the first step every later step must add to a state scaled by 2^-80; in the last step of the last
    split the running (m, l, O) of that wave and the merges must all be rescaled by it.

    The lse of query 0 is the spiked score itself.  With three bf16 products per score (hi + lo operands, ~2^-17 of the sum of the
    terms' magnitudes) it was off by 1.58e-4 on this input, above the 1e-4 bound, while the outputs were inside theirs; the kernel
    therefore takes its scores on six products (hi + mid + lo operands)."""
    q, k, v, plan = merge_case
    lk = k.shape[0]
    j = 5 if where == 'first_step' else lk - 7
    k = k.clone()
    q0 = q[0].view(-1, H, 32)                                                  # (B, H, 32)
    k[j] = (q0 * (57.0 * 32 ** 0.5 / (q0 * q0).sum(-1, keepdim=True))).view(-1, C)
    s = torch.einsum('qbhd,kbhd->bhqk', q.double().view(-1, q.shape[1], H, 32), k.double().view(lk, -1, H, 32)) / 32 ** 0.5
    others = torch.cat([s[:, :, 0, :j], s[:, :, 0, j + 1:]], dim=-1).max(-1).values
    assert float((s[:, :, 0, j] - others).min()) > 50
    from graph_detr4d_amd import ops
    kv = ops.cross_mha_pack_kv(k, v)
    for mask in (None, _random_mask(lk, k.shape[1], 11) & (torch.arange(lk, device=DEV) != j)):
        _check(q, k, v, mask, kv=kv)


def test_fully_masked_batch_is_nan_and_leaves_the_other_alone():
    from graph_detr4d_amd import ops
    q, k, v = _inputs(17, 33, 2)
    mask = torch.zeros(2, 33, dtype=torch.bool, device=DEV)
    mask[1] = True
    mask[0, 4:9] = True
    kv = ops.cross_mha_pack_kv(k, v)
    for plan in (dict(), dict(splits=2)):
        out, lse = ops.cross_mha_fwd(q, kv, H, key_padding_mask=mask, want_lse=True, **plan)
        assert torch.isnan(out[:, 1]).all() and bool((lse[:, 1] == float('-inf')).all())
        _within(out[:, :1], lse[:, :1], *R.core(q[:, :1], k[:, :1], v[:, :1], H, mask[:1]))           # batch 0
    out8 = ops.cross_mha_fwd(q, kv, H, key_padding_mask=mask.to(torch.uint8))      # uint8 masks are taken as they are
    assert torch.equal(torch.isnan(out8), torch.isnan(out)) and torch.equal(out8[:, 0], out[:, 0])


@pytest.mark.parametrize('lk', [33, 95])
def test_poisoned_planes_are_fully_rewritten(lk):
    """The pad keys of the last step must be written or never read: the storage starts as bf16 NaN."""
    from graph_detr4d_amd import ops
    q, k, v = _inputs(17, lk, 2)
    kv = ops.CrossKV(lk, 2, DEV)
    kv.k.view(torch.int16).fill_(0x7fc0)
    kv.v.view(torch.int16).fill_(0x7fc0)
    assert torch.isnan(kv.k.float()).all()
    assert ops.cross_mha_pack_kv(k, v, kv) is kv
    assert torch.isfinite(kv.k.float()).all() and torch.isfinite(kv.v.float()).all()
    for mask in (None, _random_mask(lk, 2, lk)):
        _check(q, k, v, mask, kv=kv)
    # hi + lo (K: hi + mid) reproduce the fp32 rows to 2^-16 relative, K's three pieces to 2^-22 (24 bits in three 8-bit pieces, one
    # fp32 rounding in this sum); the pad rows are zeros
    k3 = kv.k_rows()
    assert bool(((k3.float().sum(0)[:lk] - k).abs() <= 2.0 ** -22 * k.abs()).all()) and bool((k3[2, lk:] == 0).all())
    for rows, src, planes in ((k3, k, 3), (kv.v_rows(), v, 2)):
        assert tuple(rows.shape) == (planes, kv.steps * 32, 2, C)
        back = rows[0].float() + rows[1].float()
        assert bool((back[lk:] == 0).all())
        assert bool(((back[:lk] - src).abs() <= 2.0 ** -16 * src.abs()).all())
        assert bool((rows[0, :lk].float() == src.bfloat16().float()).all())       # hi is the value rounded to bf16


def test_equals_the_self_attention_core_at_batch_1():
    """The only way to compute this before: gd4d_mha_core_fwd on the fp32 rows with the mask expanded to (Lq, Lk).  Same arithmetic,
    another summation order: equal to the tolerance of that arithmetic, not bitwise."""
    from graph_detr4d_amd import ops
    lq, lk = 900, 1000
    q, k, v = _inputs(lq, lk, 1)
    mask = _random_mask(lk, 1, 77)
    kv = ops.cross_mha_pack_kv(k, v)
    out, lse = ops.cross_mha_fwd(q, kv, H, key_padding_mask=mask, want_lse=True)
    want, want_lse = ops.mha_core_fwd(q, k, v, H, mask.expand(lq, lk).contiguous(), want_lse=True)
    e, e_lse = float((out - want).abs().max()), float((lse - want_lse).abs().max())
    print(f'max {e:.2e} lse {e_lse:.2e}')
    assert e < 1e-4 and e_lse < 1e-4


def test_shape_and_type_errors():
    from graph_detr4d_amd import _lib, ops
    q, k, v = _inputs(17, 33, 2, packed=False)
    kv = ops.cross_mha_pack_kv(k, v)
    with pytest.raises(ValueError):
        ops.cross_mha_fwd(q[:, :1], kv, H)
    with pytest.raises(ValueError):
        ops.cross_mha_fwd(q, kv, H, key_padding_mask=torch.zeros(2, 34, dtype=torch.bool, device=DEV))
    with pytest.raises(ValueError):
        ops.cross_mha_fwd(q, kv, H, key_padding_mask=torch.zeros(2, 33, device=DEV))
    with pytest.raises(ValueError):
        ops.cross_mha_pack_kv(k, v[:32])
    with pytest.raises(_lib.Gd4dError):
        ops.cross_mha_fwd(q, kv, H, q_tile=48)
    with pytest.raises(TypeError):
        ops.cross_mha_fwd(q, (k, v), H)
