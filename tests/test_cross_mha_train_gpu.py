"""gd4d_cross_mha_train_fwd / gd4d_cross_mha_bwd / gd4d_cross_mha_pack_kv_train (training PETR's global cross-attention core) against
torch autograd in float64 on the device: tests/petr_ref.py::core's arithmetic with the keep mask of ops.mha_dropout_keep_mask
multiplied in (the restatement below equals petr_ref.core without dropout - asserted).

Bounds are the project's own for split-bf16 arithmetic with fp32 accumulation:
  out, lse        tests/test_cross_mha_gpu.py: max < 1e-4, median < 5e-6, lse < 1e-4
  dq, dk, dv      max < 1e-4 max(1, sqrt(Lq) / 10): the rule of test_dense_gpu.py::test_mha_core_bwd_matches_fp64
  with dropout    out < 4e-5, gradients < 2e-4: test_mha_core_dropout_*'s bounds at these sizes
Every case prints its figures before it asserts.  Data is randn; every batch row of every mask keeps at least one key."""
import math
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
    qq = torch.randn(lq, b, 2 * C, generator=g).to(DEV)
    kvp = torch.randn(lk, b, 2 * C, generator=g).to(DEV)
    dout = torch.randn(lq, b, C, generator=g).to(DEV)
    if packed:                                   # last-dim slices of wider buffers, as a module hands them over
        return qq[..., C:], kvp[..., :C], kvp[..., C:], dout
    return qq[..., C:].contiguous(), kvp[..., :C].contiguous(), kvp[..., C:].contiguous(), dout


def _random_mask(lk, b, seed, p=0.3):
    g = torch.Generator().manual_seed(seed)
    m = torch.rand(b, lk, generator=g) < p       # differs per batch
    m[:, int(torch.randint(0, lk, (1,), generator=g))] = False      # every batch row keeps a key
    return m.to(DEV)


def _reference(q, k, v, dout, mask=None, keep=None, p=0.):
    """out, lse, dq, dk, dv in float64; keep (B, H, Lq, Lk) bool."""
    q, k, v = (t.detach().double().clone().requires_grad_(True) for t in (q, k, v))
    lq, b, c = q.shape
    lk = k.shape[0]
    heads = lambda t, n: t.reshape(n, b, H, 32).permute(1, 2, 0, 3)      # noqa: E731
    s = heads(q, lq) @ heads(k, lk).transpose(-1, -2) / math.sqrt(32)
    if mask is not None:
        s = s.masked_fill(mask.bool()[:, None, None, :], float('-inf'))
    lse = torch.logsumexp(s, dim=-1).permute(2, 0, 1)
    pr = torch.softmax(s, dim=-1)
    if keep is not None:
        pr = pr * keep.double() / (1.0 - p)
    out = (pr @ heads(v, lk)).permute(2, 0, 1, 3).reshape(lq, b, c)
    out.backward(dout.double())
    return out.detach(), lse.detach(), q.grad, k.grad, v.grad


def _run(q, k, v, dout, mask=None, dropout_p=0., seed=None, packed=False, fwd_plan=None, bwd_plan=None):
    from graph_detr4d_amd import ops
    kv = ops.cross_mha_pack_kv(k, v, train=True)
    out, lse = ops.cross_mha_fwd(q, kv, H, key_padding_mask=mask, want_lse=True, dropout_p=dropout_p, seed=seed, **(fwd_plan or {}))
    res = ops.cross_mha_bwd(dout, q, out, lse, kv, H, key_padding_mask=mask, dropout_p=dropout_p, seed=seed, packed_kv=packed,
                            **(bwd_plan or {}))
    if packed:
        dq, dkv = res
        assert tuple(dkv.shape) == (k.shape[0], k.shape[1], 2 * C)
        return out, lse, dq, dkv[..., :C], dkv[..., C:]
    return (out, lse) + tuple(res)


def _grad_bound(lq):
    return 1e-4 * max(1.0, math.sqrt(lq) / 10)


def _compare(got, ref, lq, mask, out_bounds=(1e-4, 5e-6, 1e-4), grad_bound=None):
    out, lse, dq, dk, dv = got
    r_out, r_lse, r_dq, r_dk, r_dv = ref
    err = (out.double() - r_out).abs()
    e_max, e_med, e_lse = float(err.max()), float(err.median()), float((lse.double() - r_lse).abs().max())
    e_dq, e_dk, e_dv = (float((a.double() - r).abs().max()) for a, r in ((dq, r_dq), (dk, r_dk), (dv, r_dv)))
    bound = _grad_bound(lq) if grad_bound is None else grad_bound
    print(f'out max {e_max:.2e} median {e_med:.2e} lse {e_lse:.2e} | dq {e_dq:.2e} dk {e_dk:.2e} dv {e_dv:.2e} (bound {bound:.2e}) | '
          f'scale dq {float(r_dq.abs().max()):.2e} dk {float(r_dk.abs().max()):.2e} dv {float(r_dv.abs().max()):.2e}')
    for t in got:
        assert torch.isfinite(t).all()
    assert e_max < out_bounds[0]
    if out_bounds[1] is not None:
        assert e_med < out_bounds[1]
    assert e_lse < out_bounds[2]
    assert e_dq < bound and e_dk < bound and e_dv < bound
    if mask is not None:                         # rows of masked keys: exact zeros
        gone = mask.t()                          # (Lk, B)
        assert bool((dk[gone] == 0).all()) and bool((dv[gone] == 0).all())
    return e_dq, e_dk, e_dv


@pytest.mark.parametrize('packed', [True, False])
@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('lq,lk,b', [(1, 1, 1), (17, 33, 2), (65, 95, 1), (64, 31, 2), (70, 120, 2), (200, 4096, 2)])
def test_backward_matches_fp64(lq, lk, b, masked, packed):
    q, k, v, dout = _inputs(lq, lk, b, packed=packed)
    mask = _random_mask(lk, b, lq + lk) if masked else None
    ref = _reference(q, k, v, dout, mask)
    want_out, want_lse = R.core(q, k, v, H, mask)                   # the restatement above is petr_ref.core
    assert float((ref[0] - want_out).abs().max()) < 1e-12 and float((ref[1] - want_lse).abs().max()) < 1e-12
    _compare(_run(q, k, v, dout, mask, packed=packed), ref, lq, mask)


@pytest.mark.parametrize('p', [0.1, 0.3])
@pytest.mark.parametrize('lq,lk,b', [(65, 95, 2), (70, 120, 2)])
def test_dropout_matches_fp64_with_the_rebuilt_mask(lq, lk, b, p):
    from graph_detr4d_amd import ops
    q, k, v, dout = _inputs(lq, lk, b)
    mask = _random_mask(lk, b, lq + lk)
    torch.manual_seed(7)
    seed, seed2 = ops.mha_dropout_seed(DEV), ops.mha_dropout_seed(DEV)
    keep = ops.mha_dropout_keep_mask(seed, b, H, lq, lk, p)
    n = keep.numel()
    frac, sigma = float(keep.double().mean()), math.sqrt(p * (1 - p) / n)
    print(f'kept {frac:.5f} of {n}, expected {1 - p} +- {sigma:.1e}')
    assert abs(frac - (1 - p)) < 4 * sigma
    got = _run(q, k, v, dout, mask, dropout_p=p, seed=seed)
    # lse is the full softmax's; the out median bound belongs to the no-dropout cases
    _compare(got, _reference(q, k, v, dout, mask, keep, p), lq, mask, out_bounds=(4e-5, None, 1e-4), grad_bound=2e-4)
    again = _run(q, k, v, dout, mask, dropout_p=p, seed=seed.clone())
    assert all(torch.equal(a, c) for a, c in zip(got, again))       # the same seed: the same bits, forward and backward
    other = _run(q, k, v, dout, mask, dropout_p=p, seed=seed2)
    assert not torch.equal(ops.mha_dropout_keep_mask(seed2, b, H, lq, lk, p), keep)
    assert torch.equal(other[1], got[1]) and not torch.equal(other[0], got[0]) and not torch.equal(other[4], got[4])
    _compare(other, _reference(q, k, v, dout, mask, ops.mha_dropout_keep_mask(seed2, b, H, lq, lk, p), p), lq, mask,
             out_bounds=(4e-5, None, 1e-4), grad_bound=2e-4)


@pytest.mark.parametrize('plan', [dict(q_tile=32), dict(splits=2), dict(splits=5), dict(q_tile=32, splits=64)])
def test_every_plan_the_export_takes(plan):
    """The 32-query tile, forced splits, and more splits than the 3 key steps (empty splits add zeros) - forward and backward."""
    q, k, v, dout = _inputs(65, 95, 2, packed=False)
    for mask in (_random_mask(95, 2, 5), None):
        ref = _reference(q, k, v, dout, mask)
        _compare(_run(q, k, v, dout, mask, fwd_plan=plan, bwd_plan=plan), ref, 65, mask)
    from graph_detr4d_amd import ops
    mask, seed = _random_mask(95, 2, 5), torch.tensor([12345678901], device=DEV)
    keep = ops.mha_dropout_keep_mask(seed, 2, H, 65, 95, 0.1)
    _compare(_run(q, k, v, dout, mask, dropout_p=0.1, seed=seed, fwd_plan=plan, bwd_plan=plan),
             _reference(q, k, v, dout, mask, keep, 0.1), 65, mask, out_bounds=(4e-5, None, 1e-4), grad_bound=2e-4)


@pytest.fixture(scope='module')
def merge_case():
    """(65, 4096, 2): 3 query blocks x several key splits per (batch, head), 64 key blocks."""
    from graph_detr4d_amd import ops
    lq, lk, b = 65, 4096, 2
    plan = ops.cross_mha_bwd_plan(lq, lk, b, H)
    print(plan)
    assert plan.splits >= 3 and all((last - first) // 32 >= 8 for first, last in plan.ranges)
    return _inputs(lq, lk, b) + (plan,)


@pytest.mark.parametrize('which', ['first_split', 'last_split', 'one_survivor', 'one_wave'])
def test_masks_that_hit_the_merge_paths(merge_case, which):
    q, k, v, dout, plan = merge_case
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
    mask = mask.to(DEV)
    got = _run(q, k, v, dout, mask)
    _compare(got, _reference(q, k, v, dout, mask), q.shape[0], mask)
    if which == 'one_survivor':                      # P = 1 for the survivor: dv of its row is the column sum of dout
        want = dout.double().sum(0)
        assert float((got[4][lk - 3, 0].double() - want[0]).abs().max()) < 1e-4


@pytest.mark.parametrize('where', ['first_step', 'last_step_of_last_split'])
def test_spiked_key_gradients(merge_case, where):
    """The construction of test_cross_mha_gpu.py::test_spiked_key_forces_the_rescale: one key scores 57 for query 0, more than 50
    above every other (asserted), so that row's lse is the spiked score itself and P = exp(score - lse) is only right if the
    recompute reproduces the forward's six-product score."""
    q, k, v, dout, plan = merge_case
    lk = k.shape[0]
    j = 5 if where == 'first_step' else lk - 7
    k = k.clone()
    q0 = q[0].reshape(-1, H, 32)
    k[j] = (q0 * (57.0 * 32 ** 0.5 / (q0 * q0).sum(-1, keepdim=True))).reshape(-1, C)
    s = torch.einsum('qbhd,kbhd->bhqk', q.double().reshape(-1, q.shape[1], H, 32), k.double().reshape(lk, -1, H, 32)) / 32 ** 0.5
    others = torch.cat([s[:, :, 0, :j], s[:, :, 0, j + 1:]], dim=-1).max(-1).values
    assert float((s[:, :, 0, j] - others).min()) > 50
    for mask in (None, _random_mask(lk, k.shape[1], 11) & (torch.arange(lk, device=DEV) != j)):
        _compare(_run(q, k, v, dout, mask), _reference(q, k, v, dout, mask), q.shape[0], mask)


def test_two_backward_calls_are_bit_identical():
    from graph_detr4d_amd import ops
    q, k, v, dout = _inputs(200, 4096, 2)
    mask = _random_mask(4096, 2, 3)
    seed = torch.tensor([-987654321012], device=DEV)
    for p in (0., 0.1):
        a = _run(q, k, v, dout, mask, dropout_p=p, seed=seed if p else None)
        c = _run(q, k, v, dout, mask, dropout_p=p, seed=seed if p else None)
        assert all(torch.equal(x, y) for x, y in zip(a, c))
    assert ops.cross_mha_bwd_plan(200, 4096, 2).splits > 1           # (the split merge was part of it)


def _rows_of(planes, columns):
    """(3, steps, B, H, 2, 64, 8) planes -> (3, steps * 32, B, C) plain rows: CrossKV.k_rows' view (row fragments) or v_rows' (columns)."""
    n, b, h, s = planes.shape[0], planes.shape[1], planes.shape[2], planes.shape[3]
    if columns:
        return planes.view(n, b, h, s, 2, 4, 16, 2, 4).permute(0, 3, 7, 5, 8, 1, 2, 4, 6).reshape(n, s * 32, b, h * 32)
    return planes.view(n, b, h, s, 2, 4, 16, 8).permute(0, 3, 4, 6, 1, 2, 5, 7).reshape(n, s * 32, b, h * 32)


@pytest.mark.parametrize('lq,lk', [(17, 33), (70, 95)])
@pytest.mark.parametrize('p', [0., 0.1])
def test_poisoned_planes_and_workspace_are_fully_rewritten(lq, lk, p):
    """The pad rows of the last key step and of the last query step must be written or never read: all four plane groups and the
    backward's workspace (twelve query planes, Dq, lse, dq partials of forced splits) start as NaN bit patterns.  0 x NaN would reach
    dq, dk and dv otherwise."""
    from graph_detr4d_amd import ops
    b = 2
    q, k, v, dout = _inputs(lq, lk, b)
    kv = ops.CrossKV(lk, b, DEV, train=True)
    for t in (kv.k, kv.v, kv.vk, kv.kv):
        t.view(torch.int16).fill_(0x7fc0)
        assert torch.isnan(t.float()).all()
    assert ops.cross_mha_pack_kv(k, v, kv, train=True) is kv
    for planes, src, columns in ((kv.k, k, False), (kv.v, v, True), (kv.vk, v, False), (kv.kv, k, True)):
        rows = _rows_of(planes, columns).float()
        assert torch.isfinite(rows).all() and bool((rows[:, lk:] == 0).all())          # pad keys: zeros in every piece
        assert bool(((rows.sum(0)[:lk] - src).abs() <= 2.0 ** -22 * src.abs()).all())    # hi + mid + lo hold the fp32 rows
    mask = _random_mask(lk, b, lk)
    seed = torch.tensor([2468013579], device=DEV) if p else None
    keep = ops.mha_dropout_keep_mask(seed, b, H, lq, lk, p) if p else None
    ref = _reference(q, k, v, dout, mask, keep, p)
    out, lse = ops.cross_mha_fwd(q, kv, H, key_padding_mask=mask, want_lse=True, dropout_p=p, seed=seed)
    for plan in (dict(), dict(splits=2)):
        need = ops.cross_mha_bwd_plan(lq, lk, b, H, **plan).workspace_bytes
        ws = torch.full((need // 4 + 64,), float('nan'), device=DEV)
        dq, dk, dv = ops.cross_mha_bwd(dout, q, out, lse, kv, H, key_padding_mask=mask, dropout_p=p, seed=seed, workspace=ws, **plan)
        _compare((out, lse, dq, dk, dv), ref, lq, mask, out_bounds=(4e-5 if p else 1e-4, None, 1e-4), grad_bound=2e-4 if p else None)
        assert torch.isnan(ws[need // 4:]).all()                                          # nothing written past what the plan asks for
    with pytest.raises(ValueError):
        ops.cross_mha_bwd(dout, q, out, lse, kv, H, workspace=ws[:8])


def test_yardstick_the_self_attention_backward_at_batch_1():
    """Information for docs/measurements_r37.md: both kernels' errors against fp64 at (200, 4096), B = 1, no dropout.  The parent's
    only kernel way was ops.mha_core_fwd / mha_core_bwd with the mask expanded to (Lq, Lk).  Each is held to the bound of its own test."""
    from graph_detr4d_amd import ops
    lq, lk = 200, 4096
    q, k, v, dout = _inputs(lq, lk, 1, packed=False)
    mask = _random_mask(lk, 1, 77)
    ref = _reference(q, k, v, dout, mask)
    new = _compare(_run(q, k, v, dout, mask), ref, lq, mask)
    full = mask.expand(lq, lk).contiguous()
    out, lse = ops.mha_core_fwd(q, k, v, H, full, want_lse=True)
    old = [float((g.double() - r).abs().max()) for g, r in zip(ops.mha_core_bwd(q, k, v, out, dout, lse, H, full), ref[2:])]
    print('            dq        dk        dv')
    print('cross_mha   ' + '  '.join(f'{e:.2e}' for e in new))
    print('mha_core    ' + '  '.join(f'{e:.2e}' for e in old))
    assert max(old) < _grad_bound(lq)


def test_shape_and_type_errors():
    from graph_detr4d_amd import _lib, ops
    q, k, v, dout = _inputs(17, 33, 2, packed=False)
    kv = ops.cross_mha_pack_kv(k, v, train=True)
    out, lse = ops.cross_mha_fwd(q, kv, H, want_lse=True)
    with pytest.raises(TypeError):                                   # the inference planes do not hold what the backward reads
        ops.cross_mha_bwd(dout, q, out, lse, ops.cross_mha_pack_kv(k, v), H)
    with pytest.raises(ValueError):
        ops.cross_mha_bwd(dout[:5], q, out, lse, kv, H)
    with pytest.raises(ValueError):                                  # dropout without a seed
        ops.cross_mha_fwd(q, kv, H, dropout_p=0.1)
    with pytest.raises(_lib.Gd4dError):                              # the backward's workgroup owns 32 queries
        ops.cross_mha_bwd(dout, q, out, lse, kv, H, q_tile=64)
    with pytest.raises(_lib.Gd4dError):
        ops.cross_mha_fwd(q, kv, H, dropout_p=1.0, seed=torch.zeros(1, dtype=torch.int64, device=DEV))
