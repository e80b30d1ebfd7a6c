"""The fp64 restatements of loss_ref.py against the fixtures captured from the reference, before any kernel is judged by them, and the
closed forms they must meet exactly.  No GPU.

Bounds: the fixtures are fp32 results, so each comparison uses the bound of the fixture's own GPU test, named where it is used; this
file adds no number of its own.  The MixDistill fixtures distill_loss / distill_loss_b2_mean belong to another loss (no matching;
oracle.instance_distill_loss, test_distill_oracle.py) which none of the four restatements expresses; they stay with that test."""
import math

import pytest
import torch

import loss_cases as C
import loss_ref as R
from golden_io import Golden

HEAD = ['head_loss', 'head_loss_b2', 'head_loss_b2_both', 'head_loss_degenerate']
HDETR = ['head_loss_hdetr', 'head_loss_hdetr_b2', 'head_loss_hdetr_dense']
DISTILL = ['detr4d_distill_b1_rw', 'detr4d_distill_b2', 'detr4d_distill_fewer_teacher', 'detr4d_distill_degenerate']


def _packed(g, rep=1):
    """The fixture's per-sample ground truth (each repeated `rep` times, as H-DETR's one-to-many branch does) in the kernels' packed form."""
    m = g.meta
    boxes = [g.t(f'gt_boxes{i}').repeat(rep, 1) for i in range(m['batch'])]
    labels = [g.t(f'gt_labels{i}').repeat(rep) for i in range(m['batch'])]
    start = [0]
    for b in boxes:
        start.append(start[-1] + b.shape[0])
    return torch.cat(boxes), torch.cat(labels).to(torch.int32), start


def _assigned(g, start, q, prefix=''):
    """The fixture's gt_inds (0 background, j + 1) of every (layer, sample) as the solvers write them: start_b + j, or -1."""
    m = g.meta
    a = torch.full((m['num_layers'], m['batch'], q), -1, dtype=torch.int32)
    for l in range(m['num_layers']):
        for b in range(m['batch']):
            inds = g.t(f'{prefix}assigned_l{l}_b{b}').long()
            a[l, b] = torch.where(inds > 0, inds - 1 + start[b], torch.full_like(inds, -1)).to(torch.int32)
    return a


def _check_cost_blocks(g, packed, cls, box, start, q, prefix=''):
    """test_head_loss_gpu.test_cost_matrices_match_reference: the nan_to_num entries exactly, the others to rtol = atol = 2e-6 - met by
    the restatement run in float32, the fixture's own arithmetic, at every entry, and by the float64 one wherever the focal term is
    well-conditioned (class logit x <= 0: 1 - p keeps its bits).  For x > 0 the float64 value must explain the fixture through the
    rounding of p alone: the fixture lies in loss_cases.focal_interval, widened by that same bound."""
    m = g.meta
    gt, lab = packed
    sum_gt = start[-1]
    args = (cls, box, gt, lab, start, m['cls_cost_weight'], m['reg_cost_weight'], m['alpha'])
    cost, x = R.match_cost64(*args)
    cost32, _ = R.match_cost64(*args, dtype=torch.float32)
    for l in range(m['num_layers']):
        for b in range(m['batch']):
            n = start[b + 1] - start[b]
            if n == 0:
                continue
            off = q * (l * sum_gt + start[b])
            blk = lambda t: t[off:off + q * n].view(q, n)        # noqa: E731
            want = g.t(f'{prefix}cost_l{l}_b{b}')
            for got in (blk(cost), blk(cost32)):
                assert torch.equal(got == 100.0, want == 100.0)
            torch.testing.assert_close(blk(cost32), want, rtol=2e-6, atol=2e-6)
            plain = want != 100.0
            neg = plain & (blk(x) <= 0)
            torch.testing.assert_close(blk(cost)[neg].float(), want[neg], rtol=2e-6, atol=2e-6)
            pos = plain & (blk(x) > 0)
            lo, hi = C.focal_interval(blk(cost)[pos], blk(x)[pos], m['cls_cost_weight'], m['alpha'])
            wide = 2e-6 + 2e-6 * want[pos].double().abs()
            assert bool(((want[pos].double() >= lo - wide) & (want[pos].double() <= hi + wide)).all())


def _layer_losses(g):
    """(NL, 2) from the fixture's keyed losses: the last layer is loss_cls / loss_bbox, layer i is d{i}.* (detr3d_head_pe.py:1078-1092)."""
    nl = g.meta['num_layers']
    keys = [f'd{i}.' for i in range(nl - 1)] + ['']
    return torch.stack([torch.stack([g.t(f'loss.{k}loss_cls').reshape(()), g.t(f'loss.{k}loss_bbox').reshape(())]) for k in keys])


@pytest.mark.parametrize('name', HEAD)
def test_match_cost_and_head_loss_restatements_reproduce_the_head_loss_fixtures(name):
    g = Golden(name)
    m = g.meta
    cls, box = g.t('all_cls_scores'), g.t('all_bbox_preds')
    gt, lab, start = _packed(g)
    q = cls.shape[2]
    _check_cost_blocks(g, (gt, lab), cls, box, start, q)
    assigned = _assigned(g, start, q)
    npos = float((assigned >= 0).sum() / m['num_layers'])
    assert npos == float((assigned[0] >= 0).sum())                           # every layer matches min(G, Q) per sample
    loss, gc, gb = R.head_loss64(cls, box, assigned, gt, lab, torch.tensor(m['code_weights']), torch.tensor([npos, npos]), m['alpha'],
                                 m['loss_cls_weight'], m['loss_bbox_weight'])
    # test_head_loss_gpu.test_criterion_losses_and_gradients_match_reference's three bounds
    torch.testing.assert_close(loss.float(), _layer_losses(g), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(gc.float(), g.t('grad_cls'), rtol=1e-4, atol=1e-7)
    torch.testing.assert_close(gb.float(), g.t('grad_box'), rtol=1e-5, atol=1e-8)


@pytest.mark.parametrize('name', HDETR)
def test_restatements_reproduce_both_branches_of_the_hdetr_fixtures(name):
    """The one-to-many branch in the kernel's form: the UNREPEATED ground truth and `assigned` reduced modulo G_b (HDetr3DCriterion's
    two launches); the fixture's losses are one + lambda many, its one-to-many gradients carry lambda."""
    g = Golden(name)
    m = g.meta
    k, lam = m['k_one2many'], m['lambda_one2many']
    cw = torch.tensor(m['code_weights'])
    gt, lab, start = _packed(g)
    total, grads = 0, []
    for prefix, pre, rep in (('o2o_', '', 1), ('o2m_', '_one2many', k)):
        cls, box = g.t('all_cls_scores' + pre), g.t('all_bbox_preds' + pre)
        q = cls.shape[2]
        gt_r, lab_r, start_r = _packed(g, rep)
        _check_cost_blocks(g, (gt_r, lab_r), cls, box, start_r, q, prefix)
        rep_a = _assigned(g, start_r, q, prefix)                             # indices into the repeated ground truth
        a = rep_a.clone()
        for b in range(m['batch']):
            n = start[b + 1] - start[b]
            a[:, b] = torch.where(rep_a[:, b] >= 0, (rep_a[:, b] - start_r[b]) % max(n, 1) + start[b], -1)
        npos = float((a[0] >= 0).sum())
        loss, gc, gb = R.head_loss64(cls, box, a, gt, lab, cw, torch.tensor([npos, npos]), m['alpha'], m['loss_cls_weight'],
                                     m['loss_bbox_weight'])
        scale = 1.0 if rep == 1 else lam
        total = total + loss * scale
        grads += [gc * scale, gb * scale]
    # test_hdetr_loss_gpu.test_losses_gradients_and_assignments_match_reference's bounds
    torch.testing.assert_close(total.float(), _layer_losses(g), rtol=1e-5, atol=1e-6)
    for got, key in zip(grads, ('grad_cls', 'grad_box', 'grad_cls_one2many', 'grad_box_one2many')):
        torch.testing.assert_close(got.float(), g.t(key), rtol=1e-4, atol=1e-7)


@pytest.mark.parametrize('name', DISTILL)
def test_distill_restatements_reproduce_the_detr4d_distill_fixtures(name):
    g = Golden(name)
    m = g.meta
    nl, nb, qs, qt = m['num_layers'], m['batch'], m['num_student'], m['num_teacher']
    t_cls, t_box, s_cls, s_box = g.t('t_cls'), g.t('t_box'), g.t('s_cls'), g.t('s_box')
    cost = R.distill_match_cost64(s_cls, s_box, t_cls, t_box, m['cls_cost_weight'], m['reg_cost_weight'])
    # pseudo_gt: the assigner's own inputs give the same blocks
    soft = t_cls[:, :1].sigmoid().expand_as(t_cls).contiguous()
    pseudo = R.distill_match_cost64(s_cls, s_box, soft, R.denormalize9(t_box), m['cls_cost_weight'], m['reg_cost_weight'], pseudo_gt=True)
    assigned = torch.full((nl, nb, qs), -1, dtype=torch.int32)
    for l in range(nl):
        for b in range(nb):
            off = qs * (l * nb * qt + b * qt)
            want = g.t(f'cost_l{l}_b{b}')
            for got in (cost, pseudo):
                got = got[off:off + qs * qt].view(qs, qt).float()
                # test_detr4d_distill_gpu.test_cost_assignment_loss_and_gradients_match_reference: inf positions, then rtol = atol = 1e-5
                assert torch.equal(torch.isinf(got), torch.isinf(want))
                fin = torch.isfinite(want)
                torch.testing.assert_close(got[fin], want[fin], rtol=1e-5, atol=1e-5)
            inds = g.t(f'assigned_l{l}_b{b}').long()
            assigned[l, b] = torch.where(inds > 0, inds - 1 + b * qt, torch.full_like(inds, -1)).to(torch.int32)
    npos = float((assigned[0] >= 0).sum())
    loss, gc, gb = R.distill_loss64(s_cls, s_box, t_cls, t_box, assigned, torch.tensor(m['code_weights']), torch.tensor([npos, npos]),
                                    m['reweight_score'], m['loss_cls_weight'], m['loss_reg_weight'])
    # the same GPU test: losses rtol = atol = 1e-5, gradients 1e-4 of the largest entry
    torch.testing.assert_close(loss.reshape(-1).float(), g.t('losses'), rtol=1e-5, atol=1e-5)
    for got, ref in ((gc, g.t('grad_s_cls')), (gb, g.t('grad_s_box'))):
        torch.testing.assert_close(got.float(), ref, rtol=0, atol=1e-4 * float(ref.abs().max()))


# ------------------------------------------------------------------------------------------------------------------- closed forms
def _one_box(gt_dim=9):
    return torch.tensor([[1.0, 2.0, 3.0, 1.0, 1.0, 1.0, 0.0, 0.5, -0.25][:gt_dim]])     # log sizes 0, sin 0, cos 1: exact in fp64


def test_one_row_one_class_logit_zero_is_exact():
    """x = 0, p = 1/2.  Background: focal = log 2 (1 - alpha) / 4; matched to class 0: log 2 alpha / 4 and d/dx = alpha (-1/8 - log 2 / 4).
    Cost: (alpha - (1 - alpha)) / 4 (-log(1/2 + 1e-12)) w.  Distill: BCE(0, y) = log 2 for any y, d/dx = 1/2 - y."""
    z = torch.zeros(1, 1, 1, 1)
    box = torch.zeros(1, 1, 1, 10)
    gt, lab, cw, avg = _one_box(), torch.tensor([0], dtype=torch.int32), torch.ones(10), torch.tensor([1.0, 1.0])
    ln2, alpha = math.log(2.0), 0.25
    loss, gc, _ = R.head_loss64(z, box, torch.tensor([[[-1]]]), gt, lab, cw, avg, alpha, 2.0, 0.25)
    assert loss[0, 0].item() == 2.0 * (ln2 * (1 - alpha) * 0.25) and loss[0, 1].item() == 0.0
    assert gc.item() == pytest.approx(2.0 * (1 - alpha) * (0.125 + ln2 * 0.25), rel=1e-15)
    loss, gc, _ = R.head_loss64(z, box, torch.tensor([[[0]]]), gt, lab, cw, avg, alpha, 2.0, 0.25)
    assert loss[0, 0].item() == 2.0 * (ln2 * alpha * 0.25)
    assert gc.item() == pytest.approx(2.0 * alpha * (-0.125 - ln2 * 0.25), rel=1e-15)
    cost, x = R.match_cost64(z, box, gt, lab, [0, 1], 2.0, 0.0, alpha)
    assert cost.item() == pytest.approx((alpha - (1 - alpha)) * 0.25 * -math.log(0.5 + 1e-12) * 2.0, rel=1e-15) and x.item() == 0.0
    t_cls = torch.tensor([[[[1.25]]]])
    t_box = torch.zeros(1, 1, 1, 10)
    t_box[..., 7] = 1.0
    y = 1.0 / (1.0 + math.exp(-1.25))
    loss, gc, _ = R.distill_loss64(z, box, t_cls, t_box, torch.tensor([[[0]]]), cw, avg)
    assert loss[0, 0].item() == pytest.approx(ln2, rel=1e-15) and gc.item() == pytest.approx(0.5 - y, rel=1e-15)
    dc = R.distill_match_cost64(z, box, t_cls, t_box, 1.0, 0.0)
    assert dc.item() == pytest.approx(ln2, rel=1e-15)                         # pos = neg = log 2: log 2 (y + 1 - y)


@pytest.mark.parametrize('gt_dim, code', [(9, 10), (7, 8), (9, 16)])
def test_a_prediction_equal_to_its_target_has_zero_l1_and_zero_gradient(gt_dim, code):
    gt = _one_box(gt_dim)
    nk = 10 if gt_dim == 9 else 8
    box = torch.zeros(1, 1, 2, code)
    box[0, 0, 0, :nk] = R.normalize10(gt.double())[0, :nk].float()
    box[0, 0, 0, nk:] = 7.0                                                  # columns the loss never reads
    box[0, 0, 1] = 3.0                                                       # an unmatched row
    cls = torch.zeros(1, 1, 2, 3)
    a = torch.tensor([[[0, -1]]])
    loss, _, gb = R.head_loss64(cls, box, a, gt, torch.tensor([1], dtype=torch.int32), torch.ones(10), torch.tensor([1.0, 1.0]))
    assert loss[0, 1].item() == 0.0 and torch.count_nonzero(gb).item() == 0
    cost, _ = R.match_cost64(cls, box, gt, torch.tensor([1], dtype=torch.int32), [0, 1], 0.0, 1.0)
    assert cost[0].item() == 0.0 and cost[1].item() > 0.0
    if code >= 10 and gt_dim == 9:
        t_box = torch.zeros(1, 1, 1, 10)
        t_box[0, 0, 0] = torch.tensor([1.0, 2.0, 0.0, 0.0, 3.0, 0.0, 0.0, 1.0, 0.5, -0.25])
        s_box = torch.zeros(1, 1, 2, code)
        s_box[0, 0, 0, :10] = t_box[0, 0, 0]                                 # exp(0) = 1, log 1 = 0, atan2(0, 1) = 0: the round trip is exact
        for rw in (False, True):
            loss, _, gb = R.distill_loss64(cls, s_box, torch.zeros(1, 1, 1, 3), t_box, a, torch.ones(10), torch.tensor([1.0, 1.0]), rw)
            assert loss[0, 1].item() == 0.0 and torch.count_nonzero(gb).item() == 0
        dc = R.distill_match_cost64(cls, s_box, torch.zeros(1, 1, 1, 3), t_box, 0.0, 1.0)
        assert dc[0].item() == 0.0 and dc[1].item() == 1.0 + 2.0 + 3.0 + 1.0  # the zero row: |cx| + |cy| + |cz| + |cos|


def test_an_all_background_layer():
    """No matched row: the focal loss is the background sum, the box term 0 with a zero gradient; the distill labels are C everywhere,
    and under reweight_score the divisor is rows * C when C != 10 but 0 when C == 10: loss 0 after nan_to_num either way."""
    g = torch.Generator().manual_seed(5)
    for c in (10, 12):
        cls, box = torch.randn(2, 2, 5, c, generator=g), torch.randn(2, 2, 5, 10, generator=g)
        a = torch.full((2, 2, 5), -1)
        a[1, 0, 2] = 0                                                       # the other layer has one match
        gt, lab = _one_box(), torch.tensor([3], dtype=torch.int32)
        loss, gc, gb = R.head_loss64(cls, box, a, gt, lab, torch.ones(10), torch.tensor([0.0, 0.0]))
        x = cls[0].double().reshape(-1, c)
        p = x.sigmoid()
        want = 2.0 * (0.75 * p * p * (x.clamp(min=0) + torch.log1p(torch.exp(-x.abs())))).sum()
        assert loss[0, 0].item() == pytest.approx(want.item(), rel=1e-14) and loss[0, 1].item() == 0.0
        assert torch.count_nonzero(gb[0]).item() == 0 and torch.count_nonzero(gb[1]).item() == 10
        t_cls, t_box = torch.randn(2, 2, 4, c, generator=g), torch.randn(2, 2, 4, 10, generator=g)
        a = torch.full((2, 2, 5), -1)
        a[1, 1, 0] = 4 + 1                                                   # sample 1's teacher row 1
        for rw in (False, True):
            info = {}
            loss, gc, gb = R.distill_loss64(cls, box, t_cls, t_box, a, torch.ones(10), torch.tensor([0.0, 0.0]), rw, info=info)
            want = (x.clamp(min=0) - x * c + torch.log1p(torch.exp(-x.abs()))).sum()
            assert loss[0, 0].item() == pytest.approx(want.item(), rel=1e-14) and loss[0, 1].item() == 0.0
            assert torch.equal(gc[0].reshape(-1, c), p - c)
            assert torch.count_nonzero(gb[0]).item() == 0                    # torch: the isfinite filter drops every row before the division
            if rw:
                assert info['div'][0] == (0.0 if c == 10 else 10 * c)
                assert info['div'][1] == pytest.approx(float(t_cls[1, 0, 1].double().sigmoid().max()) + (0 if c == 10 else 9 * c), rel=1e-15)
