"""Detr4D_Distiller's instance term without a GPU: the reference fixtures against a plain-torch restatement (cost blocks, scipy's
assignment, loss terms, gradients by autograd), the C ABI's argument checks and the assigner's config surface."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from golden_io import Golden

CASES = ['detr4d_distill_b1_rw', 'detr4d_distill_b2', 'detr4d_distill_fewer_teacher', 'detr4d_distill_degenerate']


def normalize(b):
    """core/bbox/util.py:38-58 for 9-entry boxes."""
    return torch.cat([b[..., 0:2], b[..., 3:5].log(), b[..., 2:3], b[..., 5:6].log(), b[..., 6:7].sin(), b[..., 6:7].cos(),
                      b[..., 7:9]], -1)


def denormalize(n):
    """core/bbox/util.py:60-87 for 10-entry codes."""
    rot = torch.atan2(n[..., 6:7], n[..., 7:8])
    return torch.cat([n[..., 0:2], n[..., 4:5], n[..., 2:4].exp(), n[..., 5:6].exp(), rot, n[..., 8:10]], -1)


def restated_cost(s_cls, s_box, soft, t_den, cls_w=1.0, reg_w=0.25):
    pos = F.binary_cross_entropy_with_logits(s_cls, torch.ones_like(s_cls), reduction='none')
    neg = F.binary_cross_entropy_with_logits(s_cls, torch.zeros_like(s_cls), reduction='none')
    cls = pos @ soft.T + neg @ (1 - soft).T
    return cls * cls_w + torch.cdist(s_box[:, :8], normalize(t_den)[:, :8], p=1) * reg_w


def restated_term(m, t_cls, t_box, s_cls, s_box, assigned_fn):
    """get_instance_distill_loss + loss_distill_single in plain torch; assigned_fn(l, b, cost) -> col of each student row (-1)."""
    nl, b, qs, ncls = s_cls.shape
    cw = torch.tensor(m['code_weights'])
    out, costs, cols = [], [], []
    for l in range(nl):
        soft = t_cls[l, 0].sigmoid()                                         # batch 0 for every sample (detr4d_distiller.py:159)
        labels, tgt, bw = [], [], []
        for i in range(b):
            t_den = denormalize(t_box[l, i])
            c = restated_cost(s_cls[l, i].detach(), s_box[l, i].detach(), soft, t_den)
            costs.append(c)
            col = assigned_fn(l, i, c)
            cols.append(col)
            lab = torch.full((qs, ncls), 10.0)
            tg = torch.zeros(qs, 9)
            w = torch.zeros(qs, 10)
            pos = col >= 0
            lab[pos] = soft[col[pos]]
            tg[pos] = t_den[col[pos]]
            w[pos] = 1.0
            labels.append(lab), tgt.append(tg), bw.append(w)
        labels, tgt, bw = torch.cat(labels), torch.cat(tgt), torch.cat(bw)
        npos = float(sum(int((c >= 0).sum()) for c in cols[-b:]))
        x = s_cls[l].reshape(-1, ncls)
        lc = F.binary_cross_entropy_with_logits(x, labels, reduction='none').sum() / max(npos, 1) * m['loss_cls_weight']
        div = max(npos, 1)
        if m['reweight_score']:
            rs = labels.max(-1, keepdim=True)[0]
            bw = bw * rs
            div = rs[labels[:, 0] != 10].sum()
        tn = normalize(tgt)
        ok = torch.isfinite(tn).all(-1)
        bw = bw * cw
        p = s_box[l].reshape(-1, 10)
        lr = ((p[ok] - tn[ok]).abs() * bw[ok]).sum() / div * m['loss_reg_weight']
        out += [torch.nan_to_num(lc), torch.nan_to_num(lr)]
    return torch.stack(out), costs, cols


@pytest.mark.parametrize('name', CASES)
def test_fixture_agrees_with_a_plain_torch_restatement(name):
    from scipy.optimize import linear_sum_assignment
    g = Golden(name)
    m = g.meta
    s_cls, s_box = g.t('s_cls').requires_grad_(), g.t('s_box').requires_grad_()
    nl, b = m['num_layers'], m['batch']

    def scipy_cols(l, i, c):
        r, cc = linear_sum_assignment(c.numpy())
        col = torch.full((c.shape[0],), -1, dtype=torch.long)
        col[torch.from_numpy(r)] = torch.from_numpy(cc)
        return col
    losses, costs, cols = restated_term(m, g.t('t_cls'), g.t('t_box'), s_cls, s_box, scipy_cols)
    for k in range(nl * b):
        l, i = divmod(k, b)
        torch.testing.assert_close(costs[k], g.t(f'cost_l{l}_b{i}'), rtol=1e-5, atol=1e-5)
        assert torch.equal(cols[k] + 1, g.t(f'assigned_l{l}_b{i}').long())
    torch.testing.assert_close(losses, g.t('losses'), rtol=1e-5, atol=1e-6)
    losses.sum().backward()
    torch.testing.assert_close(s_cls.grad, g.t('grad_s_cls'), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(s_box.grad, g.t('grad_s_box'), rtol=1e-5, atol=1e-6)


def test_fixtures_cover_the_issue_cases():
    b2 = Golden('detr4d_distill_b2')
    assert b2.meta['batch'] == 2 and not b2.meta['reweight_score']
    # the soft labels of sample 1's matched rows are sample 0's teacher scores (the batch-0 quirk): the two differ
    assert not torch.allclose(b2.t('t_cls')[0, 0], b2.t('t_cls')[0, 1])
    assert Golden('detr4d_distill_b1_rw').meta['reweight_score']
    few = Golden('detr4d_distill_fewer_teacher').meta
    assert few['num_teacher'] < few['num_student']
    few_a = Golden('detr4d_distill_fewer_teacher').t('assigned_l0_b0')
    assert int((few_a == 0).sum()) == few['num_student'] - few['num_teacher']      # rows labelled 10.0
    deg = Golden('detr4d_distill_degenerate')
    assert torch.isinf(deg.t('cost_l0_b0')).any() and not torch.isnan(deg.t('cost_l0_b0')).any()
    assert torch.isinf(deg.t('t_box')[..., 2].exp()).any()


def test_entry_points_validate_before_any_gpu_work():
    from graph_detr4d_amd import _lib
    lib = _lib.load()
    EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -5
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 64)()
    ptr = ctypes.c_void_p(ctypes.addressof(buf))
    f = ctypes.c_float
    cost = lib.gd4d_distill_match_cost_fwd
    assert cost(null, ptr, ptr, ptr, ptr, 6, 1, 900, 900, 10, 10, 0, f(1.0), f(0.25), null) == EINVAL
    assert cost(ptr, ptr, ptr, ptr, null, 6, 1, 900, 900, 10, 10, 0, f(1.0), f(0.25), null) == EINVAL
    assert cost(ptr, ptr, ptr, ptr, ptr, 6, 1, 0, 900, 10, 10, 0, f(1.0), f(0.25), null) == EINVAL
    assert cost(ptr, ptr, ptr, ptr, ptr, 6, 1, 900, 900, 10, 7, 0, f(1.0), f(0.25), null) == EUNSUPPORTED      # code < 8
    assert cost(ptr, ptr, ptr, ptr, ptr, 6, 1, 900, 900, 65, 10, 0, f(1.0), f(0.25), null) == EUNSUPPORTED     # classes > 64
    ws = lib.gd4d_lsa_dense_workspace_bytes
    assert ws(6, 2, 900, 900) == 6 * 2 * 900 * 900 * 4 and ws(0, 2, 900, 900) == 0
    lsa = lib.gd4d_lsa_dense_fwd
    assert lsa(null, ptr, ptr, ptr, ptr, 1 << 40, 6, 1, 900, 900, 900, null) == EINVAL
    assert lsa(ptr, ptr, ptr, null, ptr, 1 << 40, 6, 1, 900, 900, 900, null) == EINVAL
    assert lsa(ptr, ptr, ptr, ptr, ptr, 16, 6, 1, 900, 900, 900, null) == EWORKSPACE
    assert lsa(ptr, ptr, ptr, ptr, null, 1 << 40, 6, 1, 900, 900, 900, null) == EWORKSPACE
    assert lsa(ptr, ptr, ptr, ptr, ptr, 1 << 40, 1, 1, 5000, 5000, 5000, null) == EUNSUPPORTED                # > 4096 columns
    loss = lib.gd4d_distill_loss_fwd_bwd
    args = [ptr] * 10 + [6, 1, 900, 900, 10, 10, 0, f(1.0), f(0.25), null]
    for k in range(10):
        a = list(args)
        a[k] = null
        assert loss(*a) == EINVAL
    a = list(args)
    a[12] = 0
    assert loss(*a) == EINVAL
    a = list(args)
    a[15] = 8
    assert loss(*a) == EUNSUPPORTED                                                                         # box code < 10


def test_exports_in_header_and_bindings(repo_root):
    from graph_detr4d_amd import _lib
    hdr = open(os.path.join(repo_root, 'include', 'gd4d.h')).read()
    for name in ('gd4d_distill_match_cost_fwd', 'gd4d_lsa_dense_workspace_bytes', 'gd4d_lsa_dense_fwd', 'gd4d_distill_loss_fwd_bwd'):
        assert name in _lib.SIGNATURES and re.search(rf'\b{name}\s*\(', hdr)


def test_ops_refuse_cpu_tensors():
    from graph_detr4d_amd import _lib, ops
    z = torch.zeros
    with pytest.raises(_lib.Gd4dError):
        ops.distill_match_cost_fwd(z(1, 1, 4, 10), z(1, 1, 4, 10), z(1, 1, 4, 10), z(1, 1, 4, 10))
    with pytest.raises(_lib.Gd4dError):
        ops.lsa_dense_fwd(z(16), torch.tensor([0, 4], dtype=torch.int32), 1, 1, 4, 4, 4)
    with pytest.raises(_lib.Gd4dError):
        ops.distill_loss_fwd_bwd(z(1, 1, 4, 10), z(1, 1, 4, 10), z(1, 1, 4, 10), z(1, 1, 4, 10), z(1, 1, 4, dtype=torch.int32),
                                 z(10), z(2))


DISTILL_CFG = dict(
    loss_reg_distill=dict(type='L1Loss', loss_weight=0.25),
    loss_cls_distill=dict(type='DistillCrossEntropyLoss', use_sigmoid=True, loss_weight=0.0),
    reweight_score=True,
    distill_assigner=dict(type='DistillHungarianAssigner3D', cls_cost=dict(type='DistillCrossEntropyLossCost', weight=1.0),
                          reg_cost=dict(type='BBox3DL1Cost', weight=0.25), iou_cost=dict(type='IoUCost', weight=0.0),
                          pc_range=[-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]))


def test_assigner_config_surface():
    from graph_detr4d_amd import BBOX_ASSIGNERS, DistillHungarianAssigner3D, build_assigner
    cfg = dict(DISTILL_CFG['distill_assigner'])
    a = build_assigner(cfg)
    assert isinstance(a, DistillHungarianAssigner3D) and BBOX_ASSIGNERS.get('DistillHungarianAssigner3D') is DistillHungarianAssigner3D
    assert a.cls_weight == 1.0 and a.reg_weight == 0.25 and a.pc_range == cfg['pc_range']
    with pytest.raises(NotImplementedError):
        DistillHungarianAssigner3D(cls_cost=dict(type='FocalLossCost', weight=2.0), reg_cost=dict(type='BBox3DL1Cost', weight=0.25))
    with pytest.raises(NotImplementedError):
        DistillHungarianAssigner3D(cls_cost=dict(type='DistillCrossEntropyLossCost'), reg_cost=dict(type='IoUCost'))
    with pytest.raises(NotImplementedError):
        DistillHungarianAssigner3D()                                          # the reference's defaults (ClassificationCost)


def test_loss_config_surface():
    from graph_detr4d_amd import get_instance_distill_loss
    z = torch.zeros(1, 1, 4, 10)
    outs = dict(all_cls_scores=z, all_bbox_preds=z)
    bad = dict(DISTILL_CFG, loss_cls_distill=dict(type='CrossEntropyLoss', loss_weight=1.0))
    with pytest.raises(NotImplementedError):
        get_instance_distill_loss(outs, outs, **bad)
    with pytest.raises(NotImplementedError):
        get_instance_distill_loss(outs, outs, **dict(DISTILL_CFG, loss_reg_distill=None))


def test_cpu_model_of_the_dense_solver_matches_scipy():
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import lsa_dense_model as M
    from scipy.optimize import linear_sum_assignment
    for fam, c in M.families(60, 3).items():
        col, _, _ = M.solve(c, 'dense')
        assert np.array_equal(col, linear_sum_assignment(c)[1]), fam
    c = np.random.default_rng(4).random((20, 50)).astype(np.float32)
    col, _, _ = M.solve(c, 'dense')
    assert np.array_equal(col, linear_sum_assignment(c)[1])
