"""Detr4D_Distiller's / MixDistill's distillation terms on the device: the instance term (the student's predictions matched against
the teacher's) and the pyramid feature-distillation term.

Mirrors of
  * `DistillHungarianAssigner3D` (projects/mmdet3d_plugin/core/bbox/assigners/distill_hungarian_assigner_3d.py:16-134): same constructor
    keywords, `assign(bbox_pred, cls_pred, gt_bboxes, gt_labels)` returning an AssignResult, plus `assign_layers` for every decoder
    layer and sample at once;
  * `Detr4D_Distiller.get_instance_distill_loss` (distillation/distillers/detr4d_distiller.py:143-168) with the student head's
    `loss_distill_single` (dense_heads/detr3d_head_pe.py:851-925) and its targets (:927-1012): `get_instance_distill_loss(teacher_outs,
    student_outs, ...)` returns the reference's dictionary (`distill_loss_cls.{l}`, `distill_loss_reg.{l}`);
  * `MixDistill.get_feat_distill_loss` with its `lateral_convs` (distillation/distillers/mix_distill.py:51-55, 118-138):
    `FeatureDistillLoss` / `get_feat_distill_loss(teacher_feats, student_feats, lateral_convs, loss_feat_distill)` return the
    reference's dictionary (`feat_loss`).

The reference builds 6 x B cost matrices of Qs x Qt (900 x 900), copies each to the host for scipy and calls .item() once per layer.
Here: one launch for every cost block (gd4d_distill_match_cost_fwd), one for every assignment (gd4d_lsa_dense_fwd, exact, on the device),
one for both loss terms of every layer and their gradients (gd4d_distill_loss_fwd_bwd).  The normalisers follow from the query counts
(every student query is matched when Qs <= Qt, Qt of them otherwise): no .item(), at most one collective.  The whole term can be
captured in one graph.

The feature term in torch ops is four nn.Conv2d, a converted student pyramid as large as the student's own, mse_loss and autograd back
through all of it.  Here: per level ONE launch (gd4d_feat_distill_fwd) loads a pixel tile once, converts it on the split-bf16 MFMAs,
meets the teacher's tile in registers and writes the tile's loss partial and the student's gradient; the converted pyramid is never
written.  The weight and bias gradients are contracted from the one gradient map a level writes; the attention type's two maps come
from one pass over the teacher (gd4d_feat_distill_stats_fwd).  No host synchronisation, fixed summation orders (two runs: same bits).
"""
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import functional as Fn
from . import ops
from .criterion import AssignResult, HungarianAssigner3D, _LayerLossFunction, build_assigner, reduce_mean_normalisers
from .registry import BBOX_ASSIGNERS


def _stacked(x):
    return x if torch.is_tensor(x) else torch.stack(list(x))


@BBOX_ASSIGNERS.register_module()
class DistillHungarianAssigner3D(HungarianAssigner3D):
    """Matching of the student's predictions to the teacher's (pseudo ground truth).  Cost: DistillCrossEntropyLossCost (soft-label BCE,
    match_cost.py:30-91) + BBox3DL1Cost on the first 8 normalised box entries (match_cost.py:7-28); IoUCost is built by the reference
    but never used (any weight accepted).  Status words as HungarianAssigner3D's: check_status() / poll_status()."""

    def __init__(self, cls_cost=dict(type='ClassificationCost', weight=1.), reg_cost=dict(type='BBoxL1Cost', weight=1.0),
                 iou_cost=dict(type='IoUCost', weight=0.0), pc_range=None):
        cls_cost, reg_cost = cls_cost or {}, reg_cost or {}
        if cls_cost.get('type', 'DistillCrossEntropyLossCost') != 'DistillCrossEntropyLossCost' or \
                reg_cost.get('type', 'BBox3DL1Cost') != 'BBox3DL1Cost':
            raise NotImplementedError('gd4d_distill_match_cost_fwd implements the shipped distill configs\' costs: '
                                      'DistillCrossEntropyLossCost + BBox3DL1Cost (projects/distill_cfg/*)')
        if not cls_cost.get('use_sigmoid', True):
            raise NotImplementedError('DistillCrossEntropyLossCost(use_sigmoid=False) is not supported by the reference either')
        self.cls_weight = float(cls_cost.get('weight', 1.0))
        self.reg_weight = float(reg_cost.get('weight', 1.0))
        self.pc_range = pc_range

    @staticmethod
    def _raise_for(st, ncls):
        if bool((st == 1).any()):
            raise ValueError('matrix contains invalid numeric entries (a NaN or -inf distillation cost: scipy refuses it)')
        if bool((st == 2).any()):
            raise ops._lib.Gd4dError('gd4d_lsa_dense_fwd: cost matrix is infeasible')

    def _solve(self, cost, nl, b, qs, qt, host):
        dev = cost.device
        if not host:
            start = torch.arange(0, (b + 1) * qt, qt, dtype=torch.int32, device=dev)
            self.poll_status()
            assigned, status = ops.lsa_dense_fwd(cost, start, nl, b, qs, b * qt, qt)
            self._status = (status, None)
            return assigned
        c = cost.cpu().numpy()                                   # the reference's route: every block to the host ...
        if np.isnan(c).any():
            raise ValueError('matrix contains invalid numeric entries (a NaN or -inf distillation cost: scipy refuses it)')
        problems = [(qs * (l * b * qt + i * qt), qs, qt) for l in range(nl) for i in range(b)]
        matched = ops.linear_sum_assignment_batch(c, problems, num_threads=min(len(problems), 8))
        a = np.stack(matched).reshape(nl, b, qs)
        for i in range(b):
            a[:, i][a[:, i] >= 0] += i * qt
        return torch.from_numpy(a).to(dev)                       # ... and back

    def assign_layers(self, s_cls, s_box, t_cls, t_box, host=False):
        """Every decoder layer and sample at once.  s_cls (NL, B, Qs, C) / s_box (NL, B, Qs, code) the student's head outputs,
        t_cls (NL, B, Qt, C) / t_box (NL, B, Qt, 10) the teacher's (its sigmoid, batch-0 soft labels and denormalise -> normalise round
        trip are done in the cost kernel).  Returns assigned (NL, B, Qs) int32 on the device: b * Qt + teacher index, or -1.
        host=True: the cost blocks go to the host, gd4d_linear_sum_assignment_batch solves them, the matches come back (A/B route)."""
        nl, b, qs, _ = s_cls.shape
        qt = t_cls.shape[2]
        cost = ops.distill_match_cost_fwd(s_cls.detach().float().contiguous(), s_box.detach().float().contiguous(),
                                          t_cls.detach().float().contiguous(), t_box.detach().float().contiguous(),
                                          self.cls_weight, self.reg_weight)
        self.last_cost = cost
        return self._solve(cost, nl, b, qs, qt, host)

    def assign(self, bbox_pred, cls_pred, gt_bboxes, gt_labels, gt_bboxes_ignore=None, eps=1e-7, host=False):
        """The reference's per-problem entry point (:52-134): gt_bboxes (Qt, 9) denormalised teacher boxes, gt_labels (Qt, C) soft
        labels.  gt_inds: 0 = background, t + 1 = matched to teacher t; labels (Qs, C): the matched teacher's soft labels, -1 elsewhere."""
        assert gt_bboxes_ignore is None, 'Only case when gt_bboxes_ignore is None is supported.'
        num_gts, q = gt_bboxes.size(0), bbox_pred.size(0)
        gt_inds = bbox_pred.new_full((q,), -1, dtype=torch.long)
        lab = bbox_pred.new_full((q, cls_pred.size(1)), -1, dtype=torch.float)
        if num_gts == 0 or q == 0:
            if num_gts == 0:
                gt_inds[:] = 0
            return AssignResult(num_gts, gt_inds, None, labels=lab)
        cost = ops.distill_match_cost_fwd(cls_pred.detach().float().contiguous()[None, None],
                                          bbox_pred.detach().float().contiguous()[None, None],
                                          gt_labels.detach().float().contiguous()[None, None],
                                          gt_bboxes.detach().float()[:, :9].contiguous()[None, None],
                                          self.cls_weight, self.reg_weight, pseudo_gt=True)
        self.last_cost = cost
        a = self._solve(cost, 1, 1, q, num_gts, host)[0, 0].long()
        if not host:
            self.check_status()                                  # (the reference's entry point raises where it stands)
        gt_inds = a + 1
        pos = a >= 0
        lab[pos] = gt_labels[a[pos]].float()
        return AssignResult(num_gts, gt_inds, None, labels=lab)


def distill_normalisers(batch, num_student, num_teacher, bg_cls_weight=0.0, sync_cls_avg_factor=True, device=None):
    """(cls_avg_factor, num_total_pos) of loss_distill_single (:893-905) as a 2-element device tensor.  PseudoSampler's positives are
    the matched student queries: min(Qs, Qt) per sample.  reduce_mean over the ranks: ONE all-reduce of both (num_total_pos is always
    averaged, cls_avg_factor only with sync_cls_avg_factor), as Detr3DCriterion.normalisers."""
    num_pos = float(batch * min(num_student, num_teacher))
    num_neg = float(batch * num_student) - num_pos
    avg = torch.tensor([num_pos + num_neg * float(bg_cls_weight), num_pos], dtype=torch.float32, device=device)
    return reduce_mean_normalisers(avg, sync_cls_avg_factor)


def _loss_weight(cfg, kind, **required):
    if cfg is None:
        raise NotImplementedError(f'loss_distill_single calls both distillation losses: {kind} must be given')
    if cfg.get('type') != kind or any(cfg.get(k, v) != v for k, v in required.items()):
        raise NotImplementedError(f'gd4d_distill_loss_fwd_bwd implements the shipped distill configs\' losses: {kind} {required}')
    return float(cfg.get('loss_weight', 1.0))


def get_instance_distill_loss(teacher_outs, stu_outs, loss_cls_distill=None, loss_reg_distill=None, reweight_score=False,
                              pc_range=None, code_weights=None, sync_cls_avg_factor=True, bg_cls_weight=0.0, distill_assigner=None,
                              host=False, avg_factors=None):
    """Detr4D_Distiller.get_instance_distill_loss (detr4d_distiller.py:143-168).  teacher_outs / stu_outs: the heads' output dicts
    (`all_cls_scores` (NL, B, Q, C) logits, `all_bbox_preds` (NL, B, Q, 10) box codes; tensors or per-layer lists).  The teacher is
    detached.  loss_cls_distill: DistillCrossEntropyLoss(use_sigmoid=True) config, loss_reg_distill: L1Loss config (a loss_weight of 0.0
    is allowed; the term is still computed), reweight_score, and the student head's code_weights / sync_cls_avg_factor / bg_cls_weight.
    pc_range is accepted for the reference's signature (normalize_bbox / denormalize_bbox ignore it).  distill_assigner: a config dict
    or a DistillHungarianAssigner3D (default: the configs' - DistillCrossEntropyLossCost 1.0 + BBox3DL1Cost 0.25).  host=True: the
    assignment's host route (A/B comparison).  avg_factors: precomputed distill_normalisers (a captured step computes them outside).
    Returns {'distill_loss_cls.{l}', 'distill_loss_reg.{l}'} through one autograd Function."""
    wc = _loss_weight(loss_cls_distill, 'DistillCrossEntropyLoss', use_sigmoid=True)
    wr = _loss_weight(loss_reg_distill, 'L1Loss')
    t_cls = _stacked(teacher_outs['all_cls_scores']).detach().float().contiguous()
    t_box = _stacked(teacher_outs['all_bbox_preds']).detach().float().contiguous()
    s_cls = _stacked(stu_outs['all_cls_scores'])
    s_box = _stacked(stu_outs['all_bbox_preds'])
    nl, b, qs, _ = s_cls.shape
    qt = t_cls.shape[2]
    if t_box.shape[-1] != 10 or s_box.shape[-1] < 10:
        raise NotImplementedError('the distillation targets need 10-entry box codes (velocity included): the reference\'s '
                                  'bbox_targets has code_size - 1 = 9 columns (detr3d_head_pe.py:988)')
    asg = distill_assigner
    if asg is None:
        asg = dict(cls_cost=dict(type='DistillCrossEntropyLossCost', weight=1.0), reg_cost=dict(type='BBox3DL1Cost', weight=0.25),
                   iou_cost=dict(type='IoUCost', weight=0.0), pc_range=pc_range)
    asg = build_assigner(asg, DistillHungarianAssigner3D)
    assigned = asg.assign_layers(s_cls, s_box, t_cls, t_box, host=host)
    cw = code_weights if code_weights is not None else [1.0] * 8 + [0.2, 0.2]
    cw = cw.detach().float().to(s_cls.device) if torch.is_tensor(cw) else torch.tensor(cw, dtype=torch.float32, device=s_cls.device)
    avg = avg_factors if avg_factors is not None else distill_normalisers(b, qs, qt, bg_cls_weight, sync_cls_avg_factor, s_cls.device)
    loss = _LayerLossFunction.apply(ops.distill_loss_fwd_bwd, s_cls.float().contiguous(), s_box.float().contiguous(), t_cls, t_box,
                                    assigned, cw.contiguous(), avg, bool(reweight_score), wc, wr)            # (the teacher gets none)
    out = {}
    for l in range(nl):
        out[f'distill_loss_cls.{l}'] = loss[l, 0]
        out[f'distill_loss_reg.{l}'] = loss[l, 1]
    get_instance_distill_loss.last_assigned = assigned
    get_instance_distill_loss.last_assigner = asg
    return out


FEAT_DISTILL_TYPES = ('vanilla', 'attention')
FEAT_DISTILL_TEMPERATURE = 0.5                              # T of mix_distill.py:131


class _FeatDistillFunction(torch.autograd.Function):
    """feat_loss (scalar) of every level from gd4d_feat_distill_fwd; the gradients for the student's levels and the lateral convolutions'
    weights and biases come out of the same call, backward only scales them.  The teacher gets none."""

    @staticmethod
    def forward(ctx, kind, loss_weight, nl, *tensors):
        teacher, student = tensors[:nl], tensors[nl:2 * nl]
        weights, biases = tensors[2 * nl:3 * nl], tensors[3 * nl:4 * nl]
        t = [x.detach().reshape(-1, *x.shape[-3:]) for x in teacher]
        s = [x.detach().reshape(-1, *x.shape[-3:]) for x in student]
        w = torch.stack([x.detach().reshape(x.shape[0], x.shape[1]) for x in weights])
        b = torch.stack([x.detach() for x in biases])
        a_c = a_s = None
        if kind == 'attention':
            a_c, a_s = ops.feat_distill_stats_fwd(t, FEAT_DISTILL_TEMPERATURE)
        loss, gx, gw, gb = ops.feat_distill_fwd(s, t, w, b, loss_weight, a_c, a_s)
        ctx.nl = nl
        ctx.shapes = [x.shape for x in student]
        ctx.save_for_backward(gw, gb, *gx)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad_loss):
        nl = ctx.nl
        gw, gb, gx = ctx.saved_tensors[0], ctx.saved_tensors[1], ctx.saved_tensors[2:]
        g_s = tuple((x * grad_loss).view(shp) for x, shp in zip(gx, ctx.shapes))
        g_w = tuple((gw[l] * grad_loss).view(gw.shape[1], gw.shape[2], 1, 1) for l in range(nl))
        g_b = tuple(gb[l] * grad_loss for l in range(nl))
        return (None, None, None) + (None,) * nl + g_s + g_w + g_b


def _feat_distill_torch(teacher_feats, student_feats, lateral_convs, kind, loss_weight):
    """The reference's op sequence (mix_distill.py:118-138) in torch: the torch_ops route."""
    num_levels = len(teacher_feats)
    feat_loss = 0
    for level_id in range(num_levels):
        student_feat, teacher_feat = student_feats[level_id], teacher_feats[level_id]
        bs, num_cams, num_c, w, h = student_feat.shape
        student_feat = lateral_convs[level_id](student_feat.reshape(bs * num_cams, num_c, w, h))
        teacher_feat = teacher_feat.reshape(bs * num_cams, num_c, w, h)
        if kind == 'vanilla':
            feat_loss = feat_loss + F.mse_loss(student_feat, teacher_feat)
        else:
            T = FEAT_DISTILL_TEMPERATURE
            g_c = torch.mean(torch.abs(teacher_feat), dim=1, keepdim=True).reshape(bs * num_cams, 1, w * h)
            g_s = torch.mean(torch.abs(teacher_feat), dim=(2, 3), keepdim=True)
            a_c = num_c * F.softmax(g_c / T, dim=2).reshape(bs * num_cams, 1, w, h)
            a_s = w * h * F.softmax(g_s / T, dim=1)
            feat_loss = feat_loss + torch.mean(a_c * a_s * F.mse_loss(teacher_feat, student_feat, reduction='none'))
    return loss_weight * feat_loss / num_levels


def _feat_distill_type(loss_feat_distill):
    kind = loss_feat_distill.get('type', 'vanilla')
    if kind not in FEAT_DISTILL_TYPES:
        raise ValueError(f'loss_feat_distill type {kind!r}: the supported types are \'vanilla\' and \'attention\'')
    return kind


def get_feat_distill_loss(teacher_feats, student_feats, lateral_convs, loss_feat_distill, torch_ops=False, module=None):
    """MixDistill.get_feat_distill_loss (mix_distill.py:118-138).  teacher_feats / student_feats: the pyramids as the FPNs emit them,
    one (B, N, 256, H_l, W_l) fp32 tensor per level; lateral_convs: the nn.Conv2d(256, 256, 1) of each level (:51-55; level l uses
    lateral_convs[l], the levels given are the levels summed and divided by); loss_feat_distill: the reference's dict, `type` 'vanilla'
    (mse_loss) or 'attention' (both attention maps from the TEACHER, T = 0.5, :131-137) and `loss_weight`.
    Returns {'feat_loss': loss_weight * sum_l loss_l / num_levels} through one autograd Function: gradients for the student's levels and
    every convolution's weight and bias; the teacher gets none.
    Deviations from the reference, both errors instead of silence: a `type` other than the two raises ValueError (the reference adds
    nothing and returns 0); a teacher level that requires grad raises ValueError (the teacher is detached in the reference's step: it
    runs under no_grad, :92-95).  CPU tensors raise (no CPU fallback).  torch_ops=True (or GD4D_TORCH_OPS=1): the reference's op sequence
    in torch, an explicit choice (Fn.torch_ops_route)."""
    kind = _feat_distill_type(loss_feat_distill)
    loss_weight = float(loss_feat_distill['loss_weight'])
    teacher_feats, student_feats = list(teacher_feats), list(student_feats)
    nl = len(teacher_feats)
    if nl == 0 or len(student_feats) < nl or len(lateral_convs) < nl:
        raise ValueError(f'get_feat_distill_loss: {nl} teacher levels need as many student levels and lateral convolutions '
                         f'({len(student_feats)}, {len(lateral_convs)})')
    if any(t.requires_grad for t in teacher_feats):
        raise ValueError('get_feat_distill_loss: a teacher level requires grad; the teacher is detached in the reference\'s step '
                         '(MixDistill.forward_train runs it under torch.no_grad()): pass teacher_feats detached')
    student_feats = student_feats[:nl]
    for t, s in zip(teacher_feats, student_feats):
        if t.dim() != 5 or t.shape != s.shape:
            raise ValueError(f'get_feat_distill_loss: levels (B, N, C, H, W) of equal shapes expected, got {tuple(t.shape)} / {tuple(s.shape)}')
    convs = [lateral_convs[l] for l in range(nl)]
    ok = all(t.shape[2] == 256 and t.dtype == torch.float32 and s.dtype == torch.float32 for t, s in zip(teacher_feats, student_feats)) \
        and all(tuple(c.weight.shape) == (256, 256, 1, 1) and c.bias is not None for c in convs)
    holder = module if module is not None else types.SimpleNamespace(torch_ops=bool(torch_ops))
    if Fn.torch_ops_route('get_feat_distill_loss with channels other than 256, a lateral convolution other than Conv2d(256, 256, 1) with '
                          'bias, or levels that are not float32', ok, module=holder):
        return dict(feat_loss=_feat_distill_torch(teacher_feats, student_feats, convs, kind, loss_weight))
    tensors = [t.contiguous() for t in teacher_feats] + [s.contiguous() for s in student_feats] + \
        [c.weight for c in convs] + [c.bias for c in convs]
    return dict(feat_loss=_FeatDistillFunction.apply(kind, loss_weight, nl, *tensors))


class FeatureDistillLoss(nn.Module):
    """MixDistill's feature-distillation term with the parameters it owns (mix_distill.py:51-55, 118-138): `lateral_convs`, one
    nn.Conv2d(256, 256, 1) per FPN level - state-dict keys `lateral_convs.{i}.weight` / `.bias`, the reference's, so a MixDistill
    checkpoint's entries load with strict=True.  loss_feat_distill: the reference's dict verbatim (`type`: 'vanilla' or 'attention',
    `loss_weight`); any other type raises ValueError here (the reference would silently add nothing).
    forward(teacher_feats, student_feats) -> {'feat_loss': tensor}; see get_feat_distill_loss.  torch_ops=True selects the reference's
    op sequence in torch."""

    def __init__(self, loss_feat_distill, num_levels=4, torch_ops=False):
        super().__init__()
        self.loss_feat_distill = dict(loss_feat_distill)
        _feat_distill_type(self.loss_feat_distill)
        if 'loss_weight' not in self.loss_feat_distill:
            raise ValueError('loss_feat_distill needs a loss_weight (mix_distill.py:138 reads it)')
        self.torch_ops = bool(torch_ops)
        self.lateral_convs = nn.ModuleList(nn.Conv2d(256, 256, 1, 1, 0) for _ in range(num_levels))

    def forward(self, teacher_feats, student_feats):
        return get_feat_distill_loss(teacher_feats, student_feats, self.lateral_convs, self.loss_feat_distill, module=self)
