"""Detr4D_Distiller's instance distillation term: the student's predictions matched against the teacher's, on the device.

Mirrors of
  * `DistillHungarianAssigner3D` (projects/mmdet3d_plugin/core/bbox/assigners/distill_hungarian_assigner_3d.py:16-134): same constructor
    keywords, `assign(bbox_pred, cls_pred, gt_bboxes, gt_labels)` returning an AssignResult, plus `assign_layers` for every decoder
    layer and sample at once;
  * `Detr4D_Distiller.get_instance_distill_loss` (distillation/distillers/detr4d_distiller.py:143-168) with the student head's
    `loss_distill_single` (dense_heads/detr3d_head_pe.py:851-925) and its targets (:927-1012): `get_instance_distill_loss(teacher_outs,
    student_outs, ...)` returns the reference's dictionary (`distill_loss_cls.{l}`, `distill_loss_reg.{l}`).

The reference builds 6 x B cost matrices of Qs x Qt (900 x 900), copies each to the host for scipy and calls .item() once per layer.
Here: one launch for every cost block (gd4d_distill_match_cost_fwd), one for every assignment (gd4d_lsa_dense_fwd, exact, on the device),
one for both loss terms of every layer and their gradients (gd4d_distill_loss_fwd_bwd).  The normalisers follow from the query counts
(every student query is matched when Qs <= Qt, Qt of them otherwise): no .item(), at most one collective.  The whole term can be
captured in one graph.
"""
import numpy as np
import torch
import torch.distributed as dist

from . import ops
from .criterion import AssignResult, HungarianAssigner3D
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


class _DistillLossFunction(torch.autograd.Function):
    """loss (NL, 2) from gd4d_distill_loss_fwd_bwd; the gradients come out of the same launch.  The teacher gets none."""

    @staticmethod
    def forward(ctx, s_cls, s_box, t_cls, t_box, assigned, code_weights, avg, reweight, wc, wr):
        loss, gcls, gbox = ops.distill_loss_fwd_bwd(s_cls, s_box, t_cls, t_box, assigned, code_weights, avg, reweight, wc, wr)
        ctx.save_for_backward(gcls, gbox)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        gcls, gbox = ctx.saved_tensors
        gl = grad_loss.view(-1, 2)
        return (gcls * gl[:, 0].view(-1, 1, 1, 1), gbox * gl[:, 1].view(-1, 1, 1, 1)) + (None,) * 8


def distill_normalisers(batch, num_student, num_teacher, bg_cls_weight=0.0, sync_cls_avg_factor=True, device=None):
    """(cls_avg_factor, num_total_pos) of loss_distill_single (:893-905) as a 2-element device tensor.  PseudoSampler's positives are
    the matched student queries: min(Qs, Qt) per sample.  reduce_mean over the ranks: ONE all-reduce of both (num_total_pos is always
    averaged, cls_avg_factor only with sync_cls_avg_factor), as Detr3DCriterion.normalisers."""
    num_pos = float(batch * min(num_student, num_teacher))
    num_neg = float(batch * num_student) - num_pos
    avg = torch.tensor([num_pos + num_neg * float(bg_cls_weight), num_pos], dtype=torch.float32, device=device)
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        local_cls = avg[0].clone()
        dist.all_reduce(avg)
        avg /= dist.get_world_size()
        if not sync_cls_avg_factor:
            avg[0] = local_cls
    return avg


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
    if isinstance(asg, dict):
        asg = dict(asg)
        asg.pop('type', None)
        asg = DistillHungarianAssigner3D(**asg)
    assigned = asg.assign_layers(s_cls, s_box, t_cls, t_box, host=host)
    cw = code_weights if code_weights is not None else [1.0] * 8 + [0.2, 0.2]
    cw = cw.detach().float().to(s_cls.device) if torch.is_tensor(cw) else torch.tensor(cw, dtype=torch.float32, device=s_cls.device)
    avg = avg_factors if avg_factors is not None else distill_normalisers(b, qs, qt, bg_cls_weight, sync_cls_avg_factor, s_cls.device)
    loss = _DistillLossFunction.apply(s_cls.float().contiguous(), s_box.float().contiguous(), t_cls, t_box, assigned, cw.contiguous(),
                                      avg, bool(reweight_score), wc, wr)
    out = {}
    for l in range(nl):
        out[f'distill_loss_cls.{l}'] = loss[l, 0]
        out[f'distill_loss_reg.{l}'] = loss[l, 1]
    get_instance_distill_loss.last_assigned = assigned
    get_instance_distill_loss.last_assigner = asg
    return out
