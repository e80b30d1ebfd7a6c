"""Plain-torch restatements of the four loss-side kernels in the kernels' own layouts, on the CPU, in float64 (or float32: the reference's
own arithmetic, whose distance from float64 is the yardstick of test_loss_kernels_gpu.py).  Not a test module.

  match_cost64          gd4d_match_cost_fwd          HungarianAssigner3D's cost (core/bbox/assigners/hungarian_assigner_3d.py:117-130)
  head_loss64           gd4d_head_loss_fwd_bwd       Detr3DHeadPE.loss_single (dense_heads/detr3d_head_pe.py:782-849, targets :704-729)
  distill_match_cost64  gd4d_distill_match_cost_fwd  DistillHungarianAssigner3D's cost (distill_hungarian_assigner_3d.py:106-114)
  distill_loss64        gd4d_distill_loss_fwd_bwd    Detr3DHeadPE.loss_distill_single (detr3d_head_pe.py:851-925, targets :952-1011)

Gradients come from autograd of the restated loss.  `before_nan_to_num=True` differentiates the two terms as they are before
torch.nan_to_num (:847-848, :923-924) replaces them - the kernels' documented deviation; the default goes through it, as the reference does.

Where the reference has no behaviour (it raises, or its shapes disagree) the kernels' own rule is restated and marked KERNEL RULE."""
import math

import torch
import torch.nn.functional as F

from oracle import torch_oracle as O

F64 = torch.float64
FLT_MAX = 3.4028234663852886e38


def _c(t, dtype):
    return t.detach().cpu().to(dtype)


def nan_to_num32(x):
    """torch.nan_to_num of an fp32 tensor (detr3d_head_pe.py:847-848): nan -> 0, +/-inf -> +/-FLT_MAX, whatever dtype x has here."""
    return torch.nan_to_num(x, nan=0.0, posinf=FLT_MAX, neginf=-FLT_MAX)


def normalize10(b):
    """core/bbox/util.py:38-58 through oracle.normalize_bbox.  KERNEL RULE for 8-entry boxes: the reference's cat gives 9 columns (vy = an
    empty slice), which fits no prediction; the kernels take the missing vy as 0."""
    n = O.normalize_bbox(b)
    if b.shape[-1] == 8:
        n = torch.cat([n, torch.zeros_like(n[..., :1])], -1)
    return n


def exp32(x):
    """x.exp() as the fp32 reference sees it: rounded to float32, so that it overflows to inf and underflows to 0 where float32 does
    (core/bbox/util.py:77-79 runs in fp32).  The identity on float32 input."""
    return x.exp().to(torch.float32).to(x.dtype)


def denormalize9(n):
    """core/bbox/util.py:60-87 for a 10-entry code: (cx, cy, cz, exp w, exp l, exp h, atan2(sin, cos), vx, vy)."""
    rot = torch.atan2(n[..., 6:7], n[..., 7:8])                                                                    # :62-65
    return torch.cat([n[..., 0:2], n[..., 4:5], exp32(n[..., 2:4]), exp32(n[..., 5:6]), rot, n[..., 8:10]], -1)    # :68-84


def l1_pairs(a, b):
    """torch.cdist(a, b, p=1) (match_cost.py:27) written out, so that inf and NaN entries follow plain arithmetic."""
    return (a[:, None, :] - b[None, :, :]).abs().sum(-1)


# ---------------------------------------------------------------------------------------------------------------------------------------
def match_cost64(cls, box, gt_boxes, gt_labels, gt_start, cls_weight=2.0, reg_weight=0.25, alpha=0.25, dtype=F64):
    """-> (cost, x): the flat buffer (NL * Q * sumG), block (l, b) at Q * (l * sumG + gt_start[b]) of shape (Q, G_b), and for every entry
    the logit of its box's class (what the focal term's conditioning depends on; NaN at the marker entries)."""
    cls, box, gt_boxes = _c(cls, dtype), _c(box, dtype), _c(gt_boxes, dtype)
    labels = gt_labels.detach().cpu().long()
    start = [int(s) for s in gt_start]
    nl, nb, q, c = cls.shape
    sum_gt = gt_boxes.shape[0]
    cost = torch.full((nl * q * sum_gt,), float('nan'), dtype=dtype)
    xs = torch.full((nl * q * sum_gt,), float('nan'), dtype=dtype)
    for l in range(nl):
        for b in range(nb):
            g0, g1 = start[b], start[b + 1]
            if g1 == g0:                                                                                 # hungarian_assigner_3d.py:104-110
                continue
            lab = labels[g0:g1]
            good = (lab >= 0) & (lab < c)
            safe = torch.where(good, lab, torch.zeros_like(lab))
            focal = O.focal_loss_cost(cls[l, b], safe, cls_weight, alpha)                                 # :117 (mmdet FocalLossCost)
            reg = l1_pairs(box[l, b, :, :8], O.normalize_bbox(gt_boxes[g0:g1])[:, :8]) * reg_weight       # :119-120, match_cost.py:27-28
            blk = torch.nan_to_num(focal + reg, nan=100.0, posinf=100.0, neginf=-100.0)                  # :123, :128
            x = cls[l, b][:, safe].clone()
            # KERNEL RULE: cls_pred[:, gt_labels] raises for a label outside [0, C) (:117); the kernel marks that column with NaN
            blk[:, ~good] = float('nan')
            x[:, ~good] = float('nan')
            off = q * (l * sum_gt + g0)
            cost[off:off + q * (g1 - g0)] = blk.reshape(-1)
            xs[off:off + q * (g1 - g0)] = x.reshape(-1)
    return cost, xs


def focal_cost_of_p(p, cls_weight=2.0, alpha=0.25):
    """mmdet FocalLossCost's entry (gamma = 2, eps = 1e-12) as a function of the sigmoid value, in the dtype of p."""
    neg = -(1 - p + 1e-12).log() * (1 - alpha) * p.pow(2)
    pos = -(p + 1e-12).log() * alpha * (1 - p).pow(2)
    return (pos - neg) * cls_weight


# ---------------------------------------------------------------------------------------------------------------------------------------
def _finish(terms, grads_of, before_nan_to_num):
    """terms: list over layers of (loss_cls, loss_box) scalars with graph -> (loss (NL, 2) after nan_to_num, the gradients)."""
    raw = torch.stack([torch.stack(t) for t in terms])
    loss = nan_to_num32(raw)                                                                             # :847-848 / :923-924
    (raw if before_nan_to_num else loss).sum().backward()
    return loss.detach(), [g.grad for g in grads_of]


def head_loss64(cls, box, assigned, gt_boxes, gt_labels, code_weights, avg_factors, alpha=0.25, loss_cls_weight=2.0,
                loss_bbox_weight=0.25, dtype=F64, before_nan_to_num=False, info=None):
    """-> (loss (NL, 2), grad_cls, grad_box).  `assigned` as the solvers write it: (NL, B, Q), an index into the packed ground truth or -1.
    info (a dict) receives 'abs_cls' / 'abs_box' (NL,): the sums of |term| behind each loss (for the L1 term of |pred| + |target|, both
    weighted: the target's rounding does not shrink with the difference), already times the normalisers, and 'matched' (NL,)."""
    cls, box = _c(cls, dtype).requires_grad_(), _c(box, dtype).requires_grad_()
    gt_boxes, cw, avg = _c(gt_boxes, dtype), _c(code_weights, dtype), _c(avg_factors, dtype)
    labels = gt_labels.detach().cpu().long()
    nl, nb, q, c = cls.shape
    sum_gt, gt_dim, code = gt_boxes.shape[0], gt_boxes.shape[1], box.shape[-1]
    cls_avg = max(float(avg[0]), 1.0)                                                                    # :828
    pos_avg = max(float(avg[1]), 1.0)                                                                    # :835
    # KERNEL RULE: the reference compares pred[:, :10] with all 8 / 10 normalised columns (:843-845) and so only admits (gt_dim, code) =
    # (7, 8) and (9, >= 10); the kernel compares the first nk columns of both for every pair, which is the same where the reference runs
    nk = min(10 if gt_dim > 7 else 8, code)
    terms, abs_cls, abs_box, matched = [], [], [], []
    for l in range(nl):
        a = assigned[l].detach().cpu().long().reshape(-1)
        a = torch.where((a >= 0) & (a < sum_gt), a, torch.full_like(a, -1))       # KERNEL RULE: an index outside the ground truth = background
        pos = a >= 0
        lab = torch.full_like(a, c)                                                                      # :714-716
        lab[pos] = labels[a[pos]]                                                                        # :717
        lab = torch.where((lab < 0) | (lab > c), torch.full_like(lab, c), lab)    # KERNEL RULE: one_hot raises; such a label = background
        x = cls[l].reshape(-1, c)
        t = F.one_hot(lab, num_classes=c + 1)[:, :c].to(dtype)                                           # mmdet FocalLoss: label C = background
        p = x.sigmoid()
        pt = (1 - p) * t + p * (1 - t)
        fw = (alpha * t + (1 - alpha) * (1 - t)) * pt.pow(2)
        focal = F.binary_cross_entropy_with_logits(x, t, reduction='none') * fw                          # = O.sigmoid_focal_loss_sum's summands
        loss_cls = loss_cls_weight * focal.sum() / cls_avg                                               # :829-830
        tgt = torch.zeros(a.numel(), gt_dim, dtype=dtype)                                                # :721-722
        tgt[pos] = gt_boxes[a[pos]]                                                                      # :727
        w = torch.zeros(a.numel(), nk, dtype=dtype)                                                      # :723
        w[pos] = 1.0                                                                                     # :724
        norm = normalize10(tgt)[:, :nk]                                                                  # :839
        ok = torch.isfinite(norm).all(-1)                                                                # :840
        w = w * cw[:nk]                                                                                  # :841
        pred = box[l].reshape(-1, code)                                                                  # :838
        l1 = (pred[ok, :nk] - norm[ok]).abs() * w[ok]                                                    # :843-844 (mmdet L1Loss, weighted)
        loss_box = loss_bbox_weight * l1.sum() / pos_avg                                                 # :845
        terms.append((loss_cls, loss_box))
        abs_cls.append(float(focal.detach().abs().nan_to_num(0, 0, 0).sum()) * abs(loss_cls_weight) / cls_avg)
        abs_box.append(float(((pred[ok, :nk].detach().abs() + norm[ok].abs()) * w[ok]).nan_to_num(0, 0, 0).sum())
                       * abs(loss_bbox_weight) / pos_avg)
        matched.append(int(pos.sum()))
    if info is not None:
        info.update(abs_cls=torch.tensor(abs_cls, dtype=F64), abs_box=torch.tensor(abs_box, dtype=F64), matched=matched, nk=nk)
    loss, (gc, gb) = _finish(terms, (cls, box), before_nan_to_num)
    return loss, gc, gb


# ---------------------------------------------------------------------------------------------------------------------------------------
def distill_match_cost64(s_cls, s_box, t_cls, t_box, cls_weight=1.0, reg_weight=0.25, pseudo_gt=False, dtype=F64):
    """-> the flat buffer (NL * B * Qs * Qt), block (l, b) at Qs * (l * B * Qt + b * Qt) of shape (Qs, Qt)."""
    s_cls, s_box, t_cls, t_box = _c(s_cls, dtype), _c(s_box, dtype), _c(t_cls, dtype), _c(t_box, dtype)
    nl, nb, qs, c = s_cls.shape
    qt = t_cls.shape[2]
    cost = torch.full((nl * nb * qs * qt,), float('nan'), dtype=dtype)
    for l in range(nl):
        for b in range(nb):
            if pseudo_gt:                                              # DistillHungarianAssigner3D.assign's own inputs
                soft, den = t_cls[l, b], t_box[l, b]
            else:
                soft = t_cls[l, 0].sigmoid()                           # detr4d_distiller.py:159: batch 0 for every sample
                den = denormalize9(t_box[l, b])                        # :160-161 (denormalize_bbox of each sample's own boxes)
            pos = F.binary_cross_entropy_with_logits(s_cls[l, b], torch.ones_like(s_cls[l, b]), reduction='none')     # match_cost.py:67-68
            neg = F.binary_cross_entropy_with_logits(s_cls[l, b], torch.zeros_like(s_cls[l, b]), reduction='none')    # match_cost.py:69-70
            ccost = (pos @ soft.T + neg @ (1 - soft).T) * cls_weight                                                  # match_cost.py:71-72, :92
            reg = l1_pairs(s_box[l, b, :, :8], O.normalize_bbox(den)[:, :8]) * reg_weight       # distill_hungarian_assigner_3d.py:109-110
            blk = ccost + reg                                                                   # :113 (no nan_to_num)
            # KERNEL RULE: scipy refuses -inf like NaN (:117); the kernel writes both as NaN, the solvers' status-1 marker
            blk = torch.where(blk == -math.inf, torch.full_like(blk, float('nan')), blk)
            off = qs * (l * nb * qt + b * qt)
            cost[off:off + qs * qt] = blk.reshape(-1)
    return cost


def distill_loss64(s_cls, s_box, t_cls, t_box, assigned, code_weights, avg_factors, reweight_score=False, loss_cls_weight=1.0,
                   loss_reg_weight=1.0, dtype=F64, before_nan_to_num=False, info=None):
    """-> (loss (NL, 2), grad_s_cls, grad_s_box).  `assigned` (NL, B, Qs) = b * Qt + teacher index, or -1.  info receives 'abs_cls' /
    'abs_box' (NL,) as in head_loss64 (the class term's parts summed by absolute value, the L1 term's with + 1 per entry for the
    target's round trip), 'div' (NL,): the reg divisors, and 'matched'."""
    s_cls, s_box = _c(s_cls, dtype).requires_grad_(), _c(s_box, dtype).requires_grad_()
    t_cls, t_box, cw, avg = _c(t_cls, dtype), _c(t_box, dtype), _c(code_weights, dtype), _c(avg_factors, dtype)
    nl, nb, qs, c = s_cls.shape
    qt, code = t_cls.shape[2], s_box.shape[-1]
    cls_avg = max(float(avg[0]), 1.0)                                                                    # :898
    pos_avg = max(float(avg[1]), 1.0)                                                                    # :905
    terms, abs_cls, abs_box, divs, matched = [], [], [], [], []
    for l in range(nl):
        soft = t_cls[l, 0].sigmoid()                                   # detr4d_distiller.py:159: sample 0's scores are every sample's labels
        a = assigned[l].detach().cpu().long().reshape(-1)
        b = torch.arange(nb).repeat_interleave(qs)
        t = a - b * qt
        pos = (a >= 0) & (t >= 0) & (t < qt)                           # KERNEL RULE: an index outside the sample's teacher rows = unmatched
        labels = torch.full((a.numel(), c), float(c), dtype=dtype)                                       # :969-971
        labels[pos] = soft[t[pos]]                                                                       # :972
        tgt = torch.zeros(a.numel(), 9, dtype=dtype)                                                     # :976
        tgt[pos] = denormalize9(t_box[l])[b[pos], t[pos]]                                                # :1009
        bw = torch.zeros(a.numel(), 10, dtype=dtype)                                                     # :977
        bw[pos] = 1.0                                                                                    # :978
        x = s_cls[l].reshape(-1, c)                                                                      # :890
        bce = F.binary_cross_entropy_with_logits(x, labels, reduction='none')                            # distill_cross_entropy_loss.py:141-142
        loss_cls = loss_cls_weight * bce.sum() / cls_avg                                                 # :144-145, :240, :899-900
        div = torch.tensor(pos_avg, dtype=dtype)
        if reweight_score:
            rs = labels.max(-1, keepdim=True)[0]                                                         # :908
            bw = bw * rs                                                                                 # :909
            div = rs[labels[:, 0] != 10].sum()                                                           # :910-911: the literal 10, no clamp
        tn = O.normalize_bbox(tgt)                                                                       # :915
        ok = torch.isfinite(tn).all(-1)                                                                  # :916
        bw = bw * cw                                                                                     # :917
        pred = s_box[l].reshape(-1, code)                                                                # :914
        l1 = (pred[ok, :10] - tn[ok, :10]).abs() * bw[ok, :10]                                           # :919-920
        loss_reg = loss_reg_weight * l1.sum() / div                                                      # :921
        terms.append((loss_cls, loss_reg))
        xd = x.detach()
        parts = xd.clamp(min=0) + (xd * labels).abs() + torch.log1p(torch.exp(-xd.abs()))
        abs_cls.append(float(parts.nan_to_num(0, 0, 0).sum()) * abs(loss_cls_weight) / cls_avg)
        ad = float(div.abs()) if float(div) != 0 and math.isfinite(float(div)) else 1.0
        abs_box.append(float(((pred[ok, :10].detach().abs() + tn[ok, :10].abs() + 1) * bw[ok, :10]).nan_to_num(0, 0, 0).sum())
                       * abs(loss_reg_weight) / ad)
        divs.append(float(div))
        matched.append(int(pos.sum()))
    if info is not None:
        info.update(abs_cls=torch.tensor(abs_cls, dtype=F64), abs_box=torch.tensor(abs_box, dtype=F64), div=divs, matched=matched)
    loss, (gc, gb) = _finish(terms, (s_cls, s_box), before_nan_to_num)
    return loss, gc, gb
