"""The covering tables, the inputs and the comparison rules of test_loss_kernels_gpu.py.  Everything here runs on the CPU
(test_loss_ref_cpu.py uses focal_interval on the fixtures); not a test module.

Tolerances - nothing here is fitted to a kernel's output.

U = 2^-24 is one rounding of a float32 operation.  The device's expf, logf, log1pf, sinf, cosf and atan2f are taken to be within 2 ulp
(4 U) each and float32 division within 1 ulp (2 U): an assumption - the public HIP math API table as recalled; no copy of it ships
with the toolchain, see docs/measurements_r46.md.

  element-wise (gradients, well-conditioned cost entries): the error of a float32 CPU evaluation of the SAME restatement against its
      float64 evaluation is measured on the case's own inputs (the reference's error); the kernel may be MULT = 4 times as far: its
      functions are allowed 2 ulp where the host's are good to half an ulp.  A case too small to show any rounding gets the floor
      k_ops U, k_ops the number of rounded operations on the longest path to one element (stated per kernel below).
  sums (the losses): (serial + 22 + k_term) U sum|term| - serial additions per thread, 6 butterfly steps and 16 wave partials, k_term
      roundings in one term - plus the additive pieces stated at SUM_RULES; derived, not measured.
  the focal cost: three regimes by the logit x of the box's class, see check_match_cost."""
import math

import torch

import loss_ref as R

U = 2.0 ** -24
MULT = 4.0
X_LOW = 6.0
# 1 / (1 + expf(-x)) == 1.0f as soon as 1 + e rounds to 1: e <= 2^-24 (the tie goes to the even 1.0).  With expf within 2 ulp,
# e <= exp(-x) (1 + 2^-22), so x >= 24 ln 2 + 2^-22 suffices; 1e-3 leaves three orders of magnitude of room.
X_SAT = 24.0 * math.log(2.0) + 1e-3
# p = 1 / (1 + expf(-x)) for x > 6, in ulps of p (2^-24 on [1/2, 1)): expf's 2 ulp of e <= exp(-6) move p by 2^-22 e < 0.01; the
# rounding of 1 + e is half an ulp of [1, 2) = 2^-24 -> at most 1; the division at most 1; rounding sigmoid64(x) itself to float32
# half.  0.01 + 1 + 1 + 0.5 < 3, and p lies on the grid.
K_ULP = 3
MID_SHARE = 0.05
K_OPS = dict(match_cost=48,      # per entry: p (expf 4, add, div 2), two logs (4 + 1 each), 8 products, 8 (sub, abs, add) x 2 with logf / sinf in
                                 # the target (4), 2 weights, 1 add
             head_cls=40,        # p (7), pt (1), bce (expf 4, log1pf 4, 2 adds), fw (3), two products and a sum (6), dpt (3), kc (2)
             head_box=4,         # kb = w / avg (2), kb w (1), sign: exact
             distill_cost=24,    # relative to its own value: a sum of non-negative terms; per term bce (10), p (7), 2 products, adds: the
                                 # sum's roundings are bounded by C + 8 <= 72 more, counted separately in check
             distill_cls=16,     # y (7), sigmoid (7), sub, kc
             distill_box=16)     # lmax (7), w (2), kb = w / div (3), the product (1), 3 spare; under reweight_score the divisor is a
                                 # fixed-order float32 sum of its own: + ceil(rows / 1024) + 22, added by the test


# ---------------------------------------------------------------------------------------------------------------------------------------
# covering tables (the issue's values; every value appears, and each pair that shares an index expression - Q with the counts and NL in
# the block offset, Q with C and code in the row pointers, gt_dim with the counts in the box pointer - meets its neighbour's edge values)
MATCH_CASES = [
    # Q, counts, NL, C, code, gt_dim
    (1, [1], 1, 1, 8, 7),
    (63, [3, 0, 5], 3, 10, 10, 9),
    (64, [0, 4], 1, 23, 11, 8),
    (65, [4, 0], 3, 10, 8, 9),
    (130, [257], 1, 23, 10, 7),
    (65, [1024], 1, 10, 11, 9),
    (64, [3, 0, 5], 1, 1, 10, 8),
    (130, [3, 0, 5], 3, 10, 11, 7),
    (1, [0, 4], 3, 23, 10, 9),
    (63, [4, 0], 1, 10, 8, 8),
    (64, [257], 3, 1, 8, 9),
    (1, [1024], 1, 23, 11, 7),
]
HEAD_CASES = [
    # B, Q, NL, C, gt_dim, code, avg_factors
    (1, 1, 1, 1, 7, 8, (0.0, 0.0)),
    (1, 63, 3, 10, 9, 10, (0.5, 0.5)),
    (3, 21, 1, 23, 7, 10, (37.0, 12.0)),
    (1, 1023, 1, 10, 8, 10, (37.0, 12.0)),
    (3, 341, 3, 1, 9, 8, (0.5, 0.5)),
    (1, 1024, 3, 23, 9, 16, (37.0, 12.0)),
    (2, 512, 1, 10, 7, 8, (0.0, 0.0)),
    (1, 1025, 1, 23, 9, 10, (0.0, 0.0)),
    (5, 205, 3, 10, 9, 16, (37.0, 12.0)),
    (1, 2055, 1, 10, 9, 10, (37.0, 12.0)),
    (3, 685, 3, 23, 8, 10, (0.5, 0.5)),
]
DCOST_CASES = [
    # Qs, Qt, C, code, pseudo_gt, NL  (B = 2 throughout)
    (1, 1, 1, 8, 0, 1),
    (63, 64, 10, 10, 0, 2),
    (64, 65, 64, 12, 1, 1),
    (65, 63, 10, 8, 1, 2),
    (130, 1, 64, 10, 0, 1),
    (1, 130, 10, 12, 0, 2),
    (64, 64, 1, 10, 1, 1),
    (65, 130, 10, 10, 0, 1),
    (130, 65, 1, 12, 1, 2),
    (63, 63, 64, 8, 0, 1),
    (130, 130, 10, 10, 1, 1),
]
# The issue asks for head_loss's row counts and for B = 2; 1, 63, 1023, 1025 and 2055 are odd, so B = 2 is kept where it divides (1024) and
# the others split over 1, 3 or 5 samples, which exercises b = row / Qs the same way.
DLOSS_CASES = [
    # B, Qs, Qt, NL, C, code, reweight
    (1, 1, 1, 1, 10, 10, 0),
    (3, 21, 30, 3, 12, 16, 1),
    (3, 341, 64, 1, 10, 10, 1),
    (2, 512, 300, 3, 12, 10, 0),
    (5, 205, 205, 1, 10, 16, 0),
    (3, 685, 100, 3, 10, 10, 1),
    (1, 1025, 7, 3, 12, 10, 1),
    (1, 1023, 1023, 1, 10, 16, 0),
    (1, 63, 5, 3, 10, 16, 0),
]

LOW_X = [5.9, -5.9, 30.0, -30.0, 100.0, -100.0, 17.5, 20.0]      # outside the ill-conditioned band (X_LOW, X_SAT)
MID_X = [7.5, 9.0, 12.0, 15.0, 16.5]                               # inside it: a fixed handful, placed while the share allows


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _boxes(n, gt_dim, g):
    b = torch.randn(n, 9, generator=g)
    b[:, 0:2] *= 30.0
    b[:, 3:6] = b[:, 3:6].abs() * 2 + 0.3
    return b[:, :gt_dim].contiguous()


def _codes(shape, g):
    """Box codes as a head emits them: centres of tens of metres, log sizes, (sin, cos), velocities."""
    c = torch.randn(*shape, generator=g)
    c[..., 0:2] *= 30.0
    return c


def match_inputs(case, seed):
    """-> dict of CPU tensors and scalars for one MATCH_CASES row.  Layer 0 is free of non-finite predictions."""
    q, counts, nl, c, code, gt_dim = case
    g = _gen(seed)
    nb, sum_gt = len(counts), sum(counts)
    start = [0]
    for n in counts:
        start.append(start[-1] + n)
    cls = (torch.randn(nl, nb, q, c, generator=g) * 3).clamp(max=5.5)
    box = _codes((nl, nb, q, code), g)
    gt = _boxes(sum_gt, gt_dim, g)
    lab = torch.randint(0, c, (sum_gt,), generator=g).to(torch.int32)
    # degenerate ground truth, at most half of each sample's boxes: zero width, negative width, NaN entry, +inf entry, a label out of range
    for b, n in enumerate(counts):
        for i in range(min(5, n // 2)):
            j = start[b] + (i * 2 + 1) % n
            if i == 0:
                gt[j, 3] = 0.0
            elif i == 1:
                gt[j, 4] = -1.5
            elif i == 2:
                gt[j, 1] = float('nan')
            elif i == 3:
                gt[j, 0] = float('inf')
            else:
                lab[j] = c if b % 2 == 0 else -1
    # deliberate logits in the classes the boxes carry
    b0 = next(i for i, n in enumerate(counts) if n)
    plain = [j for j in range(start[b0], start[b0 + 1]) if 0 <= int(lab[j]) < c]
    total = nl * q * sum_gt
    per_label = torch.bincount(lab[start[b0]:start[b0 + 1]].clamp(0, c - 1).long(), minlength=c)
    mid = 0
    for i, x in enumerate(LOW_X + MID_X):
        l, qq, col = i % nl, (i * 7) % q, int(lab[plain[i % len(plain)]])
        if x in MID_X:
            if (mid + int(per_label[col])) > 0.8 * MID_SHARE * total:
                continue
            mid += int(per_label[col])
        cls[l, b0, qq, col] = x
    if q > 2:
        cls[nl - 1, b0, q - 1, int(lab[plain[0]])] = float('nan')          # a NaN logit in one layer only
        if nl > 1:
            box[nl - 1, b0, q - 2, 3] = float('nan')                         # a NaN and a +inf box prediction
            box[1, b0, q - 3 if q > 3 else 0, 0] = float('inf')
    return dict(cls=cls, box=box, gt_boxes=gt, gt_labels=lab, gt_start=torch.tensor(start, dtype=torch.int32), start=start,
                max_gt=max(counts), cls_weight=2.0, reg_weight=0.25, alpha=0.25)


def head_inputs(case, seed):
    """-> dict for one HEAD_CASES row.  Layer 0 has finite predictions only; with NL > 1 layer 1 holds a +inf box prediction in a matched
    row and layer NL - 1 a NaN logit and a NaN box prediction."""
    nb, q, nl, c, gt_dim, code, avg = case
    g = _gen(seed)
    sum_gt, rows = 12, nb * q
    cls = torch.randn(nl, nb, q, c, generator=g) * 3
    box = _codes((nl, nb, q, code), g)
    gt = _boxes(sum_gt, gt_dim, g)
    lab = torch.randint(0, c, (sum_gt,), generator=g).to(torch.int32)
    gt[1, 3] = 0.0                                                           # zero width: log -> -inf, the row is dropped
    gt[3, 5] = -2.0                                                          # negative height: NaN
    gt[5, 2] = float('nan')
    gt[7, 0] = float('inf')
    lab[2], lab[4], lab[6] = c, -1, c + 3                                    # stored labels: C (background, box term stays), out of range
    a = torch.full((nl, rows), -1, dtype=torch.int32)
    pick = torch.rand(nl, rows, generator=g) < 0.3
    a[pick] = torch.randint(0, sum_gt, (int(pick.sum()),), generator=g).to(torch.int32)
    for l in range(nl):
        for i, v in enumerate([sum_gt, sum_gt + 5, -7, 2, 1, 8]):            # index-safety values, the label == C box, a dropped box, a plain one
            a[l, (i * 5 + l) % rows] = v
    a = a.view(nl, nb, q)
    norm = R.normalize10(gt.double()).float()
    exact = [k for k in (0, 1, 4, 8) if k < min(10 if gt_dim > 7 else 8, code)]   # columns whose target is a copy of a float32 input
    n_exact = 0
    for l in range(nl):
        for r in range(rows):
            j = int(a.view(nl, rows)[l, r])
            if 0 <= j < sum_gt and (r + l) % 3 == 0 and j not in (5, 7):
                for k in exact[:1 + (r % len(exact))]:
                    box.view(nl, rows, code)[l, r, k] = norm[j, k]
                n_exact += 1
    flat = cls.view(nl, rows, c)
    for i, x in enumerate(LOW_X + MID_X if rows >= 16 else []):               # (a one-row case keeps its plain logit)
        l, r = i % nl, (i * 11) % rows
        j = int(a.view(nl, rows)[l, r])
        col = int(lab[j]) if 0 <= j < sum_gt and 0 <= int(lab[j]) < c and i % 2 == 0 else (i % c)    # at the target class and beside it
        flat[l, r, col] = x
    if nl > 1:
        matched = [[r for r in range(rows) if int(a.view(nl, rows)[l, r]) == 8] for l in range(nl)]
        box.view(nl, rows, code)[1, matched[1][0], 2] = float('inf')
        box.view(nl, rows, code)[nl - 1, matched[nl - 1][0], 6] = float('nan')
        flat[nl - 1, rows // 2, c // 2] = float('nan')
    cw = torch.tensor([1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.2])
    return dict(cls=cls, box=box, assigned=a, gt_boxes=gt, gt_labels=lab, code_weights=cw, avg_factors=torch.tensor(avg), alpha=0.25,
                loss_cls_weight=2.0, loss_bbox_weight=0.25, exact_rows=n_exact, exact_cols=exact)


def _teacher_codes(shape, g):
    t = _codes(shape, g)
    n = t.reshape(-1, shape[-1])
    specials = min(5, n.shape[0] // 2)
    for i in range(specials):
        j = (i * 2 + 1) % n.shape[0]
        if i == 0:
            n[j, 2] = 100.0                                                  # exp overflow: the target is +inf
        elif i == 1:
            n[j, 3] = -110.0                                                 # exp underflow to 0: log gives -inf
        elif i == 2:
            n[j, 6], n[j, 7] = 0.0, 0.0                                      # atan2(0, 0) = 0: (sin, cos) comes back as (0, 1)
        elif i == 3:
            n[j, 4] = float('nan')
        else:
            n[j, 0] = float('inf')
    return t


def _student_logits(shape, g):
    x = torch.randn(*shape, generator=g) * 3
    f = x.reshape(-1)
    for i, v in enumerate(LOW_X + MID_X):                                    # the stable BCE forms have no band: all of them, everywhere
        f[(i * 13 + 1) % f.numel()] = v
    return x


def dcost_inputs(case, seed):
    """-> dict for one DCOST_CASES row; B = 2 with different teacher logits per sample.  The last layer holds the student's NaN logit and
    non-finite boxes (row 0 of sample 0 stays clean when Qs > 3)."""
    qs, qt, c, code, pseudo, nl = case
    g = _gen(seed)
    nb = 2
    s_cls, s_box = _student_logits((nl, nb, qs, c), g), _codes((nl, nb, qs, code), g)
    t_cls = _student_logits((nl, nb, qt, c), g)
    if pseudo:
        t_cls = t_cls.sigmoid()                                              # soft labels per sample
        t_box = _boxes(nl * nb * qt, 9, g).view(nl, nb, qt, 9)
        n = t_box.view(-1, 9)
        for i in range(min(4, n.shape[0] // 2)):
            j = (i * 2 + 1) % n.shape[0]
            if i == 0:
                n[j, 3] = 0.0
            elif i == 1:
                n[j, 4] = -1.5
            elif i == 2:
                n[j, 1] = float('nan')
            else:
                n[j, 0] = float('inf')
    else:
        t_box = _teacher_codes((nl, nb, qt, 10), g)
    if qs > 3:
        s_cls[nl - 1, 0, qs - 1, c // 2] = float('nan')
        s_box[nl - 1, 1, qs - 2, 3] = float('nan')
        s_box[nl - 1, 1, qs - 3, 0] = float('inf')
    return dict(s_cls=s_cls, s_box=s_box, t_cls=t_cls, t_box=t_box, cls_weight=1.0, reg_weight=0.25, pseudo_gt=bool(pseudo))


def dloss_inputs(case, seed):
    """-> dict for one DLOSS_CASES row.  Layer 0 has finite student predictions; with NL = 3 layer 1 has NO matched row and layer 2 a NaN
    logit, a NaN box entry and a +inf box entry in matched rows."""
    nb, qs, qt, nl, c, code, rw = case
    g = _gen(seed)
    rows = nb * qs
    s_cls, s_box = _student_logits((nl, nb, qs, c), g), _codes((nl, nb, qs, code), g)
    t_cls, t_box = _student_logits((nl, nb, qt, c), g), _teacher_codes((nl, nb, qt, 10), g)
    a = torch.full((nl, nb, qs), -1, dtype=torch.int32)
    for l in range(nl):
        for b in range(nb):
            pick = torch.rand(qs, generator=g) < 0.5
            a[l, b][pick] = (b * qt + torch.randint(0, qt, (int(pick.sum()),), generator=g)).to(torch.int32)
            if qs > 6:
                a[l, b, 0] = b * qt + (1 % qt)                               # teacher rows with the degenerate codes
                a[l, b, 1] = b * qt + (3 % qt)
                a[l, b, 2] = b * qt + (5 % qt)
                a[l, b, 3] = b * qt - 1                                      # below the sample's range (another sample's row, or < 0)
                a[l, b, 4] = (b + 1) * qt                                    # above it
                a[l, b, 5] = -7
                a[l, b, 6] = b * qt                                          # a plain match
    if nl == 3:
        a[1] = -1
        s_cls[2, nb - 1, qs - 1, c // 2] = float('nan')
        if qs > 6:
            s_box[2, 0, 6, 4] = float('nan')
            s_box[2, nb - 1, 6, 1] = float('inf') if nb > 1 else s_box[2, nb - 1, 6, 1]
    # predictions equal to their target in columns the teacher round trip copies (0, 4, 9), in the plain match of layer 0
    if qs > 6:
        for b in range(nb):
            for k in (0, 4, 9):
                s_box[0, b, 6, k] = t_box[0, b, int(a[0, b, 6]) - b * qt, k]
    cw = torch.tensor([1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.2])
    return dict(s_cls=s_cls, s_box=s_box, t_cls=t_cls, t_box=t_box, assigned=a, code_weights=cw, avg_factors=torch.tensor([37.0, 12.0]),
                reweight_score=bool(rw), loss_cls_weight=1.0, loss_reg_weight=0.25)


# ---------------------------------------------------------------------------------------------------------------------------------------
# comparison rules.  Each returns the largest observed error as a fraction of its bound (for docs/measurements_r46.md) and prints it.
def same_marks(what, got, ref):
    """NaN, +inf, -inf and the clamp values 100 / -100 sit at the same places; returns the mask of the entries left to compare."""
    for name, f in (('NaN', torch.isnan), ('+inf', lambda t: t == math.inf), ('-inf', lambda t: t == -math.inf)):
        assert torch.equal(f(got), f(ref)), f'{what}: the {name} entries are not where the restatement has them'
    return torch.isfinite(ref)


def elementwise(what, got, ref64, ref32, k_ops, scale=None, mask=None):
    """|got - ref64| <= max(MULT * (the float32 restatement's error on these inputs), k_ops U), both relative to `scale` (default: the
    largest finite |ref64|; a tensor gives a scale per element)."""
    fin = same_marks(what, got, ref64)
    if mask is not None:
        fin = fin & mask
    fin32 = fin & torch.isfinite(ref32)
    if int(fin.sum()) == 0:
        return 0.0
    if scale is None:
        scale = float(ref64[fin].abs().max())
        scale = scale if scale > 0 else 1.0
    s = scale[fin] if torch.is_tensor(scale) else scale
    s32 = scale[fin32] if torch.is_tensor(scale) else scale
    ref_err = float(((ref32.double()[fin32] - ref64[fin32]).abs() / s32).max()) if int(fin32.sum()) else 0.0
    bound = max(MULT * ref_err, k_ops * U)
    err = float(((got.double()[fin] - ref64[fin]).abs() / s).max())
    print(f'{what}: error {err:.3e}, reference float32 error {ref_err:.3e}, bound {bound:.3e}, fraction {err / bound:.3f}')
    assert err <= bound, f'{what}: {err:.3e} > {bound:.3e} (float32 restatement: {ref_err:.3e})'
    return err / bound


def check_match_cost(what, got, cost64, cost32, x, cls_weight=2.0, alpha=0.25):
    """The focal cost's three regimes, by the logit x of the entry's class:
      x <= X_LOW           the element-wise rule against float64;
      x >= X_SAT           p is exactly 1.0f whatever expf does within its error: the cost is a constant of the float32 formula - the
                           element-wise rule against the float32 CPU evaluation;
      in between           the entry lies between the float64 formula at float32(sigmoid64(x)) moved K_ULP ulp either way (the cost falls
                           as p grows), each end widened by the element-wise bound; at most MID_SHARE of the compared entries.
    Clamp values and markers exactly."""
    for v in (100.0, -100.0):
        assert torch.equal(got == v, cost64 == v), f'{what}: the entries clamped to {v} are not where the restatement has them'
    plain = same_marks(what, got, cost64) & (cost64.abs() != 100.0)
    scale = cost64.abs().clamp(min=1.0).nan_to_num(1.0, 1.0, 1.0)
    low, sat = plain & (x <= X_LOW), plain & (x >= X_SAT)
    mid = plain & ~low & ~sat
    n = int(plain.sum())
    share = int(mid.sum()) / max(n, 1)
    print(f'{what}: {n} entries, {int(low.sum())} low, {int(mid.sum())} in the band ({share:.4f}), {int(sat.sum())} saturated')
    assert share <= MID_SHARE, f'{what}: {share:.3f} of the entries lie in the ill-conditioned band'
    frac = elementwise(what + ' [x <= 6]', got, cost64, cost32, K_OPS['match_cost'], scale, low)
    fin = low & torch.isfinite(cost32)
    ref_err = float(((cost32.double()[fin] - cost64[fin]).abs() / scale[fin]).max()) if int(fin.sum()) else 0.0
    bound = max(MULT * ref_err, K_OPS['match_cost'] * U)
    if int(sat.sum()):
        err = float(((got.double()[sat] - cost32.double()[sat]).abs() / scale[sat]).max())
        print(f'{what} [saturated]: {err:.3e} against the float32 evaluation, bound {bound:.3e}')
        assert err <= bound, f'{what}: saturated entries {err:.3e} > {bound:.3e}'
        frac = max(frac, err / bound)
    if int(mid.sum()):
        lo, hi = focal_interval(cost64[mid], x[mid], cls_weight, alpha)
        w = bound * scale[mid]
        g = got.double()[mid]
        out = float(torch.maximum((lo - g) / w, (g - hi) / w).max())
        print(f'{what} [band]: outside its interval by {max(out, 0.0):.3f} of the widening')
        assert out <= 1.0, f'{what}: a band entry leaves its interval by {out:.2f} x the element-wise bound'
        frac = max(frac, max(out, 0.0))
    return frac


def focal_interval(cost64, x, cls_weight=2.0, alpha=0.25, k=K_ULP):
    """[lo, hi] of an entry whose class logit is x > 0: cost64 with its focal part re-evaluated (in float64) at float32(sigmoid64(x)) moved
    k float32 ulp (2^-24 on [1/2, 1), never above 1) either way."""
    p64 = x.sigmoid()
    rest = cost64 - R.focal_cost_of_p(p64, cls_weight, alpha)
    p32 = p64.float().double()
    step = k * 2.0 ** -24
    lo = R.focal_cost_of_p((p32 + step).clamp(max=1.0), cls_weight, alpha) + rest
    hi = R.focal_cost_of_p(p32 - step, cls_weight, alpha) + rest
    return lo, hi


# SUM_RULES.  loss = k * sum(term), compared after the same k and nan_to_num in float64.
#   head_loss focal   serial = ceil(rows / 1024) C; k_term = 24: bce 10 (expf 4, log1pf 4, two additions), p 7, pt^2 and its weight 4, the
#                     product 1, k 2.  pt = 1 - p at the target class cancels, which k_term does not cover: there |d term| <= bce aw 2 pt
#                     |d p| <= 0.7 * 1 * 2 * 4 U per MATCHED row, an additive `matched 6 U k`.
#   head_loss L1      serial = ceil(rows / 1024) nk; k_term = 8 on sum w (|pred| + |target|): the target's logf / sinf 4, sub, product, k 2.
#   distill BCE       serial = ceil(rows / 1024) C; k_term = 24 on sum (max(v, 0) + |v y| + log1p(exp(-|v|))): y 7, expf 4, log1pf 4, product,
#                     three additions, k 2, and 3 spare.
#   distill L1        serial = ceil(rows / 1024) 10; k_term = 24 on sum w (|pred| + |target| + 1): the round trip log(exp(t)) is within
#                     (4 + 4 |t|) U and sin(atan2) within 8 U absolute (hence the + 1), w = cw lmax 8, sub, product, the division by the
#                     divisor and its own fixed-order sum (ceil(rows / 1024) + 22) U relative, added to k_term under reweight_score.
def check_loss_sums(what, got, ref64, abs_terms, serial, k_term, extra=None):
    """got, ref64 (NL,): one loss column.  A term nan_to_num replaced (0, or +/-FLT_MAX) and an exactly-zero loss are compared exactly."""
    worst = 0.0
    for l in range(ref64.numel()):
        r, gv = float(ref64[l]), float(got[l])
        if r == 0.0 or abs(r) == R.FLT_MAX:
            assert gv == r or (abs(r) == R.FLT_MAX and gv == float(torch.tensor(r).float())), f'{what} layer {l}: {gv} where the restatement has {r}'
            continue
        bound = (serial + 22 + k_term) * U * float(abs_terms[l]) + (float(extra[l]) if extra is not None else 0.0)
        err = abs(gv - r)
        print(f'{what} layer {l}: {gv:.9g} vs {r:.9g}, error {err:.3e}, bound {bound:.3e}, fraction {err / bound:.3f}')
        assert err <= bound, f'{what} layer {l}: {err:.3e} > {bound:.3e}'
        worst = max(worst, err / bound)
    return worst
