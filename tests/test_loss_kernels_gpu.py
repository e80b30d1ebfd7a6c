"""gd4d_match_cost_fwd, gd4d_head_loss_fwd_bwd, gd4d_distill_match_cost_fwd and gd4d_distill_loss_fwd_bwd at their edges, called through
ops.* directly, element by element against the float64 restatements of loss_ref.py (themselves pinned to the reference's fixtures by
test_loss_ref_cpu.py).  The tables, inputs, rules and the derivation of every bound are in loss_cases.py (each rule prints the
error as a fraction of its bound; the largest per kernel are recorded in docs/measurements_r46.md).  GPU only.

Every case runs under the memory contract: floating-point inputs embedded in NaN, outputs in guarded buffers - pre-filled with NaN for
the first launch and with a finite value for the second, so that equal bits prove both "two runs agree" and "every element was
written" even where the result itself is NaN - and, with more than one layer, a third launch with the LAST layer's predictions
changed, after which the other layers keep their bits."""
import pytest
import torch

import loss_cases as C
import loss_ref as R
from contract import DEV, Handed, Run, as_input

pytestmark = pytest.mark.gpu
F32 = torch.float32


def _launch(fn, args, kw, float_inputs, shapes, fill):
    """One launch of ops.<fn> with the named floating-point inputs embedded in NaN and its outputs guarded -> list of CPU results."""
    from graph_detr4d_amd import ops
    run = Run()
    dev = {k: (as_input(v) if k in float_inputs else v.to(DEV)) if torch.is_tensor(v) else v for k, v in args.items()}
    outs = tuple(run.out(s, fill=fill) for s in shapes)
    with Handed() as seen:
        res = getattr(ops, fn)(*[dev[k] for k in args], **kw, outs=outs)
    torch.cuda.synchronize()
    res = (res,) if torch.is_tensor(res) else tuple(res)
    for i, (shape, _, view) in enumerate(run.guards):
        assert view.data_ptr() in seen.ptrs, f'{fn}: guarded buffer {i} {shape} was never handed to the library'
        assert res[i].data_ptr() == view.data_ptr(), f'{fn}: result {i} is not the guarded buffer'
    run.check(fn)
    return [t.cpu() for t in res]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _three_launches(fn, args, kw, float_inputs, shapes, nl, other_layer):
    """-> the first launch's results, after: guards intact; a second launch into buffers of another fill gives the same bits (fixed-order
    sums; nothing left unwritten); with nl > 1 a launch on other_layer(args) keeps every layer but the last bit for bit."""
    first = _launch(fn, args, kw, float_inputs, shapes, float('nan'))
    second = _launch(fn, args, kw, float_inputs, shapes, 0.5)
    for i, (a, b) in enumerate(zip(first, second)):
        assert torch.equal(_bits(a), _bits(b)), f'{fn}: output {i} differs between two runs, or keeps elements of its pre-fill'
    if nl > 1:
        third = _launch(fn, other_layer(args), kw, float_inputs, shapes, float('nan'))
        for i, (a, b) in enumerate(zip(first, third)):
            a, b = _bits(a).reshape(nl, -1), _bits(b).reshape(nl, -1)
            assert torch.equal(a[:nl - 1], b[:nl - 1]), f'{fn}: output {i} of an untouched layer changed with the last layer\'s inputs'
            if a.shape[1] > 2:                                               # (the loss pair of a layer nan_to_num replaced stays (0, 0))
                assert not torch.equal(a[nl - 1], b[nl - 1]), f'{fn}: output {i} of the changed layer did not move'
    return first


def _shift_last(args, names):
    out = dict(args)
    for k in names:
        t = args[k].clone()
        t[-1] = t[-1].flip(1) * 0.75 + 0.125                                 # other predictions in the last layer only
        out[k] = t
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', C.MATCH_CASES, ids=lambda c: 'Q%d-G%s-NL%d-C%d-code%d-gt%d' % (c[0], '_'.join(map(str, c[1])), *c[2:]))
def test_match_cost_tile_edges_ragged_layout_columns_saturation_and_markers(case):
    """Items 2-6 of the issue for gd4d_match_cost_fwd.  Mutations this fails under: `nq = min(MC_QB, Q - q0)` -> `MC_QB` (guard, Q = 63,
    65, 130); `g0` dropped from the block offset (cases with an empty sample first or in the middle); the k < 8 loops run to `code`
    (code 10, 11); `o[8]`-style reads of a 7-entry box (gt_dim 7: the NaN around the embedded input); `1e-12f` dropped (x = -100);
    `c == INFINITY` -> 100 removed (the +inf box); the label check `lab >= p.C` -> `>` (label == C reads the next row's logit).
    Bounds: loss_cases.check_match_cost (three regimes by the class logit; band share <= 5 % asserted there)."""
    q, counts, nl, c, code, gt_dim = case
    d = C.match_inputs(case, seed=4600 + q + sum(counts))
    names = ('cls', 'box', 'gt_boxes', 'gt_labels', 'gt_start')
    args = {k: d[k] for k in names}
    args['max_gt'] = d['max_gt']
    kw = dict(cls_weight=d['cls_weight'], reg_weight=d['reg_weight'], alpha=d['alpha'])
    got, = _three_launches('match_cost_fwd', args, kw, ('cls', 'box', 'gt_boxes'), [(nl * q * sum(counts),)], nl,
                           lambda a: _shift_last(a, ('cls', 'box')))
    ref = (d['cls'], d['box'], d['gt_boxes'], d['gt_labels'], d['start'], d['cls_weight'], d['reg_weight'], d['alpha'])
    cost64, x = R.match_cost64(*ref)
    cost32, _ = R.match_cost64(*ref, dtype=F32)
    assert not torch.isnan(got[torch.isfinite(cost64)]).any()
    C.check_match_cost('match_cost', got, cost64, cost32, x, d['cls_weight'], d['alpha'])


def test_match_cost_refuses_more_boxes_than_its_lds_holds():
    """max_gt = 1025 > MC_MAX_GT: GD4D_EUNSUPPORTED, as include/gd4d.h states (max_gt <= 1024), before any launch."""
    from graph_detr4d_amd import _lib, ops
    z = torch.zeros
    with pytest.raises(_lib.Gd4dError, match=r'code -2\b'):
        ops.match_cost_fwd(z(1, 1, 1, 10, device=DEV), z(1, 1, 1, 10, device=DEV), z(1025, 9, device=DEV),
                           z(1025, dtype=torch.int32, device=DEV), torch.tensor([0, 1025], dtype=torch.int32, device=DEV), 1025)


# ---------------------------------------------------------------------------------------------------------------------------------------
def _grad_rules(kernel, got_c, got_b, ref, ref32, nk_cols, code, box_extra=0):
    """Both gradients element by element (loss_cases.elementwise), columns >= nk exactly +0.0.  box_extra: roundings of a divisor that
    is itself a fixed-order float32 sum."""
    _, gc64, gb64 = ref
    _, gc32, gb32 = ref32
    C.elementwise(kernel + ' grad_cls', got_c, gc64, gc32, C.K_OPS[kernel + '_cls'])
    C.elementwise(kernel + ' grad_box', got_b, gb64, gb32, C.K_OPS[kernel + '_box'] + box_extra)
    if nk_cols < code:
        assert torch.count_nonzero(_bits(got_b[..., nk_cols:])).item() == 0, f'{kernel}: gradient columns >= {nk_cols} are not +0.0'


@pytest.mark.parametrize('case', C.HEAD_CASES, ids=lambda c: 'B%d-Q%d-NL%d-C%d-gt%d-code%d' % c[:6] + '-avg%g' % c[6][0])
def test_head_loss_sweep_loop_columns_saturation_nonfinite_and_index_safety(case):
    """Items 1, 4, 5, 6, 7 and the label == C quirk of item 8 for gd4d_head_loss_fwd_bwd.  Mutations this fails under: the row loop
    dropped (`for (r = tid; ...; r += 1024)` -> one pass: 1025 and 2055 rows leave gradients unwritten and the sums short); `nk` fixed
    at 10 (gt_dim 7, code 8 / 16: reads past the box, non-zero gradient columns); the `a >= p.sumG` line removed (assigned = sumG,
    sumG + 5 index past gt_labels and gt_boxes); `if (a >= 0)` -> `if (label < p.C)` around the box term (the label == C box loses its L1
    term and gradient); `fmaxf(avg, 1)` dropped (avg 0 and 0.5); `if (s != s) s = 0` dropped (the NaN layer); `d > 0.f ? 1 : (d < 0.f
    ? -1 : 0)` -> `d >= 0.f ? 1 : -1` (the prediction == target columns).  NOT visible: `label > p.C` -> `>=` (both are background).
    Sums: loss_cases.check_loss_sums (SUM_RULES); gradients: loss_cases.elementwise against the gradient BEFORE nan_to_num - the
    documented deviation (include/gd4d.h): layers whose terms are finite equal torch's through nan_to_num bit for bit in float64, which is
    asserted on the restatement, so the deviation is confined to the replaced layers."""
    nb, q, nl, c, gt_dim, code, avg = case
    d = C.head_inputs(case, seed=4700 + nb * q)
    names = ('cls', 'box', 'assigned', 'gt_boxes', 'gt_labels', 'code_weights', 'avg_factors')
    args = {k: d[k] for k in names}
    kw = dict(alpha=d['alpha'], loss_cls_weight=d['loss_cls_weight'], loss_bbox_weight=d['loss_bbox_weight'])
    shapes = [(nl, 2), tuple(d['cls'].shape), tuple(d['box'].shape)]
    loss, gc, gb = _three_launches('head_loss_fwd_bwd', args, kw, ('cls', 'box', 'gt_boxes', 'code_weights', 'avg_factors'), shapes, nl,
                                   lambda a: _shift_last(a, ('cls', 'box')))
    pos = [d[k] for k in names]
    info = {}
    before = R.head_loss64(*pos, **kw, before_nan_to_num=True, info=info)
    before32 = R.head_loss64(*pos, **kw, before_nan_to_num=True, dtype=F32)
    through = R.head_loss64(*pos, **kw)
    rows = nb * q
    sweeps = -(-rows // 1024)
    kc = d['loss_cls_weight'] / max(avg[0], 1.0)
    C.check_loss_sums('head_loss loss_cls', loss[:, 0], before[0][:, 0], info['abs_cls'], sweeps * c, 24,
                          extra=[m * 6 * C.U * kc for m in info['matched']])
    C.check_loss_sums('head_loss loss_bbox', loss[:, 1], before[0][:, 1], info['abs_box'], sweeps * info['nk'], 8)
    _grad_rules('head', gc, gb, before, before32, info['nk'], code)
    replaced = (~torch.isfinite(torch.stack([torch.stack([d['cls'][l].sum(), d['box'][l].sum()]) for l in range(nl)])))
    for l in range(nl):
        for col, (g_b, g_t) in enumerate(((before[1], through[1]), (before[2], through[2]))):
            if not bool(replaced[l, col]):
                assert torch.equal(g_b[l], g_t[l])                           # finite layers: the deviation does not exist
    # matched rows whose prediction equals the target in some columns: exactly zero there (the restatement has them, so elementwise saw
    # them; here that the case really contains such entries)
    assert d['exact_rows'] > 0 or rows < 8
    tgt_zero = (before[2] == 0) & (torch.isfinite(d['box'])) & (d['assigned'].unsqueeze(-1) >= 0)
    assert torch.count_nonzero(gb[tgt_zero]).item() == 0


# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', C.DCOST_CASES, ids=lambda c: 'Qs%d-Qt%d-C%d-code%d-pseudo%d-NL%d' % c)
def test_distill_cost_tiles_batch0_labels_pseudo_gt_and_nonfinite(case):
    """Items 2, 4, 5, 6 and the batch-0 quirk of item 8 for gd4d_distill_match_cost_fwd.  Mutations this fails under: `t0row` -> `trow` in
    the soft labels (B = 2 with different teacher logits per sample); the `q0 + r < p.Qs` / `t0 + r < p.Qt` staging guards removed (NaN
    from beyond the embedded inputs is read but unused - NOT visible; the guard on the store, `t0 + t >= p.Qt`, is: the NaN guard
    flips); `nqt` computed from Qs (Qs != Qt); the k < 8 loops run to code; `cst == -INFINITY` compared the other way (+inf costs turn
    NaN); pseudo_gt's `* 9` stride -> 10.
    Bound: loss_cases.elementwise relative to max(|cost|, 1) per entry, k_ops = 24 + C + 8 (the class sum's own roundings)."""
    qs, qt, c, code, pseudo, nl = case
    d = C.dcost_inputs(case, seed=4800 + qs * 131 + qt)
    names = ('s_cls', 's_box', 't_cls', 't_box')
    args = {k: d[k] for k in names}
    kw = dict(cls_weight=d['cls_weight'], reg_weight=d['reg_weight'], pseudo_gt=d['pseudo_gt'])
    got, = _three_launches('distill_match_cost_fwd', args, kw, names, [(nl * 2 * qs * qt,)], nl,
                           lambda a: _shift_last(a, ('s_cls', 's_box')))
    pos = [d[k] for k in names]
    ref64 = R.distill_match_cost64(*pos, **kw)
    ref32 = R.distill_match_cost64(*pos, **kw, dtype=F32)
    scale = ref64.abs().clamp(min=1.0).nan_to_num(1.0, 1.0, 1.0)
    C.elementwise('distill_match_cost', got, ref64, ref32, C.K_OPS['distill_cost'] + c + 8, scale)
    if not pseudo and qt > 1:                                                # the quirk is visible: sample 1's own labels give other costs
        own = dict(zip(names, pos))
        own['t_cls'] = d['t_cls'].flip(1)
        other = R.distill_match_cost64(*[own[k] for k in names], **kw).view(nl, 2, -1)
        fin = torch.isfinite(other[:, 1]) & torch.isfinite(ref64.view(nl, 2, -1)[:, 1])
        assert float((other[:, 1][fin] - ref64.view(nl, 2, -1)[:, 1][fin]).abs().max()) > 1e-2


def test_distill_cost_refuses_65_classes():
    """C = 65 > DC_MAX_C: GD4D_EUNSUPPORTED (include/gd4d.h: C <= 64)."""
    from graph_detr4d_amd import _lib, ops
    z = lambda *s: torch.zeros(*s, device=DEV)                              # noqa: E731
    with pytest.raises(_lib.Gd4dError, match=r'code -2\b'):
        ops.distill_match_cost_fwd(z(1, 1, 2, 65), z(1, 1, 2, 10), z(1, 1, 2, 65), z(1, 1, 2, 10))


# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', C.DLOSS_CASES, ids=lambda c: 'B%d-Qs%d-Qt%d-NL%d-C%d-code%d-rw%d' % c)
def test_distill_loss_sweep_loops_rescale_pass_quirks_and_index_safety(case):
    """Items 1, 4, 5, 6, 7 and 8 for gd4d_distill_loss_fwd_bwd.  Mutations this fails under: either row loop dropped (1025, 2055 rows:
    unwritten gradients, or grad_box left unscaled by reg_weight / divisor); `10.0f` -> `(float)C` in the divisor rule (C = 12 under
    reweight: every unmatched row must add 12); the soft labels read from `trow` instead of batch 0 (B > 1); `t >= p.Qt` removed
    (assigned above the sample's range reads the next sample's teacher, or the NaN beyond it); `k < 10` -> `k < code` in the rescale
    pass or the L1 loop (code 16); the divisor clamped (`fmaxf(d_, 1)`: changes every reweighted loss and pins the div = 0 layer).
    Sums: loss_cases.check_loss_sums; gradients: loss_cases.elementwise against the gradient BEFORE nan_to_num (the documented
    deviation), except a layer whose reg divisor is 0: there grad_s_box[:, :10] is NaN in every row (include/gd4d.h), columns >= 10
    are 0, and the loss is 0."""
    nb, qs, qt, nl, c, code, rw = case
    d = C.dloss_inputs(case, seed=4900 + nb * qs + qt)
    names = ('s_cls', 's_box', 't_cls', 't_box', 'assigned', 'code_weights', 'avg_factors')
    args = {k: d[k] for k in names}
    kw = dict(reweight_score=d['reweight_score'], loss_cls_weight=d['loss_cls_weight'], loss_reg_weight=d['loss_reg_weight'])
    shapes = [(nl, 2), tuple(d['s_cls'].shape), tuple(d['s_box'].shape)]
    loss, gc, gb = _three_launches('distill_loss_fwd_bwd', args, kw, ('s_cls', 's_box', 't_cls', 't_box', 'code_weights', 'avg_factors'),
                                   shapes, nl, lambda a: _shift_last(a, ('s_cls', 's_box')))
    pos = [d[k] for k in names]
    info = {}
    before = R.distill_loss64(*pos, **kw, before_nan_to_num=True, info=info)
    before32 = R.distill_loss64(*pos, **kw, before_nan_to_num=True, dtype=F32)
    through = R.distill_loss64(*pos, **kw)
    rows = nb * qs
    sweeps = -(-rows // 1024)
    C.check_loss_sums('distill_loss cls', loss[:, 0], before[0][:, 0], info['abs_cls'], sweeps * c, 24)
    C.check_loss_sums('distill_loss reg', loss[:, 1], before[0][:, 1], info['abs_box'], sweeps * 10, 24 + (sweeps + 22 if rw else 0))
    zero_div = [l for l in range(nl) if rw and info['div'][l] == 0.0]
    if case == (3, 685, 100, 3, 10, 10, 1):
        assert zero_div == [1]                                               # reweight, C == 10, nothing matched: the unclamped divisor is 0
    if case == (1, 1025, 7, 3, 12, 10, 1):
        assert info['div'][1] == 1025 * 12 and not zero_div                  # "!= 10": with C = 12 every unmatched row adds 12
    gb_ref, gb_ref32, gb_got = before[2].clone(), before32[2].clone(), gb.clone()
    for l in zero_div:
        assert float(loss[l, 1]) == 0.0
        assert bool(torch.isnan(gb[l][..., :10]).all()) and torch.count_nonzero(_bits(gb[l][..., 10:])).item() == 0
        gb_ref[l], gb_ref32[l], gb_got[l] = 0.0, 0.0, 0.0
    _grad_rules('distill', gc, gb_got, (None, before[1], gb_ref), (None, before32[1], gb_ref32), 10, code,
                box_extra=sweeps + 22 if rw else 0)
    for l in range(nl):
        finite = bool(torch.isfinite(d['s_cls'][l]).all()), bool(torch.isfinite(d['s_box'][l]).all()) and l not in zero_div
        for col, ok in enumerate(finite):
            if ok:
                assert torch.equal(before[1 + col][l], through[1 + col][l])  # finite layers: the deviation does not exist
