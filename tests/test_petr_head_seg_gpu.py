"""PETRHeadseg on the GPU: gd4d_lane_mask_loss and gd4d_lane_map_fwd against the fp64 / integer restatement of
tests/petr_head_seg_ref.py (edge inputs, every code path, the memory contract of tests/guarded.py), the head's kernel route against the
fixture captured from the reference (tests/golden/petr_head_seg.npz) and against torch_ops=True, hip_train=True through loss(), and
loss() / get_lane_map themselves."""
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

import graph_detr4d_amd as G
from golden_io import Golden
from graph_detr4d_amd import ops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import petr_head_ref as P  # noqa: E402
import petr_head_seg_ref as S  # noqa: E402
from guarded import embedded, guarded  # noqa: E402
from oracle import torch_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
OUT_TOL = dict(rtol=1e-3, atol=1e-3)  # tests/test_petr_head_gpu.OUT_TOL
BWD_TOL = 1e-3                        # tests/test_petr_head_train_gpu.BWD_TOL: relative Frobenius per tensor
KEY_SIDE = ('input_proj.', 'position_encoder.', 'adapt_pos3d.', 'se.')
LANE_SIDE = ('lane_branches.', 'query_embedding_lane.', 'transformer_lane.')
ASSIGNER = dict(type='HungarianAssigner3D', cls_cost=dict(type='FocalLossCost', weight=2.0), reg_cost=dict(type='BBox3DL1Cost', weight=0.25),
                iou_cost=dict(type='IoUCost', weight=0.0), pc_range=P.PC_RANGE)


# ---- gd4d_lane_mask_loss ---------------------------------------------------------------------------------------------------
_LOSS_REF = {}


def _loss_reference(nl, r, c, lw):
    """(logits, targets, fp64 losses (L,), fp64 gradients (L, R, C), weights (R, C)); computed once per case."""
    key = (nl, r, c, lw)
    if key not in _LOSS_REF:
        x, t = S.loss_case(nl, r, c)
        per = [S.sigmoid_ce(x[l], t, lw) for l in range(nl)]
        _LOSS_REF[key] = (x, t, torch.stack([p[0] for p in per]), torch.stack([p[1] for p in per]), per[0][2])
    return _LOSS_REF[key]


def _lw(nl):
    return 1.0 if nl == 1 else 0.5


@pytest.mark.parametrize('nl,r,c', S.LOSS_SHAPES)
def test_lane_mask_loss_against_fp64(nl, r, c):
    """Loss within 2e-6 relative (terms good to a few ulp, the sum in fp64), every gradient within 1e-6 loss_weight w / (R C) absolute.
    C = 64 / 768 take the 16-byte path, 1 / 63 / 65 the 4-byte one; 9 x 768 spans two workgroups per layer."""
    lw = _lw(nl)
    x, t, want, want_grad, w = _loss_reference(nl, r, c, lw)
    loss, grad = ops.lane_mask_loss(x.to(DEV), t.to(DEV), lw)
    assert tuple(loss.shape) == (nl,) and tuple(grad.shape) == (nl, r, c)
    err = (loss.double().cpu() - want).abs()
    excess = float(((grad.double().cpu() - want_grad).abs() - 1e-6 * lw * w / (r * c)).max())
    print(f'L {nl}, {r} x {c}: loss {[round(float(v), 6) for v in want]}, max relative error '
          f'{float((err / want.abs().clamp(min=1e-300)).max()):.1e}; gradient error minus its bound, max: {excess:.1e}')
    assert bool((err <= 2e-6 * want.abs()).all())
    assert excess <= 0


@pytest.mark.parametrize('r,c', [(4, 64), (4, 65)])
def test_a_nan_layer_is_zeroed_and_the_other_layers_keep_their_bits(r, c):
    x, t, _, _, _ = _loss_reference(6, r, c, 0.5)
    x, t = x.to(DEV), t.to(DEV)
    loss, grad = ops.lane_mask_loss(x, t, 0.5)
    again, grad_again = ops.lane_mask_loss(x, t, 0.5)
    assert torch.equal(loss, again) and torch.equal(grad, grad_again)     # two runs: the same bits
    bad = x.clone()
    bad[2, r - 1, c // 2] = float('nan')
    loss_b, grad_b = ops.lane_mask_loss(bad, t, 0.5)
    keep = [l for l in range(6) if l != 2]
    assert float(loss_b[2]) == 0.0 and bool((grad_b[2] == 0).all())
    assert torch.equal(loss_b[keep], loss[keep]) and torch.equal(grad_b[keep], grad[keep])
    # a loss that overflows fp32 (the mean is above 1.01, the weight 3.4e38): nan_to_num's largest float, and a zero gradient as well
    loss_i, grad_i = ops.lane_mask_loss(x[:1].contiguous(), t, 3.4e38)
    assert float(loss[0]) * 2 > 1.01 and float(loss_i[0]) == torch.finfo(torch.float32).max and bool((grad_i == 0).all())


@pytest.mark.parametrize('nl,r,c', [(6, 9, 768), (6, 4, 65), (1, 1, 1), (6, 9, 63)])
def test_contract_lane_mask_loss(nl, r, c):
    """Outputs and workspace inside guarded buffers, inputs inside NaNs: pads intact, every output written and finite, and the same
    bits as the plain call."""
    lw = _lw(nl)
    x, t, _, _, _ = _loss_reference(nl, r, c, lw)
    plain = ops.lane_mask_loss(x.to(DEV), t.to(DEV), lw)
    loss, ok_loss = guarded((nl,), device=DEV)
    grad, ok_grad = guarded((nl, r, c), device=DEV)
    need = int(ops._lib.load().gd4d_lane_mask_loss_workspace_bytes(nl, r, c))
    ws, ok_ws = guarded((need,), dtype=torch.uint8, device=DEV)
    got = ops.lane_mask_loss(embedded(x.to(DEV)), embedded(t.to(DEV)), lw, outs=(loss, grad), workspace=ws)
    assert got[0] is loss and got[1] is grad
    assert ok_loss() and ok_grad() and ok_ws()
    assert ok_loss.unwritten() == 0 and ok_grad.unwritten() == 0
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(grad).all())
    assert torch.equal(loss, plain[0]) and torch.equal(grad, plain[1])
    with pytest.raises(ValueError, match='workspace'):
        ops.lane_mask_loss(x.to(DEV), t.to(DEV), lw, workspace=ws[:need - 16])


def test_lane_mask_loss_autograd_node():
    """LaneMaskLossFunction: dlogits[l] scaled by the incoming gradient of loss[l], nothing for the targets, one backward only; the
    Sigmoid_ce_loss module is the node with one layer."""
    x, t, want, want_grad, _ = _loss_reference(6, 4, 65, 0.5)
    logits = x.to(DEV).requires_grad_(True)
    targets = t.to(DEV).requires_grad_(True)
    crit = G.Sigmoid_ce_loss(loss_weight=0.5)
    loss = crit.layers(logits, targets)
    coef = torch.arange(1, 7, device=DEV, dtype=torch.float32) / 4
    (loss * coef).sum().backward(retain_graph=True)
    assert targets.grad is None
    torch.testing.assert_close(logits.grad.double().cpu(), want_grad * coef.double().cpu().view(-1, 1, 1), rtol=1e-5, atol=1e-9)
    with pytest.raises(RuntimeError, match='consumed by the first backward'):
        (loss * coef).sum().backward()
    single = crit(x[3].to(DEV), t.to(DEV))
    assert single.dim() == 0 and torch.equal(single, loss[3].detach())
    crit.torch_ops = True                                                  # the reference's four lines on the same tensors
    torch.testing.assert_close(crit(x[3].to(DEV), t.to(DEV)).double().cpu(), want[3], rtol=2e-6, atol=0)


# ---- gd4d_lane_map_fwd -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('g', S.MAP_GRIDS)
def test_lane_map_against_the_restatement(g):
    b = 1 if g == 16 else 2
    x, gt = S.map_case(b, g)
    prob64, binary, sums, iou = S.lane_map(x, gt)
    got = ops.lane_map_fwd(x.to(DEV), gt.to(DEV))
    assert [tuple(t.shape) for t in got] == [(b, 3, 16 * g, 16 * g)] * 2 + [(b, 3, 3), (b, 3)]
    err = float((got[0].double().cpu() - prob64).abs().max())
    print(f'g {g}: max |prob - fp64| = {err:.1e}; sums {sums[0].tolist()}')
    assert torch.equal(got[1].cpu().long(), binary)
    assert torch.equal(got[2].cpu().double(), sums.double())              # integers: exact
    assert err < 2e-7
    torch.testing.assert_close(got[3].double().cpu(), iou, rtol=1e-6, atol=0)
    # query 0's first three elements land at [class 0, row 0, columns 0, 1, 2]: - 2^-30 -> 1, - 2^-10 -> 0, exact 0 -> 1
    assert got[1][0, 0, 0, :3].tolist() == [1.0, 0.0, 1.0] and float(got[0][0, 0, 0, 0]) == 0.5
    bare = ops.lane_map_fwd(x.to(DEV))                                     # without a ground truth: g workgroups per plane
    assert len(bare) == 2 and torch.equal(bare[0], got[0]) and torch.equal(bare[1], got[1])


def test_lane_map_iou_of_two_empty_maps_is_one():
    x = torch.full((1, 4, 768), -1.0, device=DEV)
    _, binary, sums, iou = ops.lane_map_fwd(x, torch.zeros(1, 3, 32, 32, device=DEV))
    assert not bool(binary.any()) and not bool(sums.any()) and iou.tolist() == [[1.0, 1.0, 1.0]]


@pytest.mark.parametrize('g,with_gt', [(3, True), (3, False), (1, True)])
def test_contract_lane_map(g, with_gt):
    x, gt = S.map_case(2, g)
    shape = (2, 3, 16 * g, 16 * g)
    bufs = [guarded(shape, device=DEV), guarded(shape, device=DEV)] + ([guarded((2, 3, 3), device=DEV), guarded((2, 3), device=DEV)] if with_gt else [])
    got = ops.lane_map_fwd(embedded(x.to(DEV)), embedded(gt.to(DEV)) if with_gt else None, outs=[v for v, _ in bufs])
    plain = ops.lane_map_fwd(x.to(DEV), gt.to(DEV) if with_gt else None)
    for (view, ok), a, b in zip(bufs, got, plain):
        assert a is view and ok() and ok.unwritten() == 0 and bool(torch.isfinite(view).all()) and torch.equal(view, b)


# ---- the head ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def golden():
    return Golden('petr_head_seg')


def _state(g):
    keys = json.loads(bytes(g.arrays['keys']).decode())
    shapes = json.loads(bytes(g.arrays['shapes']).decode())
    return S.state_dict(keys, shapes)


def _metas(g):
    return P.img_metas(g.arrays['lidar2img'].astype(np.float64), g.arrays['timestamps'])


def _feat():
    return P.features(S.head_config()['in_channels'])


def _head(g, **kw):
    head = G.build_head(S.head_config(**kw))
    head.load_state_dict(_state(g), strict=True)
    return head.to(DEV).eval()


@pytest.fixture(scope='module')
def head(golden):
    return _head(golden)


@pytest.fixture(scope='module')
def kernel_outputs(golden, head):
    """One kernel-route call with the rows handed to each decoder's forward_keys recorded; shared by the tests below."""
    seen = {}

    def spy(tag, real):
        def call(keys, key_pos, mask, query_embed, reg_branch=None):
            seen[tag] = dict(keys=keys.clone(), key_pos=key_pos.clone(), mask=mask.clone(), query_embeds=query_embed.clone(),
                             ptrs=(keys.data_ptr(), key_pos.data_ptr()))
            return real(keys, key_pos, mask, query_embed, reg_branch)
        return call
    head.transformer.forward_keys = spy('det', head.transformer.forward_keys)
    head.transformer_lane.forward_keys = spy('lane', head.transformer_lane.forward_keys)
    try:
        with torch.no_grad():
            outs = head([_feat().to(DEV)], _metas(golden))
    finally:
        del head.transformer.forward_keys, head.transformer_lane.forward_keys
    return outs, seen


def test_head_key_rows_match_the_reference(golden, kernel_outputs):
    g, (_, seen) = golden, kernel_outputs
    flat = lambda t: t.permute(1, 3, 4, 0, 2).reshape(-1, t.shape[0], 256)      # noqa: E731
    assert seen['det']['ptrs'] == seen['lane']['ptrs']                       # ONE key side: both decoders read the same rows
    det = seen['det']
    torch.testing.assert_close(det['keys'].cpu(), flat(g.t('x@512').float().div(512)), rtol=2e-4, atol=2e-4)
    assert torch.equal(det['mask'].cpu(), g.t('mask').reshape(2, -1)) and torch.equal(seen['lane']['mask'], det['mask'])
    torch.testing.assert_close(det['query_embeds'].cpu(), g.t('query_embeds'), rtol=2e-4, atol=2e-4)
    torch.testing.assert_close(seen['lane']['query_embeds'].cpu(), g.t('query_embeds_lane'), rtol=2e-4, atol=2e-4)
    ref = flat(g.t('pos_embed'))
    d = (det['key_pos'].cpu() - ref).abs()
    print(f'max |key_pos - reference| = {float(d.max()):.2e}, share above 1e-2: {float((d > 1e-2).float().mean()):.2e}')
    assert float(d[ref.abs() < 8].max()) < 2e-4                            # the rule of tests/test_head_pe_gpu.py:44-45
    assert float((d > 1e-2).float().mean()) < 1e-3


def test_head_outputs_match_the_reference(golden, kernel_outputs):
    outs, _ = kernel_outputs
    assert list(outs) == ['all_cls_scores', 'all_bbox_preds', 'all_lane_preds', 'enc_cls_scores', 'enc_bbox_preds']
    assert outs['enc_cls_scores'] is None and outs['enc_bbox_preds'] is None
    assert tuple(outs['all_lane_preds'].shape) == (P.LAYERS, P.BS, S.NUM_LANE, 768)
    for name in ('all_cls_scores', 'all_bbox_preds', 'all_lane_preds'):
        want = golden.t(name)
        print(f'{name}: max |kernel route - reference| = {float((outs[name].cpu() - want).abs().max()):.2e}')
        torch.testing.assert_close(outs[name].cpu(), want, **OUT_TOL)


def test_kernel_route_matches_torch_ops_with_one_key_launch(golden, head, kernel_outputs, monkeypatch):
    feat, metas = [_feat().to(DEV)], _metas(golden)
    head.torch_ops = True
    try:
        with torch.no_grad():
            want = head(feat, metas)
    finally:
        head.torch_ops = False
    for name in ('all_cls_scores', 'all_bbox_preds', 'all_lane_preds'):
        torch.testing.assert_close(want[name].cpu(), golden.t(name), **OUT_TOL)                 # torch: the reference's op sequence
        torch.testing.assert_close(kernel_outputs[0][name], want[name], **OUT_TOL)
    calls = []
    real = ops.petr_keys_fwd
    monkeypatch.setattr(ops, 'petr_keys_fwd', lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    with torch.no_grad():
        again = head(feat, metas)
    assert len(calls) == 1                                                   # exactly one key-side launch per forward
    assert all(torch.equal(again[k], kernel_outputs[0][k]) for k in ('all_cls_scores', 'all_bbox_preds', 'all_lane_preds'))


def test_kept_lane_embedding_follows_its_parameters(golden, head):
    feat, metas = [_feat().to(DEV)], _metas(golden)
    with torch.no_grad():
        first = head(feat, metas)
        p = head.query_embedding_lane[2].bias
        p.add_(0.25)
        changed = head(feat, metas)
        # (a stale kept value would give the first result bit for bit; 1e-5 is far above the fp32 rounding of logits below 1)
        assert float((changed['all_lane_preds'] - first['all_lane_preds']).abs().max()) > 1e-5, 'the kept lane embedding outlived its parameter'
        assert torch.equal(changed['all_cls_scores'], first['all_cls_scores'])              # the detection half does not read it
        p.sub_(0.25)
        assert torch.equal(head(feat, metas)['all_lane_preds'], first['all_lane_preds'])


# ---- loss() and get_lane_map ---------------------------------------------------------------------------------------------------
def _ground_truth(device, dtype=torch.float32):
    boxes = torch.tensor([[10.0, 5.0, -1.0, 4.0, 2.0, 1.5, 0.3, 1.0, 0.5], [-20.0, 12.0, 0.5, 1.0, 0.75, 1.75, -1.2, 0.0, 0.25],
                          [3.0, -30.0, -2.0, 10.0, 2.5, 3.0, 2.0, -2.0, 1.0]], dtype=dtype, device=device)
    return [boxes], [torch.tensor([1, 4, 7], device=device)]


def _lane_target():
    return S.loss_case(1, S.NUM_LANE, 768)[1]


def test_loss_keys_and_lane_terms(golden):
    head = _head(golden, train_cfg=dict(assigner=ASSIGNER))
    with torch.no_grad():
        outs = head([_feat()[:1].to(DEV)], _metas(golden)[:1])
        boxes, labels = _ground_truth(DEV)
        target = _lane_target().to(DEV)
        losses = head.loss(boxes, labels, outs, [target])
        assert list(losses) == ['loss_cls', 'loss_bbox', 'loss_mask', 'd0.loss_cls', 'd0.loss_bbox', 'd0.loss_mask']
        assert all(v.dim() == 0 and bool(torch.isfinite(v)) for v in losses.values())
        lanes = outs['all_lane_preds']
        singles = [head.loss_lane_mask(lanes[l, 0], target) for l in range(P.LAYERS)]
        assert torch.equal(losses['d0.loss_mask'], singles[0]) and torch.equal(losses['loss_mask'], singles[1])
        want = S.sigmoid_ce(lanes[1, 0].cpu(), target.cpu(), S.LOSS_WEIGHT)[0]
        assert abs(float(losses['loss_mask']) - float(want)) <= 2e-6 * float(want)
        det = head.criterion().loss(boxes, labels, outs)
        assert torch.equal(det['loss_cls'], losses['loss_cls']) and torch.equal(det['d0.loss_bbox'], losses['d0.loss_bbox'])
        with pytest.raises(G._lib.Gd4dError, match='batch size 1 only'):
            head.loss(boxes * 2, labels * 2, head([_feat().to(DEV)], _metas(golden)), [target, target])


def test_get_lane_map_equals_the_restatement(golden, head, kernel_outputs):
    outs, _ = kernel_outputs
    logits = outs['all_lane_preds'][-1].cpu()
    gt = S.map_case(P.BS, 2)[1]
    _, binary, _, iou = S.lane_map(logits, gt)
    got, got_iou = head.get_lane_map(outs, gt.to(DEV))
    assert tuple(got.shape) == (P.BS, 3, 32, 32) and torch.equal(got.cpu().long(), binary)
    torch.testing.assert_close(got_iou.double().cpu(), iou, rtol=1e-6, atol=0)
    assert head.get_lane_map(outs)[1] is None and torch.equal(head.get_lane_map(outs)[0], got)
    head.torch_ops = True                                                  # the reference's op sequence
    try:
        ref, ref_iou = head.get_lane_map(outs, gt.to(DEV))
    finally:
        head.torch_ops = False
    assert torch.equal(ref, got)
    torch.testing.assert_close(ref_iou, got_iou, rtol=1e-6, atol=0)


# ---- hip_train=True --------------------------------------------------------------------------------------------------------------
def _coef(key, i):
    return 1.0 + 0.5 * i if key.endswith('loss_mask') else 1.0


def _scalar(losses):
    """The scalar of the gradient tests: every term of loss()'s dict, the lane terms with a coefficient per layer."""
    return sum(_coef(k, i) * losses[k] for i, k in enumerate(sorted(losses)))


def _step(head, g):
    """One forward + loss() + backward at batch 1: (outputs, loss dict, {parameter name or 'feat': gradient}, assignment)."""
    feat = _feat()[:1].to(DEV).requires_grad_(True)
    outs = head([feat], _metas(g)[:1])
    boxes, labels = _ground_truth(DEV)
    losses = head.loss(boxes, labels, outs, [_lane_target().to(DEV)])
    _scalar(losses).backward()
    grads = {k: p.grad for k, p in head.named_parameters() if p.grad is not None}
    grads['feat'] = feat.grad
    detached = {k: v.detach() for k, v in outs.items() if v is not None}
    return detached, {k: v.detach() for k, v in losses.items()}, grads, head.criterion().last_assigned.clone()


@pytest.fixture(scope='module')
def steps(golden):
    """hip_train=True and torch_ops=True, one step each, and the fp64 restatement's gradients; computed once."""
    cfg = dict(train_cfg=dict(assigner=ASSIGNER))
    hip = _step(_head(golden, hip_train=True, **cfg), golden)
    ref = _step(_head(golden, torch_ops=True, **cfg), golden)
    sd = {k: v.double().requires_grad_(k != 'code_weights') for k, v in _state(golden).items()}
    feat = _feat()[:1].double().requires_grad_(True)
    o64 = S.head_forward(sd, S.head_config(), feat, _metas(golden)[:1])
    boxes, labels = _ground_truth('cpu', torch.float64)
    l64, assigned = O.head_loss(o64['all_cls_scores'], o64['all_bbox_preds'], boxes, labels, sd['code_weights'])
    target = _lane_target()
    nl = o64['all_lane_preds'].shape[0]
    for l in range(nl):
        l64['loss_mask' if l == nl - 1 else f'd{l}.loss_mask'] = S.sigmoid_ce(o64['all_lane_preds'][l, 0], target, S.LOSS_WEIGHT)[0]
    _scalar(l64).backward()
    g64 = {k: v.grad for k, v in sd.items() if v.grad is not None}
    # the restatement reads `X_branches.N.*` per level from separate leaves; the module has ONE object under the six names, whose
    # gradient - listed under N = 0 - is the sum over the levels
    for k in [k for k in g64 if re.match(r'(cls|reg|lane)_branches\.0\.', k)]:
        stem, rest = k.split('.0.', 1)
        g64[k] = sum(g64[f'{stem}.{n}.{rest}'] for n in range(6) if f'{stem}.{n}.{rest}' in g64)
    g64['feat'] = feat.grad
    return dict(hip=hip, ref=ref, g64=g64, l64={k: v.detach() for k, v in l64.items()},
                assigned64=torch.stack([a[0] for a in assigned]) - 1)


def _fro(got, ref):
    ref = ref.double().cpu()
    den = float(ref.norm())
    num = float((got.double().cpu() - ref).norm())
    return num / den if den > 0 else num


def _norm(t):
    return float(t.double().norm())


def test_head_gradients_match_torch_ops_and_fp64(steps):
    """The rule of tests/test_petr_head_train_gpu.py::test_head_gradients_match_torch_ops_and_fp64 on the scalar made of loss()'s dict
    at batch 1: per tensor, relative Frobenius <= BWD_TOL against torch_ops=True - every parameter and feat - and against the fp64
    restatement - the key side (input_proj receives both decoders' gradients), feat, lane_branches, query_embedding_lane and
    transformer_lane.  The gradients that are zero identically (read from the fp64 restatement alone: a norm below 1e-9 of the largest)
    are held to BWD_TOL of the largest gradient norm among the same module's other parameters, and the set is asserted by name:
    adapt_pos3d's last bias (a shift of every key's encoding, cancelled by both softmaxes) and layer 0's self-attention in-projection
    weight of BOTH decoders (a zero query).  All three routes must have matched the same queries."""
    (o_hip, l_hip, g_hip, a_hip), (o_ref, l_ref, g_ref, a_ref), g64 = steps['hip'], steps['ref'], steps['g64']
    assert torch.equal(a_hip, a_ref) and torch.equal(a_hip[:, 0].cpu().long(), steps['assigned64'])
    for k in o_hip:
        print(f'{k}: max |hip_train - torch_ops| = {float((o_hip[k] - o_ref[k]).abs().max()):.2e}')
        torch.testing.assert_close(o_hip[k], o_ref[k], **OUT_TOL)
    assert list(l_hip) == list(l_ref) and sorted(l_hip) == sorted(steps['l64'])
    for k in l_hip:
        print(f'{k}: hip_train {float(l_hip[k]):.6f}, torch_ops {float(l_ref[k]):.6f}, fp64 {float(steps["l64"][k]):.6f}')
        torch.testing.assert_close(l_hip[k], l_ref[k], **OUT_TOL)
        torch.testing.assert_close(l_hip[k].double().cpu(), steps['l64'][k], **OUT_TOL)
    assert sorted(g_hip) == sorted(g_ref)                                   # every parameter that trains on one route trains on the other
    top64 = max(_norm(v) for v in g64.values())
    zero = sorted(k for k in g_ref if k in g64 and _norm(g64[k]) <= 1e-9 * top64)
    errs = {k: _fro(g_hip[k], g_ref[k]) for k in g_ref if k not in zero}
    e64 = {k: _fro(g_hip[k], g64[k]) for k in errs if k in g64 and (k.startswith(KEY_SIDE + LANE_SIDE) or k == 'feat')}
    t64 = {k: _fro(g_ref[k], g64[k]) for k in e64}
    print(f'{"tensor":60s} {"vs torch_ops":>12s} {"vs fp64":>10s} {"torch/fp64":>10s}')
    for k in sorted(errs):
        print(f'{k:60s} {errs[k]:12.2e} ' + (f'{e64[k]:10.2e} {t64[k]:10.2e}' if k in e64 else ''))
    assert all(bool(torch.isfinite(v).all()) for v in g_hip.values())
    for prefix in KEY_SIDE + LANE_SIDE:
        assert any(k.startswith(prefix) for k in e64), prefix
    assert 'lane_branches.0.4.weight' in errs and 'input_proj.weight' in e64 and 'feat' in e64
    late = {k: v for k, v in errs.items() if v > BWD_TOL}
    assert not late, late
    late = {k: v for k, v in e64.items() if v > BWD_TOL}
    assert not late, late
    layer0 = 'decoder.layers.0.attentions.0.attn.in_proj_weight'
    assert zero == sorted(['adapt_pos3d.2.bias', 'transformer.' + layer0, 'transformer_lane.' + layer0]), zero      # these, no others
    for k in zero:
        module = k.rsplit('.', 1)[0] + '.'
        scale = max(_norm(g_ref[j]) for j in g_ref if j.startswith(module) and j.count('.') == k.count('.') and j not in zero)
        print(f'{k}: |hip_train| {_norm(g_hip[k]):.2e}, |torch_ops| {_norm(g_ref[k]):.2e}, the module\'s other gradients {scale:.2e}')
        assert _norm(g_hip[k]) <= BWD_TOL * scale, k


def test_train_mode_is_deterministic_under_a_seed(golden):
    head = _head(golden, hip_train=True, train_cfg=dict(assigner=ASSIGNER)).train()          # default dropout
    runs = []
    for _ in range(2):
        head.zero_grad(set_to_none=True)
        torch.manual_seed(7)
        runs.append(_step(head, golden))
    (o1, l1, g1, _), (o2, l2, g2, _) = runs
    assert all(torch.equal(o1[k], o2[k]) and bool(torch.isfinite(o1[k]).all()) for k in o1)
    assert all(torch.equal(l1[k], l2[k]) for k in l1)
    assert sorted(g1) == sorted(g2)
    assert all(torch.equal(g1[k], g2[k]) and bool(torch.isfinite(g1[k]).all()) for k in g1)


def test_eval_without_autograd_takes_the_inference_route_unchanged(golden, kernel_outputs):
    head = _head(golden, hip_train=True)
    with torch.no_grad():
        outs = head([_feat().to(DEV)], _metas(golden))
    for k in ('all_cls_scores', 'all_bbox_preds', 'all_lane_preds'):
        assert torch.equal(outs[k], kernel_outputs[0][k]), k
    assert 'query_embeds_lane' in head._kept                               # the inference route's kept value was used
    from graph_detr4d_amd.petr_transformer import PETRMultiheadAttention
    for decoder in (head.transformer, head.transformer_lane):              # both transformers were told
        flagged = [m for m in decoder.modules() if isinstance(m, PETRMultiheadAttention)]
        assert len(flagged) >= P.LAYERS and all(m.hip_train for m in flagged)
    assert all(m.hip_train for m in head.modules() if type(m).__name__ == 'RegLayer')


def test_with_detach_cuts_the_past_frames_off(golden):
    """with_detach: cameras 6: of the feature map get no gradient under autograd and nothing changes without it.  The fixture has two
    cameras, so here every camera is a current one: the cut lies past the end and the gradients are those without the switch."""
    head = _head(golden, hip_train=True, with_detach=True)
    feat = _feat()[:1].to(DEV).requires_grad_(True)
    cut = head._past_frames_detached(torch.cat([feat] * 4, 1))             # eight cameras: 0 - 5 current, 6 - 7 past
    (cut * 1.0).sum().backward()
    assert bool((feat.grad == 3.0).all())                                  # copies 0 - 2 in full (6 cameras); copy 3 is the past pair
    with torch.no_grad():
        assert head._past_frames_detached(feat) is feat
