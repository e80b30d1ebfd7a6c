"""The stepped-backward checker of tests/train_step.py has teeth: on the CPU, a stand-in "implementation" - the fp32 oracle's own
autograd through the six-layer loop, with its own decisions recorded - passes, and each planted mistake is flagged at exactly its
place and nowhere above it.  So a green tests/test_train_layers_gpu.py means every layer of the real training call passed the
right gradient on.  Also: the oracle's decision arguments (explicit-gather corners, ReLU masks, dropout keep masks) compute
what the oracle computes when they repeat its own decisions.

60 queries = 3 full row blocks of 16 and a partial block of 12, 6 cameras, 6 layers, bench.build_decoder."""
import copy

import pytest
import torch

import bench
import graph_detr4d_amd as G
from graph_detr4d_amd import synthetic
from oracle import torch_oracle as O

from train_step import (RELU_KINDS, compare, decisions_from_parts, mismatch_failures, stepped_backward)

NL, Q, N = 6, 60, 6
PARTIAL = slice(48, 60)                  # the partial row block


@pytest.fixture(scope='module')
def small():
    img_hw, levels = (128, 224), [(16, 28), (8, 14), (4, 7), (2, 4)]
    tr, regs = bench.build_decoder(G, N, NL, 'fp32', 1002)
    _, layer_params = bench.state_as_oracle_params(tr)
    sd = {k: v.detach() for k, v in tr.state_dict().items()}
    metas = synthetic.make_img_metas(synthetic.camera_rig(1, img_hw), img_shape=(*img_hw, 3), pad_shape=(*img_hw, 3))
    gen = torch.Generator().manual_seed(6)
    return dict(layer_params=layer_params, regs=list(regs), metas=metas, levels=levels, pc=synthetic.PC_RANGE,
                feats=synthetic.feature_pyramid(N, levels, seed=5), qe=torch.randn(Q, 512, generator=gen),
                probes=torch.randn(NL, Q, 1, 256, generator=gen), ref_probes=torch.randn(NL, 1, Q, 3, generator=gen),
                ref_params={'weight': sd['reference_points.weight'], 'bias': sd['reference_points.bias']})


def _dropout_sites(seed):
    """Five seeded keep masks per layer (p = 0.1), in fused_train's s.drop order."""
    g = torch.Generator().manual_seed(seed)
    keep = lambda *shape: torch.rand(*shape, generator=g) >= 0.1          # noqa: E731
    return [[(keep(1, 8, Q, Q), 0.1), (keep(Q, 256), 0.1), (keep(Q, 256), 0.1), (keep(Q, 512), 0.1), (keep(Q, 256), 0.1)]
            for _ in range(NL)]


def _stand_in(s, refine=True, mistake=None, dropout=None):
    """The fp32 oracle's autograd through the loop (O.decoder + O.transformer's reference-point head, written out), with one
    planted mistake.  Returns what an implementation returns: (states, init_ref, refs, grads, decisions)."""
    lp = [{k: v.clone().requires_grad_() for k, v in p.items()} for p in s['layer_params']]
    rp = {k: v.clone().requires_grad_() for k, v in s['ref_params'].items()}
    feats = [f.clone().requires_grad_() for f in s['feats']]
    regs = [copy.deepcopy(r) for r in s['regs']] if refine else None
    qe = s['qe'].clone().requires_grad_()
    qp, query = (t.unsqueeze(1) for t in torch.split(qe, 256, dim=1))
    init_ref = torch.sigmoid(torch.nn.functional.linear(qp.permute(1, 0, 2), rp['weight'], rp['bias']))
    x, ref = query, init_ref
    states, refs, decisions, grad_y3 = [], [], [], []
    for lid in range(NL):
        fl = feats
        if mistake == 'pyramid-camera' and lid == 4:
            fl = [torch.cat([f[:, :2], f[:, 2:3].detach(), f[:, 3:]], 1) for f in feats]     # camera 2 loses layer 4's part
        use_ref = init_ref.detach() if (mistake == 'ref0' and lid == 0) else ref
        drop = None if dropout is None else dropout[lid]
        y, parts = O.decoder_layer(lp[lid], x, fl, qp, use_ref, s['metas'], s['pc'], return_parts=True, dropout=drop)
        decisions.append(decisions_from_parts(parts, s['levels'], dropout=drop))
        if lid == 3:
            y.retain_grad()
            grad_y3.append(y)
        if regs is not None:
            ref = O.refine_points(regs[lid], y, ref)
        states.append(y)
        refs.append(ref)
        x = y.detach() if (mistake == 'no-upstream' and lid == 2) else y        # layer 2 sees G_2 = probe_2 only
    st, rf = torch.stack(states), torch.stack(refs)
    loss = (st * s['probes']).sum() + (init_ref ** 2).sum()
    if not refine:
        loss = loss + (rf * s['ref_probes']).sum()
    loss.backward()
    if mistake == 'partial-block':
        # layer 3's FFN weight gradient without the partial block's rows: the FFN is row-local, so the rows' share of that
        # gradient is the one of <y3[rows], G3[rows]> - subtract it
        g3 = grad_y3[0].grad
        w = lp[3]['ffns.0.layers.0.0.weight']
        p3 = dict(lp[3], **{'ffns.0.layers.0.0.weight': w.detach().clone().requires_grad_()})
        y3 = O.decoder_layer(p3, states[2].detach(), [f.detach() for f in feats], qp.detach(), refs[2].detach() if refine
                             else init_ref.detach(), s['metas'], s['pc'], dropout=None if dropout is None else dropout[3])
        share, = torch.autograd.grad((y3[PARTIAL] * g3[PARTIAL]).sum(), [p3['ffns.0.layers.0.0.weight']])
        with torch.no_grad():
            w.grad -= share
    grads = dict(layers=[{k: v.grad for k, v in p.items()} for p in lp], reference_points={k: v.grad for k, v in rp.items()},
                 query_embed=qe.grad, feats=[f.grad for f in feats],
                 regs=None if regs is None else [{k: v.grad for k, v in r.named_parameters()} for r in regs])
    return st.detach(), init_ref.detach(), rf.detach(), grads, decisions


def _check(s, refine=True, mistake=None, dropout=None, swap_relu=False):
    st, init_ref, rf, grads, decisions = _stand_in(s, refine, mistake, dropout)
    if swap_relu:
        decisions[1] = dict(decisions[1], relu=decisions[2]['relu'])       # layer 1 forced onto layer 2's ReLU units
    ref = stepped_backward(s['layer_params'], s['ref_params'], s['qe'], s['feats'], s['metas'], s['pc'], st, init_ref, rf,
                           decisions, s['probes'], regs=s['regs'] if refine else None,
                           ref_probes=None if refine else s['ref_probes'])
    rows, fails = compare(grads, ref)
    return rows, fails, ref


def _places(fails):
    return sorted({f[0] for f in fails})


@pytest.mark.parametrize('refine', [True, False], ids=['refine', 'no-refine'])
def test_unmodified_fp32_loop_fits_the_bounds(small, refine):
    rows, fails, ref = _check(small, refine)
    assert not fails, fails
    assert not mismatch_failures(ref['mismatch']), ref['mismatch']
    assert all(m['mask_rows'] == 0 for m in ref['mismatch']), ref['mismatch']
    worst = max(r[2] for r in rows)
    print(f'{"refine" if refine else "no-refine"}: worst relative Frobenius error {worst:.2e}')
    # every parameter of every layer was compared, and the reg branches' gradient is the oracle's: none (detached points)
    assert len([r for r in rows if r[0].startswith('layer ')]) == NL * len(small['layer_params'][0])
    if refine:
        assert all(g is None for r in ref['regs'] for g in r.values())


def test_dropout_sites_fit_the_bounds(small):
    rows, fails, ref = _check(small, True, dropout=_dropout_sites(7))
    assert not fails, fails
    assert not mismatch_failures(ref['mismatch']), ref['mismatch']


def test_missing_partial_block_rows_flagged_in_exactly_that_tensor(small):
    _, fails, _ = _check(small, mistake='partial-block')
    assert [(f[0], f[1]) for f in fails] == [('layer 3', 'ffns.0.layers.0.0.weight')], fails


def test_missing_upstream_term_flagged_at_layer_2_first(small):
    _, fails, _ = _check(small, mistake='no-upstream')
    places = _places(fails)
    assert 'layer 2' in places and not {'layer 3', 'layer 4', 'layer 5'} & set(places), places
    assert {'layer 0', 'layer 1'} <= set(places), places     # (the wrong gradient travels down)


def test_missing_camera_of_pyramid_gradient_flagged_at_that_camera(small):
    _, fails, _ = _check(small, mistake='pyramid-camera')
    assert all(f[0].startswith('pyramid level') for f in fails), fails
    cams = {f[1] for f in fails if f[1].startswith('camera')}
    assert cams == {'camera 2'}, fails


def test_dropped_reference_point_gradient_of_layer_0_flagged_at_reference_points(small):
    _, fails, _ = _check(small, mistake='ref0')
    places = _places(fails)
    assert 'reference_points' in places and not any(p.startswith('layer') or p.startswith('pyramid') for p in places), fails


def test_swapped_relu_masks_flagged_by_the_mismatch_report_at_layer_1(small):
    _, fails, ref = _check(small, swap_relu=True)
    bad = mismatch_failures(ref['mismatch'])
    assert list(bad) == [1], bad
    assert all(any(k in why for k in RELU_KINDS) for why in bad[1]), bad
    assert not {'layer 2', 'layer 3', 'layer 4', 'layer 5'} & set(_places(fails)), fails


def test_decision_arguments_repeating_the_oracle_change_nothing(small):
    """Forced decisions equal to the oracle's own: the explicit-gather corners, the ReLU masks and all-kept dropout sites
    (p = 0) reproduce the plain oracle layer (bit-identical apart from the gather's summation order)."""
    s = small
    d = torch.float64
    lp = {k: v.to(d) for k, v in s['layer_params'][0].items()}
    feats = [f.to(d) for f in s['feats']]
    qp, query = (t.unsqueeze(1).to(d) for t in torch.split(s['qe'], 256, dim=1))
    ref = torch.sigmoid(torch.nn.functional.linear(qp.permute(1, 0, 2), s['ref_params']['weight'].to(d),
                                                   s['ref_params']['bias'].to(d)))
    y0, parts = O.decoder_layer(lp, query, feats, qp, ref, s['metas'], s['pc'], return_parts=True)
    level_hw = s['levels']
    corners = torch.stack([torch.stack((torch.floor(parts['uv'][..., 0] * w - 0.5),
                                        torch.floor(parts['uv'][..., 1] * h - 0.5)), -1).long() for h, w in level_hw], dim=4)
    relu = {k: parts['pre_' + k] > 0 for k in RELU_KINDS}
    ones = lambda *shape: torch.ones(*shape, dtype=torch.bool)           # noqa: E731
    drop = [(ones(1, 8, Q, Q), 0.), (ones(Q, 256), 0.), (ones(Q, 256), 0.), (ones(Q, 512), 0.), (ones(Q, 256), 0.)]
    y1 = O.decoder_layer(lp, query, feats, qp, ref, s['metas'], s['pc'], vis_mask=parts['mask'], corners=corners,
                         relu_masks=relu, dropout=drop)
    assert (y1 - y0).abs().max().item() < 1e-12
    # one shifted corner changes the result: the corners are used
    c2 = corners.clone()
    vis = parts['mask'].nonzero()[0]
    c2[tuple(vis[:4].tolist()) + (0, vis[4].item(), 0)] += 1
    y2 = O.decoder_layer(lp, query, feats, qp, ref, s['metas'], s['pc'], vis_mask=parts['mask'], corners=c2)
    assert (y2 - y0).abs().max().item() > 1e-6
