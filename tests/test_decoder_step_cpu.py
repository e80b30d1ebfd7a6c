"""The stepping checker of tests/decoder_step.py has teeth: on the CPU, a stand-in "implementation" - the oracle's own decoder
loop with one deliberate cross-layer mistake - is flagged at exactly the layer that made it, and the unmodified oracle loop
passes with zero error.  So a green stepped check in tests/test_decoder_layers_gpu.py means every layer of the real call
consumed what the previous layer returned.  Also: the oracle's decoder path runs in fp64 on fp64 inputs."""
import copy

import pytest
import torch

import bench
import graph_detr4d_amd as G
from graph_detr4d_amd import synthetic
from oracle import torch_oracle as O

from decoder_step import refine, step_check, step_stats

NL = 6
IN_PROJ = ('attentions.0.attn.in_proj_weight', 'attentions.0.attn.in_proj_bias')


@pytest.fixture(scope='module')
def small():
    """60 queries x 6 cameras x 6 layers on 128 x 224 images: the bench's decoder (build_decoder) at a CPU size."""
    n, q = 6, 60
    img_hw, levels = (128, 224), [(16, 28), (8, 14), (4, 7), (2, 4)]
    tr, regs = bench.build_decoder(G, n, NL, 'fp32', 1002)
    _, layer_params = bench.state_as_oracle_params(tr)
    sd = {k: v.detach() for k, v in tr.state_dict().items()}
    metas = synthetic.make_img_metas(synthetic.camera_rig(1, img_hw), img_shape=(*img_hw, 3), pad_shape=(*img_hw, 3))
    feats = synthetic.feature_pyramid(n, levels, seed=5)
    qe = torch.randn(q, 512, generator=torch.Generator().manual_seed(6))
    query_pos, query = (t.unsqueeze(1).contiguous() for t in torch.split(qe, 256, dim=1))
    with torch.no_grad():
        ref0 = torch.nn.functional.linear(query_pos.permute(1, 0, 2), sd['reference_points.weight'],
                                          sd['reference_points.bias']).sigmoid()
    return dict(layer_params=layer_params, regs=list(regs), query=query, query_pos=query_pos, feats=feats, metas=metas,
                pc=synthetic.PC_RANGE, ref0=ref0, sd=sd, qe=qe)


def _stand_in(s, mistake=None):
    """The oracle's decoder loop (O.decoder) written out, with one cross-layer mistake.  Returns (states, refs, masks) as an
    implementation would."""
    x, ref = s['query'], s['ref0']
    states, refs, masks = [], [], []
    with torch.no_grad():
        for lid in range(NL):
            p, use_ref = s['layer_params'][lid], ref
            if mistake == 'stale-ref' and lid == 3:
                use_ref = refs[1]                     # the points from BEFORE layer 2's refinement
            if mistake == 'prev-in-proj' and lid == 4:
                p = dict(p, **{k: s['layer_params'][3][k] for k in IN_PROJ})       # layer 3's in-projection weights
            y, parts = O.decoder_layer(p, x, s['feats'], s['query_pos'], use_ref, s['metas'], s['pc'], return_parts=True)
            ref = refine(s['regs'][lid], y, use_ref)
            states.append(y)
            refs.append(ref)
            masks.append(parts['mask'].to(torch.uint8))
            x = y
    return torch.stack(states), torch.stack(refs), masks


def _stats(s, states, refs, masks):
    return step_stats(s['layer_params'], s['regs'], s['query'], s['query_pos'], s['feats'], s['metas'], s['pc'], states,
                      s['ref0'], refs, masks=masks)


def test_unmodified_oracle_loop_steps_with_zero_error(small):
    s = small
    with torch.no_grad():
        states, refs = O.decoder(s['layer_params'], s['query'], s['feats'], s['query_pos'], s['ref0'], s['metas'], s['pc'],
                                 reg_branches=s['regs'])
    _, _, masks = _stand_in(s)
    for m in (masks, None):
        stats = _stats(s, states, refs, m)
        assert all(t.ok and t[1:] == (0.0, 0.0, 0.0) for t in stats), stats
        assert m is None or all(t[0] == 0 for t in stats), stats
    # the written-out loop is the oracle's loop
    st2, refs2, _ = _stand_in(s)
    assert torch.equal(st2, states) and torch.equal(refs2, refs)
    step_check(s['layer_params'], s['regs'], s['query'], s['query_pos'], s['feats'], s['metas'], s['pc'], states, s['ref0'],
               refs, masks=masks, label='oracle loop')


@pytest.mark.parametrize('mistake, layer', [('stale-ref', 3), ('prev-in-proj', 4)])
@pytest.mark.parametrize('with_masks', [True, False])
def test_a_cross_layer_mistake_is_flagged_at_exactly_its_layer(small, mistake, layer, with_masks):
    """stale-ref: layer 3 samples around the reference points from before layer 2's refinement (and refines those);
    prev-in-proj: layer 4's self-attention runs on layer 3's in-projection weights.  with_masks=False: the exclusion rule of a
    route without a mask spy (rows near a visibility threshold in the oracle's own projection)."""
    s = small
    states, refs, masks = _stand_in(s, mistake)
    stats = _stats(s, states, refs, masks if with_masks else None)
    assert [lid for lid, t in enumerate(stats) if not t.ok] == [layer], stats
    assert all(t[1:] == (0.0, 0.0, 0.0) for lid, t in enumerate(stats) if lid != layer), stats
    with pytest.raises(AssertionError, match=f'stepped layers fail: {{{layer}:'):
        step_check(s['layer_params'], s['regs'], s['query'], s['query_pos'], s['feats'], s['metas'], s['pc'], states,
                   s['ref0'], refs, masks=masks if with_masks else None, label=mistake)


def test_oracle_decoder_runs_in_fp64_on_fp64_inputs(small):
    """The free-running yardstick (tools/freerun_parity.py) needs the oracle's decoder path in fp64: every intermediate
    follows the dtype of the parameters, features, queries and reference points (lidar2img takes the reference points' dtype)."""
    s = small
    d = torch.float64
    lp64 = [{k: v.to(d) for k, v in p.items()} for p in s['layer_params']]
    regs64 = [copy.deepcopy(r).to(d) for r in s['regs']]
    sd64 = {k: v.to(d) for k, v in s['sd'].items()}
    with torch.no_grad():
        st64, ref64, refs64 = O.transformer(sd64, lp64, [f.to(d) for f in s['feats']], s['qe'].to(d), s['metas'], s['pc'],
                                            reg_branches=regs64)
        y, parts = O.decoder_layer(lp64[0], s['query'].to(d), [f.to(d) for f in s['feats']], s['query_pos'].to(d),
                                   s['ref0'].to(d), s['metas'], s['pc'], return_parts=True)
        st32, _, refs32 = O.transformer(s['sd'], s['layer_params'], s['feats'], s['qe'], s['metas'], s['pc'],
                                        reg_branches=s['regs'])
    assert st64.dtype == ref64.dtype == refs64.dtype == d
    assert all(t.dtype == d for k, t in parts.items() if t.is_floating_point()), {k: t.dtype for k, t in parts.items()}
    assert st32.dtype == torch.float32
    # fp32 rounding only: the first layer agrees to fp32 accuracy
    assert (st32[0].double() - st64[0]).abs().max().item() < 1e-4
    assert (refs32[0].double() - refs64[0]).abs().max().item() < 1e-5
