"""PETRHead / PETRv2Head on the GPU: ops.petr_keys_fwd alone (memory bit-equal to the permuted x; key_pos against fp64 MLPs over the
inputs ops.frustum_pe_input_fwd writes, 2e-4 - the bound tests/test_head_pe_gpu.py holds this MLP to), both heads against the fixture
captured from the reference (tests/golden/petr_head.npz), the kernel route against torch_ops=True, and the call checks."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import graph_detr4d_amd as G
from golden_io import Golden
from graph_detr4d_amd import ops, synthetic
from graph_detr4d_amd.petr_transformer import PETRTransformer

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import petr_head_ref as P  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
OUT_TOL = dict(rtol=1e-3, atol=1e-3)          # the two-layer out_dec bound of tests/test_petr_transformer_gpu.py; row-local layers behind it


@pytest.fixture(scope='module')
def golden():
    return Golden('petr_head')


def _state(g, kind):
    keys = json.loads(bytes(g.arrays[kind + '.keys']).decode())
    shapes = json.loads(bytes(g.arrays[kind + '.shapes']).decode())
    return P.state_dict(keys, shapes, shared=kind == 'v1')


def _metas(g, kind):
    ts = g.arrays[kind + '.timestamps'] if g.has(kind + '.timestamps') else None
    return P.img_metas(g.arrays[kind + '.lidar2img'].astype(np.float64), ts)


@pytest.fixture(scope='module')
def heads(golden):
    """Both heads with the fixture's parameters, on the GPU in eval mode; built once."""
    out = {}
    for kind in ('v1', 'v2'):
        head = G.build_head(P.head_config(kind))
        head.load_state_dict(_state(golden, kind), strict=True)
        out[kind] = head.to(DEV).eval()
    return out


# ---- the launch alone ----------------------------------------------------------------------------------------------------
def _grid(shape, seed, k, scale):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-k, k + 1, shape, generator=g).float() / scale


@pytest.fixture(scope='module')
def mlps():
    """position_encoder and fpe weights on a grid, their images, and fp64 copies; shared by the cases."""
    w = dict(pe0=_grid((1024, 192), 1, 3, 64), pe0b=_grid((1024,), 2, 3, 64), pe2=_grid((256, 1024), 3, 3, 64), pe2b=_grid((256,), 4, 3, 64),
             cr=_grid((256, 256), 5, 3, 64), crb=_grid((256,), 6, 3, 64), ce=_grid((256, 256), 7, 3, 64), ceb=_grid((256,), 8, 3, 64))
    d = {k: v.to(DEV) for k, v in w.items()}
    return dict(w=w, d=d, pe_image=ops.mlp2_frustum_image(d['pe0'], d['pe0b'], d['pe2']), se_image=ops.mlp2_image(d['cr'], d['crb'], d['ce']))


@pytest.mark.parametrize('gate', [True, False])
@pytest.mark.parametrize('bs,n,h,w', [(1, 3, 5, 7), (2, 3, 5, 7), (2, 2, 6, 10), (1, 2, 6, 10)])
def test_petr_keys_fwd_alone(mlps, bs, n, h, w, gate):
    """105 keys per sample at 3 x 5 x 7: not a multiple of the 128-pixel tile nor of the core's 32-key step; bs = 2 interleaves the
    rows.  The outputs start NaN-filled: every row must be written."""
    r, s = bs * n, h * w
    pad_hw = (16 * h, 16 * w)
    l2i = np.asarray(synthetic.camera_rig(num_frames=1, img_hw=pad_hw), dtype=np.float64)[:r]
    i2l = torch.from_numpy(np.linalg.inv(l2i)).float().to(DEV)
    x = _grid((bs, n, 256, h, w), 11, 16, 8).to(DEV)
    sine = _grid((r, s, 256), 12, 16, 8).to(DEV)
    memory = torch.full((n * s, bs, 256), float('nan'), device=DEV)
    key_pos = torch.full((n * s, bs, 256), float('nan'), device=DEV)
    d = mlps['d']
    got = ops.petr_keys_fwd(x, i2l, pad_hw, 64, 1, P.POSITION_RANGE, mlps['pe_image'], d['pe2b'], sine,
                            mlps['se_image'] if gate else None, d['ceb'] if gate else None, memory=memory, key_pos=key_pos)
    assert got[0] is memory and got[1] is key_pos
    assert torch.equal(memory, PETRTransformer._camera_pixels_first(x))                                    # a bit copy
    fr, _ = ops.frustum_pe_input_fwd(i2l, (h, w), pad_hw, 64, 1, P.POSITION_RANGE)                       # (R, 192, H, W): pinned to the reference
    w64 = {k: v.double() for k, v in mlps['w'].items()}
    rows = lambda t: t.double().cpu().flatten(2).transpose(1, 2)                                          # noqa: E731  (R, S, C)
    pe = torch.relu(rows(fr) @ w64['pe0'].t() + w64['pe0b']) @ w64['pe2'].t() + w64['pe2b']
    if gate:
        logits = torch.relu(rows(x.flatten(0, 1)) @ w64['cr'].t() + w64['crb']) @ w64['ce'].t() + w64['ceb']
        pe = pe * torch.sigmoid(logits)
    want = (pe + sine.double().cpu()).view(bs, n, s, 256).permute(1, 2, 0, 3).reshape(n * s, bs, 256)
    err = float((key_pos.double().cpu() - want).abs().max())
    print(f'bs {bs}, {n} cameras of {h} x {w}, gate {gate}: max |key_pos - fp64| = {err:.2e} (values up to {float(want.abs().max()):.1f})')
    assert not torch.isnan(key_pos).any() and err < 2e-4


def test_petr_keys_fwd_refuses_other_shapes(mlps):
    from graph_detr4d_amd._lib import Gd4dError
    i2l = torch.eye(4, device=DEV).repeat(2, 1, 1)
    with pytest.raises(ValueError):
        ops.petr_keys_fwd(torch.zeros(1, 2, 128, 4, 4, device=DEV), i2l, (64, 64), 64, 1, P.POSITION_RANGE, mlps['pe_image'], None,
                          torch.zeros(2, 16, 256, device=DEV))
    small = ops.mlp2_frustum_image(torch.zeros(512, 192, device=DEV), None, torch.zeros(256, 512, device=DEV))
    with pytest.raises(Gd4dError, match='not supported'):
        ops.petr_keys_fwd(torch.zeros(1, 2, 256, 4, 4, device=DEV), i2l, (64, 64), 64, 1, P.POSITION_RANGE, small, None,
                          torch.zeros(2, 16, 256, device=DEV))


def test_petr_keys_fwd_checks_its_biases(mlps):
    i2l = torch.eye(4, device=DEV).repeat(2, 1, 1)
    x, sine, d = torch.zeros(1, 2, 256, 4, 4, device=DEV), torch.zeros(2, 16, 256, device=DEV), mlps['d']
    args = (x, i2l, (64, 64), 64, 1, P.POSITION_RANGE, mlps['pe_image'])
    with pytest.raises(ValueError, match='pe_b2'):
        ops.petr_keys_fwd(*args, d['pe2b'][:128], sine)
    with pytest.raises(ValueError, match='se_b2'):
        ops.petr_keys_fwd(*args, d['pe2b'], sine, mlps['se_image'], d['ceb'][:64])
    with pytest.raises(ValueError, match='se_image'):
        ops.petr_keys_fwd(*args, d['pe2b'], sine, None, d['ceb'])


# ---- forward_keys --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('torch_route', [True, False])
def test_forward_keys_equals_forward_through_the_real_decoder(torch_route):
    """PETRTransformer.forward on the petr_transformer.npz inputs against forward_keys on rows permuted by hand, the real two-layer
    decoder in between, on the torch-op route (every module under Fn.torch_ops_for) and on the kernel route.  The same operations on
    the same values in the same layout: bit-equal."""
    from graph_detr4d_amd import functional as Fn
    g = Golden('petr_transformer')
    model = G.build_transformer(P.R.petr_config(g.meta['num_layers'], g.meta['feedforward_channels']))
    model.load_state_dict(g.state(), strict=True)
    model = model.to(DEV).eval()
    x, pos = g.t('x').float().to(DEV), g.t('pos_embed').float().to(DEV)
    mask, qe = g.t('mask').to(DEV), g.t('query_embed').float().to(DEV)
    bs = x.shape[0]
    keys = x.permute(1, 3, 4, 0, 2).reshape(-1, bs, 256).contiguous()
    key_pos = pos.permute(1, 3, 4, 0, 2).reshape(-1, bs, 256).contiguous()
    routed = [m for m in model.modules() if hasattr(m, 'torch_ops')] if torch_route else []
    with torch.no_grad(), Fn.torch_ops_for(*routed):
        want, memory = model(x, mask, qe, pos)
        got = model.forward_keys(keys, key_pos, mask.reshape(bs, -1), qe)
    assert torch.equal(memory, x) and tuple(got.shape) == (g.meta['num_layers'], bs, g.meta['num_query'], 256)
    assert torch.equal(got, want)
    torch.testing.assert_close(got.cpu(), g.t('out_dec'), **OUT_TOL)


# ---- the heads ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def kernel_outputs(golden, heads):
    """One kernel-route call per head with the key rows it handed to forward_keys recorded; shared by the tests below."""
    out = {}
    for kind, head in heads.items():
        seen = {}
        real = head.transformer.forward_keys

        def spy(keys, key_pos, mask, query_embed, reg_branch=None, _real=real, _seen=seen):
            _seen.update(keys=keys.clone(), key_pos=key_pos.clone(), mask=mask.clone(), query_embeds=query_embed.clone())
            return _real(keys, key_pos, mask, query_embed, reg_branch)
        head.transformer.forward_keys = spy
        try:
            with torch.no_grad():
                outs = head([golden.t(kind + '.feat').float().to(DEV)], _metas(golden, kind))
        finally:
            del head.transformer.forward_keys
        out[kind] = (outs, seen)
    return out


@pytest.mark.parametrize('kind', ['v1', 'v2'])
def test_head_key_rows_match_the_reference(golden, kernel_outputs, kind):
    g, (_, seen) = golden, kernel_outputs[kind]
    flat = lambda t: t.permute(1, 3, 4, 0, 2).reshape(-1, t.shape[0], 256)      # noqa: E731
    x = g.t(kind + '.x@512').float().div(512)
    torch.testing.assert_close(seen['keys'].cpu(), flat(x), rtol=2e-4, atol=2e-4)          # input_proj on the split-bf16 1x1 kernel
    assert torch.equal(seen['mask'].cpu(), g.t(kind + '.mask').reshape(2, -1))
    torch.testing.assert_close(seen['query_embeds'].cpu(), g.t(kind + '.query_embeds'), rtol=2e-4, atol=2e-4)
    ref = flat(g.t(kind + '.pos_embed'))
    d = (seen['key_pos'].cpu() - ref).abs()
    print(f'{kind}: max |key_pos - reference| = {float(d.max()):.2e}, share above 1e-2: {float((d > 1e-2).float().mean()):.2e}')
    assert float(d[ref.abs() < 8].max()) < 2e-4                            # the rule of tests/test_head_pe_gpu.py:44-45
    assert float((d > 1e-2).float().mean()) < 1e-3


@pytest.mark.parametrize('kind', ['v1', 'v2'])
def test_head_outputs_match_the_reference(golden, kernel_outputs, kind):
    outs, _ = kernel_outputs[kind]
    assert outs['enc_cls_scores'] is None and outs['enc_bbox_preds'] is None
    for name in ('all_cls_scores', 'all_bbox_preds'):
        want = golden.t(kind + '.' + name)
        assert tuple(outs[name].shape) == tuple(want.shape) == (P.LAYERS, P.BS, P.QUERIES, 10)
        print(f'{kind} {name}: max |kernel route - reference| = {float((outs[name].cpu() - want).abs().max()):.2e}')
        torch.testing.assert_close(outs[name].cpu(), want, **OUT_TOL)


@pytest.mark.parametrize('kind', ['v1', 'v2'])
def test_kernel_route_matches_torch_ops_and_makes_no_copies(golden, heads, kernel_outputs, kind, monkeypatch):
    head = heads[kind]
    feat, metas = [golden.t(kind + '.feat').float().to(DEV)], _metas(golden, kind)
    head.torch_ops = True
    try:
        with torch.no_grad():
            want = head(feat, metas)
    finally:
        head.torch_ops = False
    for name in ('all_cls_scores', 'all_bbox_preds'):
        torch.testing.assert_close(want[name].cpu(), golden.t(kind + '.' + name), **OUT_TOL)                # torch: the reference's op sequence
        torch.testing.assert_close(kernel_outputs[kind][0][name], want[name], **OUT_TOL)

    def refuse(t):
        raise AssertionError('the kernel route made a _camera_pixels_first copy')
    monkeypatch.setattr(PETRTransformer, '_camera_pixels_first', staticmethod(refuse))
    with torch.no_grad():
        again = head(feat, metas)
        assert torch.equal(again['all_cls_scores'], kernel_outputs[kind][0]['all_cls_scores'])
        with pytest.raises(AssertionError, match='_camera_pixels_first'):
            head.torch_ops = True
            try:
                head(feat, metas)
            finally:
                head.torch_ops = False


def test_kept_values_follow_their_parameters(golden, heads):
    """The sine branch and the query embedding are kept under ops._Stamp: an in-place update of adapt_pos3d / query_embedding shows in
    the next call, and undoing it restores the first result bit for bit.  (adapt_pos3d's FIRST bias: a shift of its last one moves every
    key's encoding by the same vector, which the softmax over the keys cancels.)"""
    head = heads['v2']
    feat, metas = [golden.t('v2.feat').float().to(DEV)], _metas(golden, 'v2')
    with torch.no_grad():
        first = head(feat, metas)['all_cls_scores'].clone()
        assert torch.equal(head(feat, metas)['all_cls_scores'], first)
        for p in (head.adapt_pos3d[0].bias, head.query_embedding[2].bias):
            p.add_(0.25)
            changed = head(feat, metas)['all_cls_scores'].clone()
            # (a stale kept value would give the first result bit for bit; 1e-5 is far above the fp32 rounding of scores below 1)
            assert float((changed - first).abs().max()) > 1e-5, 'a kept value outlived its parameter'
            p.sub_(0.25)
            assert torch.equal(head(feat, metas)['all_cls_scores'], first)


def test_get_bboxes_goes_through_the_coder(kernel_outputs):
    outs, _ = kernel_outputs['v1']
    head_cfg = P.head_config('v1')
    head = G.build_head(head_cfg)
    res = head.get_bboxes({k: (v.clone() if v is not None else None) for k, v in outs.items()}, [dict(), dict()])
    assert len(res) == P.BS
    boxes, scores, labels = res[0]
    assert boxes.shape[-1] == 9 and scores.shape == labels.shape and scores.numel() <= 300
