"""PETR's transformer modules on the GPU against the fixture captured from the reference (tests/golden/petr_transformer.npz):
the cross-attention module alone (TOL of tests/test_modules_gpu.py, 2e-4), the two-layer transformer (1e-3, as that file holds
multi-layer states), the kernel route against torch_ops=True, the refusals, and batch_first."""
import pytest
import torch

import graph_detr4d_amd as G
from golden_io import Golden, sub
from graph_detr4d_amd import _lib
from graph_detr4d_amd import functional as Fn
from petr_ref import petr_config

pytestmark = pytest.mark.gpu
TOL = dict(rtol=2e-4, atol=2e-4)
DEV = 'cuda'


@pytest.fixture(scope='module')
def golden():
    return Golden('petr_transformer')


@pytest.fixture(scope='module')
def cross_inputs(golden):
    """The recorded call of decoder layer 0's cross-attention: query, key = value = memory, encodings, mask - (L, B, C) on the GPU."""
    g, bs = golden, golden.meta['batch']
    flat = lambda t: t.float().permute(1, 3, 4, 0, 2).reshape(-1, bs, 256).contiguous().to(DEV)      # noqa: E731
    return dict(query=g.t('cross0_query').to(DEV), memory=flat(g.t('x')), key_pos=flat(g.t('pos_embed')),
                query_pos=g.t('query_embed').float().unsqueeze(1).repeat(1, bs, 1).to(DEV),
                mask=g.t('mask').reshape(bs, -1).to(DEV), want=g.t('cross0_out').to(DEV))


def _attention(golden, **kw):
    m = G.build_attention(dict(type='PETRMultiheadAttention', embed_dims=256, num_heads=8, dropout=0.1, **kw))
    m.load_state_dict(sub(golden.state(), 'decoder.layers.0.attentions.1.'), strict=True)
    return m.to(DEV).eval()


def _call(m, c, **over):
    a = dict(query=c['query'], key=c['memory'], value=c['memory'], query_pos=c['query_pos'], key_pos=c['key_pos'],
             key_padding_mask=c['mask'])
    a.update(over)
    query, key, value, identity = a.pop('query'), a.pop('key'), a.pop('value'), a.pop('identity', None)
    return m(query, key, value, identity, **a)


def test_attention_module_matches_the_reference(golden, cross_inputs):
    m = _attention(golden)
    with torch.no_grad():
        got = _call(m, cross_inputs)
    print(f'max |kernel route - reference| = {float((got - cross_inputs["want"]).abs().max()):.2e}')
    torch.testing.assert_close(got, cross_inputs['want'], **TOL)


def test_attention_kernel_route_matches_torch_ops(golden, cross_inputs):
    c = cross_inputs
    m, t = _attention(golden), _attention(golden, torch_ops=True)
    with torch.no_grad():
        got, want = _call(m, c), _call(t, c)
        torch.testing.assert_close(want, c['want'], rtol=1e-5, atol=1e-5)          # torch on the GPU: the reference's own op sequence
        torch.testing.assert_close(got, want, **TOL)
        # no mask, no encodings, a distinct value tensor (two GEMMs), an identity of its own
        value = torch.randn_like(c['memory'])
        identity = torch.randn_like(c['query'])
        for over in (dict(key_padding_mask=None), dict(query_pos=None, key_pos=None), dict(value=value), dict(identity=identity),
                     dict(key_padding_mask=c['mask'].to(torch.uint8))):
            torch.testing.assert_close(_call(m, c, **over), _call(t, c, **over), **TOL)
        with Fn.torch_ops_for(m):                                                  # the same module, switched for a block
            torch.testing.assert_close(_call(m, c), want, rtol=1e-6, atol=1e-6)
    assert not m.torch_ops


def test_torch_ops_route_is_differentiable(golden, cross_inputs):
    c = cross_inputs
    t = _attention(golden, torch_ops=True)
    q = c['query'].clone().requires_grad_(True)
    _call(t, c, query=q).square().sum().backward()
    assert q.grad is not None and torch.isfinite(q.grad).all() and t.attn.in_proj_weight.grad is not None


def test_transformer_matches_the_reference(golden):
    g, m = golden, golden.meta
    model = G.build_transformer(petr_config(m['num_layers'], m['feedforward_channels']))
    model.load_state_dict(g.state(), strict=True)
    model = model.to(DEV).eval()
    x, pos, qe, mask = g.t('x').float().to(DEV), g.t('pos_embed').float().to(DEV), g.t('query_embed').float().to(DEV), g.t('mask').to(DEV)
    seen = {}
    hook = model.decoder.layers[0].attentions[1].register_forward_hook(lambda mod, inp, out: seen.update(out=out))
    with torch.no_grad():
        out_dec, memory = model(x, mask, qe, pos)
        hook.remove()
        cross = [l.attentions[1] for l in model.decoder.layers]
        with Fn.torch_ops_for(*cross):
            out_torch, _ = model(x, mask, qe, pos)
    assert tuple(out_dec.shape) == (m['num_layers'], m['batch'], m['num_query'], 256)
    assert tuple(memory.shape) == tuple(x.shape) and torch.equal(memory, x)
    print(f'out_dec: max |kernel route - reference| = {float((out_dec.cpu() - g.t("out_dec")).abs().max()):.2e}')
    # inside the layer the module takes the LayerNorm that follows it into its out-projection: what it returns is norms.1 of the sum
    sd = g.state()
    normed = torch.nn.functional.layer_norm(g.t('cross0_out'), (256,), sd['decoder.layers.0.norms.1.weight'], sd['decoder.layers.0.norms.1.bias'])
    torch.testing.assert_close(seen['out'].cpu(), normed, **TOL)
    torch.testing.assert_close(out_dec.cpu(), g.t('out_dec'), rtol=1e-3, atol=1e-3)
    torch.testing.assert_close(out_dec, out_torch, rtol=1e-3, atol=1e-3)
    # a decoder that returns the last layer only: (1, bs, queries, c), the last intermediate
    model.decoder.return_intermediate = False
    with torch.no_grad():
        last, _ = model(x, mask, qe, pos)
    torch.testing.assert_close(last, out_dec[-1:], rtol=1e-6, atol=1e-6)


def test_refusals_name_torch_ops(golden, cross_inputs):
    c = cross_inputs
    m = _attention(golden)
    lq, lk = c['query'].shape[0], c['memory'].shape[0]
    with torch.no_grad():
        with pytest.raises(_lib.Gd4dError, match='torch_ops'):
            _call(m, c, attn_mask=torch.zeros(lq, lk, dtype=torch.bool, device=DEV))
    with pytest.raises(_lib.Gd4dError, match='torch_ops'):                          # autograd: parameters want gradients
        _call(m, c)
    with torch.no_grad():
        m.train()
        with pytest.raises(_lib.Gd4dError, match='torch_ops'):
            _call(m, c)
        m.eval()
        q = c['query'].clone().requires_grad_(True)
    for p in m.parameters():
        p.requires_grad_(False)
    with pytest.raises(_lib.Gd4dError, match='torch_ops'):                          # autograd on an input
        _call(m, c, query=q)
    with torch.no_grad():
        wide = G.build_attention(dict(type='PETRMultiheadAttention', embed_dims=256, num_heads=4)).to(DEV).eval()       # head dim 64
        with pytest.raises(_lib.Gd4dError, match='torch_ops'):
            _call(wide, c)
        small = G.build_attention(dict(type='PETRMultiheadAttention', embed_dims=128, num_heads=4)).to(DEV).eval()      # 128 channels
        with pytest.raises(_lib.Gd4dError, match='torch_ops'):
            small(c['query'][..., :128].contiguous(), c['memory'][..., :128].contiguous())
        wide.torch_ops = True
        assert torch.isfinite(_call(wide, c)).all()


def test_batch_first_equals_the_transposed_call(golden, cross_inputs):
    c = cross_inputs
    m, bf = _attention(golden), _attention(golden, batch_first=True)
    tr = lambda t: t.transpose(0, 1).contiguous()                                   # noqa: E731
    with torch.no_grad():
        want = _call(m, c)
        got = _call(bf, c, query=tr(c['query']), key=(mem := tr(c['memory'])), value=mem, query_pos=tr(c['query_pos']),
                    key_pos=tr(c['key_pos']))
        assert tuple(got.shape) == (c['query'].shape[1], c['query'].shape[0], 256)
        torch.testing.assert_close(got.transpose(0, 1), want, rtol=1e-6, atol=1e-6)
        with Fn.torch_ops_for(bf):
            torch.testing.assert_close(_call(bf, c, query=tr(c['query']), key=mem, value=mem, query_pos=tr(c['query_pos']),
                                             key_pos=tr(c['key_pos'])), got, **TOL)
