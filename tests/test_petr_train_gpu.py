"""PETRMultiheadAttention(hip_train=True) on the GPU: the two-layer transformer's gradients against the fixture captured from the
reference (tests/golden/petr_transformer_grads.npz), one module against its torch_ops=True route, a checkpointed decoder layer
against a plain one, and the refusals.  Every case prints its figures before it asserts."""
import copy
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import graph_detr4d_amd as G  # noqa: E402
import petr_grads as PG  # noqa: E402
import petr_ref as R  # noqa: E402
from golden_io import Golden, sub  # noqa: E402
from graph_detr4d_amd import _lib  # noqa: E402
from graph_detr4d_amd import functional as Fn  # noqa: E402
from petr_ref import petr_config  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module')
def golden():
    return Golden('petr_transformer')


@pytest.fixture(scope='module')
def grads():
    return Golden('petr_transformer_grads')


def _config(num_layers, ffn, **cross):
    cfg = petr_config(num_layers, ffn)
    cfg['decoder']['transformerlayers']['attn_cfgs'][1].update(cross)
    return cfg


def _transformer_grads(golden, grads, **cross):
    g, m = golden, golden.meta
    model = G.build_transformer(_config(m['num_layers'], m['feedforward_channels'], **cross))
    model.load_state_dict(g.state(), strict=True)
    model = model.to(DEV).eval()                                     # eval mode with autograd: no dropout, with_cp inactive
    x, pos, qe = (g.t(k).float().to(DEV).requires_grad_(True) for k in ('x', 'pos_embed', 'query_embed'))
    out_dec, _ = model(x, g.t('mask').to(DEV), qe, pos)
    (out_dec * grads.t('G').float().to(DEV)).sum().backward()
    return out_dec.detach(), PG.as_fixture(x, pos, qe, [(k, p.grad) for k, p in model.named_parameters()])


def test_transformer_gradients_match_the_reference_fixture(golden, grads):
    """The yardstick is the fp32 torch_ops=True route of the cross-attentions on the GPU, run here on the same inputs: per tensor, the
    kernel route gets four times that route's observed max error against the fixture - no floor.  What the fixture itself is off by
    (its distance from the fp64 restatement, tests/test_petr_train_cpu.py) is printed beside the two for information only.

    Observed on an MI355X (docs/measurements_r37.md has the table), kernels / torch_ops / fixture: grad.x 2.1e-7 / 1.7e-7 / 1.4e-7,
    grad.pos_embed 1.3e-7 / 8.2e-8 / 9.1e-8, the cross-attention weight sums 1e-5 - 5e-5 in all three on values of 28 - 65; the largest
    kernels / torch_ops ratio of the 54 tensors is 1.6.  (With three bf16 products in the core the same run had nine tensors beyond
    the bound, up to 10 x the torch-op route: every product of the training core now takes six.)"""
    g, m = golden, golden.meta
    out_dec, got = _transformer_grads(golden, grads, hip_train=True)
    e_out = float((out_dec.cpu() - g.t('out_dec')).abs().max())
    print(f'out_dec: max |hip_train route - reference| = {e_out:.2e}')
    assert e_out < 1e-3
    _, torch_route = _transformer_grads(golden, grads, torch_ops=True)
    sd = {k: v.double().to(DEV).requires_grad_(True) for k, v in g.state().items()}
    x, pos, qe = (g.t(k).double().to(DEV).requires_grad_(True) for k in ('x', 'pos_embed', 'query_embed'))
    ref_out, _, _ = R.transformer(sd, m['num_heads'], m['num_layers'], x, g.t('mask').to(DEV), qe, pos)
    (ref_out * grads.t('G').double().to(DEV)).sum().backward()
    e_fix = PG.errors(PG.as_fixture(x, pos, qe, [(k, v.grad) for k, v in sd.items()]), grads)
    e_torch, e_kernel = PG.errors(torch_route, grads), PG.errors(got, grads)
    print(f'{"tensor":58s} {"kernels":>9s} {"torch_ops":>9s} {"fixture":>9s} {"scale":>9s}')
    for k in sorted(e_kernel):
        print(f'{k:58s} {e_kernel[k][0]:9.2e} {e_torch[k][0]:9.2e} {e_fix[k][0]:9.2e} {e_kernel[k][1]:9.2e}')
    print('worst relative (error / max(1, scale)): kernels %.2e (%s), torch_ops %.2e (%s), fixture %.2e (%s)'
          % (PG.worst_relative(e_kernel) + PG.worst_relative(e_torch) + PG.worst_relative(e_fix)))
    ratio, key = max((e_kernel[k][0] / e_torch[k][0], k) for k in e_kernel if e_torch[k][0] > 0)
    print(f'largest kernels / torch_ops ratio: {ratio:.2f} ({key})')
    late = [k for k in e_kernel if e_kernel[k][0] > 4 * e_torch[k][0]]
    assert not late, late
    # no gradient reaches a padded pixel: the key-side kernel writes exact zeros for masked keys
    pad = g.t('mask')[:, :, None].expand_as(g.t('x')).to(DEV)
    assert bool(pad.any()) and bool((got['grad.x'][pad] == 0).all()) and bool((got['grad.pos_embed'][pad] == 0).all())


def _module(golden, **kw):
    m = G.build_attention(dict(type='PETRMultiheadAttention', embed_dims=256, num_heads=8, dropout=0.0, **kw))
    m.load_state_dict(sub(golden.state(), 'decoder.layers.0.attentions.1.'), strict=True)
    return m.to(DEV).train()


def _module_inputs(golden, lq=40):
    g, bs = golden, golden.meta['batch']
    flat = lambda t: t.float().permute(1, 3, 4, 0, 2).reshape(-1, bs, 256).contiguous().to(DEV)      # noqa: E731
    gen = torch.Generator().manual_seed(5)
    memory = flat(g.t('x'))
    return dict(query=g.t('cross0_query').to(DEV), key=memory, value=torch.randn(memory.shape, generator=gen).to(DEV),
                key_pos=flat(g.t('pos_embed')), query_pos=g.t('query_embed').float().unsqueeze(1).repeat(1, bs, 1).to(DEV),
                identity=torch.randn(lq, bs, 256, generator=gen).to(DEV), mask=g.t('mask').reshape(bs, -1).to(DEV),
                weight=torch.randn(lq, bs, 256, generator=gen).to(DEV))


@pytest.mark.parametrize('case', ['key_is_value', 'own_value', 'batch_first', 'no_encodings'])
def test_module_in_train_mode_matches_torch_ops(golden, case):
    """attn_drop = 0, train mode: output and the gradients of query, key, (value,) key_pos, query_pos, identity, in_proj_weight /
    bias and out_proj against F.multi_head_attention_forward on the same parameters.  Both routes are fp32 on the GPU (the kernel
    route's core on six split-bf16 products per multiply-add); the bound is tests/test_modules_gpu.py's 2e-4, taken relative to each
    tensor's largest value (the bias gradients here reach 27).  Observed: at most 7.2e-6 on 11.8 (in_proj_bias), inputs 3e-8 - 8e-8 on 0.05 - 0.1."""
    c = _module_inputs(golden)
    names = ['query', 'key', 'key_pos', 'query_pos', 'identity'] + (['value'] if case == 'own_value' else [])
    if case == 'no_encodings':
        names = ['query', 'key', 'identity']
    results = []
    for kw in (dict(hip_train=True), dict(torch_ops=True)):
        m = _module(golden, batch_first=case == 'batch_first', **kw)
        t = {k: c[k].clone().requires_grad_(True) for k in names}
        tr = (lambda v: v.transpose(0, 1)) if case == 'batch_first' else (lambda v: v)      # noqa: E731
        value = tr(t['value']) if case == 'own_value' else tr(t['key'])
        pos = {} if case == 'no_encodings' else dict(query_pos=tr(t['query_pos']), key_pos=tr(t['key_pos']))
        out = m(tr(t['query']), tr(t['key']), value, tr(t['identity']), key_padding_mask=c['mask'], **pos)
        (out * tr(c['weight'])).sum().backward()
        res = {'out': tr(out).detach()}
        res.update({'d ' + k: v.grad for k, v in t.items()})
        res.update({'d ' + k: p.grad for k, p in m.named_parameters()})
        results.append(res)
    got, want = results
    assert set(got) == set(want) and {'d attn.in_proj_weight', 'd attn.in_proj_bias', 'd attn.out_proj.weight', 'd attn.out_proj.bias'} <= set(got)
    worst = 0.
    for k in sorted(got):
        e, s = float((got[k] - want[k]).abs().max()), float(want[k].abs().max())
        worst = max(worst, e / max(1.0, s))
        print(f'{k:26s} max error {e:.2e}  scale {s:.2e}')
        assert torch.isfinite(got[k]).all() and e <= 2e-4 * max(1.0, s), k
    # masked keys take no gradient, exactly (batch 0 has padded pixels)
    gone = c['mask'].t()
    assert bool(gone.any()) and bool((got['d key'][gone] == 0).all())


def _layer(golden, with_cp):
    cfg = copy.deepcopy(_config(1, golden.meta['feedforward_channels'], hip_train=True)['decoder']['transformerlayers'])
    cfg['with_cp'] = with_cp
    layer = G.build_transformer_layer(cfg)
    layer.load_state_dict(sub(golden.state(), 'decoder.layers.0.'), strict=True)
    return layer.to(DEV).train()


def test_checkpointed_layer_equals_the_plain_layer_bit_for_bit(golden):
    """dropout = 0.1 everywhere, train mode, the same torch.manual_seed: torch.utils.checkpoint restores the generator state, so the
    recomputed forward draws the same seeds and masks - outputs and all gradients are torch.equal."""
    c = _module_inputs(golden)
    results = []
    for with_cp in (True, False):
        layer = _layer(golden, with_cp)
        assert layer.use_checkpoint == with_cp and layer.attentions[1].hip_train and layer.attentions[1].attn_drop == 0.1
        t = {k: c[k].clone().requires_grad_(True) for k in ('query', 'key', 'query_pos', 'key_pos')}
        torch.manual_seed(1234)
        out = layer(t['query'], t['key'], t['key'], query_pos=t['query_pos'], key_pos=t['key_pos'], key_padding_mask=c['mask'])
        (out * c['weight']).sum().backward()
        res = {'out': out.detach()}
        res.update({'d ' + k: v.grad for k, v in t.items()})
        res.update({'d ' + k: p.grad for k, p in layer.named_parameters()})
        results.append(res)
    cp, plain = results
    assert set(cp) == set(plain)
    diff = {k: float((cp[k] - plain[k]).abs().max()) for k in cp if not torch.equal(cp[k], plain[k])}
    print(f'{len(cp)} tensors, differing: {diff}')
    assert not diff
    # and dropout was on: another seed gives another output
    layer = _layer(golden, False)
    torch.manual_seed(4321)
    with torch.no_grad():
        other = layer(c['query'], c['key'], c['key'], query_pos=c['query_pos'], key_pos=c['key_pos'], key_padding_mask=c['mask'])
    assert not torch.equal(other, plain['out'])


@pytest.mark.parametrize('cross', [False, True])
def test_train_mode_without_autograd_draws_what_autograd_draws(golden, cross):
    """MultiheadAttention (and PETRMultiheadAttention with hip_train) in train mode: a call under torch.no_grad() - the first pass of a
    reentrant checkpoint - takes the training path, so under one torch.manual_seed it returns the bits of the call with autograd, its
    attention dropout is on (another seed, another output), and it leaves the generator where the autograd call leaves it."""
    c = _module_inputs(golden)
    if cross:
        m = G.build_attention(dict(type='PETRMultiheadAttention', embed_dims=256, num_heads=8, attn_drop=0.3, hip_train=True,
                                   dropout_layer=None))
        m.load_state_dict(sub(golden.state(), 'decoder.layers.0.attentions.1.'), strict=True)
        call = lambda: m(c['query'], c['key'], c['key'], query_pos=c['query_pos'], key_pos=c['key_pos'], key_padding_mask=c['mask'])      # noqa: E731
    else:
        m = G.build_attention(dict(type='MultiheadAttention', embed_dims=256, num_heads=8, attn_drop=0.3))
        m.load_state_dict(sub(golden.state(), 'decoder.layers.0.attentions.0.'), strict=True)
        call = lambda: m(c['query'], query_pos=c['query_pos'])      # noqa: E731
    m = m.to(DEV).train()
    torch.manual_seed(99)
    with_grad = call()
    after_grad = torch.cuda.get_rng_state()
    with torch.no_grad():
        torch.manual_seed(99)
        quiet = call()
        after_quiet = torch.cuda.get_rng_state()
        torch.manual_seed(100)
        other = call()
    assert with_grad.requires_grad and not quiet.requires_grad
    assert torch.equal(with_grad.detach(), quiet) and torch.equal(after_grad, after_quiet)
    assert not torch.equal(other, quiet)
    m.eval()
    with torch.no_grad():                                               # eval mode: no dropout, no draw
        before = torch.cuda.get_rng_state()
        assert torch.equal(call(), call()) and torch.equal(torch.cuda.get_rng_state(), before)


def test_dropout_in_train_mode_only(golden):
    """attn_drop is applied inside the kernel in train mode and is 0 in eval mode; proj_drop / dropout_layer stay nn.Dropout."""
    c = _module_inputs(golden)
    m = G.build_attention(dict(type='PETRMultiheadAttention', embed_dims=256, num_heads=8, attn_drop=0.5, hip_train=True,
                               dropout_layer=None))
    m.load_state_dict(sub(golden.state(), 'decoder.layers.0.attentions.1.'), strict=True)
    m = m.to(DEV)
    call = lambda: m(c['query'], c['key'], c['key'], query_pos=c['query_pos'], key_pos=c['key_pos'], key_padding_mask=c['mask'])      # noqa: E731
    torch.manual_seed(1)
    a = call()
    torch.manual_seed(1)
    b = call()
    torch.manual_seed(2)
    d = call()
    assert a.requires_grad and torch.equal(a, b) and not torch.equal(a, d)
    m.eval()
    e, f = call(), call()
    assert e.requires_grad and torch.equal(e, f)
    with torch.no_grad():
        quiet = G.build_attention(dict(type='PETRMultiheadAttention', embed_dims=256, num_heads=8, attn_drop=0.5, dropout_layer=None))
        quiet.load_state_dict(m.state_dict())
        want = quiet.to(DEV).eval()(c['query'], c['key'], c['key'], query_pos=c['query_pos'], key_pos=c['key_pos'], key_padding_mask=c['mask'])
    err = float((e.detach() - want).abs().max())
    print(f'eval mode with autograd against the inference route: {err:.2e}')
    assert err < 2e-4


def test_refusals(golden):
    c = _module_inputs(golden)
    call = lambda m, **kw: m(c['query'], c['key'], c['key'], query_pos=c['query_pos'], key_pos=c['key_pos'],      # noqa: E731
                             key_padding_mask=c['mask'], **kw)
    m = _module(golden, hip_train=True)
    lq, lk = c['query'].shape[0], c['key'].shape[0]
    with pytest.raises(_lib.Gd4dError, match='torch_ops'):
        call(m, attn_mask=torch.zeros(lq, lk, dtype=torch.bool, device=DEV))
    wide = G.build_attention(dict(type='PETRMultiheadAttention', embed_dims=256, num_heads=4, hip_train=True)).to(DEV).train()
    with pytest.raises(_lib.Gd4dError, match='torch_ops'):                # head dim 64
        call(wide)
    small = G.build_attention(dict(type='PETRMultiheadAttention', embed_dims=128, num_heads=4, hip_train=True)).to(DEV).train()
    with pytest.raises(_lib.Gd4dError, match='torch_ops'):                # 128 channels
        small(c['query'][..., :128].contiguous(), c['key'][..., :128].contiguous())
    half = _module(golden, hip_train=True).half()
    with pytest.raises(_lib.Gd4dError, match='torch_ops'):                # float16
        half(c['query'].half(), c['key'].half(), c['key'].half())
    # B heads Lq Lk >= 2^32 with dropout: refused from the shapes, before anything is computed (expanded views, no memory behind them)
    drop = G.build_attention(dict(type='PETRMultiheadAttention', embed_dims=256, num_heads=8, attn_drop=0.1, hip_train=True)).to(DEV).train()
    big_q, big_k = torch.zeros(1, 1, 256, device=DEV).expand(8192, 2, 256), torch.zeros(1, 1, 256, device=DEV).expand(32768, 2, 256)
    with pytest.raises(_lib.Gd4dError, match='torch_ops'):
        drop(big_q, big_k, big_k)
    # hip_train=False: train mode and autograd are still refused, naming torch_ops
    plain = _module(golden)
    with pytest.raises(_lib.Gd4dError, match='torch_ops'):
        call(plain)
    with pytest.raises(_lib.Gd4dError, match='torch_ops'):
        call(plain.eval())                                                     # parameters want gradients
    # and the choice still stands
    with Fn.torch_ops_for(m):
        assert torch.isfinite(call(m, attn_mask=torch.zeros(lq, lk, dtype=torch.bool, device=DEV))).all()
