"""DepthNet(hip_train=True): the training forward and backward on the library's kernels against the fp64 restatement
(depth_net_train_ref.py) and against the module's torch-op route.  GPU only.

The backward is compared as the derivative of the forward the DEVICE computed: the helper gets the device's own ReLU mask
(out_dev > 0), and a separate condition bounds where that mask may differ from the fp64 one."""
import functools

import numpy as np
import pytest
import torch

from depth_net_train_ref import backward64, forward64, rel_fro, running_update

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
# the smallest levels at which each mechanism can go wrong: 2 N values per channel and fewer tiles than wgrad partitions; inside one
# tile with every pixel on the halo's border; exactly one tile; ragged in both directions (2 x 3 tiles)
ALL4 = ((1, 2), (5, 7), (16, 16), (17, 33))
FIVE = ALL4 + ((3, 4),)                                                     # a fifth level forces a second launch
CASES = [(2, ALL4), (3, ALL4), (3, FIVE)] + [(2, (lvl,)) for lvl in ALL4] + [(3, (ALL4[0],)), (3, (ALL4[3],))]
IDS = [f'n{n}-' + '+'.join(f'{h}x{w}' for h, w in lv) for n, lv in CASES]
FWD_TOL, MASK_BAND, MASK_SHARE, BWD_TOL, ROUTES_TOL, STAT_TOL = 2e-4, 2e-4, 1e-3, 1e-3, 2e-4, 1e-5


def _metas(n):
    focal = (600.0, 1500.0, 3000.0)
    ks = []
    for i in range(n):
        k = np.eye(4, dtype=np.float32)
        k[0, 0], k[1, 1], k[0, 2], k[1, 2] = focal[i], focal[i] * 1.05, 800.0, 450.0
        ks.append(k)
    ida = [torch.tensor([[0.8, 0., -20.], [0., 0.8, -40.], [0., 0., 1.]], dtype=torch.float32)]
    return [dict(intrinsics=ks, ida_mats=ida)]


def _module(seed, **kw):
    from graph_detr4d_amd import DepthNet
    torch.manual_seed(seed)
    mod = DepthNet(256, 256, 80, **kw)
    bn = mod.reduce_conv[1]
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(256) * 0.3)
        bn.running_var.copy_(0.25 + 2 * torch.rand(256))
        bn.weight.copy_(1 + 0.2 * torch.randn(256))
        bn.bias.copy_(0.2 * torch.randn(256))
        mod.reduce_conv[0].bias.copy_(0.1 * torch.randn(256))
        for p in list(mod.mlp.parameters()) + list(mod.se.parameters()):
            p.copy_(torch.randn(p.shape) * 0.15)
    return mod.to(DEV)


def _inputs(n, levels, seed=11):
    gen = torch.Generator().manual_seed(seed + 97 * n + len(levels) + 13 * levels[0][0])
    xs = [torch.randn(n, 256, h, w, generator=gen) for h, w in levels]
    rs = [torch.randn(n, 256, h, w, generator=gen) for h, w in levels]
    return xs, rs


def _run(mod, xs, rs, metas, per_level=False):
    """Forward + backward of sum_l (out_l r_l).sum(); returns outs, input grads and parameter grads (clones)."""
    mod.zero_grad(set_to_none=True)
    feats = [x.to(DEV).requires_grad_() for x in xs]
    if per_level:
        mats = dict(intrin_mats=metas[0]['intrinsics'], ida_mats=metas[0]['ida_mats'])
        outs = [mod(f, mats) for f in feats]
    else:
        outs = [o[0] for o in mod.forward_levels([f[None] for f in feats], metas)]
    loss = sum((o * r.to(DEV)).sum() for o, r in zip(outs, rs))
    loss.backward()
    grads = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in mod.named_parameters()}
    return [o.detach() for o in outs], [f.grad.detach().clone() for f in feats], grads


def _gate_grad(mod, metas):
    """The gate the module's own layers give (fp32, device), differentiable towards mlp / se."""
    intr = np.stack(metas[0]['intrinsics']).reshape(-1, 16)
    ida00 = np.full((intr.shape[0],), float(metas[0]['ida_mats'][0][0, 0]), dtype=np.float32)
    return mod._gate_torch_device(intr, ida00, 1000.0, torch.device(DEV))


def _gate(mod, metas):
    with torch.no_grad():
        return _gate_grad(mod, metas)


@functools.lru_cache(maxsize=None)
def _case(n, levels, frozen=False):
    """One HIP forward + backward of the case and its fp64 reference (computed once, shared by the tests, never changed)."""
    metas = _metas(n)
    xs, rs = _inputs(n, levels)
    mod = _module(5, hip_train=True)
    mod.train(not frozen)
    if len(levels) == 1 and not frozen:
        # one call from known initial buffers: zeros, so that the buffers afterwards are momentum x the statistics, one rounding
        with torch.no_grad():
            mod.reduce_conv[1].running_mean.zero_()
            mod.reduce_conv[1].running_var.zero_()
    state0 = {k: v.detach().clone() for k, v in mod.state_dict().items()}
    outs, dxs, grads = _run(mod, xs, rs, metas)
    gate = _gate(mod, metas)
    conv, bn = mod.reduce_conv[0], mod.reduce_conv[1]
    fwd, bwd_dev, bwd_own = [], [], []
    for x, r, o in zip(xs, rs, outs):
        f = forward64(x, conv.weight, conv.bias, bn.weight, bn.bias, gate, bn.eps,
                      running=(state0['reduce_conv.1.running_mean'], state0['reduce_conv.1.running_var']) if frozen else None)
        fwd.append(f)
        bwd_dev.append(backward64(f, r, o.cpu() > 0))
    return dict(mod=mod, metas=metas, xs=xs, rs=rs, state0=state0, outs=outs, dxs=dxs, grads=grads, gate=gate, fwd=fwd, bwd=bwd_dev)


def _torch_twin(c, frozen=False):
    twin = _module(5, torch_ops=True)
    twin.load_state_dict(c['state0'], strict=True)
    return twin.train(not frozen)


def test_gates_differ_clearly():
    g = _case(3, ALL4)['gate']
    assert g.shape == (3, 256) and float((g[0] - g[1]).abs().max()) > 0.05 and float((g[1] - g[2]).abs().max()) > 0.05


@pytest.mark.parametrize('n,levels', CASES, ids=IDS)
def test_forward_train_mode(n, levels):
    c = _case(n, levels)
    bn = c['mod'].reduce_conv[1]
    rm, rv = c['state0']['reduce_conv.1.running_mean'].double().cpu(), c['state0']['reduce_conv.1.running_var'].double().cpu()
    mom = bn.momentum
    for (h, w), f, o in zip(levels, c['fwd'], c['outs']):
        err = float((o.double().cpu() - f['out']).abs().max() / f['out'].abs().max())
        print(f'forward n={n} {h}x{w}: max err / max|ref| = {err:.3e}')
        assert err <= FWD_TOL
    m_last = n * levels[-1][0] * levels[-1][1]
    for f, (h, w) in zip(c['fwd'][:-1], levels[:-1]):
        rm, rv = running_update(rm, rv, f['mu'], f['var'], n * h * w, mom)
    if len(levels) == 1:
        # mu and the biased variance recovered from the buffers after ONE call from known (zero) initial buffers
        assert float(rm.abs().max()) == 0 and float(rv.abs().max()) == 0
        mu_dev = bn.running_mean.double().cpu() / mom
        var_dev = bn.running_var.double().cpu() / mom * (m_last - 1) / m_last
        e_mu = float((mu_dev - c['fwd'][-1]['mu']).abs().max() / c['fwd'][-1]['mu'].abs().max())
        e_var = float((var_dev - c['fwd'][-1]['var']).abs().max() / c['fwd'][-1]['var'].abs().max())
        print(f'statistics n={n} {levels[-1]}: mu {e_mu:.3e}, var {e_var:.3e} (max error / max|ref|)')
        assert e_mu <= STAT_TOL and e_var <= STAT_TOL
    # and after all levels the buffers are those of L fp64 BatchNorm2d calls
    rm2, rv2 = running_update(rm, rv, c['fwd'][-1]['mu'], c['fwd'][-1]['var'], m_last, mom)
    assert float((bn.running_mean.double().cpu() - rm2).abs().max() / rm2.abs().max()) <= STAT_TOL
    assert float((bn.running_var.double().cpu() - rv2).abs().max() / rv2.abs().max()) <= STAT_TOL
    assert int(bn.num_batches_tracked) - int(c['state0']['reduce_conv.1.num_batches_tracked']) == len(levels)


@pytest.mark.parametrize('n,levels', [CASES[0], CASES[2]], ids=[IDS[0], IDS[2]])
def test_forward_levels_equals_per_level_calls(n, levels):
    c = _case(n, levels)
    mod = _module(5, hip_train=True).train()
    mod.load_state_dict(c['state0'], strict=True)
    outs, dxs, grads = _run(mod, c['xs'], c['rs'], c['metas'], per_level=True)
    for a, b in zip(outs, c['outs']):
        assert torch.equal(a, b)
    for k, v in mod.state_dict().items():
        assert torch.equal(v, c['mod'].state_dict()[k]), k
    for a, b in zip(dxs, c['dxs']):
        assert torch.equal(a, b)


@pytest.mark.parametrize('n,levels', CASES[:3], ids=IDS[:3])
def test_relu_mask_condition(n, levels):
    c = _case(n, levels)
    twin = _torch_twin(c)
    with torch.no_grad():
        t_outs = [o[0] for o in twin.forward_levels([x.to(DEV)[None] for x in c['xs']], c['metas'])]
    for (h, w), f, o_dev, o_t in zip(levels, c['fwd'], c['outs'], t_outs):
        z = f['z']
        band = z.abs() <= MASK_BAND * z.abs().max()
        for name, o in (('torch-op fp32', o_t), ('hip', o_dev)):       # the fp32 torch route first: the seeds meet the cap
            differ = (o.cpu() > 0) != (z > 0)
            share = float(differ.double().mean())
            print(f'mask n={n} {h}x{w} {name}: {int(differ.sum())} of {differ.numel()} differ')
            assert bool((differ & ~band).sum() == 0), name
            assert share <= MASK_SHARE, name


def _check_backward(c, n, levels, grads, dxs, label):
    want = {k: sum(b[k] for b in c['bwd']) for k in ('dW', 'db', 'dgamma', 'dbeta', 'dg')}
    errs = {}
    for (h, w), b, dx in zip(levels, c['bwd'], dxs):
        errs[f'dx {h}x{w}'] = rel_fro(dx, b['dx'])
    errs['dW'] = rel_fro(grads['reduce_conv.0.weight'], want['dW'])
    errs['dgamma'] = rel_fro(grads['reduce_conv.1.weight'], want['dgamma'])
    errs['dbeta'] = rel_fro(grads['reduce_conv.1.bias'], want['dbeta'])
    print(f'backward {label} n={n}: ' + ', '.join(f'{k} {v:.2e}' for k, v in errs.items()))
    return errs, want


@pytest.mark.parametrize('n,levels', CASES, ids=IDS)
def test_backward_against_fp64_with_device_mask(n, levels):
    c = _case(n, levels)
    errs, want = _check_backward(c, n, levels, c['grads'], c['dxs'], 'hip')
    # the Function's gate gradient: through the module's layers it reaches mlp / se; compare it where it leaves the Function,
    # as the gradient of se.conv_expand's bias = dg g (1 - g)
    g = c['gate'].double().cpu()
    dexp = (want['dg'] * g * (1 - g)).sum(0)
    errs['dg'] = rel_fro(c['grads']['se.conv_expand.bias'], dexp)
    print(f'backward hip n={n}: dg (as se.conv_expand.bias) {errs["dg"]:.2e}')
    for k, v in errs.items():
        assert v <= BWD_TOL, (k, v)
    # the convolution bias gradient: zero up to rounding with batch statistics - an absolute bound, per channel
    bound = 1e-3 * sum(b['dy'].abs().sum((0, 2, 3)) / (n * h * w) for b, (h, w) in zip(c['bwd'], levels))
    db = c['grads']['reduce_conv.0.bias'].double().cpu()
    print(f'backward hip n={n}: max |db| {float(db.abs().max()):.2e}, smallest bound {float(bound.min()):.2e}')
    assert bool((db.abs() <= bound).all())


def test_torch_op_route_backward_error_for_the_record():
    """The fp32 torch-op route against the same fp64 (its own mask): the figures docs/measurements_r16.md quotes next to the HIP
    route's.  Bounded by the same tolerance."""
    n, levels = CASES[1]
    c = _case(n, levels)
    twin = _torch_twin(c)
    outs, dxs, grads = _run(twin, c['xs'], c['rs'], c['metas'])
    own = dict(c)
    own['bwd'] = [backward64(f, r, o.cpu() > 0) for f, r, o in zip(c['fwd'], c['rs'], outs)]
    errs, _ = _check_backward(own, n, levels, grads, dxs, 'torch-op fp32')
    for k, v in errs.items():
        assert v <= BWD_TOL, (k, v)


def _mask_deltas(c, twin, twin_outs):
    """What the fp64 closed form says the two routes' gradients differ by where their ReLU decisions differ (zeros where they
    agree, the usual case).  A decision flipped at a near-zero entry - which test_relu_mask_condition allows either route - changes
    dz there by dout g, not by a rounding, so the routes are compared as derivatives of the forwards they each computed:
    (hip - twin) against (fp64 with the device's mask - fp64 with the twin's mask), within the two-routes bound."""
    if all(torch.equal(a > 0, b > 0) for a, b in zip(c['outs'], twin_outs)):
        return None
    own = [backward64(f, r, o.cpu() > 0) for f, r, o in zip(c['fwd'], c['rs'], twin_outs)]
    d = {k: sum(b[k] - t[k] for b, t in zip(c['bwd'], own)) for k in ('dW', 'dgamma', 'dbeta', 'dg')}
    delta = {'reduce_conv.0.weight': d['dW'], 'reduce_conv.1.weight': d['dgamma'], 'reduce_conv.1.bias': d['dbeta'],
             'dx': [b['dx'] - t['dx'] for b, t in zip(c['bwd'], own)]}
    gate = _gate_grad(twin, c['metas'])
    names = [k for k, _ in twin.named_parameters() if k.startswith(('mlp.', 'se.'))]
    gs = torch.autograd.grad(gate, [dict(twin.named_parameters())[k] for k in names], grad_outputs=d['dg'].float().to(DEV))
    delta.update({k: g.double().cpu() for k, g in zip(names, gs)})
    return delta


@pytest.mark.parametrize('n,levels', CASES[:3], ids=IDS[:3])
def test_module_level_against_the_torch_op_twin(n, levels):
    c = _case(n, levels)
    twin = _torch_twin(c)
    outs, dxs, grads = _run(twin, c['xs'], c['rs'], c['metas'])
    delta = _mask_deltas(c, twin, outs)
    print(f'routes n={n}: ReLU decisions {"agree" if delta is None else "differ: compared net of the fp64 closed form of the difference"}')
    for k, ref in grads.items():
        got = c['grads'][k]
        if k.startswith('context_conv.'):
            assert got is None and ref is None
            continue
        assert got is not None and float(got.abs().max()) > 0 and float(ref.abs().max()) > 0, k
        if k == 'reduce_conv.0.bias':
            continue                                                     # zero up to rounding on both routes: bounded in the fp64 test
        diff = (got - ref).double().cpu() - (0 if delta is None else delta[k].reshape(got.shape))
        err = float(diff.abs().max() / ref.abs().max())
        print(f'routes n={n} {k}: {err:.2e}')
        assert err <= ROUTES_TOL, k
    assert any(k.startswith('mlp.') for k in grads) and any(k.startswith('se.') for k in grads)
    for i, (a, b) in enumerate(zip(c['dxs'], dxs)):
        diff = (a - b).double().cpu() - (0 if delta is None else delta['dx'][i])
        assert float(diff.abs().max() / b.abs().max()) <= ROUTES_TOL
    for k, v in twin.state_dict().items():                               # the running buffers moved alike
        torch.testing.assert_close(c['mod'].state_dict()[k], v, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize('n,levels', [CASES[1], CASES[2]], ids=[IDS[1], IDS[2]])
def test_frozen_batchnorm(n, levels):
    c = _case(n, levels, True)
    infer = _module(5).eval()
    infer.load_state_dict(c['state0'], strict=True)
    with torch.no_grad():
        ref_outs = [o[0] for o in infer.forward_levels([x.to(DEV)[None] for x in c['xs']], c['metas'])]
        same_mod = [o[0] for o in c['mod'].forward_levels([x.to(DEV)[None] for x in c['xs']], c['metas'])]
    for a, b, d in zip(c['outs'], ref_outs, same_mod):
        assert torch.equal(a, b) and torch.equal(b, d)                      # the inference path's bits
    for k, v in c['mod'].state_dict().items():
        assert torch.equal(v, c['state0'][k]), k                            # no buffer moved
    errs, want = _check_backward(c, n, levels, c['grads'], c['dxs'], 'hip frozen')
    errs['db'] = rel_fro(c['grads']['reduce_conv.0.bias'], want['db'])        # not zero when frozen: a relative bound holds
    for k, v in errs.items():
        assert v <= BWD_TOL, (k, v)


def test_backward_is_deterministic():
    """Two forward + backward passes of one module on the same inputs: every gradient bit for bit (the buffers restored between)."""
    n, levels = CASES[2]
    c = _case(n, levels)
    mod = _module(5, hip_train=True).train()
    runs = []
    for _ in range(2):
        mod.load_state_dict(c['state0'], strict=True)
        runs.append(_run(mod, c['xs'], c['rs'], c['metas']))
    (outs0, dxs0, grads0), (outs1, dxs1, grads1) = runs
    for a, b, d in zip(dxs0, dxs1, c['dxs']):
        assert torch.equal(a, b) and torch.equal(a, d)
    for k in ('reduce_conv.0.weight', 'reduce_conv.0.bias', 'reduce_conv.1.weight', 'reduce_conv.1.bias'):
        assert torch.equal(grads0[k], c['grads'][k]), k                      # and the same bits as another module's pass
    for k, v in grads0.items():
        assert (v is None and grads1[k] is None) or torch.equal(v, grads1[k]), k


def test_wgrad_partitions():
    from graph_detr4d_amd import ops
    n, levels = CASES[1]
    c = _case(n, levels)
    dys = [b['dy'].float().to(DEV) for b in c['bwd']]
    xs = [x.to(DEV) for x in c['xs']]
    tiles = ops.depth_conv_tiles(levels, n)
    assert tiles == n * (1 + 1 + 1 + 6)
    ref = sum(b['dW'] for b in c['bwd'])
    got = [ops.depth_conv_wgrad(dys, xs, partitions=p) for p in (1, tiles, tiles + 5)] + [ops.depth_conv_wgrad(dys, xs)]
    for g in got:
        e = rel_fro(g, ref)
        print(f'wgrad: {e:.2e} against fp64')
        assert e <= BWD_TOL
    for g in got[1:]:
        assert rel_fro(g, got[0]) <= 1e-5


def test_dgrad_image_follows_the_weight():
    from graph_detr4d_amd import ops
    n, levels = CASES[0]
    c = _case(n, levels)
    mod = _module(5, hip_train=True).train()
    mod.load_state_dict(c['state0'], strict=True)
    _, dx0, _ = _run(mod, c['xs'], c['rs'], c['metas'])
    w = mod.reduce_conv[0].weight
    w.data.mul_(torch.linspace(0.5, 1.5, 256, device=DEV)[:, None, None, None])   # (through .data: no version counter moves)
    ops.invalidate_chain_images()
    state1 = {k: v.detach().clone() for k, v in mod.state_dict().items()}
    _, dx1, _ = _run(mod, c['xs'], c['rs'], c['metas'])
    fresh = _module(7, hip_train=True).train()
    fresh.load_state_dict(state1, strict=True)
    _, dx2, _ = _run(fresh, c['xs'], c['rs'], c['metas'])
    for a, b, d in zip(dx0, dx1, dx2):
        assert torch.equal(b, d) and not torch.equal(a, b)


def test_defaults_untouched():
    from graph_detr4d_amd import DepthNet
    from graph_detr4d_amd._lib import Gd4dError
    mod = DepthNet(256, 256, 80).to(DEV).train()
    with pytest.raises(Gd4dError, match='torch_ops'):
        mod.forward_levels([torch.zeros(1, 2, 256, 4, 4, device=DEV)], _metas(2))
    both = DepthNet(256, 256, 80, torch_ops=True, hip_train=True).to(DEV).train()   # torch_ops wins: context_conv aside, autograd's graph
    out = both.forward_levels([torch.randn(1, 2, 256, 4, 4, device=DEV)], _metas(2))[0]
    assert out.grad_fn is not None and 'DepthNetTrain' not in type(out.grad_fn).__name__
    big = DepthNet(128, 128, 80, hip_train=True).to(DEV).train()
    with pytest.raises(Gd4dError, match='torch_ops'):
        big.forward_levels([torch.zeros(1, 2, 128, 4, 4, device=DEV)], _metas(2))
