"""VoVNet training on the library's kernels (gd4d_vovnet_train.hip, vovnet.py hip_train=True) against the fp64 closed form
(vovnet_train_ref.py) linearised at the DEVICE'S OWN forward maps: the ReLU masks, gate branches and pool indices are the device's
decisions, so no entry is excluded (the convention of test_depth_net_train_gpu.py).  GPU only.

Shapes: N = 2 and the forward tests' shapes - 13 x 21 is two ragged pixel tiles each way, 5 x 7 one ragged tile; (1024, 224) and the
2144-channel aggregation (67 row blocks of 32, a prime) are stage 5's own.
Tolerances: KERNEL_TOL = 1e-4 of a gradient's largest |entry| per kernel (test_fpn_train_gpu.py); one module (L + 3) x
KERNEL_TOL, the longest chain of backward kernels in front of any gradient (eSE, aggregation, L chain steps, a weight gradient),
accumulated linearly as the forward tests do over modules; a whole network that, times the modules between a parameter and the loss.

For the record, one run on an MI355X (docs/measurements_r29.md): kernels 1.8e-07 .. 7.1e-06, one module 1.2e-05; whole networks, the
worst parameter gradient as a fraction of its bound, HIP route | fp32 torch-op route against the same fp64: fixture 0.014 | 0.002, V-99
0.013 | 0.015 (the fp64 is linearised at the HIP route's maps: the torch-op route's figure includes where its own forward branches
differently)."""
import functools

import pytest
import torch

import vovnet_ref as R
import vovnet_train_ref as T
from golden_io import Golden

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
N = 2
KERNEL_TOL = 1e-4
# (cin, cout, h, w)
CONV_CASES = [(64, 64, 13, 21), (128, 128, 5, 7), (256, 160, 13, 21), (160, 160, 5, 7), (224, 224, 13, 21), (1024, 224, 5, 7), (32, 32, 5, 7)]
# (source channels, cout, h, w, the first map is a slice of a larger buffer)
OSA_CASES = [((128,) * 6, 256, 13, 21, False), ((256,) + (160,) * 5, 512, 13, 21, True), ((1024,) + (224,) * 5, 1024, 5, 7, False),
             ((64,), 32, 5, 7, False)]
ESE_CASES = [(256, 13, 21), (1024, 5, 7), (32, 1, 2)]


def _rand(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _tilings(c):
    return [mt for mt in (1, 2, 3, 4, 5, 7) if (c // 32) % mt == 0]


def _bn(c, seed):
    """randomize_'s statistics: gamma, beta, running mean, running var."""
    g = torch.Generator().manual_seed(seed)
    return (1.0 + 0.25 * (torch.rand(c, generator=g) - 0.5), 0.5 * torch.randn(c, generator=g), 0.2 * torch.randn(c, generator=g),
            0.75 + 0.5 * torch.rand(c, generator=g))


def _bn_dev(gamma, beta, mean, var):
    rstd = torch.rsqrt(var + R.EPS)
    return torch.stack((gamma * rstd, rstd, mean)).contiguous().to(DEV)


def _check(what, got, ref, bound=KERNEL_TOL):
    err = T.rel_err(got, ref)
    print(f'{what}: rel_err {err:.3e} (bound {bound:.1e})')
    assert err <= bound, what
    return err


def _guarded(shape, pad=64):
    """A map inside a larger buffer of NaNs, and the check that nothing beyond the map was written."""
    numel = 1
    for s in shape:
        numel *= s
    big = torch.full((numel + 2 * pad,), float('nan'), device=DEV)
    view = big[pad:pad + numel].view(shape)

    def untouched():
        return bool(torch.isnan(big[:pad]).all() and torch.isnan(big[pad + numel:]).all())
    return view, untouched


# ---- 1. kernels ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _conv_case(cin, cout, h, w):
    x = torch.relu(_rand(N, cin, h, w, seed=1))
    weight = _rand(cout, cin, 3, 3, seed=2, scale=(2.0 / (9 * cin)) ** 0.5)
    bn = _bn(cout, 3)
    dz = _rand(N, cout, h, w, seed=4) * (_rand(N, cout, h, w, seed=5) > 0)     # a masked gradient, as behind a ReLU
    add, mask, add2 = _rand(N, cin, h, w, seed=6), _rand(N, cin, h, w, seed=7), _rand(N, cin, h, w, seed=8)
    return x, weight, bn, dz, add, mask, add2


@pytest.mark.parametrize('case', CONV_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_conv3x3_dgrad_against_fp64(case):
    from graph_detr4d_amd import ops
    cin, cout, h, w = case
    x, weight, (gamma, beta, mean, var), dz, add, mask, add2 = _conv_case(*case)
    scale = (gamma * torch.rsqrt(var + R.EPS)).to(DEV)
    image_t = ops.conv3x3_image_t(weight.to(DEV), scale)
    ddz, dadd, dmask, dadd2 = (t.to(DEV) for t in (dz, add, mask, add2))
    plain = T.conv_data_grad(dz.double(), weight, gamma, var)
    variants = {'plain': ({}, plain),
                'add+mask': (dict(add=dadd, mask=dmask), (plain + add.double()) * (mask > 0)),
                'add+add2': (dict(add=dadd, add2=dadd2), plain + add.double() + add2.double()),
                'add+mask+add2': (dict(add=dadd, mask=dmask, add2=dadd2), (plain + add.double()) * (mask > 0) + add2.double())}
    for name, (kw, ref) in variants.items():
        out, untouched = _guarded((N, cin, h, w))
        assert ops.conv3x3_dgrad(ddz, image_t, cin, out=out, **kw) is out
        torch.cuda.synchronize()
        assert untouched()
        _check(f'conv3x3_dgrad {case} {name}', out, ref)
        assert torch.equal(out, ops.conv3x3_dgrad(ddz, image_t, cin, **kw))                          # two runs, the same bits
        for mt in _tilings(cin):                                                                     # ... and every M tiling
            assert torch.equal(out, ops.conv3x3_dgrad(ddz, image_t, cin, m_blocks=mt, **kw)), (name, mt)
    acc = dadd.clone()                                                                               # in place on `add`
    ops.conv3x3_dgrad(ddz, image_t, cin, add=acc, mask=dmask, out=acc)
    assert torch.equal(acc, ops.conv3x3_dgrad(ddz, image_t, cin, add=dadd, mask=dmask))


@pytest.mark.parametrize('case', CONV_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_conv3x3_wgrad_against_fp64(case):
    from graph_detr4d_amd import ops
    cin, cout, h, w = case
    x, weight, (gamma, beta, mean, var), dz, *_ = _conv_case(*case)
    refs = T.conv_param_grads(dz.double(), x.double(), weight, gamma, beta, mean, var)
    args = (dz.to(DEV), x.to(DEV), weight.to(DEV), _bn_dev(gamma, beta, mean, var))
    got = ops.conv3x3_wgrad(*args)
    torch.cuda.synchronize()
    for name, a, r in zip(('dW', 'dgamma', 'dbeta'), got, refs):
        assert a.shape == r.shape
        _check(f'conv3x3_wgrad {case} {name}', a, r)
    again = ops.conv3x3_wgrad(*args)
    assert all(torch.equal(a, b) for a, b in zip(got, again))                                        # no atomics
    for parts in (1, 3):                                                                             # 4 tiles (13 x 21) or 2 (5 x 7)
        other = ops.conv3x3_wgrad(*args, partitions=parts)
        for name, a, r in zip(('dW', 'dgamma', 'dbeta'), other, refs):
            _check(f'conv3x3_wgrad {case} {name}, {parts} partitions', a, r)
    only = ops.conv3x3_wgrad(*args, want=(False, True, False))
    assert only[0] is None and only[2] is None and torch.equal(only[1], got[1])


@functools.lru_cache(maxsize=None)
def _osa_case(chans, cout, h, w):
    srcs = [torch.relu(_rand(N, c, h, w, seed=10 + i)) for i, c in enumerate(chans)]
    k = sum(chans)
    weight = _rand(cout, k, 1, 1, seed=20, scale=(2.0 / k) ** 0.5)
    bn = _bn(cout, 21)
    dz = _rand(N, cout, h, w, seed=22) * (_rand(N, cout, h, w, seed=23) > 0)
    return srcs, weight, bn, dz


_OSA_IDS = lambda c: f'{c[0][0]}+{len(c[0]) - 1}x{c[0][-1]}-{c[1]}-{c[2]}x{c[3]}'                      # noqa: E731


@pytest.mark.parametrize('case', OSA_CASES, ids=_OSA_IDS)
def test_osa_concat_dgrad_against_fp64(case):
    from graph_detr4d_amd import ops
    chans, cout, h, w, _ = case
    srcs, weight, (gamma, beta, mean, var), dz = _osa_case(chans, cout, h, w)
    scale = (gamma * torch.rsqrt(var + R.EPS)).to(DEV)
    image_t = ops.osa_concat_image_t(weight.to(DEV), scale)
    ddz, mask = dz.to(DEV), srcs[-1].to(DEV)
    refs = list(T.conv_data_grad(dz.double(), weight, gamma, var).split(list(chans), dim=1))
    for masked in (False, True):
        want = refs[:-1] + [refs[-1] * (srcs[-1] > 0)] if masked else refs
        guarded = [_guarded((N, c, h, w)) for c in chans]                      # every destination its own buffer, NaNs around it
        outs = ops.osa_concat_dgrad(ddz, image_t, chans, mask_last=mask if masked else None, outs=[v for v, _ in guarded])
        torch.cuda.synchronize()
        for i, (o, r) in enumerate(zip(outs, want)):
            assert guarded[i][1](), f'memory beyond destination {i} was written'
            _check(f'osa_concat_dgrad {chans} <- {cout} at {h} x {w}, map {i}, masked {masked}', o, r)
        again = ops.osa_concat_dgrad(ddz, image_t, chans, mask_last=mask if masked else None)
        assert all(torch.equal(a, b) for a, b in zip(outs, again))
        common = [mt for mt in (1, 2, 3, 4, 5, 7) if all((c // 32) % mt == 0 for c in chans)]
        for mt in common:                                                      # (1024 + 5 x 224: only 1 divides 32 and 7)
            forced = ops.osa_concat_dgrad(ddz, image_t, chans, mask_last=mask if masked else None, m_blocks=mt)
            assert all(torch.equal(a, b) for a, b in zip(outs, forced)), mt


@pytest.mark.parametrize('case', OSA_CASES, ids=_OSA_IDS)
def test_osa_concat_wgrad_against_fp64(case):
    from graph_detr4d_amd import ops
    chans, cout, h, w, sliced = case
    srcs, weight, (gamma, beta, mean, var), dz = _osa_case(chans, cout, h, w)
    refs = T.conv_param_grads(dz.double(), torch.cat(srcs, dim=1).double(), weight, gamma, beta, mean, var)
    dsrcs = [s.to(DEV) for s in srcs]
    if sliced:                                                                 # its own base pointer inside a larger buffer
        big = torch.full((N + 1, chans[0], h, w), float('nan'), device=DEV)
        big[1:] = dsrcs[0]
        dsrcs[0] = big[1:]
        assert dsrcs[0].is_contiguous() and dsrcs[0].data_ptr() != big.data_ptr()
    ddz = dz.to(DEV)
    args = (ddz, ddz.sum(dim=(2, 3)), dsrcs, weight.to(DEV), _bn_dev(gamma, beta, mean, var))
    got = ops.osa_concat_wgrad(*args)
    torch.cuda.synchronize()
    for name, a, r in zip(('dW', 'dgamma', 'dbeta'), got, refs):
        assert a.shape == r.shape
        _check(f'osa_concat_wgrad {chans} -> {cout} at {h} x {w} {name}', a, r)
    assert all(torch.equal(a, b) for a, b in zip(got, ops.osa_concat_wgrad(*args)))
    for parts in (1, 3):
        for name, a, r in zip(('dW', 'dgamma', 'dbeta'), ops.osa_concat_wgrad(*args, partitions=parts), refs):
            _check(f'osa_concat_wgrad {chans} -> {cout} {name}, {parts} partitions', a, r)


@pytest.mark.parametrize('case', ESE_CASES, ids=lambda c: f'{c[0]}-{c[1]}x{c[2]}')
def test_ese_bwd_against_fp64(case):
    from graph_detr4d_amd import ops
    c, h, w = case
    xt = torch.relu(_rand(N, c, h, w, seed=30))
    dout = _rand(N, c, h, w, seed=31)
    fc_w = _rand(c, c, 1, 1, seed=32, scale=c ** -0.5)
    fc_b = _rand(c, seed=33, scale=0.5)
    fc_b[0::7], fc_b[3::7] = 8.0, -8.0                                         # gates of exactly 1 and exactly 0
    flat = xt.reshape(N, c, h * w)
    partials = torch.stack([t.sum(dim=2) for t in flat.split(128, dim=2)], dim=1).contiguous().to(DEV)
    gate = ops.ese_gate(partials, h * w, fc_w.to(DEV), fc_b.to(DEV))           # the device's own gate: its branches are the ones taken
    assert (gate == 0).any() and (gate == 1).any() and ((gate > 0) & (gate < 1)).any()
    ref_dz, ref_w, ref_b = T.ese_backward(dout.double(), xt.double(), gate.cpu().double(), fc_w)
    args = (dout.to(DEV), xt.to(DEV), partials, gate, fc_w.to(DEV))
    dz, sums, dfc_w, dfc_b = ops.ese_bwd(*args)
    torch.cuda.synchronize()
    tag = f'ese_bwd C = {c}, HW = {h * w}'
    _check(f'{tag} dz', dz, ref_dz)
    _check(f'{tag} plane sums', sums, ref_dz.sum(dim=(2, 3)))
    _check(f'{tag} dfc_w', dfc_w, ref_w)
    _check(f'{tag} dfc_b', dfc_b, ref_b)
    assert float(dfc_b[gate.sum(0) == N].abs().max()) == 0                      # a channel saturated in every image passes nothing
    again = ops.ese_bwd(*args)
    assert all(torch.equal(a, b) for a, b in zip((dz, sums, dfc_w, dfc_b), again))
    none = ops.ese_bwd(*args, want_fc=(False, False))
    assert none[2] is None and none[3] is None and torch.equal(none[0], dz) and torch.equal(none[1], sums)


# ---- 2. one OSA module through the class ------------------------------------------------------------------------------------------
def _module(identity, **kw):
    from graph_detr4d_amd import vovnet
    in_ch, stage_ch, concat_ch = (256, 160, 256) if identity else (128, 128, 256)
    m = R.randomize_(vovnet._OSA_module(in_ch, stage_ch, concat_ch, 5, 'OSA3_2', identity=identity, hip_train=True, **kw), seed=40).eval()
    x = torch.relu(_rand(N, in_ch, 13, 21, seed=41))
    dout = _rand(N, concat_ch, 13, 21, seed=42)
    return m.to(DEV), x.to(DEV), dout.to(DEV)


def _run(m, x, dout):
    """One forward + backward: (dx, {name: grad})."""
    m.zero_grad(set_to_none=True)
    x = x.detach().clone().requires_grad_(True)
    m(x).backward(dout)
    return x.grad, {k: (None if p.grad is None else p.grad.clone()) for k, p in m.named_parameters()}


@pytest.mark.parametrize('identity', [False, True], ids=['plain', 'identity'])
def test_osa_module_gradients_against_fp64(identity):
    m, x, dout = _module(identity)
    bound = (5 + 3) * KERNEL_TOL
    with torch.no_grad():
        maps, xt, _, gate, out = m.forward_maps(x)                              # the same launches as the node's: the device's maps
    assert (gate == 0).any() and (gate == 1).any() and ((gate > 0) & (gate < 1)).any()
    x_req = x.detach().clone().requires_grad_(True)
    assert torch.equal(m(x_req), out)                                          # the node's forward is the inference route's, bit for bit
    dx, grads = _run(m, x, dout)
    torch.cuda.synchronize()
    ref_dx, ref = T.osa_backward({k: v.cpu() for k, v in m.state_dict().items()}, '', 'OSA3_2', maps, xt, gate, dout, identity)
    _check(f'_OSA_module identity={identity} dx', dx, ref_dx, bound)
    assert set(grads) == set(ref)
    for k in sorted(ref):
        assert grads[k].shape == ref[k].shape
        _check(f'_OSA_module identity={identity} {k}', grads[k], ref[k], bound)
    dx2, grads2 = _run(m, x, dout)                                              # two runs, the same bits
    assert torch.equal(dx, dx2) and all(torch.equal(grads[k], grads2[k]) for k in grads)
    # with_cp in train() mode: only the input is kept, the forward launches run again in backward - the same bits
    m.with_cp = True
    m.train()
    for b in m._norms:
        b.eval()
    dx3, grads3 = _run(m, x, dout)
    assert torch.equal(dx, dx3) and all(torch.equal(grads[k], grads3[k]) for k in grads)


def test_osa_module_frozen_parameters_and_dtypes(monkeypatch):
    from graph_detr4d_amd import ops
    m, x, dout = _module(False)
    dx, grads = _run(m, x, dout)
    calls = dict(wgrad=0, dgrad=0, fc=[])
    for name, key in (('conv3x3_wgrad', 'wgrad'), ('conv3x3_dgrad', 'dgrad')):
        def counted(*a, _f=getattr(ops, name), _k=key, **kw):
            calls[_k] += 1
            return _f(*a, **kw)
        monkeypatch.setattr(ops, name, counted)

    def ese(*a, _f=ops.ese_bwd, **kw):
        calls['fc'].append(kw.get('want_fc'))
        return _f(*a, **kw)
    monkeypatch.setattr(ops, 'ese_bwd', ese)
    m.ese.fc.requires_grad_(False)
    m.layers[0].requires_grad_(False)
    dx2, grads2 = _run(m, x, dout)
    assert calls == dict(wgrad=4, dgrad=5, fc=[(False, False)])                 # layer 0's and ese.fc's launches are skipped
    frozen = [k for k in grads if k.startswith(('ese.fc', 'layers.0.'))]
    assert len(frozen) == 5 and all(grads2[k] is None for k in frozen)
    assert torch.equal(dx, dx2) and all(torch.equal(grads[k], grads2[k]) for k in grads if k not in frozen)
    # an input that needs no gradient: the chain stops at the lowest layer that does
    calls.update(wgrad=0, dgrad=0)
    m.zero_grad(set_to_none=True)
    m(x).backward(dout)
    assert calls['wgrad'] == 4 and calls['dgrad'] == 3 and torch.equal(m.layers[1][0].weight.grad, grads['layers.1.OSA3_2_1/conv.weight'])
    # an fp16 input gets an fp16 gradient
    m.requires_grad_(True)
    xh = x.half().requires_grad_(True)
    m(xh).backward(dout)
    assert xh.grad.dtype == torch.float16 and T.rel_err(xh.grad, _run(m, x.half().float(), dout)[0]) <= 1e-3


# ---- 3. whole networks -----------------------------------------------------------------------------------------------------------
STAGES = ('stage2', 'stage3', 'stage4', 'stage5')


def _recorded(net):
    """Wraps every OSA module's forward_maps so that the maps of its training node are kept: {prefix: (maps, xt, partials, gate, out)}."""
    from graph_detr4d_amd import vovnet
    rec = {}
    for name, m in net.named_modules():
        if isinstance(m, vovnet._OSA_module):
            def wrapped(x, keep=True, _f=m.forward_maps, _k=name + '.'):
                res = _f(x, keep)
                if keep:
                    rec[_k] = res
                return res
            m.forward_maps = wrapped
    return rec


def _network_check(net, image, tag, frozen_stages=-1):
    """Forward + backward of `net` (hip_train, train() mode) with a fixed random cotangent per output; every parameter gradient and the
    image gradient against the closed form chained over the modules, and the fp32 torch-op route's error against the same fp64."""
    import copy
    from graph_detr4d_amd import functional as Fn
    sd = {k: v.cpu() for k, v in net.state_dict().items()}
    mods = T.module_names(sd)
    first_stage = frozen_stages + 2 if frozen_stages >= 0 else 2
    rec = _recorded(net)
    x = image.to(DEV).requires_grad_(frozen_stages < 0)
    outs = net(x)
    couts = [_rand(*o.shape, seed=90 + i).to(DEV) for i, o in enumerate(outs)]

    def backward(outs):                                                        # (a frozen stage's output has no graph behind it)
        torch.autograd.backward(*zip(*[(o, c) for o, c in zip(outs, couts) if o.requires_grad]))
    backward(outs)
    torch.cuda.synchronize()
    trained = [prefix for s, prefix, _, _ in mods if s >= first_stage]
    assert sorted(rec) == sorted(trained)                                      # the others took the inference launches
    hip = {k: (None if p.grad is None else p.grad.clone()) for k, p in net.named_parameters()}
    stem = None if frozen_stages >= 0 else copy.deepcopy(net.stem).cpu().double()
    ref, ref_dx = T.network_backward(sd, stem, image, rec, {int(f[-1]): c for f, c in zip(STAGES, couts)}, first_stage)
    # the torch-op route on the same inputs, for the record
    net.zero_grad(set_to_none=True)
    xt = image.to(DEV).requires_grad_(frozen_stages < 0)
    with Fn.torch_ops_for(net):
        backward(net(xt))
    torch.cuda.synchronize()
    tor = {k: p.grad for k, p in net.named_parameters()}
    layers = max(int(m.group(1)) for k in sd for m in [__import__('re').search(r'layers\.(\d+)\.', k)] if m) + 1
    per_module = (layers + 3) * KERNEL_TOL
    after = {prefix: len(mods) - i for i, (_, prefix, _, _) in enumerate(mods)}   # modules from this one to the last, inclusive
    worst = (0.0, 0.0, '')
    for k in sorted(hip):
        prefix = next((p for p in after if k.startswith(p)), None)
        if k not in ref:
            assert hip[k] is None and prefix not in trained, k                 # a frozen stage: no gradient
            continue
        bound = per_module * (after[prefix] if prefix else len(mods) + 1)     # (the stem sits behind every module)
        e_hip, e_tor = T.rel_err(hip[k], ref[k]), T.rel_err(tor[k], ref[k])
        if e_hip / bound > worst[0]:
            worst = (e_hip / bound, e_tor / bound, k)
        assert e_hip <= bound, f'{tag} {k}: {e_hip:.3e} > {bound:.1e} (torch ops {e_tor:.3e})'
    print(f'{tag}: {len(ref)} parameter gradients; the worst against its bound: {worst[2]} at {worst[0]:.3f} of it on the HIP route '
          f'(the fp32 torch-op route: {worst[1]:.3f})')
    if frozen_stages < 0:
        bound = per_module * (len(mods) + 1)
        e_hip, e_tor = T.rel_err(x.grad, ref_dx), T.rel_err(xt.grad, ref_dx)
        print(f'{tag}: image gradient HIP route {e_hip:.3e}, torch-op route {e_tor:.3e} (bound {bound:.1e})')
        assert e_hip <= bound
    else:
        assert x.grad is None


def test_fixture_network_gradients(monkeypatch):
    from graph_detr4d_amd import vovnet
    g = Golden('vovnet_tiny')
    monkeypatch.setitem(vovnet._STAGE_SPECS, g.meta['spec_name'], g.meta['spec'])
    net = vovnet.VoVNetCP(g.meta['spec_name'], out_features=STAGES, norm_eval=True, hip_train=True)
    net.load_state_dict(g.state(), strict=True)
    _network_check(net.to(DEV).train(), g.t('img').float() / g.meta['feat_scale'], 'fixture network')


@pytest.mark.parametrize('frozen_stages', [-1, 2], ids=['all', 'frozen_stages=2'])
def test_v99_gradients(frozen_stages):
    from graph_detr4d_amd import VoVNetCP
    net = R.randomize_(VoVNetCP('V-99-eSE', out_features=STAGES, norm_eval=True, frozen_stages=frozen_stages, hip_train=True), seed=70)
    _network_check(net.to(DEV).train(), _rand(N, 3, 52, 84, seed=71), f'V-99 frozen_stages={frozen_stages}', frozen_stages)
