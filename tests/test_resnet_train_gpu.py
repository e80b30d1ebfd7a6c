"""ResNet training on the library's kernels (gd4d_resnet_train.hip, backbones.py plain_train=True) against the fp64 closed form
(resnet_train_ref.py) linearised at the DEVICE'S OWN forward maps: every ReLU mask is the device's decision, so no entry is excluded
(the convention of test_vovnet_train_gpu.py).  GPU only.

Shapes: resnet_train_cases.py (N = 2, the smallest at which a tile count, a parity or a channel block can go wrong).
Tolerances: KERNEL_TOL = 1e-4 of a gradient's largest |entry| per kernel (test_fpn_train_gpu.py).  A block: KERNEL_TOL times
the backward kernels on the longest chain in front of any of its gradients -
    Bottleneck   4   the mask pass, conv3's and conv2's data gradients, then conv1's data gradient (dx) or its weight gradient; the
                     downsample's adjoint runs beside that chain and enters conv1's epilogue
    BasicBlock   3   the mask pass, conv2's data gradient, then conv1's data or weight gradient
    DCN block    6   the tail's mask pass and conv3's data gradient, the DCN layer's data gradient and its offset convolution's, the
                     head's mask pass, then conv1's data or weight gradient
- and a network that, accumulated linearly over the blocks between a parameter and the loss, as test_vovnet_train_gpu.py does over
modules."""
import copy

import pytest
import torch

import resnet_ref as R
import resnet_train_cases as C
import resnet_train_ref as T

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
N = C.N
KERNEL_TOL = C.KERNEL_TOL
CHAIN = {'Bottleneck': 4, 'BasicBlock': 3, 'dcn': 6}
DCN = dict(type='DCNv2', deform_groups=1, fallback_on_stride=False)


def _check(what, got, ref, bound=KERNEL_TOL):
    err = T.rel_err(got, ref)
    print(f'{what}: rel_err {err:.3e} (bound {bound:.1e})')
    assert err <= bound, what
    return err


def _tilings(c):
    return [mt for mt in (1, 2, 3, 4, 5, 7) if (c // 32) % mt == 0]


def _scale(bn):
    return (bn[0] * torch.rsqrt(bn[3] + T.EPS)).to(DEV)


# ---- 1. kernels ------------------------------------------------------------------------------------------------------------
def _dgrad(taps, cin, cout, stride, h, w, even):
    from graph_detr4d_amd import ops
    weight, bn, dz, operands, variants = C.dgrad_case(taps, cin, cout, stride, h, w, even)
    dev = {k: v.to(DEV) for k, v in operands.items()}
    ddz = dz.to(DEV)
    if taps == 9:
        image_t = ops.conv3x3_act_image_t(weight.to(DEV), _scale(bn))
        run = lambda **kw: ops.conv3x3_act_dgrad(ddz, image_t, cin, hw=(h, w), stride=stride, **kw)          # noqa: E731
    else:
        image_t = ops.conv1x1_image_t(weight.to(DEV), _scale(bn))
        run = lambda **kw: ops.conv1x1_dgrad(ddz, image_t, cin, **kw)                                         # noqa: E731
    tag = f'{"conv3x3_act" if taps == 9 else "conv1x1"}_dgrad {(cin, cout, stride, h, w)}'
    for name, (names, ref) in variants.items():
        kw = {k: dev[k] for k in names}
        out = run(**kw)
        torch.cuda.synchronize()
        assert tuple(out.shape) == (N, cin, h, w)
        _check(f'{tag} {name}', out, ref)
        assert torch.equal(out, run(**kw))                                                   # two runs, the same bits
        for mt in _tilings(cin):                                                             # ... and every M tiling
            assert torch.equal(out, run(m_blocks=mt, **kw)), (name, mt)
    acc = dev['add'].clone()                                                                 # in place on `add`
    run(add=acc, mask=dev['mask'], out=acc)
    assert torch.equal(acc, run(add=dev['add'], mask=dev['mask']))


@pytest.mark.parametrize('case', C.PW_DGRAD_CASES, ids=C.case_id)
def test_conv1x1_dgrad_against_fp64(case):
    cin, cout, h, w, even = case
    _dgrad(1, cin, cout, 1, h, w, even)


@pytest.mark.parametrize('case', C.C3_DGRAD_CASES, ids=C.case_id)
def test_conv3x3_act_dgrad_against_fp64(case):
    cin, cout, stride, h, w, even = case
    _dgrad(9, cin, cout, stride, h, w, even)


@pytest.mark.parametrize('case', C.WGRAD_CASES, ids=C.case_id)
def test_wgrad_against_fp64(case):
    from graph_detr4d_amd import _lib, ops
    taps, cin, cout, stride, h, w = case
    x, weight, bn, dz, refs = C.wgrad_case(*case)
    run = ops.conv3x3_act_wgrad if taps == 9 else ops.conv1x1_wgrad
    args = (dz.to(DEV), x.to(DEV), weight.to(DEV), C.bn_stats(bn).to(DEV))
    got = run(*args, stride=stride)
    torch.cuda.synchronize()
    for name, a, r in zip(('dW', 'dgamma', 'dbeta'), got, refs):
        assert a.shape == r.shape
        _check(f'wgrad {case} {name}', a, r)
    assert all(torch.equal(a, b) for a, b in zip(got, run(*args, stride=stride)))              # no atomics
    tiles = int(_lib.load().gd4d_resnet_wgrad_tiles(taps, N, h, w, stride))
    for parts in (1, tiles + 3):                                                              # one partition; empty ones store zeros
        for name, a, r in zip(('dW', 'dgamma', 'dbeta'), run(*args, stride=stride, partitions=parts), refs):
            _check(f'wgrad {case} {name}, {parts} partitions of {tiles} tiles', a, r)
    only = run(*args, stride=stride, want=(False, True, False))
    assert only[0] is None and only[2] is None and torch.equal(only[1], got[1])


def test_mask_and_scatter_kernels():
    from graph_detr4d_amd import ops
    dout, out = C.rand(N, 32, 9, 11, seed=1).to(DEV), torch.relu(C.rand(N, 32, 9, 11, seed=2)).to(DEV)
    assert torch.equal(ops.relu_mask_bwd(dout, out), dout * (out > 0))
    for h, w in ((9, 11), (8, 12), (1, 1)):
        src = C.rand(N, 32, *C.half(h, w), seed=3).to(DEV)
        ref = torch.zeros(N, 32, h, w, device=DEV)
        ref[:, :, ::2, ::2] = src
        assert torch.equal(ops.even_pixels_scatter(src, (h, w)), ref)


# ---- 2. blocks through the classes ---------------------------------------------------------------------------------------------
def _block(kind, inplanes, planes, stride, seed, dcn=None):
    import graph_detr4d_amd as G
    block = G.Bottleneck if kind == 'Bottleneck' else G.BasicBlock
    kw = dict(plain_kernels=True, plain_train=True, hip_train=dcn is not None)
    norm_cfg = None if dcn is None else _frozen_bn()          # (the DCN layer's folded epilogue has no gradient for bn2's parameters)
    if stride != 1 or inplanes != planes * block.expansion:
        blk = G.ResNet._make_stage(inplanes, planes, 1, stride, 1, norm_cfg, dcn, False, kw['hip_train'], block, True, True)[0]
    else:
        blk = block(inplanes, planes, norm_cfg=norm_cfg, dcn=dcn, **kw)
    return R.randomize_(blk, seed=seed).eval().to(DEV)


def _device_maps(blk, x):
    """(x, a1 (, a2), out): the inference launches, unit by unit - the maps the training node records."""
    with torch.no_grad():
        if not getattr(blk, 'with_dcn', False):
            return blk.forward_maps(x)
        a1 = blk._conv('conv1', x, blk.conv1, blk.bn1)
        a2 = blk.conv2.forward_bn_relu(a1, blk.bn2)
        identity = x if blk.downsample is None else blk._conv('downsample', x, *blk.downsample, relu=False)
        return x, a1, a2, blk._conv('conv3', a2, blk.conv3, blk.bn3, identity=identity)


def _run(blk, x, dout):
    blk.zero_grad(set_to_none=True)
    x = x.detach().clone().requires_grad_(True)
    out = blk(x)
    out.backward(dout)
    return out.detach(), x.grad, {k: (None if p.grad is None else p.grad.clone()) for k, p in blk.named_parameters()}


# (kind, inplanes, planes, stride, H, W)
BLOCK_CASES = [('Bottleneck', 256, 64, 1, 13, 21), ('Bottleneck', 256, 128, 2, 13, 21), ('BasicBlock', 64, 64, 1, 13, 21),
               ('BasicBlock', 64, 128, 2, 13, 21)]


@pytest.mark.parametrize('case', BLOCK_CASES, ids=lambda c: '-'.join(map(str, c)))
def test_plain_block_gradients_against_fp64(case):
    kind, inplanes, planes, stride, h, w = case
    blk = _block(kind, inplanes, planes, stride, seed=40)
    assert (blk.downsample is not None) == (stride == 2)
    x = torch.relu(C.rand(N, inplanes, h, w, seed=41)).to(DEV)
    maps = _device_maps(blk, x)
    dout = C.rand(*maps[-1].shape, seed=42).to(DEV)
    with torch.no_grad():
        infer = blk(x)
    out, dx, grads = _run(blk, x, dout)
    torch.cuda.synchronize()
    assert torch.equal(out, infer) and torch.equal(out, maps[-1])              # the node's forward is the inference route's, bit for bit
    bound = CHAIN[kind] * KERNEL_TOL
    ref_dx, ref = T.block_backward({k: v.cpu() for k, v in blk.state_dict().items()}, '', maps, dout, stride)
    _check(f'{case} dx', dx, ref_dx, bound)
    assert set(grads) == set(ref)
    for k in sorted(ref):
        assert grads[k].shape == ref[k].shape
        _check(f'{case} {k}', grads[k], ref[k], bound)
    out2, dx2, grads2 = _run(blk, x, dout)                                      # two runs, the same bits
    assert torch.equal(dx, dx2) and all(torch.equal(grads[k], grads2[k]) for k in grads)
    # an input that needs no gradient and a frozen conv1: no data gradient below the lowest unit that asks
    blk.conv1.requires_grad_(False)
    blk.bn1.requires_grad_(False)
    blk.zero_grad(set_to_none=True)
    blk(x).backward(dout)
    assert blk.conv1.weight.grad is None and torch.equal(blk.conv2.weight.grad, grads['conv2.weight'])
    # an fp16 input gets an fp16 gradient
    blk.requires_grad_(True)
    xh = x.half().requires_grad_(True)
    blk(xh).backward(dout)
    assert xh.grad.dtype == torch.float16 and T.rel_err(xh.grad, _run(blk, x.half().float(), dout)[1]) <= 1e-3


@pytest.mark.parametrize('stride', [1, 2], ids=['s1', 's2'])
def test_dcn_block_gradients_against_fp64(stride):
    blk = _block('Bottleneck', 256, 128 if stride == 2 else 64, stride, seed=50, dcn=DCN)
    if stride == 1:
        assert blk.downsample is None
    x = torch.relu(C.rand(N, 256, 13, 21, seed=51)).to(DEV)
    maps = _device_maps(blk, x)
    dout = C.rand(*maps[-1].shape, seed=52).to(DEV)
    out, dx, grads = _run(blk, x, dout)
    torch.cuda.synchronize()
    assert torch.equal(out, maps[-1])
    bound = CHAIN['dcn'] * KERNEL_TOL
    sd = {k: v.cpu() for k, v in blk.state_dict().items()}
    _, a1, a2, _ = maps
    da2, r, ref = T.tail_backward(sd, '', a2, x, out, dout, stride)
    conv2 = copy.deepcopy(blk.conv2).cpu().double()
    da1, dcn_grads = T.dcn_unit_backward(conv2, copy.deepcopy(blk.bn2).cpu().double(), a1, a2, da2)
    head_dx, head = T.head_backward(sd, '', x, a1, da1)
    ref.update(head)
    ref.update(dcn_grads)
    _check(f'DCN block stride {stride} dx', dx, head_dx + r, bound)
    trained = {'conv1.weight', 'conv2.weight', 'conv2.conv_offset.weight', 'conv2.conv_offset.bias', 'conv3.weight'}
    trained |= {'downsample.0.weight'} if stride == 2 else set()
    assert {k for k, g in grads.items() if g is not None} == trained           # frozen BatchNorms: no gradient
    for k in sorted(trained):
        _check(f'DCN block stride {stride} {k}', grads[k], ref[k], bound)


# ---- 3. whole networks -----------------------------------------------------------------------------------------------------------
def _recorded(net):
    """Wraps every routed block so that the maps of its training forward are kept: {prefix: maps}."""
    rec = {}
    for name, m in net._routed():
        def wrapped(x, _m=m, _f=m._hip_train, _k=name + '.'):
            rec[_k] = _device_maps(_m, x.detach())
            return _f(x)
        m._hip_train = wrapped
    return rec


def _network_check(net, image, tag, dcn=False):
    from graph_detr4d_amd import functional as Fn
    sd = {k: v.cpu() for k, v in net.state_dict().items()}
    blocks = T.block_names(sd)
    rec = _recorded(net)
    outs = net(image.to(DEV))
    # the frozen layer1 runs the inference launches: no node is built
    assert outs[0].grad_fn is None and not outs[0].requires_grad and all(o.grad_fn is not None for o in outs[1:])
    assert sorted(rec) == sorted(p for layer, _, p, _ in blocks if layer >= 2)
    with torch.no_grad():
        for o, i in zip(outs, net.eval()(image.to(DEV))):                     # the training route's forward: the inference route's bits
            assert torch.equal(o, i)
        net.train()
    couts = {i + 1: C.rand(*o.shape, seed=90 + i).to(DEV) for i, o in enumerate(outs)}

    def backward(outs):
        torch.autograd.backward(outs[1:], [couts[i] for i in (2, 3, 4)])
    backward(outs)
    torch.cuda.synchronize()
    hip = {k: (None if p.grad is None else p.grad.clone()) for k, p in net.named_parameters()}
    dcn_layers = {}
    if dcn:
        for name, m in net._routed():
            if getattr(m, 'with_dcn', False):
                dcn_layers[name + '.'] = (copy.deepcopy(m.conv2).cpu().double(), copy.deepcopy(m.bn2).cpu().double())
    ref = T.network_backward(sd, rec, couts, first_layer=2, dcn_layers=dcn_layers)
    # the fp32 torch-op route on the same inputs, for the record
    net.zero_grad(set_to_none=True)
    with Fn.torch_ops_for(net):
        backward(net(image.to(DEV)))
    torch.cuda.synchronize()
    tor = {k: p.grad for k, p in net.named_parameters()}
    kind = type(net.layer1[0]).__name__
    per_block = {p: CHAIN['dcn' if p in dcn_layers else kind] * KERNEL_TOL for _, _, p, _ in blocks}
    after = {p: sum(per_block[q] for _, _, q, _ in blocks[i:]) for i, (_, _, p, _) in enumerate(blocks)}   # from this block to the last
    worst = (0.0, 0.0, '')
    params = dict(net.named_parameters())
    for k in sorted(hip):
        if k not in ref or not params[k].requires_grad:
            assert hip[k] is None, k                                           # the stem, layer1, frozen BatchNorms: no gradient
            continue
        bound = after[next(p for p in after if k.startswith(p))]
        e_hip, e_tor = T.rel_err(hip[k], ref[k]), T.rel_err(tor[k], ref[k])
        if e_hip / bound > worst[0]:
            worst = (e_hip / bound, e_tor / bound, k)
        assert e_hip <= bound, f'{tag} {k}: {e_hip:.3e} > {bound:.1e} (torch ops {e_tor:.3e})'
    assert sum(g is not None for g in hip.values()) > 10
    print(f'{tag}: {len(ref)} parameter gradients; the worst against its bound: {worst[2]} at {worst[0]:.3f} of it on the HIP route '
          f'(the fp32 torch-op route: {worst[1]:.3f})')
    return hip


def _frozen_bn():
    return dict(type='BN', requires_grad=False)


def test_resnet18_gradients():
    import graph_detr4d_amd as G
    net = R.randomize_(G.ResNet(18, frozen_stages=1, norm_cfg=_frozen_bn(), plain_kernels=True, plain_train=True), seed=70).to(DEV).train()
    image = C.rand(2, 3, 64, 96, seed=71)
    hip = _network_check(net, image, 'ResNet-18')
    net.zero_grad(set_to_none=True)                                            # two runs, the same bits for every gradient
    outs = net(image.to(DEV))
    torch.autograd.backward(outs[1:], [C.rand(*o.shape, seed=90 + i).to(DEV) for i, o in enumerate(outs)][1:])
    for k, p in net.named_parameters():
        assert (p.grad is None and hip[k] is None) or torch.equal(p.grad, hip[k]), k


def test_resnet50_dcn_gradients():
    import graph_detr4d_amd as G
    net = R.randomize_(G.ResNet(50, frozen_stages=1, norm_cfg=_frozen_bn(), dcn=DCN, stage_with_dcn=(False, False, True, True),
                                plain_kernels=True, plain_train=True, hip_train=True), seed=72).to(DEV).train()
    _network_check(net, C.rand(1, 3, 64, 96, seed=73), 'ResNet-50 + DCN', dcn=True)
