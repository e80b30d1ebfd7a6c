"""ResNet's `plain_train` switch without a GPU: the fp64 closed-form backward (resnet_train_ref.py) of a unit, a plain block, the DCN
block's head and tail and a network against fp64 torch autograd through the default route's stock layers, and the keyword rules.  The
closed form is linearised at the fp64 forward's own maps here; the GPU tests hand it the device's.

Every case's mask maps satisfy the project's ReLU rule - at least a fifth of the entries at 0 and a fifth positive - asserted below."""
import copy

import pytest
import torch
import torch.nn.functional as F

import resnet_ref as R
import resnet_train_ref as T
from graph_detr4d_amd._lib import Gd4dError

TOL = 1e-9          # fp64 against fp64: two orders of summation


def _rand(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def _relu_rule(maps, what):
    for i, m in enumerate(maps):
        zero, pos = float((m == 0).double().mean()), float((m > 0).double().mean())
        assert zero >= 0.2 and pos >= 0.2, f'{what}: mask map {i} has {zero:.2f} at 0 and {pos:.2f} positive'


def block_maps(blk, x):
    """(x, a1 (, a2), out) of a block through its own stock layers, unit by unit."""
    a1 = F.relu(blk.bn1(blk.conv1(x)))
    identity = x if blk.downsample is None else blk.downsample(x)
    if hasattr(blk, 'conv3'):
        a2 = blk.conv2.forward_bn_relu(a1, blk.bn2) if blk.with_dcn else F.relu(blk.bn2(blk.conv2(a1)))
        return x, a1, a2, F.relu(blk.bn3(blk.conv3(a2)) + identity)
    return x, a1, F.relu(blk.bn2(blk.conv2(a1)) + identity)


def _autograd(blk, x, dout):
    blk.zero_grad(set_to_none=True)
    x = x.clone().requires_grad_(True)
    out = blk(x)
    out.backward(dout)
    return out.detach(), x.grad, {k: p.grad for k, p in blk.named_parameters()}


def _make(kind, inplanes, planes, stride, seed, **kw):
    import graph_detr4d_amd as G
    block = G.Bottleneck if kind == 'bottleneck' else G.BasicBlock
    downsample = stride != 1 or inplanes != planes * block.expansion
    if downsample:
        blk = G.ResNet._make_stage(inplanes, planes, 1, stride, 1, None, kw.pop('dcn', None), kw.pop('torch_ops', False), False, block)[0]
    else:
        blk = block(inplanes, planes, **kw)
    return R.randomize_(blk, seed=seed).eval().double()


# (kind, inplanes, planes, stride, H, W)
BLOCK_CASES = [('bottleneck', 32, 8, 1, 6, 8), ('bottleneck', 16, 8, 1, 5, 7), ('bottleneck', 16, 8, 2, 9, 11), ('bottleneck', 16, 8, 2, 8, 12),
               ('bottleneck', 32, 8, 1, 1, 1), ('bottleneck', 16, 8, 2, 1, 1),
               ('basic', 16, 16, 1, 5, 7), ('basic', 16, 16, 1, 6, 8), ('basic', 16, 32, 2, 9, 11), ('basic', 16, 32, 2, 8, 12),
               ('basic', 16, 32, 1, 5, 6), ('basic', 16, 16, 1, 1, 1), ('basic', 16, 32, 2, 1, 1)]


@pytest.mark.parametrize('case', BLOCK_CASES, ids=lambda c: '-'.join(map(str, c)))
def test_plain_block_closed_form_against_fp64_autograd(case):
    kind, inplanes, planes, stride, h, w = case
    blk = _make(kind, inplanes, planes, stride, seed=3)
    n = 2 if h * w > 1 else 8                                                  # a 1 x 1 map: more images, so that the rule has entries
    x = torch.relu(_rand(n, inplanes, h, w, seed=4))
    with torch.no_grad():
        maps = block_maps(blk, x)
    _relu_rule(maps[1:], str(case))
    dout = _rand(*maps[-1].shape, seed=5)
    out, dx, grads = _autograd(blk, x, dout)
    assert torch.equal(out, maps[-1])
    ref_dx, ref = T.block_backward(blk.state_dict(), '', maps, dout, stride)
    assert T.rel_err(dx, ref_dx) <= TOL
    assert set(ref) == set(grads)                                              # every weight, gamma and beta (dgamma / dbeta included)
    for k in ref:
        assert ref[k].shape == grads[k].shape and T.rel_err(grads[k], ref[k]) <= TOL, k


@pytest.mark.parametrize('stride,hw', [(1, (5, 7)), (2, (9, 11)), (2, (8, 12))], ids=['s1', 's2-odd', 's2-even'])
def test_unit_and_even_pixel_add(stride, hw):
    """A single unit, both kernel sizes: the strided weight and data gradients, and that a stride-2 1x1's adjoint is its stride-1
    adjoint on the half-resolution grid added at the even pixels."""
    h, w = hw
    for k in (1, 3):
        conv = torch.nn.Conv2d(16, 24, k, stride=stride, padding=k // 2, bias=False).double()
        bn = R.randomize_(torch.nn.BatchNorm2d(24), seed=6).eval().double()
        x = _rand(2, 16, h, w, seed=7).requires_grad_(True)
        y = bn(conv(x))
        dz = _rand(*y.shape, seed=8)
        y.backward(dz)
        bnp = (bn.weight, bn.bias, bn.running_mean, bn.running_var)
        dw, dgamma, dbeta = T.unit_param_grads(dz, x.detach(), conv.weight, bnp, stride)
        for got, ref in ((conv.weight.grad, dw), (bn.weight.grad, dgamma), (bn.bias.grad, dbeta)):
            assert T.rel_err(got, ref) <= TOL
        full = T.unit_data_grad(dz, conv.weight, bnp, (h, w), stride)
        assert full.shape == x.shape and T.rel_err(x.grad, full) <= TOL
        if k == 1 and stride == 2:
            half = T.unit_data_grad(dz, conv.weight, bnp, dz.shape[2:], 1)
            assert torch.equal(T.even_pixels_add(torch.zeros_like(full), half), full)


@pytest.mark.parametrize('stride,hw', [(1, (5, 7)), (2, (9, 11))], ids=['s1', 's2'])
def test_dcn_block_head_and_tail_against_fp64_autograd(stride, hw):
    blk = _make('bottleneck', 16, 8, stride, seed=9, dcn=dict(type='DCNv2', deform_groups=1, fallback_on_stride=False), torch_ops=True)
    assert blk.with_dcn and blk.downsample is not None
    x = torch.relu(_rand(2, 16, *hw, seed=10))
    with torch.no_grad():
        maps = block_maps(blk, x)
    _relu_rule(maps[1:], f'DCN block stride {stride}')
    dout = _rand(*maps[-1].shape, seed=11)
    out, dx, grads = _autograd(blk, x, dout)
    assert torch.equal(out, maps[-1])
    sd = blk.state_dict()
    x_, a1, a2, _ = maps
    da2, r, ref = T.tail_backward(sd, '', a2, x, out, dout, stride)
    da1, dcn_grads = T.dcn_unit_backward(copy.deepcopy(blk.conv2), blk.bn2, a1, a2, da2)
    head_dx, head = T.head_backward(sd, '', x, a1, da1)
    ref.update(head)
    ref.update(dcn_grads)
    assert T.rel_err(dx, head_dx + r) <= TOL
    for k in ref:
        assert T.rel_err(grads[k], ref[k]) <= TOL, k
    assert set(grads) - set(ref) == {'bn2.weight', 'bn2.bias'}                  # (the DCN layer's BatchNorm: its own node's business)


def test_network_closed_form_against_fp64_autograd():
    import graph_detr4d_amd as G
    net = R.randomize_(G.ResNet(18, base_channels=8, frozen_stages=1), seed=12).train().double()
    assert not any(m.training for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d))
    img = _rand(2, 3, 64, 96, seed=13)
    recorded = {}
    with torch.no_grad():
        x = net.maxpool(net.relu(net.bn1(net.conv1(img))))
        for layer in (1, 2, 3, 4):
            for b, blk in enumerate(getattr(net, f'layer{layer}')):
                recorded[f'layer{layer}.{b}.'] = block_maps(blk, x)
                x = recorded[f'layer{layer}.{b}.'][-1]
    outs = net(img)
    assert torch.equal(outs[-1], x) and not outs[0].requires_grad
    for prefix, maps in recorded.items():
        if not prefix.startswith('layer1'):
            _relu_rule(maps[1:], prefix)
    couts = {i + 1: _rand(*o.shape, seed=20 + i) for i, o in enumerate(outs)}
    torch.autograd.backward(outs[1:], [couts[i] for i in (2, 3, 4)])
    ref = T.network_backward(net.state_dict(), recorded, couts, first_layer=2)
    trained = {k for k, p in net.named_parameters() if p.grad is not None}
    assert trained == set(ref) and all(k.startswith(('layer2', 'layer3', 'layer4')) for k in trained)
    for k, p in net.named_parameters():
        if k in ref:
            assert T.rel_err(p.grad, ref[k]) <= TOL, k


# ---- the keyword rules ---------------------------------------------------------------------------------------------------------
DCN = dict(type='DCNv2', deform_groups=1, fallback_on_stride=False)


def _frozen(**kw):
    return dict(dict(norm_cfg=dict(type='BN', requires_grad=False)), **kw)


def test_plain_train_keyword_rules():
    import graph_detr4d_amd as G
    # plain_train needs plain_kernels
    for make in (lambda: G.ResNet(18, plain_train=True), lambda: G.Bottleneck(256, 64, plain_train=True),
                 lambda: G.BasicBlock(64, 64, plain_train=True)):
        with pytest.raises(Gd4dError, match='plain_kernels.*torch_ops'):
            make()
    # a DCN block needs hip_train too
    with pytest.raises(Gd4dError, match='hip_train.*torch_ops'):
        G.Bottleneck(256, 64, dcn=DCN, plain_kernels=True, plain_train=True)
    with pytest.raises(Gd4dError, match='hip_train.*torch_ops'):
        G.ResNet(50, dcn=DCN, stage_with_dcn=(False, False, True, True), plain_kernels=True, plain_train=True)
    # what was refused before still is, naming torch_ops
    with pytest.raises(Gd4dError, match='torch_ops'):
        G.ResNet(50, plain_kernels=True, hip_train=True)
    with pytest.raises(Gd4dError, match='torch_ops'):
        G.Bottleneck(256, 64, plain_kernels=True, hip_train=True)
    with pytest.raises(Gd4dError, match='torch_ops'):
        G.BasicBlock(64, 64, plain_kernels=True, hip_train=True)
    net = G.ResNet(18, plain_kernels=True, **_frozen()).eval()
    with pytest.raises(Gd4dError, match='autograd is on.*torch_ops'):
        net(torch.randn(1, 3, 32, 40))
    # the attribute the route rule looks for: only with the keyword
    for blk in (G.Bottleneck(256, 64), G.Bottleneck(256, 64, plain_kernels=True), G.BasicBlock(64, 64, plain_kernels=True),
                G.ResNet(18, plain_kernels=True).layer2[0]):
        assert 'hip_train' not in blk.__dict__ and not blk.plain_train and not blk._has_train_route()
    for blk in (G.Bottleneck(256, 64, plain_kernels=True, plain_train=True), G.BasicBlock(64, 64, plain_kernels=True, plain_train=True),
                G.Bottleneck(256, 64, dcn=DCN, plain_kernels=True, plain_train=True, hip_train=True)):
        assert blk.__dict__['hip_train'] is True and blk.plain_train and blk._has_train_route()
    # passed down by _make_stage, positionally compatible
    stage = G.ResNet._make_stage(64, 128, 2, 2, 1, None, None, False, False, G.BasicBlock, True, True)
    assert all(b.plain_kernels and b.plain_train for b in stage)
    assert not any(b.plain_train for b in G.ResNet._make_stage(64, 128, 2, 2, 1, None, None, False, False, G.BasicBlock, True))
    r18 = G.ResNet(18, plain_kernels=True, plain_train=True)
    assert r18.plain_train and all(m.plain_train for _, m in r18._routed()) and len(r18._routed()) == 8
    r50 = G.ResNet(50, dcn=DCN, stage_with_dcn=(False, False, True, True), plain_kernels=True, plain_train=True, hip_train=True)
    assert all(m.plain_train for _, m in r50._routed()) and r50.layer3[0].conv2.hip_train
    # module tree and state-dict keys are untouched
    assert set(r18.state_dict()) == set(G.ResNet(18).state_dict())
    assert set(r50.state_dict()) == set(G.ResNet(50, dcn=DCN, stage_with_dcn=(False, False, True, True)).state_dict())
    assert [n for n, _ in r18.named_modules()] == [n for n, _ in G.ResNet(18).named_modules()]


def test_training_route_refusals_and_torch_ops():
    import graph_detr4d_amd as G
    x = torch.randn(1, 3, 32, 40)
    # an unfrozen BatchNorm in train() mode
    unfrozen = G.ResNet(18, plain_kernels=True, plain_train=True, norm_eval=False, **_frozen()).train()
    with pytest.raises(Gd4dError, match='not frozen.*torch_ops=True'):
        unfrozen.layer2[1](torch.randn(1, 128, 4, 5))
    # no CPU fallback on the training route either
    net = R.randomize_(G.ResNet(18, plain_kernels=True, plain_train=True, frozen_stages=1, **_frozen()), seed=14).train()
    with pytest.raises(Gd4dError, match='GPU'):
        net(x)
    # torch_ops=True still wins
    net.torch_ops = True
    out = net(x)
    sum(o.sum() for o in out[1:]).backward()
    assert float(net.layer4[1].conv2.weight.grad.abs().max()) > 0
    # what the kernels do not take stays refused
    with pytest.raises(Gd4dError, match='torch_ops'):
        G.ResNet(18, plain_kernels=True, plain_train=True, dilations=(1, 1, 2, 4))
    for kw in (dict(with_cp=True), dict(deep_stem=True), dict(avg_down=True), dict(plugins=[dict()])):
        with pytest.raises(Gd4dError):
            G.ResNet(50, plain_kernels=True, plain_train=True, **kw)
