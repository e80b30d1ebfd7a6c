"""ResNet depths 18 / 34 (BasicBlock) and the `plain_kernels` switch without a GPU: state-dict keys, the registry, the new block's data
flow against the fp64 restatement (resnet_ref.py), the refusals of the route rule and their torch-op counterparts, and - on the fp64
references alone - that the GPU tests' kernel cases exercise the ReLU."""
import pytest
import torch

import resnet_cases as C
import resnet_ref as R
from graph_detr4d_amd._lib import Gd4dError

RES18_CFG = dict(type='ResNet', depth=18, num_stages=4, out_indices=(0, 1, 2, 3), frozen_stages=1,
                 norm_cfg=dict(type='BN2d', requires_grad=False), norm_eval=True, style='pytorch')
RES50_DCN_CFG = dict(type='ResNet', depth=50, num_stages=4, out_indices=(0, 1, 2, 3), frozen_stages=1,
                     norm_cfg=dict(type='BN', requires_grad=False), norm_eval=True, style='pytorch',
                     dcn=dict(type='DCNv2', deform_groups=1, fallback_on_stride=False), stage_with_dcn=(False, False, True, True))


def test_basic_block_depths_have_mmdets_keys():
    import graph_detr4d_amd as G
    assert G.BasicBlock.expansion == 1 and G.Bottleneck.expansion == 4 and 'BasicBlock' in G.__all__
    r18, r34 = G.ResNet(18), G.ResNet(34)
    keys = set(r18.state_dict())
    for k in ('conv1.weight', 'bn1.running_mean', 'layer1.0.conv1.weight', 'layer1.1.bn2.bias', 'layer2.0.conv1.weight', 'layer2.0.bn2.running_var',
              'layer2.0.downsample.0.weight', 'layer2.0.downsample.1.running_mean', 'layer3.1.conv2.weight', 'layer4.0.downsample.1.weight',
              'layer4.1.bn2.num_batches_tracked'):
        assert k in keys, k
    assert not any(k.startswith('layer1.0.downsample') or '.conv3.' in k or '.bn3.' in k or k.startswith('layer1.2.') for k in keys)
    assert [len(getattr(r18, f'layer{i}')) for i in (1, 2, 3, 4)] == [2, 2, 2, 2]
    assert [len(getattr(r34, f'layer{i}')) for i in (1, 2, 3, 4)] == [3, 4, 6, 3] and 'layer3.5.conv2.weight' in r34.state_dict()
    assert tuple(r18.layer2[0].conv1.weight.shape) == (128, 64, 3, 3) and r18.layer2[0].conv1.stride == (2, 2)
    assert tuple(r18.layer2[0].downsample[0].weight.shape) == (128, 64, 1, 1) and r18.layer2[0].downsample[0].stride == (2, 2)
    assert tuple(r18.layer4[1].conv2.weight.shape) == (512, 512, 3, 3) and r18.feat_dim == 512
    assert float(r18.layer1[0].bn2.weight.detach().abs().max()) == 0 and float(r18.layer1[0].bn1.weight.detach().min()) == 1    # zero_init_residual
    for depth in (18, 50):
        assert set(G.ResNet(depth, plain_kernels=True).state_dict()) == set(G.ResNet(depth).state_dict())
    with pytest.raises(Gd4dError, match=r'depths \[18, 34, 50, 101\]'):
        G.ResNet(152)


def test_build_backbone_of_the_configs_dicts():
    import graph_detr4d_amd as G
    r18 = G.build_backbone(RES18_CFG)
    assert isinstance(r18.layer1[0], G.BasicBlock) and not r18.plain_kernels and not r18.layer1[0].plain_kernels
    assert not r18.layer1[0].conv1.weight.requires_grad and r18.layer2[0].conv1.weight.requires_grad and not r18.layer2[0].bn1.weight.requires_grad
    r18.train()
    assert not any(m.training for m in r18.modules() if isinstance(m, torch.nn.BatchNorm2d))
    r50 = G.build_backbone(dict(RES50_DCN_CFG, plain_kernels=True))
    assert r50.plain_kernels and all(m.plain_kernels for m in r50.modules() if isinstance(m, G.Bottleneck))
    assert isinstance(r50.layer3[0].conv2, G.ModulatedDeformConv2dPack) and isinstance(r50.layer2[0].conv2, torch.nn.Conv2d)
    assert [k for k, _, _ in r50.layer3[0]._plain_layers()] == ['conv1', 'downsample', 'conv3']
    assert [k for k, _, _ in r50.layer2[1]._plain_layers()] == ['conv1', 'conv2', 'conv3']
    assert set(r50.state_dict()) == set(G.build_backbone(RES50_DCN_CFG).state_dict())
    # the network's switch reaches every routed block, and through a DCN block its conv2
    from graph_detr4d_amd import functional as Fn
    with Fn.torch_ops_for(r50):
        assert r50.layer1[0].torch_ops and r50.layer3[0].torch_ops and r50.layer3[0].conv2.torch_ops
    assert not r50.layer1[0].torch_ops and not r50.layer3[0].conv2.torch_ops


def test_resnet18_default_route_against_fp64():
    """The new block's data flow: stock torch layers in fp64 on the CPU against the restatement.  No kernels."""
    import graph_detr4d_amd as G
    net = R.randomize_(G.ResNet(18), seed=7).eval().double()
    x = C.rand(2, 3, 52, 84, seed=8).double()
    with torch.no_grad():
        outs = net(x)
    want = R.resnet(net.state_dict(), x, 18)
    assert [tuple(o.shape) for o in outs] == [(2, 64, 13, 21), (2, 128, 7, 11), (2, 256, 4, 6), (2, 512, 2, 3)]
    for o, w in zip(outs, want):
        assert float(w.abs().max()) > 0 and R.rel_err(o, w) <= 1e-5
    blk = R.randomize_(G.ResNet._make_stage(64, 128, 1, 2, 1, None, None, False, False, G.BasicBlock)[0], seed=9).eval().double()
    xb = torch.relu(C.rand(2, 64, 9, 11, seed=10)).double()
    with torch.no_grad():
        assert R.rel_err(blk(xb), R.basic_block(blk.state_dict(), '', xb, 2)) <= 1e-5


def _frozen(**kw):
    return dict(dict(norm_cfg=dict(type='BN', requires_grad=False)), **kw)


def test_refusals_name_torch_ops():
    import graph_detr4d_amd as G
    x = torch.randn(1, 3, 32, 40)
    with pytest.raises(Gd4dError, match='torch_ops'):
        G.ResNet(18, plain_kernels=True, base_channels=8)
    with pytest.raises(Gd4dError, match='torch_ops'):
        G.ResNet(50, plain_kernels=True, base_channels=8)
    with pytest.raises(Gd4dError, match='torch_ops'):
        G.ResNet(18, plain_kernels=True, dilations=(1, 1, 2, 4))
    with pytest.raises(Gd4dError, match='torch_ops'):
        G.ResNet(50, plain_kernels=True, strides=(1, 2, 1, 1), dilations=(1, 1, 2, 4))
    with pytest.raises(Gd4dError, match='torch_ops'):
        G.ResNet(50, plain_kernels=True, hip_train=True)
    with pytest.raises(Gd4dError, match='torch_ops'):
        G.Bottleneck(256, 64, plain_kernels=True, hip_train=True)
    with pytest.raises(Gd4dError, match='torch_ops'):
        G.ResNet(18, dcn=dict(type='DCNv2'), stage_with_dcn=(False, False, True, True))
    with pytest.raises(Gd4dError, match='torch_ops'):
        G.BasicBlock(64, 64, dcn=dict(type='DCNv2'))
    # a block on its own refuses at the call what the network refuses at construction
    with pytest.raises(Gd4dError, match='torch_ops'), torch.no_grad():
        G.BasicBlock(8, 8, plain_kernels=True).eval()(torch.randn(1, 8, 5, 7))
    net = G.ResNet(18, plain_kernels=True, **_frozen()).eval()
    with pytest.raises(Gd4dError, match='GPU'), torch.no_grad():
        net(x)                                                              # CPU tensors on the kernel route
    with pytest.raises(Gd4dError, match='autograd is on.*torch_ops'):
        net(x)                                                              # trainable convolutions, grad mode on
    unfrozen = G.ResNet(18, plain_kernels=True, norm_eval=False, **_frozen()).train()
    assert unfrozen.layer1[0].bn1.training
    with pytest.raises(Gd4dError, match='train\\(\\) mode.*torch_ops'), torch.no_grad():
        unfrozen(x)
    unfrozen.eval()
    unfrozen.layer2[1].bn2.train()                                          # any one of a block's BatchNorms
    with pytest.raises(Gd4dError, match='BasicBlock\\(128, 128\\) in train\\(\\) mode'), torch.no_grad():
        unfrozen.layer2[1](torch.randn(1, 128, 4, 5))                       # (the block itself: layer1 would refuse the CPU input first)


def test_the_same_configurations_run_on_the_torch_route():
    import graph_detr4d_amd as G
    from graph_detr4d_amd import functional as Fn
    x = torch.randn(1, 3, 32, 40)
    with torch.no_grad():
        small = G.ResNet(18, plain_kernels=True, base_channels=8, torch_ops=True).eval()
        assert [tuple(o.shape) for o in small(x)] == [(1, 8, 8, 10), (1, 16, 4, 5), (1, 32, 2, 3), (1, 64, 1, 2)]
        dilated = G.ResNet(18, plain_kernels=True, strides=(1, 2, 1, 1), dilations=(1, 1, 2, 4), base_channels=8, torch_ops=True).eval()
        assert [tuple(o.shape) for o in dilated(x)] == [(1, 8, 8, 10), (1, 16, 4, 5), (1, 32, 4, 5), (1, 64, 4, 5)]
    net = R.randomize_(G.ResNet(18, plain_kernels=True, **_frozen()), seed=11).eval()
    stock = G.ResNet(18, **_frozen()).eval()
    stock.load_state_dict(net.state_dict(), strict=True)
    with torch.no_grad(), Fn.torch_ops_for(net):
        assert all(torch.equal(a, b) for a, b in zip(net(x), stock(x)))     # CPU input: the block's own torch layers
    net.torch_ops = True
    net.train()                                                             # norm_eval keeps the BatchNorms frozen; autograd on
    out = net(x)
    sum(o.sum() for o in out).backward()
    assert net.layer4[1].conv2.weight.grad is not None and float(net.layer4[1].conv2.weight.grad.abs().max()) > 0
    unfrozen = G.ResNet(18, plain_kernels=True, norm_eval=False, torch_ops=True, base_channels=8).train()
    assert unfrozen(torch.randn(2, 3, 32, 40))[-1].requires_grad            # batch statistics, trainable


def test_kernel_cases_exercise_the_relu():
    """The fp64 references of the GPU tests' kernel cases: with the ReLU on at least a fifth of the outputs are 0, with it off at least a
    fifth are negative (so a ReLU that ran would be seen)."""
    for taps, cases in ((1, C.CONV1X1_CASES), (9, C.CONV3X3_CASES)):
        for case in cases:
            *_, ident, ref = C.conv_case(taps, *case)
            assert (ident is not None) == case[3]
            if ident is not None:
                assert abs(float(ident.mean())) < 0.05
            share = float(((ref == 0) if case[4] else (ref < 0)).double().mean())
            assert share > 0.2, (taps, case, share)
