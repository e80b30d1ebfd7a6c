"""DCNv2 (dcn.py, backbones.py, gd4d_dcn.hip) without a GPU: the fp64 restatement against a grid_sample formulation, the module's torch-op
route against the restatement (forward and gradcheck), state-dict keys, the C ABI's symbols and argument checks, and the default
route's refusals."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

import dcn_ref as R

F64 = torch.float64


def grid_sample_dcn(x, offset, mask, weight, bias, stride):
    """The same function through F.grid_sample(align_corners=True, zeros) in fp64, written independently of the package."""
    n, c, h, w = x.shape
    ho, wo = R.out_hw(h, w, stride)
    ys = (torch.arange(ho, dtype=F64) * stride - 1).view(1, ho, 1)
    xs = (torch.arange(wo, dtype=F64) * stride - 1).view(1, 1, wo)
    out = torch.zeros(n, weight.shape[0], ho, wo, dtype=F64)
    for k in range(9):
        py, px = ys + k // 3 + offset[:, 2 * k], xs + k % 3 + offset[:, 2 * k + 1]
        grid = torch.stack((2 * px / (w - 1) - 1, 2 * py / (h - 1) - 1), dim=-1)
        s = F.grid_sample(x, grid, mode='bilinear', padding_mode='zeros', align_corners=True) * mask[:, k:k + 1]
        out += torch.einsum('ncyx,oc->noyx', s, weight[:, :, k // 3, k % 3])
    return out + bias.view(1, -1, 1, 1)


def _problem(stride, h=5, w=7, cin=3, cout=4, n=2, seed=0):
    g = torch.Generator().manual_seed(seed)
    ho, wo = R.out_hw(h, w, stride)
    x = torch.randn(n, cin, h, w, generator=g, dtype=F64)
    weight = torch.randn(cout, cin, 3, 3, generator=g, dtype=F64)
    bias = torch.randn(cout, generator=g, dtype=F64)
    offset = 2.0 * torch.randn(n, 18, ho, wo, generator=g, dtype=F64)
    mask = torch.rand(n, 9, ho, wo, generator=g, dtype=F64)
    return x, offset, mask, weight, bias


@pytest.mark.parametrize('stride', [1, 2])
def test_reference_agrees_with_grid_sample(stride):
    x, offset, mask, weight, bias = _problem(stride)
    ref = R.dcn_ref(x, offset, mask, weight, bias, stride)
    assert R.rel_err(grid_sample_dcn(x, offset, mask, weight, bias, stride), ref) < 1e-12
    for name, plane in R.crafted_offsets(5, 7, stride).items():
        o = plane.to(F64).expand(2, -1, -1, -1)
        ref = R.dcn_ref(x, o, mask, weight, bias, stride)
        assert R.rel_err(grid_sample_dcn(x, o, mask, weight, bias, stride), ref) < 1e-12, name
        if name in ('at_minus_1', 'at_h_and_w', 'plus_1000', 'minus_1000'):                     # nothing sampled: the bias alone
            assert torch.equal(ref, bias.view(1, -1, 1, 1).expand_as(ref)), name
        if name.startswith('corner_'):                                                          # one corner, weight 0.75 * 0.75
            yy = 0 if name[-2] == 't' else 4
            xx = 0 if name[-1] == 'l' else 6
            want = 0.5625 * torch.einsum('nc,ock,nkyx->noyx', x[:, :, yy, xx], weight.flatten(2), mask) + bias.view(1, -1, 1, 1)
            assert R.rel_err(ref, want) < 1e-12, name


@pytest.mark.parametrize('stride', [1, 2])
def test_torch_route_matches_reference(stride):
    from graph_detr4d_amd import ModulatedDeformConv2d, ModulatedDeformConv2dPack
    x, offset, mask, weight, bias = _problem(stride, cin=4, cout=6)
    m = ModulatedDeformConv2d(4, 6, 3, stride=stride, padding=1, torch_ops=True).double()
    with torch.no_grad():
        m.weight.copy_(weight)
        m.bias.copy_(bias)
    assert R.rel_err(m(x, offset, mask), R.dcn_ref(x, offset, mask, weight, bias, stride)) < 1e-12
    for name, plane in R.crafted_offsets(5, 7, stride).items():
        o = plane.to(F64).expand(2, -1, -1, -1)
        assert R.rel_err(m(x, o, mask), R.dcn_ref(x, o, mask, weight, bias, stride)) < 1e-12, name
    p = ModulatedDeformConv2dPack(4, 6, 3, stride=stride, padding=1, torch_ops=True).double()
    with torch.no_grad():
        p.conv_offset.weight.normal_(std=0.3)
        p.conv_offset.bias.normal_()
    off, msk = R.offset_conv_ref(x, p.conv_offset.weight, p.conv_offset.bias, stride)
    assert float(off.detach().abs().max()) > 1.0
    assert R.rel_err(p(x), R.dcn_ref(x, off, msk, p.weight, p.bias, stride)) < 1e-12
    bn = torch.nn.BatchNorm2d(6).double().eval()
    with torch.no_grad():
        bn.running_mean.normal_()
        bn.running_var.uniform_(0.5, 2.0)
        bn.weight.normal_()
        bn.bias.normal_()
    assert torch.equal(p.forward_bn_relu(x, bn), F.relu(bn(p(x))))


def test_torch_route_gradcheck():
    from graph_detr4d_amd.dcn import modulated_deform_conv2d_torch
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1, 2, 5, 7, generator=g, dtype=F64, requires_grad=True)
    weight = torch.randn(2, 2, 3, 3, generator=g, dtype=F64, requires_grad=True)
    bias = torch.randn(2, generator=g, dtype=F64, requires_grad=True)
    # offsets with fractions away from 0 and 1: bilinear interpolation has a kink at every integer coordinate
    offset = (torch.randint(-2, 3, (1, 18, 5, 7), generator=g).to(F64) + 0.2 + 0.6 * torch.rand(1, 18, 5, 7, generator=g, dtype=F64))
    offset.requires_grad_(True)
    mask = torch.rand(1, 9, 5, 7, generator=g, dtype=F64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda *a: modulated_deform_conv2d_torch(*a, stride=1, padding=1), (x, offset, mask, weight, bias),
                                    eps=1e-6, atol=1e-6)


def test_zero_init_pack_is_half_the_convolution():
    from graph_detr4d_amd import ModulatedDeformConv2dPack
    p = ModulatedDeformConv2dPack(4, 6, 3, stride=1, padding=1, torch_ops=True).double()
    assert float(p.conv_offset.weight.detach().abs().max()) == 0 and float(p.conv_offset.bias.detach().abs().max()) == 0
    with torch.no_grad():
        p.bias.normal_()
    x = torch.randn(2, 4, 5, 7, dtype=F64)
    want = 0.5 * F.conv2d(x, p.weight, None, padding=1) + p.bias.view(1, -1, 1, 1)
    assert R.rel_err(p(x), want) < 1e-12


def test_state_dict_keys_and_registries():
    import graph_detr4d_amd as G
    p = G.build_conv_layer(dict(type='DCNv2', deform_groups=1), 256, 256, kernel_size=3, stride=2, padding=1, bias=False)
    assert isinstance(p, G.ModulatedDeformConv2dPack) and p._version == 2
    assert list(p.state_dict()) == ['weight', 'conv_offset.weight', 'conv_offset.bias']
    assert tuple(p.conv_offset.weight.shape) == (27, 256, 3, 3) and p.conv_offset.stride == (2, 2)
    q = G.ModulatedDeformConv2dPack(64, 64, 3, padding=1)
    assert list(q.state_dict()) == ['weight', 'bias', 'conv_offset.weight', 'conv_offset.bias']
    assert isinstance(G.build_conv_layer(None, 3, 8, 1), torch.nn.Conv2d)
    cfg = dict(type='ResNet', depth=50, num_stages=4, out_indices=(0, 1, 2, 3), frozen_stages=1, norm_cfg=dict(type='BN', requires_grad=False),
               norm_eval=True, style='pytorch', dcn=dict(type='DCNv2', deform_groups=1, fallback_on_stride=False),
               stage_with_dcn=(False, False, True, True))
    r = G.build_backbone(cfg)
    keys = list(r.state_dict())
    offs = [k for k in keys if k.endswith('conv_offset.weight')]
    assert offs == [f'layer3.{i}.conv2.conv_offset.weight' for i in range(6)] + [f'layer4.{i}.conv2.conv_offset.weight' for i in range(3)]
    assert [k for k in keys if k.endswith('conv_offset.bias')] == [k.replace('weight', 'bias') for k in offs]
    for k in ('conv1.weight', 'bn1.running_var', 'layer1.0.downsample.0.weight', 'layer1.0.downsample.1.running_mean', 'layer2.3.conv2.weight',
              'layer3.0.conv2.weight', 'layer4.2.bn3.num_batches_tracked'):
        assert k in keys, k
    assert not any('conv2.bias' in k for k in keys)
    assert tuple(r.layer3[0].conv2.weight.shape) == (256, 256, 3, 3) and r.layer3[0].conv2.stride == (2, 2)
    assert tuple(r.layer4[1].conv2.weight.shape) == (512, 512, 3, 3) and r.layer4[1].conv2.stride == (1, 1)
    assert not r.layer1[0].conv1.weight.requires_grad and r.layer3[0].conv1.weight.requires_grad and not r.layer3[0].bn1.weight.requires_grad
    r.train()
    assert not any(m.training for m in r.modules() if isinstance(m, torch.nn.BatchNorm2d))
    sd = {k: torch.randn_like(v) if v.is_floating_point() else v.clone() for k, v in r.state_dict().items()}
    r2 = G.build_backbone(cfg)
    r2.load_state_dict(sd, strict=True)
    assert all(torch.equal(v, sd[k]) for k, v in r2.state_dict().items())
    r101 = G.ResNet(101, dcn=dict(type='DCNv2'), stage_with_dcn=(False, False, True, True))
    assert sum(k.endswith('conv_offset.weight') for k in r101.state_dict()) == 23 + 3


def test_small_resnet_forward_on_the_torch_route():
    """The block's data flow, CPU: a two-stage ResNet with DCN in stage 2 against the same weights in plain-torch layers."""
    import graph_detr4d_amd as G
    r = G.ResNet(50, num_stages=2, strides=(1, 2), dilations=(1, 1), out_indices=(0, 1), base_channels=8, dcn=dict(type='DCNv2'),
                 stage_with_dcn=(False, True), torch_ops=True, zero_init_residual=False).eval()
    x = torch.randn(1, 3, 32, 40)
    with torch.no_grad():
        outs = r(x)
        assert [tuple(o.shape) for o in outs] == [(1, 32, 8, 10), (1, 64, 4, 5)]
        # zero-initialised offsets: every DCN conv2 is 0.5 x its plain convolution
        y = r.layer1(r.maxpool(r.relu(r.bn1(r.conv1(x)))))
        for blk in r.layer2:
            h = blk.relu(blk.bn1(blk.conv1(y)))
            h = F.relu(blk.bn2(0.5 * F.conv2d(h, blk.conv2.weight, None, stride=blk.stride, padding=1)))
            h = blk.bn3(blk.conv3(h))
            y = F.relu(h + (y if blk.downsample is None else blk.downsample(y)))
        torch.testing.assert_close(outs[1], y, rtol=1e-5, atol=1e-5)


def test_symbols_in_header_lib_and_library(repo_root):
    from graph_detr4d_amd import _lib
    hdr = open(os.path.join(repo_root, 'include', 'gd4d.h')).read()
    assert re.search(r'#define GD4D_ABI_VERSION 56\b', hdr)
    assert _lib.ABI_VERSION == 56
    lib = _lib.load()
    assert lib.gd4d_abi_version() == 56
    for name in ('gd4d_dcn_weight_image_bytes', 'gd4d_dcn_weight_image', 'gd4d_dcn_offset_conv_fwd', 'gd4d_dcn_fwd'):
        assert name in _lib.SIGNATURES and re.search(rf'\b{name}\s*\(', hdr) and hasattr(lib, name)


def test_entry_points_validate_before_any_gpu_work():
    from graph_detr4d_amd import _lib
    lib = _lib.load()
    EINVAL, EUNSUPPORTED, EALIGN = -1, -2, -3
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 96)()
    ptr = ctypes.c_void_p((ctypes.addressof(buf) + 63) & ~63)               # 64-byte aligned: alignment checks pass
    odd = ctypes.c_void_p(ptr.value + 4)
    # image sizes: 9 Cin Mpad 4 bytes, Mpad = 32 (conv_offset), 256 or 512
    nbytes = lib.gd4d_dcn_weight_image_bytes
    assert nbytes(256, 256) == 9 * 256 * 256 * 4 and nbytes(512, 512) == 9 * 512 * 512 * 4 and nbytes(256, 512) == 9 * 256 * 512 * 4
    assert nbytes(256, 27) == 9 * 256 * 32 * 4 and nbytes(64, 128) == 9 * 64 * 256 * 4 and nbytes(512, 320) == 9 * 512 * 512 * 4
    for cin, cout in ((0, 256), (32, 256), (96, 256), (576, 256), (256, 0), (256, 32), (256, 96), (256, 576), (256, 26), (-64, 64)):
        assert nbytes(cin, cout) == 0, (cin, cout)
        assert lib.gd4d_dcn_weight_image(ptr, cin, cout, ptr, null) == EUNSUPPORTED
    assert lib.gd4d_dcn_weight_image(null, 256, 256, ptr, null) == EINVAL
    assert lib.gd4d_dcn_weight_image(ptr, 256, 256, null, null) == EINVAL
    assert lib.gd4d_dcn_weight_image(ptr, 256, 256, odd, null) == EALIGN

    def offs(x=ptr, n=2, cin=256, h=13, w=21, stride=1, image=ptr, bias=ptr, out=ptr):
        return lib.gd4d_dcn_offset_conv_fwd(x, n, cin, h, w, stride, image, bias, out, null)
    assert offs(x=null) == EINVAL and offs(image=null) == EINVAL and offs(out=null) == EINVAL
    assert offs(n=0) == EUNSUPPORTED and offs(h=0) == EUNSUPPORTED and offs(w=-1) == EUNSUPPORTED
    assert offs(stride=3) == EUNSUPPORTED and offs(stride=0) == EUNSUPPORTED
    assert offs(cin=100) == EUNSUPPORTED and offs(cin=1024) == EUNSUPPORTED
    assert offs(h=1 << 11, w=1 << 11) == EUNSUPPORTED                       # 256 x 2^22 elements in one image: past the 32-bit offsets
    assert offs(image=odd) == EALIGN

    def conv(x=ptr, om=ptr, n=2, cin=256, cout=256, h=13, w=21, stride=1, image=ptr, scale=ptr, shift=ptr, relu=1, out=ptr):
        return lib.gd4d_dcn_fwd(x, om, n, cin, cout, h, w, stride, image, scale, shift, relu, out, null)
    assert conv(x=null) == EINVAL and conv(om=null) == EINVAL and conv(image=null) == EINVAL and conv(out=null) == EINVAL
    assert conv(n=0) == EUNSUPPORTED and conv(h=0) == EUNSUPPORTED and conv(w=0) == EUNSUPPORTED
    assert conv(stride=3) == EUNSUPPORTED and conv(relu=2) == EUNSUPPORTED
    assert conv(cin=96) == EUNSUPPORTED and conv(cout=27) == EUNSUPPORTED and conv(cout=1024) == EUNSUPPORTED and conv(cout=100) == EUNSUPPORTED
    assert conv(h=1 << 11, w=1 << 11) == EUNSUPPORTED
    assert conv(image=odd) == EALIGN


def test_default_route_refuses_cpu_train_autograd_and_limits():
    import graph_detr4d_amd as G
    from graph_detr4d_amd import ops
    from graph_detr4d_amd._lib import Gd4dError
    p = G.ModulatedDeformConv2dPack(64, 64, 3, padding=1).eval()
    x = torch.zeros(1, 64, 5, 7)
    with torch.no_grad(), pytest.raises(Gd4dError, match='GPU'):
        p(x)                                                                # no CPU fallback
    bn = torch.nn.BatchNorm2d(64).eval()
    with torch.no_grad(), pytest.raises(Gd4dError, match='GPU'):
        p.forward_bn_relu(x, bn)
    with torch.no_grad(), pytest.raises(Gd4dError, match='eval'):
        p.forward_bn_relu(x, torch.nn.BatchNorm2d(64))                      # batch statistics are not folded
    with pytest.raises(Gd4dError, match='torch_ops'):                      # autograd on, parameters that require grad
        p(x)
    p.train()
    with torch.no_grad(), pytest.raises(Gd4dError, match='train'):
        p(x)
    for kw in (dict(groups=2), dict(deform_groups=2), dict(dilation=2, padding=2), dict(kernel_size=5, padding=2), dict(stride=3)):
        args = dict(in_channels=64, out_channels=64, kernel_size=3, padding=1)
        args.update(kw)
        m = G.ModulatedDeformConv2dPack(**args).eval()
        with torch.no_grad(), pytest.raises(Gd4dError, match='torch_ops'):
            m(x)
    for cin, cout in ((48, 64), (64, 1024), (1024, 64)):
        m = G.ModulatedDeformConv2dPack(cin, cout, 3, padding=1).eval()
        with torch.no_grad(), pytest.raises(Gd4dError, match='torch_ops'):
            m(torch.zeros(1, cin, 5, 7))
    # outside the limits the chosen torch-op route serves
    m = G.ModulatedDeformConv2dPack(4, 4, 3, padding=2, dilation=2, groups=2, deform_groups=2, torch_ops=True)
    assert tuple(m(torch.randn(1, 4, 5, 7)).shape) == (1, 4, 5, 7)
    with pytest.raises(Gd4dError):
        ops.dcn_weight_image(torch.zeros(256, 256, 3, 3))
    with pytest.raises(Gd4dError):
        ops.dcn_offset_conv_fwd(x, torch.zeros(16, dtype=torch.uint8))
    with pytest.raises(Gd4dError):
        ops.dcn_fwd(torch.zeros(1, 64, 5, 7), torch.zeros(1, 27, 5, 7), torch.zeros(9 * 64 * 256 * 4, dtype=torch.uint8), 64)
