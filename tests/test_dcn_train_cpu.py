"""DCNv2 training (dcn.py's hip_train, gd4d_dcn_train.hip) without a GPU: the closed-form backward the kernels implement against fp64
autograd through dcn_ref (including the convention at integer sample coordinates), the `hip_train` keyword, and the new exports'
argument checks."""
import ctypes
import os
import re

import pytest
import torch

import dcn_ref as R
import dcn_train_ref as T

F64 = torch.float64
TOL = 1e-10


def _problem(stride, h=5, w=7, cin=3, cout=4, n=2, seed=0):
    g = torch.Generator().manual_seed(seed)
    ho, wo = R.out_hw(h, w, stride)
    x = torch.randn(n, cin, h, w, generator=g, dtype=F64)
    weight = torch.randn(cout, cin, 3, 3, generator=g, dtype=F64)
    offset = 2.0 * torch.randn(n, 18, ho, wo, generator=g, dtype=F64)
    mask = torch.rand(n, 9, ho, wo, generator=g, dtype=F64)
    dout = torch.randn(n, cout, ho, wo, generator=g, dtype=F64)
    scale = torch.randn(cout, generator=g, dtype=F64) + 1.5
    relu_mask = torch.rand(n, cout, ho, wo, generator=g) > 0.4
    return x, offset, mask, weight, dout, scale, relu_mask


def _compare(got, ref, what):
    for key, r in ref.items():
        if float(r.abs().max()) == 0.0:
            assert float(got[key].abs().max()) == 0.0, f'{what} {key}: the reference is exactly zero'
        else:
            assert R.rel_err(got[key], r) <= TOL, f'{what} {key}: {R.rel_err(got[key], r):.3e}'


@pytest.mark.parametrize('stride', [1, 2])
def test_closed_form_agrees_with_autograd_on_random_offsets(stride):
    x, offset, mask, weight, dout, scale, relu_mask = _problem(stride)
    _compare(T.closed_form(x, offset, mask, weight, dout, stride), T.autograd(x, offset, mask, weight, dout, stride), 'plain')
    _compare(T.closed_form(x, offset, mask, weight, dout, stride, scale, relu_mask),
             T.autograd(x, offset, mask, weight, dout, stride, scale, relu_mask), 'scale + relu')


@pytest.mark.parametrize('stride', [1, 2])
def test_closed_form_on_every_crafted_plane_is_the_right_derivative(stride):
    """The convention test: on `zero` and `integers` every sample coordinate is an integer, where the offset gradient has a kink; floor-based
    autograd takes the derivative from the right, and so must the closed form.  Nothing is excluded."""
    x, _, mask, weight, dout, scale, relu_mask = _problem(stride)
    planes = R.crafted_offsets(5, 7, stride)
    assert {'zero', 'integers', 'at_minus_1', 'at_h_minus_1', 'at_h_and_w', 'plus_1000', 'minus_1000', 'corner_tl', 'corner_tr',
            'corner_bl', 'corner_br'} == set(planes)
    for name, plane in planes.items():
        o = plane.to(F64).expand(2, -1, -1, -1).contiguous()
        ref = T.autograd(x, o, mask, weight, dout, stride, scale, relu_mask)
        _compare(T.closed_form(x, o, mask, weight, dout, stride, scale, relu_mask), ref, name)
        if name in ('plus_1000', 'minus_1000', 'at_h_and_w'):               # nothing sampled: only the bias has a gradient
            assert all(float(ref[k].abs().max()) == 0.0 for k in ('x', 'offset', 'mask', 'weight')), name
        if name == 'at_minus_1':                                            # the one corner inside has weight 0 and derivative 0
            assert float(ref['offset'].abs().max()) == 0.0
        if name in ('zero', 'integers'):
            assert float(ref['offset'].abs().max()) > 0.0


@pytest.mark.parametrize('stride', [1, 2])
def test_closed_form_through_conv_offset(stride):
    x, _, _, weight, dout, scale, relu_mask = _problem(stride)
    g = torch.Generator().manual_seed(9)
    off_w = 0.3 * torch.randn(27, 3, 3, 3, generator=g, dtype=F64)
    off_b = torch.randn(27, generator=g, dtype=F64)
    ref = T.autograd_pack(x, weight, off_w, off_b, dout, stride, scale, relu_mask)
    got = T.closed_form_pack(x, weight, off_w, off_b, dout, stride, scale, relu_mask)
    _compare({k: got[k] for k in ref}, ref, 'pack')
    # a fresh layer: conv_offset zero, every offset exactly 0 - its gradients follow the right derivative
    zero_w, zero_b = torch.zeros_like(off_w), torch.zeros_like(off_b)
    ref = T.autograd_pack(x, weight, zero_w, zero_b, dout, stride)
    got = T.closed_form_pack(x, weight, zero_w, zero_b, dout, stride)
    _compare({k: got[k] for k in ref}, ref, 'fresh pack')
    assert float(ref['off_weight'].abs().max()) > 0.0
    # the conv_offset formulas alone against conv2d's autograd
    do = torch.randn(2, 27, *R.out_hw(5, 7, stride), generator=g, dtype=F64)
    xx, ww = x.clone().requires_grad_(True), off_w.clone().requires_grad_(True)
    bb = off_b.clone().requires_grad_(True)
    (torch.nn.functional.conv2d(xx, ww, bb, stride=stride, padding=1) * do).sum().backward()
    term, dow, dob = T.offset_conv_closed_form(x, off_w, do, stride)
    assert R.rel_err(term, xx.grad) <= TOL and R.rel_err(dow, ww.grad) <= TOL and R.rel_err(dob, bb.grad) <= TOL


def test_hip_train_keyword():
    import graph_detr4d_amd as G
    from graph_detr4d_amd._lib import Gd4dError
    p = G.ModulatedDeformConv2dPack(64, 64, 3, padding=1, hip_train=True)
    q = G.ModulatedDeformConv2d(64, 64, 3, padding=1, hip_train=True)
    assert p.hip_train and q.hip_train and not G.ModulatedDeformConv2dPack(64, 64, 3, padding=1).hip_train
    assert list(p.state_dict()) == ['weight', 'bias', 'conv_offset.weight', 'conv_offset.bias'] and list(q.state_dict()) == ['weight', 'bias']
    b = G.build_conv_layer(dict(type='DCNv2', deform_groups=1), 256, 256, kernel_size=3, stride=2, padding=1, bias=False, hip_train=True)
    assert b.hip_train and list(b.state_dict()) == ['weight', 'conv_offset.weight', 'conv_offset.bias']
    dcn = dict(type='DCNv2', deform_groups=1, fallback_on_stride=False)
    blk = G.Bottleneck(256, 64, stride=2, dcn=dcn, hip_train=True)
    assert blk.conv2.hip_train and not G.Bottleneck(256, 64, stride=2, dcn=dcn).conv2.hip_train
    kw = dict(num_stages=2, strides=(1, 2), dilations=(1, 1), out_indices=(0, 1), dcn=dict(type='DCNv2'), stage_with_dcn=(False, True))
    r, r0 = G.ResNet(50, hip_train=True, **kw), G.ResNet(50, **kw)
    assert all(m.conv2.hip_train for m in r.layer2) and not any(m.conv2.hip_train for m in r0.layer2)
    assert list(r.state_dict()) == list(r0.state_dict())
    # without the switch the module still raises in train() mode; the message now names both switches
    m = G.ModulatedDeformConv2dPack(64, 64, 3, padding=1).train()
    with torch.no_grad(), pytest.raises(Gd4dError, match='train') as e:
        m(torch.zeros(1, 64, 5, 7))
    assert 'torch_ops' in str(e.value) and 'hip_train' in str(e.value)
    m.eval()
    with pytest.raises(Gd4dError, match='torch_ops') as e:
        m(torch.zeros(1, 64, 5, 7))
    assert 'hip_train' in str(e.value)
    # with it, a CPU tensor is still refused (no CPU fallback), and torch_ops=True still wins
    with pytest.raises(Gd4dError, match='GPU'):
        p.train()(torch.zeros(1, 64, 5, 7))
    t = G.ModulatedDeformConv2dPack(4, 4, 3, padding=1, torch_ops=True, hip_train=True).train()
    t(torch.randn(1, 4, 5, 7)).sum().backward()
    assert t.conv_offset.weight.grad is not None


def test_symbols_in_header_lib_and_library(repo_root):
    from graph_detr4d_amd import _lib
    hdr = open(os.path.join(repo_root, 'include', 'gd4d.h')).read()
    lib = _lib.load()
    assert lib.gd4d_abi_version() == 56
    for name in ('gd4d_dcn_weight_image_t_bytes', 'gd4d_dcn_weight_image_t', 'gd4d_dcn_bwd_data', 'gd4d_dcn_wgrad_tiles',
                 'gd4d_dcn_wgrad_workspace_bytes', 'gd4d_dcn_wgrad', 'gd4d_dcn_offset_conv_dgrad',
                 'gd4d_dcn_offset_conv_wgrad_workspace_bytes', 'gd4d_dcn_offset_conv_wgrad'):
        assert name in _lib.SIGNATURES and re.search(rf'\b{name}\s*\(', hdr) and hasattr(lib, name)


def test_entry_points_validate_before_any_gpu_work():
    from graph_detr4d_amd import _lib
    lib = _lib.load()
    EINVAL, EUNSUPPORTED, EALIGN = -1, -2, -3
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 96)()
    ptr = ctypes.c_void_p((ctypes.addressof(buf) + 63) & ~63)
    odd = ctypes.c_void_p(ptr.value + 4)
    nbytes = lib.gd4d_dcn_weight_image_t_bytes
    assert nbytes(256, 256) == 9 * 256 * 256 * 4 and nbytes(256, 512) == 9 * 256 * 512 * 4 and nbytes(64, 128) == 9 * 64 * 128 * 4
    for cin, cout in ((0, 256), (32, 256), (96, 256), (576, 256), (256, 0), (256, 27), (256, 96), (256, 576), (-64, 64)):
        assert nbytes(cin, cout) == 0, (cin, cout)
        assert lib.gd4d_dcn_weight_image_t(ptr, cin, cout, ptr, null) == EUNSUPPORTED
    assert lib.gd4d_dcn_weight_image_t(null, 256, 256, ptr, null) == EINVAL
    assert lib.gd4d_dcn_weight_image_t(ptr, 256, 256, null, null) == EINVAL
    assert lib.gd4d_dcn_weight_image_t(ptr, 256, 256, odd, null) == EALIGN

    def data(dout=ptr, y=ptr, scale=ptr, x=ptr, om=ptr, n=2, cin=256, cout=256, h=13, w=21, stride=1, image=ptr, sig=1, dx=ptr, doff=ptr):
        return lib.gd4d_dcn_bwd_data(dout, y, scale, x, om, n, cin, cout, h, w, stride, image, sig, dx, doff, null)
    assert data(dout=null) == EINVAL and data(x=null) == EINVAL and data(om=null) == EINVAL and data(image=null) == EINVAL
    assert data(doff=null) == EINVAL
    assert data(n=0) == EUNSUPPORTED and data(h=0) == EUNSUPPORTED and data(w=-1) == EUNSUPPORTED and data(stride=3) == EUNSUPPORTED
    assert data(cin=96) == EUNSUPPORTED and data(cout=27) == EUNSUPPORTED and data(cout=1024) == EUNSUPPORTED and data(sig=2) == EUNSUPPORTED
    assert data(h=1 << 11, w=1 << 11) == EUNSUPPORTED
    assert data(image=odd) == EALIGN

    tiles = lib.gd4d_dcn_wgrad_tiles
    assert tiles(2, 13, 21, 1) == 2 * 5 and tiles(2, 26, 37, 2) == 2 * 4 and tiles(1, 5, 7, 1) == 1
    assert tiles(0, 5, 7, 1) == 0 and tiles(1, 5, 7, 3) == 0 and tiles(1, 0, 7, 1) == 0
    wsb = lib.gd4d_dcn_wgrad_workspace_bytes
    assert wsb(256, 512, 3) == 3 * 512 * (256 * 9 + 1) * 4
    assert wsb(96, 256, 1) == 0 and wsb(256, 27, 1) == 0 and wsb(256, 256, 0) == 0 and wsb(256, 256, 4097) == 0

    def wgrad(dout=ptr, y=ptr, scale=ptr, x=ptr, om=ptr, n=2, cin=256, cout=256, h=13, w=21, stride=1, parts=2, ws=ptr, dw=ptr, db=ptr):
        return lib.gd4d_dcn_wgrad(dout, y, scale, x, om, n, cin, cout, h, w, stride, parts, ws, dw, db, null)
    assert wgrad(dout=null) == EINVAL and wgrad(x=null) == EINVAL and wgrad(om=null) == EINVAL and wgrad(ws=null) == EINVAL
    assert wgrad(dw=null) == EINVAL and wgrad(db=null) == EINVAL
    assert wgrad(n=0) == EUNSUPPORTED and wgrad(stride=0) == EUNSUPPORTED and wgrad(cin=100) == EUNSUPPORTED and wgrad(cout=27) == EUNSUPPORTED
    assert wgrad(parts=0) == EUNSUPPORTED and wgrad(parts=4097) == EUNSUPPORTED and wgrad(h=1 << 11, w=1 << 11) == EUNSUPPORTED
    assert wgrad(ws=odd) == EALIGN

    def dgrad(doff=ptr, weight=ptr, n=2, cin=256, h=13, w=21, stride=1, dx=ptr):
        return lib.gd4d_dcn_offset_conv_dgrad(doff, weight, n, cin, h, w, stride, dx, null)
    assert dgrad(doff=null) == EINVAL and dgrad(weight=null) == EINVAL and dgrad(dx=null) == EINVAL
    assert dgrad(n=0) == EUNSUPPORTED and dgrad(cin=96) == EUNSUPPORTED and dgrad(stride=3) == EUNSUPPORTED and dgrad(h=0) == EUNSUPPORTED

    owsb = lib.gd4d_dcn_offset_conv_wgrad_workspace_bytes
    assert owsb(256, 5) == 5 * 27 * (256 * 9 + 1) * 4 and owsb(96, 1) == 0 and owsb(256, 0) == 0 and owsb(256, 4097) == 0

    def owgrad(doff=ptr, x=ptr, n=2, cin=256, h=13, w=21, stride=1, parts=2, ws=ptr, dw=ptr, db=ptr):
        return lib.gd4d_dcn_offset_conv_wgrad(doff, x, n, cin, h, w, stride, parts, ws, dw, db, null)
    assert owgrad(doff=null) == EINVAL and owgrad(x=null) == EINVAL and owgrad(ws=null) == EINVAL and owgrad(dw=null) == EINVAL
    assert owgrad(db=null) == EINVAL
    assert owgrad(n=0) == EUNSUPPORTED and owgrad(cin=1024) == EUNSUPPORTED and owgrad(stride=3) == EUNSUPPORTED
    assert owgrad(parts=0) == EUNSUPPORTED and owgrad(ws=odd) == EALIGN


def test_ops_wrappers_refuse_cpu_tensors():
    from graph_detr4d_amd import ops
    from graph_detr4d_amd._lib import Gd4dError
    x, om, dout = torch.zeros(1, 64, 5, 7), torch.zeros(1, 27, 5, 7), torch.zeros(1, 64, 5, 7)
    with pytest.raises(Gd4dError):
        ops.dcn_weight_image_t(torch.zeros(64, 64, 3, 3))
    with pytest.raises(Gd4dError):
        ops.dcn_weight_image_t(torch.zeros(64, 48, 3, 3))
    with pytest.raises(Gd4dError):
        ops.dcn_bwd_data(dout, x, om, torch.zeros(9 * 64 * 64 * 4, dtype=torch.uint8), 64)
    with pytest.raises(Gd4dError):
        ops.dcn_bwd_data(dout, x, om, torch.zeros(16, dtype=torch.uint8), 64)
    with pytest.raises(Gd4dError):
        ops.dcn_wgrad(dout, x, om, 64)
    with pytest.raises(Gd4dError):
        ops.dcn_offset_conv_dgrad(om, torch.zeros(27, 64, 3, 3), x)
    with pytest.raises(Gd4dError):
        ops.dcn_offset_conv_wgrad(om, x)
