"""DepthNet training without a GPU: the fp64 helper against fp64 autograd (pins the yardstick of the GPU tests), the running-buffer
rule against nn.BatchNorm2d, and the new entry points' exports and argument checks."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from depth_net_train_ref import backward64, forward64, rel_fro, running_update
from test_depth_net_cpu import REF_KEYS

NEW_SYMBOLS = ('gd4d_depth_net_image_mode', 'gd4d_depth_conv_tiles', 'gd4d_depth_conv_raw', 'gd4d_depth_bn_stats',
               'gd4d_depth_bn_act_fwd', 'gd4d_depth_bn_bwd_workspace_bytes', 'gd4d_depth_bn_bwd',
               'gd4d_depth_conv_wgrad_workspace_bytes', 'gd4d_depth_conv_wgrad')


@pytest.mark.parametrize('frozen', [False, True])
@pytest.mark.parametrize('shape', [(2, 6, 1, 2), (3, 5, 5, 7), (2, 4, 9, 6)])
def test_helper_equals_fp64_autograd(shape, frozen):
    n, c, h, w = shape
    gen = torch.Generator().manual_seed(100 * n + h)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    x, wt, b = r(n, c, h, w).requires_grad_(), (0.3 * r(c, c, 3, 3)).requires_grad_(), (0.1 * r(c)).requires_grad_()
    gamma, beta, g = (1 + 0.2 * r(c)).requires_grad_(), (0.2 * r(c)).requires_grad_(), torch.rand(n, c, generator=gen, dtype=torch.float64).requires_grad_()
    rm, rv = 0.3 * r(c), 0.5 + torch.rand(c, generator=gen, dtype=torch.float64)
    dout = r(n, c, h, w)
    eps = 1e-5
    y = F.conv2d(x, wt, b, padding=1)
    bn = F.batch_norm(y, rm.clone(), rv.clone(), gamma, beta, training=not frozen, momentum=0.1, eps=eps)
    out = F.relu(bn) * g[:, :, None, None]
    (out * dout).sum().backward()
    fwd = forward64(x, wt, b, gamma, beta, g, eps, running=(rm, rv) if frozen else None)
    assert rel_fro(fwd['out'], out) < 1e-12
    got = backward64(fwd, dout, fwd['z'] > 0)
    for name, ref in (('dx', x.grad), ('dW', wt.grad), ('dgamma', gamma.grad), ('dbeta', beta.grad), ('dg', g.grad)):
        assert rel_fro(got[name], ref) < 1e-10, name
    if frozen:
        assert rel_fro(got['db'], b.grad) < 1e-10
    else:                                                    # zero up to rounding: an absolute bound only
        assert float(b.grad.abs().max()) < 1e-10 and float(got['db'].abs().max()) < 1e-10


def test_running_buffer_rule_against_batchnorm2d():
    torch.manual_seed(3)
    c, n, momentum = 7, 3, 0.1
    bn = nn.BatchNorm2d(c, momentum=momentum).double().train()
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(c))
        bn.running_var.copy_(0.5 + torch.rand(c))
    rm, rv = bn.running_mean.clone(), bn.running_var.clone()
    levels = [(1, 2), (5, 7), (16, 16), (17, 33)]
    for h, w in levels:
        y = torch.randn(n, c, h, w, dtype=torch.float64) * 1.7 + 0.4
        bn(y)
        rm, rv = running_update(rm, rv, y.mean((0, 2, 3)), y.var((0, 2, 3), unbiased=False), n * h * w, momentum)
    torch.testing.assert_close(rm, bn.running_mean, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(rv, bn.running_var, rtol=1e-12, atol=1e-12)
    assert int(bn.num_batches_tracked) == len(levels)


def test_new_symbols_are_exported_and_declared(repo_root):
    from graph_detr4d_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(repo_root, 'include', 'gd4d.h')).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and hasattr(lib, name) and re.search(rf'\b{name}\s*\(', hdr), name
    assert lib.gd4d_abi_version() == _lib.ABI_VERSION                      # additive exports


def test_new_entry_points_validate_before_any_gpu_work():
    from graph_detr4d_amd import _lib
    lib = _lib.load()
    EINVAL, EUNSUPPORTED, EALIGN = -1, -2, -3
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 96)()
    ptr = ctypes.c_void_p((ctypes.addressof(buf) + 63) & ~63)
    odd = ctypes.c_void_p(ptr.value + 4)
    lv = (ctypes.c_int32 * 10)(9, 17, 5, 9, 3, 5, 2, 3, 1, 1)
    zero = (ctypes.c_int32 * 8)(9, 17, 0, 9, 3, 5, 2, 3)
    one = (ctypes.c_int32 * 2)(1, 1)
    ps = (ctypes.c_void_p * 5)(*[ptr.value] * 5)
    holes = (ctypes.c_void_p * 5)(ptr.value, None, ptr.value, ptr.value, ptr.value)
    # transposed image
    assert lib.gd4d_depth_net_image_mode(null, 256, 1, ptr, null) == EINVAL
    assert lib.gd4d_depth_net_image_mode(ptr, 256, 1, null, null) == EINVAL
    assert lib.gd4d_depth_net_image_mode(ptr, 128, 1, ptr, null) == EUNSUPPORTED
    assert lib.gd4d_depth_net_image_mode(ptr, 256, 2, ptr, null) == EUNSUPPORTED
    assert lib.gd4d_depth_net_image_mode(ptr, 256, 1, odd, null) == EALIGN
    # tiles: 6 cameras x (1 x 2 + 1 + 1 + 1) tiles
    assert lib.gd4d_depth_conv_tiles(lv, 4, 6) == 6 * 5
    assert lib.gd4d_depth_conv_tiles(zero, 4, 6) == 0 and lib.gd4d_depth_conv_tiles(null, 4, 6) == 0

    def raw(x=ps, y=ps, hw=lv, levels=4, n=6, c=256, image=ptr, bias=ptr, partials=ptr):
        return lib.gd4d_depth_conv_raw(x, y, hw, levels, n, c, image, bias, partials, null)
    assert raw(x=null) == EINVAL and raw(y=null) == EINVAL and raw(hw=null) == EINVAL and raw(image=null) == EINVAL
    assert raw(x=holes) == EINVAL and raw(y=holes) == EINVAL and raw(hw=zero) == EINVAL
    assert raw(c=128) == EUNSUPPORTED and raw(levels=5) == EUNSUPPORTED and raw(levels=0) == EUNSUPPORTED and raw(n=0) == EUNSUPPORTED
    assert raw(image=odd) == EALIGN

    def stats(partials=ptr, hw=lv, levels=4, n=6, c=256, w=ptr, rm=ptr, rv=ptr, frozen=0, out=ptr):
        return lib.gd4d_depth_bn_stats(partials, hw, levels, n, c, w, rm, rv, 0.1, 1e-5, frozen, out, null)
    assert stats(partials=null) == EINVAL and stats(hw=null) == EINVAL and stats(w=null) == EINVAL and stats(rm=null) == EINVAL
    assert stats(rv=null) == EINVAL and stats(out=null) == EINVAL and stats(hw=zero) == EINVAL
    assert stats(c=128) == EUNSUPPORTED and stats(levels=5) == EUNSUPPORTED and stats(n=0) == EUNSUPPORTED
    assert stats(hw=one, levels=1, n=1) == EUNSUPPORTED                      # the unbiased variance of a single value

    def act(y=ps, out=ps, hw=lv, levels=4, n=6, c=256, st=ptr, beta=ptr, gate=ptr):
        return lib.gd4d_depth_bn_act_fwd(y, out, hw, levels, n, c, st, beta, gate, null)
    assert act(y=null) == EINVAL and act(out=null) == EINVAL and act(hw=null) == EINVAL and act(st=null) == EINVAL
    assert act(beta=null) == EINVAL and act(gate=null) == EINVAL and act(y=holes) == EINVAL and act(hw=zero) == EINVAL
    assert act(c=128) == EUNSUPPORTED and act(levels=5) == EUNSUPPORTED and act(n=0) == EUNSUPPORTED

    assert lib.gd4d_depth_bn_bwd_workspace_bytes(4, 6) == (4 * 6 * 4 + 4 * 2) * 256 * 4
    assert lib.gd4d_depth_bn_bwd_workspace_bytes(5, 6) == 0

    def bwd(dout=ps, y=ps, dy=ps, hw=lv, levels=4, n=6, c=256, rest=(ptr,) * 3, outs=(ptr,) * 5):
        return lib.gd4d_depth_bn_bwd(dout, y, dy, hw, levels, n, c, *rest, 0, *outs, null)
    assert bwd(dout=null) == EINVAL and bwd(y=null) == EINVAL and bwd(dy=null) == EINVAL and bwd(hw=null) == EINVAL
    for i in range(3):
        assert bwd(rest=(ptr,) * i + (null,) + (ptr,) * (2 - i)) == EINVAL
    for i in range(5):
        assert bwd(outs=(ptr,) * i + (null,) + (ptr,) * (4 - i)) == EINVAL
    assert bwd(dout=holes) == EINVAL and bwd(hw=zero) == EINVAL
    assert bwd(c=128) == EUNSUPPORTED and bwd(levels=5) == EUNSUPPORTED and bwd(n=0) == EUNSUPPORTED

    assert lib.gd4d_depth_conv_wgrad_workspace_bytes(3) == 3 * 256 * 256 * 9 * 4
    assert lib.gd4d_depth_conv_wgrad_workspace_bytes(0) == 0

    def wgrad(dy=ps, x=ps, hw=lv, levels=4, n=6, c=256, parts=8, ws=ptr, dw=ptr):
        return lib.gd4d_depth_conv_wgrad(dy, x, hw, levels, n, c, parts, ws, dw, null)
    assert wgrad(dy=null) == EINVAL and wgrad(x=null) == EINVAL and wgrad(hw=null) == EINVAL and wgrad(ws=null) == EINVAL
    assert wgrad(dw=null) == EINVAL and wgrad(dy=holes) == EINVAL and wgrad(x=holes) == EINVAL and wgrad(hw=zero) == EINVAL
    assert wgrad(c=128) == EUNSUPPORTED and wgrad(levels=5) == EUNSUPPORTED and wgrad(n=0) == EUNSUPPORTED
    assert wgrad(parts=0) == EUNSUPPORTED
    assert wgrad(ws=odd) == EALIGN


def test_keyword_constructs_and_changes_no_state():
    from graph_detr4d_amd import DepthNet
    plain = DepthNet(256, 256, 80)
    m = DepthNet(256, 256, 80, hip_train=True)
    assert m.hip_train is True and m.torch_ops is False and plain.hip_train is False
    assert list(m.state_dict()) == REF_KEYS
    m.load_state_dict(plain.state_dict(), strict=True)
    both = DepthNet(256, 256, 80, torch_ops=True, hip_train=True)
    assert both.torch_ops and both.hip_train
    plain.hip_train = True                                                # settable after construction, as torch_ops is
    assert plain.hip_train


def test_ops_refuse_cpu_tensors():
    from graph_detr4d_amd import _lib, ops
    z = torch.zeros
    with pytest.raises(_lib.Gd4dError):
        ops.depth_net_image_t(z(256, 256, 3, 3))
    with pytest.raises(_lib.Gd4dError):
        ops.depth_conv_raw([z(2, 256, 4, 4)], z(16, dtype=torch.uint8), z(256))
    with pytest.raises(_lib.Gd4dError):
        ops.depth_bn_act_fwd([z(2, 256, 4, 4)], z(1, 3, 256), z(256), z(2, 256))
    with pytest.raises(_lib.Gd4dError):
        ops.depth_bn_bwd([z(2, 256, 4, 4)], [z(2, 256, 4, 4)], z(1, 3, 256), z(256), z(2, 256))
    with pytest.raises(_lib.Gd4dError):
        ops.depth_conv_wgrad([z(2, 256, 4, 4)], [z(2, 256, 4, 4)], partitions=1)
    assert ops.depth_conv_tiles([(17, 33), (1, 2)], 3) == 3 * (6 + 1)
