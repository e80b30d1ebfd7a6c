"""Camera-aware DepthNet (Detr3DHeadPECAM's depth_net): the reference fixture against a plain-torch restatement, the module's
parameter names, and the C ABI's argument checks - no GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from golden_io import Golden, sub

REF_KEYS = ['reduce_conv.0.weight', 'reduce_conv.0.bias', 'reduce_conv.1.weight', 'reduce_conv.1.bias', 'reduce_conv.1.running_mean',
            'reduce_conv.1.running_var', 'reduce_conv.1.num_batches_tracked', 'context_conv.weight', 'context_conv.bias',
            'mlp.fc1.weight', 'mlp.fc1.bias', 'mlp.fc2.weight', 'mlp.fc2.bias', 'se.conv_reduce.weight', 'se.conv_reduce.bias',
            'se.conv_expand.weight', 'se.conv_expand.bias']


def restated_gate(sd, intrinsics, ida, scale=1000.0):
    """detr3d_head_pe_camaware.py:86-100 in plain torch: pixel size from the inverse intrinsics, the ida scale ([0, 0] read twice),
    the 1 -> 256 -> 256 MLP and the SE gate's two 1x1 convolutions on (N, 256, 1, 1)."""
    inv = torch.inverse(intrinsics)
    pixel = torch.sqrt(inv[:, 0, 0] ** 2 + inv[:, 1, 1] ** 2).reshape(-1, 1)
    d = ida[..., 0, 0].reshape(-1, 1)
    s = pixel * scale / torch.sqrt(d * d + d * d)
    h = F.linear(F.relu(F.linear(s, sd['mlp.fc1.weight'], sd['mlp.fc1.bias'])), sd['mlp.fc2.weight'], sd['mlp.fc2.bias'])
    h = h[..., None, None]
    r = F.relu(F.conv2d(h, sd['se.conv_reduce.weight'], sd['se.conv_reduce.bias']))
    return torch.sigmoid(F.conv2d(r, sd['se.conv_expand.weight'], sd['se.conv_expand.bias'])).flatten(1)


def restated_depth_net(sd, x, gate, eps=1e-5):
    """relu(BN_eval(conv3x3(x) + b)) * gate for x (N, C, H, W)."""
    y = F.conv2d(x, sd['reduce_conv.0.weight'], sd['reduce_conv.0.bias'], padding=1)
    y = (y - sd['reduce_conv.1.running_mean'][:, None, None]) / torch.sqrt(sd['reduce_conv.1.running_var'][:, None, None] + eps)
    y = y * sd['reduce_conv.1.weight'][:, None, None] + sd['reduce_conv.1.bias'][:, None, None]
    return F.relu(y) * gate[:, :, None, None]


def test_fixture_agrees_with_a_plain_torch_restatement():
    g = Golden('head_pe_cam')
    sd = sub(g.state(), 'depth_net.')
    gate = restated_gate(sd, g.t('intrinsics'), g.t('ida')[None])
    torch.testing.assert_close(gate, g.t('cam_gate'), rtol=0, atol=1e-6)
    assert float(gate.max() - gate.min()) > 0.1                            # the gate is not a constant
    for lvl, f in enumerate(g.feats()):
        got = restated_depth_net(sd, f[0], gate, g.meta['bn_eps'])
        ref = g.t(f'depth{lvl}')
        assert tuple(ref.shape) == tuple(f.shape[1:]) and tuple(f.shape[-2:]) == tuple(g.meta['levels'][lvl])
        torch.testing.assert_close(got, ref, rtol=1e-5, atol=1e-5)
        assert 0.3 < float((ref > 0).float().mean()) < 0.7                  # BN statistics move the ReLU's threshold
    # the head's hand-over is the DepthNet's output plus the position embedding: the levels keep their shapes
    for lvl in range(len(g.meta['levels'])):
        assert g.t(f'out{lvl}').shape[1:] == g.t(f'depth{lvl}').shape
    assert min(h for h, _ in g.meta['levels']) >= 2 and len(g.meta['levels']) == 4


def test_module_names_and_strict_load():
    from graph_detr4d_amd import DepthNet
    m = DepthNet(256, 256, 80)
    assert list(m.state_dict()) == REF_KEYS
    g = Golden('head_pe_cam')
    sd = sub(g.state(), 'depth_net.')
    assert sorted(sd) == sorted(REF_KEYS)                                  # the keys the reference module saved
    m.load_state_dict(sd, strict=True)
    bn = m.reduce_conv[1]
    assert torch.equal(bn.running_var, sd['reduce_conv.1.running_var']) and float(bn.running_var.min()) > 0.2
    assert not torch.allclose(bn.running_mean, torch.zeros(256))


def test_module_refuses_cpu_maps_and_batches():
    from graph_detr4d_amd import DepthNet
    from graph_detr4d_amd._lib import Gd4dError
    g = Golden('head_pe_cam')
    m = DepthNet(256, 256, 80).eval()
    metas = [dict(intrinsics=list(g.arrays['intrinsics']), ida_mats=[g.t('ida')])]
    with torch.no_grad(), pytest.raises(Gd4dError):
        m.forward_levels(g.feats(), metas)                                 # no CPU fallback
    with pytest.raises(ValueError):
        m.forward_levels([torch.zeros(2, 6, 256, 4, 4)], metas)            # B = 1 only, as the reference
    with pytest.raises(ValueError):
        m.forward_levels(g.feats(), [dict(intrinsics=list(g.arrays['intrinsics']), ida_mats=[g.t('ida')] * 4)])   # 1 or N


def test_ops_refuse_cpu_tensors():
    from graph_detr4d_amd import _lib, ops
    z = torch.zeros
    with pytest.raises(_lib.Gd4dError):
        ops.depth_net_image(z(256, 256, 3, 3))
    with pytest.raises(_lib.Gd4dError):
        ops.cam_gate_fwd(z(6, 4, 4), z(1), z(256, 1), z(256), z(256, 256), z(256), z(256, 256, 1, 1), z(256), z(256, 256, 1, 1),
                         z(256))
    with pytest.raises(_lib.Gd4dError):
        ops.depth_conv_fwd([z(6, 256, 4, 4)], z(16, dtype=torch.uint8), *[z(256)] * 5, 1e-5, z(6, 256))


def test_abi_56_in_header_lib_and_library(repo_root):
    from graph_detr4d_amd import _lib
    hdr = open(os.path.join(repo_root, 'include', 'gd4d.h')).read()
    assert re.search(r'#define GD4D_ABI_VERSION 56\b', hdr)
    assert _lib.ABI_VERSION == 56
    assert _lib.load().gd4d_abi_version() == 56
    for name in ('gd4d_depth_net_image_bytes', 'gd4d_depth_net_image', 'gd4d_cam_gate_fwd', 'gd4d_depth_conv_fwd'):
        assert name in _lib.SIGNATURES and re.search(rf'\b{name}\s*\(', hdr)


def test_entry_points_validate_before_any_gpu_work():
    from graph_detr4d_amd import _lib
    lib = _lib.load()
    EINVAL, EUNSUPPORTED, EALIGN = -1, -2, -3
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 96)()
    ptr = ctypes.c_void_p((ctypes.addressof(buf) + 63) & ~63)               # 64-byte aligned: alignment checks pass
    odd = ctypes.c_void_p(ptr.value + 4)
    assert lib.gd4d_depth_net_image_bytes(256) == 72 * 32768
    assert lib.gd4d_depth_net_image_bytes(128) == 0
    # image
    assert lib.gd4d_depth_net_image(null, 256, ptr, null) == EINVAL
    assert lib.gd4d_depth_net_image(ptr, 256, null, null) == EINVAL
    assert lib.gd4d_depth_net_image(ptr, 128, ptr, null) == EUNSUPPORTED
    assert lib.gd4d_depth_net_image(ptr, 256, odd, null) == EALIGN
    # gate
    w8 = [ptr] * 8

    def gate(intr=ptr, ida=ptr, n=6, n_ida=1, ws=w8, c=256, out=ptr):
        return lib.gd4d_cam_gate_fwd(intr, ida, n, n_ida, 1000.0, *ws, c, out, null)
    assert gate(intr=null) == EINVAL and gate(ida=null) == EINVAL and gate(out=null) == EINVAL
    for i in range(8):
        assert gate(ws=w8[:i] + [null] + w8[i + 1:]) == EINVAL
    assert gate(c=128) == EUNSUPPORTED
    assert gate(n=0) == EUNSUPPORTED
    assert gate(n_ida=3) == EUNSUPPORTED                                   # 1 or N ida scales
    assert gate(ws=[ptr, ptr, odd] + w8[3:]) == EALIGN
    # convolution
    lv = (ctypes.c_int32 * 10)(9, 17, 5, 9, 3, 5, 2, 3, 1, 1)
    xs = (ctypes.c_void_p * 5)(*[ptr.value] * 5)
    outs = (ctypes.c_void_p * 5)(*[ptr.value] * 5)
    holes = (ctypes.c_void_p * 5)(ptr.value, None, ptr.value, ptr.value, ptr.value)

    def conv(x=xs, out=outs, hw=lv, levels=4, n=6, c=256, image=ptr, bn=(ptr,) * 5, gate_=ptr):
        return lib.gd4d_depth_conv_fwd(x, out, hw, levels, n, c, image, *bn, 1e-5, gate_, null)
    assert conv(x=null) == EINVAL and conv(out=null) == EINVAL and conv(hw=null) == EINVAL
    assert conv(image=null) == EINVAL and conv(gate_=null) == EINVAL
    for i in range(5):
        assert conv(bn=(ptr,) * i + (null,) + (ptr,) * (4 - i)) == EINVAL
    assert conv(x=holes) == EINVAL and conv(out=holes) == EINVAL           # a level without a map
    assert conv(c=128) == EUNSUPPORTED
    assert conv(levels=5) == EUNSUPPORTED and conv(levels=0) == EUNSUPPORTED
    assert conv(n=0) == EUNSUPPORTED
    assert conv(image=odd) == EALIGN
    zero = (ctypes.c_int32 * 8)(9, 17, 0, 9, 3, 5, 2, 3)
    assert conv(hw=zero) == EINVAL
