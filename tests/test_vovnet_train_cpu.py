"""VoVNet training on the library's kernels (vovnet.py hip_train=True, gd4d_vovnet_train.hip) without a GPU: the fp64 closed form
(vovnet_train_ref.py) against fp64 autograd of the module's own torch layers, the keyword and the network property, what is refused, that
nothing differs with the switch off, and the C ABI's argument checks."""
import ctypes
import os
import re

import pytest
import torch

import vovnet_ref as R
import vovnet_train_ref as T

NEW_SYMBOLS = ('gd4d_conv3x3_image_t_bytes', 'gd4d_conv3x3_image_t', 'gd4d_osa_concat_image_t_bytes', 'gd4d_osa_concat_image_t',
               'gd4d_conv3x3_dgrad', 'gd4d_osa_concat_dgrad', 'gd4d_conv3x3_wgrad_tiles', 'gd4d_osa_concat_wgrad_tiles',
               'gd4d_conv_wgrad_workspace_bytes', 'gd4d_conv3x3_wgrad', 'gd4d_osa_concat_wgrad', 'gd4d_ese_bwd_workspace_bytes', 'gd4d_ese_bwd')
NEW_OPS = ('conv3x3_image_t', 'osa_concat_image_t', 'conv3x3_dgrad', 'osa_concat_dgrad', 'conv3x3_wgrad', 'osa_concat_wgrad', 'ese_bwd')


def _rand(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ---- the closed form ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('identity', [False, True], ids=['plain', 'identity'])
def test_closed_form_agrees_with_fp64_autograd(identity):
    """(128 -> 160, 13 x 21) with randomize_'s statistics, linearised at the fp64 forward itself: every gradient within 1e-10 of its
    largest entry - the dgamma identity included, which never forms a pre-BatchNorm map."""
    from graph_detr4d_amd import vovnet
    in_ch, concat_ch = (256, 256) if identity else (128, 256)
    m = R.randomize_(vovnet._OSA_module(in_ch, 160, concat_ch, 5, 'OSA3_2', identity=identity, torch_ops=True), seed=40).eval().double()
    x = torch.relu(_rand(2, in_ch, 13, 21, seed=41).double()).requires_grad_(True)
    dout = _rand(2, concat_ch, 13, 21, seed=42).double()
    out = m(x)
    (out * dout).sum().backward()
    with torch.no_grad():                                                      # the fp64 forward's own maps
        maps = [x.detach()]
        for layer in m.layers:
            maps.append(layer(maps[-1]))
        xt = m.concat(torch.cat(maps, dim=1))
        gate = R.ese_gate(xt.mean(dim=(2, 3)), m.ese.fc.weight, m.ese.fc.bias)
    assert (gate == 0).any() and (gate == 1).any() and ((gate > 0) & (gate < 1)).any()      # randomize_ saturates some gates
    dx, grads = T.osa_backward(m.state_dict(), '', 'OSA3_2', maps, xt, gate, dout, identity)
    assert T.rel_err(dx, x.grad) <= 1e-10
    names = dict(m.named_parameters())
    assert set(grads) == set(names)
    for k, p in names.items():
        assert T.rel_err(grads[k], p.grad) <= 1e-10, k


# ---- the switch ------------------------------------------------------------------------------------------------------------------
def test_keyword_on_all_four_classes_and_the_network_property():
    from graph_detr4d_amd import VoVNet, VoVNetCP, build_backbone, vovnet
    assert vovnet._OSA_module(128, 128, 256, 5, 'OSA2_1', hip_train=True).hip_train is True
    assert vovnet._OSA_module(128, 128, 256, 5, 'OSA2_1').hip_train is False
    assert vovnet._Stem(3, [64, 64, 128], False, False, hip_train=True).hip_train is True
    for cls in (VoVNet, VoVNetCP):
        net = cls('V-19-eSE', out_features=('stage5',), hip_train=True)
        assert net.hip_train is True and len(net._routed()) == 5 and all(m.hip_train for m in net._routed()) and not net.torch_ops
        net.hip_train = False
        assert net.hip_train is False and not any(m.hip_train for m in net._routed())
        assert cls('V-19-eSE', out_features=('stage5',)).hip_train is False
    built = build_backbone(dict(type='VoVNetCP', spec_name='V-19-eSE', out_features=('stage4', 'stage5'), hip_train=True))
    assert type(built) is VoVNetCP and built.hip_train and all(m.with_cp for m in built.modules() if isinstance(m, vovnet._OSA_module))


def test_torch_ops_wins_over_hip_train():
    from graph_detr4d_amd import VoVNetCP
    net = VoVNetCP('V-19-eSE', out_features=('stage5',), torch_ops=True, hip_train=True).train()
    x = torch.randn(1, 3, 32, 32, requires_grad=True)
    net(x)[0].sum().backward()                                                  # CPU tensors: only the torch route can have run
    assert x.grad is not None and net.stage5.OSA5_1.ese.fc.weight.grad is not None


def test_unfrozen_batchnorm_is_refused_naming_torch_ops(monkeypatch):
    from graph_detr4d_amd import VoVNetCP, _lib
    monkeypatch.delenv('GD4D_TORCH_OPS', raising=False)
    net = VoVNetCP('V-19-eSE', out_features=('stage5',), norm_eval=False, hip_train=True).train()
    x = torch.zeros(1, 3, 32, 32)
    with pytest.raises(_lib.Gd4dError, match=r'hip_train=True.*frozen BatchNorms only.*torch_ops=True'):
        net(x)                                                                  # the stem is the first to refuse
    with pytest.raises(_lib.Gd4dError, match=r'_OSA_module.*frozen BatchNorms only.*torch_ops=True'):
        net.stage2.OSA2_1(torch.zeros(1, 128, 8, 8))
    with torch.no_grad(), pytest.raises(_lib.Gd4dError, match='frozen BatchNorms only'):
        net.stage2.OSA2_1(torch.zeros(1, 128, 8, 8))
    # frozen: nothing left to object to but the device - the training route has no CPU fallback either
    frozen = VoVNetCP('V-19-eSE', out_features=('stage5',), norm_eval=True, hip_train=True).train()
    with pytest.raises(_lib.Gd4dError, match='GPU'):
        frozen.stage2.OSA2_1(torch.zeros(1, 128, 8, 8))


def test_with_the_switch_off_routing_is_what_it_was(monkeypatch):
    """Route for route and message for message: the refusals of a module without the switch (they do not mention hip_train)."""
    from graph_detr4d_amd import VoVNetCP, _lib, kernel_route
    monkeypatch.delenv('GD4D_TORCH_OPS', raising=False)
    net = VoVNetCP('V-19-eSE', out_features=('stage5',)).eval()
    mod, x = net.stage2.OSA2_1, torch.zeros(1, 128, 8, 8)

    class Plain(kernel_route.KernelRoute, torch.nn.Module):                    # the skeleton's own answers, no switch at all
        _kernels = type(mod)._kernels

        def __init__(self):
            torch.nn.Module.__init__(self)
            self.p = torch.nn.Parameter(torch.zeros(1))
            self._init_route(False)

        def _route_name(self):
            return mod._route_name()

    def message(fn):
        with pytest.raises(_lib.Gd4dError) as e:
            fn()
        return str(e.value)
    plain = Plain().eval()
    assert message(lambda: mod._route(x)) == message(lambda: plain._route(x)) and 'hip_train' not in message(lambda: mod._route(x))
    with torch.no_grad():
        assert message(lambda: mod._route(x)) == message(lambda: plain._route(x))          # the device
        mod.train()                                                                         # (a BatchNorm in train mode)
        assert message(lambda: mod._route(x)) == message(lambda: plain.train()._route(x)) and 'hip_train' not in message(lambda: mod._route(x))
    mod.eval()
    monkeypatch.setattr(kernel_route.Fn, 'require_gpu', lambda t, name: None)
    with torch.no_grad():
        assert mod._route(x) == 'infer'
        mod.hip_train = True
        assert mod._route(x) == 'infer'                                         # nothing wants a gradient: the inference launches
    assert mod._route(x) == 'train'
    mod.requires_grad_(False)
    assert mod._route(x) == 'infer' and mod._route(x.clone().requires_grad_(True)) == 'train'


def test_frozen_stages_keep_the_inference_route(monkeypatch):
    from graph_detr4d_amd import VoVNetCP, kernel_route
    monkeypatch.delenv('GD4D_TORCH_OPS', raising=False)
    monkeypatch.setattr(kernel_route.Fn, 'require_gpu', lambda t, name: None)
    net = VoVNetCP('V-19-eSE', out_features=('stage5',), frozen_stages=2, hip_train=True).train()
    x = torch.zeros(1, 3, 32, 32)
    assert net.stem._route(x) == 'infer' and net.stage2.OSA2_1._route(x) == 'infer' and net.stage3.OSA3_1._route(x) == 'infer'
    assert net.stage4.OSA4_1._route(x) == 'train'


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_abi_stays_56_and_declares_the_training_entry_points(repo_root):
    from graph_detr4d_amd import _lib
    hdr = open(os.path.join(repo_root, 'include', 'gd4d.h')).read()
    assert re.search(r'#define GD4D_ABI_VERSION 56\b', hdr) and _lib.ABI_VERSION == 56 and _lib.load().gd4d_abi_version() == 56
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and re.search(rf'\b{name}\s*\(', hdr) and hasattr(lib, name), name


def test_training_entry_points_validate_before_any_gpu_work():
    from graph_detr4d_amd import _lib
    lib = _lib.load()
    EINVAL, EUNSUPPORTED, EALIGN = -1, -2, -3
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 96)()
    ptr = ctypes.c_void_p((ctypes.addressof(buf) + 63) & ~63)
    odd = ctypes.c_void_p(ptr.value + 4)
    # images: the forward's sizes and limits
    assert lib.gd4d_conv3x3_image_t_bytes(64, 128) == lib.gd4d_conv3x3_image_bytes(64, 128) == 128 * 64 * 9 * 4
    assert lib.gd4d_conv3x3_image_t_bytes(48, 64) == 0 and lib.gd4d_conv3x3_image_t_bytes(64, 288) == 0
    assert lib.gd4d_osa_concat_image_t_bytes(2144, 1024) == 1024 * 2144 * 4 and lib.gd4d_osa_concat_image_t_bytes(2336, 1024) == 0
    for fn, a, b in ((lib.gd4d_conv3x3_image_t, 64, 64), (lib.gd4d_osa_concat_image_t, 128, 64)):
        assert fn(null, a, b, ptr, null) == EINVAL and fn(ptr, a, b, null, null) == EINVAL
        assert fn(ptr, 48, b, ptr, null) == EUNSUPPORTED and fn(ptr, a, b, odd, null) == EALIGN

    def dgrad(dz=ptr, n=2, cin=64, cout=64, h=5, w=7, image=ptr, dx=ptr, mt=0):
        return lib.gd4d_conv3x3_dgrad(dz, n, cin, cout, h, w, image, null, null, null, dx, mt, null)
    assert dgrad(dz=null) == EINVAL and dgrad(image=null) == EINVAL and dgrad(dx=null) == EINVAL
    assert dgrad(cin=48) == EUNSUPPORTED and dgrad(cout=288) == EUNSUPPORTED and dgrad(cin=2048) == EUNSUPPORTED and dgrad(n=0) == EUNSUPPORTED
    assert dgrad(h=0) == EUNSUPPORTED and dgrad(mt=3) == EUNSUPPORTED and dgrad(mt=6) == EUNSUPPORTED and dgrad(image=odd) == EALIGN

    chans = (ctypes.c_int32 * 2)(64, 64)
    dsts = (ctypes.c_void_p * 2)(ptr.value, ptr.value)

    def odgrad(dz=ptr, n=2, cout=64, h=5, w=7, image=ptr, dst=dsts, ch=chans, nd=2, mt=0):
        return lib.gd4d_osa_concat_dgrad(dz, n, cout, h, w, image, dst, ch, nd, null, mt, null)
    assert odgrad(dz=null) == EINVAL and odgrad(image=null) == EINVAL and odgrad(dst=null) == EINVAL and odgrad(ch=null) == EINVAL
    assert odgrad(dst=(ctypes.c_void_p * 2)(ptr.value, None)) == EINVAL                                   # a NULL destination
    assert odgrad(nd=0) == EUNSUPPORTED and odgrad(nd=7) == EUNSUPPORTED and odgrad(cout=48) == EUNSUPPORTED and odgrad(w=0) == EUNSUPPORTED
    assert odgrad(ch=(ctypes.c_int32 * 2)(64, 48)) == EUNSUPPORTED and odgrad(mt=4) == EUNSUPPORTED and odgrad(image=odd) == EALIGN

    assert lib.gd4d_conv3x3_wgrad_tiles(2, 13, 21) == 4 and lib.gd4d_conv3x3_wgrad_tiles(2, 17, 16) == 4 and lib.gd4d_conv3x3_wgrad_tiles(0, 5, 7) == 0
    assert lib.gd4d_osa_concat_wgrad_tiles(2, 13, 21) == 10 and lib.gd4d_osa_concat_wgrad_tiles(2, 0, 21) == 0
    assert lib.gd4d_conv_wgrad_workspace_bytes(64, 128, 9, 3) == 3 * (9 * 128 * 64 + 128) * 4
    assert lib.gd4d_conv_wgrad_workspace_bytes(2144, 1024, 1, 2) == 2 * (1024 * 2144 + 1024) * 4
    assert lib.gd4d_conv_wgrad_workspace_bytes(2144, 1024, 9, 2) == 0 and lib.gd4d_conv_wgrad_workspace_bytes(64, 64, 3, 2) == 0
    assert lib.gd4d_conv_wgrad_workspace_bytes(64, 64, 9, 0) == 0 and lib.gd4d_conv_wgrad_workspace_bytes(64, 64, 9, 4097) == 0

    def wgrad(dz=ptr, x=ptr, n=2, cin=64, cout=64, h=5, w=7, parts=2, ws=ptr, weight=ptr, bn=ptr, dw=ptr, dg=ptr, db=ptr):
        return lib.gd4d_conv3x3_wgrad(dz, x, n, cin, cout, h, w, parts, ws, weight, bn, dw, dg, db, null)
    assert wgrad(dz=null) == EINVAL and wgrad(x=null) == EINVAL and wgrad(ws=null) == EINVAL and wgrad(weight=null) == EINVAL
    assert wgrad(bn=null) == EINVAL and wgrad(dw=null, dg=null, db=null) == EINVAL
    assert wgrad(cin=48) == EUNSUPPORTED and wgrad(cout=288) == EUNSUPPORTED and wgrad(n=0) == EUNSUPPORTED and wgrad(parts=0) == EUNSUPPORTED
    assert wgrad(parts=4097) == EUNSUPPORTED and wgrad(h=-1) == EUNSUPPORTED and wgrad(ws=odd) == EALIGN

    srcs = (ctypes.c_void_p * 2)(ptr.value, ptr.value)

    def owgrad(dz=ptr, sums=ptr, src=srcs, ch=chans, ns=2, n=2, h=5, w=7, cout=64, parts=2, ws=ptr, weight=ptr, bn=ptr, dw=ptr):
        return lib.gd4d_osa_concat_wgrad(dz, sums, src, ch, ns, n, h, w, cout, parts, ws, weight, bn, dw, null, null, null)
    assert owgrad(dz=null) == EINVAL and owgrad(sums=null) == EINVAL and owgrad(src=null) == EINVAL and owgrad(ws=null) == EINVAL
    assert owgrad(dw=null) == EINVAL and owgrad(src=(ctypes.c_void_p * 2)(ptr.value, None)) == EINVAL
    assert owgrad(ns=7) == EUNSUPPORTED and owgrad(cout=1056) == EUNSUPPORTED and owgrad(parts=0) == EUNSUPPORTED and owgrad(n=0) == EUNSUPPORTED
    assert owgrad(ch=(ctypes.c_int32 * 2)(64, 48)) == EUNSUPPORTED and owgrad(ws=odd) == EALIGN

    assert lib.gd4d_ese_bwd_workspace_bytes(2, 256) == 4 * 2 * 256 * 4
    assert lib.gd4d_ese_bwd_workspace_bytes(2, 48) == 0 and lib.gd4d_ese_bwd_workspace_bytes(2, 1056) == 0 and lib.gd4d_ese_bwd_workspace_bytes(0, 256) == 0

    def ese(dout=ptr, xt=ptr, partials=ptr, tiles=1, gate=ptr, fc_w=ptr, n=2, c=64, hw=35, ws=ptr, dz=ptr, sums=ptr):
        return lib.gd4d_ese_bwd(dout, xt, partials, tiles, gate, fc_w, n, c, hw, ws, dz, sums, null, null, null)
    assert ese(dout=null) == EINVAL and ese(xt=null) == EINVAL and ese(partials=null) == EINVAL and ese(gate=null) == EINVAL
    assert ese(fc_w=null) == EINVAL and ese(ws=null) == EINVAL and ese(dz=null) == EINVAL and ese(sums=null) == EINVAL
    assert ese(c=48) == EUNSUPPORTED and ese(c=1056) == EUNSUPPORTED and ese(n=0) == EUNSUPPORTED and ese(tiles=0) == EUNSUPPORTED and ese(hw=0) == EUNSUPPORTED


def test_wrappers_carry_the_device_guard_and_refuse_cpu_tensors():
    from graph_detr4d_amd import _lib, ops
    for name in NEW_OPS:
        assert hasattr(getattr(ops, name), '__wrapped__'), name
    z = torch.zeros
    img = z(64 * 64 * 9 * 4, dtype=torch.uint8)
    with pytest.raises(_lib.Gd4dError):
        ops.conv3x3_image_t(z(64, 64, 3, 3), z(64))
    with pytest.raises(_lib.Gd4dError):
        ops.conv3x3_image_t(z(64, 48, 3, 3))
    with pytest.raises(_lib.Gd4dError):
        ops.osa_concat_image_t(z(64, 128, 1, 1), z(64))
    with pytest.raises(_lib.Gd4dError):
        ops.conv3x3_dgrad(z(2, 64, 5, 7), img, 64)
    with pytest.raises(_lib.Gd4dError):
        ops.osa_concat_dgrad(z(2, 64, 5, 7), z(128 * 64 * 4, dtype=torch.uint8), [64, 64])
    with pytest.raises(_lib.Gd4dError):
        ops.conv3x3_wgrad(z(2, 64, 5, 7), z(2, 64, 5, 7), z(64, 64, 3, 3), z(3, 64), partitions=1)
    with pytest.raises(_lib.Gd4dError):
        ops.osa_concat_wgrad(z(2, 64, 5, 7), z(2, 64), [z(2, 64, 5, 7)] * 2, z(64, 128, 1, 1), z(3, 64), partitions=1)
    with pytest.raises(_lib.Gd4dError):
        ops.ese_bwd(z(2, 64, 5, 7), z(2, 64, 5, 7), z(2, 1, 64), z(2, 64), z(64, 64, 1, 1))
