"""The FPN neck (fpn.py, gd4d_fpn.hip) without a GPU: the fp64 restatement against the modules' torch-op route and the reference
fixture, the nearest-index rule against ATen, state-dict names, the registry, what raises, and the C ABI's argument checks."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

import fpn_ref as R
from golden_io import Golden

FPN_SHIPPED = dict(type='FPN', in_channels=[256, 512, 1024, 2048], out_channels=256, start_level=1, add_extra_convs='on_output',
                   num_outs=4, relu_before_extra_convs=True)
CPFPN_SHIPPED = dict(type='CPFPN', in_channels=[256, 512, 768, 1024], out_channels=256, start_level=0, add_extra_convs='on_output',
                     num_outs=4, relu_before_extra_convs=True)
SMALL = dict(in_channels=[32, 64, 96, 128], out_channels=256)
HW = [(26, 42), (13, 21), (7, 11), (4, 6)]


def _inputs(channels, hw=HW, n=2, seed=3):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, c, *s, generator=g) for c, s in zip(channels, hw)]


def test_nearest_index_rule_is_atens():
    """min(floor(float(dst) * (float(in) / float(out))), in - 1) against F.interpolate for every pair in < 40, in <= out <= 2 in + 1."""
    pairs = 0
    for n_in in range(1, 40):
        src = torch.arange(n_in, dtype=torch.float32).view(1, 1, 1, n_in)
        for n_out in range(n_in, 2 * n_in + 2):
            want = F.interpolate(src, size=(1, n_out), mode='nearest').view(-1).long()
            assert torch.equal(R.nearest_index(torch.arange(n_out), n_in, n_out), want), (n_in, n_out)
            pairs += 1
    assert pairs == 858
    x = torch.randn(2, 3, 7, 11)
    assert torch.equal(R.upsample_nearest(x, (13, 21)), F.interpolate(x, size=(13, 21), mode='nearest'))


@pytest.mark.parametrize('cls, kw', [('FPN', dict(start_level=1, num_outs=5)), ('FPN', dict(start_level=0, num_outs=4)),
                                     ('CPFPN', dict(start_level=0, num_outs=4))])
def test_restatement_agrees_with_the_torch_route(cls, kw):
    import graph_detr4d_amd as G
    torch.manual_seed(1)
    mod = getattr(G, cls)(**SMALL, add_extra_convs='on_output', relu_before_extra_convs=True, torch_ops=True, **kw).eval()
    with torch.no_grad():
        for p in mod.parameters():
            if p.dim() == 1:
                p.normal_(0, 0.1)
    xs = _inputs(SMALL['in_channels'])
    with torch.no_grad():
        got = mod(xs)
    _, ref = R.fpn_forward(mod.state_dict(), xs, start_level=kw['start_level'], num_outs=kw['num_outs'], relu_before_extra_convs=True,
                           cp=cls == 'CPFPN')
    assert len(got) == len(ref) == kw['num_outs']
    for g, r in zip(got, ref):
        assert g.shape == r.shape and R.rel_err(g, r) < 1e-5                 # fp32 convolutions against fp64
    sizes = [tuple(o.shape[2:]) for o in got]
    assert sizes[:len(HW) - kw['start_level']] == HW[kw['start_level']:]
    for a, b in zip(sizes[len(HW) - kw['start_level'] - 1:], sizes[len(HW) - kw['start_level']:]):
        assert b == ((a[0] + 1) // 2, (a[1] + 1) // 2)                       # an extra level: (H + 1) // 2


def test_restatement_and_module_agree_with_the_reference_fixture():
    import graph_detr4d_amd as G
    g = Golden('fpn_cp')
    m = g.meta
    sd = g.state()
    xs = [g.t(f'in{i}').float() / m['feat_scale'] for i in range(len(m['cfg']['in_channels']))]
    assert [tuple(x.shape[2:]) for x in xs] == [tuple(hw) for hw in m['levels']] and xs[0].shape[0] == m['num_cams']
    lats, outs = R.fpn_forward(sd, xs, start_level=0, num_outs=m['cfg']['num_outs'], relu_before_extra_convs=True, cp=True)
    mod = G.CPFPN(**m['cfg'], torch_ops=True).eval()
    mod.load_state_dict(sd, strict=True)
    with torch.no_grad():
        tor = mod(xs)
    cs = m['chan_stride']
    assert R.rel_err(lats[0][:, ::cs], g.t('lat0')) < 1e-5
    for lvl in range(m['cfg']['num_outs']):
        ref = g.t(f'out{lvl}')
        pick = (lambda t: t[:, ::cs]) if lvl == 0 else (lambda t: t)
        assert pick(outs[lvl]).shape == ref.shape
        assert R.rel_err(pick(outs[lvl]), ref) < 1e-5 and R.rel_err(pick(tor[lvl]), ref) < 1e-5
    assert float(g.t('out0').abs().max()) > 0.5 and not torch.equal(outs[1].float(), lats[1].float() * 0)


def test_state_dict_names_strict_load_and_registry():
    import graph_detr4d_amd as G
    fpn, cp = G.build_neck(FPN_SHIPPED), G.build_neck(CPFPN_SHIPPED)
    assert type(fpn) is G.FPN and type(cp) is G.CPFPN and G.NECKS.get('FPN') is G.FPN and G.NECKS.get('CPFPN') is G.CPFPN
    keys = lambda name, n: [f'{name}.{i}.conv.{t}' for i in range(n) for t in ('weight', 'bias')]                        # noqa: E731
    assert list(fpn.state_dict()) == keys('lateral_convs', 3) + keys('fpn_convs', 4)      # three output convolutions + one extra
    assert list(cp.state_dict()) == keys('lateral_convs', 4) + keys('fpn_convs', 1)       # level 0's only
    assert tuple(fpn.lateral_convs[0].conv.weight.shape) == (256, 512, 1, 1) and fpn.fpn_convs[3].conv.stride == (2, 2)
    assert float(fpn.lateral_convs[0].conv.bias.detach().abs().max()) == 0                         # the default init_cfg: Xavier, zero biases
    g = Golden('fpn_cp')
    small = G.CPFPN(**g.meta['cfg'])
    assert sorted(small.state_dict()) == sorted(g.state())                                # the keys the reference module saved
    small.load_state_dict(g.state(), strict=True)
    other = G.FPN(**{k: v for k, v in FPN_SHIPPED.items() if k != 'type'})
    other.load_state_dict(fpn.state_dict(), strict=True)


@pytest.mark.parametrize('kw', [dict(out_channels=128), dict(end_level=3, num_outs=3), dict(upsample_cfg=dict(mode='bilinear')),
                                dict(upsample_cfg=dict(scale_factor=2, mode='nearest')), dict(add_extra_convs='on_input', num_outs=5),
                                dict(add_extra_convs='on_lateral', num_outs=5), dict(add_extra_convs=True, num_outs=5),
                                dict(add_extra_convs=False, num_outs=5), dict(in_channels=[32, 64, 96, 100])],
                         ids=lambda kw: ','.join(kw))
def test_unsupported_keywords_raise_at_construction(kw, monkeypatch):
    import graph_detr4d_amd as G
    from graph_detr4d_amd._lib import Gd4dError
    monkeypatch.delenv('GD4D_TORCH_OPS', raising=False)
    cfg = dict(SMALL, num_outs=4, add_extra_convs='on_output')
    cfg.update(kw)
    for cls in (G.FPN, G.CPFPN):
        if cls is G.CPFPN and cfg['add_extra_convs'] and cfg['num_outs'] > 4:
            continue                                                           # (refused for a reason of its own, below)
        with pytest.raises(Gd4dError, match='torch_ops'):
            cls(**cfg)
        mod = cls(**cfg, torch_ops=True).eval()                                # the explicit choice builds and runs
        pow2 = [(32, 48), (16, 24), (8, 12), (4, 6)]                           # (a fixed scale_factor of 2 needs exact halvings)
        with torch.no_grad():
            outs = mod(_inputs(cfg['in_channels'], pow2))
        assert len(outs) == cfg['num_outs'] and all(o.shape[1] == cfg['out_channels'] for o in outs)
        mod.torch_ops = False                                                  # ... and cannot be switched onto the kernels afterwards
        with torch.no_grad(), pytest.raises(Gd4dError, match='torch_ops'):
            mod(_inputs(cfg['in_channels'], pow2))


@pytest.mark.parametrize('kw', [dict(norm_cfg=dict(type='BN')), dict(act_cfg=dict(type='ReLU')), dict(conv_cfg=dict(type='Conv2d'))],
                         ids=lambda kw: ','.join(kw))
def test_layer_configs_raise_on_both_routes(kw):
    import graph_detr4d_amd as G
    from graph_detr4d_amd._lib import Gd4dError
    for cls in (G.FPN, G.CPFPN):
        for torch_ops in (False, True):
            with pytest.raises(Gd4dError, match='torch_ops'):
                cls(**SMALL, num_outs=4, torch_ops=torch_ops, **kw)


def test_cpfpn_refuses_what_the_reference_cannot_run():
    import graph_detr4d_amd as G
    from graph_detr4d_amd._lib import Gd4dError
    with pytest.raises(Gd4dError, match='IndexError'):
        G.CPFPN(**SMALL, num_outs=5, add_extra_convs='on_output', torch_ops=True)
    with pytest.raises(Gd4dError, match='start_level'):
        G.CPFPN(**SMALL, num_outs=3, start_level=1, torch_ops=True)


def test_train_mode_autograd_and_cpu_maps_raise(monkeypatch):
    import graph_detr4d_amd as G
    from graph_detr4d_amd._lib import Gd4dError
    monkeypatch.delenv('GD4D_TORCH_OPS', raising=False)
    xs = _inputs(SMALL['in_channels'])
    for cls in (G.FPN, G.CPFPN):
        mod = cls(**SMALL, num_outs=4)
        with torch.no_grad(), pytest.raises(Gd4dError, match='no CPU fallback'):
            mod.eval()(xs)
    # the mode and autograd checks come before any device work: a stand-in for the GPU check lets them be seen here
    from graph_detr4d_amd import functional as Fn
    monkeypatch.setattr(Fn, 'require_gpu', lambda t, name: None)
    for cls in (G.FPN, G.CPFPN):
        mod = cls(**SMALL, num_outs=4)
        with torch.no_grad(), pytest.raises(Gd4dError, match='train.*torch_ops=True'):
            mod.train()(xs)
        with pytest.raises(Gd4dError, match='autograd.*torch_ops=True'):
            mod.eval()(xs)                                                     # parameters require grad
        for p in mod.parameters():
            p.requires_grad_(False)
        with pytest.raises(Gd4dError, match='autograd.*torch_ops=True'):
            mod([x.clone().requires_grad_() for x in xs])                      # an input requires grad
        mod.torch_ops = True                                                   # the torch route trains
        for p in mod.parameters():
            p.requires_grad_(True)
        sum(o.sum() for o in mod.train()(xs)).backward()
        assert mod.lateral_convs[0].conv.weight.grad is not None
    monkeypatch.setenv('GD4D_TORCH_OPS', '1')
    assert len(G.FPN(**SMALL, num_outs=4)(xs)) == 4                            # the process-wide switch


def test_abi_stays_56_and_declares_the_new_entry_points(repo_root):
    from graph_detr4d_amd import _lib
    hdr = open(os.path.join(repo_root, 'include', 'gd4d.h')).read()
    assert re.search(r'#define GD4D_ABI_VERSION 56\b', hdr) and _lib.ABI_VERSION == 56 and _lib.load().gd4d_abi_version() == 56
    for name in ('gd4d_fpn_lateral_image_bytes', 'gd4d_fpn_lateral_image', 'gd4d_fpn_lateral_fwd', 'gd4d_fpn_conv_fwd',
                 'gd4d_fpn_extra_conv_fwd'):
        assert name in _lib.SIGNATURES and re.search(rf'\b{name}\s*\(', hdr)


def test_entry_points_validate_before_any_gpu_work():
    from graph_detr4d_amd import _lib
    lib = _lib.load()
    EINVAL, EUNSUPPORTED, EALIGN = -1, -2, -3
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 96)()
    ptr = ctypes.c_void_p((ctypes.addressof(buf) + 63) & ~63)               # 64-byte aligned: alignment checks pass
    odd = ctypes.c_void_p(ptr.value + 4)
    # image
    assert lib.gd4d_fpn_lateral_image_bytes(512) == 16 * 32768 and lib.gd4d_fpn_lateral_image_bytes(2048) == 64 * 32768
    for cin in (0, 16, 48, 2080, -32):
        assert lib.gd4d_fpn_lateral_image_bytes(cin) == 0
        assert lib.gd4d_fpn_lateral_image(ptr, cin, 256, ptr, null) == EUNSUPPORTED
    assert lib.gd4d_fpn_lateral_image(null, 64, 256, ptr, null) == EINVAL and lib.gd4d_fpn_lateral_image(ptr, 64, 256, null, null) == EINVAL
    assert lib.gd4d_fpn_lateral_image(ptr, 64, 128, ptr, null) == EUNSUPPORTED
    assert lib.gd4d_fpn_lateral_image(ptr, 64, 256, odd, null) == EALIGN

    # lateral
    def lat(x=ptr, n=2, cin=64, h=13, w=21, image=ptr, bias=ptr, up=null, uh=0, uw=0, up_cl=0, out=ptr, c=256, out_cl=0):
        return lib.gd4d_fpn_lateral_fwd(x, n, cin, h, w, image, bias, up, uh, uw, up_cl, out, c, out_cl, null)
    assert lat(x=null) == EINVAL and lat(image=null) == EINVAL and lat(bias=null) == EINVAL and lat(out=null) == EINVAL
    assert lat(h=0) == EINVAL and lat(w=-1) == EINVAL and lat(up=ptr, uh=0, uw=11) == EINVAL
    assert lat(c=128) == EUNSUPPORTED and lat(n=0) == EUNSUPPORTED and lat(cin=48) == EUNSUPPORTED and lat(cin=4096) == EUNSUPPORTED
    assert lat(out_cl=2) == EUNSUPPORTED and lat(up_cl=-1) == EUNSUPPORTED
    assert lat(up=ptr, uh=14, uw=11) == EUNSUPPORTED                          # the top-down path only upsamples
    assert lat(image=odd) == EALIGN and lat(out=odd, out_cl=1) == EALIGN and lat(up=odd, uh=7, uw=11, up_cl=1) == EALIGN

    # 3x3 output convolutions
    lv = (ctypes.c_int32 * 10)(9, 17, 5, 9, 3, 5, 2, 3, 1, 1)
    five = (ctypes.c_void_p * 5)(*[ptr.value] * 5)
    holes = (ctypes.c_void_p * 5)(ptr.value, None, ptr.value, ptr.value, ptr.value)
    odds = (ctypes.c_void_p * 5)(ptr.value, odd.value, ptr.value, ptr.value, ptr.value)

    def conv(x=five, out=five, hw=lv, levels=4, n=2, c=256, images=five, biases=five, cl=0):
        return lib.gd4d_fpn_conv_fwd(x, out, hw, levels, n, c, images, biases, cl, null)
    assert conv(x=null) == EINVAL and conv(out=null) == EINVAL and conv(hw=null) == EINVAL and conv(images=null) == EINVAL
    assert conv(x=holes) == EINVAL and conv(out=holes) == EINVAL and conv(images=holes) == EINVAL
    assert conv(c=128) == EUNSUPPORTED and conv(levels=5) == EUNSUPPORTED and conv(levels=0) == EUNSUPPORTED and conv(n=0) == EUNSUPPORTED
    assert conv(cl=2) == EUNSUPPORTED
    assert conv(images=odds) == EALIGN and conv(out=odds, cl=1) == EALIGN
    assert conv(hw=(ctypes.c_int32 * 8)(9, 17, 0, 9, 3, 5, 2, 3)) == EINVAL

    # extra level
    def extra(x=ptr, n=2, c=256, h=4, w=6, in_cl=0, image=ptr, bias=ptr, relu=0, out=ptr, out_cl=0):
        return lib.gd4d_fpn_extra_conv_fwd(x, n, c, h, w, in_cl, image, bias, relu, out, out_cl, null)
    assert extra(x=null) == EINVAL and extra(image=null) == EINVAL and extra(out=null) == EINVAL and extra(h=0) == EINVAL
    assert extra(c=128) == EUNSUPPORTED and extra(n=0) == EUNSUPPORTED
    assert extra(in_cl=2) == EUNSUPPORTED and extra(out_cl=2) == EUNSUPPORTED and extra(relu=2) == EUNSUPPORTED
    assert extra(image=odd) == EALIGN and extra(out=odd, out_cl=1) == EALIGN


def test_ops_refuse_cpu_tensors():
    from graph_detr4d_amd import _lib, ops
    z = torch.zeros
    with pytest.raises(_lib.Gd4dError):
        ops.fpn_lateral_image(z(256, 64, 1, 1))
    with pytest.raises(_lib.Gd4dError):
        ops.fpn_lateral_image(z(256, 48, 1, 1))
    with pytest.raises(_lib.Gd4dError):
        ops.fpn_lateral_fwd(z(2, 64, 4, 6), z(16, dtype=torch.uint8), z(256), out=z(2, 256, 4, 6))
    with pytest.raises(_lib.Gd4dError):
        ops.fpn_conv_fwd([z(2, 256, 4, 6)], [z(16, dtype=torch.uint8)], [z(256)], outs=[z(2, 256, 4, 6)])
    with pytest.raises(_lib.Gd4dError):
        ops.fpn_extra_conv_fwd(z(2, 256, 4, 6), z(16, dtype=torch.uint8), z(256), out=z(2, 256, 2, 3))
