"""VoVNet / VoVNetCP without a GPU: the fp64 restatement (vovnet_ref.py) against the reference's recorded maps (tests/golden/
vovnet_tiny.npz, written by tools/gen_golden.py from the reference's own VoVNetCP), the module tree's state-dict keys, freezing, and
the routing errors."""
import functools

import pytest
import torch
import torch.nn as nn

import vovnet_ref as R
from golden_io import Golden

FEATS = ('stem', 'stage2', 'stage3', 'stage4', 'stage5')
V99_NAMES = ['stem.stem_1/conv.weight', 'stage3.OSA3_2.layers.4.OSA3_2_4/norm.running_var', 'stage2.OSA2_1.concat.OSA2_1_concat/conv.weight',
             'stage5.OSA5_3.ese.fc.bias', 'stem.stem_3/norm.num_batches_tracked', 'stage4.OSA4_9.layers.0.OSA4_9_0/conv.weight',
             'stage5.OSA5_1.ese.fc.weight']


@functools.lru_cache(maxsize=None)
def _golden():
    return Golden('vovnet_tiny')


@pytest.fixture
def tiny(monkeypatch):
    """A builder of the fixture's tiny spec, inserted into the package's table (as the generator inserts it into the reference's) for
    the duration of the test."""
    from graph_detr4d_amd import vovnet
    g = _golden()
    monkeypatch.setitem(vovnet._STAGE_SPECS, g.meta['spec_name'], g.meta['spec'])
    return lambda cls_name, **kw: getattr(vovnet, cls_name)(g.meta['spec_name'], out_features=FEATS, **kw)


def _image(g):
    return g.t('img').float() / g.meta['feat_scale']


def test_restatement_reproduces_the_recorded_maps():
    g = _golden()
    outs = R.vovnet(g.state(), _image(g))
    cs = g.meta['chan_stride']
    for f in FEATS:
        ref = outs[f][:, ::cs] if f in ('stem', 'stage2') else outs[f]
        rec = g.t(f)
        assert list(outs[f].shape) == g.meta['shapes'][f] and rec.shape == ref.shape
        err = R.rel_err(rec, ref)
        print(f'vovnet_ref {f}: recorded fp32 against fp64 {err:.3e}')
        assert err <= 1e-6
    assert (outs['stage5'] == 0).all(dim=(2, 3)).any()                      # the fixture has gates of exactly 0: whole planes of zeros


@pytest.mark.parametrize('cls_name', ['VoVNet', 'VoVNetCP'])
def test_state_dict_keys(cls_name, tiny):
    from graph_detr4d_amd import BACKBONES, vovnet
    g = _golden()
    tiny = tiny(cls_name, torch_ops=True)
    assert list(tiny.state_dict()) == g.meta['keys']
    tiny.load_state_dict(g.state(), strict=True)
    assert BACKBONES.get(cls_name) is getattr(vovnet, cls_name)
    v99 = BACKBONES.build(dict(type=cls_name, spec_name='V-99-eSE', norm_eval=True, frozen_stages=-1, input_ch=3,
                               out_features=('stage4', 'stage5')))
    keys = list(v99.state_dict())
    # 3 stem layers and 16 OSA modules of 5 layers + the aggregation, 6 keys per conv + BatchNorm, 2 per eSE fc
    assert len(keys) == 3 * 6 + 16 * (6 * 6 + 2) == 626
    assert all(k in keys for k in V99_NAMES)
    assert v99.state_dict()['stage5.OSA5_2.layers.0.OSA5_2_0/conv.weight'].shape == (224, 1024, 3, 3)
    assert v99.state_dict()['stage5.OSA5_2.concat.OSA5_2_concat/conv.weight'].shape == (1024, 1024 + 5 * 224, 1, 1)


def test_torch_route_reproduces_the_recorded_maps_on_cpu(tiny):
    """The torch-op route is the reference's op sequence: fp32 against the recording to rounding."""
    g = _golden()
    cs = g.meta['chan_stride']
    cp_net = tiny('VoVNetCP', torch_ops=True).eval()
    cp_net.load_state_dict(g.state(), strict=True)
    dict_net = tiny('VoVNet', torch_ops=True).eval()
    dict_net.load_state_dict(g.state(), strict=True)
    with torch.no_grad():
        outs = cp_net(_image(g))
        named = dict_net(_image(g))
    assert isinstance(outs, list) and list(named) == list(FEATS)
    for f, o in zip(FEATS, outs):
        assert torch.equal(o, named[f])
        got = o[:, ::cs] if f in ('stem', 'stage2') else o
        assert R.rel_err(got, g.t(f)) <= 1e-5


def test_freezing(tiny):
    net = tiny('VoVNetCP', torch_ops=True, frozen_stages=2, norm_eval=True)
    assert net.train() is net
    for name in ('stem', 'stage2', 'stage3'):
        m = getattr(net, name)
        assert not m.training and all(not s.training for s in m.modules())
        assert all(not p.requires_grad for p in m.parameters())
    for name in ('stage4', 'stage5'):
        m = getattr(net, name)
        assert m.training and all(p.requires_grad for p in m.parameters())
    assert all(not m.training for m in net.modules() if isinstance(m, nn.BatchNorm2d))
    loose = tiny('VoVNet', torch_ops=True, frozen_stages=-1, norm_eval=False).train()
    assert all(m.training for m in loose.modules() if isinstance(m, nn.BatchNorm2d))
    assert all(p.requires_grad for p in loose.parameters())


@pytest.mark.parametrize('spec_name', ['V-19-slim-dw-eSE', 'V-19-dw-eSE', 'V-19-slim-eSE'])
def test_specs_outside_the_kernels_are_refused_at_construction(spec_name, monkeypatch):
    from graph_detr4d_amd import VoVNet, VoVNetCP, _lib
    monkeypatch.delenv('GD4D_TORCH_OPS', raising=False)
    for cls in (VoVNet, VoVNetCP):
        with pytest.raises(_lib.Gd4dError, match='torch_ops=True'):
            cls(spec_name, out_features=('stage5',))
        net = cls(spec_name, out_features=('stage5',), torch_ops=True).eval()
        with torch.no_grad():
            out = net(torch.zeros(1, 3, 32, 32))
        out = out['stage5'] if cls is VoVNet else out[0]
        assert out.shape[1] == (512 if 'slim' in spec_name else 1024)


def test_kernel_route_refuses_autograd_and_unfrozen_batchnorm(monkeypatch, tiny):
    from graph_detr4d_amd import _lib
    monkeypatch.delenv('GD4D_TORCH_OPS', raising=False)
    net = tiny('VoVNetCP').eval()                                   # parameters require grad, grad mode is on
    x = torch.zeros(1, 3, 32, 32)
    with pytest.raises(_lib.Gd4dError, match='torch_ops=True'):
        net(x)
    loose = tiny('VoVNetCP', norm_eval=False).train()
    with torch.no_grad(), pytest.raises(_lib.Gd4dError, match='torch_ops=True'):
        loose(x)
    with torch.no_grad(), pytest.raises(_lib.Gd4dError, match='GPU'):  # nothing left to object to but the device: no CPU fallback
        net(x)


def test_torch_route_trains_with_checkpointing(tiny):
    net = tiny('VoVNetCP', torch_ops=True, norm_eval=True).train()
    x = torch.randn(1, 3, 32, 32, requires_grad=True)
    outs = net(x)
    sum(o.sum() for o in outs).backward()
    assert x.grad is not None and net.stage5.OSA5_1.ese.fc.weight.grad is not None


def test_network_switch_reaches_every_routed_module(tiny, monkeypatch):
    """`net.torch_ops` and `Fn.torch_ops_for(net)` switch the stem and every OSA module, which decide their route themselves."""
    from graph_detr4d_amd import functional as Fn
    monkeypatch.delenv('GD4D_TORCH_OPS', raising=False)
    net = tiny('VoVNetCP').eval()
    assert len(net._routed()) == 1 + 5 and not net.torch_ops and not any(m.torch_ops for m in net._routed())
    x = torch.zeros(1, 3, 32, 32)
    with torch.no_grad():
        with Fn.torch_ops_for(net):
            assert net.torch_ops and all(m.torch_ops for m in net._routed())
            assert len(net(x)) == len(FEATS)                            # runs on the CPU: the torch-op route
        assert not net.torch_ops and not any(m.torch_ops for m in net._routed())
        net.torch_ops = True
        assert all(m.torch_ops for m in net._routed()) and len(net(x)) == len(FEATS)


def test_with_cp_belongs_to_vovnetcp(tiny):
    from graph_detr4d_amd import vovnet
    assert all(m.with_cp for m in tiny('VoVNetCP', torch_ops=True).modules() if isinstance(m, vovnet._OSA_module))
    assert not any(m.with_cp for m in tiny('VoVNetCP', torch_ops=True, with_cp=False).modules() if isinstance(m, vovnet._OSA_module))
    assert not any(m.with_cp for m in tiny('VoVNet', torch_ops=True).modules() if isinstance(m, vovnet._OSA_module))
    with pytest.raises(TypeError):
        tiny('VoVNet', torch_ops=True, with_cp=True)


def test_wrappers_run_under_the_device_guard():
    """Every public op is rebound to run with its first tensor's device current (ops._on_tensor_device): the VoVNet wrappers too."""
    from graph_detr4d_amd import ops
    for name in ('conv3x3_image', 'conv3x3_bn_relu', 'osa_concat_image', 'osa_concat_conv', 'ese_gate', 'ese_apply'):
        assert hasattr(getattr(ops, name), '__wrapped__'), name
