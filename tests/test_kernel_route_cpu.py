"""The one route rule (kernel_route.KernelRoute._route) as every module that mixes it in shows it, on small CPU tensors: the chosen
torch-op route runs, and the refusals come in the one order - limits, train mode, autograd, and the device last.

DepthNet refuses CPU maps on every route with one line in front of the rule, so through its public call nothing but that refusal can
be seen without a GPU: its case asks the rule itself (`_route`, what `forward_levels` calls next) for the order, and the public call
for the refusal."""
import numpy as np
import pytest
import torch

TINY_SPEC = dict(stem=[32, 32, 32], stage_conv_ch=[32, 32, 32, 32], stage_out_ch=[32, 32, 32, 32], layer_per_block=1,
                 block_per_stage=[1, 1, 1, 1], eSE=True, dw=False)
ODD_SPEC = dict(TINY_SPEC, stem=[32, 32, 48])            # 48 channels, no multiple of 32, in the stem: the first module called
FPN_CH = [32, 64, 96, 128]
FPN_HW = [(8, 12), (4, 6), (2, 3), (1, 2)]


class Case:
    """make(outside=False, **switches) builds the module; args() its small CPU inputs; call(module, args) the public call."""
    hip_train = True                  # the module has that switch
    refused_at_construction = False   # ... outside the limits (else at the call)
    serves_cpu = True                 # the chosen torch-op route runs on CPU tensors

    def rule(self, mod, args):
        return self.call(mod, args)


class DepthNetCase(Case):
    serves_cpu = False

    def make(self, outside=False, **kw):
        from graph_detr4d_amd import DepthNet
        c = 128 if outside else 256
        return DepthNet(c, c, 80, **kw)

    def args(self, mod):
        c = mod.reduce_conv[0].in_channels
        k = np.eye(4, dtype=np.float32)
        k[0, 0] = k[1, 1] = 1200.0
        return [torch.zeros(1, 2, c, 3, 4)], [dict(intrinsics=[k, k], ida_mats=[torch.eye(3)])]

    def call(self, mod, args):
        return mod.forward_levels(*args)

    def rule(self, mod, args):
        return mod._route(*[f[0] for f in args[0]])


class FpnCase(Case):
    refused_at_construction = True

    def __init__(self, name):
        self.name = name

    def make(self, outside=False, **kw):
        import graph_detr4d_amd as G
        return getattr(G, self.name)(in_channels=FPN_CH, out_channels=128 if outside else 256, num_outs=4, **kw)

    def args(self, mod):
        return [torch.zeros(1, c, *hw) for c, hw in zip(FPN_CH, FPN_HW)]

    def call(self, mod, args):
        return mod(args)


class DcnCase(Case):
    def __init__(self, name):
        self.name = name

    def make(self, outside=False, **kw):
        import graph_detr4d_amd as G
        geometry = dict(padding=2, dilation=2) if outside else dict(padding=1)
        return getattr(G, self.name)(64, 64, 3, **geometry, **kw)

    def args(self, mod):
        z = torch.zeros
        return (z(1, 64, 5, 7),) if self.name.endswith('Pack') else (z(1, 64, 5, 7), z(1, 18, 5, 7), z(1, 9, 5, 7))

    def call(self, mod, args):
        return mod(*args)


class VoVNetCase(Case):
    hip_train = False
    refused_at_construction = True

    def make(self, outside=False, **kw):
        from graph_detr4d_amd import VoVNetCP
        # norm_eval=False: train() reaches the BatchNorms, which is what train mode means for this network
        return VoVNetCP('odd' if outside else 'tiny', out_features=('stage5',), norm_eval=False, **kw)

    def args(self, mod):
        return torch.zeros(1, 3, 32, 32)

    def call(self, mod, args):
        return mod(args)


CASES = {'DepthNet': DepthNetCase(), 'FPN': FpnCase('FPN'), 'CPFPN': FpnCase('CPFPN'),
         'ModulatedDeformConv2d': DcnCase('ModulatedDeformConv2d'), 'ModulatedDeformConv2dPack': DcnCase('ModulatedDeformConv2dPack'),
         'VoVNet': VoVNetCase()}


@pytest.mark.parametrize('name', list(CASES))
def test_the_route_rule_in_its_one_order(name, monkeypatch):
    from graph_detr4d_amd import vovnet
    from graph_detr4d_amd._lib import Gd4dError
    monkeypatch.delenv('GD4D_TORCH_OPS', raising=False)
    monkeypatch.setitem(vovnet._STAGE_SPECS, 'tiny', TINY_SPEC)
    monkeypatch.setitem(vovnet._STAGE_SPECS, 'odd', ODD_SPEC)
    case = CASES[name]
    device = 'no CPU fallback|GPU'

    # 1. the chosen torch-op route runs and returns
    chosen = case.make(torch_ops=True).eval()
    with torch.no_grad():
        if case.serves_cpu:
            assert case.call(chosen, case.args(chosen)) is not None
        else:
            assert case.rule(chosen, case.args(chosen)) == 'torch'
            with pytest.raises(Gd4dError, match=device):
                case.call(chosen, case.args(chosen))

    # 2. outside the limits the refusal names torch_ops=True, where it is raised today; inside a train() module under autograd it
    #    still comes first
    if case.refused_at_construction:
        with pytest.raises(Gd4dError, match='torch_ops=True'):
            case.make(outside=True)
        outside = case.make(outside=True, torch_ops=True)
        outside.torch_ops = False                    # (built on the torch-op route; it cannot be switched onto the kernels)
    else:
        outside = case.make(outside=True)
    with pytest.raises(Gd4dError, match='torch_ops=True') as e:
        case.rule(outside.train(), case.args(outside))
    assert 'outside the limits' in str(e.value)

    mod = case.make()
    args = case.args(mod)
    assert all(p.requires_grad for p in mod.parameters())
    # 3. train() mode, under no_grad (so autograd has no objection): refused for the mode
    with torch.no_grad(), pytest.raises(Gd4dError, match='train.*torch_ops=True' + ('.*hip_train=True' if case.hip_train else '')):
        case.rule(mod.train(), args)
    # 4. eval() mode, grad mode on, parameters that require grad: refused for autograd
    with pytest.raises(Gd4dError, match='autograd.*torch_ops=True' + ('.*hip_train=True' if case.hip_train else '')):
        case.rule(mod.eval(), args)
    # 5. eval() under no_grad: nothing left to object to but the device, which is checked last
    with torch.no_grad(), pytest.raises(Gd4dError, match=device):
        case.rule(mod.eval(), args)
    if case.hip_train:                               # ... also with the training route switched on
        mod.hip_train = True
        with pytest.raises(Gd4dError, match=device):
            case.rule(mod.train(), args)
    if not case.serves_cpu:                          # the public call: the device refusal in every one of these states
        for m in (outside, mod.train(), mod.eval()):
            with pytest.raises(Gd4dError, match=device):
                case.call(m, case.args(m))
