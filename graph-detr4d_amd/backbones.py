"""The image backbone the configs build: mmdet's `ResNet` (depth 18 / 34 of BasicBlocks, 50 / 101 of Bottlenecks, style='pytorch'),
in the DCN configurations with stages 3 and 4 replacing the 3x3 convolution of every bottleneck with DCNv2 -
    img_backbone=dict(type='ResNet', depth=50, num_stages=4, out_indices=(0, 1, 2, 3), frozen_stages=1,
                      norm_cfg=dict(type='BN', requires_grad=False), norm_eval=True, style='pytorch',
                      dcn=dict(type='DCNv2', deform_groups=1, fallback_on_stride=False), stage_with_dcn=(False, False, True, True))
- with mmdet's state-dict keys (`conv1.weight`, `bn1.*`, `layer3.0.conv2.conv_offset.weight`, `layer1.0.downsample.0.weight`, ...), so a
trained checkpoint's backbone slice loads with strict=True.

By default every layer is stock torch except the DCN conv2 (dcn.ModulatedDeformConv2dPack, the library's kernels).  With its BatchNorm in eval
mode - every config: norm_eval=True - a DCN bottleneck computes relu(bn2(conv2(x))) in ONE call, `conv2.forward_bn_relu(x, bn2)`: the
BatchNorm and the ReLU run in the deformable convolution's epilogue.  `torch_ops=True` is handed to the DCN layers (their
differentiable grid_sample route), and so is `hip_train=True`: the same one call then trains on the library's own backward kernels
(dcn.py), with no grid_sample and no tensor of 9 Cin x pixels.

`plain_kernels=True` (opt-in; `ResNet`, `Bottleneck`, `BasicBlock`) runs the blocks' plain convolutions on the library's kernels too
(gd4d_resnet.hip), each with its frozen BatchNorm folded into the epilogue.  A block is then a kernel_route.KernelRoute module, and its
route 'infer' is
    Bottleneck   conv1 -> relu(bn1);  conv2 -> relu(bn2) (the plain 3x3 with the block's stride, or the DCN's forward_bn_relu as before);
                 downsample -> bn, no ReLU (a stage's first block);  conv3 -> relu(bn3 + identity): 3 launches, 4 with a downsample
    BasicBlock   conv1 (3x3, the stride) -> relu(bn1);  downsample -> bn;  conv2 (3x3) -> relu(bn2 + identity): 2 launches, 3 with one
with no separate BatchNorm, ReLU or add pass.  Weight images and the folded (scale, shift) are kept at fixed addresses (`_keep`), so a
forward is capturable in a hipGraph after one eager call and `refresh_images()` serves in-place parameter edits, as for VoVNet.  The
kernels take channels that are multiples of 32 (1x1: K up to 2304, Cout up to 2048; 3x3: Cin up to 1024, Cout up to 512), stride 1 or
2, dilation 1 and frozen BatchNorms; anything else is refused at construction or at the call, naming `torch_ops=True`.  They have no
backward: `plain_kernels=True` with `hip_train=True` is refused, and autograd on trainable parameters raises.  `torch_ops=True`,
`with Fn.torch_ops_for(net):` or GD4D_TORCH_OPS=1 choose the block's own torch layers.  The 7x7 stem (3 input channels) and the
max-pooling stay on torch on every route.

Scope: depth 18 / 34 / 50 / 101, style 'pytorch', the plain 7x7 stem, BatchNorm, `fallback_on_stride=False`; `num_stages`, `out_indices`,
`strides`, `dilations`, `frozen_stages`, `norm_eval`, `dcn`, `stage_with_dcn`, `zero_init_residual`.  deep_stem, avg_down, plugins, other
norms and `with_cp` are refused: nothing shipped uses them.

The VoVNet configurations' backbone, `VoVNet` / `VoVNetCP`, is in vovnet.py and re-exported here.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, ops
from . import functional as Fn
from .kernel_route import KernelRoute, f32, refuse_outside_limits
from .registry import BACKBONES, build_conv_layer
from .vovnet import VoVNet, VoVNetCP  # noqa: F401  (the VoVNet configurations' backbone: vovnet.py)


def _norm(norm_cfg, channels):
    cfg = dict(norm_cfg or dict(type='BN'))
    if cfg.pop('type', 'BN') not in ('BN', 'BN2d'):
        raise _lib.Gd4dError(f'ResNet: norm_cfg={norm_cfg}; this backbone builds BatchNorm2d layers (what every shipped config uses)')
    requires_grad = cfg.pop('requires_grad', True)
    bn = nn.BatchNorm2d(channels, **cfg)
    for p in bn.parameters():
        p.requires_grad = requires_grad
    return bn


class _PlainKernels(KernelRoute):
    """What `plain_kernels=True` adds to a block: the route rule (kernel_route.py) in front of its forward, its convolutions' weight
    images and folded BatchNorms as kept values.  A block supplies `_plain_layers()`, `_torch(x)` and `_hip(x)`.  With
    `plain_kernels=False` none of this is consulted: forward is `_torch`, stock layers (and the DCN conv2's own route)."""
    _kernels = ('ResNet kernels fold the BatchNorms\' running statistics into the convolutions (so every BatchNorm of the block must be '
                'frozen: eval() mode with running statistics, what norm_eval=True keeps in every config) and have no backward')
    plain_kernels = False

    def _init_plain(self, plain_kernels, torch_ops, hip_train):
        self.plain_kernels = bool(plain_kernels)
        if not self.plain_kernels:
            return
        if hip_train:
            raise _lib.Gd4dError(f'{type(self).__name__}: plain_kernels=True with hip_train=True - the plain convolutions\' kernels have no '
                                 'backward (hip_train trains the DCN layers behind stock torch layers).  Choose one of the two, or '
                                 '`torch_ops=True` for training by autograd.')
        self._norms = tuple(m for m in self.modules() if isinstance(m, nn.BatchNorm2d))
        self._init_route(torch_ops, self._plain_limits())

    # `blk.torch_ops = True` / `with Fn.torch_ops_for(blk):` reach the DCN conv2 too, which decides its own route
    @property
    def torch_ops(self):
        return self.__dict__.get('_torch_ops', False)

    @torch_ops.setter
    def torch_ops(self, value):
        self.__dict__['_torch_ops'] = bool(value)
        conv2 = self.__dict__.get('_modules', {}).get('conv2')
        if self.plain_kernels and isinstance(conv2, KernelRoute):
            conv2.torch_ops = bool(value)

    def _plain_layers(self):
        """[(key, conv, bn)] of the plain convolutions the kernels run, in launch order."""
        raise NotImplementedError

    def _plain_limits(self):
        why = []
        for key, conv, _ in self._plain_layers():
            k3 = conv.kernel_size == (3, 3)
            lim_in, lim_out = (1024, 512) if k3 else (2304, 2048)
            for what, c, lim in (('input', conv.in_channels, lim_in), ('output', conv.out_channels, lim_out)):
                if c % 32 or not 32 <= c <= lim:
                    why.append(f'{key}: {c} {what} channels (kernels: multiples of 32 in [32, {lim}])')
            if conv.stride not in ((1, 1), (2, 2)):
                why.append(f'{key}: stride={conv.stride} (kernels: 1 or 2)')
            if k3 and (conv.dilation != (1, 1) or conv.padding != (1, 1)):
                why.append(f'{key}: dilation={conv.dilation}, padding={conv.padding} (kernels: 1)')
        conv2 = getattr(self, 'conv2', None)
        if isinstance(conv2, KernelRoute):
            why += [f'conv2 (DCN): {w}' for w in conv2._kernel_limits]
        return why

    def _route_name(self):
        return f'{type(self).__name__}({self.inplanes}, {self.planes})'

    def _in_train_mode(self):
        return any(m.training or m.running_mean is None for m in self._norms)

    def _image(self, key, conv):
        build = ops.conv3x3_act_image if conv.kernel_size == (3, 3) else ops.conv1x1_image
        return self._keep(('image', key), (conv.weight,), lambda: build(conv.weight.detach().float()))

    def _folded(self, key, bn):
        """(2, C): scale = gamma / sqrt(var + eps) and shift = beta - mean scale of an eval()-mode BatchNorm2d."""
        sources = (bn.running_var, bn.running_mean, bn.weight, bn.bias)
        return self._keep(('bn', key, float(bn.eps)), sources, lambda: Fn.folded_batchnorm(bn))

    def _conv(self, key, x, conv, bn, identity=None, relu=True):
        """act(bn(conv(x)) (+ identity)) in one launch."""
        scale, shift = self._folded(key, bn)
        run = ops.conv3x3_bn_act if conv.kernel_size == (3, 3) else ops.conv1x1_bn_act
        return run(x, self._image(key, conv), conv.out_channels, scale, shift, stride=conv.stride[0], identity=identity, relu=relu)

    def _kept_values(self):
        for key, conv, bn in self._plain_layers():
            self._image(key, conv)
            self._folded(key, bn)
        conv2 = getattr(self, 'conv2', None)
        if isinstance(conv2, KernelRoute):
            conv2._bns[id(self.bn2)] = self.bn2
            conv2._kept_values()

    def forward(self, x):
        if not self.plain_kernels or self._route(x) == 'torch':
            return self._torch(x)
        with torch.no_grad():
            return self._hip(f32(x))


class Bottleneck(_PlainKernels, nn.Module):
    """mmdet.models.backbones.resnet.Bottleneck, style 'pytorch' (the stride sits on the 3x3 convolution)."""
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, dilation=1, downsample=None, norm_cfg=None, dcn=None, torch_ops=False,
                 hip_train=False, plain_kernels=False):
        super().__init__()
        self.inplanes, self.planes, self.stride, self.dilation = inplanes, planes, stride, dilation
        self.with_dcn = dcn is not None
        self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=1, stride=1, bias=False)
        self.bn1 = _norm(norm_cfg, planes)
        if self.with_dcn:
            dcn = dict(dcn)
            if dcn.pop('fallback_on_stride', False):
                raise _lib.Gd4dError('Bottleneck: dcn fallback_on_stride=True is not built (every shipped config sets False)')
            self.conv2 = build_conv_layer(dcn, planes, planes, kernel_size=3, stride=stride, padding=dilation, dilation=dilation,
                                          bias=False, torch_ops=torch_ops, hip_train=hip_train)
        else:
            self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, stride=stride, padding=dilation, dilation=dilation, bias=False)
        self.bn2 = _norm(norm_cfg, planes)
        self.conv3 = nn.Conv2d(planes, planes * self.expansion, kernel_size=1, bias=False)
        self.bn3 = _norm(norm_cfg, planes * self.expansion)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self._init_plain(plain_kernels, torch_ops, hip_train)

    def _plain_layers(self):
        layers = [('conv1', self.conv1, self.bn1)] + ([] if self.with_dcn else [('conv2', self.conv2, self.bn2)])
        if self.downsample is not None:
            layers.append(('downsample', self.downsample[0], self.downsample[1]))
        return layers + [('conv3', self.conv3, self.bn3)]

    def _hip(self, x):
        out = self._conv('conv1', x, self.conv1, self.bn1)
        out = self.conv2.forward_bn_relu(out, self.bn2) if self.with_dcn else self._conv('conv2', out, self.conv2, self.bn2)
        identity = x if self.downsample is None else self._conv('downsample', x, *self.downsample, relu=False)
        return self._conv('conv3', out, self.conv3, self.bn3, identity=identity)

    def _torch(self, x):
        out = self.relu(self.bn1(self.conv1(x)))
        if self.with_dcn and not self.bn2.training:
            out = self.conv2.forward_bn_relu(out, self.bn2)       # BatchNorm and ReLU in the deformable convolution's epilogue
        else:
            out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        identity = x if self.downsample is None else self.downsample(x)
        return F.relu(out + identity)


class BasicBlock(_PlainKernels, nn.Module):
    """mmdet.models.backbones.resnet.BasicBlock: conv1 3x3 with the stride, bn1, ReLU, conv2 3x3, bn2, the residual, ReLU."""
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, dilation=1, downsample=None, norm_cfg=None, dcn=None, torch_ops=False,
                 hip_train=False, plain_kernels=False):
        super().__init__()
        if dcn is not None:
            raise _lib.Gd4dError('BasicBlock: dcn is not built for the basic block (mmdet asserts the same; depths 50 / 101 take it) - on '
                                 'no route: `torch_ops=True` does not serve it either')
        self.inplanes, self.planes, self.stride, self.dilation = inplanes, planes, stride, dilation
        self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=3, stride=stride, padding=dilation, dilation=dilation, bias=False)
        self.bn1 = _norm(norm_cfg, planes)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, padding=1, bias=False)
        self.bn2 = _norm(norm_cfg, planes)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self._init_plain(plain_kernels, torch_ops, hip_train)

    def _plain_layers(self):
        down = [] if self.downsample is None else [('downsample', self.downsample[0], self.downsample[1])]
        return [('conv1', self.conv1, self.bn1)] + down + [('conv2', self.conv2, self.bn2)]

    def _hip(self, x):
        out = self._conv('conv1', x, self.conv1, self.bn1)
        identity = x if self.downsample is None else self._conv('downsample', x, *self.downsample, relu=False)
        return self._conv('conv2', out, self.conv2, self.bn2, identity=identity)

    def _torch(self, x):
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        identity = x if self.downsample is None else self.downsample(x)
        return F.relu(out + identity)


@BACKBONES.register_module()
class ResNet(nn.Module):
    """mmdet.models.backbones.ResNet for depth 18 / 34 (BasicBlock) and 50 / 101 (Bottleneck).  `net.torch_ops` (or `with
    Fn.torch_ops_for(net):`) is the route switch of every `plain_kernels=True` block, which decide their route themselves."""
    arch_settings = {18: (BasicBlock, (2, 2, 2, 2)), 34: (BasicBlock, (3, 4, 6, 3)), 50: (Bottleneck, (3, 4, 6, 3)),
                     101: (Bottleneck, (3, 4, 23, 3))}

    def __init__(self, depth, in_channels=3, stem_channels=None, base_channels=64, num_stages=4, strides=(1, 2, 2, 2),
                 dilations=(1, 1, 1, 1), out_indices=(0, 1, 2, 3), style='pytorch', deep_stem=False, avg_down=False, frozen_stages=-1,
                 conv_cfg=None, norm_cfg=dict(type='BN', requires_grad=True), norm_eval=True, dcn=None,
                 stage_with_dcn=(False, False, False, False), plugins=None, with_cp=False, zero_init_residual=True, pretrained=None,
                 init_cfg=None, torch_ops=False, hip_train=False, plain_kernels=False):
        super().__init__()
        if depth not in self.arch_settings:
            raise _lib.Gd4dError(f'ResNet: depth={depth}; this backbone builds the depths {sorted(self.arch_settings)}')
        refused = [k for k, v in (('deep_stem', deep_stem), ('avg_down', avg_down), ('conv_cfg', conv_cfg), ('plugins', plugins),
                                  ('with_cp', with_cp)) if v]
        if style != 'pytorch':
            refused.append(f'style={style!r}')
        if refused:
            raise _lib.Gd4dError(f'ResNet: {", ".join(refused)} - not built here (see the module docstring for the scope)')
        assert 1 <= num_stages <= 4 and len(strides) == len(dilations) == num_stages and max(out_indices) < num_stages
        block, stage_blocks = self.arch_settings[depth]
        if dcn is not None:
            assert len(stage_with_dcn) == num_stages
            if block is BasicBlock and any(stage_with_dcn):
                raise _lib.Gd4dError(f'ResNet: dcn with depth={depth} - not built for the basic block (mmdet asserts the same; depths 50 / '
                                     '101 take it), on no route: `torch_ops=True` does not serve it either')
        if plain_kernels and hip_train:
            raise _lib.Gd4dError('ResNet: plain_kernels=True with hip_train=True - the plain convolutions\' kernels have no backward '
                                 '(hip_train trains the DCN layers behind stock torch layers).  Choose one of the two, or `torch_ops=True` '
                                 'for training by autograd.')
        self.block, self.plain_kernels = block, bool(plain_kernels)
        self.depth, self.num_stages, self.out_indices = depth, num_stages, tuple(out_indices)
        self.frozen_stages, self.norm_eval, self.zero_init_residual = frozen_stages, norm_eval, zero_init_residual
        stem_channels = stem_channels or base_channels
        self.conv1 = nn.Conv2d(in_channels, stem_channels, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = _norm(norm_cfg, stem_channels)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.res_layers = []
        inplanes = stem_channels
        for i, blocks in enumerate(stage_blocks[:num_stages]):
            planes = base_channels * 2 ** i
            stage_dcn = dcn if dcn is not None and stage_with_dcn[i] else None
            layer = self._make_stage(inplanes, planes, blocks, strides[i], dilations[i], norm_cfg, stage_dcn, torch_ops, hip_train,
                                     block, self.plain_kernels)
            inplanes = planes * block.expansion
            name = f'layer{i + 1}'
            self.add_module(name, layer)
            self.res_layers.append(name)
        self.feat_dim = inplanes
        self.init_weights()
        self._freeze_stages()
        self.torch_ops = torch_ops
        # refused here, not at the first forward
        refuse_outside_limits(self, f'ResNet({depth}, plain_kernels=True)', [f'{name}: {w}' for name, m in self._routed() for w in m._kernel_limits])

    @staticmethod
    def _make_stage(inplanes, planes, blocks, stride, dilation, norm_cfg, dcn, torch_ops, hip_train=False, block=Bottleneck,
                    plain_kernels=False):
        downsample = None
        if stride != 1 or inplanes != planes * block.expansion:
            downsample = nn.Sequential(nn.Conv2d(inplanes, planes * block.expansion, kernel_size=1, stride=stride, bias=False),
                                       _norm(norm_cfg, planes * block.expansion))
        layers = [block(inplanes, planes, stride, dilation, downsample, norm_cfg, dcn, torch_ops, hip_train, plain_kernels)]
        inplanes = planes * block.expansion
        for _ in range(1, blocks):
            layers.append(block(inplanes, planes, 1, dilation, None, norm_cfg, dcn, torch_ops, hip_train, plain_kernels))
        return nn.Sequential(*layers)

    def _routed(self):
        """(name, block) of the blocks on the route rule: every block with plain_kernels=True, none without."""
        return [(name, m) for name, m in self.named_modules() if isinstance(m, _PlainKernels) and m.plain_kernels]

    @property
    def torch_ops(self):
        return self._torch_ops

    @torch_ops.setter
    def torch_ops(self, value):
        self._torch_ops = bool(value)
        for _, m in self._routed():
            m.torch_ops = self._torch_ops

    def refresh_images(self):
        """Rebuild every changed weight image and folded BatchNorm into the buffers a captured graph reads (kernel_route.py)."""
        for _, m in self._routed():
            m.refresh_images()

    def init_weights(self):
        """mmdet's default: Kaiming-normal convolutions, unit BatchNorms, zero conv_offset, zero-initialised last BatchNorm of a block."""
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)
        for m in self.modules():
            if isinstance(m, Bottleneck):
                if m.with_dcn and hasattr(m.conv2, 'conv_offset'):
                    nn.init.zeros_(m.conv2.conv_offset.weight)
                    nn.init.zeros_(m.conv2.conv_offset.bias)
                if self.zero_init_residual:
                    nn.init.zeros_(m.bn3.weight)
            elif isinstance(m, BasicBlock) and self.zero_init_residual:
                nn.init.zeros_(m.bn2.weight)

    def _freeze_stages(self):
        if self.frozen_stages >= 0:
            for m in (self.conv1, self.bn1):
                m.eval()
                for p in m.parameters():
                    p.requires_grad = False
        for i in range(1, self.frozen_stages + 1):
            m = getattr(self, f'layer{i}')
            m.eval()
            for p in m.parameters():
                p.requires_grad = False

    def forward(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        outs = []
        for i, name in enumerate(self.res_layers):
            x = getattr(self, name)(x)
            if i in self.out_indices:
                outs.append(x)
        return tuple(outs)

    def train(self, mode=True):
        super().train(mode)
        self._freeze_stages()
        if mode and self.norm_eval:
            for m in self.modules():
                if isinstance(m, nn.BatchNorm2d):
                    m.eval()
        return self
