"""The image backbone the configs build: mmdet's `ResNet` (depth 50 / 101, style='pytorch') whose stages 3 and 4 replace the 3x3
convolution of every bottleneck with DCNv2 -
    img_backbone=dict(type='ResNet', depth=50, num_stages=4, out_indices=(0, 1, 2, 3), frozen_stages=1,
                      norm_cfg=dict(type='BN', requires_grad=False), norm_eval=True, style='pytorch',
                      dcn=dict(type='DCNv2', deform_groups=1, fallback_on_stride=False), stage_with_dcn=(False, False, True, True))
- with mmdet's state-dict keys (`conv1.weight`, `bn1.*`, `layer3.0.conv2.conv_offset.weight`, `layer1.0.downsample.0.weight`, ...), so a
trained checkpoint's backbone slice loads with strict=True.

Every layer is stock torch except the DCN conv2 (dcn.ModulatedDeformConv2dPack, the library's kernels).  With its BatchNorm in eval
mode - every config: norm_eval=True - a DCN bottleneck computes relu(bn2(conv2(x))) in ONE call, `conv2.forward_bn_relu(x, bn2)`: the
BatchNorm and the ReLU run in the deformable convolution's epilogue.  `torch_ops=True` is handed to the DCN layers (their
differentiable grid_sample route), and so is `hip_train=True`: the same one call then trains on the library's own backward kernels
(dcn.py), with no grid_sample and no tensor of 9 Cin x pixels.

Scope: depth 50 / 101, style 'pytorch', the plain 7x7 stem, BatchNorm, `fallback_on_stride=False`; `num_stages`, `out_indices`,
`strides`, `dilations`, `frozen_stages`, `norm_eval`, `dcn`, `stage_with_dcn`, `zero_init_residual`.  deep_stem, avg_down, plugins, other
norms and `with_cp` are refused: nothing shipped uses them.

The VoVNet configurations' backbone, `VoVNet` / `VoVNetCP`, is in vovnet.py and re-exported here.
"""
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
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


class Bottleneck(nn.Module):
    """mmdet.models.backbones.resnet.Bottleneck, style 'pytorch' (the stride sits on the 3x3 convolution)."""
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, dilation=1, downsample=None, norm_cfg=None, dcn=None, torch_ops=False,
                 hip_train=False):
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

    def forward(self, x):
        out = self.relu(self.bn1(self.conv1(x)))
        if self.with_dcn and not self.bn2.training:
            out = self.conv2.forward_bn_relu(out, self.bn2)       # BatchNorm and ReLU in the deformable convolution's epilogue
        else:
            out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        identity = x if self.downsample is None else self.downsample(x)
        return F.relu(out + identity)


@BACKBONES.register_module()
class ResNet(nn.Module):
    """mmdet.models.backbones.ResNet for depth 50 / 101."""
    arch_settings = {50: (3, 4, 6, 3), 101: (3, 4, 23, 3)}

    def __init__(self, depth, in_channels=3, stem_channels=None, base_channels=64, num_stages=4, strides=(1, 2, 2, 2),
                 dilations=(1, 1, 1, 1), out_indices=(0, 1, 2, 3), style='pytorch', deep_stem=False, avg_down=False, frozen_stages=-1,
                 conv_cfg=None, norm_cfg=dict(type='BN', requires_grad=True), norm_eval=True, dcn=None,
                 stage_with_dcn=(False, False, False, False), plugins=None, with_cp=False, zero_init_residual=True, pretrained=None,
                 init_cfg=None, torch_ops=False, hip_train=False):
        super().__init__()
        if depth not in self.arch_settings:
            raise _lib.Gd4dError(f'ResNet: depth={depth}; this backbone builds the bottleneck depths {sorted(self.arch_settings)}')
        refused = [k for k, v in (('deep_stem', deep_stem), ('avg_down', avg_down), ('conv_cfg', conv_cfg), ('plugins', plugins),
                                  ('with_cp', with_cp)) if v]
        if style != 'pytorch':
            refused.append(f'style={style!r}')
        if refused:
            raise _lib.Gd4dError(f'ResNet: {", ".join(refused)} - not built here (see the module docstring for the scope)')
        assert 1 <= num_stages <= 4 and len(strides) == len(dilations) == num_stages and max(out_indices) < num_stages
        if dcn is not None:
            assert len(stage_with_dcn) == num_stages
        self.depth, self.num_stages, self.out_indices = depth, num_stages, tuple(out_indices)
        self.frozen_stages, self.norm_eval, self.zero_init_residual = frozen_stages, norm_eval, zero_init_residual
        stem_channels = stem_channels or base_channels
        self.conv1 = nn.Conv2d(in_channels, stem_channels, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = _norm(norm_cfg, stem_channels)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.res_layers = []
        inplanes = stem_channels
        for i, blocks in enumerate(self.arch_settings[depth][:num_stages]):
            planes = base_channels * 2 ** i
            stage_dcn = dcn if dcn is not None and stage_with_dcn[i] else None
            layer = self._make_stage(inplanes, planes, blocks, strides[i], dilations[i], norm_cfg, stage_dcn, torch_ops, hip_train)
            inplanes = planes * Bottleneck.expansion
            name = f'layer{i + 1}'
            self.add_module(name, layer)
            self.res_layers.append(name)
        self.feat_dim = inplanes
        self.init_weights()
        self._freeze_stages()

    @staticmethod
    def _make_stage(inplanes, planes, blocks, stride, dilation, norm_cfg, dcn, torch_ops, hip_train=False):
        downsample = None
        if stride != 1 or inplanes != planes * Bottleneck.expansion:
            downsample = nn.Sequential(nn.Conv2d(inplanes, planes * Bottleneck.expansion, kernel_size=1, stride=stride, bias=False),
                                       _norm(norm_cfg, planes * Bottleneck.expansion))
        layers = [Bottleneck(inplanes, planes, stride, dilation, downsample, norm_cfg, dcn, torch_ops, hip_train)]
        inplanes = planes * Bottleneck.expansion
        for _ in range(1, blocks):
            layers.append(Bottleneck(inplanes, planes, 1, dilation, None, norm_cfg, dcn, torch_ops, hip_train))
        return nn.Sequential(*layers)

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
