"""mmdet's ResNet (style 'pytorch', BatchNorm on its running statistics) in fp64 plain torch, restated from the formulas and built from a
state dict with mmdet's key names; what the ResNet tests compare against.  It shares no code with the package.
    cb(x; conv, bn, s)   = (conv(x, W[conv]; stride s, pad k // 2) - mean) / sqrt(var + eps) * gamma + beta
    Bottleneck(x; s)     : relu(cb(relu(cb(relu(cb(x; conv1, bn1)); conv2, bn2, s)); conv3, bn3) + id),  id = x or cb(x; downsample, s)
    BasicBlock(x; s)     : relu(cb(relu(cb(x; conv1, bn1, s)); conv2, bn2) + id)
    network              : relu(cb(x; conv1 7x7, bn1, 2)), max_pool(3, 2, pad 1), then layer1 .. layer4; a layer's first block has the
                           layer's stride (1, 2, 2, 2) and the downsample.
The structure (blocks per layer) is read off the state dict's keys; the block type comes with the depth."""
import re

import torch
import torch.nn.functional as F

from vovnet_ref import rel_err  # noqa: F401  (the tests' measure: max |diff| over the map's largest |entry|)

F64 = torch.float64
EPS = 1e-5
STRIDES = (1, 2, 2, 2)


def _per_channel(t):
    return t.to(F64).view(1, -1, 1, 1)


def folded_conv_act(x, w, scale, shift, stride=1, identity=None, relu=True):
    """act(conv(x) * scale + shift (+ identity)): the kernels' epilogue, in fp64.  w (Cout, Cin, k, k), pad k // 2."""
    w = w.to(F64)
    y = F.conv2d(x.to(F64), w, None, stride, w.shape[-1] // 2) * _per_channel(scale) + _per_channel(shift)
    if identity is not None:
        y = y + identity.to(F64)
    return torch.relu(y) if relu else y


def _cb(sd, conv, bn, x, stride=1):
    w = sd[f'{conv}.weight'].to(F64)
    y = F.conv2d(x, w, None, stride, w.shape[-1] // 2)
    y = (y - _per_channel(sd[f'{bn}.running_mean'])) / torch.sqrt(_per_channel(sd[f'{bn}.running_var']) + EPS)
    return y * _per_channel(sd[f'{bn}.weight']) + _per_channel(sd[f'{bn}.bias'])


def _identity(sd, prefix, x, stride):
    if f'{prefix}downsample.0.weight' not in sd:
        return x
    return _cb(sd, f'{prefix}downsample.0', f'{prefix}downsample.1', x, stride)


def bottleneck(sd, prefix, x, stride=1):
    """prefix 'layer2.0.' (or '' for a block's own state dict)."""
    x = x.to(F64)
    out = torch.relu(_cb(sd, f'{prefix}conv1', f'{prefix}bn1', x))
    out = torch.relu(_cb(sd, f'{prefix}conv2', f'{prefix}bn2', out, stride))
    return torch.relu(_cb(sd, f'{prefix}conv3', f'{prefix}bn3', out) + _identity(sd, prefix, x, stride))


def basic_block(sd, prefix, x, stride=1):
    x = x.to(F64)
    out = torch.relu(_cb(sd, f'{prefix}conv1', f'{prefix}bn1', x, stride))
    return torch.relu(_cb(sd, f'{prefix}conv2', f'{prefix}bn2', out) + _identity(sd, prefix, x, stride))


def blocks_of(sd, layer):
    return sorted({int(m.group(1)) for k in sd for m in [re.match(rf'layer{layer}\.(\d+)\.', k)] if m})


def blocks_up_to(sd, layer):
    """The number of blocks in layer1 .. layer<layer>."""
    return sum(len(blocks_of(sd, i)) for i in range(1, layer + 1))


def resnet(sd, x, depth):
    """(layer1, .., layer4) outputs in fp64."""
    block = basic_block if depth in (18, 34) else bottleneck
    x = torch.relu(_cb(sd, 'conv1', 'bn1', x.to(F64), 2))
    x = F.max_pool2d(x, kernel_size=3, stride=2, padding=1)
    outs = []
    for layer in (1, 2, 3, 4):
        for b in blocks_of(sd, layer):
            x = block(sd, f'layer{layer}.{b}.', x, STRIDES[layer - 1] if b == 0 else 1)
        outs.append(x)
    return tuple(outs)


def randomize_(net, seed):
    """He-scaled random convolutions (std sqrt(2 / fan_in); a DCN's conv_offset too, with a bias of std 0.5), random running statistics,
    and gamma around 1 and a random beta for EVERY BatchNorm - bn3 included, which zero_init_residual leaves at gamma = 0: a block whose
    conv3 were broken would pass on that."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if p.dim() == 4:
                p.copy_(torch.randn(p.shape, generator=g) * (2.0 / (p.shape[1] * p.shape[2] * p.shape[3])) ** 0.5)
            elif name.endswith('.weight'):
                p.copy_(1.0 + 0.25 * (torch.rand(p.shape, generator=g) - 0.5))
            else:
                p.copy_(0.5 * torch.randn(p.shape, generator=g))
        for name, b in net.named_buffers():
            if name.endswith('running_mean'):
                b.copy_(0.2 * torch.randn(b.shape, generator=g))
            elif name.endswith('running_var'):
                b.copy_(0.75 + 0.5 * torch.rand(b.shape, generator=g))
    return net
