"""VoVNet-eSE in fp64 plain torch, restated from the formulas and built from a state dict with the reference's key names; what the VoVNet
tests compare against.  With every tensor in fp64 and BatchNorm on its running statistics:
    cbr(x; name, s)  = relu((conv(x, W[name/conv]; stride s, pad k // 2) - mean) / sqrt(var + eps) * gamma + beta)
    OSA(x; m)        : x_0 = x, x_i = cbr(x_{i-1}; layers.(i-1).m_(i-1)), xt = cbr(cat(x_0 .. x_L); concat.m_concat)
                       g = clamp(fc_w mean_hw(xt) + fc_b + 3, 0, 6) / 6,  out = xt g (+ x when the module is not its stage's first)
    network          : stem_1 (s = 2), stem_2, stem_3 (s = 2); stage 2; for stages 3-5 max_pool(3, 2, ceil_mode) first.
The structure (layers per module, modules per stage) is read off the state dict's keys."""
import re

import torch
import torch.nn.functional as F

F64 = torch.float64
EPS = 1e-5


def rel_err(got, ref):
    """max |got - ref| over the map's largest |entry|."""
    ref = ref.detach().to(F64)
    return float((got.detach().cpu().to(F64) - ref).abs().max() / ref.abs().max().clamp(min=1e-30))


def bn_relu(y, gamma, beta, mean, var, eps=EPS):
    v = lambda t: t.to(F64).view(1, -1, 1, 1)
    return torch.relu((y - v(mean)) / torch.sqrt(v(var) + eps) * v(gamma) + v(beta))


def conv_bn_relu(x, weight, gamma, beta, mean, var, stride=1, eps=EPS):
    w = weight.to(F64)
    return bn_relu(F.conv2d(x.to(F64), w, None, stride, w.shape[-1] // 2), gamma, beta, mean, var, eps)


def folded_conv_relu(x, weight, scale, shift, stride=1):
    """relu(conv(x) * scale + shift): the kernels' epilogue, in fp64."""
    w = weight.to(F64)
    y = F.conv2d(x.to(F64), w, None, stride, w.shape[-1] // 2)
    return torch.relu(y * scale.to(F64).view(1, -1, 1, 1) + shift.to(F64).view(1, -1, 1, 1))


def ese_gate(mean, fc_w, fc_b):
    """mean (N, C) -> (N, C)."""
    c = fc_b.numel()
    v = mean.to(F64) @ fc_w.to(F64).reshape(c, c).t() + fc_b.to(F64)
    return (v + 3.0).clamp(0.0, 6.0) / 6.0


def _cbr(sd, x, name, stride=1):
    return conv_bn_relu(x, sd[f'{name}/conv.weight'], sd[f'{name}/norm.weight'], sd[f'{name}/norm.bias'], sd[f'{name}/norm.running_mean'],
                        sd[f'{name}/norm.running_var'], stride)


def osa_module(sd, prefix, name, x, identity, return_gate=False):
    """prefix 'stage3.OSA3_2.', name 'OSA3_2'.  return_gate: (out, the eSE gate (N, C))."""
    layers = sorted({int(m.group(1)) for k in sd for m in [re.match(re.escape(prefix) + r'layers\.(\d+)\.', k)] if m})
    x = x.to(F64)
    maps = [x]
    for i in layers:
        maps.append(_cbr(sd, maps[-1], f'{prefix}layers.{i}.{name}_{i}'))
    xt = _cbr(sd, torch.cat(maps, dim=1), f'{prefix}concat.{name}_concat')
    gate = ese_gate(xt.mean(dim=(2, 3)), sd[f'{prefix}ese.fc.weight'], sd[f'{prefix}ese.fc.bias'])
    out = xt * gate[:, :, None, None]
    out = out + x if identity else out
    return (out, gate) if return_gate else out


def vovnet(sd, x):
    """{'stem', 'stage2' .. 'stage5'} -> fp64 maps."""
    x = _cbr(sd, x.to(F64), 'stem.stem_1', 2)
    x = _cbr(sd, x, 'stem.stem_2', 1)
    x = _cbr(sd, x, 'stem.stem_3', 2)
    outs = {'stem': x}
    for s in (2, 3, 4, 5):
        if s != 2:
            x = F.max_pool2d(x, kernel_size=3, stride=2, ceil_mode=True)
        blocks = sorted({int(m.group(1)) for k in sd for m in [re.match(rf'stage{s}\.OSA{s}_(\d+)\.', k)] if m})
        for b in blocks:
            x = osa_module(sd, f'stage{s}.OSA{s}_{b}.', f'OSA{s}_{b}', x, identity=b > 1)
        outs[f'stage{s}'] = x
    return outs


def modules_up_to(sd, stage):
    """The number of OSA modules in stages 2 .. stage."""
    return len({m.group(0) for k in sd for m in [re.match(r'stage(\d)\.OSA\d_\d+\.', k)] if m and int(m.group(1)) <= stage})


def randomize_(net, seed, bias_saturate=True):
    """He-scaled random convolutions (std sqrt(2 / fan_in)), random BatchNorm statistics and affine terms, eSE fc weights of std
    1 / sqrt(C) with every 7th bias at +8 / -8 (gates of exactly 1 / 0)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if p.dim() == 4 and 'ese.fc' not in name:
                p.copy_(torch.randn(p.shape, generator=g) * (2.0 / (p.shape[1] * p.shape[2] * p.shape[3])) ** 0.5)
            elif p.dim() == 4:
                p.copy_(torch.randn(p.shape, generator=g) * p.shape[1] ** -0.5)
            elif name.endswith('norm.weight'):
                p.copy_(1.0 + 0.25 * (torch.rand(p.shape, generator=g) - 0.5))
            else:
                p.copy_(0.5 * torch.randn(p.shape, generator=g))
                if bias_saturate and name.endswith('ese.fc.bias'):
                    p[0::7] = 8.0
                    p[3::7] = -8.0
        for name, b in net.named_buffers():
            if name.endswith('running_mean'):
                b.copy_(0.2 * torch.randn(b.shape, generator=g))
            elif name.endswith('running_var'):
                b.copy_(0.75 + 0.5 * torch.rand(b.shape, generator=g))
    return net
