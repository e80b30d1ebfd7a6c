"""The backward of mmdet's ResNet blocks behind frozen BatchNorms as an fp64 closed form in plain torch - what gd4d_resnet_train.hip and
backbones.py's plain_train nodes implement - and its chaining over a network.  It extends vovnet_train_ref.py's pattern to strides 1
and 2, and like it is LINEARISED AT THE FORWARD MAPS IT IS GIVEN: every ReLU mask is [map > 0] of a given map.  The GPU tests pass the
device's own maps, so every such decision is the device's and no entry has to be excluded; the CPU test passes the fp64 forward's and
compares with fp64 autograd.

A unit is conv (stride st, pad k // 2) -> BatchNorm on its running statistics (s = gamma rstd).  With dz the gradient of the BatchNorm's
output after the ReLU's mask:
    G = sum dz (x) x_in  (the plain weight gradient of the strided convolution for the unscaled dz);  dW = s (x) G;  dbeta = sum dz;
    dgamma = rstd (<W, G> - mean dbeta)        (the pre-BatchNorm map is W * x_in: none is needed);      dx_in = conv^T(s dz)
A Bottleneck, given dout and the maps (x, a1, a2, out):
    g3 = dout [out > 0];  g2 = conv3^T(s3 g3) [a2 > 0];  g1 = conv2^T(s2 g2) [a1 > 0];  dx = conv1^T(s1 g1) + r
    r = g3 without a downsample, else downsample^T(s_d g3) (a stride-2 one touches the even pixels only)
A BasicBlock the same with two units.  A DCN bottleneck is the head (conv1: g1 = da1 [a1 > 0]) and the tail (conv3, downsample, the
residual: returns conv3^T(s3 g3) UNMASKED for a2 and r for the block input) around the DCN layer."""
import re

import torch
import torch.nn.functional as F

from vovnet_train_ref import _d, rel_err  # noqa: F401

F64 = torch.float64
EPS = 1e-5
STRIDES = (1, 2, 2, 2)


def _bn(sd, name):
    return tuple(_d(sd[f'{name}.{k}']) for k in ('weight', 'bias', 'running_mean', 'running_var'))


def unit_param_grads(dz, x_in, weight, bn, stride=1, eps=EPS):
    """(dW, dgamma, dbeta) from fp64 dz (N, Cout, Ho, Wo) and x_in (N, Cin, H, W); bn = (gamma, beta, mean, var)."""
    gamma, _, mean, var = (_d(t) for t in bn)
    w = _d(weight)
    rstd = 1.0 / torch.sqrt(var + eps)
    g = torch.nn.grad.conv2d_weight(x_in, w.shape, dz, stride=stride, padding=w.shape[-1] // 2)
    dbeta = dz.sum(dim=(0, 2, 3))
    dgamma = rstd * ((w * g).sum(dim=(1, 2, 3)) - mean * dbeta)
    return (gamma * rstd).view(-1, 1, 1, 1) * g, dgamma, dbeta


def unit_data_grad(dz, weight, bn, hw, stride=1, eps=EPS):
    """conv^T(s dz) at the input's size hw = (H, W): the input gradient of BN(conv(x; stride)) for the BatchNorm output's gradient dz."""
    gamma, _, _, var = (_d(t) for t in bn)
    w = _d(weight)
    k, pad = w.shape[-1], w.shape[-1] // 2
    s = gamma / torch.sqrt(var + eps)
    extra = tuple(int(full) - ((int(o) - 1) * stride - 2 * pad + k) for full, o in zip(hw, dz.shape[2:]))
    return F.conv_transpose2d(dz * s.view(1, -1, 1, 1), w, stride=stride, padding=pad, output_padding=extra)


def even_pixels_add(full, half):
    """full with half added at the pixels whose row and column are both even (what add_even does)."""
    out = full.clone()
    out[:, :, ::2, ::2] += half
    return out


def _unit(sd, prefix, conv, bn, dz, x_in, stride, grads, hw=None):
    """Records the unit's parameter gradients under its state-dict keys; returns its data gradient when hw is given."""
    bnp = _bn(sd, f'{prefix}{bn}')
    w = sd[f'{prefix}{conv}.weight']
    grads[f'{prefix}{conv}.weight'], grads[f'{prefix}{bn}.weight'], grads[f'{prefix}{bn}.bias'] = unit_param_grads(dz, x_in, w, bnp, stride)
    return None if hw is None else unit_data_grad(dz, w, bnp, hw, stride)


def _residual(sd, prefix, g3, x, stride, grads):
    if f'{prefix}downsample.0.weight' not in sd:
        return g3
    return _unit(sd, prefix, 'downsample.0', 'downsample.1', g3, x, stride, grads, x.shape[2:])


def block_backward(sd, prefix, maps, dout, stride=1):
    """One plain block: maps (x, a1, a2, out) of a Bottleneck or (x, a1, out) of a BasicBlock, dout -> (dx, {state-dict key: gradient})."""
    *inputs, out = [_d(t) for t in maps]
    dout = _d(dout)
    grads = {}
    x = inputs[0]
    g3 = dout * (out > 0)
    r = _residual(sd, prefix, g3, x, stride, grads)
    n_units = len(inputs)
    strided = 2 if n_units == 3 else 1                      # the unit that carries the block's stride: conv2 of three, conv1 of two
    g = g3
    for i in range(n_units, 0, -1):
        st = stride if i == strided else 1
        g = _unit(sd, prefix, f'conv{i}', f'bn{i}', g, inputs[i - 1], st, grads, inputs[i - 1].shape[2:])
        if i > 1:
            g = g * (inputs[i - 1] > 0)
    return g + r, grads


def head_backward(sd, prefix, x, a1, da1):
    """The DCN bottleneck's head: (dx, grads) from the gradient of a1 (unmasked)."""
    x, a1 = _d(x), _d(a1)
    grads = {}
    dx = _unit(sd, prefix, 'conv1', 'bn1', _d(da1) * (a1 > 0), x, 1, grads, x.shape[2:])
    return dx, grads


def tail_backward(sd, prefix, a2, x, out, dout, stride=1):
    """The DCN bottleneck's tail: (da2 unmasked, the residual path's dx, grads)."""
    a2, x, out = _d(a2), _d(x), _d(out)
    grads = {}
    g3 = _d(dout) * (out > 0)
    r = _residual(sd, prefix, g3, x, stride, grads)
    da2 = _unit(sd, prefix, 'conv3', 'bn3', g3, a2, 1, grads, a2.shape[2:])
    return da2, r, grads


def dcn_unit_backward(conv2, bn2, a1, a2, da2):
    """relu(bn2(conv2(a1))) of a DCN layer through fp64 autograd on an fp64 CPU copy of the layer (its torch-op route), with the ReLU
    replaced by the mask [a2 > 0] of the GIVEN a2.  Returns (da1, {name under the block: gradient})."""
    a1 = _d(a1).requires_grad_(True)
    conv2.zero_grad(set_to_none=True)
    z = conv2._torch(a1, *conv2.offsets_torch(a1))
    gamma, beta, mean, var = (_d(t) for t in (bn2.weight, bn2.bias, bn2.running_mean, bn2.running_var))
    z = (z - mean.view(1, -1, 1, 1)) / torch.sqrt(var.view(1, -1, 1, 1) + bn2.eps) * gamma.view(1, -1, 1, 1) + beta.view(1, -1, 1, 1)
    (z * (_d(a2) > 0)).backward(_d(da2))
    return a1.grad, {f'conv2.{k}': p.grad for k, p in conv2.named_parameters()}


def block_names(sd):
    """[(layer, block index, 'layer2.0.', stride)] in network order."""
    found = sorted({(int(m.group(1)), int(m.group(2))) for k in sd for m in [re.match(r'layer(\d)\.(\d+)\.', k)] if m})
    return [(layer, b, f'layer{layer}.{b}.', STRIDES[layer - 1] if b == 0 else 1) for layer, b in found]


def network_backward(sd, recorded, couts, first_layer=2, dcn_layers=None):
    """The chain over the blocks of layer<first_layer> .. layer4 (the stem, the max-pooling and the layers below are frozen).  recorded:
    {block prefix: maps} of the device's forward - (x, a1, a2, out) / (x, a1, out) of a plain block, the same four of a DCN bottleneck;
    couts: {layer: cotangent of that layer's output}; dcn_layers: {block prefix: (fp64 CPU copy of its conv2, its bn2)}.  Returns
    {state-dict key: gradient}."""
    blocks = block_names(sd)
    grads, g = {}, None
    for idx in range(len(blocks) - 1, -1, -1):
        layer, b, prefix, stride = blocks[idx]
        if layer < first_layer:
            break
        if (idx == len(blocks) - 1 or blocks[idx + 1][0] != layer) and layer in couts:
            g = _d(couts[layer]) if g is None else g + _d(couts[layer])
        if g is None:
            continue
        maps = recorded[prefix]
        if dcn_layers and prefix in dcn_layers:
            x, a1, a2, out = maps
            da2, r, bg = tail_backward(sd, prefix, a2, x, out, g, stride)
            da1, dg = dcn_unit_backward(*dcn_layers[prefix], a1, a2, da2)
            bg.update({f'{prefix}{k}': v for k, v in dg.items()})
            dx, hg = head_backward(sd, prefix, x, a1, da1)
            bg.update(hg)
            g = dx + r
        else:
            g, bg = block_backward(sd, prefix, maps, g, stride)
        grads.update(bg)
    return grads
