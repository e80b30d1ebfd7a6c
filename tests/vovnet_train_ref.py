"""The backward of one VoVNet OSA module behind frozen BatchNorms as an fp64 closed form in plain torch - what gd4d_vovnet_train.hip and
vovnet.py's hip_train node implement - and its chaining over a whole network.  It is LINEARISED AT THE FORWARD MAPS IT IS GIVEN: the ReLU
masks are [map > 0] of those maps, the gate's branch is read off the given gate and the pool indices off the given stage outputs.  The
GPU tests pass the device's own maps, so every such decision is the device's and no entry has to be excluded (the convention of
test_depth_net_train_gpu.py); the CPU test passes the fp64 forward's and compares with fp64 autograd.

With s = gamma rstd per BatchNorm and the forward of vovnet_ref.py, given dout:
    dgate = sum_hw dout xt;  dv = dgate / 6 where 0 < gate < 1, else 0 (the clamp's corners included);  m = mean_hw xt
    dfc_b = sum_n dv;  dfc_w = sum_n dv (x) m;  dm = fc_w^T dv;  dz_c = (dout gate + dm / HW) [xt > 0]
    g_0 .. g_L = the slices of W_c^T (s_c dz_c);  for i = L .. 1:  dz_i = g_i [x_i > 0],  g_{i-1} += conv3x3_i^T(s_i dz_i);  dx = g_0 (+ dout)
    per convolution:  G = sum dz (x) x_in (the plain weight gradient for the unscaled dz);  dW = s (x) G;  dbeta = sum dz;
                      dgamma = rstd (<W, G> - mean dbeta)      (the pre-BatchNorm map is W * x_in: none is needed)"""
import re

import torch
import torch.nn.functional as F

F64 = torch.float64
EPS = 1e-5


def _d(t):
    return t.detach().cpu().to(F64)


def conv_param_grads(dz, x_in, weight, gamma, beta, mean, var, eps=EPS):
    """(dW, dgamma, dbeta) of relu(BN(conv(x_in))) from dz, the gradient of the BatchNorm's output after the ReLU mask (fp64)."""
    w = _d(weight)
    rstd = 1.0 / torch.sqrt(_d(var) + eps)
    s = _d(gamma) * rstd
    g = torch.nn.grad.conv2d_weight(x_in, w.shape, dz, padding=w.shape[-1] // 2)
    dbeta = dz.sum(dim=(0, 2, 3))
    dgamma = rstd * ((w * g).sum(dim=(1, 2, 3)) - _d(mean) * dbeta)
    return s.view(-1, 1, 1, 1) * g, dgamma, dbeta


def conv_data_grad(dz, weight, gamma, var, eps=EPS):
    """conv^T(s dz): the input gradient of BN(conv(x)) for the BatchNorm output's gradient dz."""
    w = _d(weight)
    s = _d(gamma) / torch.sqrt(_d(var) + eps)
    return F.conv_transpose2d(dz * s.view(1, -1, 1, 1), w, padding=w.shape[-1] // 2)


def ese_backward(dout, xt, gate, fc_w):
    """(dz_c, dfc_w, dfc_b) from fp64 dout, xt (N, C, H, W), the gate (N, C) whose branch is taken as given, fc_w (C, C[, 1, 1])."""
    c = xt.shape[1]
    hw = xt.shape[2] * xt.shape[3]
    w = _d(fc_w).reshape(c, c)
    dgate = (dout * xt).sum(dim=(2, 3))
    dv = torch.where((gate > 0) & (gate < 1), dgate / 6.0, torch.zeros_like(dgate))
    m = xt.mean(dim=(2, 3))
    dm = dv @ w
    dz = (dout * gate[:, :, None, None] + dm[:, :, None, None] / hw) * (xt > 0)
    return dz, (dv.t() @ m).reshape(fc_w.shape), dv.sum(dim=0)


def _bn(sd, name):
    return (sd[f'{name}/norm.weight'], sd[f'{name}/norm.bias'], sd[f'{name}/norm.running_mean'], sd[f'{name}/norm.running_var'])


def osa_backward(sd, prefix, name, maps, xt, gate, dout, identity):
    """One module: maps [x_0 .. x_L], xt, gate (N, C), dout -> (dx, {state-dict key: gradient}), all fp64.  prefix 'stage3.OSA3_2.',
    name 'OSA3_2' as vovnet_ref.osa_module."""
    maps, xt, gate, dout = [_d(t) for t in maps], _d(xt), _d(gate), _d(dout)
    n_layers = len(maps) - 1
    grads = {}
    dz, grads[f'{prefix}ese.fc.weight'], grads[f'{prefix}ese.fc.bias'] = ese_backward(dout, xt, gate, sd[f'{prefix}ese.fc.weight'])
    cname = f'{prefix}concat.{name}_concat'
    gamma, beta, mean, var = _bn(sd, cname)
    dw, dg, db = conv_param_grads(dz, torch.cat(maps, dim=1), sd[f'{cname}/conv.weight'], gamma, beta, mean, var)
    grads[f'{cname}/conv.weight'], grads[f'{cname}/norm.weight'], grads[f'{cname}/norm.bias'] = dw, dg, db
    g = list(conv_data_grad(dz, sd[f'{cname}/conv.weight'], gamma, var).split([t.shape[1] for t in maps], dim=1))
    for i in range(n_layers, 0, -1):
        lname = f'{prefix}layers.{i - 1}.{name}_{i - 1}'
        gamma, beta, mean, var = _bn(sd, lname)
        dz = g[i] * (maps[i] > 0)
        dw, dg, db = conv_param_grads(dz, maps[i - 1], sd[f'{lname}/conv.weight'], gamma, beta, mean, var)
        grads[f'{lname}/conv.weight'], grads[f'{lname}/norm.weight'], grads[f'{lname}/norm.bias'] = dw, dg, db
        g[i - 1] = g[i - 1] + conv_data_grad(dz, sd[f'{lname}/conv.weight'], gamma, var)
    return (g[0] + dout if identity else g[0]), grads


def module_names(sd):
    """[(stage, 'stage3.OSA3_2.', 'OSA3_2', identity)] in network order."""
    found = sorted({(int(m.group(1)), int(m.group(2))) for k in sd for m in [re.match(r'stage(\d)\.OSA\d_(\d+)\.', k)] if m})
    return [(s, f'stage{s}.OSA{s}_{b}.', f'OSA{s}_{b}', b > 1) for s, b in found]


def network_backward(sd, stem, image, recorded, couts, first_stage=2):
    """The chain over a whole network.  recorded: {module prefix: (maps, xt, partials, gate, out)} of the device's forward; couts:
    {stage number: cotangent of that stage's output}; stem: an fp64 CPU copy of the stem module (its own torch layers), or None when the
    stem and the stages below first_stage are frozen.  The MaxPool2d's are fp64 autograd at the indices of the device's maps.  Returns
    ({state-dict key: gradient}, image gradient or None)."""
    mods = module_names(sd)
    grads, g = {}, None
    for idx in range(len(mods) - 1, -1, -1):
        s, prefix, name, identity = mods[idx]
        if s < first_stage:
            break
        last_of_stage = idx == len(mods) - 1 or mods[idx + 1][0] != s
        if last_of_stage:
            if g is not None:                                                 # through the next stage's pool, at this output's indices
                t = _d(recorded[prefix][4]).requires_grad_(True)
                F.max_pool2d(t, kernel_size=3, stride=2, ceil_mode=True).backward(g)
                g = t.grad
            if s in couts:
                g = _d(couts[s]) if g is None else g + _d(couts[s])
        if g is None:
            continue
        maps, xt, _, gate, _ = recorded[prefix]
        g, mg = osa_backward(sd, prefix, name, maps, xt, gate, g, identity)
        grads.update(mg)
    if stem is None or g is None:
        return grads, None
    x = _d(image).requires_grad_(True)
    torch.nn.Sequential.forward(stem, x).backward(g)                          # its own torch layers, whatever its route switches say
    for k, p in stem.named_parameters():
        grads[f'stem.{k}'] = p.grad
    return grads, x.grad


def rel_err(got, ref):
    """max |got - ref| over the reference's largest |entry|."""
    ref = _d(ref)
    return float((_d(got) - ref).abs().max() / ref.abs().max().clamp(min=1e-30))
