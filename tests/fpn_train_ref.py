"""fp64 backward of the neck: autograd over fpn_ref's restatement in float64, with a hook to impose a given ReLU mask on the extra
levels' input (the backward is then the derivative of the forward a device computed, not of the fp64 one), the adjoint of the nearest
upsampling, and the candidate rule by which the top-down adjoint kernel finds a coarse pixel's children.  Plain torch on the CPU."""
import torch

import fpn_ref as R


def rel_fro(got, ref):
    """|got - ref|_F / |ref|_F."""
    ref = ref.double()
    return float((got.detach().cpu().double() - ref).norm() / ref.norm().clamp(min=1e-300))


def forward(sd, inputs, *, start_level=0, num_outs, relu_before_extra_convs=False, cp=False, relu_masks=None):
    """fpn_ref.fpn_forward's outputs from its own pieces.  relu_masks: {output index k: bool mask} - the extra level reading output k
    takes x * mask instead of relu(x) (None: relu)."""
    n_lat = len([k for k in sd if k.startswith('lateral_convs.') and k.endswith('.conv.weight')])
    lats = [None] * n_lat
    for i in range(n_lat - 1, -1, -1):
        lats[i] = R.lateral(inputs[i + start_level], sd[f'lateral_convs.{i}.conv.weight'], sd[f'lateral_convs.{i}.conv.bias'],
                            lats[i + 1] if i + 1 < n_lat else None)
    if cp:
        outs = [R.conv3x3(lats[0], sd['fpn_convs.0.conv.weight'], sd['fpn_convs.0.conv.bias'])] + lats[1:]
        k = 1
    else:
        outs = [R.conv3x3(lats[i], sd[f'fpn_convs.{i}.conv.weight'], sd[f'fpn_convs.{i}.conv.bias']) for i in range(n_lat)]
        k = n_lat
    first = True
    while len(outs) < num_outs:
        x, relu = outs[-1], relu_before_extra_convs and not first
        mask = None if relu_masks is None else relu_masks.get(len(outs) - 1)
        if relu and mask is not None:
            x, relu = x * mask.to(x.dtype), False
        outs.append(R.conv3x3(x, sd[f'fpn_convs.{k}.conv.weight'], sd[f'fpn_convs.{k}.conv.bias'], stride=2, relu_in=relu))
        first = False
        k += 1
    return outs


def backward(sd, inputs, rs, forward_fn=forward, **cfg):
    """Gradients of sum_k (out_k * r_k).sum() in fp64 -> (outs, {state-dict key: grad}, [input grad or None (an input not read)])."""
    sd64 = {k: v.detach().double().requires_grad_(True) for k, v in sd.items()}
    xs = [x.detach().double().requires_grad_(True) for x in inputs]
    outs = forward_fn(sd64, xs, **cfg)
    if isinstance(outs, tuple) and len(outs) == 2 and isinstance(outs[0], list):
        outs = outs[1]                                                       # (fpn_ref.fpn_forward returns (laterals, outs))
    sum((o * r.double()).sum() for o, r in zip(outs, rs)).backward()
    return [o.detach() for o in outs], {k: v.grad for k, v in sd64.items()}, [x.grad for x in xs]


def upsample_adjoint(g_fine, coarse_hw):
    """U^T g_fine for U = fpn_ref.upsample_nearest to g_fine's size, by fp64 autograd."""
    z = torch.zeros(*g_fine.shape[:-2], *coarse_hw, dtype=torch.float64, requires_grad=True)
    (R.upsample_nearest(z, g_fine.shape[-2:]) * g_fine.double()).sum().backward()
    return z.grad


def topdown_children(n_coarse, n_fine):
    """What gd4d_fpn_topdown_bwd does along one axis: for each coarse index c, the candidates lo .. hi (the exact-ratio range, one pixel
    wider on both sides, integer arithmetic) that fpn_ref.nearest_index sends to c."""
    src = R.nearest_index(torch.arange(n_fine), n_coarse, n_fine).tolist()
    out = []
    for c in range(n_coarse):
        lo = max(0, c * n_fine // n_coarse - 1)
        hi = min(n_fine - 1, ((c + 1) * n_fine + n_coarse - 1) // n_coarse + 1)
        out.append([d for d in range(lo, hi + 1) if src[d] == c])
    return out
