"""fp64 restatement of the neck: mmdet's FPN and the reference's CPFPN (projects/mmdet3d_plugin/models/necks/cp_fpn.py:157-208), from
a state dict with the reference's keys.  Plain torch on the CPU; ATen arbitrates the convolutions and the nearest interpolation."""
import torch
import torch.nn.functional as F


def nearest_index(dst, n_in, n_out):
    """ATen's nearest source index, the rule the lateral kernel restates: min(floor(float(dst) * (float(in) / float(out))), in - 1),
    every operation in fp32."""
    scale = torch.tensor(n_in, dtype=torch.float32) / torch.tensor(n_out, dtype=torch.float32)
    src = torch.floor(torch.as_tensor(dst, dtype=torch.float32) * scale).to(torch.int64)
    return torch.clamp(src, max=n_in - 1)


def upsample_nearest(x, size):
    """F.interpolate(x, size=size, mode='nearest') by the index rule (any dtype)."""
    iy = nearest_index(torch.arange(size[0]), x.shape[-2], size[0])
    ix = nearest_index(torch.arange(size[1]), x.shape[-1], size[1])
    return x[..., iy, :][..., ix]


def lateral(x, w, b, up=None):
    """(conv1x1(x) + b) + nearest(up), fp64."""
    y = F.conv2d(x.double(), w.double().reshape(w.shape[0], -1, 1, 1), b.double())
    return y if up is None else y + upsample_nearest(up.double(), y.shape[-2:])


def conv3x3(x, w, b=None, stride=1, relu_in=False):
    x = x.double()
    return F.conv2d(F.relu(x) if relu_in else x, w.double(), None if b is None else b.double(), stride=stride, padding=1)


def fpn_forward(sd, inputs, *, start_level=0, num_outs, relu_before_extra_convs=False, cp=False):
    """(laterals, outs) in fp64 for add_extra_convs='on_output'.  cp: CPFPN - only level 0 has a 3x3 output convolution
    (fpn_convs.0), the other levels return their laterals; the extras follow in fpn_convs."""
    n_lat = len([k for k in sd if k.startswith('lateral_convs.') and k.endswith('.conv.weight')])
    lats = [None] * n_lat
    for i in range(n_lat - 1, -1, -1):                                                        # :162-178
        lats[i] = lateral(inputs[i + start_level], sd[f'lateral_convs.{i}.conv.weight'], sd[f'lateral_convs.{i}.conv.bias'],
                          lats[i + 1] if i + 1 < n_lat else None)
    if cp:                                                                                    # :182-184
        outs = [conv3x3(lats[0], sd['fpn_convs.0.conv.weight'], sd['fpn_convs.0.conv.bias'])] + lats[1:]
        k = 1
    else:
        outs = [conv3x3(lats[i], sd[f'fpn_convs.{i}.conv.weight'], sd[f'fpn_convs.{i}.conv.bias']) for i in range(n_lat)]
        k = n_lat
    first = True
    while len(outs) < num_outs:                                                               # :202-207
        outs.append(conv3x3(outs[-1], sd[f'fpn_convs.{k}.conv.weight'], sd[f'fpn_convs.{k}.conv.bias'], stride=2,
                            relu_in=relu_before_extra_convs and not first))
        first = False
        k += 1
    return lats, outs


def rel_err(got, ref):
    """max |got - ref| over the map, divided by the map's largest |entry|."""
    ref = ref.double()
    return float((got.detach().cpu().double() - ref).abs().max() / ref.abs().max())
