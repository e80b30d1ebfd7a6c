"""fp64 restatement of DCNv2 (mmcv 1.x ModulatedDeformConv2d, 3x3, padding 1, dilation 1, groups = deform_groups = 1) by explicit index
arithmetic - no grid_sample: what tests/test_dcn_cpu.py and tests/test_dcn_gpu.py compare against.

    out[n, co, y, x] = bias[co] + sum_{ci, k} w[co, ci, k] m_k[n, y, x] bilinear0(x[n, ci], y s - 1 + ky + dy_k, x s - 1 + kx + dx_k)
with tap k = 3 ky + kx, dy_k = offset[2 k], dx_k = offset[2 k + 1]; bilinear0 has corners at floor and floor + 1 and a corner outside
[0, H - 1] x [0, W - 1] contributes 0."""
import torch

F64 = torch.float64


def out_hw(h, w, stride):
    return (h - 1) // stride + 1, (w - 1) // stride + 1


def bilinear0(x, py, px):
    """x (N, C, H, W), py / px (N, Ho, Wo) pixel coordinates -> (N, C, Ho, Wo), fp64."""
    x, py, px = x.to(F64), py.to(F64), px.to(F64)
    n, c, h, w = x.shape
    # (coordinates far outside sample nothing; clamping them first keeps the integer conversion defined)
    py, px = py.clamp(-4.0, h + 4.0), px.clamp(-4.0, w + 4.0)
    y0, x0 = torch.floor(py), torch.floor(px)
    ly, lx = py - y0, px - x0
    flat = x.reshape(n, c, h * w)
    out = torch.zeros(n, c, *py.shape[1:], dtype=F64)
    for dy, wy in ((0, 1.0 - ly), (1, ly)):
        for dx, wx in ((0, 1.0 - lx), (1, lx)):
            yy, xx = (y0 + dy).long(), (x0 + dx).long()
            inside = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
            idx = (yy.clamp(0, h - 1) * w + xx.clamp(0, w - 1)).reshape(n, 1, -1).expand(n, c, -1)
            v = torch.gather(flat, 2, idx).reshape(n, c, *py.shape[1:])
            out += v * (wy * wx * inside.to(F64)).unsqueeze(1)
    return out


def dcn_ref(x, offset, mask, weight, bias=None, stride=1):
    """x (N, Cin, H, W), offset (N, 18, Ho, Wo), mask (N, 9, Ho, Wo) (already through the sigmoid), weight (Cout, Cin, 3, 3) -> fp64
    (N, Cout, Ho, Wo)."""
    n, cin, h, w = x.shape
    ho, wo = out_hw(h, w, stride)
    assert tuple(offset.shape) == (n, 18, ho, wo) and tuple(mask.shape) == (n, 9, ho, wo)
    offset, mask, weight = offset.to(F64), mask.to(F64), weight.to(F64)
    base_y = (torch.arange(ho, dtype=F64) * stride - 1).view(1, ho, 1)
    base_x = (torch.arange(wo, dtype=F64) * stride - 1).view(1, 1, wo)
    out = torch.zeros(n, weight.shape[0], ho, wo, dtype=F64)
    for k in range(9):
        s = bilinear0(x, base_y + k // 3 + offset[:, 2 * k], base_x + k % 3 + offset[:, 2 * k + 1]) * mask[:, k:k + 1]
        out += torch.einsum('ncyx,oc->noyx', s, weight[:, :, k // 3, k % 3])
    if bias is not None:
        out += bias.to(F64).view(1, -1, 1, 1)
    return out


def offset_conv_ref(x, weight, bias, stride=1):
    """conv_offset and mmcv's split: fp64 (offset (N, 18, Ho, Wo), mask (N, 9, Ho, Wo) through the sigmoid)."""
    o = torch.nn.functional.conv2d(x.to(F64), weight.to(F64), None if bias is None else bias.to(F64), stride=stride, padding=1)
    return o[:, :18], torch.sigmoid(o[:, 18:])


def rel_err(got, ref):
    """max |got - ref| over the map's largest |entry|."""
    ref = ref.detach().to(F64)
    return float((got.detach().cpu().to(F64) - ref).abs().max() / ref.abs().max().clamp(min=1e-30))


def crafted_offsets(h, w, stride, seed=0):
    """name -> offset (1, 18, Ho, Wo) fp32: the planes of the issue's list.  The sample coordinate of tap (ky, kx) at output (y, x) is
    (y s - 1 + ky + dy, x s - 1 + kx + dx)."""
    ho, wo = out_hw(h, w, stride)
    g = torch.Generator().manual_seed(seed)
    ys = (torch.arange(ho, dtype=torch.float32) * stride - 1).view(ho, 1).expand(ho, wo)
    xs = (torch.arange(wo, dtype=torch.float32) * stride - 1).view(1, wo).expand(ho, wo)
    planes = {'zero': torch.zeros(1, 18, ho, wo), 'integers': torch.randint(-3, 4, (1, 18, ho, wo), generator=g).float()}

    def land_on(ty, tx):
        """every tap of every pixel samples exactly (ty, tx)"""
        o = torch.zeros(1, 18, ho, wo)
        for k in range(9):
            o[0, 2 * k] = ty - (ys + k // 3)
            o[0, 2 * k + 1] = tx - (xs + k % 3)
        return o
    planes['at_minus_1'] = land_on(-1.0, -1.0)
    planes['at_h_minus_1'] = land_on(h - 1.0, w - 1.0)
    planes['at_h_and_w'] = land_on(float(h), float(w))
    planes['plus_1000'] = torch.full((1, 18, ho, wo), 1000.0)
    planes['minus_1000'] = torch.full((1, 18, ho, wo), -1000.0)
    # one corner inside, at each of the four image corners: the sample sits 0.25 px outside the corner pixel on both axes
    for name, (ty, tx) in dict(corner_tl=(-0.25, -0.25), corner_tr=(-0.25, w - 0.75), corner_bl=(h - 0.75, -0.25),
                               corner_br=(h - 0.75, w - 0.75)).items():
        planes[name] = land_on(ty, tx)
    return planes
