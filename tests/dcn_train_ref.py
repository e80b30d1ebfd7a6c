"""fp64 gradients of DCNv2 (dcn_ref.py's function), two ways: the closed form the training kernels implement, by explicit index
arithmetic, and autograd through dcn_ref.dcn_ref / offset_conv_ref - the arbiter (floor-based corners: at an integer sample
coordinate the offset gradient is the derivative from the right, mmcv's convention; grid_sample takes the other side there).

With g = dout x (ReLU mask) x (scale), tap k = 3 ky + kx, m_k the modulation, S the unmodulated sample, v_ab / wgt_ab the corners:
    c[ci, k, p] = sum_co w[co, ci, k] g[co, p]        dmod_k = sum_ci c S
    d(dy_k) = m_k sum_ci c ((1 - lx)(v10 - v00) + lx (v11 - v01))      d(dx_k) = m_k sum_ci c ((1 - ly)(v01 - v00) + ly (v11 - v10))
    dX[ci, corner] += m_k wgt c        dW[co, ci, k] = sum g m_k S        dbias[co] = sum g
and through conv_offset: do = (d offset, dmod m (1 - m)), dX += conv_transpose(do, W_off), dW_off = sum do x, db_off = sum do."""
import torch

import dcn_ref as R

F64 = R.F64


def _g(dout, scale=None, relu_mask=None):
    g = dout.to(F64)
    if relu_mask is not None:
        g = g * relu_mask.to(F64)
    if scale is not None:
        g = g * scale.to(F64).view(1, -1, 1, 1)
    return g


def closed_form(x, offset, mask, weight, dout, stride=1, scale=None, relu_mask=None):
    """dict(x, offset, mask, weight, bias): the fp64 gradients of sum(dcn_ref(...) * scale, masked, * dout) by the formulas above."""
    x, offset, mask, weight = x.to(F64), offset.to(F64), mask.to(F64), weight.to(F64)
    g = _g(dout, scale, relu_mask)
    n, cin, h, w = x.shape
    ho, wo = R.out_hw(h, w, stride)
    base_y = (torch.arange(ho, dtype=F64) * stride - 1).view(1, ho, 1)
    base_x = (torch.arange(wo, dtype=F64) * stride - 1).view(1, 1, wo)
    flat = x.reshape(n, cin, h * w)
    dx = torch.zeros(n, cin, h * w, dtype=F64)
    doffset, dmask, dweight = torch.zeros_like(offset), torch.zeros_like(mask), torch.zeros_like(weight)
    for k in range(9):
        ky, kx = k // 3, k % 3
        c = torch.einsum('oc,noyx->ncyx', weight[:, :, ky, kx], g)
        py = (base_y + ky + offset[:, 2 * k]).clamp(-4.0, h + 4.0)          # (dcn_ref's clamp: far outside samples nothing)
        px = (base_x + kx + offset[:, 2 * k + 1]).clamp(-4.0, w + 4.0)
        y0, x0 = torch.floor(py), torch.floor(px)
        ly, lx = (py - y0).unsqueeze(1), (px - x0).unsqueeze(1)
        m = mask[:, k:k + 1]
        v, idx, inside = {}, {}, {}
        for a in (0, 1):
            for b in (0, 1):
                yy, xx = (y0 + a).long(), (x0 + b).long()
                inside[a, b] = ((yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)).to(F64).unsqueeze(1)
                idx[a, b] = (yy.clamp(0, h - 1) * w + xx.clamp(0, w - 1)).reshape(n, 1, -1).expand(n, cin, -1)
                v[a, b] = torch.gather(flat, 2, idx[a, b]).reshape(n, cin, ho, wo) * inside[a, b]
        wgt = {(0, 0): (1 - ly) * (1 - lx), (0, 1): (1 - ly) * lx, (1, 0): ly * (1 - lx), (1, 1): ly * lx}
        s = sum(wgt[ab] * v[ab] for ab in wgt)
        dmask[:, k] = (c * s).sum(1)
        doffset[:, 2 * k] = (m * c * ((1 - lx) * (v[1, 0] - v[0, 0]) + lx * (v[1, 1] - v[0, 1]))).sum(1)
        doffset[:, 2 * k + 1] = (m * c * ((1 - ly) * (v[0, 1] - v[0, 0]) + ly * (v[1, 1] - v[1, 0]))).sum(1)
        for ab in wgt:
            dx.scatter_add_(2, idx[ab], (m * wgt[ab] * inside[ab] * c).reshape(n, cin, -1))
        dweight[:, :, ky, kx] = torch.einsum('noyx,ncyx->oc', g, m * s)
    return dict(x=dx.reshape(n, cin, h, w), offset=doffset, mask=dmask, weight=dweight, bias=g.sum((0, 2, 3)))


def closed_form_pack(x, weight, off_weight, off_bias, dout, stride=1, scale=None, relu_mask=None):
    """dict(x, weight, bias, off_weight, off_bias, do, x_offset_term) for the Pack: the formulas above continued through conv_offset."""
    x64 = x.to(F64)
    off, msk = R.offset_conv_ref(x64, off_weight, off_bias, stride)
    d = closed_form(x64, off, msk, weight, dout, stride, scale, relu_mask)
    do = torch.cat((d['offset'], d['mask'] * msk * (1 - msk)), dim=1)
    term, dow, dob = offset_conv_closed_form(x64, off_weight, do, stride)
    return dict(x=d['x'] + term, weight=d['weight'], bias=d['bias'], off_weight=dow, off_bias=dob, do=do, x_offset_term=term)


def offset_conv_closed_form(x, off_weight, do, stride=1):
    """(conv_transpose3x3(do, W_off), dW_off, db_off) in fp64 by slicing a padded image."""
    x, off_weight, do = x.to(F64), off_weight.to(F64), do.to(F64)
    n, cin, h, w = x.shape
    ho, wo = R.out_hw(h, w, stride)
    hp, wp = stride * (ho - 1) + 3, stride * (wo - 1) + 3                   # the padded extent the taps reach
    xp = torch.zeros(n, cin, max(hp, h + 2), max(wp, w + 2), dtype=F64)
    xp[:, :, 1:h + 1, 1:w + 1] = x
    dxp = torch.zeros_like(xp)
    dow = torch.zeros_like(off_weight)
    for ky in range(3):
        for kx in range(3):
            sl = (slice(None), slice(None), slice(ky, ky + stride * (ho - 1) + 1, stride), slice(kx, kx + stride * (wo - 1) + 1, stride))
            dxp[sl] += torch.einsum('njyx,jc->ncyx', do, off_weight[:, :, ky, kx])
            dow[:, :, ky, kx] = torch.einsum('njyx,ncyx->jc', do, xp[sl])
    return dxp[:, :, 1:h + 1, 1:w + 1].clone(), dow, do.sum((0, 2, 3))


def autograd(x, offset, mask, weight, dout, stride=1, scale=None, relu_mask=None):
    """The same dict by fp64 autograd through dcn_ref.dcn_ref: the arbiter."""
    x, offset, mask, weight = (t.detach().to(F64).clone().requires_grad_(True) for t in (x, offset, mask, weight))
    bias = torch.zeros(weight.shape[0], dtype=F64, requires_grad=True)
    out = R.dcn_ref(x, offset, mask, weight, bias, stride)
    (out * _g(dout, scale, relu_mask)).sum().backward()
    return dict(x=x.grad, offset=offset.grad, mask=mask.grad, weight=weight.grad, bias=bias.grad)


def autograd_pack(x, weight, off_weight, off_bias, dout, stride=1, scale=None, relu_mask=None):
    """dict(x, weight, bias, off_weight, off_bias) by fp64 autograd through offset_conv_ref and dcn_ref."""
    x, weight, off_weight, off_bias = (t.detach().to(F64).clone().requires_grad_(True) for t in (x, weight, off_weight, off_bias))
    bias = torch.zeros(weight.shape[0], dtype=F64, requires_grad=True)
    off, msk = R.offset_conv_ref(x, off_weight, off_bias, stride)
    out = R.dcn_ref(x, off, msk, weight, bias, stride)
    (out * _g(dout, scale, relu_mask)).sum().backward()
    return dict(x=x.grad, weight=weight.grad, bias=bias.grad, off_weight=off_weight.grad, off_bias=off_bias.grad)


def rel_fro(got, ref):
    """||got - ref||_F / ||ref||_F."""
    ref = ref.detach().to(F64)
    return float((got.detach().cpu().to(F64) - ref).norm() / ref.norm().clamp(min=1e-300))
