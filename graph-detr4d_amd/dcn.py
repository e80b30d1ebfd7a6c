"""DCNv2, the modulated deformable convolution of the R50 / R101 backbones: mmcv 1.x's `ModulatedDeformConv2d` (offset and mask from the
caller) and `ModulatedDeformConv2dPack` (its own `conv_offset`), which 27 of the reference's configs build with
`dcn=dict(type='DCNv2', deform_groups=1, fallback_on_stride=False), stage_with_dcn=(False, False, True, True)`.  mmcv is not in the
reference tree and not installable here: the semantics are restated from its published definition, and ATen arbitrates.

Both classes take mmcv's constructor keywords and keep its state-dict keys (`weight`, `bias`, `conv_offset.weight`, `conv_offset.bias`;
`_version = 2`).  With s the stride, p the padding, d the dilation, tap k = kw ky + kx of deformable group g, K = kh kw:
    o = conv_offset(x)                         (deform_groups 3 K channels, the convolution's own stride, padding and dilation; zero-init)
    o1, o2, mask = chunk(o, 3); offset = cat(o1, o2); mask = sigmoid(mask)          (the cat restores o[: 2 gK]: the order is unchanged)
    dy_k = offset[2 (g K + k)], dx_k = offset[2 (g K + k) + 1], m_k = mask[g K + k]
    out[n, co, y, x] = bias[co] + sum_{ci, k} weight[co, ci, k] m_k[n, y, x] bilinear0(x[n, ci], y s - p + ky d + dy_k, x s - p + kx d + dx_k)
bilinear0: corners at floor and floor + 1, a corner outside the image contributes 0: F.grid_sample(mode='bilinear',
padding_mode='zeros', align_corners=True) at the same pixel coordinates.

What runs where.  The default route is two launches: gd4d_dcn_offset_conv_fwd (the 27-channel convolution, + bias, sigmoid on the
modulation channels) and gd4d_dcn_fwd (the deformable implicit GEMM on the split-bf16 MFMA; gd4d_dcn.hip).  `forward_bn_relu(x, bn)`
folds an eval()-mode BatchNorm2d and the ReLU behind it into that kernel's epilogue: the bottleneck's relu(bn2(conv2(x))) of every
config (norm_eval=True, frozen).  Inputs that are not fp32 contiguous NCHW are converted with `.float().contiguous()` first (a torch copy).
    torch_ops=False   True (or GD4D_TORCH_OPS=1 for the whole process): K grid_sample calls and one einsum over K Cin - differentiable,
                      any device and dtype, and the route for configurations outside the kernels' limits.
    hip_train=False   True: the kernel route trains.  In train() mode, or with autograd on and a parameter or an input that requires
                      grad, the call is ONE autograd node (_DcnTrainFunction): its forward is the two launches above (the same bits),
                      its backward gd4d_dcn_train.hip's kernels (below).  `torch_ops=True` wins over it.
The kernels' limits: kernel size 3, padding 1, dilation 1, groups = deform_groups = 1, stride 1 or 2, in / out channels multiples of 64
in [64, 512].  The route of a call follows kernel_route.py's rule, the limits checked per call.

The backward (hip_train=True).  The node keeps x (fp32), the 27-channel offset map and - when the ReLU ran - the output (its mask).
    gd4d_dcn_bwd_data            the offset / modulation gradients and dX in one pass: c = W^T g (g = dout x ReLU mask x BatchNorm scale)
                                 stays in the MFMA accumulators, never in memory; dX by float atomicAdd (the one output whose last
                                 bits differ between runs)
    gd4d_dcn_wgrad               dW, dbias: the modulated samples recomputed as the forward forms them, partial sums per pixel
                                 partition added in order
    gd4d_dcn_offset_conv_dgrad / _wgrad   the Pack's conv_offset: dX += conv_transpose(do), dW_off, db_off
Only what `needs_input_grad` asks for is launched: a frozen `weight` skips gd4d_dcn_wgrad, a frozen `conv_offset` its weight gradient,
and with nothing upstream needing grad as well the data kernel.  Gradients come back in the dtype of their tensor.  `forward_bn_relu`
needs the BatchNorm's parameters frozen (requires_grad=False, every config); otherwise it raises and names `torch_ops=True`.  Under
hipGraph capture with gradients wanted the call raises: the node allocates and re-images changed weights.
THE CONVENTION AT INTEGER SAMPLE COORDINATES.  The offset gradient has a kink wherever a sample coordinate is an integer - every offset
of a fresh layer (conv_offset zero-initialised) at training step 0.  The kernels take floor and fraction of the offset, as the forward
does: corners at floor and floor + 1, the derivative from the RIGHT, mmcv's convention and what fp64 autograd through floor-based index
arithmetic gives.  The torch-op route's `grid_sample` normalises the coordinate first, rounds some integers down by an ulp and takes
the LEFT derivative there: on exactly-integer offsets the two routes' offset gradients differ (by as much as the gradient itself); on
any other offsets they agree to rounding.  The arbiter is the floor-based fp64 form, never grid_sample.

Kept state (kernel_route.py): the two weight images and the folded (scale, shift) of a BatchNorm.  The outputs and the offset map
are new tensors every call (torch's caching allocator).
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from . import functional as Fn
from . import ops
from .kernel_route import KernelRoute, f32
from .registry import CONV_LAYERS


def _pair(v):
    return (int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else (int(v), int(v))


def modulated_deform_conv2d_torch(x, offset, mask, weight, bias=None, stride=1, padding=0, dilation=1, groups=1, deform_groups=1):
    """The torch-op route: K grid_sample calls (align_corners=True, zero padding, at pixel coordinates), the modulation, then one
    einsum over K Cin.  offset (N, 2 G K, Ho, Wo), mask (N, G K, Ho, Wo) already through the sigmoid.  Differentiable in every input."""
    sh, sw = _pair(stride)
    ph, pw = _pair(padding)
    dh, dw = _pair(dilation)
    n, cin, h, w = x.shape
    cout, cin_g, kh, kw = weight.shape
    k_all, g = kh * kw, int(deform_groups)
    ho = (h + 2 * ph - dh * (kh - 1) - 1) // sh + 1
    wo = (w + 2 * pw - dw * (kw - 1) - 1) // sw + 1
    if tuple(offset.shape) != (n, 2 * g * k_all, ho, wo) or tuple(mask.shape) != (n, g * k_all, ho, wo):
        raise ValueError(f'modulated_deform_conv2d: offset {tuple(offset.shape)} / mask {tuple(mask.shape)} for an output of '
                         f'({n}, {cout}, {ho}, {wo}) and {g} deformable group(s) of {k_all} taps')
    if cin % g or cin % groups or cout % groups or cin_g * groups != cin:
        raise ValueError('modulated_deform_conv2d: channels do not divide into the groups')
    base_y = (torch.arange(ho, device=x.device, dtype=x.dtype) * sh - ph).view(1, ho, 1)
    base_x = (torch.arange(wo, device=x.device, dtype=x.dtype) * sw - pw).view(1, 1, wo)
    xg = x.reshape(n * g, cin // g, h, w)
    off = offset.reshape(n * g, k_all, 2, ho, wo)
    cols = []
    for k in range(k_all):
        py = base_y + (k // kw) * dh + off[:, k, 0]
        px = base_x + (k % kw) * dw + off[:, k, 1]
        # align_corners=True: pixel p of an axis of size S sits at -1 + 2 p / (S - 1); an axis of one pixel maps every p in (-1, 1) to it
        gx = 2.0 * px / (w - 1) - 1.0 if w > 1 else px
        gy = 2.0 * py / (h - 1) - 1.0 if h > 1 else py
        cols.append(F.grid_sample(xg, torch.stack((gx, gy), dim=-1), mode='bilinear', padding_mode='zeros', align_corners=True))
    col = torch.stack(cols, dim=2).reshape(n, g, cin // g, k_all, ho, wo) * mask.reshape(n, g, 1, k_all, ho, wo)
    col = col.reshape(n, groups, cin // groups, k_all, ho, wo)
    out = torch.einsum('ngckyx,gock->ngoyx', col, weight.reshape(groups, cout // groups, cin_g, k_all)).reshape(n, cout, ho, wo)
    if bias is not None:
        out = out + bias.view(1, -1, 1, 1)
    return out


class _DcnTrainFunction(torch.autograd.Function):
    """The kernel route as one autograd node, for both classes and for forward / forward_bn_relu: forward = the module's two launches,
    backward = the module docstring's kernels.  offset / mask are the caller's (ModulatedDeformConv2d) or None (the Pack, which hands
    its conv_offset parameters instead).  Keeps x, the 27-channel offset map and, when the ReLU ran, the output."""

    @staticmethod
    def forward(ctx, module, bn, relu, x, offset, mask, weight, bias, off_weight, off_bias):
        xf = f32(x)
        pack = offset is None
        offmask = module._offmask_hip(xf) if pack else torch.cat((f32(offset), f32(mask)), dim=1)
        out = module._hip(xf, offmask, bn, relu=relu)
        ctx.module, ctx.bn, ctx.relu, ctx.pack = module, bn, relu, pack
        ctx.dtypes = [None if t is None else t.dtype for t in (x, offset, mask, weight, bias, off_weight, off_bias)]
        ctx.save_for_backward(xf, offmask, out if relu else None, off_weight)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        m = ctx.module
        x, offmask, y, off_weight = ctx.saved_tensors
        need_x, need_off, need_mask, need_w, need_b, need_ow, need_ob = ctx.needs_input_grad[3:]
        g = dout.float().contiguous()
        scale = None if ctx.bn is None else m._folded(ctx.bn)[0]
        stride, cout = m.stride[0], m.out_channels
        grads = [None] * 7
        if need_x or need_off or need_mask or need_ow or need_ob:
            dx, doff = ops.dcn_bwd_data(g, x, offmask, m._weight_image_t(), cout, stride=stride, y=y, scale=scale, sigmoid_grad=ctx.pack,
                                        want_dx=need_x)
            if ctx.pack:
                if need_x:
                    ops.dcn_offset_conv_dgrad(doff, off_weight.detach().float().contiguous(), dx, stride=stride)
                if need_ow or need_ob:
                    grads[5], grads[6] = ops.dcn_offset_conv_wgrad(doff, x, stride=stride)
            else:
                grads[1], grads[2] = doff[:, :18], doff[:, 18:]
            grads[0] = dx
        if need_w or need_b:
            grads[3], grads[4] = ops.dcn_wgrad(g, x, offmask, cout, stride=stride, y=y, scale=scale)
        need = (need_x, need_off, need_mask, need_w, need_b, need_ow, need_ob)
        grads = [gr.to(dt) if gr is not None and wanted else None for gr, wanted, dt in zip(grads, need, ctx.dtypes)]
        return (None, None, None, *grads)


@CONV_LAYERS.register_module('ModulatedDeformConv2d')
class ModulatedDeformConv2d(KernelRoute, nn.Module):
    """mmcv.ops.ModulatedDeformConv2d: forward(x, offset, mask) with the offset (N, 18, Ho, Wo) and the mask (N, 9, Ho, Wo, already
    through the sigmoid) from the caller."""
    _version = 2
    _kernels = 'deformable-convolution kernels have no backward unless asked (a frozen layer belongs in eval() mode)'

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, deform_groups=1, bias=True,
                 torch_ops=False, hip_train=False):
        super().__init__()
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.kernel_size = _pair(kernel_size)
        self.stride, self.padding, self.dilation = _pair(stride), _pair(padding), _pair(dilation)
        self.groups, self.deform_groups = int(groups), int(deform_groups)
        self.transposed, self.output_padding = False, (0, 0)
        self.hip_train = bool(hip_train)
        self.weight = nn.Parameter(torch.empty(self.out_channels, self.in_channels // self.groups, *self.kernel_size))
        if bias:
            self.bias = nn.Parameter(torch.empty(self.out_channels))
        else:
            self.register_parameter('bias', None)
        self._bns = {}              # id -> the BatchNorm2d modules forward_bn_relu has folded (refresh_images re-folds them)
        self.init_weights()
        self._init_route(torch_ops, self._outside_kernel_limits())

    def init_weights(self):
        n = self.in_channels
        for k in self.kernel_size:
            n *= k
        stdv = 1.0 / math.sqrt(n)
        with torch.no_grad():
            self.weight.uniform_(-stdv, stdv)
            if self.bias is not None:
                self.bias.zero_()

    # ---- routes ---------------------------------------------------------------------------------------------------------
    def _outside_kernel_limits(self):
        why = []
        if self.kernel_size != (3, 3):
            why.append(f'kernel_size={self.kernel_size} (kernels: 3)')
        if self.padding != (1, 1):
            why.append(f'padding={self.padding} (kernels: 1)')
        if self.dilation != (1, 1):
            why.append(f'dilation={self.dilation} (kernels: 1)')
        if self.stride not in ((1, 1), (2, 2)):
            why.append(f'stride={self.stride} (kernels: 1 or 2)')
        if self.groups != 1:
            why.append(f'groups={self.groups} (kernels: 1)')
        if self.deform_groups != 1:
            why.append(f'deform_groups={self.deform_groups} (kernels: 1)')
        for name, c in (('in_channels', self.in_channels), ('out_channels', self.out_channels)):
            if c % 64 or not 64 <= c <= 512:
                why.append(f'{name}={c} (kernels: multiples of 64 in [64, 512])')
        return why

    def _route_name(self):
        return f'{type(self).__name__}({self.in_channels}, {self.out_channels})'

    def _route(self, *inputs):
        route = KernelRoute._route(self, *inputs)
        # under torch.no_grad() the training node would record nothing, and its forward IS the inference launches: take those
        return 'infer' if route == 'train' and not torch.is_grad_enabled() else route

    def _train_node(self, x, offset, mask, bn, relu):
        if bn is not None and any(p is not None and p.requires_grad for p in (bn.weight, bn.bias)):
            raise _lib.Gd4dError(f'{type(self).__name__}.forward_bn_relu with hip_train: the BatchNorm2d\'s parameters require grad, and '
                                 'the folded epilogue has no gradient for them.  Freeze them (norm_cfg requires_grad=False, every config) or '
                                 'choose the torch-op route (`torch_ops=True` / GD4D_TORCH_OPS=1).')
        if torch.cuda.is_current_stream_capturing():
            raise _lib.Gd4dError(f'{type(self).__name__} with hip_train under hipGraph capture with gradients wanted: the training node '
                                 'allocates and re-images changed weights.  Capture the forward under torch.no_grad() in eval() mode.')
        conv_offset = getattr(self, 'conv_offset', None) if offset is None else None
        off_weight, off_bias = (None, None) if conv_offset is None else (conv_offset.weight, conv_offset.bias)
        return _DcnTrainFunction.apply(self, bn, relu, x, offset, mask, self.weight, self.bias, off_weight, off_bias)

    # ---- kept values ----------------------------------------------------------------------------------------------------
    def _weight_image(self):
        return self._keep('weight', (self.weight,), lambda: ops.dcn_weight_image(self.weight.detach().float()))

    def _weight_image_t(self):
        return self._keep('weight_t', (self.weight,), lambda: ops.dcn_weight_image_t(self.weight.detach().float()))

    def _folded(self, bn):
        """(2, Cout): scale = gamma / sqrt(var + eps) and shift = beta + (bias - mean) scale of an eval()-mode BatchNorm2d behind the
        convolution's bias."""
        sources = (bn.weight, bn.bias, bn.running_mean, bn.running_var, self.bias)
        return self._keep(('bn', id(bn), float(bn.eps)), sources, lambda: Fn.folded_batchnorm(bn, self.bias))

    def _kept_values(self):
        self._weight_image()
        for bn in self._bns.values():
            self._folded(bn)

    # ---- forward --------------------------------------------------------------------------------------------------------
    def _check_bn(self, bn):
        if not isinstance(bn, nn.BatchNorm2d) or bn.num_features != self.out_channels:
            raise ValueError(f'forward_bn_relu: a BatchNorm2d of {self.out_channels} features expected')
        if bn.training or bn.running_mean is None:
            raise _lib.Gd4dError('forward_bn_relu: the BatchNorm2d must be in eval() mode with running statistics (the frozen form every '
                                 'config uses: norm_eval=True); batch statistics are not folded into a convolution')

    def _hip(self, x, offmask, bn=None, relu=False):
        if bn is None:
            scale, shift = None, None if self.bias is None else self.bias.detach()
        else:
            self._bns[id(bn)] = bn
            scale, shift = self._folded(bn)
        return ops.dcn_fwd(x, offmask, self._weight_image(), self.out_channels, stride=self.stride[0], scale=scale, shift=shift, relu=relu)

    def _torch(self, x, offset, mask):
        return modulated_deform_conv2d_torch(x, offset, mask, self.weight, self.bias, self.stride, self.padding, self.dilation,
                                             self.groups, self.deform_groups)

    def forward(self, x, offset, mask):
        route = self._route(x, offset, mask)
        if route == 'torch':
            return self._torch(x, offset, mask)
        if route == 'train':
            return self._train_node(x, offset, mask, None, False)
        with torch.no_grad():
            return self._hip(f32(x), torch.cat((f32(offset), f32(mask)), dim=1))

    def forward_bn_relu(self, x, offset, mask, bn):
        """relu(bn(forward(x, offset, mask))) for an eval()-mode BatchNorm2d, folded into the kernel's epilogue."""
        self._check_bn(bn)
        route = self._route(x, offset, mask)
        if route == 'torch':
            return F.relu(bn(self._torch(x, offset, mask)))
        if route == 'train':
            return self._train_node(x, offset, mask, bn, True)
        with torch.no_grad():
            return self._hip(f32(x), torch.cat((f32(offset), f32(mask)), dim=1), bn, relu=True)


@CONV_LAYERS.register_module('DCNv2')
class ModulatedDeformConv2dPack(ModulatedDeformConv2d):
    """mmcv.ops.ModulatedDeformConv2dPack ('DCNv2'): the layer computes its own offsets and modulation with `conv_offset`, a plain
    convolution of 3 K deform_groups channels, zero-initialised (so a fresh layer is 0.5 x the plain convolution)."""
    _version = 2

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.conv_offset = nn.Conv2d(self.in_channels, self.deform_groups * 3 * self.kernel_size[0] * self.kernel_size[1],
                                     kernel_size=self.kernel_size, stride=self.stride, padding=self.padding, dilation=self.dilation,
                                     bias=True)
        with torch.no_grad():
            self.conv_offset.weight.zero_()
            self.conv_offset.bias.zero_()

    def init_weights(self):
        super().init_weights()
        if hasattr(self, 'conv_offset'):
            with torch.no_grad():
                self.conv_offset.weight.zero_()
                self.conv_offset.bias.zero_()

    def _offset_image(self):
        return self._keep('conv_offset', (self.conv_offset.weight,), lambda: ops.dcn_weight_image(self.conv_offset.weight.detach().float()))

    def _kept_values(self):
        super()._kept_values()
        self._offset_image()

    def offsets_torch(self, x):
        """(offset, mask) by the module's own torch layers, mmcv's op sequence."""
        o1, o2, mask = torch.chunk(self.conv_offset(x), 3, dim=1)
        return torch.cat((o1, o2), dim=1), torch.sigmoid(mask)

    def _offmask_hip(self, x):
        return ops.dcn_offset_conv_fwd(x, self._offset_image(), self.conv_offset.bias.detach(), stride=self.stride[0])

    def forward(self, x):
        route = self._route(x)
        if route == 'torch':
            return self._torch(x, *self.offsets_torch(x))
        if route == 'train':
            return self._train_node(x, None, None, None, False)
        with torch.no_grad():
            x = f32(x)
            return self._hip(x, self._offmask_hip(x))

    def forward_bn_relu(self, x, bn):
        """relu(bn(forward(x))) for an eval()-mode BatchNorm2d: the bottleneck's relu(bn2(conv2(x))), folded into the kernel's epilogue."""
        self._check_bn(bn)
        route = self._route(x)
        if route == 'torch':
            return F.relu(bn(self._torch(x, *self.offsets_torch(x))))
        if route == 'train':
            return self._train_node(x, None, None, bn, True)
        with torch.no_grad():
            x = f32(x)
            return self._hip(x, self._offmask_hip(x), bn, relu=True)

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        version = local_metadata.get('version', None)
        if version is None or version < 2:
            # mmcv: before version 2 the offset convolution was saved as `<name>_offset` next to the layer
            for leaf in ('weight', 'bias'):
                old, new = f'{prefix[:-1]}_offset.{leaf}', f'{prefix}conv_offset.{leaf}'
                if old in state_dict and new not in state_dict:
                    state_dict[new] = state_dict.pop(old)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)


CONV_LAYERS.register_module('ModulatedDeformConv2dPack', module=ModulatedDeformConv2dPack)
