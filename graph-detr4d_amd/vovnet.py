"""VoVNet with eSE, the image backbone of the reference's VoVNet configurations (models/backbones/vovnet.py `VoVNet`, vovnetcp.py
`VoVNetCP`; eight shipped configs, all `spec_name='V-99-eSE'`):
    img_backbone=dict(type='VoVNetCP', spec_name='V-99-eSE', norm_eval=True, frozen_stages=-1, input_ch=3, out_features=('stage4', 'stage5'))
`VoVNet.forward` returns a dict keyed by feature name, `VoVNetCP.forward` a list in stage order.  Both keep the reference's module
tree, so the state-dict keys are its own (`stem.stem_1/conv.weight`, `stage3.OSA3_2.layers.4.OSA3_2_4/norm.running_var`,
`stage2.OSA2_1.concat.OSA2_1_concat/conv.weight`, `stage5.OSA5_3.ese.fc.bias`) and a checkpoint's backbone slice loads with strict=True.

The network: a stem of three conv3x3 + BN + ReLU (strides 2, 1, 2), then stages 2-5 of OSA modules, a MaxPool2d(3, 2, ceil_mode=True)
in front of stages 3-5.  One OSA module (L layers of `stage_ch` channels, `concat_ch` outputs):
    x_0 = input;  x_i = relu(bn_i(conv3x3_i(x_{i-1})))  (i = 1 .. L);  xt = relu(bn(conv1x1(cat(x_0 .. x_L))))
    out = xt * relu6(fc(mean_{hw}(xt)) + 3) / 6  (+ input, in every module of a stage but its first)

What runs where.  The default route is inference on the library's kernels (gd4d_vovnet.hip), eight launches per five-layer module:
    ops.conv3x3_bn_relu   x L     the 3x3 convolutions, BatchNorm (folded: scale, shift) and ReLU in the epilogue; also stem_2 and stem_3
    ops.osa_concat_conv           the aggregation reads the L + 1 maps where they lie: the concatenation is never written; its epilogue
                                  also leaves each tile's per-channel sums for the pool
    ops.ese_gate, ops.ese_apply   the (C x C) matvec per image, then xt * gate (+ input) in place
Stock torch inside the kernel route, deliberately: `stem_1` (3 input channels, K = 27: F.conv2d, then the folded BatchNorm and ReLU)
and the MaxPool2d in front of stages 3-5.  Inputs that are not fp32 contiguous NCHW are converted with `.float().contiguous()`.
    torch_ops=False   True (or GD4D_TORCH_OPS=1 for the whole process): the reference's op sequence - differentiable, any device and
                      dtype, `torch.utils.checkpoint` per OSA module for VoVNetCP (with_cp=True) in train() mode, and the route for the
                      specs outside the kernels' limits.
                      The switch lives on the stem and on each OSA module (they decide their route per call); the network's
                      `torch_ops` attribute, and `with Fn.torch_ops_for(net):`, set all of them.
The kernels' limits: plain (not depthwise) 3x3 layers, every channel count a multiple of 32, 3x3 inputs up to 1024 and outputs up to 256
channels, at most five layers per module, concatenations up to 2304 and module outputs up to 1024 channels: V-19-eSE, V-39, V-57 and
V-99.  The two depthwise specs and V-19-slim-eSE (80- and 112-channel layers) are refused AT CONSTRUCTION unless torch_ops=True.  The
route of a call follows kernel_route.py's rule; "train mode" is here a BatchNorm that is not frozen (norm_eval=False).

Training on the kernels is opt-in: `hip_train=True` (a keyword of VoVNet / VoVNetCP, of the stem and of the OSA module, and like
`torch_ops` a network attribute that reaches every routed module; `torch_ops=True` wins over it; off, nothing differs).  What every
config trains with - norm_eval=True, frozen_stages=-1, with_cp=True - then runs each OSA module as ONE autograd node
(`_OsaTrainFunction`) on gd4d_vovnet_train.hip.  With s_i = gamma_i rstd_i the backward, given dout:
    1. eSE        dgate[n, c] = sum_hw dout xt;  dv = dgate / 6 where 0 < gate < 1 ON THE STORED fp32 GATE, else 0 (the clamp's two
                  corners pass nothing, as its flat parts);  dfc_b = sum_n dv, dfc_w = sum_n dv (x) m, dm = fc_w^T dv;
                  dz_c = (dout gate + dm / HW) [xt > 0];  m is re-formed from the kept pool partials in the forward's order: the same bits
    2. aggregation  g_i = the rows of source i of (s_c W_c)^T dz_c, written into L + 1 separate maps; the last one masked: dz_L
    3. the chain, i = L .. 1:  g_{i-1} += conv3x3^T((s_i W_i) transposed, taps flipped; dz_i), then dz_{i-1} = g_{i-1} [x_{i-1} > 0]
                  in the same epilogue; at the input no mask, and dx_0 = g_0 (+ dout with the residual)
    4. parameters of every convolution:  G[c, k, tap] = sum dz[c, p] x_in[k, p + tap] on the unscaled dz;  dW = s (x) G,
                  dbeta[c] = sum dz,  dgamma[c] = rstd[c] (<W[c], G[c]> - mean[c] dbeta[c]) - the pre-BatchNorm map is W * x_in, so
                  none is stored or recomputed, and gamma = 0 is exact
Gradients are computed only for what asks (a frozen ese.fc or layer gets None and its launch is skipped; the chain stops at the
lowest layer that needs it); dx comes back in the input's dtype.  With with_cp=True in train() mode the node keeps only its input
and runs the forward launches again in backward (deterministic kernels: the same bits); otherwise it keeps x_1 .. x_L, xt, the
partials and the gate.  Modules of frozen stages (eval(), no gradient wanted) keep taking the inference launches.
Outside the HIP training route: an unfrozen BatchNorm (refused at the call, naming torch_ops=True); the stem - one that needs
gradients runs its own torch layers, stem_1 and the stride-2 stem_3 have no HIP backward; the MaxPool2d's (torch autograd between
the nodes); accumulation into the flat gradient buffer (dist.FlatGradAllReducer's fused weight gradients); hipGraph capture of the
training step; the depthwise and slim specs.

Kept state (kernel_route.py): per convolution its weight image and the folded (scale, shift) of its BatchNorm; with hip_train also the
scaled transposed image of the data gradient and (scale, rstd, mean), sources (conv.weight, bn.*): the one validity rule covers them and
`refresh_images()` rebuilds them.  The maps, partials and gates are new tensors every call (torch's caching allocator).
"""
import warnings
from collections import OrderedDict

import torch
import torch.nn as nn
import torch.nn.functional as F
import torch.utils.checkpoint as cp
from torch.nn.modules.batchnorm import _BatchNorm

from . import functional as Fn
from . import _lib, ops
from .kernel_route import KernelRoute, f32, refuse_outside_limits
from .registry import BACKBONES


def _spec(stem, conv_ch, out_ch, layers, blocks, dw):
    return dict(stem=stem, stage_conv_ch=conv_ch, stage_out_ch=out_ch, layer_per_block=layers, block_per_stage=blocks, eSE=True, dw=dw)


_WIDE, _SLIM = ([128, 160, 192, 224], [256, 512, 768, 1024]), ([64, 80, 96, 112], [112, 256, 384, 512])
_STAGE_SPECS = {
    'V-19-slim-dw-eSE': _spec([64, 64, 64], *_SLIM, 3, [1, 1, 1, 1], True),
    'V-19-dw-eSE': _spec([64, 64, 64], *_WIDE, 3, [1, 1, 1, 1], True),
    'V-19-slim-eSE': _spec([64, 64, 128], *_SLIM, 3, [1, 1, 1, 1], False),
    'V-19-eSE': _spec([64, 64, 128], *_WIDE, 3, [1, 1, 1, 1], False),
    'V-39-eSE': _spec([64, 64, 128], *_WIDE, 5, [1, 1, 2, 2], False),
    'V-57-eSE': _spec([64, 64, 128], *_WIDE, 5, [1, 1, 4, 3], False),
    'V-99-eSE': _spec([64, 64, 128], *_WIDE, 5, [1, 3, 9, 3], False),
}


def _conv_bn_relu(cin, cout, name, kernel_size, stride=1):
    """The reference's conv3x3 / conv1x1 triple: `<name>/conv` (no bias), `<name>/norm`, `<name>/relu`."""
    return [(f'{name}/conv', nn.Conv2d(cin, cout, kernel_size=kernel_size, stride=stride, padding=kernel_size // 2, bias=False)),
            (f'{name}/norm', nn.BatchNorm2d(cout)),
            (f'{name}/relu', nn.ReLU(inplace=True))]


def _dw_conv_bn_relu(cin, cout, name, stride=1):
    """The reference's dw_conv3x3: a depthwise 3x3 (groups = out channels), a pointwise 1x1, one BatchNorm, ReLU."""
    return [(f'{name}/dw_conv3x3', nn.Conv2d(cin, cout, kernel_size=3, stride=stride, padding=1, groups=cout, bias=False)),
            (f'{name}/pw_conv1x1', nn.Conv2d(cin, cout, kernel_size=1, bias=False)),
            (f'{name}/pw_norm', nn.BatchNorm2d(cout)),
            (f'{name}/pw_relu', nn.ReLU(inplace=True))]


class Hsigmoid(nn.Module):
    """The hard sigmoid clamp(v + 3, 0, 6) / 6."""

    def forward(self, v):
        return torch.clamp(v + 3.0, min=0.0, max=6.0) / 6.0


class eSEModule(nn.Module):
    """Effective squeeze-excitation: x * hsigmoid(fc(mean over the pixels of x)), fc a 1x1 convolution C -> C with a bias (the only
    parameters, so the keys are `ese.fc.weight` / `ese.fc.bias`)."""

    def __init__(self, channels):
        super().__init__()
        self.fc = nn.Conv2d(channels, channels, 1)
        self.avg_pool, self.hsigmoid = nn.AdaptiveAvgPool2d(1), Hsigmoid()

    def forward(self, x):
        return x * self.hsigmoid(self.fc(self.avg_pool(x)))


class _KernelRoute(KernelRoute):
    """What the stem and the OSA module add to the skeleton: their BatchNorms decide what train mode is, and every kept value is a
    convolution's weight image or the folded constants of the BatchNorm behind it."""
    _kernels = ('VoVNet kernels fold the BatchNorms\' running statistics into the convolutions (so every BatchNorm must be frozen: '
                'eval() mode with running statistics, what norm_eval=True keeps in every config) and have no backward')

    def _init_route(self, torch_ops, limits, hip_train=False):
        KernelRoute._init_route(self, torch_ops, limits)
        self.hip_train = bool(hip_train)
        # what the route decision reads on every call, listed once: the subtree is built in __init__ and never altered
        self._norms = tuple(m for m in self.modules() if isinstance(m, _BatchNorm))

    def _in_train_mode(self):
        return any(m.training or m.running_mean is None for m in self._norms)

    def _image(self, key, conv):
        build = ops.conv3x3_image if conv.kernel_size == (3, 3) else ops.osa_concat_image
        return self._keep(('image', key), (conv.weight,), lambda: build(conv.weight.detach().float()))

    def _folded(self, key, bn):
        """(2, C): scale = gamma / sqrt(var + eps) and shift = beta - mean scale of an eval()-mode BatchNorm2d."""
        sources = (bn.running_var, bn.running_mean, bn.weight, bn.bias)
        return self._keep(('bn', key, float(bn.eps)), sources, lambda: Fn.folded_batchnorm(bn))

    def _conv3x3_hip(self, key, x, conv, bn):
        scale, shift = self._folded(key, bn)
        return ops.conv3x3_bn_relu(x, self._image(key, conv), conv.out_channels, scale, shift, stride=conv.stride[0])

    def _image_t(self, key, conv, bn):
        """The data gradient's image: (scale (x) weight) transposed, a 3x3's taps flipped."""
        build = ops.conv3x3_image_t if conv.kernel_size == (3, 3) else ops.osa_concat_image_t
        sources = (conv.weight, bn.running_var, bn.running_mean, bn.weight, bn.bias)
        return self._keep(('image_t', key, float(bn.eps)), sources, lambda: build(conv.weight.detach().float(), self._folded(key, bn)[0]))

    def _bn_stats(self, key, bn):
        """(3, C): scale (the folded one, bit for bit), rstd and mean of a frozen BatchNorm2d: what the parameter gradients read."""
        def build():
            rstd = torch.rsqrt(bn.running_var.detach().float() + bn.eps)
            return torch.stack((self._folded(key, bn)[0], rstd, bn.running_mean.detach().float())).contiguous()
        return self._keep(('bn_train', key, float(bn.eps)), (bn.running_var, bn.running_mean, bn.weight, bn.bias), build)

    def _has_train_route(self):
        return self.hip_train                   # (off: the refusals are what they were before the switch existed)

    def _refuse_train_route(self):
        if self._in_train_mode():
            raise _lib.Gd4dError(f'{self._route_name()} with hip_train=True and a BatchNorm that is not frozen: graph-detr4d_amd\'s HIP route '
                                 'trains behind frozen BatchNorms only (eval() mode with running statistics, what norm_eval=True keeps).  '
                                 '`torch_ops=True` (or GD4D_TORCH_OPS=1) runs the module\'s own torch layers, batch statistics included.')

    def _kept_values(self):
        for key, conv, bn in self._kernel_layers():
            self._image(key, conv)
            self._folded(key, bn)


def _channel_limits(name, cin, cout, k3=True):
    why = []
    lim_in, lim_out = (1024, 256) if k3 else (2304, 1024)
    if cin % 32 or not 32 <= cin <= lim_in:
        why.append(f'{name}: {cin} input channels (kernels: multiples of 32 in [32, {lim_in}])')
    if cout % 32 or not 32 <= cout <= lim_out:
        why.append(f'{name}: {cout} output channels (kernels: multiples of 32 in [32, {lim_out}])')
    return why


class _OsaTrainFunction(torch.autograd.Function):
    """One OSA module's kernel route as one autograd node: forward = `_OSA_module.forward_maps`, backward = the module docstring's
    steps.  tensors: the input, then `_train_tensors()` (they are inputs only so that autograd asks for their gradients).  With
    `with_cp` in train() mode the node keeps the input alone and runs the forward launches again in backward - the kernels are
    deterministic, the maps come back with the same bits; otherwise it keeps x_0 .. x_L, xt, the pool partials and the gate."""

    @staticmethod
    def forward(ctx, module, x, *params):
        maps, xt, partials, gate, out = module.forward_maps(x)
        ctx.module, ctx.x_dtype = module, x.dtype
        ctx.recompute = bool(module.with_cp and module.training)
        ctx.save_for_backward(*((maps[0],) if ctx.recompute else (*maps, xt, partials, gate)))
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        m = ctx.module
        if ctx.recompute:
            maps, xt, partials, gate, _ = m.forward_maps(ctx.saved_tensors[0])
        else:
            *maps, xt, partials, gate = ctx.saved_tensors
        *layers, (ckey, cconv, cbn) = m._kernel_layers()
        n_layers = len(layers)
        need_x, need = ctx.needs_input_grad[1], ctx.needs_input_grad[2:]
        want = lambda j: tuple(need[3 * j:3 * j + 3])                              # noqa: E731  (weight, gamma, beta) of convolution j
        grads = [None] * len(need)
        dout = f32(dout)
        w32 = lambda conv: conv.weight.detach().float().contiguous()               # noqa: E731
        # 1. eSE and the aggregation's activation
        dz, sums, grads[-2], grads[-1] = ops.ese_bwd(dout, xt, partials, gate, m.ese.fc.weight.detach(), want_fc=tuple(need[-2:]))
        # 4. (aggregation) its parameters
        if any(want(n_layers)):
            grads[3 * n_layers:3 * n_layers + 3] = ops.osa_concat_wgrad(dz, sums, maps, w32(cconv), m._bn_stats(ckey, cbn), want=want(n_layers))
        # the lowest map whose gradient anything asks for: 0 for the input's, i for layer i's parameters
        lowest = 0 if need_x else next((i for i in range(1, n_layers + 1) if any(want(i - 1))), None)
        dx = None
        if lowest is not None:
            # 2. the aggregation's data gradient, one map per source; the last one masked: dz_L
            g = ops.osa_concat_dgrad(dz, m._image_t(ckey, cconv, cbn), [t.shape[1] for t in maps], mask_last=maps[-1] if n_layers else None)
            # 3. the chain
            for i in range(n_layers, 0, -1):
                key, conv, bn = layers[i - 1]
                if any(want(i - 1)):
                    grads[3 * (i - 1):3 * i] = ops.conv3x3_wgrad(g[i], maps[i - 1], w32(conv), m._bn_stats(key, bn), want=want(i - 1))
                if i - 1 < lowest:
                    break
                first = i == 1
                ops.conv3x3_dgrad(g[i], m._image_t(key, conv, bn), conv.in_channels, add=g[i - 1], mask=None if first else maps[i - 1],
                                  add2=dout if first and m.identity else None, out=g[i - 1])
            if need_x:
                dx = (g[0] + dout if m.identity and not n_layers else g[0]).to(ctx.x_dtype)
        grads = [None if g_ is None else g_.to(t.dtype) for g_, t in zip(grads, m._train_tensors())]
        return (None, dx, *grads)


class _Stem(_KernelRoute, nn.Sequential):
    """`stem`: stem_1 (stride 2), stem_2, stem_3 (stride 2).  On the kernel route stem_1 runs on F.conv2d (3 input channels)."""

    def __init__(self, input_ch, stem_ch, depthwise, torch_ops, hip_train=False):
        conv_type = _dw_conv_bn_relu if depthwise else (lambda cin, cout, name, stride=1: _conv_bn_relu(cin, cout, name, 3, stride))
        layers = _conv_bn_relu(input_ch, stem_ch[0], 'stem_1', 3, 2)
        layers += conv_type(stem_ch[0], stem_ch[1], 'stem_2', 1)
        layers += conv_type(stem_ch[1], stem_ch[2], 'stem_3', 2)
        nn.Sequential.__init__(self, OrderedDict(layers))
        limits = ['depthwise stem (kernels: plain 3x3 convolutions)'] if depthwise else \
            _channel_limits('stem_2', stem_ch[0], stem_ch[1]) + _channel_limits('stem_3', stem_ch[1], stem_ch[2])
        self._init_route(torch_ops, limits, hip_train)

    def _kernel_layers(self):
        return [(i, getattr(self, f'stem_{i}/conv'), getattr(self, f'stem_{i}/norm')) for i in (1, 2, 3)]

    def _kept_values(self):
        (_, _, bn1), *rest = self._kernel_layers()
        self._folded(1, bn1)                    # (stem_1 runs on F.conv2d: no weight image)
        for key, conv, bn in rest:
            self._image(key, conv)
            self._folded(key, bn)

    def forward(self, x):
        if self._route(x) != 'infer':           # 'train': stem_1 and the stride-2 stem_3 have no HIP backward - the stem's own torch layers
            return nn.Sequential.forward(self, x)
        with torch.no_grad():
            (_, conv1, bn1), *rest = self._kernel_layers()
            scale, shift = self._folded(1, bn1)
            x = F.conv2d(f32(x), conv1.weight.detach().float(), None, conv1.stride, conv1.padding)
            x = x.mul_(scale.view(1, -1, 1, 1)).add_(shift.view(1, -1, 1, 1)).relu_()
            for key, conv, bn in rest:
                x = self._conv3x3_hip(key, x, conv, bn)
            return x


class _OSA_module(_KernelRoute, nn.Module):
    """One-shot aggregation: `layers` (a chain of 3x3 conv + BN + ReLU), `concat` (the 1x1 over the input and every layer's output),
    `ese`; `identity` adds the input (the modules of a stage after its first).  A depthwise module whose input is wider than its
    layers narrows it first (`conv_reduction`)."""

    def __init__(self, in_ch, stage_ch, concat_ch, num_layers, module_name, identity=False, depthwise=False, with_cp=False,
                 torch_ops=False, hip_train=False):
        nn.Module.__init__(self)
        self.module_name, self.identity, self.depthwise, self.with_cp = module_name, identity, depthwise, with_cp
        self.reduced = depthwise and in_ch != stage_ch
        if self.reduced:
            self.conv_reduction = nn.Sequential(OrderedDict(_conv_bn_relu(in_ch, stage_ch, f'{module_name}_reduction_0', 1)))
        widths = [stage_ch if depthwise else in_ch] + [stage_ch] * num_layers          # of the chain's maps
        make = _dw_conv_bn_relu if depthwise else (lambda cin, cout, name: _conv_bn_relu(cin, cout, name, 3))
        self.layers = nn.ModuleList(nn.Sequential(OrderedDict(make(widths[i], widths[i + 1], f'{module_name}_{i}')))
                                    for i in range(num_layers))
        k = in_ch + num_layers * stage_ch
        self.concat = nn.Sequential(OrderedDict(_conv_bn_relu(k, concat_ch, f'{module_name}_concat', 1)))
        self.ese = eSEModule(concat_ch)

        limits = ['depthwise layers (kernels: plain 3x3 convolutions)'] if depthwise else \
            [w for i in range(min(num_layers, 2)) for w in _channel_limits(f'{module_name}_{i}' + ('..' if i else ''), widths[i], stage_ch)]
        if num_layers + 1 > ops.OSA_MAX_SOURCES:
            limits.append(f'{num_layers} layers per module (kernels: up to {ops.OSA_MAX_SOURCES - 1})')
        limits += _channel_limits(f'{module_name}_concat', k, concat_ch, k3=False)
        self._init_route(torch_ops, limits, hip_train)

    def _kernel_layers(self):
        n = self.module_name
        layers = [(i, getattr(seq, f'{n}_{i}/conv'), getattr(seq, f'{n}_{i}/norm')) for i, seq in enumerate(self.layers)]
        return layers + [('concat', getattr(self.concat, f'{n}_concat/conv'), getattr(self.concat, f'{n}_concat/norm'))]

    def _torch(self, x):
        """The torch-op route: the chain, torch.cat, the aggregation, eSE, the residual."""
        maps = [x]
        y = self.conv_reduction(x) if self.reduced else x
        for layer in self.layers:
            y = layer(y)
            maps.append(y)
        out = self.ese(self.concat(torch.cat(maps, dim=1)))
        return out + x if self.identity else out

    def forward_maps(self, x, keep=True):
        """The kernel route's launches: (maps [x_0 .. x_L], xt, partials, gate, out).  keep=False: xt is overwritten by out (inference
        keeps nothing).  What the training node keeps or recomputes, and what its tests linearise the closed form at."""
        *layers, (ckey, cconv, cbn) = self._kernel_layers()
        maps = [f32(x)]
        for key, conv, bn in layers:
            maps.append(self._conv3x3_hip(key, maps[-1], conv, bn))
        scale, shift = self._folded(ckey, cbn)
        xt, partials = ops.osa_concat_conv(maps, self._image(ckey, cconv), cconv.out_channels, scale, shift)
        gate = ops.ese_gate(partials, xt.shape[2] * xt.shape[3], self.ese.fc.weight.detach(), self.ese.fc.bias.detach())
        out = ops.ese_apply(xt, gate, identity=maps[0] if self.identity else None, out=None if keep else xt)
        return maps, xt, partials, gate, out

    def _hip(self, x):
        return self.forward_maps(x, keep=False)[-1]

    def _train_tensors(self):
        """The node's parameter inputs: (weight, gamma, beta) per convolution, layers first, then the aggregation; then ese.fc's two."""
        return [t for _, conv, bn in self._kernel_layers() for t in (conv.weight, bn.weight, bn.bias)] + [self.ese.fc.weight, self.ese.fc.bias]

    def _kept_values(self):
        _KernelRoute._kept_values(self)
        if self.hip_train:
            for key, conv, bn in self._kernel_layers():
                self._image_t(key, conv, bn)
                self._bn_stats(key, bn)

    def forward(self, x):
        route = self._route(x)
        if route == 'torch':
            if self.with_cp and self.training:
                return cp.checkpoint(self._torch, x, use_reentrant=False)
            return self._torch(x)
        if route == 'train':
            return _OsaTrainFunction.apply(self, x, *self._train_tensors())
        with torch.no_grad():
            return self._hip(x)


class _OSA_stage(nn.Sequential):
    """`stage<n>`: `Pooling` (not in stage 2), then `OSA<n>_1` .. `OSA<n>_<blocks>`; every module but the first has the residual."""

    def __init__(self, stage_num, in_ch, stage_ch, concat_ch, blocks, num_layers, depthwise=False, with_cp=False, torch_ops=False,
                 hip_train=False):
        super().__init__()
        if stage_num != 2:
            self.add_module('Pooling', nn.MaxPool2d(kernel_size=3, stride=2, ceil_mode=True))
        for b in range(1, blocks + 1):
            name = f'OSA{stage_num}_{b}'
            self.add_module(name, _OSA_module(in_ch if b == 1 else concat_ch, stage_ch, concat_ch, num_layers, name, identity=b > 1,
                                              depthwise=depthwise, with_cp=with_cp, torch_ops=torch_ops, hip_train=hip_train))


@BACKBONES.register_module()
class VoVNet(nn.Module):
    """The reference's VoVNet: forward returns {feature name: map} for the names in `out_features` ('stem', 'stage2' .. 'stage5').
    `pretrained` / `init_cfg` are kept as attributes and not acted on: load the checkpoint slice with load_state_dict.
    `net.torch_ops` is the route switch of the whole network: setting it (or `with Fn.torch_ops_for(net):`) sets it on the stem and on
    every OSA module, which decide their route themselves (so a single stage can be switched too).  `net.hip_train` reaches them the same
    way: the opt-in training route of the module docstring."""
    _with_cp = False

    def __init__(self, spec_name, input_ch=3, out_features=None, frozen_stages=-1, norm_eval=True, pretrained=None, init_cfg=None,
                 torch_ops=False, hip_train=False):
        super().__init__()
        if spec_name not in _STAGE_SPECS:
            raise KeyError(f'{type(self).__name__}: spec_name={spec_name!r}; known: {sorted(_STAGE_SPECS)}')
        spec = _STAGE_SPECS[spec_name]
        self.spec_name, self.frozen_stages, self.norm_eval = spec_name, frozen_stages, norm_eval
        self._out_features = out_features
        if isinstance(pretrained, str):
            warnings.warn('VoVNet: `pretrained` is deprecated, use init_cfg=dict(type="Pretrained", checkpoint=...)', DeprecationWarning)
            init_cfg = dict(type='Pretrained', checkpoint=pretrained)
        self.init_cfg = init_cfg
        stem_ch, widths = spec['stem'], [spec['stem'][2]] + list(spec['stage_out_ch'])
        self.stem = _Stem(input_ch, stem_ch, spec['dw'], torch_ops, hip_train)
        self.stage_names = [f'stage{n}' for n in (2, 3, 4, 5)]
        for i, name in enumerate(self.stage_names):
            self.add_module(name, _OSA_stage(i + 2, widths[i], spec['stage_conv_ch'][i], widths[i + 1], spec['block_per_stage'][i],
                                             spec['layer_per_block'], spec['dw'], with_cp=self._with_cp, torch_ops=torch_ops,
                                             hip_train=hip_train))
        self._out_feature_channels = dict(zip(['stem'] + self.stage_names, widths))
        self._out_feature_strides = dict(zip(['stem'] + self.stage_names, (4, 4, 8, 16, 32)))
        self.torch_ops = torch_ops
        self.hip_train = hip_train
        # refused here, not at the first forward
        refuse_outside_limits(self, f'{type(self).__name__}({spec_name!r})', [w for m in self._routed() for w in m._kernel_limits])

    def _routed(self):
        return [m for m in self.modules() if isinstance(m, _KernelRoute)]

    @property
    def torch_ops(self):
        return self._torch_ops

    @torch_ops.setter
    def torch_ops(self, value):
        self._torch_ops = bool(value)
        for m in self._routed():
            m.torch_ops = self._torch_ops

    @property
    def hip_train(self):
        return self._hip_train

    @hip_train.setter
    def hip_train(self, value):
        self._hip_train = bool(value)
        for m in self._routed():
            m.hip_train = self._hip_train

    def refresh_images(self):
        """Rebuild every changed weight image and folded BatchNorm into the buffers a captured graph reads (see the module docstring)."""
        for m in self._routed():
            m.refresh_images()

    def _features(self, x):
        x = self.stem(x)
        if 'stem' in self._out_features:
            yield 'stem', x
        for name in self.stage_names:
            x = getattr(self, name)(x)
            if name in self._out_features:
                yield name, x

    def forward(self, x):
        return dict(self._features(x))

    def _freeze_stages(self):
        """frozen_stages = k >= 0 freezes the stem and stages 2 .. k + 1: eval() mode, no gradients."""
        frozen = ['stem'] + self.stage_names[:self.frozen_stages] if self.frozen_stages >= 0 else []
        for name in frozen:
            getattr(self, name).eval().requires_grad_(False)

    def train(self, mode=True):
        """Training mode with the frozen stages and (norm_eval) every BatchNorm kept in eval() mode."""
        super().train(mode)
        self._freeze_stages()
        if mode and self.norm_eval:
            for m in self.modules():
                if isinstance(m, _BatchNorm):
                    m.eval()
        return self


@BACKBONES.register_module()
class VoVNetCP(VoVNet):
    """The reference's VoVNetCP: forward returns the list of the `out_features` maps in network order; on the torch-op route each
    OSA module runs under torch.utils.checkpoint in train() mode unless with_cp=False; on the kernel route inference ignores it, and the
    hip_train node recomputes its forward maps in backward instead of keeping them."""

    def __init__(self, *args, with_cp=True, **kwargs):
        self._with_cp = bool(with_cp)
        super().__init__(*args, **kwargs)

    def forward(self, x):
        return [m for _, m in self._features(x)]
