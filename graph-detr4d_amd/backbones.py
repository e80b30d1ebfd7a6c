"""The image backbone the configs build: mmdet's `ResNet` (depth 18 / 34 of BasicBlocks, 50 / 101 of Bottlenecks, style='pytorch'),
in the DCN configurations with stages 3 and 4 replacing the 3x3 convolution of every bottleneck with DCNv2 -
    img_backbone=dict(type='ResNet', depth=50, num_stages=4, out_indices=(0, 1, 2, 3), frozen_stages=1,
                      norm_cfg=dict(type='BN', requires_grad=False), norm_eval=True, style='pytorch',
                      dcn=dict(type='DCNv2', deform_groups=1, fallback_on_stride=False), stage_with_dcn=(False, False, True, True))
- with mmdet's state-dict keys (`conv1.weight`, `bn1.*`, `layer3.0.conv2.conv_offset.weight`, `layer1.0.downsample.0.weight`, ...), so a
trained checkpoint's backbone slice loads with strict=True.

By default every layer is stock torch except the DCN conv2 (dcn.ModulatedDeformConv2dPack, the library's kernels).  With its BatchNorm in eval
mode - every config: norm_eval=True - a DCN bottleneck computes relu(bn2(conv2(x))) in ONE call, `conv2.forward_bn_relu(x, bn2)`: the
BatchNorm and the ReLU run in the deformable convolution's epilogue.  `torch_ops=True` is handed to the DCN layers (their
differentiable grid_sample route), and so is `hip_train=True`: the same one call then trains on the library's own backward kernels
(dcn.py), with no grid_sample and no tensor of 9 Cin x pixels.

`plain_kernels=True` (opt-in; `ResNet`, `Bottleneck`, `BasicBlock`) runs the blocks' plain convolutions on the library's kernels too
(gd4d_resnet.hip), each with its frozen BatchNorm folded into the epilogue.  A block is then a kernel_route.KernelRoute module, and its
route 'infer' is
    Bottleneck   conv1 -> relu(bn1);  conv2 -> relu(bn2) (the plain 3x3 with the block's stride, or the DCN's forward_bn_relu as before);
                 downsample -> bn, no ReLU (a stage's first block);  conv3 -> relu(bn3 + identity): 3 launches, 4 with a downsample
    BasicBlock   conv1 (3x3, the stride) -> relu(bn1);  downsample -> bn;  conv2 (3x3) -> relu(bn2 + identity): 2 launches, 3 with one
with no separate BatchNorm, ReLU or add pass.  Weight images and the folded (scale, shift) are kept at fixed addresses (`_keep`), so a
forward is capturable in a hipGraph after one eager call and `refresh_images()` serves in-place parameter edits, as for VoVNet.  The
kernels take channels that are multiples of 32 (1x1: K up to 2304, Cout up to 2048; 3x3: Cin up to 1024, Cout up to 512), stride 1 or
2, dilation 1 and frozen BatchNorms; anything else is refused at construction or at the call, naming `torch_ops=True`.  Without
`plain_train` they run no backward: `plain_kernels=True` with `hip_train=True` alone is refused, and autograd on trainable parameters
raises.  `torch_ops=True`, `with Fn.torch_ops_for(net):` or GD4D_TORCH_OPS=1 choose the block's own torch layers.  The 7x7 stem (3
input channels) and the max-pooling stay on torch on every route.

`plain_train=True` (opt-in; `ResNet`, `Bottleneck`, `BasicBlock`; needs `plain_kernels=True`, and in a block with DCN `hip_train=True`
too - the DCN layer keeps its own training route and keyword) adds the training route of kernel_route's rule, steps 3 and 4, on
gd4d_resnet_train.hip.  A plain block (a Bottleneck without DCN, a BasicBlock) is ONE autograd node, `_BlockTrainFunction`: forward =
the inference launches above with the same bits, keeping the input, each unit's output and the block output; backward, given dout,
with s the folded scale of a unit's BatchNorm:
    g3 = dout [out > 0]                         the block's one elementwise pass (dout arrives unmasked: its consumers sum into it)
    per unit, from the top: (dW, dgamma, dbeta) from (g, the unit's input) - one weight-gradient GEMM and its finishing kernel - then
    g = conv^T(g; s W) [input > 0], the mask in the data gradient's epilogue; at conv1  dx = conv^T(g1) + r  in the same epilogue,
    r = g3 (no downsample), downsample^T(g3) (stride 1), or downsample^T(g3) on the half-resolution grid, added at the even pixels
    only (stride 2: no zero-filled map is written)
A DCN bottleneck is two nodes around the DCN layer's own: `_HeadTrainFunction` (conv1, bn1, ReLU; its backward masks the DCN node's
unmasked gradient first) and `_TailTrainFunction` (conv3, downsample, the residual, ReLU), which returns the gradients of a2 and of
the block input; autograd adds the head's and the tail's input gradients - one torch add per DCN block - and a stride-2 downsample's
share is scattered to a full-resolution map for it (ops.even_pixels_scatter: two blocks of a ResNet-50).  All three nodes share
`_unit_bwd`.  Gradients only where needs_input_grad asks, no data gradient below the lowest unit that needs one, dx in the input's
dtype.  Every BatchNorm must be frozen (train() mode with an unfrozen one raises, naming `torch_ops=True`); affine BatchNorm
parameters that require grad get dgamma / dbeta from the finishing kernel (not bn2 of a DCN block: the DCN layer refuses that).  A
block whose parameters are frozen behind an input that needs no gradient takes the inference launches and builds no node: layer1
under frozen_stages=1.  The stem and the max-pooling stay on torch autograd; `with_cp`, deep_stem, avg_down, plugins and dilation
other than 1 stay refused.  Module tree and state-dict keys are untouched.  Measured (docs/measurements_r44.md): level with the stock
layers at 24 cameras, slower at 6.

Scope: depth 18 / 34 / 50 / 101, style 'pytorch', the plain 7x7 stem, BatchNorm, `fallback_on_stride=False`; `num_stages`, `out_indices`,
`strides`, `dilations`, `frozen_stages`, `norm_eval`, `dcn`, `stage_with_dcn`, `zero_init_residual`.  deep_stem, avg_down, plugins, other
norms and `with_cp` are refused: nothing shipped uses them.

The VoVNet configurations' backbone, `VoVNet` / `VoVNetCP`, is in vovnet.py and re-exported here.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, ops
from . import functional as Fn
from .kernel_route import KernelRoute, f32, refuse_outside_limits
from .registry import BACKBONES, build_conv_layer
from .vovnet import VoVNet, VoVNetCP  # noqa: F401  (the VoVNet configurations' backbone: vovnet.py)


def _norm(norm_cfg, channels):
    cfg = dict(norm_cfg or dict(type='BN'))
    if cfg.pop('type', 'BN') not in ('BN', 'BN2d'):
        raise _lib.Gd4dError(f'ResNet: norm_cfg={norm_cfg}; this backbone builds BatchNorm2d layers (what every shipped config uses)')
    requires_grad = cfg.pop('requires_grad', True)
    bn = nn.BatchNorm2d(channels, **cfg)
    for p in bn.parameters():
        p.requires_grad = requires_grad
    return bn


class _PlainKernels(KernelRoute):
    """What `plain_kernels=True` adds to a block: the route rule (kernel_route.py) in front of its forward, its convolutions' weight
    images and folded BatchNorms as kept values.  A block supplies `_plain_layers()`, `_torch(x)` and `_hip(x)`.  With
    `plain_kernels=False` none of this is consulted: forward is `_torch`, stock layers (and the DCN conv2's own route)."""
    _kernels = ('ResNet kernels fold the BatchNorms\' running statistics into the convolutions (so every BatchNorm of the block must be '
                'frozen: eval() mode with running statistics, what norm_eval=True keeps in every config) and have no backward')
    plain_kernels = plain_train = False

    def _init_plain(self, plain_kernels, torch_ops, hip_train, plain_train=False):
        self.plain_kernels, self.plain_train = bool(plain_kernels), bool(plain_train)
        name = type(self).__name__
        if self.plain_train and not self.plain_kernels:
            raise _lib.Gd4dError(f'{name}: plain_train=True without plain_kernels=True - plain_train is the training route of the plain '
                                 'convolutions\' kernels, which plain_kernels=True chooses.  Pass both, or `torch_ops=True` for training by '
                                 'autograd on the stock layers.')
        if not self.plain_kernels:
            return
        if self.plain_train and getattr(self, 'with_dcn', False) and not hip_train:
            raise _lib.Gd4dError(f'{name}: plain_train=True on a block with DCN needs hip_train=True too - the DCN layer keeps its own '
                                 'training route and keyword, and without it has no backward on the kernels.  Pass hip_train=True, or '
                                 '`torch_ops=True` for training by autograd.')
        if hip_train and not self.plain_train:
            raise _lib.Gd4dError(f'{name}: plain_kernels=True with hip_train=True - without plain_train=True the plain convolutions\' '
                                 'kernels run no backward (hip_train trains the DCN layers behind stock torch layers).  Add '
                                 'plain_train=True, choose one of the two, or `torch_ops=True` for training by autograd.')
        self._norms = tuple(m for m in self.modules() if isinstance(m, nn.BatchNorm2d))
        self._init_route(torch_ops, self._plain_limits())
        if self.plain_train:
            self.hip_train = True               # the attribute kernel_route's rule looks for (steps 3 and 4); absent without the keyword

    # `blk.torch_ops = True` / `with Fn.torch_ops_for(blk):` reach the DCN conv2 too, which decides its own route
    @property
    def torch_ops(self):
        return self.__dict__.get('_torch_ops', False)

    @torch_ops.setter
    def torch_ops(self, value):
        self.__dict__['_torch_ops'] = bool(value)
        conv2 = self.__dict__.get('_modules', {}).get('conv2')
        if self.plain_kernels and isinstance(conv2, KernelRoute):
            conv2.torch_ops = bool(value)

    def _plain_layers(self):
        """[(key, conv, bn)] of the plain convolutions the kernels run, in launch order."""
        raise NotImplementedError

    def _plain_limits(self):
        why = []
        for key, conv, _ in self._plain_layers():
            k3 = conv.kernel_size == (3, 3)
            lim_in, lim_out = (1024, 512) if k3 else (2304, 2048)
            for what, c, lim in (('input', conv.in_channels, lim_in), ('output', conv.out_channels, lim_out)):
                if c % 32 or not 32 <= c <= lim:
                    why.append(f'{key}: {c} {what} channels (kernels: multiples of 32 in [32, {lim}])')
            if conv.stride not in ((1, 1), (2, 2)):
                why.append(f'{key}: stride={conv.stride} (kernels: 1 or 2)')
            if k3 and (conv.dilation != (1, 1) or conv.padding != (1, 1)):
                why.append(f'{key}: dilation={conv.dilation}, padding={conv.padding} (kernels: 1)')
        conv2 = getattr(self, 'conv2', None)
        if isinstance(conv2, KernelRoute):
            why += [f'conv2 (DCN): {w}' for w in conv2._kernel_limits]
        return why

    def _route_name(self):
        return f'{type(self).__name__}({self.inplanes}, {self.planes})'

    def _in_train_mode(self):
        return any(m.training or m.running_mean is None for m in self._norms)

    def _image(self, key, conv):
        build = ops.conv3x3_act_image if conv.kernel_size == (3, 3) else ops.conv1x1_image
        return self._keep(('image', key), (conv.weight,), lambda: build(conv.weight.detach().float()))

    def _folded(self, key, bn):
        """(2, C): scale = gamma / sqrt(var + eps) and shift = beta - mean scale of an eval()-mode BatchNorm2d."""
        sources = (bn.running_var, bn.running_mean, bn.weight, bn.bias)
        return self._keep(('bn', key, float(bn.eps)), sources, lambda: Fn.folded_batchnorm(bn))

    def _conv(self, key, x, conv, bn, identity=None, relu=True):
        """act(bn(conv(x)) (+ identity)) in one launch."""
        scale, shift = self._folded(key, bn)
        run = ops.conv3x3_bn_act if conv.kernel_size == (3, 3) else ops.conv1x1_bn_act
        return run(x, self._image(key, conv), conv.out_channels, scale, shift, stride=conv.stride[0], identity=identity, relu=relu)

    def _kept_values(self):
        for key, conv, bn in self._plain_layers():
            self._image(key, conv)
            self._folded(key, bn)
            if self.plain_train:
                self._image_t(key, conv, bn)
                self._bn_stats(key, bn)
        conv2 = getattr(self, 'conv2', None)
        if isinstance(conv2, KernelRoute):
            conv2._bns[id(self.bn2)] = self.bn2
            conv2._kept_values()

    # ---- the training route (plain_train=True) ---------------------------------------------------------------------------------
    def _refuse_train_route(self):
        if self._in_train_mode():
            raise _lib.Gd4dError(f'{self._route_name()} with plain_train=True and a BatchNorm that is not frozen: graph-detr4d_amd\'s HIP '
                                 'route trains behind frozen BatchNorms only (eval() mode with running statistics, what norm_eval=True '
                                 'keeps).  `torch_ops=True` (or GD4D_TORCH_OPS=1) runs the block\'s own torch layers, batch statistics '
                                 'included.')

    def _image_t(self, key, conv, bn):
        """The data gradient's image: (scale (x) weight) transposed, a 3x3's taps flipped."""
        build = ops.conv3x3_act_image_t if conv.kernel_size == (3, 3) else ops.conv1x1_image_t
        sources = (conv.weight, bn.running_var, bn.running_mean, bn.weight, bn.bias)
        return self._keep(('image_t', key, float(bn.eps)), sources, lambda: build(conv.weight.detach().float(), self._folded(key, bn)[0]))

    def _bn_stats(self, key, bn):
        """(3, C): scale (the folded one, bit for bit), rstd and mean of a frozen BatchNorm2d: what the parameter gradients read."""
        def build():
            rstd = torch.rsqrt(bn.running_var.detach().float() + bn.eps)
            return torch.stack((self._folded(key, bn)[0], rstd, bn.running_mean.detach().float())).contiguous()
        return self._keep(('bn_train', key, float(bn.eps)), (bn.running_var, bn.running_mean, bn.weight, bn.bias), build)

    def _unit_bwd(self, unit, g, x_in, want, need_dx, **epilogue):
        """One unit's backward, what the plain block's node and the DCN block's head and tail nodes share.  unit = (key, conv, bn); g:
        the gradient of the BatchNorm's output after the ReLU's mask; x_in: the convolution's input.  Returns (dx or None, (dW, dgamma,
        dbeta)): the parameter gradients `want` asks for in one weight-gradient launch and its finish, and with need_dx
        dx = (conv^T(g; scale (x) weight) (+ add)) ([mask > 0]) (+ add2) (+ add_even), the epilogue's operands being the keywords."""
        key, conv, bn = unit
        k3, stride = conv.kernel_size == (3, 3), conv.stride[0]
        grads = (None, None, None)
        if any(want):
            wgrad = ops.conv3x3_act_wgrad if k3 else ops.conv1x1_wgrad
            grads = wgrad(g, x_in, conv.weight.detach().float().contiguous(), self._bn_stats(key, bn), stride=stride, want=tuple(want))
        dx = None
        if need_dx:
            image_t = self._image_t(key, conv, bn)
            if k3:
                dx = ops.conv3x3_act_dgrad(g, image_t, conv.in_channels, hw=x_in.shape[2:], stride=stride, **epilogue)
            elif stride == 1:
                dx = ops.conv1x1_dgrad(g, image_t, conv.in_channels, **epilogue)
            else:       # a stride-2 downsample: its adjoint on the half-resolution grid; the caller adds it at the even pixels
                assert not epilogue
                dx = ops.conv1x1_dgrad(g, image_t, conv.in_channels)
        return dx, grads

    def _residual_bwd(self, g3, x, want_ds, need_x):
        """The residual path's share of the block input's gradient as the epilogue keyword of the lowest unit's data gradient -
        {add2: g3} without a downsample, {add: r} with one of stride 1, {add_even: r} (half resolution) with one of stride 2,
        r = downsample^T(g3) - and the downsample's parameter gradients."""
        if self.downsample is None:
            return ({'add2': g3} if need_x else {}), (None, None, None)
        unit = ('downsample', self.downsample[0], self.downsample[1])
        r, grads = self._unit_bwd(unit, g3, x, want_ds, need_x)
        if not need_x:
            return {}, grads
        return ({'add': r} if unit[1].stride[0] == 1 else {'add_even': r}), grads

    def _train_units(self):
        """The units of the node(s), in the order of their parameter inputs."""
        return self._plain_layers()

    def _train_tensors(self):
        """The node's parameter inputs: (weight, gamma, beta) per unit of `_train_units()` (inputs only so that autograd asks for
        their gradients)."""
        return [t for _, conv, bn in self._train_units() for t in (conv.weight, bn.weight, bn.bias)]

    def forward(self, x):
        if not self.plain_kernels:
            return self._torch(x)
        route = self._route(x)
        if route == 'torch':
            return self._torch(x)
        if route == 'train':        # (a frozen block behind an input that needs no gradient answers 'infer': no node is built)
            return self._hip_train(x)
        with torch.no_grad():
            return self._hip(f32(x))


def _cast_grads(grads, tensors):
    return [None if g is None else g.to(t.dtype) for g, t in zip(grads, tensors)]


class _BlockTrainFunction(torch.autograd.Function):
    """A plain block (a Bottleneck without DCN, a BasicBlock) on the kernel route as ONE autograd node.  forward = the block's inference
    launches, `forward_maps`, with the same bits; the node keeps the block input, each unit's output and the block output.  backward,
    given dout (unmasked: the next block and the neck sum into it), with `chain` the units from conv1 up:
        g = dout [out > 0]                                      the block's one elementwise pass
        for the units from the top down: its parameter gradients from (g, the unit's input); then g = conv^T(g) [input > 0], the mask
            in the data gradient's epilogue - and at conv1  dx = conv^T(g) + r, r the residual path's gradient in the same epilogue
            (`_residual_bwd`): no pass of its own for a BatchNorm scale, an inner mask or either sum into dx.
    Gradients only where needs_input_grad asks; the data gradients stop at the lowest unit whose parameters (or the input) need one."""

    @staticmethod
    def forward(ctx, blk, x, *params):
        maps = blk.forward_maps(x)
        ctx.blk, ctx.x_dtype = blk, x.dtype
        ctx.save_for_backward(*maps)
        return maps[-1]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        blk = ctx.blk
        *inputs, out = ctx.saved_tensors                        # x, a1 (, a2): each chain unit's input
        units = blk._train_units()
        chain = [u for u in units if u[0] != 'downsample']
        need_x, need = ctx.needs_input_grad[1], ctx.needs_input_grad[2:]
        want = {u[0]: tuple(need[3 * j:3 * j + 3]) for j, u in enumerate(units)}
        got = {}
        g = g3 = ops.relu_mask_bwd(f32(dout), out)
        # the lowest chain unit a data gradient must reach: 0 with the input's, else the lowest one with a parameter that asks
        lowest = 0 if need_x else next((i for i, u in enumerate(chain) if any(want[u[0]])), len(chain))
        residual, got['downsample'] = blk._residual_bwd(g3, inputs[0], want.get('downsample', (False,) * 3), need_x)
        dx = None
        for i in range(len(chain) - 1, lowest - 1, -1):
            epilogue = {'mask': inputs[i]} if i else residual
            below, got[chain[i][0]] = blk._unit_bwd(chain[i], g, inputs[i], want[chain[i][0]], i > lowest or need_x, **epilogue)
            if i:
                g = below
            else:
                dx = below
        grads = [t for u in units for t in got.get(u[0], (None, None, None))]
        return (None, None if dx is None else dx.to(ctx.x_dtype), *_cast_grads(grads, blk._train_tensors()))


class _HeadTrainFunction(torch.autograd.Function):
    """The head node of a DCN bottleneck: a1 = relu(bn1(conv1(x))).  backward: g1 = da1 [a1 > 0] (the DCN layer's node returns da1
    unmasked), then conv1's unit backward."""

    @staticmethod
    def forward(ctx, blk, x, *params):
        x32 = f32(x)
        a1 = blk._conv('conv1', x32, blk.conv1, blk.bn1)
        ctx.blk, ctx.x_dtype = blk, x.dtype
        ctx.save_for_backward(x32, a1)
        return a1

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, da1):
        blk = ctx.blk
        x32, a1 = ctx.saved_tensors
        g1 = ops.relu_mask_bwd(f32(da1), a1)
        dx, grads = blk._unit_bwd(('conv1', blk.conv1, blk.bn1), g1, x32, ctx.needs_input_grad[2:5], ctx.needs_input_grad[1])
        return (None, None if dx is None else dx.to(ctx.x_dtype), *_cast_grads(grads, (blk.conv1.weight, blk.bn1.weight, blk.bn1.bias)))


class _TailTrainFunction(torch.autograd.Function):
    """The tail node of a DCN bottleneck: out = relu(bn3(conv3(a2)) + identity), identity = x or bn(downsample(x)).  backward returns the
    gradients of a2 (unmasked: a2's ReLU is the DCN layer's node's) and of the block input (the residual path's: g3, or downsample^T(g3),
    a stride-2 one scattered to the even pixels of a full-resolution map, which autograd's add needs)."""

    @staticmethod
    def forward(ctx, blk, a2, x, *params):
        x32, a2 = f32(x), f32(a2)
        identity = x32 if blk.downsample is None else blk._conv('downsample', x32, *blk.downsample, relu=False)
        out = blk._conv('conv3', a2, blk.conv3, blk.bn3, identity=identity)
        ctx.blk, ctx.dtypes = blk, (a2.dtype, x.dtype)
        ctx.save_for_backward(a2, x32, out)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        blk = ctx.blk
        a2, x32, out = ctx.saved_tensors
        units = blk._tail_units()
        need_a2, need_x, need = ctx.needs_input_grad[1], ctx.needs_input_grad[2], ctx.needs_input_grad[3:]
        want = {u[0]: tuple(need[3 * j:3 * j + 3]) for j, u in enumerate(units)}
        got = {}
        g3 = ops.relu_mask_bwd(f32(dout), out)
        da2, got['conv3'] = blk._unit_bwd(('conv3', blk.conv3, blk.bn3), g3, a2, want['conv3'], need_a2)
        residual, got['downsample'] = blk._residual_bwd(g3, x32, want.get('downsample', (False,) * 3), need_x)
        dx = None
        if need_x:
            (kind, r), = residual.items()
            dx = ops.even_pixels_scatter(r, x32.shape[2:]) if kind == 'add_even' else r
        grads = [t for u in units for t in got.get(u[0], (None, None, None))]
        tensors = [t for _, conv, bn in units for t in (conv.weight, bn.weight, bn.bias)]
        return (None, None if da2 is None else da2.to(ctx.dtypes[0]), None if dx is None else dx.to(ctx.dtypes[1]),
                *_cast_grads(grads, tensors))


class Bottleneck(_PlainKernels, nn.Module):
    """mmdet.models.backbones.resnet.Bottleneck, style 'pytorch' (the stride sits on the 3x3 convolution)."""
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, dilation=1, downsample=None, norm_cfg=None, dcn=None, torch_ops=False,
                 hip_train=False, plain_kernels=False, plain_train=False):
        super().__init__()
        self.inplanes, self.planes, self.stride, self.dilation = inplanes, planes, stride, dilation
        self.with_dcn = dcn is not None
        self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=1, stride=1, bias=False)
        self.bn1 = _norm(norm_cfg, planes)
        if self.with_dcn:
            dcn = dict(dcn)
            if dcn.pop('fallback_on_stride', False):
                raise _lib.Gd4dError('Bottleneck: dcn fallback_on_stride=True is not built (every shipped config sets False)')
            self.conv2 = build_conv_layer(dcn, planes, planes, kernel_size=3, stride=stride, padding=dilation, dilation=dilation,
                                          bias=False, torch_ops=torch_ops, hip_train=hip_train)
        else:
            self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, stride=stride, padding=dilation, dilation=dilation, bias=False)
        self.bn2 = _norm(norm_cfg, planes)
        self.conv3 = nn.Conv2d(planes, planes * self.expansion, kernel_size=1, bias=False)
        self.bn3 = _norm(norm_cfg, planes * self.expansion)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self._init_plain(plain_kernels, torch_ops, hip_train, plain_train)

    def _plain_layers(self):
        layers = [('conv1', self.conv1, self.bn1)] + ([] if self.with_dcn else [('conv2', self.conv2, self.bn2)])
        if self.downsample is not None:
            layers.append(('downsample', self.downsample[0], self.downsample[1]))
        return layers + [('conv3', self.conv3, self.bn3)]

    def _hip(self, x):
        out = self._conv('conv1', x, self.conv1, self.bn1)
        out = self.conv2.forward_bn_relu(out, self.bn2) if self.with_dcn else self._conv('conv2', out, self.conv2, self.bn2)
        identity = x if self.downsample is None else self._conv('downsample', x, *self.downsample, relu=False)
        return self._conv('conv3', out, self.conv3, self.bn3, identity=identity)

    def forward_maps(self, x):
        """The plain block's inference launches, keeping what the training node keeps: (x, a1, a2, out)."""
        x = f32(x)
        a1 = self._conv('conv1', x, self.conv1, self.bn1)
        a2 = self._conv('conv2', a1, self.conv2, self.bn2)
        identity = x if self.downsample is None else self._conv('downsample', x, *self.downsample, relu=False)
        return x, a1, a2, self._conv('conv3', a2, self.conv3, self.bn3, identity=identity)

    def _tail_units(self):
        down = [] if self.downsample is None else [('downsample', self.downsample[0], self.downsample[1])]
        return down + [('conv3', self.conv3, self.bn3)]

    def _hip_train(self, x):
        """One node for a plain block.  With DCN, two nodes around the DCN layer's own (dcn.py, hip_train=True): head (conv1, bn1,
        ReLU) and tail (conv3, downsample, residual, ReLU); autograd adds the head's and the tail's gradients of the block input -
        one torch add per DCN block, the only one."""
        if not self.with_dcn:
            return _BlockTrainFunction.apply(self, x, *self._train_tensors())
        a1 = _HeadTrainFunction.apply(self, x, self.conv1.weight, self.bn1.weight, self.bn1.bias)
        a2 = self.conv2.forward_bn_relu(a1, self.bn2)
        tail = [t for _, conv, bn in self._tail_units() for t in (conv.weight, bn.weight, bn.bias)]
        return _TailTrainFunction.apply(self, a2, x, *tail)

    def _torch(self, x):
        out = self.relu(self.bn1(self.conv1(x)))
        if self.with_dcn and not self.bn2.training:
            out = self.conv2.forward_bn_relu(out, self.bn2)       # BatchNorm and ReLU in the deformable convolution's epilogue
        else:
            out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        identity = x if self.downsample is None else self.downsample(x)
        return F.relu(out + identity)


class BasicBlock(_PlainKernels, nn.Module):
    """mmdet.models.backbones.resnet.BasicBlock: conv1 3x3 with the stride, bn1, ReLU, conv2 3x3, bn2, the residual, ReLU."""
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, dilation=1, downsample=None, norm_cfg=None, dcn=None, torch_ops=False,
                 hip_train=False, plain_kernels=False, plain_train=False):
        super().__init__()
        if dcn is not None:
            raise _lib.Gd4dError('BasicBlock: dcn is not built for the basic block (mmdet asserts the same; depths 50 / 101 take it) - on '
                                 'no route: `torch_ops=True` does not serve it either')
        self.inplanes, self.planes, self.stride, self.dilation = inplanes, planes, stride, dilation
        self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=3, stride=stride, padding=dilation, dilation=dilation, bias=False)
        self.bn1 = _norm(norm_cfg, planes)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, padding=1, bias=False)
        self.bn2 = _norm(norm_cfg, planes)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self._init_plain(plain_kernels, torch_ops, hip_train, plain_train)

    def _plain_layers(self):
        down = [] if self.downsample is None else [('downsample', self.downsample[0], self.downsample[1])]
        return [('conv1', self.conv1, self.bn1)] + down + [('conv2', self.conv2, self.bn2)]

    def _hip(self, x):
        out = self._conv('conv1', x, self.conv1, self.bn1)
        identity = x if self.downsample is None else self._conv('downsample', x, *self.downsample, relu=False)
        return self._conv('conv2', out, self.conv2, self.bn2, identity=identity)

    def forward_maps(self, x):
        """The block's inference launches, keeping what the training node keeps: (x, a1, out)."""
        x = f32(x)
        a1 = self._conv('conv1', x, self.conv1, self.bn1)
        identity = x if self.downsample is None else self._conv('downsample', x, *self.downsample, relu=False)
        return x, a1, self._conv('conv2', a1, self.conv2, self.bn2, identity=identity)

    def _hip_train(self, x):
        return _BlockTrainFunction.apply(self, x, *self._train_tensors())

    def _torch(self, x):
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        identity = x if self.downsample is None else self.downsample(x)
        return F.relu(out + identity)


@BACKBONES.register_module()
class ResNet(nn.Module):
    """mmdet.models.backbones.ResNet for depth 18 / 34 (BasicBlock) and 50 / 101 (Bottleneck).  `net.torch_ops` (or `with
    Fn.torch_ops_for(net):`) is the route switch of every `plain_kernels=True` block, which decide their route themselves."""
    arch_settings = {18: (BasicBlock, (2, 2, 2, 2)), 34: (BasicBlock, (3, 4, 6, 3)), 50: (Bottleneck, (3, 4, 6, 3)),
                     101: (Bottleneck, (3, 4, 23, 3))}

    def __init__(self, depth, in_channels=3, stem_channels=None, base_channels=64, num_stages=4, strides=(1, 2, 2, 2),
                 dilations=(1, 1, 1, 1), out_indices=(0, 1, 2, 3), style='pytorch', deep_stem=False, avg_down=False, frozen_stages=-1,
                 conv_cfg=None, norm_cfg=dict(type='BN', requires_grad=True), norm_eval=True, dcn=None,
                 stage_with_dcn=(False, False, False, False), plugins=None, with_cp=False, zero_init_residual=True, pretrained=None,
                 init_cfg=None, torch_ops=False, hip_train=False, plain_kernels=False, plain_train=False):
        super().__init__()
        if depth not in self.arch_settings:
            raise _lib.Gd4dError(f'ResNet: depth={depth}; this backbone builds the depths {sorted(self.arch_settings)}')
        refused = [k for k, v in (('deep_stem', deep_stem), ('avg_down', avg_down), ('conv_cfg', conv_cfg), ('plugins', plugins),
                                  ('with_cp', with_cp)) if v]
        if style != 'pytorch':
            refused.append(f'style={style!r}')
        if refused:
            raise _lib.Gd4dError(f'ResNet: {", ".join(refused)} - not built here (see the module docstring for the scope)')
        assert 1 <= num_stages <= 4 and len(strides) == len(dilations) == num_stages and max(out_indices) < num_stages
        block, stage_blocks = self.arch_settings[depth]
        if dcn is not None:
            assert len(stage_with_dcn) == num_stages
            if block is BasicBlock and any(stage_with_dcn):
                raise _lib.Gd4dError(f'ResNet: dcn with depth={depth} - not built for the basic block (mmdet asserts the same; depths 50 / '
                                     '101 take it), on no route: `torch_ops=True` does not serve it either')
        if plain_train and not plain_kernels:
            raise _lib.Gd4dError('ResNet: plain_train=True without plain_kernels=True - plain_train is the training route of the plain '
                                 'convolutions\' kernels, which plain_kernels=True chooses.  Pass both, or `torch_ops=True` for training by '
                                 'autograd on the stock layers.')
        if plain_kernels and hip_train and not plain_train:
            raise _lib.Gd4dError('ResNet: plain_kernels=True with hip_train=True - without plain_train=True the plain convolutions\' '
                                 'kernels run no backward (hip_train trains the DCN layers behind stock torch layers).  Add '
                                 'plain_train=True, choose one of the two, or `torch_ops=True` for training by autograd.')
        self.block, self.plain_kernels, self.plain_train = block, bool(plain_kernels), bool(plain_train)
        self.depth, self.num_stages, self.out_indices = depth, num_stages, tuple(out_indices)
        self.frozen_stages, self.norm_eval, self.zero_init_residual = frozen_stages, norm_eval, zero_init_residual
        stem_channels = stem_channels or base_channels
        self.conv1 = nn.Conv2d(in_channels, stem_channels, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = _norm(norm_cfg, stem_channels)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.res_layers = []
        inplanes = stem_channels
        for i, blocks in enumerate(stage_blocks[:num_stages]):
            planes = base_channels * 2 ** i
            stage_dcn = dcn if dcn is not None and stage_with_dcn[i] else None
            layer = self._make_stage(inplanes, planes, blocks, strides[i], dilations[i], norm_cfg, stage_dcn, torch_ops, hip_train,
                                     block, self.plain_kernels, self.plain_train)
            inplanes = planes * block.expansion
            name = f'layer{i + 1}'
            self.add_module(name, layer)
            self.res_layers.append(name)
        self.feat_dim = inplanes
        self.init_weights()
        self._freeze_stages()
        self.torch_ops = torch_ops
        # refused here, not at the first forward
        refuse_outside_limits(self, f'ResNet({depth}, plain_kernels=True)', [f'{name}: {w}' for name, m in self._routed() for w in m._kernel_limits])

    @staticmethod
    def _make_stage(inplanes, planes, blocks, stride, dilation, norm_cfg, dcn, torch_ops, hip_train=False, block=Bottleneck,
                    plain_kernels=False, plain_train=False):
        downsample = None
        if stride != 1 or inplanes != planes * block.expansion:
            downsample = nn.Sequential(nn.Conv2d(inplanes, planes * block.expansion, kernel_size=1, stride=stride, bias=False),
                                       _norm(norm_cfg, planes * block.expansion))
        layers = [block(inplanes, planes, stride, dilation, downsample, norm_cfg, dcn, torch_ops, hip_train, plain_kernels, plain_train)]
        inplanes = planes * block.expansion
        for _ in range(1, blocks):
            layers.append(block(inplanes, planes, 1, dilation, None, norm_cfg, dcn, torch_ops, hip_train, plain_kernels, plain_train))
        return nn.Sequential(*layers)

    def _routed(self):
        """(name, block) of the blocks on the route rule: every block with plain_kernels=True, none without."""
        return [(name, m) for name, m in self.named_modules() if isinstance(m, _PlainKernels) and m.plain_kernels]

    @property
    def torch_ops(self):
        return self._torch_ops

    @torch_ops.setter
    def torch_ops(self, value):
        self._torch_ops = bool(value)
        for _, m in self._routed():
            m.torch_ops = self._torch_ops

    def refresh_images(self):
        """Rebuild every changed weight image and folded BatchNorm into the buffers a captured graph reads (kernel_route.py)."""
        for _, m in self._routed():
            m.refresh_images()

    def init_weights(self):
        """mmdet's default: Kaiming-normal convolutions, unit BatchNorms, zero conv_offset, zero-initialised last BatchNorm of a block."""
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)
        for m in self.modules():
            if isinstance(m, Bottleneck):
                if m.with_dcn and hasattr(m.conv2, 'conv_offset'):
                    nn.init.zeros_(m.conv2.conv_offset.weight)
                    nn.init.zeros_(m.conv2.conv_offset.bias)
                if self.zero_init_residual:
                    nn.init.zeros_(m.bn3.weight)
            elif isinstance(m, BasicBlock) and self.zero_init_residual:
                nn.init.zeros_(m.bn2.weight)

    def _freeze_stages(self):
        if self.frozen_stages >= 0:
            for m in (self.conv1, self.bn1):
                m.eval()
                for p in m.parameters():
                    p.requires_grad = False
        for i in range(1, self.frozen_stages + 1):
            m = getattr(self, f'layer{i}')
            m.eval()
            for p in m.parameters():
                p.requires_grad = False

    def forward(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        outs = []
        for i, name in enumerate(self.res_layers):
            x = getattr(self, name)(x)
            if i in self.out_indices:
                outs.append(x)
        return tuple(outs)

    def train(self, mode=True):
        super().train(mode)
        self._freeze_stages()
        if mode and self.norm_eval:
            for m in self.modules():
                if isinstance(m, nn.BatchNorm2d):
                    m.eval()
        return self
