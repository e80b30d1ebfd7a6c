"""The image neck: mmdet's `FPN` and the reference's `CPFPN` (projects/mmdet3d_plugin/models/necks/cp_fpn.py) - the stage between the
backbone and everything this package runs (position embedding, DepthNet, decoder, distillation).

Both classes take the reference's constructor keywords and keep its state-dict keys (`lateral_convs.{i}.conv.weight/bias`,
`fpn_convs.{i}.conv.weight/bias`: mmcv's ConvModule holds its nn.Conv2d as `.conv`), so a reference checkpoint's neck slice loads with
strict=True.  For inputs C_0..C_{n-1} and s = start_level (cp_fpn.py:157-208; mmdet's FPN.forward is the same but for the outputs):
    laterals   lat_i = conv1x1_i(C_{i+s}) + b_i                                                          (:162-165)
    top-down   lat_{i-1} += F.interpolate(lat_i, size=lat_{i-1}.shape[2:], mode='nearest'), coarse to fine (:169-178)
    outputs    FPN: conv3x3_i(lat_i) + b_i for every level; CPFPN: level 0 only, the others ARE their laterals (:124-134, :182-184)
    extras     add_extra_convs='on_output': conv3x3 stride 2 pad 1 of outs[-1], from the second extra on of relu(outs[-1]) when
               relu_before_extra_convs (:202-207)

What runs where (inference, fp32 maps, 256 output channels): one gd4d_fpn_lateral_fwd launch per level, coarse to fine, computes
the lateral with the top-down add fused in; the 3x3 output convolutions of all levels are ONE gd4d_fpn_conv_fwd launch (a weight
image per level); each extra level is one gd4d_fpn_extra_conv_fwd launch.  Inputs that are not fp32 or not contiguous NCHW are
converted with `.float().contiguous()` first: that cast is a torch copy, not fused into the kernels' loads.

Two keywords are not the reference's:
    torch_ops=False          True: the module's own nn.Conv2d / F.interpolate, the reference's op sequence - trainable, and the route
                             for configurations outside the kernels' limits (GD4D_TORCH_OPS=1 chooses it for the whole process).
    channels_last_out=False  True: the outputs are logical (N, 256, H, W) tensors STORED (N, H, W, 256), written that way by the
                             kernels, so ImageFeatureExtractor(channels_last=True)'s `.contiguous(memory_format=...)` is a no-op and
                             the decoder gathers them in place (ops.PyramidView.channels_last_levels).
    hip_train=False          True: the kernel route trains.  In train() mode, or with autograd on and a parameter or an input that
                             requires grad, the call runs as ONE autograd node (_FpnTrainFunction): its forward is the launches
                             above (the same bits), its backward the library's kernels (below).  `torch_ops=True` wins over it.
The route of a call follows kernel_route.py's rule; a configuration outside the kernels' limits is refused at construction.

The backward (hip_train=True), with dout_k the gradient of output k and gl_i the gradient of lateral i:
    extras     last to first: g(outs[k-1]) = dout_{k-1} + [outs[k-1] > 0]? dgrad_stride2(g(outs[k])) (gd4d_fpn_extra_conv_dgrad, the mask
               where the forward applied its ReLU on read); dW, db by gd4d_fpn_extra_conv_wgrad
    3x3        gl_i = conv3x3^T(g(outs[i])): ONE gd4d_fpn_conv_fwd launch on transposed, tap-flipped images; dW by gd4d_depth_conv_wgrad
               per level, db by gd4d_fpn_bias_grad.  CPFPN's levels >= 1: gl_i = g(outs[i])
    top-down   fine to coarse, gl_{i+1} += U^T gl_i in place (gd4d_fpn_topdown_bwd), U the forward's nearest upsampling
    laterals   dW_i, db_i by gd4d_fpn_lateral_wgrad, dx_i = W_i^T gl_i by gd4d_fpn_lateral_dgrad
Incoming gradients that are not fp32 contiguous NCHW (every one of them when channels_last_out=True) are made so with `.contiguous()`
first, and so are channels-last outputs the backward reads: torch copies, as the forward's cast of its inputs.  Gradients of inputs
that do not require grad (a frozen backbone, a teacher, the levels below start_level) and of frozen parameters are not computed.
On this route the laterals are new tensors every call (the node keeps them until its backward; the kept per-slot buffers would be
overwritten by the next call).  All sums run in a fixed order: two runs give the same bits.

Kept state: the weights' fragment images (kernel_route.py), and the intermediate laterals, per (device, request slot, shapes).  The
outputs are new tensors every call.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from . import functional as Fn
from . import ops
from .kernel_route import KernelRoute, f32, refuse_outside_limits
from .registry import NECKS

OUT_CHANNELS = 256
MAX_LEVELS_PER_LAUNCH = 4


class _FpnTrainFunction(torch.autograd.Function):
    """The neck's kernel route as one autograd node: forward = FPN._forward_hip's launches, backward = the module docstring's data flow.
    tensors: the lateral (weight, bias) pairs, the fpn_convs (weight, bias) pairs, then the used inputs.  Keeps the inputs, the
    laterals that feed a 3x3 convolution and the outputs the extra levels read."""

    @staticmethod
    def forward(ctx, module, *tensors):
        used, nconv = len(module.lateral_convs), len(module.fpn_convs)
        xs = tensors[2 * (used + nconv):]
        outs, laterals, xs = module._forward_hip(list(xs), used_inputs=True, fresh_laterals=True)
        ctx.module = module
        ctx.shapes = [tuple(o.shape) for o in outs]
        ctx.x_dtypes = [t.dtype for t in tensors[2 * (used + nconv):]]
        has_conv = [module._output_conv_of(i) is not None for i in range(used)]
        extra_in = list(outs[used - 1:len(outs) - 1])            # the input of extra level e is output used - 1 + e
        ctx.save_for_backward(*xs, *[l for l, h in zip(laterals, has_conv) if h], *extra_in)
        return tuple(outs)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *douts):
        m = ctx.module
        used, nconv, n3 = len(m.lateral_convs), len(m.fpn_convs), m.num_output_convs
        extras = nconv - n3
        saved = ctx.saved_tensors
        xs = saved[:used]
        has_conv = [m._output_conv_of(i) is not None for i in range(used)]
        conv_in = dict(zip([i for i in range(used) if has_conv[i]], saved[used:used + sum(has_conv)]))
        extra_in = [t.contiguous() for t in saved[used + sum(has_conv):]]
        need = ctx.needs_input_grad[1:]                          # (lateral w, b) * used, (conv w, b) * nconv, inputs * used
        need_lat = lambda i: (need[2 * i], need[2 * i + 1])                                                      # noqa: E731
        need_conv = lambda k: (need[2 * (used + k)], need[2 * (used + k) + 1])                                   # noqa: E731
        need_x = need[2 * (used + nconv):]
        dev = xs[0].device
        g = [torch.zeros(s, device=dev, dtype=torch.float32) if d is None else d.float().contiguous() for d, s in zip(douts, ctx.shapes)]
        grads = [None] * len(need)
        images_t = m._all_images_t()
        # extras, last to first
        for e in range(extras - 1, -1, -1):
            k, ci = used + e, n3 + e
            relu = e > 0 and m.relu_before_extra_convs
            x = extra_in[e]
            if any(need_conv(ci)):
                dw, db = ops.fpn_extra_conv_wgrad(g[k], x, relu_in=relu)
                grads[2 * (used + ci)], grads[2 * (used + ci) + 1] = (dw if need_conv(ci)[0] else None), (db if need_conv(ci)[1] else None)
            g[k - 1] = ops.fpn_extra_conv_dgrad(g[k], images_t[1][ci], x.shape[2:], mask=x if relu else None, add=g[k - 1])
        # 3x3 output convolutions: one launch for the input gradients of all levels
        gl = [None] * used
        todo = [i for i in range(used) if has_conv[i]]
        for j in range(0, len(todo), MAX_LEVELS_PER_LAUNCH):
            grp = todo[j:j + MAX_LEVELS_PER_LAUNCH]
            res = ops.fpn_conv_fwd([g[i] for i in grp], [images_t[1][m._output_conv_of(i)] for i in grp], [None] * len(grp))
            for i, r in zip(grp, res):
                gl[i] = r
        for i in range(used):
            k = m._output_conv_of(i)
            if k is None:                                        # the lateral is the output; level >= 1's gradient is added to in place
                gl[i] = g[i].clone() if i > 0 and (douts[i] is not None and g[i].data_ptr() == douts[i].data_ptr()) else g[i]
                continue
            if need_conv(k)[0]:
                grads[2 * (used + k)] = ops.depth_conv_wgrad([g[i]], [conv_in[i]])
            if need_conv(k)[1]:
                grads[2 * (used + k) + 1] = ops.fpn_bias_grad(g[i])
        # top-down, fine to coarse
        for i in range(used - 1):
            ops.fpn_topdown_bwd(gl[i], gl[i + 1])
        # laterals
        for i in range(used):
            if any(need_lat(i)):
                dw, db = ops.fpn_lateral_wgrad(gl[i], xs[i])
                grads[2 * i], grads[2 * i + 1] = (dw if need_lat(i)[0] else None), (db if need_lat(i)[1] else None)
            if need_x[i]:
                grads[2 * (used + nconv) + i] = ops.fpn_lateral_dgrad(gl[i], images_t[0][i], xs[i].shape[1]).to(ctx.x_dtypes[i])
        return (None, *grads)


class _ConvModule(nn.Module):
    """mmcv's ConvModule without norm and activation: the convolution is the submodule `conv`."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size, stride=stride, padding=padding)

    def forward(self, x):
        return self.conv(x)


@NECKS.register_module()
class FPN(KernelRoute, nn.Module):
    """mmdet.models.necks.FPN (the shipped config: in_channels=[256, 512, 1024, 2048], out_channels=256, start_level=1,
    add_extra_convs='on_output', num_outs=4, relu_before_extra_convs=True)."""
    _kernels = 'kernels give the neck\'s convolutions a backward only on request'

    def __init__(self, in_channels, out_channels, num_outs, start_level=0, end_level=-1, add_extra_convs=False,
                 relu_before_extra_convs=False, no_norm_on_lateral=False, conv_cfg=None, norm_cfg=None, act_cfg=None,
                 upsample_cfg=dict(mode='nearest'), init_cfg=dict(type='Xavier', layer='Conv2d', distribution='uniform'),
                 torch_ops=False, channels_last_out=False, hip_train=False):
        super().__init__()
        assert isinstance(in_channels, (list, tuple))
        self.in_channels = list(in_channels)
        self.out_channels = out_channels
        self.num_ins = len(in_channels)
        self.num_outs = num_outs
        self.relu_before_extra_convs = relu_before_extra_convs
        self.no_norm_on_lateral = no_norm_on_lateral
        self.upsample_cfg = dict(upsample_cfg)
        self.channels_last_out = bool(channels_last_out)
        self.hip_train = bool(hip_train)
        if end_level == -1:
            self.backbone_end_level = self.num_ins
            assert num_outs >= self.num_ins - start_level
        else:
            self.backbone_end_level = end_level
            assert end_level <= len(in_channels)
            assert num_outs == end_level - start_level
        self.start_level = start_level
        self.end_level = end_level
        assert isinstance(add_extra_convs, (str, bool))
        if isinstance(add_extra_convs, str):
            assert add_extra_convs in ('on_input', 'on_lateral', 'on_output')
        elif add_extra_convs:
            add_extra_convs = 'on_input'
        self.add_extra_convs = add_extra_convs

        built = [k for k, v in (('conv_cfg', conv_cfg), ('norm_cfg', norm_cfg), ('act_cfg', act_cfg)) if v is not None]
        if built:
            raise _lib.Gd4dError(f'{type(self).__name__}: {", ".join(built)} given; this module builds plain nn.Conv2d layers with a bias '
                                 '(what every shipped config uses), on the kernels and on the `torch_ops=True` route alike')
        self._init_route(torch_ops, self._outside_kernel_limits())
        refuse_outside_limits(self, type(self).__name__, self._kernel_limits)      # here, not at the first forward

        self.lateral_convs = nn.ModuleList()
        self.fpn_convs = nn.ModuleList()
        for i in range(self.start_level, self.backbone_end_level):
            self.lateral_convs.append(_ConvModule(in_channels[i], out_channels, 1))
            if self._has_output_conv(i):
                self.fpn_convs.append(_ConvModule(out_channels, out_channels, 3, padding=1))
        self.num_output_convs = len(self.fpn_convs)
        extra_levels = num_outs - self.backbone_end_level + self.start_level
        if self.add_extra_convs and extra_levels >= 1:
            for i in range(extra_levels):
                cin = self.in_channels[self.backbone_end_level - 1] if i == 0 and self.add_extra_convs == 'on_input' else out_channels
                self.fpn_convs.append(_ConvModule(cin, out_channels, 3, stride=2, padding=1))
        self._init_weights(init_cfg)
        self._laterals = {}         # (device, request slot, shapes) -> the intermediate laterals

    # ---- construction ---------------------------------------------------------------------------------------------------
    def _has_output_conv(self, backbone_index):
        return True

    def _output_conv_of(self, level):
        """Index into fpn_convs of the 3x3 output convolution of lateral `level`, or None (the lateral is the output)."""
        return level

    def _outside_kernel_limits(self):
        why = []
        if self.out_channels != OUT_CHANNELS:
            why.append(f'out_channels={self.out_channels} (kernels: {OUT_CHANNELS})')
        if self.end_level != -1:
            why.append(f'end_level={self.end_level} (kernels: -1)')
        if self.upsample_cfg != dict(mode='nearest'):
            why.append(f'upsample_cfg={self.upsample_cfg} (kernels: dict(mode=\'nearest\'))')
        extra_levels = self.num_outs - (self.backbone_end_level - self.start_level)
        if extra_levels > 0 and not self.add_extra_convs:
            why.append('extra levels by max-pooling (kernels: add_extra_convs=\'on_output\')')
        if self.add_extra_convs and self.add_extra_convs != 'on_output':
            why.append(f'add_extra_convs=\'{self.add_extra_convs}\' (kernels: \'on_output\')')
        used = self.in_channels[self.start_level:self.backbone_end_level]
        if any(c % 32 or not 32 <= c <= 2048 for c in used):
            why.append(f'in_channels={used} (kernels: multiples of 32 in [32, 2048])')
        return why

    def _init_weights(self, init_cfg):
        """mmcv's initialize() for the default init_cfg: Xavier-uniform weights, zero biases on every Conv2d."""
        if not init_cfg or init_cfg.get('type') != 'Xavier':
            return
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                if init_cfg.get('distribution', 'normal') == 'uniform':
                    nn.init.xavier_uniform_(m.weight, gain=init_cfg.get('gain', 1))
                else:
                    nn.init.xavier_normal_(m.weight, gain=init_cfg.get('gain', 1))
                nn.init.constant_(m.bias, init_cfg.get('bias', 0))

    # ---- torch-op route: the reference's op sequence -------------------------------------------------------------------
    def _forward_torch(self, inputs):
        laterals = [conv(inputs[i + self.start_level]) for i, conv in enumerate(self.lateral_convs)]               # :162-165
        used = len(laterals)
        for i in range(used - 1, 0, -1):                                                                           # :169-178
            if 'scale_factor' in self.upsample_cfg:
                laterals[i - 1] = laterals[i - 1] + F.interpolate(laterals[i], **self.upsample_cfg)
            else:
                laterals[i - 1] = laterals[i - 1] + F.interpolate(laterals[i], size=laterals[i - 1].shape[2:], **self.upsample_cfg)
        outs = []
        for i in range(used):                                                                                      # :182-184
            k = self._output_conv_of(i)
            outs.append(laterals[i] if k is None else self.fpn_convs[k](laterals[i]))
        if self.num_outs > len(outs):                                                                              # :186-207
            if not self.add_extra_convs:
                for _ in range(self.num_outs - used):
                    outs.append(F.max_pool2d(outs[-1], 1, stride=2))
            else:
                source = {'on_input': inputs[self.backbone_end_level - 1], 'on_lateral': laterals[-1], 'on_output': outs[-1]}
                k = self.num_output_convs
                outs.append(self.fpn_convs[k](source[self.add_extra_convs]))
                for j in range(used + 1, self.num_outs):
                    k += 1
                    outs.append(self.fpn_convs[k](F.relu(outs[-1]) if self.relu_before_extra_convs else outs[-1]))
        if self.channels_last_out:
            outs = [o.contiguous(memory_format=torch.channels_last) for o in outs]
        return tuple(outs)

    # ---- kernel route -------------------------------------------------------------------------------------------------
    def _image(self, key, weight, build):
        return self._keep(key, (weight,), lambda: build(weight.detach()))

    def _all_images(self):
        lat = [self._image(('lateral', i), m.conv.weight, ops.fpn_lateral_image) for i, m in enumerate(self.lateral_convs)]
        conv = [self._image(('conv', i), m.conv.weight, ops.depth_net_image) for i, m in enumerate(self.fpn_convs)]
        return lat, conv

    def _all_images_t(self):
        """The backward's images: the transposed laterals and the transposed, tap-flipped 3x3 weights, under the forward's rule."""
        lat = [self._image(('lateral_t', i), m.conv.weight, ops.fpn_lateral_image_t) for i, m in enumerate(self.lateral_convs)]
        conv = [self._image(('conv_t', i), m.conv.weight, ops.depth_net_image_t) for i, m in enumerate(self.fpn_convs)]
        return lat, conv

    def _kept_values(self):
        self._all_images()

    def _lateral_buffers(self, shapes, layouts, dev):
        key = (str(dev), Fn.slot_key(dev), tuple(shapes), tuple(layouts))
        bufs = self._laterals.get(key)
        if bufs is None:
            if len(self._laterals) >= 16:                  # (streams come and go: do not keep every shape ever seen)
                self._laterals.clear()
            bufs = self._laterals[key] = [None if cl is None else ops.fpn_empty(n, h, w, dev, cl) for (n, h, w), cl in zip(shapes, layouts)]
        return bufs

    def _forward_hip(self, inputs, used_inputs=False, fresh_laterals=False):
        """used_inputs: `inputs` are the used levels only.  fresh_laterals (the training node): the laterals are new tensors, and the
        call returns (outs, laterals, the fp32 contiguous inputs)."""
        used = len(self.lateral_convs)
        xs = list(inputs) if used_inputs else [inputs[i + self.start_level] for i in range(used)]
        xs = [f32(x) for x in xs]
        if any(x.dim() != 4 or x.shape[0] != xs[0].shape[0] for x in xs):
            raise ValueError(f'{type(self).__name__}: (N, C, H, W) maps of the same N expected')
        for x, m in zip(xs, self.lateral_convs):
            if x.shape[1] != m.conv.in_channels:
                raise ValueError(f'{type(self).__name__}: a {x.shape[1]}-channel map for a lateral of {m.conv.in_channels} input channels')
        dev = xs[0].device
        cl = self.channels_last_out
        lat_images, conv_images = self._all_images()
        # a lateral that is an output (CPFPN's levels >= 1) is a new tensor in the output layout; the others are kept NCHW buffers
        shapes = [(int(x.shape[0]), int(x.shape[2]), int(x.shape[3])) for x in xs]
        is_out = [self._output_conv_of(i) is None for i in range(used)]
        laterals = [None] * used if fresh_laterals else self._lateral_buffers(shapes, [None if o else False for o in is_out], dev)
        laterals = [ops.fpn_empty(*s, dev, cl) if o else (ops.fpn_empty(*s, dev) if b is None else b)
                    for s, o, b in zip(shapes, is_out, laterals)]
        for i in range(used - 1, -1, -1):
            ops.fpn_lateral_fwd(xs[i], lat_images[i], self.lateral_convs[i].conv.bias.detach(), up=laterals[i + 1] if i + 1 < used else None,
                                out=laterals[i])
        outs = list(laterals)
        todo = [i for i in range(used) if not is_out[i]]
        for j in range(0, len(todo), MAX_LEVELS_PER_LAUNCH):
            grp = todo[j:j + MAX_LEVELS_PER_LAUNCH]
            ks = [self._output_conv_of(i) for i in grp]
            res = ops.fpn_conv_fwd([laterals[i] for i in grp], [conv_images[k] for k in ks],
                                   [self.fpn_convs[k].conv.bias.detach() for k in ks], channels_last_out=cl)
            for i, r in zip(grp, res):
                outs[i] = r
        for e, k in enumerate(range(self.num_output_convs, len(self.fpn_convs))):
            outs.append(ops.fpn_extra_conv_fwd(outs[-1], conv_images[k], self.fpn_convs[k].conv.bias.detach(),
                                               relu_in=e > 0 and self.relu_before_extra_convs, channels_last_out=cl))
        if fresh_laterals:
            return outs, laterals, xs
        return tuple(outs)

    def forward(self, inputs):
        """inputs: the backbone's len(in_channels) maps (N, C_i, H_i, W_i) -> the tuple of num_outs maps (N, 256, H_l, W_l)."""
        assert len(inputs) == len(self.in_channels)
        inputs = list(inputs)
        route = self._route(*inputs)
        if route == 'torch':
            return self._forward_torch(inputs)
        if route == 'train':
            used = len(self.lateral_convs)
            params = [t for m in list(self.lateral_convs) + list(self.fpn_convs) for t in (m.conv.weight, m.conv.bias)]
            return _FpnTrainFunction.apply(self, *params, *inputs[self.start_level:self.start_level + used])
        with torch.no_grad():
            return self._forward_hip(inputs)


@NECKS.register_module()
class CPFPN(FPN):
    """The reference's CPFPN (cp_fpn.py; the VoVNet configs: in_channels=[256, 512, 768, 1024], start_level=0): an FPN whose only 3x3
    output convolution is backbone level 0's (`if i == 0`, :124); levels >= 1 return their laterals.  fpn_convs holds that one entry.
    Extra convolution levels are refused: the reference's forward cannot run them (see __init__).  With start_level > 0 the reference builds no output convolution and its forward (:183) then applies an EXTRA
    convolution to level 0: such a configuration is refused here."""

    def __init__(self, in_channels, out_channels, num_outs, start_level=0, **kwargs):
        if start_level != 0:
            raise _lib.Gd4dError('CPFPN: start_level != 0 - the reference then indexes fpn_convs[0] (cp_fpn.py:183) without having built '
                                 'level 0\'s convolution (:124); neither the kernels nor `torch_ops=True` restate that')
        if kwargs.get('add_extra_convs', False) and kwargs.get('end_level', -1) == -1 and num_outs > len(in_channels):
            raise _lib.Gd4dError('CPFPN: extra convolution levels - the reference\'s forward indexes fpn_convs[number of levels] '
                                 '(cp_fpn.py:202), past the list its constructor built (one output convolution, :124): it raises '
                                 'IndexError for every such configuration, so there is nothing to restate (`torch_ops=True` included); '
                                 'every shipped config has num_outs == len(in_channels)')
        super().__init__(in_channels, out_channels, num_outs, start_level=start_level, **kwargs)

    def _has_output_conv(self, backbone_index):
        return backbone_index == 0

    def _output_conv_of(self, level):
        return 0 if level == 0 else None
