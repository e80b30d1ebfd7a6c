"""Camera-aware DepthNet of Detr3DHeadPECAM - the stage in front of the head's position embedding.

Mirror of `DepthNet` (projects/mmdet3d_plugin/models/dense_heads/detr3d_head_pe_camaware.py:59-105, built at :198 as
`DepthNet(256, 256, 80)`, applied to every level at :313-320): same submodule names (`reduce_conv.{0,1}`, `context_conv`,
`mlp.fc{1,2}`, `se.conv_{reduce,expand}`), so the head checkpoint's `depth_net.` slice loads with strict=True.

Per level x (1, N, 256, H, W) and camera n:
    out[n] = relu(BN(conv3x3(x[n]))) * sigmoid(se(mlp(s[n]))),   s[n] = |(inv(K_n)[0,0], inv(K_n)[1,1])| * 1000 / aug_scale
with K_n the camera's 4x4 intrinsics and aug_scale from the image-augmentation matrix.  `context_conv` is computed and discarded by
the reference (`forward` returns x); it is not computed here, its parameters are kept so the state dict loads.

What runs where (inference): the gate is one kernel (ops.cam_gate_fwd) reading the intrinsics / ida scales from a persistent device
buffer (a captured graph serves new cameras after refresh_matrices), the 3x3 convolution with bias, BatchNorm (running statistics),
ReLU and the gate as its epilogue is ONE launch over all levels (ops.depth_conv_fwd, split-bf16 x 3 on the bf16 matrix cores).
The route of a call follows kernel_route.py's rule (limits per call: 256 channels, float32 maps); the torch-op route is the module's
own nn.Conv2d / BatchNorm2d / MLP / SE, the reference arithmetic.  CPU maps are refused on every route.  The two weight images
(the forward's, and the input gradient's) are kept values of that file: fixed addresses, `refresh_images()`.

Training on the kernels is opt-in (`hip_train=True`; `torch_ops=True` wins over it): one autograd node per call over all levels
(_DepthNetTrainFunction).  Forward: the same implicit GEMM with a plain-store epilogue keeps y = conv + bias and emits per-tile
(mean, M2) partials, ops.depth_bn_stats merges them per level in a fixed order and moves the running buffers as L BatchNorm2d calls
would, ops.depth_bn_act_fwd writes relu(BN(y)) * gate.  Backward: ops.depth_bn_bwd (dgamma, dbeta, the gate's gradient, dy, the
bias gradient), ops.depth_conv_wgrad (the weight gradient, K over the pixels) and the same GEMM on dy with the transposed, tap-flipped
weight image (the input gradient).  Kept for backward: x, y, the statistics and the gate - not BatchNorm's, ReLU's or the gate's
outputs.  In eval() mode with autograd on BatchNorm is frozen (mmdet's norm_eval): the affine map of the running statistics, no
buffer moves, outputs bit-identical to inference.  The camera gate is ~3 MFLOP per sample: in this route it runs through the
module's own mlp / se layers, so autograd carries the Function's gate gradient into them; the kernels multiply by the gate
kernel's value of the same quantity (frozen outputs are then the inference path's bits).
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import functional as Fn
from . import ops
from .kernel_route import KernelRoute, f32

MAX_LEVELS_PER_LAUNCH = 4


class Mlp(nn.Module):
    """detr3d_head_pe_camaware.py:33-56 (drop = 0)."""

    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.ReLU, drop=0.0):
        super().__init__()
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.act = act_layer()
        self.drop1 = nn.Dropout(drop)
        self.fc2 = nn.Linear(hidden_features, out_features)
        self.drop2 = nn.Dropout(drop)

    def forward(self, x):
        return self.drop2(self.fc2(self.drop1(self.act(self.fc1(x)))))


class SELayer(nn.Module):
    """detr3d_head_pe_camaware.py:20-31."""

    def __init__(self, channels, act_layer=nn.ReLU, gate_layer=nn.Sigmoid):
        super().__init__()
        self.conv_reduce = nn.Conv2d(channels, channels, 1, bias=True)
        self.act1 = act_layer()
        self.conv_expand = nn.Conv2d(channels, channels, 1, bias=True)
        self.gate = gate_layer()

    def forward(self, x, x_se):
        return x * self.gate(self.conv_expand(self.act1(self.conv_reduce(x_se))))


def _intrinsics(mats):
    """(N, 16) fp32 host array of the cameras' 4x4 intrinsics (img_metas[0]['intrinsics'], the pipeline's float32 viewpads)."""
    a = np.asarray([np.asarray(torch.as_tensor(m).cpu() if torch.is_tensor(m) else m, dtype=np.float32) for m in mats],
                   dtype=np.float32)
    if a.ndim != 3 or a.shape[1:] != (4, 4):
        raise ValueError(f'DepthNet: intrinsics must be N 4x4 matrices, got shape {a.shape}')
    return np.ascontiguousarray(a.reshape(-1, 16))


def _ida00(ida_mats, n):
    """ida[..., 0, 0] of torch.stack(ida_mats) (:87, :93-94) as an (N,) fp32 host array.  The list holds 1 matrix (the pipeline keeps
    one: transform_3d.py:389 resets the list per camera), broadcast over the cameras here, or N: either way the device buffer has
    the same shape, so a graph captured on one form serves the other."""
    a = np.asarray([np.asarray(m.detach().cpu() if torch.is_tensor(m) else m, dtype=np.float32) for m in ida_mats], dtype=np.float32)
    if a.ndim < 3:
        raise ValueError(f'DepthNet: ida_mats must be a list of square matrices, got shape {a.shape}')
    d = np.ascontiguousarray(a[..., 0, 0].reshape(-1))
    if d.shape[0] not in (1, n):
        raise ValueError(f'DepthNet: {d.shape[0]} ida matrices for {n} cameras (1 or {n} expected)')
    return np.array(np.broadcast_to(d, (n,)), dtype=np.float32)          # (a writable copy)


class _DepthNetTrainFunction(torch.autograd.Function):
    """relu(BN(conv3x3(x_l) + b)) * gate for all levels of a call as one node (launches of at most MAX_LEVELS_PER_LAUNCH levels).
    Keeps x, y = conv + b, the per-level statistics and the gate; out is recomputed from y in backward."""

    @staticmethod
    def forward(ctx, module, frozen, gate_value, gate, weight, bias, gamma, beta, *feats):
        # gate: the module's mlp / se layers' (N, 256), the input autograd carries the gate gradient into; gate_value: the gate
        # kernel's bits of the same quantity, what the kernels multiply by (so that frozen outputs are the inference path's bits)
        gate = gate_value
        bn = module.reduce_conv[1]
        image = module._image()
        feats = [f32(f) for f in feats]
        gate, bias, gamma, beta = (t.detach().contiguous() for t in (gate, bias, gamma, beta))
        n = feats[0].shape[0]
        ys, stats, outs = [], [], []
        for i in range(0, len(feats), MAX_LEVELS_PER_LAUNCH):
            grp = feats[i:i + MAX_LEVELS_PER_LAUNCH]
            hw = [tuple(f.shape[2:]) for f in grp]
            if frozen:
                y = ops.depth_conv_raw(grp, image, bias)
                st = ops.depth_bn_stats(None, hw, n, gamma, bn.running_mean, bn.running_var, 0.0, bn.eps, frozen=True)
            else:
                y, partials = ops.depth_conv_raw(grp, image, bias, want_partials=True)
                st = ops.depth_bn_stats(partials, hw, n, gamma, bn.running_mean, bn.running_var, bn.momentum, bn.eps)
            outs += ops.depth_bn_act_fwd(y, st, beta, gate)
            ys += y
            stats.append(st)
        ctx.module, ctx.frozen, ctx.levels = module, frozen, len(feats)
        ctx.save_for_backward(gate, weight, beta, *stats, *ys, *feats)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *douts):
        saved = ctx.saved_tensors
        nl = ctx.levels
        groups = (nl + MAX_LEVELS_PER_LAUNCH - 1) // MAX_LEVELS_PER_LAUNCH
        gate, weight, beta = saved[:3]
        stats, ys, feats = saved[3:3 + groups], saved[3 + groups:3 + groups + nl], saved[3 + groups + nl:]
        need = ctx.needs_input_grad                                         # (module, frozen, gate_value, gate, weight, bias, gamma, beta, *feats)
        douts = [torch.zeros_like(y) if d is None else d.contiguous() for d, y in zip(douts, ys)]
        dgate = dw = db = dgamma = dbeta = None
        dxs = [None] * nl
        image_t = None

        def add(a, b):
            return b.clone() if a is None else a + b                         # (the launches of a call in order: a fixed sum)
        for k in range(groups):
            lo, hi = k * MAX_LEVELS_PER_LAUNCH, min(nl, (k + 1) * MAX_LEVELS_PER_LAUNCH)
            dys, g_gamma, g_beta, g_gate, g_bias = ops.depth_bn_bwd(douts[lo:hi], ys[lo:hi], stats[k], beta, gate, frozen=ctx.frozen)
            dgate, dgamma, dbeta, db = add(dgate, g_gate), add(dgamma, g_gamma), add(dbeta, g_beta), add(db, g_bias)
            if need[4]:
                dw = add(dw, ops.depth_conv_wgrad(dys, list(feats[lo:hi])))
            if any(need[8 + lo:8 + hi]):
                if image_t is None:
                    image_t = ctx.module._image_t()
                for j, dx in enumerate(ops.depth_conv_raw(dys, image_t)):
                    if need[8 + lo + j]:
                        dxs[lo + j] = dx
        return (None, None, None, dgate if need[3] else None, dw, db if need[5] else None, dgamma if need[6] else None,
                dbeta if need[7] else None, *dxs)


class DepthNet(KernelRoute, nn.Module):
    _kernels = ('kernels run this stage\'s BatchNorm on its running statistics and give the 3x3 convolution a backward only on '
                'request (train() mode normalises with batch statistics)')

    def __init__(self, in_channels, mid_channels, context_channels, torch_ops=False, hip_train=False):
        """torch_ops (not a keyword of the reference): run the module's own torch layers (the reference arithmetic, trainable) instead
        of the library's kernels - the only route for shapes the kernels do not take.  hip_train (neither): make the kernel route
        differentiable - train() mode, or eval() mode with autograd on (frozen BatchNorm), runs on the library's forward and backward
        kernels.  Both are attributes that may be set after construction; torch_ops wins."""
        super().__init__()
        self.reduce_conv = nn.Sequential(
            nn.Conv2d(in_channels, mid_channels, kernel_size=3, stride=1, padding=1),
            nn.BatchNorm2d(mid_channels),
            nn.ReLU(inplace=True),
        )
        self.context_conv = nn.Conv2d(mid_channels, context_channels, kernel_size=1, stride=1, padding=0)
        self.mlp = Mlp(1, mid_channels, mid_channels)
        self.se = SELayer(mid_channels)
        self.hip_train = bool(hip_train)
        self._init_route(torch_ops)
        self._mats = {}             # (device, request slot, N) -> [host intrinsics, host ida00 (N), device buffer]

    # ---- routes ---------------------------------------------------------------------------------------------------------
    def _route_name(self):
        return f'camera-aware DepthNet({self.reduce_conv[0].in_channels}, {self.reduce_conv[0].out_channels})'

    def _limits(self, *feats):
        """Per call: the maps' channels and dtype are limits too."""
        conv, bn = self.reduce_conv[0], self.reduce_conv[1]
        why = []
        if conv.in_channels != 256 or conv.out_channels != 256:
            why.append(f'in / mid channels {conv.in_channels} / {conv.out_channels} (kernels: 256)')
        bad = next((f for f in feats if f.shape[-3] != 256 or f.dtype != torch.float32), None)
        if bad is not None:
            why.append(f'{bad.shape[-3]}-channel {bad.dtype} maps (kernels: 256 channels, float32)')
        if self.hip_train and self.training and (bn.momentum is None or not bn.track_running_stats):
            why.append('hip_train with a BatchNorm2d of momentum=None or track_running_stats=False (kernels: a running average)')
        return why

    @staticmethod
    def _squeeze_batch(x):
        if x.dim() == 5:
            if x.shape[0] != 1:
                raise ValueError(f'DepthNet: batch size {x.shape[0]}; the reference squeezes B and takes B = 1 only')
            return x[0]
        if x.dim() != 4:
            raise ValueError(f'DepthNet: (1, N, C, H, W) or (N, C, H, W) maps expected, got {tuple(x.shape)}')
        return x

    # ---- torch-op route: the reference arithmetic --------------------------------------------------------------------------
    def _gate_input_torch(self, intrin, ida00, scale_depth_factor, device):
        """(N, 1) scaled pixel sizes (:86-97); the 4x4 inverses of a few cameras are taken on the host."""
        inv = torch.inverse(torch.from_numpy(intrin).view(-1, 4, 4))                                          # :89
        pixel_size = torch.norm(torch.stack([inv[..., 0, 0], inv[..., 1, 1]], dim=-1), dim=-1).reshape(-1, 1)  # :91-93
        ida00 = torch.from_numpy(ida00)
        aug_scale = torch.sqrt(ida00 ** 2 + ida00 ** 2).reshape(-1, 1)     # :93-94 ([0, 0] twice, as written)
        return (pixel_size * scale_depth_factor / aug_scale).float().to(device)

    def _forward_torch(self, feats, intrin, ida00, scale_depth_factor):
        s = self._gate_input_torch(intrin, ida00, scale_depth_factor, feats[0].device)
        x_se = self.mlp(s)[..., None, None]
        return [self.se(self.reduce_conv(f), x_se) for f in feats]

    # ---- kernel route -------------------------------------------------------------------------------------------------
    def _image(self):
        """The 3x3 weight's fragment image."""
        w = self.reduce_conv[0].weight
        return self._keep('image', (w,), lambda: ops.depth_net_image(w.detach()))

    def _image_t(self):
        """The transposed, tap-flipped weight's image (the input gradient's GEMM)."""
        w = self.reduce_conv[0].weight
        return self._keep('image_t', (w,), lambda: ops.depth_net_image_t(w.detach()))

    def _kept_values(self):
        self._image()

    def _matrices_device(self, intrin, ida00, dev, capturing=False):
        """The intrinsics (N, 4, 4) and ida scales (N) on the device: ONE persistent buffer per (device, request slot, N),
        refreshed in place when the host values differ - a hipGraph captured over this module keeps a valid address, and a replay
        for new cameras only needs refresh_matrices() outside the graph (the pattern of FeaturePositionEmbedding)."""
        n = intrin.shape[0]
        key = (str(dev), Fn.slot_key(dev), n)
        ent = self._mats.get(key)
        if ent is None or not (np.array_equal(ent[0], intrin) and np.array_equal(ent[1], ida00)):
            if capturing:
                if ent is None:
                    raise RuntimeError('DepthNet under hipGraph capture: call the module (or refresh_matrices) once eagerly with these '
                                       'img_metas first - their matrices are not on the device yet')
                raise RuntimeError('DepthNet under hipGraph capture: img_metas changed since the last eager call; '
                                   'refresh_matrices(img_metas) first')
            src = torch.from_numpy(np.concatenate([intrin.reshape(-1), ida00]))
            if ent is None:
                ent = self._mats[key] = [intrin.copy(), ida00.copy(), src.to(dev)]
            else:
                ent[2].copy_(src)
                ent[0], ent[1] = intrin.copy(), ida00.copy()
        buf = ent[2]
        return buf[:16 * n].view(n, 4, 4), buf[16 * n:]

    def refresh_matrices(self, img_metas, device):
        """For the owner of a hipGraph captured over this module: put the new sample's intrinsics and ida scales into the persistent
        device buffer the graph reads (outside the graph, before the replay).  The graph recomputes the gate from them; nothing
        derived from the cameras is kept between calls."""
        intrin = _intrinsics(img_metas[0]['intrinsics'])
        return self._matrices_device(intrin, _ida00(img_metas[0]['ida_mats'], intrin.shape[0]), torch.device(device))

    def _gate(self, intrin, ida00, scale_depth_factor, dev):
        k_dev, ida_dev = self._matrices_device(intrin, ida00, dev, capturing=torch.cuda.is_current_stream_capturing())
        fc1, fc2, cr, ce = self.mlp.fc1, self.mlp.fc2, self.se.conv_reduce, self.se.conv_expand
        return ops.cam_gate_fwd(k_dev, ida_dev, fc1.weight, fc1.bias, fc2.weight, fc2.bias, cr.weight, cr.bias, ce.weight, ce.bias,
                                scale_depth_factor)

    def _forward_hip(self, feats, intrin, ida00, scale_depth_factor):
        image = self._image()                   # first: a stale image under capture raises before anything is recorded
        gate = self._gate(intrin, ida00, scale_depth_factor, feats[0].device)
        conv, bn = self.reduce_conv[0], self.reduce_conv[1]
        feats = [f32(f) for f in feats]
        outs = []
        for i in range(0, len(feats), MAX_LEVELS_PER_LAUNCH):
            outs += ops.depth_conv_fwd(feats[i:i + MAX_LEVELS_PER_LAUNCH], image, conv.bias.detach(), bn.running_mean, bn.running_var,
                                       bn.weight.detach(), bn.bias.detach(), bn.eps, gate)
        return outs

    def _gate_torch_device(self, intrin, ida00, scale_depth_factor, dev):
        """The gate (N, 256) through the module's own mlp / se layers (differentiable), _gate_input_torch's arithmetic on the
        matrices of the persistent device buffer: nothing waits for the device."""
        k_dev, ida_dev = self._matrices_device(intrin, ida00, dev, capturing=torch.cuda.is_current_stream_capturing())
        with torch.no_grad():
            inv = torch.linalg.inv_ex(k_dev).inverse                                                          # :89 (no error check: no sync)
            pixel_size = torch.sqrt(inv[:, 0, 0] ** 2 + inv[:, 1, 1] ** 2).reshape(-1, 1)                     # :91-93
            aug_scale = torch.sqrt(ida_dev ** 2 + ida_dev ** 2).reshape(-1, 1)                                # :93-94
            s = pixel_size * scale_depth_factor / aug_scale
        # se's 1x1 convolutions on (N, 256, 1, 1) taken as linears on (N, 256): the same sums, and a backward that repeats bit
        # for bit (the library convolution's input gradient does not: docs/measurements_r16.md, section 4)
        se = self.se
        r = se.act1(F.linear(self.mlp(s), se.conv_reduce.weight.flatten(1), se.conv_reduce.bias))
        return se.gate(F.linear(r, se.conv_expand.weight.flatten(1), se.conv_expand.bias))

    def _forward_hip_train(self, feats, intrin, ida00, scale_depth_factor):
        gate = self._gate_torch_device(intrin, ida00, scale_depth_factor, feats[0].device)
        with torch.no_grad():
            gate_value = self._gate(intrin, ida00, scale_depth_factor, feats[0].device)
        conv, bn = self.reduce_conv[0], self.reduce_conv[1]
        frozen = not self.training
        outs = _DepthNetTrainFunction.apply(self, frozen, gate_value, gate, conv.weight, conv.bias, bn.weight, bn.bias, *feats)
        if not frozen:
            bn.num_batches_tracked.add_(len(feats))          # one BatchNorm2d call per level
        return list(outs)

    def _run(self, feats, intrin, ida00, scale_depth_factor):
        if len({f.shape[0] for f in feats}) != 1:
            raise ValueError('DepthNet: every level must hold the same cameras')
        for f in feats:
            Fn.require_gpu(f, 'mlvl_feats')         # on every route, as this stage always has: its torch-op route is no CPU fallback
        route = self._route(*feats)
        if route == 'torch':
            return self._forward_torch(feats, intrin, ida00, scale_depth_factor)
        if route == 'train':
            # also in train() mode under torch.no_grad(): BatchNorm must take (and move) batch statistics, which only this forward does
            return self._forward_hip_train(feats, intrin, ida00, scale_depth_factor)
        with torch.no_grad():
            return self._forward_hip(feats, intrin, ida00, scale_depth_factor)

    # ---- the stage ------------------------------------------------------------------------------------------------------
    def forward(self, x, mats_dict, scale_depth_factor=1000.0):
        """The reference's per-level call (:79-105): x (1, N, C, H, W) (or (N, C, H, W)), mats_dict {'intrin_mats': N 4x4,
        'ida_mats': list of 1 or N 3x3} -> (N, C, H, W), which the head unsqueezes (:319)."""
        x = self._squeeze_batch(x)
        intrin = _intrinsics(mats_dict['intrin_mats'])
        if intrin.shape[0] != x.shape[0]:
            raise ValueError(f'DepthNet: {intrin.shape[0]} intrinsics for {x.shape[0]} cameras')
        return self._run([x], intrin, _ida00(mats_dict['ida_mats'], x.shape[0]), scale_depth_factor)[0]

    def forward_levels(self, mlvl_feats, img_metas, scale_depth_factor=1000.0):
        """The head's loop over the levels (:313-320) as one call: mlvl_feats, a list of (1, N, C, H_l, W_l) maps -> the list of
        (1, N, C, H_l, W_l) maps FeaturePositionEmbedding takes.  The gate is computed once and the levels share one launch."""
        if len(img_metas) != 1:
            raise ValueError(f'DepthNet: {len(img_metas)} samples; the reference takes B = 1 only')
        feats = [self._squeeze_batch(f) for f in mlvl_feats]
        intrin = _intrinsics(img_metas[0]['intrinsics'])
        if intrin.shape[0] != feats[0].shape[0]:
            raise ValueError(f'DepthNet: {intrin.shape[0]} intrinsics for {feats[0].shape[0]} cameras')
        outs = self._run(feats, intrin, _ida00(img_metas[0]['ida_mats'], intrin.shape[0]), scale_depth_factor)
        return [o.unsqueeze(0) for o in outs]
