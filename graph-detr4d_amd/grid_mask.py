"""GridMask: the image augmentation every training config of the reference turns on (`use_grid_mask=True`).

Mirror of `GridMask` (projects/mmdet3d_plugin/models/utils/grid_mask.py:69-123), which `Detr3D.extract_img_feat` applies to the
folded (B*N, 3, H, W) images in front of the backbone (detectors/detr3d.py:36, 53-54).  The reference builds a 1.5H x 1.5W mask on
the host, passes it through PIL, crops it, uploads it and multiplies.  With rotate = 1 the angle is always 0 and the cropped mask has a
closed form, so here the step's five integers go to one HIP kernel (gd4d_grid_mask_fwd) and no mask exists anywhere.

Two ways to draw the integers:
  eager (default)   np.random in exactly the reference's order: the same seed gives the reference's output bit for bit;
  device_draw(seed) a tiny kernel (gd4d_grid_mask_draw) draws them from device-resident state into a parameter block the apply
                    kernel reads: no host value enters the step, and a captured graph draws a new mask on every replay.
"""
import numpy as np
import torch
import torch.nn as nn

from . import _lib, ops
from . import functional as Fn

_HALF = (torch.float16, torch.bfloat16)


def prob_threshold(prob):
    """The gate's 32-bit word: apply <=> hash < round(prob 2^32), and 2^32 - 1 means always (csrc/gd4d_grid_mask_rng.h)."""
    t = float(prob) * 4294967296.0
    return 0 if t <= 0.0 else (0xFFFFFFFF if t >= 4294967295.0 else int(t + 0.5))


def _as_i32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >= (1 << 31) else v


class _GridMaskFunction(torch.autograd.Function):
    """forward: the kernel; backward: the same kernel on the gradient with the same parameters (grad * mask; an offset has no
    gradient).  `block` is this call's own copy of the parameter block on the device route."""

    @staticmethod
    def forward(ctx, x, kw, out_dtype):
        ctx.kw, ctx.in_dtype = kw, x.dtype
        return ops.grid_mask_fwd(x, out_dtype=out_dtype, **kw)

    @staticmethod
    def backward(ctx, grad):
        kw = dict(ctx.kw, offset=None, gen_offset=False)
        g = ops.grid_mask_fwd(grad.contiguous(), **kw)
        return g.to(ctx.in_dtype), None, None


class GridMask(nn.Module):
    """GridMask(use_h, use_w, rotate=1, offset=False, ratio=0.5, mode=0, prob=1.): the reference's constructor, attributes
    (`st_prob`, `prob`, `l`) and `set_prob(epoch, max_epoch)`; no parameters, no buffers, no state-dict keys.

    forward(x (N, C, H, W) on the GPU; fp32, fp16 or bf16):
      not training, or the gate says no -> `x` itself (the reference's line 85-86; np.random.rand() is consumed either way);
      otherwise the reference's draws (`host_draw`) and ONE kernel launch; with `offset` the (H, W) offset map is the only upload.
    Keywords beyond the reference's:
      out_dtype   None | torch.float16 | torch.bfloat16: the cast a half-precision backbone needs, in the same pass (fp32 input)
      inplace     write into `x` (same dtype only)
      torch_ops   the reference's own op sequence (host mask, PIL, upload, multiply): the comparison route and the only one that
                  covers rotate > 1; also chosen for every module by GD4D_TORCH_OPS=1
    device_draw(seed) switches to the device route (see the module docstring); in training it always launches the two kernels - the
    gate's decision is a word of the parameter block, and a step it rejects copies (or, in place, changes nothing).
    If `x.requires_grad` the call goes through an autograd Function whose backward is the same kernel on the gradient."""

    def __init__(self, use_h, use_w, rotate=1, offset=False, ratio=0.5, mode=0, prob=1., out_dtype=None, inplace=False,
                 torch_ops=False):
        super().__init__()
        self.use_h = use_h
        self.use_w = use_w
        self.rotate = rotate
        self.offset = offset
        self.ratio = ratio
        self.mode = mode
        self.st_prob = prob
        self.prob = prob
        self.l = None                                        # the last drawn band width, as in the reference (:92)
        self.torch_ops = bool(torch_ops)
        if out_dtype is not None and out_dtype not in _HALF:
            raise ValueError(f'GridMask: out_dtype is None, torch.float16 or torch.bfloat16, got {out_dtype}')
        self.out_dtype, self.inplace = out_dtype, bool(inplace)
        if self.inplace and out_dtype is not None:
            raise ValueError('GridMask: inplace=True writes into x and cannot change its dtype')
        if mode not in (0, 1):
            raise ValueError(f'GridMask: mode is 0 or 1, got {mode}')
        if rotate != 1:                                      # raises Gd4dError unless the torch-op route was chosen
            Fn.torch_ops_route(f'GridMask(rotate={rotate}): the kernel covers the angle 0 only (rotate=1, what every config and the '
                               'detector use); construct it with torch_ops=True', False, module=self)
        self._seed = None                                    # device route: the seed, then the tensors once a device is known
        self._state = self._block = self._thresh_host = None

    def set_prob(self, epoch, max_epoch):
        self.prob = self.st_prob * epoch / max_epoch
        if self._state is not None:
            self._write_threshold()

    # ------------------------------------------------------------------------------------------------------------------------
    def host_draw(self, h, w):
        """The reference's draws in the reference's order (:85, 91-95, 107, 118), on the host, no GPU needed: None when the gate (or
        eval mode) returns the input - np.random.rand() is consumed either way -, else dict(d, l, st_h, st_w, angle, offset) with
        offset the (h, w) fp32 map 2 (rand - 0.5) or None.  Sets `self.l`."""
        if np.random.rand() > self.prob or not self.training:
            return None
        d = int(np.random.randint(2, h))
        self.l = min(max(int(d * self.ratio + 0.5), 1), d - 1)
        st_h = int(np.random.randint(d))
        st_w = int(np.random.randint(d))
        angle = int(np.random.randint(self.rotate))
        off = (2 * (np.random.rand(h, w) - 0.5)).astype(np.float32) if self.offset else None
        return dict(d=d, l=self.l, st_h=st_h, st_w=st_w, angle=angle, offset=off)

    def device_draw(self, seed):
        """Draw on the device from now on: `seed` (64 bits) and a step counter starting at 0 live in device memory, every training
        forward issues gd4d_grid_mask_draw + gd4d_grid_mask_fwd on the current stream.  Both are capturable."""
        if self.torch_ops or self.rotate != 1:
            raise _lib.Gd4dError('GridMask.device_draw: the torch-op route draws on the host (torch_ops=True was chosen)')
        self._seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self._state = self._block = None
        return self

    def _write_threshold(self):
        self._thresh_host = torch.tensor([_as_i32(prob_threshold(self.prob))], dtype=torch.int32).pin_memory()
        self._state[3:4].copy_(self._thresh_host, non_blocking=True)       # asynchronous; outside capture (set_prob's time)

    def _device_state(self, device):
        if self._state is None or self._state.device != device:
            words = [_as_i32(self._seed), _as_i32(self._seed >> 32), 0, _as_i32(prob_threshold(self.prob))]
            self._state = torch.tensor(words, dtype=torch.int32, device=device)
            self._block = torch.zeros(ops.GRID_MASK_BLOCK_WORDS, dtype=torch.int32, device=device)
        return self._state, self._block

    def device_state(self):
        """(state (4,) int32 {seed_lo, seed_hi, step, thresh}, block (8,) int32) of the device route, None before its first forward."""
        return self._state, self._block

    # ------------------------------------------------------------------------------------------------------------------------
    def _reference_ops(self, x):
        """The reference's op sequence (:84-123): the mask as an array on the host, through PIL, cropped, uploaded, multiplied."""
        from PIL import Image
        if np.random.rand() > self.prob or not self.training:
            return x
        n, c, h, w = x.size()
        hh, ww = int(1.5 * h), int(1.5 * w)
        d = np.random.randint(2, h)
        self.l = min(max(int(d * self.ratio + 0.5), 1), d - 1)
        mask = np.ones((hh, ww), np.float32)
        st_h, st_w = np.random.randint(d), np.random.randint(d)
        for use, st, size, axis in ((self.use_h, st_h, hh, 0), (self.use_w, st_w, ww, 1)):
            for i in range(size // d if use else 0):
                band = slice(d * i + st, min(d * i + st + self.l, size))
                mask[(band, slice(None)) if axis == 0 else (slice(None), band)] = 0
        angle = np.random.randint(self.rotate)
        mask = np.asarray(Image.fromarray(np.uint8(mask)).rotate(angle))
        top, left = (hh - h) // 2, (ww - w) // 2
        mask = torch.from_numpy(np.ascontiguousarray(mask[top:top + h, left:left + w])).float().to(x.device)
        if self.mode == 1:
            mask = 1 - mask
        y = x.view(-1, h, w)
        mask = mask.expand_as(y)
        if self.offset:
            off = torch.from_numpy(2 * (np.random.rand(h, w) - 0.5)).float().to(x.device)
            y = y * mask + off * (1 - mask)
        else:
            y = y * mask
        y = y.view(n, c, h, w)
        return y if self.out_dtype is None else y.to(self.out_dtype)

    def _run(self, x, kw):
        if self.inplace:
            if x.requires_grad:
                raise _lib.Gd4dError('GridMask(inplace=True): x requires grad; use inplace=False for an input that trains')
            return ops.grid_mask_fwd(x, out=x, **kw)
        out_dtype = self.out_dtype if x.dtype == torch.float32 else None     # a 16-bit input stays what it is
        if x.requires_grad and torch.is_grad_enabled():
            return _GridMaskFunction.apply(x, kw, out_dtype)
        return ops.grid_mask_fwd(x, out_dtype=out_dtype, **kw)

    def forward(self, x):
        if Fn.torch_ops_route('GridMask', True, module=self):
            return self._reference_ops(x)
        if x.dim() != 4:
            raise ValueError(f'GridMask: x (N, C, H, W) expected, got {tuple(x.shape)}')
        if not x.is_cuda:
            raise _lib.Gd4dError('GridMask: x must live on the GPU (no CPU fallback in graph-detr4d_amd)')
        h, w = x.shape[-2:]
        base = dict(use_h=self.use_h, use_w=self.use_w, mode=self.mode)
        if self._seed is not None:                           # the device route
            if not self.training:
                return x
            if not x.is_contiguous():
                x = x.contiguous()
            state, block = self._device_state(x.device)
            ops.grid_mask_draw(state, block, h, self.ratio)
            if x.requires_grad and torch.is_grad_enabled():
                block = block.clone()                        # the backward's parameters: the next step overwrites the module's block
            return self._run(x, dict(base, block=block, gen_offset=bool(self.offset)))
        draw = self.host_draw(h, w)
        if draw is None:
            return x
        if not x.is_contiguous():
            if self.inplace:
                raise ValueError('GridMask(inplace=True): x must be contiguous')
            x = x.contiguous()
        off = None
        if draw['offset'] is not None:
            off = torch.from_numpy(draw['offset']).to(x.device, non_blocking=True)
        return self._run(x, dict(base, d=draw['d'], l=draw['l'], st_h=draw['st_h'], st_w=draw['st_w'], offset=off))
