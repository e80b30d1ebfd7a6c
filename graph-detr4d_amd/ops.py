"""Tensor-level wrappers over the C ABI: torch supplies device memory and the stream, nothing else.

Every function requires CUDA(HIP)-resident, contiguous tensors and raises otherwise - the product
path has no CPU fallback.

The wrapper convention, stated once.  A wrapper checks shapes, allocates what it returns, marshals, and launches with _call:
  _call(entry, *args)   looks `entry` up on _lib.load() AT CALL TIME (so a StepRecorder or any other _lib.recording stand-in takes
                        the call), passes args and the current stream of the current device as the last argument, and raises
                        Gd4dError in the entry's name unless the code is 0.  Entries without a trailing stream, size queries
                        (*_bytes, *_tiles) and the one wrapper that looks at the code before it is checked are written out.
  _dev(t, name, dtype)  the pointer argument of a tensor: Gd4dError unless it lives on the GPU, TypeError unless it has `dtype`
                        (None: any), ValueError unless it is contiguous - in that order.  _opt is _dev that hands None through as
                        a null pointer (dtype defaults to F32); _order_ptr does the same for a query order.
  _out(out, shape, ..)  the tensor to write: a new one, or the caller's after a ValueError if its shape is not `shape` (its device,
                        dtype and layout are _dev's business when it is passed).
  _levels / _range6 / _ptrs  the tables: c_int32[2 L] of (H, W) per level from pairs or from tensors' last two dimensions,
                        c_double[6], and c_void_p[n] with every entry checked by _dev (a None entry is a null only with
                        optional=True).  They are ctypes arrays; StepRecorder.steps takes bytes() of them.
"""
import ctypes
import functools
import inspect
import weakref

import torch

from . import _lib, switches

F32, I32, U8 = torch.float32, torch.int32, torch.uint8


def _dev(t, name, dtype=None):
    if not t.is_cuda:
        raise _lib.Gd4dError(f'{name} must live on the GPU (no CPU fallback in graph-detr4d_amd)')
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f'{name} must be {dtype}, got {t.dtype}')
    if not t.is_contiguous():
        raise ValueError(f'{name} must be contiguous')
    return ctypes.c_void_p(t.data_ptr())


def _opt(t, name, dtype=F32):
    return None if t is None else _dev(t, name, dtype)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _call(entry, *args):
    _lib.check(getattr(_lib.load(), entry)(*args, _stream()), entry)


def _out(out, shape, device, what, dtype=F32):
    if out is None:
        return torch.empty(shape, device=device, dtype=dtype)
    if tuple(out.shape) != tuple(shape):
        raise ValueError(f'{what} must be {tuple(shape)}, got {tuple(out.shape)}')
    return out


def _levels(seq):
    flat = [int(x) for e in seq for x in (e.shape[-2:] if torch.is_tensor(e) else e)]
    return (ctypes.c_int32 * len(flat))(*flat)


def _range6(pc_range):
    return (ctypes.c_double * 6)(*[float(x) for x in pc_range])


def _ptrs(tensors, name, dtype=F32, optional=False):
    vals = [None if optional and t is None else _dev(t, f'{name}[{i}]', dtype).value for i, t in enumerate(tensors)]
    return (ctypes.c_void_p * len(vals))(*vals)


def _camera_args(ref, offsets, attn_logits, cam_logits, lidar2img, pc_range, img_h, img_w):
    """The run of arguments the cross-attention entry points share, for *-splicing."""
    return (_dev(ref, 'ref', F32), _dev(offsets, 'offsets', F32), _dev(attn_logits, 'attn_logits', F32),
            _dev(cam_logits, 'cam_logits', F32), _dev(lidar2img, 'lidar2img', F32), _range6(pc_range), float(img_h), float(img_w))


def _asked(res, *optional, bare=True):
    """res (a tuple) + the optional results that were asked for (the others are None); bare: a lone result is not wrapped."""
    res += tuple(o for o in optional if o is not None)
    return res[0] if bare and len(res) == 1 else res


def _mask_uv(want_mask, want_uv, mask_out, uv_out, shape, device):
    """The optional mask (shape, uint8) and uv (shape + (2,)) of the cross-attention front ends: new, the caller's, or None."""
    mask = _out(mask_out, shape, device, 'mask_out', U8) if want_mask or mask_out is not None else None
    uv = _out(uv_out, tuple(shape) + (2,), device, 'uv_out') if want_uv or uv_out is not None else None
    return mask, uv


def _value_dtype(t):
    if t.dtype == F32:
        return _lib.F32
    if t.dtype == torch.bfloat16:
        return _lib.BF16
    raise TypeError(f'value tensors must be float32 or bfloat16, got {t.dtype}')


def cross_attn_fwd(value, level_hw, ref, offsets, attn_logits, cam_logits, lidar2img, pc_range,
                   img_h, img_w, want_mask=False, want_uv=False, out=None, head_major=False, query_order=None,
                   raw_cam_weights=False, mask_out=None, uv_out=None):
    """gd4d_cross_attn_fwd.  value (B*N, S, Hh, Dh), or (B*N, Hh, S, Dh) with head_major=True;
    ref (B,Q,3); offsets (B,Q,Hh,P,3);
    attn_logits (B,Q,Hh,L,P) (or (B,Q,Hh,L*P)); cam_logits (B,Q,N); lidar2img (B,N,4,4).
    query_order: optional int32 permutation of [0, B*Q) from query_order_fwd (scheduling only, same result).
    out / mask_out / uv_out: the tensors to write (mask_out / uv_out: asked for by being given).
    Returns out (B,Q,Hh*Dh) [, mask (B,N,Q,Hh,P) uint8] [, uv (B,N,Q,Hh,P,2)]."""
    b, q = ref.shape[0], ref.shape[1]
    n = lidar2img.shape[1]
    hh, dh = (value.shape[1], value.shape[3]) if head_major else (value.shape[2], value.shape[3])
    p = offsets.shape[3]
    nl = len(level_hw)
    if value.shape[0] != b * n or value.shape[2 if head_major else 1] != sum(h * w for h, w in level_hw):
        raise ValueError(f'value shape {tuple(value.shape)} inconsistent with B*N={b * n}, '
                         f'levels {level_hw}')
    if attn_logits.numel() != b * q * hh * nl * p or cam_logits.numel() != b * q * n:
        raise ValueError('attn_logits / cam_logits have the wrong number of elements')
    out = _out(out, (b, q, hh * dh), ref.device, 'out')
    mask, uv = _mask_uv(want_mask, want_uv, mask_out, uv_out, (b, n, q, hh, p), ref.device)
    _call('gd4d_cross_attn_fwd', _dev(value, 'value'), _levels(level_hw),
          *_camera_args(ref, offsets, attn_logits, cam_logits, lidar2img, pc_range, img_h, img_w), _dev(out, 'out', F32),
          _opt(mask, 'mask', None), _opt(uv, 'uv', None), b, n, q, hh, dh, nl, p, _value_dtype(value),
          _lib.HEAD_MAJOR if head_major else _lib.PIXEL_MAJOR, 1 if raw_cam_weights else 0, _order_ptr(query_order, b * q))
    return _asked((out,), mask, uv)


def pyramid_channels_last_fwd(feats, out=None, max_cus=0, out_dtype=torch.float32):
    """gd4d_pyramid_channels_last_fwd.  feats: list of L tensors (R, 256, H_l, W_l) fp32 (or (B, N, 256, H, W)).
    max_cus > 0: one persistent workgroup on each of that many compute units (the rest stays free for another stream).
    out_dtype torch.bfloat16: bf16 storage of the copy (reduced precision; the aggregate kernel accumulates in fp32).
    Returns (cl (R, S, 256), level_hw)."""
    fl = [f.reshape(-1, *f.shape[-3:]) for f in feats]
    r, c = fl[0].shape[0], fl[0].shape[1]
    level_hw = [(int(f.shape[-2]), int(f.shape[-1])) for f in fl]
    s = sum(h * w for h, w in level_hw)
    if any(f.shape[0] != r or f.shape[1] != c for f in fl):
        raise ValueError('feature levels disagree in rows / channels')
    if out is None:
        out = torch.empty(r, s, c, device=fl[0].device, dtype=out_dtype)
    ptrs = _ptrs(fl, 'feats')
    lv = _levels(level_hw)
    _call('gd4d_pyramid_channels_last_fwd', ptrs, lv, _dev(out, 'out'), r, c, len(fl), _lib.F32, _value_dtype(out), int(max_cus))
    return out, level_hw


def cross_attn_agg_fwd(feats_cl, level_hw, ref, offsets, attn_logits, cam_logits, lidar2img, pc_range, img_h, img_w,
                       num_heads, want_mask=False, want_uv=False, query_order=None, raw_cam_weights=False,
                       vp_weight=None, vp_bias=None, outs=None, mask_out=None, uv_out=None):
    """gd4d_cross_attn_agg_fwd.  feats_cl (B*N, S, 256) fp32 channels-last pyramid; the other arguments as cross_attn_fwd.
    Returns agg (B, Q, Hh, 256), wsum (B, Q, Hh) [, mask] [, uv]; with vp_weight (256, 256) [, vp_bias]: value_proj of the
    aggregates applied in the kernel's epilogue - returns out (B, Q, 256) [, mask] [, uv] instead.
    outs: the tensors to write, (agg, wsum) - or (out,) with vp_weight; mask_out / uv_out as cross_attn_fwd."""
    b, q = ref.shape[0], ref.shape[1]
    n = lidar2img.shape[1]
    hh, p = num_heads, offsets.shape[3]
    nl = len(level_hw)
    c = feats_cl.shape[-1]
    if feats_cl.shape[0] != b * n or feats_cl.shape[1] != sum(h * w for h, w in level_hw):
        raise ValueError(f'feats_cl shape {tuple(feats_cl.shape)} inconsistent with B*N={b * n}, levels {level_hw}')
    if offsets.numel() != b * q * hh * p * 3 or attn_logits.numel() != b * q * hh * nl * p or cam_logits.numel() != b * q * n:
        raise ValueError('offsets / attn_logits / cam_logits have the wrong number of elements')
    fused = vp_weight is not None
    if outs is not None and len(outs) != (1 if fused else 2):
        raise ValueError('outs must be (agg, wsum), or (out,) with vp_weight')
    given = (None, None) if outs is None else tuple(outs)
    agg = None if fused else _out(given[0], (b, q, hh, c), ref.device, 'outs[0]')
    wsum = None if fused else _out(given[1], (b, q, hh), ref.device, 'outs[1]')
    out = _out(given[0], (b, q, c), ref.device, 'outs[0]') if fused else None
    mask, uv = _mask_uv(want_mask, want_uv, mask_out, uv_out, (b, n, q, hh, p), ref.device)
    _call('gd4d_cross_attn_agg_fwd', _dev(feats_cl, 'feats_cl'), _levels(level_hw),
          *_camera_args(ref, offsets, attn_logits, cam_logits, lidar2img, pc_range, img_h, img_w), _opt(agg, 'agg', None),
          _opt(wsum, 'wsum', None), _opt(mask, 'mask', None), _opt(uv, 'uv', None), b, n, q, hh, c, nl, p, _value_dtype(feats_cl),
          1 if raw_cam_weights else 0, _order_ptr(query_order, b * q), _opt(vp_weight, 'vp_weight'),
          _opt(vp_bias, 'vp_bias') if fused else None, _opt(out, 'out', None))
    return _asked((out,) if fused else (agg, wsum), mask, uv, bare=False)


def pyramid_slice_planar_fwd(feats, out=None, max_cus=0, out_dtype=torch.float32):
    """gd4d_pyramid_slice_planar_fwd.  feats as pyramid_channels_last_fwd.  Returns (sp (8, R, S, 32), level_hw): the
    channels-last pyramid with the channel axis cut into 8 planes of 32 (the layout gd4d_cross_attn_agg_sliced_fwd
    gathers from when it has to make its own copy)."""
    fl = [f.reshape(-1, *f.shape[-3:]) for f in feats]
    r, c = fl[0].shape[0], fl[0].shape[1]
    level_hw = [(int(f.shape[-2]), int(f.shape[-1])) for f in fl]
    s = sum(h * w for h, w in level_hw)
    if any(f.shape[0] != r or f.shape[1] != c for f in fl):
        raise ValueError('feature levels disagree in rows / channels')
    if c != 256:
        raise ValueError('the slice-planar copy is built for 256 channels')
    if out is None:
        out = torch.empty(8, r, s, 32, device=fl[0].device, dtype=out_dtype)
    ptrs = _ptrs(fl, 'feats')
    lv = _levels(level_hw)
    _call('gd4d_pyramid_slice_planar_fwd', ptrs, lv, _dev(out, 'out'), r, c, len(fl), _lib.F32, _value_dtype(out), int(max_cus))
    return out, level_hw


class PyramidView:
    """How gd4d_cross_attn_agg_sliced_fwd addresses a 256-channel pyramid: per-level base pointers + byte strides
    (include/gd4d.h).  Three sources: the slice-planar copy, the pixel-major copy, caller-owned channels-last levels
    read in place."""

    def __init__(self, tensors, ptrs, level_hw, cam_stride, pix_stride, slice_stride, dtype, rows):
        self.tensors, self.ptrs, self.level_hw = tensors, ptrs, [tuple(int(x) for x in hw) for hw in level_hw]
        self.cam_stride, self.pix_stride, self.slice_stride = [int(x) for x in cam_stride], int(pix_stride), int(slice_stride)
        self.dtype, self.rows = dtype, int(rows)

    @property
    def device(self):
        return self.tensors[0].device

    @staticmethod
    def _starts(level_hw):
        out, s = [], 0
        for h, w in level_hw:
            out.append(s)
            s += h * w
        return out, s

    @classmethod
    def slice_planar(cls, sp, level_hw):
        """sp (8, R, S, 32) from pyramid_slice_planar_fwd."""
        es = sp.element_size()
        starts, s = cls._starts(level_hw)
        if sp.dim() != 4 or sp.shape[0] != 8 or sp.shape[2] != s or sp.shape[3] != 32 or not sp.is_contiguous():
            raise ValueError(f'slice-planar pyramid {tuple(sp.shape)} inconsistent with levels {level_hw}')
        r = sp.shape[1]
        return cls([sp], [sp.data_ptr() + st * 32 * es for st in starts], level_hw, [s * 32 * es] * len(starts), 32 * es,
                   r * s * 32 * es, sp.dtype, r)

    @classmethod
    def pixel_major(cls, cl, level_hw):
        """cl (R, S, 256) from pyramid_channels_last_fwd."""
        es = cl.element_size()
        starts, s = cls._starts(level_hw)
        if cl.dim() != 3 or cl.shape[1] != s or cl.shape[2] != 256 or not cl.is_contiguous():
            raise ValueError(f'channels-last pyramid {tuple(cl.shape)} inconsistent with levels {level_hw}')
        return cls([cl], [cl.data_ptr() + st * 256 * es for st in starts], level_hw, [s * 256 * es] * len(starts), 256 * es,
                   32 * es, cl.dtype, cl.shape[0])

    @staticmethod
    def is_channels_last_level(t):
        """(..., 256, H, W) whose memory is (..., H, W, 256): what `x.permute(.., 2, 3, 1).contiguous().permute(.., 3, 1, 2)`
        or torch.channels_last on the (rows, C, H, W) view gives."""
        if t.dim() not in (4, 5) or t.shape[-3] != 256:
            return False
        c, h, w = t.shape[-3:]
        want = {-3: 1, -1: c, -2: w * c}
        if t.dim() == 5:
            want[1], want[0] = h * w * c, t.shape[1] * h * w * c
        else:
            want[0] = h * w * c
        return all(t.shape[d] == 1 or t.stride(d) == st for d, st in want.items())   # (the stride of a size-1 dim is free)

    @classmethod
    def channels_last_levels(cls, levels):
        """levels: L tensors (B, N, 256, H, W) or (R, 256, H, W) with channels-last strides, fp32 or bf16: no copy."""
        if not all(cls.is_channels_last_level(t) for t in levels) or len({t.dtype for t in levels}) != 1:
            raise ValueError('channels_last_levels needs (.., 256, H, W) tensors stored as (.., H, W, 256), one dtype')
        es = levels[0].element_size()
        rows = levels[0].numel() // (256 * levels[0].shape[-1] * levels[0].shape[-2])
        hw = [(int(t.shape[-2]), int(t.shape[-1])) for t in levels]
        return cls(list(levels), [t.data_ptr() for t in levels], hw, [h * w * 256 * es for h, w in hw], 256 * es, 32 * es,
                   levels[0].dtype, rows)


def cross_attn_plan_bytes(b, n, q, num_heads, points=4):
    return int(_lib.load().gd4d_cross_attn_plan_bytes(b, n, q, num_heads, points))


class Plan:
    """Output of cross_attn_plan_fwd: the plan buffer, the locality order it is stored by, the pyramid it addresses and
    wsum (B, Q, Hh) - the sum of the in-bounds sampling weights per head (items form: filled by the gather, not by the
    plan kernel).  items: the buffer holds the ITEMS form (include/gd4d.h, GD4D_CA_PLAN_ITEMS) - gather only; the
    training backward kernels need the pairs form."""

    def __init__(self, buf, order, pyramid, b, q, num_heads, wsum, items=False, points=4, items_buf=None):
        self.buf, self.order, self.pyramid, self.b, self.q, self.num_heads, self.wsum = buf, order, pyramid, b, q, num_heads, wsum
        self.items, self.points = bool(items), int(points)
        self.items_buf = items_buf           # both=True: `buf` holds the pairs, this view the items (the forward gather's form)

    def need_pairs(self, who):
        if self.items:
            raise _lib.Gd4dError(f'{who} reads the pairs form of the plan; this one was made with items=True')
        if self.points not in (4, 8) or (self.points == 8 and self.num_heads != 8):
            raise _lib.Gd4dError(f'{who} is built for 4 points per head (every shipped config) and for 8 with 8 heads; this plan has '
                                 f'{self.points} - functional.pad_points pads other counts up to them')


CA_RAW_CAM_WEIGHTS, CA_PLAN_ITEMS, CA_PLAN_BOTH = 1, 2, 16


def cross_attn_plan_fwd(pyramid, ref, offsets, attn_logits, cam_logits, lidar2img, pc_range, img_h, img_w, num_heads,
                        want_mask=False, want_uv=False, raw_cam_weights=False, plan=None, query_order=None, items=False,
                        both=False, mask_out=None, uv_out=None):
    """gd4d_cross_attn_plan_fwd: projection + mask + softmax + camera weights + bilinear corners of one decoder layer's
    cross-attention -> what gd4d_cross_attn_agg_sliced_fwd walks on `pyramid` (a PyramidView).  The other arguments as
    cross_attn_fwd; plan: a Plan to overwrite; items: the 32-bytes-per-item form (the corners are worked out by the gather,
    which then also fills wsum).  both: pairs AND items in one launch (a training step: the forward gather reads the items, the
    backward kernels the pairs).  mask_out / uv_out as cross_attn_fwd.
    Returns Plan [, mask (B, N, Q, Hh, P) uint8] [, uv (B, N, Q, Hh, P, 2)]."""
    b, q = ref.shape[0], ref.shape[1]
    n = lidar2img.shape[1]
    hh, p, nl = num_heads, offsets.shape[3], len(pyramid.level_hw)
    if pyramid.rows != b * n:
        raise ValueError(f'pyramid has {pyramid.rows} camera rows, expected B*N = {b * n}')
    if offsets.numel() != b * q * hh * p * 3 or attn_logits.numel() != b * q * hh * nl * p or cam_logits.numel() != b * q * n:
        raise ValueError('offsets / attn_logits / cam_logits have the wrong number of elements')
    nbytes = cross_attn_plan_bytes(b, n, q, hh, p)
    if both and (items or plan is not None):
        raise ValueError('both=True excludes items / plan')
    buf = torch.empty(2 * nbytes if both else nbytes, device=ref.device, dtype=U8) if plan is None else plan.buf
    wsum = torch.empty(b, q, hh, device=ref.device, dtype=F32) if plan is None else plan.wsum
    plan = Plan(buf, query_order, pyramid, b, q, hh, wsum, items=items, points=p, items_buf=buf[nbytes:] if both else None)
    mask, uv = _mask_uv(want_mask, want_uv, mask_out, uv_out, (b, n, q, hh, p), ref.device)
    cs = (ctypes.c_int64 * nl)(*pyramid.cam_stride)
    _call('gd4d_cross_attn_plan_fwd', *_camera_args(ref, offsets, attn_logits, cam_logits, lidar2img, pc_range, img_h, img_w),
          _levels(pyramid.level_hw), cs, pyramid.pix_stride, _dev(buf, 'plan', U8), buf.numel(), _dev(wsum, 'wsum', F32),
          _opt(mask, 'mask', None), _opt(uv, 'uv', None), b, n, q, hh, nl, p,
          (CA_RAW_CAM_WEIGHTS if raw_cam_weights else 0) | (CA_PLAN_ITEMS if items else 0) | (CA_PLAN_BOTH if both else 0),
          _order_ptr(query_order, b * q))
    return _asked((plan,), mask, uv)


def cross_attn_agg_sliced_fwd(plan, slices=(0, 8), agg=None, count=None):
    """gd4d_cross_attn_agg_sliced_fwd on the pyramid the Plan was made for.  Returns agg (B, Q, Hh, 256); with plan.wsum
    (B, Q, Hh) that is what cross_attn_agg_fwd returns (other summation order).
    count = (PyramidGrad, layer): a training step's forward - the records of this plan get their slots in the SAME launch
    (gd4d_cross_attn_agg_items_count_fwd; needs the plan in both forms, 8 heads, 4 levels, fp32; PyramidGrad.add_layer otherwise)."""
    lib = _lib.load()
    pyramid = plan.pyramid
    dev = pyramid.device
    b, q, hh, query_order = plan.b, plan.q, plan.num_heads, plan.order
    if not plan.buf.is_cuda or plan.buf.device != dev:
        raise _lib.Gd4dError('plan must live on the pyramid\'s GPU (no CPU fallback in graph-detr4d_amd)')
    nl = len(pyramid.level_hw)
    if agg is None:
        agg = torch.empty(b, q, hh, 256, device=dev, dtype=F32)
    ptrs = (ctypes.c_void_p * nl)(*pyramid.ptrs)
    if plan.items or plan.items_buf is not None:
        lv = _levels(pyramid.level_hw)
        cs = (ctypes.c_int64 * nl)(*pyramid.cam_stride)
        if count is not None:
            sink, layer = count
            if plan.items or plan.items_buf is None or tuple(slices) != (0, 8):
                raise _lib.Gd4dError('gather + record count in one launch: a plan in both forms, all slices')
            slots, slot_bytes = sink.begin_layer(layer, plan)
            code = lib.gd4d_cross_attn_agg_items_count_fwd(
                ptrs, lv, cs, pyramid.pix_stride, pyramid.slice_stride, _dev(plan.items_buf, 'plan', U8), _dev(agg, 'agg', F32),
                _dev(plan.wsum, 'wsum', F32), b, pyramid.rows // b, q, hh, 256, nl, plan.points,
                _lib.F32 if pyramid.dtype == F32 else _lib.BF16,
                _order_ptr(query_order, b * q), _dev(plan.buf, 'plan', U8),
                _dev(sink.count, 'count', I32), _dev(slots, 'slots'), ctypes.c_size_t(slot_bytes), _stream())
            if code == -2:                               # GD4D_EUNSUPPORTED (e.g. a pyramid of 4 GiB or more): the caller launches the two
                return None
            _lib.check(code, 'gd4d_cross_attn_agg_items_count_fwd')
            sink.plans.append((int(layer), plan, slots))
            return agg
        items_buf = _dev(plan.buf if plan.items else plan.items_buf, 'plan', U8)
        dt = _lib.F32 if pyramid.dtype == F32 else _lib.BF16
        order_p = _order_ptr(query_order, b * q)
        _call('gd4d_cross_attn_agg_items_fwd', ptrs, lv, cs, pyramid.pix_stride, pyramid.slice_stride, items_buf, _dev(agg, 'agg', F32),
              _dev(plan.wsum, 'wsum', F32), b, pyramid.rows // b, q, hh, 256, nl, plan.points, dt, order_p, int(slices[0]), int(slices[1]))
        return agg
    _call('gd4d_cross_attn_agg_sliced_fwd', ptrs, pyramid.slice_stride, _dev(plan.buf, 'plan', U8), _dev(agg, 'agg', F32), b,
          pyramid.rows // b, q, hh, 256, nl, plan.points, _lib.F32 if pyramid.dtype == F32 else _lib.BF16, _order_ptr(query_order, b * q),
          int(slices[0]), int(slices[1]))
    return agg


class CoarseValues:
    """Levels 2, 3 of a pyramid with one layer's value_proj already applied (bias included): `rows` (R, S23, 256) fp32,
    level 2's pixels first - what gd4d_value_proj_fwd over those two levels writes (GD4D_LAYOUT_PIXEL_MAJOR)."""

    def __init__(self, rows, level_hw):
        (h2, w2), (h3, w3) = level_hw
        if rows.dim() != 3 or rows.shape[1] != h2 * w2 + h3 * w3 or rows.shape[2] != 256 or rows.dtype != F32 \
                or not rows.is_contiguous():
            raise ValueError(f'projected coarse levels {tuple(rows.shape)} inconsistent with {level_hw}')
        self.rows, self.level_hw = rows, [(int(h2), int(w2)), (int(h3), int(w3))]
        self.ptrs = [rows.data_ptr(), rows.data_ptr() + h2 * w2 * 1024]
        self.cam_stride = [rows.shape[1] * 1024] * 2


def coarse_supported(plan):
    """gd4d_cross_attn_agg_items_coarse_fwd: items plan, 4 levels, 8 heads."""
    return plan.items and len(plan.pyramid.level_hw) == 4 and plan.num_heads == 8


def cross_attn_agg_coarse_fwd(plan, coarse, agg=None, pagg=None, reverse=False):
    """gd4d_cross_attn_agg_items_coarse_fwd: levels 0, 1 gathered raw from the Plan's pyramid, levels 2, 3 from `coarse`
    (CoarseValues of THIS layer's value_proj).  Returns agg (B, Q, 8, 256), pagg (B, Q, 256); plan.wsum holds the fine levels'
    weight sums: value_proj_heads_fwd(agg, plan.wsum, W, b) + pagg is the layer's sampled value.  reverse: the launch walks its
    slice groups from last to first (GD4D_GATHER_REVERSED; the same bits)."""
    pyramid = plan.pyramid
    dev = pyramid.device
    b, q, hh, query_order = plan.b, plan.q, plan.num_heads, plan.order
    if not coarse_supported(plan):
        raise _lib.Gd4dError('the coarse-projected gather takes an items plan over 4 levels with 8 heads')
    if list(coarse.level_hw) != [tuple(x) for x in pyramid.level_hw[2:]] or coarse.rows.shape[0] != pyramid.rows \
            or coarse.rows.device != dev:
        raise ValueError('projected coarse levels do not belong to this pyramid')
    if agg is None:
        agg = torch.empty(b, q, hh, 256, device=dev, dtype=F32)
    if pagg is None:
        pagg = torch.empty(b, q, 256, device=dev, dtype=F32)
    ptrs = (ctypes.c_void_p * 4)(*pyramid.ptrs)
    lv = _levels(pyramid.level_hw)
    cs = (ctypes.c_int64 * 4)(*pyramid.cam_stride)
    pp = (ctypes.c_void_p * 2)(*coarse.ptrs)
    pcs = (ctypes.c_int64 * 2)(*coarse.cam_stride)
    _call('gd4d_cross_attn_agg_items_coarse_fwd', ptrs, lv, cs, pyramid.pix_stride, pyramid.slice_stride, pp, pcs,
          _dev(plan.buf, 'plan', U8), _dev(agg, 'agg', F32), _dev(plan.wsum, 'wsum', F32), _dev(pagg, 'pagg', F32), b, pyramid.rows // b, q,
          hh, 256, 4, plan.points, (_lib.F32 if pyramid.dtype == F32 else _lib.BF16) | (_lib.GATHER_REVERSED if reverse else 0),
          _order_ptr(query_order, b * q))
    return agg, pagg


def value_proj_heads_fwd(agg, wsum, weight, bias=None, out=None):
    """gd4d_value_proj_heads_fwd: agg (..., Hh, 256), wsum (..., Hh) -> out (..., 256) = value_proj of the aggregates."""
    hh, c = agg.shape[-2], agg.shape[-1]
    m = agg.numel() // (hh * c)
    if out is None:
        out = torch.empty(*agg.shape[:-2], c, device=agg.device, dtype=F32)
    _call('gd4d_value_proj_heads_fwd', _dev(agg, 'agg', F32), _dev(wsum, 'wsum', F32), _dev(weight, 'weight', F32), _opt(bias, 'bias'),
          _dev(out, 'out', F32), m, hh, c)
    return out


def value_proj_heads_bwd(grad_out, weight, bias=None, num_heads=8, grad_agg=None, beta=None):
    """gd4d_value_proj_heads_bwd: grad_out (..., 256) -> grad_agg (..., Hh, 256) = W_h^T grad_out[.., h], beta (..., Hh) =
    <b_h, grad_out[.., h]> (zeros without a bias): the gradient of value_proj_heads_fwd w.r.t. agg and wsum."""
    c = grad_out.shape[-1]
    m = grad_out.numel() // c
    if grad_agg is None:
        grad_agg = torch.empty(*grad_out.shape[:-1], num_heads, c, device=grad_out.device, dtype=F32)
    if beta is None:
        beta = torch.empty(*grad_out.shape[:-1], num_heads, device=grad_out.device, dtype=F32)
    _call('gd4d_value_proj_heads_bwd', _dev(grad_out, 'grad_out', F32), _dev(weight, 'weight', F32), _opt(bias, 'bias'),
          _dev(grad_agg, 'grad_agg', F32), _dev(beta, 'beta', F32), m, num_heads, c)
    return grad_agg, beta


def value_proj_heads_bwd_weight(grad_out, agg, wsum=None, want_bias=True, into=None):
    """gd4d_value_proj_heads_bwd_weight: grad_out (..., 256), agg (..., Hh, 256), wsum (..., Hh) -> (grad_weight (256, 256),
    grad_bias (256) or None): value_proj's gradients from the per-head aggregates of the forward pass.  into=(w_buf, b_buf):
    added to these instead."""
    lib = _lib.load()
    hh, c = agg.shape[-2], agg.shape[-1]
    m = grad_out.numel() // c
    if into is None:
        gw = torch.empty(c, c, device=grad_out.device, dtype=F32)
        gb = torch.empty(c, device=grad_out.device, dtype=F32) if want_bias else None
    else:
        gw, gb = into[0], (into[1] if want_bias else None)
    wsb = int(lib.gd4d_value_proj_heads_bwd_weight_workspace_bytes())
    ws = torch.empty(wsb, device=grad_out.device, dtype=U8)
    _call('gd4d_value_proj_heads_bwd_weight', _dev(grad_out, 'grad_out', F32), _dev(agg, 'agg', F32),
          _dev(wsum, 'wsum', F32) if want_bias else None, _dev(gw, 'grad_weight', F32), _dev(gb, 'grad_bias', F32) if want_bias else None,
          _dev(ws, 'workspace'), ctypes.c_size_t(wsb), m, hh, c, 0 if into is None else 1)
    return gw, gb


def value_proj_heads_bwd_weight_group(problems, accumulate=True):
    """gd4d_value_proj_heads_bwd_weight_group: problems = list (<= 8) of (grad_out (..., 256), agg (..., Hh, 256), wsum (..., Hh),
    grad_weight (256, 256), grad_bias (256) or None) - value_proj's gradients of several layers in one pair of launches, added to
    (accumulate) or written into the targets."""
    lib = _lib.load()
    n = len(problems)
    hh, c = problems[0][1].shape[-2], problems[0][1].shape[-1]
    dev = problems[0][0].device
    nbytes = n * int(lib.gd4d_value_proj_heads_bwd_weight_workspace_bytes())
    ws = torch.empty(nbytes, device=dev, dtype=U8)             # (scratch of this call only: see _vp_workspace)
    gos, aggs, wsums, gws, gbs = zip(*problems)
    rows = (ctypes.c_int32 * n)(*[int(g.numel() // c) for g in gos])
    _call('gd4d_value_proj_heads_bwd_weight_group', _ptrs(gos, 'grad_out'), _ptrs(aggs, 'agg'), _ptrs(wsums, 'wsum'),
          _ptrs(gws, 'grad_weight'), _ptrs(gbs, 'grad_bias', optional=True), rows, n, _dev(ws, 'workspace'), ctypes.c_size_t(nbytes), hh, c,
          1 if accumulate else 0)


def cross_attn_dot_bytes(b, n, q, num_heads, points=4):
    return int(_lib.load().gd4d_cross_attn_dot_bytes(b, n, q, num_heads, points))


def _wgrad_arrays(problems):
    """The C arrays of gd4d_linear_bwd_weight_group for problems = [(x (M, K), grad_y (M, N), grad_w (N, K), grad_b (N) or None)]."""
    n = len(problems)
    dims = []
    for x, gy, gw, gb in problems:
        k, nn_ = x.shape[-1], gy.shape[-1]
        m = x.numel() // k
        if gy.numel() // nn_ != m or tuple(gw.shape) != (nn_, k) or (gb is not None and gb.numel() != nn_):
            raise ValueError('weight-gradient group: inconsistent shapes')
        dims += [m, k, nn_, k, nn_]
    xs, gys, gws, gbs = zip(*problems) if n else [()] * 4
    return (_ptrs(xs, 'x'), _ptrs(gys, 'grad_y'), _ptrs(gws, 'grad_w'), _ptrs(gbs, 'grad_b', optional=True),
            (ctypes.c_int32 * (5 * n))(*dims), n)


def cross_attn_dot_sliced(plan, grad_agg, dpart=None, wgrads=None):
    """gd4d_cross_attn_dot_sliced: D[pair] = <grad_agg[q, h], raw pixel of the pair> for every pair of `plan`, as 8 per-slice
    partials (uint8 buffer of gd4d_cross_attn_dot_bytes; only the passes the plan uses are written).
    wgrads: up to 16 weight-gradient problems (as linear_bwd_weight_group takes them; added to their targets) whose tiles ride
    in the launch (gd4d_cross_attn_dot_sliced_wgrad; 8 heads, 4 levels, fp32: wgrads_ride_with(plan) says whether)."""
    lib = _lib.load()
    plan.need_pairs('gd4d_cross_attn_dot_sliced')
    pyramid = plan.pyramid
    b, q, hh = plan.b, plan.q, plan.num_heads
    n = pyramid.rows // b
    nl = len(pyramid.level_hw)
    nbytes = int(lib.gd4d_cross_attn_dot_bytes(b, n, q, hh, plan.points))
    if dpart is None:
        dpart = torch.empty(nbytes, device=pyramid.device, dtype=U8)
    ptrs = (ctypes.c_void_p * nl)(*pyramid.ptrs)
    if wgrads:
        xs, gys, gws, gbs, dims, cnt = _wgrad_arrays(wgrads)
        _call('gd4d_cross_attn_dot_sliced_wgrad', ptrs, pyramid.slice_stride, _dev(plan.buf, 'plan', U8), _dev(grad_agg, 'grad_agg', F32),
              _dev(dpart, 'dpart', U8), dpart.numel(), b, n, q, hh, 256, nl, plan.points, _lib.F32 if pyramid.dtype == F32 else _lib.BF16,
              _order_ptr(plan.order, b * q), xs, gys, gws, gbs, dims, cnt, 1)
        return dpart
    _call('gd4d_cross_attn_dot_sliced', ptrs, pyramid.slice_stride, _dev(plan.buf, 'plan', U8), _dev(grad_agg, 'grad_agg', F32),
          _dev(dpart, 'dpart', U8), dpart.numel(), b, n, q, hh, 256, nl, plan.points, _lib.F32 if pyramid.dtype == F32 else _lib.BF16,
          _order_ptr(plan.order, b * q))
    return dpart


def wgrads_ride_with(plan):
    """Whether cross_attn_dot_sliced(plan, ..., wgrads=...) has a launch for this plan's shape."""
    return plan.num_heads == 8 and len(plan.pyramid.level_hw) == 4 and plan.pyramid.dtype == F32


def cross_attn_plan_bwd(plan, dpart, beta, ref, offsets, attn_logits, cam_logits, lidar2img, pc_range, img_h, img_w,
                        raw_cam_weights=False, status=None, outs=None, workspace=None):
    """gd4d_cross_attn_plan_bwd: the query-side gradients of the sliced path from D (cross_attn_dot_sliced) and beta.
    outs: the four tensors to write; workspace: a uint8 buffer of gd4d_cross_attn_bwd_workspace_bytes (0 bytes with B = 1: none).
    Returns (grad_ref, grad_offsets, grad_attn_logits, grad_cam_logits) - what cross_attn_bwd returns after grad_value."""
    lib = _lib.load()
    plan.need_pairs('gd4d_cross_attn_plan_bwd')
    b, q, hh = plan.b, plan.q, plan.num_heads
    n = lidar2img.shape[1]
    p = offsets.shape[3]
    level_hw = plan.pyramid.level_hw
    nl = len(level_hw)
    dev = ref.device
    gr, go, ga, gc = _query_grads(outs, 0, (b, q, 3), (b, q, hh, p, 3), (b, q, hh, nl, p), (b, q, n), dev)
    nbytes = lib.gd4d_cross_attn_bwd_workspace_bytes(b, q, hh, nl, p)
    ws = _out(workspace, (nbytes,), dev, 'workspace', U8) if nbytes else None
    _call('gd4d_cross_attn_plan_bwd', *_camera_args(ref, offsets, attn_logits, cam_logits, lidar2img, pc_range, img_h, img_w),
          _levels(level_hw), _dev(plan.buf, 'plan', U8), _dev(dpart, 'dpart', U8), _opt(beta, 'beta'), _dev(gr, 'grad_ref'),
          _dev(go, 'grad_offsets'), _dev(ga, 'grad_attn_logits'), _dev(gc, 'grad_cam_logits'), _opt(ws, 'workspace', None),
          ctypes.c_size_t(nbytes), _opt(status, 'status', I32), b, n, q, hh, nl, p, 1 if raw_cam_weights else 0,
          _order_ptr(plan.order, b * q))
    return gr, go, ga, gc


def _query_grads(outs, first, *shapes_dev):
    """grad_ref, grad_offsets, grad_attn_logits, grad_cam_logits of the two cross-attention backwards: new, or outs[first:]."""
    *shapes, dev = shapes_dev
    if outs is not None and len(outs) != first + 4:
        raise ValueError(f'outs must hold {first + 4} tensors')
    return tuple(_out(None if outs is None else outs[first + i], s, dev, f'outs[{first + i}]') for i, s in enumerate(shapes))


_CHUNK_WALKS = {}


def _chunk_walk(level_hw, rows, device, regions=(6, 10)):
    """The order gd4d_pyramid_grad_reduce walks the chunks in: camera by camera, and inside a camera image region by image
    region (regions[0] x regions[1] per image) with ALL levels of a region together - the workgroups an XCD runs at one
    time then need the table rows of the few queries that look at one region, not of a whole camera (level-major, the
    64 chunks in flight per XCD cover most of a camera's coarse maps: 77 % L2 hits, 2.8 GB from the fabric per pass).
    Cached per geometry (an int32 permutation on the device)."""
    import numpy as np
    key = (tuple(level_hw), int(rows), str(device), regions)
    hit = _CHUNK_WALKS.get(key)
    if hit is not None:
        return hit
    lib = _lib.load()
    nl = len(level_hw)
    lv = _levels(level_hw)
    geo = (ctypes.c_int32 * (5 * nl))()
    _lib.check(lib.gd4d_pyramid_grad_chunk_geometry(lv, int(rows), nl, geo), 'gd4d_pyramid_grad_chunk_geometry')
    keys, ids = [], []
    span = max(int(geo[5 * l + 2]) * int(geo[5 * l + 3]) for l in range(nl))
    for l, (h, w) in enumerate(level_hw):
        cws, chs, cw_n, ch_n, base = geo[5 * l:5 * l + 5]
        r, cy, cx = np.meshgrid(np.arange(rows), np.arange(ch_n), np.arange(cw_n), indexing='ij')
        v = np.minimum((cy + 0.5) * (1 << chs) / h, 0.999999)
        u = np.minimum((cx + 0.5) * (1 << cws) / w, 0.999999)
        ry, rx = (v * regions[0]).astype(np.int64), (u * regions[1]).astype(np.int64)
        rx = np.where(ry % 2 == 1, regions[1] - 1 - rx, rx)                        # boustrophedon: neighbours stay neighbours
        k = (((r * regions[0] + ry) * regions[1] + rx) * nl + (nl - 1 - l)) * span + cy * cw_n + cx
        keys.append(k.reshape(-1))
        ids.append((base + (r * ch_n + cy) * cw_n + cx).reshape(-1))
    keys, ids = np.concatenate(keys), np.concatenate(ids)
    walk = torch.from_numpy(ids[np.argsort(keys, kind='stable')].astype(np.int32)).to(device)
    _CHUNK_WALKS[key] = walk
    return walk


class PyramidGrad:
    """The gradient of an NCHW pyramid from the plans of all decoder layers (gd4d_pyramid_grad_count / _scan / _fill /
    _reduce): add_layer() per layer (in any order, each with its plan and its grad_agg rows), finish() once.

    Buffers are sized for `layers` layers of B*Q*Hh rows (alloc_table with a list: per-layer Q); the slot / record buffers by
    the plans' capacity (8 bytes per pair a plan can hold - only what the counts say is touched).
    alloc(what, shape, dtype, zero): every buffer this object owns comes from it (what: 'count', 'table', 'slots', 'start',
    'scan_workspace', 'records', 'sorted', 'pxoff'; zero: the buffer must hold zeros); default: torch.zeros / torch.empty on the
    pyramid's device."""

    def _alloc(self, what, shape, dtype, zero):
        return (torch.zeros if zero else torch.empty)(shape, device=self.pyramid.device, dtype=dtype)

    def __init__(self, pyramid, layers, b, q, num_heads, chunk_walk=True, points=4, alloc=None):
        self.pyramid, self.layers, self.b, self.q, self.hh = pyramid, int(layers), int(b), int(q), int(num_heads)
        self.alloc = self._alloc if alloc is None else alloc
        self.points = int(points)                 # points per head of the plans this sink takes (4, or 8 with 8 heads)
        dev = pyramid.device
        lib = _lib.load()
        self.n = pyramid.rows // self.b
        nl = len(pyramid.level_hw)
        self._lv = _levels(pyramid.level_hw)
        self._cs = (ctypes.c_int64 * nl)(*pyramid.cam_stride)
        self.chunks = int(lib.gd4d_pyramid_grad_chunks(self._lv, pyramid.rows, nl))
        if self.chunks <= 0:
            raise _lib.Gd4dError('gd4d_pyramid_grad_chunks: unsupported pyramid')
        self.count = self.alloc('count', (self.chunks,), I32, True)
        self._scanned, self._riding = None, []
        self.table, self.layer_q = None, {}
        if self.layers > 0:
            self.alloc_table(self.layers)
        self.slot_bytes = int(lib.gd4d_pyramid_grad_slots_bytes(self.b, self.n, self.q, self.hh, self.points))
        self.plans, self.prepared = [], None
        self.order = _chunk_walk(pyramid.level_hw, pyramid.rows, dev) if chunk_walk else None

    def alloc_table(self, layers):
        """The grad_agg table (zeros: a layer whose backward never runs contributes nothing).  layers: a count (every layer
        has the constructor's Q) or a list of per-layer query counts - the passes of Detr3DTransformer.forward_shared share
        one pyramid but need not have the same number of queries (teacher_queries, detr3d_head_pe.py:560-566)."""
        qs = [self.q] * int(layers) if isinstance(layers, int) else [int(x) for x in layers]
        for layer, q in self.layer_q.items():
            if layer < len(qs) and qs[layer] != q:
                raise _lib.Gd4dError(f'PyramidGrad: layer {layer} was counted with {q} queries, the table is asked for {qs[layer]}')
        self.layers = len(qs)
        self.table_q = qs
        self.row_base = [0]
        for q in qs:
            self.row_base.append(self.row_base[-1] + self.b * q * self.hh)
        if self.row_base[-1] >= 1 << 26:
            raise _lib.Gd4dError('PyramidGrad: more than 2^26 table rows (a record keeps its row in 26 bits)')
        self.table = self.alloc('table', (max(self.row_base[-1], 1), 256), F32, True)

    def grad_agg_rows(self, layer):
        """(B, Q_layer, Hh, 256) view of the table: where layer `layer`'s gd4d_value_proj_heads_bwd writes."""
        return self.table[self.row_base[layer]:self.row_base[layer + 1]].view(self.b, self.table_q[layer], self.hh, 256)

    def add_layer(self, layer, plan):
        """Hand every record of `plan` its slot (the plan is kept until finish(): its buffer must not be overwritten).  The
        plan's own (B, Q, Hh) say where its pairs are; B and Hh must be the sink's (they fix the pyramid rows / the table's
        row width), Q is per layer."""
        slots, slot_bytes = self.begin_layer(layer, plan)
        layer = int(layer)
        _call('gd4d_pyramid_grad_count', _dev(plan.buf, 'plan', U8), self._lv, self._cs, self.pyramid.pix_stride,
              _dev(self.count, 'count', I32), _dev(slots, 'slots'), ctypes.c_size_t(slot_bytes), self.b, self.n, plan.q, self.hh,
              len(self.pyramid.level_hw), plan.points)
        self.plans.append((layer, plan, slots))

    def begin_layer(self, layer, plan):
        """The checks of add_layer and the layer's slot buffer (the count itself: add_layer, or the forward gather's launch -
        cross_attn_agg_sliced_fwd(count=...), which then appends to self.plans)."""
        lib = _lib.load()
        plan.need_pairs('gd4d_pyramid_grad_count')
        layer = int(layer)
        if plan.b != self.b or plan.num_heads != self.hh or plan.pyramid.rows != self.pyramid.rows:
            raise _lib.Gd4dError(f'PyramidGrad: plan of (B, Hh, rows) = ({plan.b}, {plan.num_heads}, {plan.pyramid.rows}) handed to a '
                                 f'sink of ({self.b}, {self.hh}, {self.pyramid.rows})')
        if self.table is not None and (layer >= self.layers or self.table_q[layer] != plan.q):
            raise _lib.Gd4dError(f'PyramidGrad: layer {layer} has {plan.q} queries, the table was made for '
                                 f'{self.table_q[layer] if layer < self.layers else "fewer layers"}')
        self.layer_q[layer] = plan.q
        if plan.points != self.points:
            raise _lib.Gd4dError(f'PyramidGrad: a plan with {plan.points} points per head handed to a sink made for {self.points}')
        slot_bytes = int(lib.gd4d_pyramid_grad_slots_bytes(self.b, self.n, plan.q, self.hh, plan.points))
        slots = self.alloc('slots', (slot_bytes,), U8, False)
        return slots, slot_bytes

    def prepare(self):
        """scan + fill + sort: the layers' records bucketed by chunk and grouped by pixel.  Needs the counts of every layer
        (add_layer) and nothing from the backward pass."""
        if self._scanned is None:
            self.scan()
        self.finish_prepare()

    def scan(self):
        """The first part of prepare(): the chunks' starts.  The fills may then ride in other launches (take_fills ->
        mha_core_bwd(fills=...)); finish_prepare() launches whatever is left of them, and the sort."""
        lib = _lib.load()
        dev = self.pyramid.device
        start = self.alloc('start', (self.chunks,), I32, False)
        wsb = int(lib.gd4d_pyramid_grad_scan_workspace_bytes(self.chunks))
        ws = self.alloc('scan_workspace', (wsb,), U8, False)
        _call('gd4d_pyramid_grad_scan', _dev(self.count, 'count', I32), _dev(start, 'start', I32), _dev(ws, 'workspace'),
              ctypes.c_size_t(wsb), self.chunks)
        if self.table is None:
            raise _lib.Gd4dError('PyramidGrad.prepare: alloc_table() first (the records carry table rows)')
        nbytes = max(sum(slots.numel() for _, _, slots in self.plans), self.slot_bytes)
        self._scanned = (start, self.alloc('records', (nbytes,), U8, False), nbytes)
        for layer, plan, slots in self.plans:
            if layer >= self.layers or self.table_q[layer] != plan.q:
                raise _lib.Gd4dError(f'PyramidGrad: layer {layer} ({plan.q} queries) does not match the table')

    def take_fills(self, n):
        """Up to n (<= 2) pending fills for another launch to carry: ([(plan, slots, first table row)], start, records, B, N, Hh),
        or None when none is left."""
        n = min(int(n), 2, len(self.plans))
        if n <= 0 or self._scanned is None:
            return None
        start, records, _ = self._scanned
        jobs = [(plan, slots, self.row_base[layer]) for layer, plan, slots in self.plans[:n]]
        self._riding += self.plans[:n]                     # (their buffers live until finish_prepare)
        self.plans = self.plans[n:]
        return jobs, start, records, self.b, self.n, self.hh

    def finish_prepare(self):
        dev = self.pyramid.device
        start, records, nbytes = self._scanned
        for layer, plan, slots in self.plans:
            _call('gd4d_pyramid_grad_fill', _dev(plan.buf, 'plan', U8), _dev(slots, 'slots'), _dev(start, 'start', I32),
                  _dev(records, 'records'), self.row_base[layer], _order_ptr(plan.order, self.b * plan.q), self.b, self.n, plan.q, self.hh,
                  plan.points)
        sorted_ = self.alloc('sorted', (nbytes,), U8, False)
        pxoff = self.alloc('pxoff', (self.chunks, 65), I32, False)
        _call('gd4d_pyramid_grad_sort', _dev(self.count, 'count', I32), _dev(start, 'start', I32), _dev(records, 'records'),
              _dev(sorted_, 'sorted'), _dev(pxoff, 'pxoff', I32), self.chunks)
        self.prepared = (start, pxoff, sorted_)
        self.plans = []
        self._riding = []
        self._scanned = None

    def reduce(self, grads=None, channels_last=False):
        """-> L tensors (R, 256, H_l, W_l) fp32: the pyramid's gradient summed over the layers (prepare() first; the table
        rows of every layer must have been written).  channels_last: the tensors are stored (R, H_l, W_l, 256) - the layout of
        levels the gather read in place - and returned as (R, 256, H_l, W_l) views of that memory."""
        py = self.pyramid
        nl = len(py.level_hw)
        start, pxoff, sorted_ = self.prepared
        if grads is None:
            grads = [torch.empty((py.rows, h, w, 256) if channels_last else (py.rows, 256, h, w), device=py.device, dtype=F32)
                     for h, w in py.level_hw]
        ptrs = _ptrs(grads, 'grads')
        _call('gd4d_pyramid_grad_reduce', _dev(start, 'start', I32), _dev(pxoff, 'pxoff', I32), _dev(sorted_, 'sorted'),
              _dev(self.table, 'table', F32), ptrs, self._lv, _opt(self.order, 'chunk_order', I32), py.rows, 256, nl,
              1 if channels_last else 0)
        self.prepared = None
        return [g.permute(0, 3, 1, 2) for g in grads] if channels_last else grads

    def finish(self, grads=None, channels_last=False):
        self.prepare()
        return self.reduce(grads, channels_last)


def _order_ptr(order, count):
    if order is None:
        return None
    if order.dtype != I32 or order.numel() != count:
        raise ValueError(f'query_order must be an int32 permutation of {count} entries')
    return _dev(order, 'query_order')


def query_order_fwd(ref, pc_range, out=None):
    """gd4d_query_order_fwd: ref (B,Q,3) in [0,1] -> int32 (B*Q) locality order for cross_attn_fwd(query_order=)."""
    b, q = ref.shape[0], ref.shape[1]
    if out is None:
        out = torch.empty(b * q, device=ref.device, dtype=I32)
    _call('gd4d_query_order_fwd', _dev(ref, 'ref', F32), _range6(pc_range), _order_ptr(out, b * q), b, q)
    return out


def _detr3d_args(feats, ref, attn_logits, lidar2img, pc_range, img_h, img_w, offsets=None):
    """The leading arguments the four detr3d entry points share (offsets: the v2 pair's, after attn_logits), for *-splicing."""
    off = () if offsets is None else (_dev(offsets, 'offsets', F32),)
    return (_ptrs(feats, 'feats'), _levels(feats), _dev(ref, 'ref', F32), _dev(attn_logits, 'attn_logits', F32), *off,
            _dev(lidar2img, 'lidar2img', F32), _range6(pc_range), float(img_h), float(img_w))


def detr3d_fwd(feats, ref, attn_logits, lidar2img, pc_range, img_h, img_w, want_out=True,
               want_mask=False, want_sampled=False):
    """gd4d_detr3d_fwd.  feats: list of L tensors (B, N, C, H_l, W_l) fp32 (NCHW per camera);
    ref (B,Q,3); attn_logits (B,Q,N,1,L) (any shape with B*Q*N*L elements in that order).
    Returns a dict with the requested 'out' (B,Q,C), 'mask' (B,N,Q) uint8,
    'sampled' (B,C,Q,N,1,L)."""
    b, n, c = feats[0].shape[:3]
    q = ref.shape[1]
    nl = len(feats)
    if attn_logits.numel() != b * q * n * nl:
        raise ValueError('attn_logits must have B*Q*N*L elements (num_points must be 1)')
    dev = ref.device
    out = torch.empty(b, q, c, device=dev, dtype=F32) if want_out else None
    mask = torch.empty(b, n, q, device=dev, dtype=U8) if want_mask else None
    sampled = torch.empty(b, c, q, n, 1, nl, device=dev, dtype=F32) if want_sampled else None
    _call('gd4d_detr3d_fwd', *_detr3d_args(feats, ref, attn_logits, lidar2img, pc_range, img_h, img_w), _opt(out, 'out', None),
          _opt(mask, 'mask', None), _opt(sampled, 'sampled', None), b, n, q, c, nl, 1)
    return dict(out=out, mask=mask, sampled=sampled)


def detr3d_bwd(feats, ref, attn_logits, lidar2img, pc_range, img_h, img_w, grad_out, want_feats=True, want_ref=True):
    """gd4d_detr3d_bwd: gradients of detr3d_fwd(...)['out'].  Returns (grad_feats: list like feats or None,
    grad_logits like attn_logits, grad_ref (B, Q, 3) or None)."""
    b, n, c = feats[0].shape[:3]
    q = ref.shape[1]
    nl = len(feats)
    gf = [torch.zeros_like(f) for f in feats] if want_feats else None
    gl = torch.empty(b * q * n * nl, device=ref.device, dtype=F32).view_as(attn_logits)
    gr = torch.empty(b, q, 3, device=ref.device, dtype=F32) if want_ref else None
    _call('gd4d_detr3d_bwd', *_detr3d_args(feats, ref, attn_logits, lidar2img, pc_range, img_h, img_w), _dev(grad_out, 'grad_out', F32),
          _ptrs(gf, 'grad_feats') if want_feats else None, _dev(gl, 'grad_logits'), _opt(gr, 'grad_ref', None), b, n, q, c, nl, 1)
    return gf, gl, gr


def detr3d_v2_fwd(feats, ref, attn_logits, offsets, lidar2img, pc_range, img_h, img_w, num_heads, want_mask=False):
    """gd4d_detr3d_v2_fwd.  feats: list of L tensors (B, N, C, H_l, W_l) fp32; attn_logits (B, Q, N, Hh, L*P);
    offsets (B, Q, N, Hh, L, P, 2), P == L.  Returns out (B, Q, C) [, mask (B, N, Q) uint8]."""
    b, n, c = feats[0].shape[:3]
    q = ref.shape[1]
    nl = len(feats)
    if attn_logits.numel() != b * q * n * num_heads * nl * nl or offsets.numel() != 2 * attn_logits.numel():
        raise ValueError('attn_logits / offsets must be (B, Q, N, heads, L*P) / (..., L, P, 2) with P == L')
    out = torch.empty(b, q, c, device=ref.device, dtype=F32)
    mask = torch.empty(b, n, q, device=ref.device, dtype=U8) if want_mask else None
    _call('gd4d_detr3d_v2_fwd', *_detr3d_args(feats, ref, attn_logits, lidar2img, pc_range, img_h, img_w, offsets), _dev(out, 'out'),
          _opt(mask, 'mask', None), b, n, q, c, int(num_heads), nl, nl)
    return (out, mask) if want_mask else out


def detr3d_v2_bwd(feats, ref, attn_logits, offsets, lidar2img, pc_range, img_h, img_w, num_heads, grad_out, want_feats=True,
                  want_ref=True):
    """gd4d_detr3d_v2_bwd: the gradients of detr3d_v2_fwd's `out`.  Returns (grad_feats list or None, grad_attn_logits
    (B, Q, N, Hh, L*P), grad_offsets (B, Q, N, Hh, L, P, 2), grad_ref (B, Q, 3) or None).  C <= 256."""
    b, n, c = feats[0].shape[:3]
    q = ref.shape[1]
    nl = len(feats)
    gfeats = [torch.zeros_like(f) for f in feats] if want_feats else None
    gl = torch.empty(b, q, n, num_heads, nl * nl, device=ref.device, dtype=F32)
    go = torch.empty(b, q, n, num_heads, nl, nl, 2, device=ref.device, dtype=F32)
    gr = torch.empty(b, q, 3, device=ref.device, dtype=F32) if want_ref else None
    _call('gd4d_detr3d_v2_bwd', *_detr3d_args(feats, ref, attn_logits, lidar2img, pc_range, img_h, img_w, offsets),
          _dev(grad_out, 'grad_out', F32), _ptrs(gfeats, 'grad_feats') if want_feats else None, _dev(gl, 'grad_logits'),
          _dev(go, 'grad_offsets'), _opt(gr, 'grad_ref', None), b, n, q, c, nl, int(num_heads))
    return gfeats, gl, go, gr


def _vp_workspace(nlayers, device):
    """Scratch for the weight fragments of a value_proj launch (rewritten by every call: stream-ordered, so a fresh
    tensor per call keeps concurrent launches on different streams apart; the caching allocator makes it free)."""
    nbytes = _lib.load().gd4d_value_proj_workspace_bytes(int(nlayers))
    return torch.empty(nbytes, device=device, dtype=U8), nbytes


def value_proj_fwd(feats, weight, bias, out_dtype=torch.float32, out=None, num_heads=8, head_major=False,
                   bf16_math=False, max_cus=0):
    """gd4d_value_proj_fwd.  feats: list of L tensors (B, N, C, H_l, W_l) or (R, C, H_l, W_l) fp32;
    weight (C, C); bias (C) or None.  Returns (R, S, C) in `out_dtype`, or (R, Hh, S, C/Hh) with
    head_major=True.  max_cus: occupy at most that many CUs (0 = all)."""
    o = value_proj_multi_fwd(feats, [weight], [bias], out_dtype, num_heads, head_major, bf16_math, max_cus,
                             outs=None if out is None else [out])
    return o[0]


def value_proj_multi_fwd(feats, weights, biases, out_dtype=torch.float32, num_heads=8, head_major=False,
                         bf16_math=False, max_cus=0, outs=None):
    """gd4d_value_proj_multi_fwd: project the same pyramid with NL (weight, bias) pairs in one
    launch.  Returns a list of NL tensors (R, S, C) (or (R, Hh, S, C/Hh) with head_major=True)."""
    nlayers = len(weights)
    c = weights[0].shape[0]
    r = feats[0].numel() // (c * feats[0].shape[-1] * feats[0].shape[-2])
    nl = len(feats)
    s = sum(f.shape[-1] * f.shape[-2] for f in feats)
    shape = (r, num_heads, s, c // num_heads) if head_major else (r, s, c)
    if outs is None:
        outs = [torch.empty(*shape, device=weights[0].device, dtype=out_dtype) for _ in range(nlayers)]
    ws, nbytes = _vp_workspace(nlayers, weights[0].device)
    ptrs = _ptrs(feats, 'feats')
    lv = _levels(feats)
    wp = _ptrs(weights, 'weight')
    bp = _ptrs(biases, 'bias', optional=True)
    op = _ptrs(outs, 'out', None)
    _call('gd4d_value_proj_multi_fwd', ptrs, lv, wp, bp, op, r, c, nl, nlayers, num_heads, _lib.F32, _value_dtype(outs[0]),
          _lib.HEAD_MAJOR if head_major else _lib.PIXEL_MAJOR, int(bool(bf16_math)), _dev(ws, 'workspace'), ctypes.c_size_t(nbytes),
          int(max_cus))
    return outs


def linear_bwd_weight(x, grad_y, want_bias=True, into=None):
    """gd4d_linear_bwd_weight.  x (..., K), grad_y (..., N) fp32 with the same leading shape (contiguous rows).
    Returns (grad_w (N, K), grad_b (N) or None).  into=(w_buf, b_buf or None): the sums are ADDED to these tensors (views
    of a flat gradient buffer) and returned."""
    k, n = x.shape[-1], grad_y.shape[-1]
    m = x.numel() // k
    if grad_y.numel() // n != m:
        raise ValueError('x and grad_y must have the same number of rows')
    if into is None:
        gw = torch.empty(n, k, device=x.device, dtype=F32)
        gb = torch.empty(n, device=x.device, dtype=F32) if want_bias else None
    else:
        gw, gb = into
        if tuple(gw.shape) != (n, k) or (want_bias and (gb is None or gb.numel() != n)):
            raise ValueError('linear_bwd_weight: the accumulation targets do not match the gradient shapes')
        gb = gb if want_bias else None
    _call('gd4d_linear_bwd_weight', _dev(x, 'x', F32), _dev(grad_y, 'grad_y', F32), _dev(gw, 'grad_w', F32), _opt(gb, 'grad_b'), m, k, n, k,
          n, 0 if into is None else 1)
    return gw, gb


def linear_bwd_weight_group(problems, accumulate=True):
    """gd4d_linear_bwd_weight_group: problems = list (<= 16) of (x (M, K), grad_y (M, N), grad_w (N, K), grad_b (N) or None);
    the sums are added to (accumulate) or written into grad_w / grad_b.  One launch for all of them."""
    xs, gys, gws, gbs, dims, n = _wgrad_arrays(problems)
    _call('gd4d_linear_bwd_weight_group', xs, gys, gws, gbs, dims, n, 1 if accumulate else 0)


def value_proj_bwd_input(grad_out, weight, shapes, grads=None, accumulate=False):
    """gd4d_value_proj_bwd_input.  grad_out (R, S, C) fp32; weight (C, C); shapes: per level (H_l, W_l).
    Returns the list of L gradients (R, C, H_l, W_l); with `grads` given they are written (accumulate=False) or added
    to (accumulate=True) in place."""
    c = weight.shape[0]
    r = grad_out.numel() // (c * sum(h * w for h, w in shapes))
    nl = len(shapes)
    if grads is None:
        if accumulate:
            raise ValueError('accumulate=True needs the tensors to add to')
        grads = [torch.empty(r, c, h, w, device=grad_out.device, dtype=F32) for h, w in shapes]
    ptrs = _ptrs(grads, 'grads')
    lv = _levels(shapes)
    _call('gd4d_value_proj_bwd_input', _dev(grad_out, 'grad_out', F32), _dev(weight, 'weight', F32), ptrs, lv, r, c, nl,
          int(bool(accumulate)))
    return grads


def value_proj_bwd_weight(grad_out, feats, want_bias=True):
    """gd4d_value_proj_bwd_weight.  grad_out (R, S, C) fp32; feats: the L NCHW levels the forward read.
    Returns (grad_weight (C, C), grad_bias (C) or None)."""
    lib = _lib.load()
    c = feats[0].shape[-3]
    nl = len(feats)
    r = feats[0].numel() // (c * feats[0].shape[-1] * feats[0].shape[-2])
    dev = grad_out.device
    nbytes = lib.gd4d_value_proj_bwd_weight_workspace_bytes()
    ws = torch.empty(nbytes, device=dev, dtype=U8)             # (scratch of this call only: see _vp_workspace)
    gw = torch.empty(c, c, device=dev, dtype=F32)
    gb = torch.empty(c, device=dev, dtype=F32) if want_bias else None
    ptrs = _ptrs(feats, 'feats')
    lv = _levels(feats)
    _call('gd4d_value_proj_bwd_weight', _dev(grad_out, 'grad_out', F32), ptrs, lv, _dev(gw, 'grad_weight'), _opt(gb, 'grad_bias', None),
          _dev(ws, 'workspace'), ctypes.c_size_t(nbytes), r, c, nl)
    return gw, gb


def linear_fwd(x, weight, bias=None, x2=None, n_split=None, relu=False, r1=None, r2=None, out=None,
               inv_sigmoid_in=False, weight_kn=False, want_xsum=False):
    """gd4d_linear_fwd on the last dimension: y = act((x [+ x2 for cols < n_split]) W^T + b) [+r1] [+r2].
    x (..., K) contiguous - or 2-D with a row stride (a column slice of a wider buffer, e.g. the q|k part of a packed
    gradient); weight (N, K); residuals (..., N) contiguous.  Returns (..., N); with want_xsum (needs x2): (y, x + x2)."""
    k = x.shape[-1]
    n = weight.shape[1] if weight_kn else weight.shape[0]      # weight_kn: weight is (K, N) - y = x W (a Linear's dgrad)
    if weight_kn and weight.shape[0] != k:
        raise ValueError('weight_kn: weight must be (K, N) with K = x.shape[-1]')
    m = x.numel() // k
    ldx = k
    if not x.is_contiguous():
        if x.dim() != 2 or x.stride(1) != 1 or x.stride(0) < k or x2 is not None:
            raise ValueError('x must be contiguous, or 2-D with unit column stride (and no x2)')
        ldx = x.stride(0)
    if out is None:
        out = torch.empty(*x.shape[:-1], n, device=x.device, dtype=F32)
    if x2 is not None and x2.shape != x.shape:
        raise ValueError('x2 must have the shape of x')
    xsum = None
    if want_xsum:
        if x2 is None:
            raise ValueError('want_xsum needs x2')
        xsum = torch.empty(x.shape, device=x.device, dtype=F32)
    xptr = _dev(x, 'x', F32) if ldx == k else _devptr_strided(x, 'x')
    _call('gd4d_linear_fwd', xptr, _opt(x2, 'x2'), _dev(weight, 'weight', F32), _opt(bias, 'bias'), _opt(r1, 'r1'), _opt(r2, 'r2'),
          _dev(out, 'out'), m, k, n, n if n_split is None else int(n_split),
          int(bool(relu)) | (2 if inv_sigmoid_in else 0) | (8 if weight_kn else 0), ldx, n, n, n, _opt(xsum, 'xsum', None))
    return (out, xsum) if want_xsum else out


def _devptr_strided(t, name):
    if not t.is_cuda or t.dtype != F32:
        raise _lib.Gd4dError(f'{name}: fp32 device tensor expected, got {t.dtype} on {t.device}')
    return ctypes.c_void_p(t.data_ptr())


def linear_group_fwd(x, weights, biases, x2=None, want_xsum=False):
    """gd4d_linear_group_fwd: [(x + x2) W_g^T + b_g for g] in one launch.  x (..., K) contiguous; returns a list
    (want_xsum, needs x2: (list, x + x2))."""
    g = len(weights)
    k = x.shape[-1]
    m = x.numel() // k
    if x2 is not None and x2.shape != x.shape:
        raise ValueError('x2 must have the shape of x')
    if want_xsum and x2 is None:
        raise ValueError('want_xsum needs x2')
    outs = [torch.empty(*x.shape[:-1], w.shape[0], device=x.device, dtype=F32) for w in weights]
    xsum = torch.empty(x.shape, device=x.device, dtype=F32) if want_xsum else None
    narr = (ctypes.c_int32 * g)(*[w.shape[0] for w in weights])
    _call('gd4d_linear_group_fwd', _dev(x, 'x', F32), _opt(x2, 'x2'), _ptrs(weights, 'weight'), _ptrs(biases, 'bias', optional=True),
          _ptrs(outs, 'out'), narr, g, m, k, k, _opt(xsum, 'xsum', None))
    return (outs, xsum) if want_xsum else outs


def layernorm_fwd(x, gamma, beta, eps=1e-5, res=None, relu=False, out=None):
    """gd4d_layernorm_fwd over the last dimension of a contiguous tensor.  out: the tensor of x's shape to write (default a new one)."""
    c = x.shape[-1]
    out = _out(out, x.shape, x.device, 'layernorm_fwd: out')
    _call('gd4d_layernorm_fwd', _dev(x, 'x', F32), _opt(res, 'res'), _dev(gamma, 'gamma', F32), _dev(beta, 'beta', F32), _dev(out, 'out'),
          x.numel() // c, c, float(eps), int(bool(relu)))
    return out


def linear_ln_fwd(x, weight, bias=None, gamma=None, beta=None, eps=1e-5, x2=None, n_split=None, relu=False, r1=None,
                  r2=None, relu_after_ln=False, out=None):
    """gd4d_linear_ln_fwd: y = [ReLU] LN(act((x [+ x2]) W^T + b) + r1 + r2); gamma=None: no LayerNorm."""
    k, n = x.shape[-1], weight.shape[0]
    m = x.numel() // k
    if out is None:
        out = torch.empty(*x.shape[:-1], n, device=x.device, dtype=F32)
    if x2 is not None and x2.shape != x.shape:
        raise ValueError('x2 must have the shape of x')
    _call('gd4d_linear_ln_fwd', _dev(x, 'x', F32), _opt(x2, 'x2'), _dev(weight, 'weight', F32), _opt(bias, 'bias'), _opt(r1, 'r1'),
          _opt(r2, 'r2'), _opt(gamma, 'gamma'), _opt(beta, 'beta'), _dev(out, 'out'), m, k, n, n if n_split is None else int(n_split),
          int(bool(relu)) | (4 if relu_after_ln else 0), float(eps), k, n, n, n)
    return out


def small_linear_layernorm_fwd(x, weight, bias, gamma, beta, eps=1e-5, relu=False, inv_sigmoid_in=False):
    """gd4d_small_linear_layernorm_fwd: [ReLU] LN(f(x) W^T + b) with x (..., K <= 4) -> (..., C)."""
    k, c = x.shape[-1], weight.shape[0]
    out = torch.empty(*x.shape[:-1], c, device=x.device, dtype=F32)
    _call('gd4d_small_linear_layernorm_fwd', _dev(x, 'x', F32), _dev(weight, 'weight', F32), _opt(bias, 'bias'), _dev(gamma, 'gamma', F32),
          _dev(beta, 'beta', F32), _dev(out, 'out'), x.numel() // k, k, c, float(eps), int(bool(relu)) | (2 if inv_sigmoid_in else 0))
    return out


def _mha_args(q, k, v, num_heads, attn_mask):
    lq, b, c = q.shape
    lk = k.shape[0]
    d = c // num_heads

    def ld(t, name):
        if not t.is_cuda or t.dtype != F32:
            raise _lib.Gd4dError(f'{name} must be a float32 GPU tensor')
        if t.stride(2) != 1 or t.stride(0) != t.stride(1) * t.shape[1]:
            raise ValueError(f'{name} must be row-strided (L, B, C)')
        return t.stride(1)
    kind, mptr = 0, None
    if attn_mask is not None:
        if attn_mask.dim() != 2:
            raise NotImplementedError('only 2-D (Lq, Lk) attention masks are supported')
        if attn_mask.dtype in (torch.bool, U8):
            attn_mask, kind = attn_mask.to(U8), 1
        else:
            attn_mask, kind = attn_mask.float(), 2
        attn_mask = attn_mask.contiguous()
        mptr = _dev(attn_mask, 'attn_mask')
    return lq, lk, b, c, d, ld, kind, mptr, attn_mask


def _mha_seed(dropout_p, seed, device):
    if not dropout_p:
        return None
    if seed is None or seed.dtype != torch.int64 or seed.numel() < 1 or not seed.is_contiguous():
        raise ValueError('dropout_p > 0 needs seed: a contiguous int64 device tensor (mha_dropout_seed)')
    return _dev(seed, 'seed', torch.int64)


def mha_dropout_seed(device):
    """A fresh (1,) int64 device tensor holding the seed of the next dropout mask (its two 32-bit words are what
    gd4d_mha_core_fwd / _bwd read), drawn ON THE DEVICE from torch's generator for that device: torch.manual_seed makes the
    masks repeatable, and a captured launch draws a new seed on every replay (torch advances the generator's offset for
    graphs, as it does for nn.Dropout in the same step)."""
    return torch.randint(-2 ** 62, 2 ** 62, (1,), device=device, dtype=torch.int64)


def mha_dropout_keep_mask(seed, b, num_heads, lq, lk, dropout_p):
    """The (B, heads, Lq, Lk) bool keep mask gd4d_mha_core_fwd draws for this seed (csrc/gd4d_mha_dropout.h restated with
    torch integer ops): what a check against torch's softmax / bmm needs.  Not used by the product path."""
    m32 = 0xFFFFFFFF
    s = int(seed.reshape(-1)[0].item()) & 0xFFFFFFFFFFFFFFFF
    lo, hi = s & m32, (s >> 32) & m32
    ids = torch.arange(b * num_heads * lq * lk, dtype=torch.int64, device=seed.device)
    x = ids ^ lo
    x = (x * 0x9E3779B1) & m32
    x = x ^ (x >> 16)
    x = (x + hi) & m32
    x = (x * 0x85EBCA6B) & m32
    x = x ^ (x >> 13)
    x = (x * 0xC2B2AE35) & m32
    x = x ^ (x >> 16)
    t = dropout_p * 4294967296.0
    thresh = 0 if t <= 0 else (m32 if t >= 4294967295.0 else int(t + 0.5))
    return (x >= thresh).view(b, num_heads, lq, lk)


def mha_core_fwd(q, k, v, num_heads, attn_mask=None, want_lse=False, dropout_p=0., seed=None):
    """gd4d_mha_core_fwd.  q (Lq, B, C), k / v (Lk, B, C): each contiguous or a last-dim slice of a packed
    (L, B, 3C) in-projection buffer.  attn_mask: None, bool/uint8 (Lq, Lk) (nonzero = masked) or float
    additive (Lq, Lk).  Returns (Lq, B, C) [, lse (Lq, B, heads) with want_lse - what mha_core_bwd needs].
    dropout_p, seed (mha_dropout_seed): dropout of the probabilities, as nn.MultiheadAttention in training."""
    lq, lk, b, c, d, ld, kind, mptr, keep = _mha_args(q, k, v, num_heads, attn_mask)
    sptr = _mha_seed(dropout_p, seed, q.device)
    out = torch.empty(lq, b, c, device=q.device, dtype=F32)
    lse = torch.empty(lq, b, num_heads, device=q.device, dtype=F32) if want_lse else None
    _call('gd4d_mha_core_fwd', ctypes.c_void_p(q.data_ptr()), ctypes.c_void_p(k.data_ptr()), ctypes.c_void_p(v.data_ptr()), mptr,
          _dev(out, 'out'), lq, lk, b, num_heads, d, ld(q, 'q'), ld(k, 'k'), ld(v, 'v'), c, kind, 1.0 / (d ** 0.5), _opt(lse, 'lse', None),
          float(dropout_p), sptr)
    return (out, lse) if want_lse else out


class FillJob(ctypes.Structure):
    """gd4d_fill_job (include/gd4d.h)."""
    _fields_ = [('plan', ctypes.c_void_p), ('slots', ctypes.c_void_p), ('query_order', ctypes.c_void_p),
                ('id_base', ctypes.c_uint32), ('Q', ctypes.c_int32)]


def _fill_args(fills):
    """What a launch that carries `fills` (PyramidGrad.take_fills) takes for them: the job table, its length, start, records, B, N, Hh,
    points per head."""
    jobs, start, records, fb, fn, fhh = fills
    arr = (FillJob * len(jobs))(*[FillJob(_dev(pl.buf, 'plan', U8).value, _dev(sl, 'slots').value,
                                          _addr(_order_ptr(pl.order, fb * pl.q)) or None, int(base), int(pl.q)) for pl, sl, base in jobs])
    return arr, len(jobs), _dev(start, 'start', I32), _dev(records, 'records'), fb, fn, fhh, int(jobs[0][0].points)


def mha_core_bwd(q, k, v, out, grad_out, lse, num_heads, attn_mask=None, packed_qk=False, dropout_p=0., seed=None, fills=None):
    """gd4d_mha_core_bwd.  Returns (dq, dk, dv), each (L, B, C) contiguous; packed_qk (self-attention, q and k the two halves
    of one (L, B, 2C) projection): (dqk (L, B, 2C), dv) - the kernel writes both halves of one buffer.  dropout_p / seed:
    the forward's.  fills: what PyramidGrad.take_fills returned - one or two layers' record fills of the pyramid gradient ride
    in the dk / dv launch (gd4d_mha_core_bwd_fill)."""
    lq, lk, b, c, d, ld, kind, mptr, keep = _mha_args(q, k, v, num_heads, attn_mask)
    sptr = _mha_seed(dropout_p, seed, q.device)
    if packed_qk:
        if lq != lk:
            raise ValueError('packed_qk needs as many queries as keys')
        dqk = torch.empty(lq, b, 2 * c, device=q.device, dtype=F32)
        dq, dk, ldd = dqk[..., :c], dqk[..., c:], 2 * c
    else:
        dq = torch.empty(lq, b, c, device=q.device, dtype=F32)
        dk = torch.empty(lk, b, c, device=q.device, dtype=F32)
        ldd = c
    dv = torch.empty(lk, b, c, device=q.device, dtype=F32)
    dsum = torch.empty(lq, b, num_heads, device=q.device, dtype=F32)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())    # noqa: E731
    fargs = () if fills is None else _fill_args(fills)
    _call('gd4d_mha_core_bwd' if fills is None else 'gd4d_mha_core_bwd_fill', vp(q), vp(k), vp(v), _dev(out, 'out', F32),
          _dev(grad_out, 'grad_out', F32), mptr, _dev(lse, 'lse', F32), _dev(dsum, 'dsum'), vp(dq), vp(dk), _dev(dv, 'dv'), lq, lk, b,
          num_heads, d, ld(q, 'q'), ld(k, 'k'), ld(v, 'v'), c, c, ldd, ldd, c, kind, 1.0 / (d ** 0.5), float(dropout_p), sptr, *fargs)
    return (dqk, dv) if packed_qk else (dq, dk, dv)


def layernorm_bwd(x, gamma, beta, grad_y, eps=1e-5, res=None, relu=False, into=None, defer=False, outs=None):
    """gd4d_layernorm_bwd.  Returns (dx like x, dgamma, dbeta); into=(g_buf, b_buf): dgamma / dbeta are ADDED to these.
    defer=True: only dx and the partial column sums are computed - returns (dx, workspace, (M, C)) for
    layernorm_bwd_reduce_group.  outs=(dx, dgamma, dbeta): the tensors to write (not with into / defer; default new ones)."""
    lib = _lib.load()
    c = x.shape[-1]
    m = x.numel() // c
    if outs is not None and (into is not None or defer):
        raise ValueError('layernorm_bwd: outs goes with neither into nor defer')
    o_dx, o_dg, o_db = outs if outs is not None else (None, None, None)
    dx = _out(o_dx, x.shape, x.device, 'layernorm_bwd: dx')
    if defer:
        dg, db = None, None
    elif into is None:
        dg = _out(o_dg, gamma.shape, gamma.device, 'layernorm_bwd: dgamma')
        db = _out(o_db, gamma.shape, gamma.device, 'layernorm_bwd: dbeta')
    else:
        dg, db = into
    nbytes = lib.gd4d_layernorm_bwd_workspace_bytes(m, c)
    ws = torch.empty(nbytes, device=x.device, dtype=U8)
    _call('gd4d_layernorm_bwd', _dev(x, 'x', F32), _opt(res, 'res'), _dev(gamma, 'gamma', F32), _opt(beta, 'beta'),
          _dev(grad_y, 'grad_y', F32), _dev(dx, 'dx'), _opt(dg, 'dgamma'), _opt(db, 'dbeta'), _dev(ws, 'workspace'),
          ctypes.c_size_t(nbytes), m, c, float(eps), (1 if relu else 0) | (0 if into is None else 2) | (4 if defer else 0))
    return (dx, ws, (m, c)) if defer else (dx, dg, db)


def layernorm_bwd_reduce_group(problems, accumulate=True):
    """gd4d_layernorm_bwd_reduce_group: problems = list (<= 32) of (workspace, (M, C), dgamma, dbeta) from layernorm_bwd(defer=True)."""
    n = len(problems)
    wss, mcs, dgs, dbs = zip(*problems) if n else [()] * 4
    dims = [int(v) for mc in mcs for v in mc]
    _call('gd4d_layernorm_bwd_reduce_group', _ptrs(wss, 'workspace', None), _ptrs(dgs, 'dgamma'), _ptrs(dbs, 'dbeta'),
          (ctypes.c_int32 * (2 * n))(*dims), n, 1 if accumulate else 0)


def inverse_sigmoid_fwd(x):
    """gd4d_inverse_sigmoid_fwd: the reference's inverse_sigmoid (eps = 1e-5) as one launch; no autograd."""
    y = torch.empty_like(x)
    _call('gd4d_inverse_sigmoid_fwd', _dev(x, 'x', F32), _dev(y, 'y'), x.numel())
    return y


def inverse_sigmoid_bwd(x, grad_y, add=None):
    """gd4d_inverse_sigmoid_bwd: grad_y * d inverse_sigmoid(x) / dx (+ add)."""
    gx = torch.empty_like(x)
    _call('gd4d_inverse_sigmoid_bwd', _dev(x, 'x', F32), _dev(grad_y, 'grad_y', F32), _opt(add, 'add'), _dev(gx, 'grad_x'), x.numel())
    return gx


def refine_reference_fwd(tmp, ref):
    """gd4d_refine_reference_fwd: tmp (..., >=5) regression deltas, ref (..., 3) in [0,1] -> new ref."""
    out = torch.empty_like(ref)
    _call('gd4d_refine_reference_fwd', _dev(tmp, 'tmp', F32), _dev(ref, 'ref', F32), _dev(out, 'out'), ref.numel() // 3, tmp.shape[-1])
    return out


def frustum_pe_input_fwd(img2lidar, feat_hw, pad_hw, depth_num, depth_start, pc_range, out=None, row_start=0):
    """gd4d_frustum_pe_input_fwd.  img2lidar (R, 4, 4) fp32 -> (x, outside (R, H, W) bool).  Without `out`: x is a new
    NCHW (R, 3*D, H, W) tensor; with `out` (R, S, 3*D) the level is written channels-last at pixels
    [row_start, row_start + H*W) of every row."""
    r = img2lidar.shape[0]
    h, w = feat_hw
    row_pixels = 0
    if out is None:
        out = torch.empty(r, 3 * depth_num, h, w, device=img2lidar.device, dtype=F32)
    else:
        row_pixels = out.shape[1]
        if out.shape != (r, row_pixels, 3 * depth_num):
            raise ValueError('out must be (R, S, 3*D)')
    outside = torch.empty(r, h, w, device=img2lidar.device, dtype=U8)
    rng = _range6(pc_range)
    _call('gd4d_frustum_pe_input_fwd', _dev(img2lidar, 'img2lidar', F32), _dev(out, 'out', F32), _dev(outside, 'outside'), r, h, w,
          int(depth_num), float(pad_hw[0]), float(pad_hw[1]), float(depth_start), rng, int(row_pixels), int(row_start))
    return out, outside.bool()


def se_fuse_chlast_fwd(feat, gate, pe, sine, row_start, out=None, out_channels_last=False):
    """gd4d_se_fuse_chlast_fwd: feat (R, C, H, W) NCHW, gate / pe (R, S, C) channels-last, sine NCHW like feat or
    channels-last like gate -> (R, C, H, W).  out_channels_last: the result's MEMORY is (R, H, W, C) - returned as its
    (R, C, H, W) view, the same values; what PyramidView.is_channels_last_level recognises and the gathers read in place."""
    r, c, h, w = feat.shape
    if out is None:
        out = torch.empty((r, h, w, c) if out_channels_last else (r, c, h, w), device=feat.device, dtype=F32)
    _call('gd4d_se_fuse_chlast_fwd', _dev(feat, 'feat', F32), _dev(gate, 'gate', F32), _dev(pe, 'pe', F32), _dev(sine, 'sine', F32),
          _dev(out, 'out'), r, c, h * w, gate.shape[1], int(row_start), int(sine.dim() == 3), 1 if out_channels_last else 0)
    return out.permute(0, 3, 1, 2) if out_channels_last else out


def sine_pe3d_fwd(n_embed, y_embed, x_embed, dim_t, out=None, row_start=0):
    """gd4d_sine_pe3d_fwd.  embeds (R, H, W) fp32, dim_t (F) -> (R, 3*F, H, W); with `out` (R, S, 3*F) the level is
    written channels-last at pixels [row_start, row_start + H*W) of every row."""
    r, h, w = n_embed.shape
    f = dim_t.numel()
    row_pixels = 0
    if out is None:
        out = torch.empty(r, 3 * f, h, w, device=n_embed.device, dtype=F32)
    else:
        row_pixels = out.shape[1]
    _call('gd4d_sine_pe3d_fwd', _dev(n_embed, 'n_embed', F32), _dev(y_embed, 'y_embed', F32), _dev(x_embed, 'x_embed', F32),
          _dev(dim_t, 'dim_t', F32), _dev(out, 'out', F32), r, h * w, f, int(row_pixels), int(row_start))
    return out


def se_fuse_chlast_bwd(grad_out, gate, pe, grad_sine, row_start):
    """gd4d_se_fuse_chlast_bwd for one level: grad_out (R, C, H, W); gate / pe (R, S, C) are REPLACED by their gradients on
    the level's rows, grad_sine (R, S, C) receives grad_out channels-last."""
    r, c, h, w = grad_out.shape
    _call('gd4d_se_fuse_chlast_bwd', _dev(grad_out, 'grad_out', F32), _dev(gate, 'gate', F32), _dev(pe, 'pe', F32), _dev(gate, 'gate'),
          _dev(pe, 'pe'), _dev(grad_sine, 'grad_sine', F32), r, c, h * w, gate.shape[1], int(row_start))


def se_fuse_fwd(feat, gate, pe, sine, out=None):
    """gd4d_se_fuse_fwd: feat + (pe * sigmoid(gate) + sine), all the same shape."""
    out = torch.empty_like(feat) if out is None else out
    _call('gd4d_se_fuse_fwd', _dev(feat, 'feat', F32), _dev(gate, 'gate', F32), _dev(pe, 'pe', F32), _dev(sine, 'sine', F32),
          _dev(out, 'out'), ctypes.c_size_t(feat.numel()))
    return out


def split_bf16_fwd(w):
    """gd4d_split_bf16_fwd: fp32 tensor -> (hi, lo) bf16 tensors of the same shape with w ~= hi + lo."""
    hi = torch.empty(w.shape, device=w.device, dtype=torch.bfloat16)
    lo = torch.empty(w.shape, device=w.device, dtype=torch.bfloat16)
    _call('gd4d_split_bf16_fwd', _dev(w, 'w', F32), _dev(hi, 'hi'), _dev(lo, 'lo'), ctypes.c_size_t(w.numel()))
    return hi, lo


def gemm_bf16x3_fwd(a, w_hi, w_lo, bias=None, relu=False, out=None, relu_in=False, mask_out=False):
    """gd4d_gemm_bf16x3_fwd: a (M, K) fp32 row-major, w_hi / w_lo (N, K) bf16 -> act(a W^T + b) (M, N) fp32.
    mask_out: `out` holds a ReLU's forward output and is replaced by the result where it was > 0, by 0 elsewhere."""
    m, k = a.shape
    n = w_hi.shape[0]
    if out is None:
        if mask_out:
            raise ValueError('mask_out=True needs `out` = the activations of the forward')
        out = torch.empty(m, n, device=a.device, dtype=F32)
    _call('gd4d_gemm_bf16x3_fwd', _dev(a, 'a', F32), _dev(w_hi, 'w_hi', torch.bfloat16), _dev(w_lo, 'w_lo', torch.bfloat16),
          _opt(bias, 'bias'), _dev(out, 'out'), m, n, k, k, n, int(bool(relu)) | (16 if relu_in else 0) | (32 if mask_out else 0))
    return out


def mlp2_image(w1, b1, w2):
    """gd4d_mlp2_image: the MFMA-fragment image of a two-layer MLP's W1 (H, K1), b1 (H) or None, W2 (N2, H) for mlp2_bf16x3_fwd."""
    lib = _lib.load()
    h, k1 = w1.shape
    n2 = w2.shape[0]
    nbytes = int(lib.gd4d_mlp2_image_bytes(k1, h, n2))
    if nbytes == 0 or w2.shape[1] != h:
        raise _lib.Gd4dError(f'mlp2: K1 = {k1} (a multiple of 16, <= 256), H = {h} (a multiple of 32), N2 = {n2} (256) are the kernel\'s limits')
    img = torch.empty(nbytes, device=w1.device, dtype=U8)
    _call('gd4d_mlp2_image', _dev(w1.contiguous(), 'w1', F32), None if b1 is None else _dev(b1.contiguous(), 'b1', F32),
          _dev(w2.contiguous(), 'w2', F32), k1, h, n2, _dev(img, 'image', U8))
    img.shape_khn = (k1, h, n2)
    return img


def mlp2_supported(k1, h, n2):
    return int(_lib.load().gd4d_mlp2_image_bytes(int(k1), int(h), int(n2))) > 0


def mlp2_bf16x3_fwd(x, image, b2=None, out=None):
    """gd4d_mlp2_bf16x3_fwd: x (M, K1) fp32 -> relu(x W1^T + b1) W2^T + b2 (M, N2), the hidden activation never stored."""
    k1, h, n2 = image.shape_khn
    m = x.shape[0]
    if x.shape[1] != k1:
        raise ValueError(f'mlp2_bf16x3_fwd: x has {x.shape[1]} columns, the image was made for {k1}')
    if out is None:
        out = torch.empty(m, n2, device=x.device, dtype=F32)
    _call('gd4d_mlp2_bf16x3_fwd', _dev(x, 'x', F32), _dev(image, 'image', U8), _opt(b2, 'b2'), _dev(out, 'out', F32), m, k1, h, n2, k1, n2)
    return out


def mlp2_pe_se_fwd(img2lidar, feats, pad_hw, depth_num, depth_start, pc_range, pe_image, pe_b2, se_image, se_b2, sine, outs=None,
                   pe_out=None):
    """gd4d_mlp2_pe_se_fwd: position_encoder(frustum) and the SE gate + fuse in one kernel - mlp2_frustum_fwd + mlp2_se_fuse_fwd without
    the (R, S, 256) embedding between them.  feats: L levels (R, 256, H_l, W_l) NCHW of the cameras of img2lidar (R, 4, 4); sine
    (R, S, 256); outs: L (R, H_l, W_l, 256) tensors to write (made when None); pe_out (R, S, 256): store the embedding as well.
    Returns the levels as (R, 256, H_l, W_l) views of channels-last memory."""
    k1, pe_h, n2 = pe_image.shape_khn
    sk, se_h, sn = se_image.shape_khn
    nl = len(feats)
    r = img2lidar.shape[0]
    if k1 != 3 * depth_num or n2 != 256 or sk != 256 or sn != 256 or any(f.shape[0] != r or f.shape[1] != 256 or f.dim() != 4 for f in feats):
        raise ValueError('mlp2_pe_se_fwd: a 3 D -> H -> 256 image, a 256 -> H -> 256 image and (R, 256, H, W) levels expected')
    s_tot = sum(f.shape[2] * f.shape[3] for f in feats)
    if sine.numel() != r * s_tot * 256 or (pe_out is not None and pe_out.numel() != r * s_tot * 256):
        raise ValueError(f'mlp2_pe_se_fwd: sine / pe_out must hold ({r}, {s_tot}, 256)')
    if outs is None:
        outs = [torch.empty(r, f.shape[2], f.shape[3], 256, device=f.device, dtype=F32) for f in feats]
    elif any(tuple(o.shape) != (r, f.shape[2], f.shape[3], 256) for o, f in zip(outs, feats)):
        raise ValueError('mlp2_pe_se_fwd: outs must be (R, H_l, W_l, 256) per level')
    fp = _ptrs(feats, 'feats')
    op = _ptrs(outs, 'outs')
    lv = _levels(feats)
    rng = _range6(pc_range)
    _call('gd4d_mlp2_pe_se_fwd', _dev(img2lidar, 'img2lidar', F32), fp, lv, nl, r, float(pad_hw[0]), float(pad_hw[1]), int(depth_num),
          float(depth_start), rng, _dev(pe_image, 'pe_image', U8), _opt(pe_b2, 'pe_b2'), pe_h, _dev(se_image, 'se_image', U8),
          _opt(se_b2, 'se_b2'), se_h, _dev(sine, 'sine', F32), op, _opt(pe_out, 'pe_out'))
    return [o.permute(0, 3, 1, 2) for o in outs]


def mlp2_se_fuse_fwd(feats, image, b2, pe, sine, outs=None):
    """gd4d_mlp2_se_fuse_fwd: feats = L levels (R, 256, H_l, W_l) NCHW, image = mlp2_image(conv_reduce.weight, conv_reduce.bias,
    conv_expand.weight), b2 = conv_expand.bias, pe / sine (R, S, 256) channels-last rows of all levels side by side ->
    L tensors feat + (pe * sigmoid(gate) + sine) as (R, 256, H_l, W_l) VIEWS of (R, H_l, W_l, 256) memory (channels-last levels;
    outs: the L (R, H_l, W_l, 256) tensors to write)."""
    k1, h, n2 = image.shape_khn
    nl = len(feats)
    r = feats[0].shape[0]
    if k1 != 256 or n2 != 256 or any(f.shape[0] != r or f.shape[1] != 256 or f.dim() != 4 for f in feats):
        raise ValueError('mlp2_se_fuse_fwd: (R, 256, H, W) levels and a 256 -> H -> 256 image expected')
    s_tot = sum(f.shape[2] * f.shape[3] for f in feats)
    if tuple(pe.shape) != (r, s_tot, 256) or tuple(sine.shape) != (r, s_tot, 256):
        raise ValueError(f'mlp2_se_fuse_fwd: pe / sine must be ({r}, {s_tot}, 256)')
    if outs is None:
        outs = [torch.empty(r, f.shape[2], f.shape[3], 256, device=f.device, dtype=F32) for f in feats]
    elif any(tuple(o.shape) != (r, f.shape[2], f.shape[3], 256) for o, f in zip(outs, feats)):
        raise ValueError('mlp2_se_fuse_fwd: outs must be (R, H_l, W_l, 256) per level')
    fp = _ptrs(feats, 'feats')
    op = _ptrs(outs, 'outs')
    lv = _levels(feats)
    _call('gd4d_mlp2_se_fuse_fwd', fp, lv, nl, r, _dev(image, 'image', U8), _opt(b2, 'b2'), _dev(pe, 'pe', F32), _dev(sine, 'sine', F32),
          op, 256, h)
    return [o.permute(0, 3, 1, 2) for o in outs]


def mlp2_frustum_image(w1, b1, w2):
    """The image gd4d_mlp2_frustum_fwd takes: mlp2_image of W1 (H, 192) with its columns in the order the kernel's lanes generate the
    frustum inputs in - column 16 st + 8 kg + e of the image's W1 = column 96 kg + 8 st + e of the module's."""
    if w1.shape[1] != 192:
        raise _lib.Gd4dError('mlp2_frustum_image: position_encoder[0] must take 3 x 64 depth bins')
    col = torch.arange(192, device=w1.device)
    st, kg, e = col // 16, (col % 16) // 8, col % 8
    return mlp2_image(w1[:, 96 * kg + 8 * st + e].contiguous(), b1, w2)


def mlp2_frustum_fwd(img2lidar, level_hw, pad_hw, depth_num, depth_start, pc_range, image, b2=None, out=None):
    """gd4d_mlp2_frustum_fwd: img2lidar (R, 4, 4) -> position_encoder(frustum coordinates) (R, S, 256), S = the pixels of `level_hw`'s
    levels side by side; image: mlp2_frustum_image.  No (R, S, 192) frustum tensor is written or read."""
    k1, h, n2 = image.shape_khn
    r = img2lidar.shape[0]
    nl = len(level_hw)
    s_tot = sum(int(a) * int(b) for a, b in level_hw)
    if k1 != 3 * depth_num or n2 != 256:
        raise ValueError(f'mlp2_frustum_fwd: the image is {k1} -> {h} -> {n2}, the frustum has {3 * depth_num} channels')
    if out is None:
        out = torch.empty(r, s_tot, n2, device=img2lidar.device, dtype=F32)
    elif out.numel() != r * s_tot * n2:
        raise ValueError('mlp2_frustum_fwd: out must hold (R, S, 256)')
    lv = _levels(level_hw)
    rng = _range6(pc_range)
    _call('gd4d_mlp2_frustum_fwd', _dev(img2lidar, 'img2lidar', F32), lv, nl, r, float(pad_hw[0]), float(pad_hw[1]), int(depth_num),
          float(depth_start), rng, _dev(image, 'image', U8), _opt(b2, 'b2'), _dev(out, 'out', F32), h, n2)
    return out.view(r, s_tot, n2)


def petr_keys_plan(bs, n, h, w, want_rows=True):
    """gd4d_petr_keys_plan (host only, no GPU): (workgroups, rows per workgroup, key_rows) of petr_keys_fwd's launch - key_rows[m], a
    list, is the key row that input row m = (b n + cam) h w + pix is written to (None with want_rows=False)."""
    lib = _lib.load()
    grid, per = ctypes.c_int32(0), ctypes.c_int32(0)
    rows = (ctypes.c_int64 * (bs * n * h * w))() if want_rows else None
    _lib.check(lib.gd4d_petr_keys_plan(int(bs), int(n), int(h), int(w), ctypes.addressof(grid), ctypes.addressof(per),
                                       None if rows is None else ctypes.addressof(rows)), 'gd4d_petr_keys_plan')
    return grid.value, per.value, None if rows is None else list(rows)


def petr_keys_fwd(x, img2lidar, pad_hw, depth_num, depth_start, position_range, pe_image, pe_b2, sine, se_image=None, se_b2=None,
                  memory=None, key_pos=None):
    """gd4d_petr_keys_fwd: x (bs, n, 256, H, W) = input_proj's output, img2lidar (bs n, 4, 4), pe_image = mlp2_frustum_image of
    position_encoder, sine (bs n, H W, 256) = the adapt_pos3d branch in channels-last rows, se_image = mlp2_image of fpe.conv_reduce /
    conv_expand or None (no gate) -> (memory, key_pos), both (n H W, bs, 256): PETRTransformer.forward_keys' keys and key_pos."""
    if x.dim() != 5 or x.shape[2] != 256:
        raise ValueError(f'petr_keys_fwd: x must be (bs, n, 256, H, W), got {tuple(x.shape)}')
    bs, n, c, h, w = x.shape
    k1, pe_h, n2 = pe_image.shape_khn
    if k1 != 3 * depth_num or n2 != 256:
        raise ValueError(f'petr_keys_fwd: the position image is {k1} -> {pe_h} -> {n2}, the frustum has {3 * depth_num} channels')
    se_h = 0
    if se_image is not None:
        sk, se_h, sn = se_image.shape_khn
        if sk != 256 or sn != 256:
            raise ValueError('petr_keys_fwd: the gate image must be 256 -> H -> 256')
    if img2lidar.numel() != bs * n * 16 or sine.numel() != bs * n * h * w * 256:
        raise ValueError(f'petr_keys_fwd: img2lidar must hold ({bs * n}, 4, 4) and sine ({bs * n}, {h * w}, 256)')
    if se_b2 is not None and se_image is None:
        raise ValueError('petr_keys_fwd: se_b2 is the gate\'s second bias: it comes with se_image')
    for bias, what in ((pe_b2, 'pe_b2'), (se_b2, 'se_b2')):               # (the kernel reads 256 floats of each)
        if bias is not None and bias.numel() != 256:
            raise ValueError(f'petr_keys_fwd: {what} must hold 256 values, got {tuple(bias.shape)}')
    memory = _out(memory, (n * h * w, bs, 256), x.device, 'memory')
    key_pos = _out(key_pos, (n * h * w, bs, 256), x.device, 'key_pos')
    _call('gd4d_petr_keys_fwd', _dev(x, 'x', F32), _dev(img2lidar, 'img2lidar', F32), bs, n, c, h, w, float(pad_hw[0]), float(pad_hw[1]),
          int(depth_num), float(depth_start), _range6(position_range), _dev(pe_image, 'pe_image', U8), _opt(pe_b2, 'pe_b2'), pe_h,
          _opt(se_image, 'se_image', U8), _opt(se_b2, 'se_b2'), se_h, _dev(sine, 'sine', F32), _dev(memory, 'memory', F32),
          _dev(key_pos, 'key_pos', F32))
    return memory, key_pos


def petr_keys_train_fwd(x, img2lidar, pad_hw, depth_num, depth_start, position_range, pe_image, pe_b2, sine, se_image=None, se_b2=None,
                        memory=None, key_pos=None, pe=None, logits=None):
    """gd4d_petr_keys_train_fwd: petr_keys_fwd (the same arguments, memory / key_pos bit for bit) that also stores what the backward
    reads.  Returns (memory, key_pos, pe, logits): with a gate pe (bs n H W, 256) = position_encoder(frustum) before the gate and logits
    (bs n H W, 256) = the gate's logits, camera-major rows; without a gate both are None (dpe = dkey_pos)."""
    if x.dim() != 5 or x.shape[2] != 256:
        raise ValueError(f'petr_keys_train_fwd: x must be (bs, n, 256, H, W), got {tuple(x.shape)}')
    bs, n, c, h, w = x.shape
    k1, pe_h, n2 = pe_image.shape_khn
    if k1 != 3 * depth_num or n2 != 256:
        raise ValueError(f'petr_keys_train_fwd: the position image is {k1} -> {pe_h} -> {n2}, the frustum has {3 * depth_num} channels')
    se_h = 0
    if se_image is not None:
        sk, se_h, sn = se_image.shape_khn
        if sk != 256 or sn != 256:
            raise ValueError('petr_keys_train_fwd: the gate image must be 256 -> H -> 256')
    if img2lidar.numel() != bs * n * 16 or sine.numel() != bs * n * h * w * 256:
        raise ValueError(f'petr_keys_train_fwd: img2lidar must hold ({bs * n}, 4, 4) and sine ({bs * n}, {h * w}, 256)')
    if se_b2 is not None and se_image is None:
        raise ValueError('petr_keys_train_fwd: se_b2 is the gate\'s second bias: it comes with se_image')
    for bias, what in ((pe_b2, 'pe_b2'), (se_b2, 'se_b2')):
        if bias is not None and bias.numel() != 256:
            raise ValueError(f'petr_keys_train_fwd: {what} must hold 256 values, got {tuple(bias.shape)}')
    m = bs * n * h * w
    memory = _out(memory, (n * h * w, bs, 256), x.device, 'memory')
    key_pos = _out(key_pos, (n * h * w, bs, 256), x.device, 'key_pos')
    if se_image is not None:
        pe = _out(pe, (m, 256), x.device, 'pe')
        logits = _out(logits, (m, 256), x.device, 'logits')
    elif pe is not None or logits is not None:
        raise ValueError('petr_keys_train_fwd: pe / logits are stored with a gate only')
    _call('gd4d_petr_keys_train_fwd', _dev(x, 'x', F32), _dev(img2lidar, 'img2lidar', F32), bs, n, c, h, w, float(pad_hw[0]),
          float(pad_hw[1]), int(depth_num), float(depth_start), _range6(position_range), _dev(pe_image, 'pe_image', U8),
          _opt(pe_b2, 'pe_b2'), pe_h, _opt(se_image, 'se_image', U8), _opt(se_b2, 'se_b2'), se_h, _dev(sine, 'sine', F32),
          _dev(memory, 'memory', F32), _dev(key_pos, 'key_pos', F32), _opt(pe, 'pe'), _opt(logits, 'logits'))
    return memory, key_pos, pe, logits


def petr_keys_bwd_rows(dkey_pos, dmemory, shape, pe=None, logits=None, outs=None):
    """gd4d_petr_keys_bwd_rows: dkey_pos, dmemory (n H W, bs, 256; dmemory None: zeros), shape = (bs, n, H, W), pe / logits = what
    petr_keys_train_fwd stored (a gate) or None -> (dpe, dlogit, dsine (bs n H W, 256) camera-major rows, dx0 (bs n, 256, H, W) =
    dmemory transposed).  Without a gate dlogit is None and dpe IS dsine; with bs = 1 key rows are camera-major rows and dsine IS
    dkey_pos (no copy).  outs = (dpe, dlogit, dsine, dx0): the tensors to write (None entries: new ones)."""
    bs, n, h, w = (int(v) for v in shape)
    m = bs * n * h * w
    if tuple(dkey_pos.shape) != (n * h * w, bs, 256) or (dmemory is not None and tuple(dmemory.shape) != (n * h * w, bs, 256)):
        raise ValueError(f'petr_keys_bwd_rows: dkey_pos / dmemory must be ({n * h * w}, {bs}, 256)')
    gate = logits is not None
    if gate != (pe is not None) or (gate and (tuple(pe.shape) != (m, 256) or tuple(logits.shape) != (m, 256))):
        raise ValueError(f'petr_keys_bwd_rows: pe and logits come together, ({m}, 256) each')
    o_dpe, o_dlogit, o_dsine, o_dx0 = outs if outs is not None else (None,) * 4
    dev = dkey_pos.device
    dsine = None if bs == 1 else _out(o_dsine, (m, 256), dev, 'petr_keys_bwd_rows: dsine')
    dpe = _out(o_dpe, (m, 256), dev, 'petr_keys_bwd_rows: dpe') if gate else None
    dlogit = _out(o_dlogit, (m, 256), dev, 'petr_keys_bwd_rows: dlogit') if gate else None
    dx0 = _out(o_dx0, (bs * n, 256, h, w), dev, 'petr_keys_bwd_rows: dx0')
    _call('gd4d_petr_keys_bwd_rows', _dev(dkey_pos, 'dkey_pos', F32), _opt(dmemory, 'dmemory'), _opt(pe, 'pe'), _opt(logits, 'logits'),
          bs, n, h, w, _opt(dpe, 'dpe'), _opt(dlogit, 'dlogit'), _opt(dsine, 'dsine'), _dev(dx0, 'dx0', F32))
    if dsine is None:
        dsine = dkey_pos.view(m, 256)
    return (dpe if gate else dsine), dlogit, dsine, dx0


def mlp2_wgrad_plan(m, partitions, h=1024):
    """gd4d_mlp2_wgrad_plan (host only, no GPU): ((hidden chunks, partitions) = the grid, [(first tile, one past the last)] per
    partition) of mlp2_wgrad over m rows: contiguous ranges of the 128-row tiles that cover every tile once; a range may be empty."""
    lib = _lib.load()
    grid = (ctypes.c_int32 * 2)()
    ranges = (ctypes.c_int32 * (2 * max(int(partitions), 1)))()
    _lib.check(lib.gd4d_mlp2_wgrad_plan(int(m), int(h), int(partitions), ctypes.addressof(grid), ctypes.addressof(ranges)),
               'gd4d_mlp2_wgrad_plan')
    return (grid[0], grid[1]), [(ranges[2 * q], ranges[2 * q + 1]) for q in range(int(partitions))]


def mlp2_wgrad(dy, w1, b1, w2, x=None, frustum=None, partitions=None, outs=None, workspace=None, want_db2=True):
    """gd4d_mlp2_wgrad: for y = relu(X W1^T + b1) W2^T + b2 and dy (M, 256) -> (dW2 (256, H), db2 (256) or None, dW1 (H, K1), db1 (H)),
    no rows x H and no rows x K1 tensor written.  X: `x` (M, 384) fp32 rows, or `frustum` = (img2lidar (R, 4, 4), (H, W), pad_hw,
    depth_num, depth_start, position_range): the 192 frustum inputs of R cameras generated in registers (M = R H W).  The rows are
    split over `partitions` partial sums added in order (default: about two workgroups per compute unit over the H / 32 hidden
    chunks, at most one partition per 128-row tile).  outs = (dW2, db2, dW1, db1) / workspace: the tensors to write and the partial
    sums' scratch floats (defaults: new ones)."""
    lib = _lib.load()
    if (x is None) == (frustum is None):
        raise ValueError('mlp2_wgrad: X is either `x` (rows in memory) or `frustum` (generated)')
    m = int(dy.shape[0])
    hid, k1 = (int(v) for v in w1.shape)
    n2 = int(w2.shape[0])
    if dy.dim() != 2 or dy.shape[1] != n2 or tuple(w2.shape) != (n2, hid) or b1.numel() != hid:
        raise ValueError(f'mlp2_wgrad: dy {tuple(dy.shape)}, W1 {tuple(w1.shape)}, b1 {tuple(b1.shape)}, W2 {tuple(w2.shape)} do not form an MLP')
    if x is not None and tuple(x.shape) != (m, k1):
        raise ValueError(f'mlp2_wgrad: x must be ({m}, {k1}), got {tuple(x.shape)}')
    i2l, r, fh, fw, pad_h, pad_w, depth_num, depth_start, rng = None, 0, 0, 0, 0.0, 0.0, 0, 0.0, None
    if frustum is not None:
        i2l, (fh, fw), (pad_h, pad_w), depth_num, depth_start, prange = frustum
        r = i2l.numel() // 16
        if r * fh * fw != m or k1 != 3 * depth_num:
            raise ValueError(f'mlp2_wgrad: {r} cameras of {fh} x {fw} pixels and {3 * depth_num} inputs for dy of {m} rows, W1 of {k1} columns')
        rng = _range6(prange)
    if partitions is None:
        tiles = (m + 127) // 128
        chunks = max(hid // 32, 1)
        cus = torch.cuda.get_device_properties(dy.device).multi_processor_count
        partitions = max(1, min(tiles, (2 * cus + chunks - 1) // chunks))
    partitions = int(partitions)
    nbytes = int(lib.gd4d_mlp2_wgrad_workspace_bytes(k1, hid, n2, partitions))
    if nbytes == 0:
        raise _lib.Gd4dError(f'mlp2_wgrad: K1 = {k1} (192 generated, 384 read), H = {hid} (a multiple of 32 up to 4096), N2 = {n2} (256), '
                             f'partitions = {partitions} (1 .. 4096) are the kernel\'s limits')
    o_dw2, o_db2, o_dw1, o_db1 = outs if outs is not None else (None,) * 4
    dev = dy.device
    ws = _out(workspace, (nbytes // 4,), dev, 'mlp2_wgrad: workspace')
    dw2 = _out(o_dw2, (n2, hid), dev, 'mlp2_wgrad: dW2')
    db2 = _out(o_db2, (n2,), dev, 'mlp2_wgrad: db2') if want_db2 else None
    dw1 = _out(o_dw1, (hid, k1), dev, 'mlp2_wgrad: dW1')
    db1 = _out(o_db1, (hid,), dev, 'mlp2_wgrad: db1')
    _call('gd4d_mlp2_wgrad', _opt(x, 'x'), k1, _opt(i2l, 'img2lidar'), r, int(fh), int(fw), float(pad_h), float(pad_w), int(depth_num),
          float(depth_start), rng, _dev(w1, 'w1', F32), _dev(b1, 'b1', F32), _dev(w2, 'w2', F32), _dev(dy, 'dy', F32), m, hid, n2,
          partitions, _dev(ws, 'workspace', F32), nbytes, _dev(dw2, 'dw2', F32), _opt(db2, 'db2'), _dev(dw1, 'dw1', F32),
          _dev(db1, 'db1', F32))
    return dw2, db2, dw1, db1


def gemm_tn_bf16x3(a, b, relu_b=False, want_colsum=True):
    """gd4d_gemm_tn_bf16x3: a (R, M), b (R, N) fp32 row-major -> (a^T b (M, N), column sums of a (M) or None): the weight /
    bias gradients of a Linear over R rows (a = output gradient, b = input; relu_b: ReLU on b as it is read)."""
    lib = _lib.load()
    r, m = a.shape
    n = b.shape[1]
    if b.shape[0] != r:
        raise ValueError(f'gemm_tn_bf16x3: {tuple(a.shape)} against {tuple(b.shape)}')
    dev = a.device
    nbytes = lib.gd4d_gemm_tn_bf16x3_workspace_bytes(r, m, n)
    ws = torch.empty(nbytes, device=dev, dtype=U8)             # (scratch of this call only: see _vp_workspace)
    c = torch.empty(m, n, device=dev, dtype=F32)
    col = torch.empty(m, device=dev, dtype=F32) if want_colsum else None
    _call('gd4d_gemm_tn_bf16x3', _dev(a, 'a', F32), _dev(b, 'b', F32), _dev(c, 'c'), _opt(col, 'colsum'), _dev(ws, 'workspace'), r, m, n, m,
          n, 16 if relu_b else 0)
    return c, col


def knn_farthest_fwd(x, k):
    """gd4d_knn_farthest_fwd: x (B, N, C) fp32 -> (B, N, K) int32 indices of the K farthest rows of the same sample."""
    b, n, c = x.shape
    idx = torch.empty(b, n, k, device=x.device, dtype=I32)
    _call('gd4d_knn_farthest_fwd', _dev(x, 'x', F32), _dev(idx, 'idx'), b, n, c, int(k))
    return idx


def edge_conv_max_fwd(ab, idx, scale, shift):
    """gd4d_edge_conv_max_fwd: ab (B, N, 2C) = [W_a x | W_b x], idx (B, N, K) int32, scale / shift (C) -> (B, N, C)."""
    b, n, c2 = ab.shape
    c = c2 // 2
    out = torch.empty(b, n, c, device=ab.device, dtype=F32)
    base = _dev(ab, 'ab', F32)
    _call('gd4d_edge_conv_max_fwd', base, ctypes.c_void_p(ab.data_ptr() + 4 * c), _dev(idx, 'idx', I32), _dev(scale, 'scale', F32),
          _dev(shift, 'shift', F32), _dev(out, 'out'), b, n, c, idx.shape[-1], c2)
    return out


def box_head_fwd(tmp, ref, pc_range, scale=1.0, out=None):
    """gd4d_box_head_fwd: tmp (..., code) raw regression output, ref (..., 3) in [0,1] -> bbox_preds."""
    out = torch.empty_like(tmp) if out is None else out
    rng = _range6(pc_range)
    _call('gd4d_box_head_fwd', _dev(tmp, 'tmp', F32), _dev(ref, 'ref', F32), rng, float(scale), _dev(out, 'out', F32), ref.numel() // 3,
          tmp.shape[-1])
    return out


def nms_free_decode_fwd(cls_scores, bbox_preds, post_center_range, max_num, score_threshold=None):
    """gd4d_nms_free_decode_fwd.  cls_scores (B, Q, C) logits, bbox_preds (B, Q, code).
    Returns boxes (B, K, 9|7), scores (B, K), labels (B, K) int32, keep (B, K) bool, all sorted by score."""
    b, q, c = cls_scores.shape
    code_size = bbox_preds.shape[-1]
    k = int(max_num)
    if k > q * c:
        raise RuntimeError('selected index k out of range')        # what torch.topk raises in the reference
    dev = cls_scores.device
    boxes = torch.empty(b, k, 9 if code_size > 8 else 7, device=dev, dtype=F32)
    scores = torch.empty(b, k, device=dev, dtype=F32)
    labels = torch.empty(b, k, device=dev, dtype=I32)
    keep = torch.empty(b, k, device=dev, dtype=U8)
    rng = (ctypes.c_float * 6)(*[float(v) for v in post_center_range])
    thr = -1.0 if score_threshold is None else float(score_threshold)
    _call('gd4d_nms_free_decode_fwd', _dev(cls_scores, 'cls_scores', F32), _dev(bbox_preds, 'bbox_preds', F32), rng, thr,
          _dev(boxes, 'boxes'), _dev(scores, 'scores'), _dev(labels, 'labels'), _dev(keep, 'keep'), b, q, c, code_size, k)
    return boxes, scores, labels, keep.bool()


def refine_reference_order_fwd(tmp, ref, pc_range):
    """gd4d_refine_reference_order_fwd: tmp (B, Q, >=5), ref (B, Q, 3) -> (new ref, int32 locality order of it)."""
    b, q = ref.shape[0], ref.shape[1]
    out = torch.empty_like(ref)
    order = torch.empty(b * q, device=ref.device, dtype=I32)
    rng = _range6(pc_range)
    _call('gd4d_refine_reference_order_fwd', _dev(tmp, 'tmp', F32), _dev(ref, 'ref', F32), _dev(out, 'out'), rng, _dev(order, 'order'), b,
          q, tmp.shape[-1])
    return out, order


def cross_attn_bwd(value, level_hw, ref, offsets, attn_logits, cam_logits, lidar2img, pc_range, img_h, img_w,
                   grad_out, query_order=None, raw_cam_weights=False, outs=None, workspace=None):
    """gd4d_cross_attn_bwd.  Returns (grad_value, grad_ref, grad_offsets, grad_attn_logits, grad_cam_logits).
    outs: the five tensors to write - grad_value is ADDED into and must hold zeros; workspace: a uint8 buffer of
    gd4d_cross_attn_bwd_workspace_bytes (0 bytes with B = 1: none)."""
    lib = _lib.load()
    b, q = ref.shape[0], ref.shape[1]
    n = lidar2img.shape[1]
    hh, dh = value.shape[2], value.shape[3]
    p = offsets.shape[3]
    nl = len(level_hw)
    gv = torch.zeros_like(value, dtype=F32) if outs is None else _out(outs[0], value.shape, ref.device, 'outs[0]')
    gr, go, ga, gc = _query_grads(outs, 1, (b, q, 3), (b, q, hh, p, 3), (b, q, hh, nl, p), (b, q, n), ref.device)
    nbytes = lib.gd4d_cross_attn_bwd_workspace_bytes(b, q, hh, nl, p)          # B > 1: partial logit gradients per sample
    ws = _out(workspace, (nbytes,), ref.device, 'workspace', U8) if nbytes else None
    _call('gd4d_cross_attn_bwd', _dev(value, 'value', F32), _levels(level_hw),
          *_camera_args(ref, offsets, attn_logits, cam_logits, lidar2img, pc_range, img_h, img_w), _dev(grad_out, 'grad_out', F32),
          _dev(gv, 'grad_value'), _dev(gr, 'grad_ref'), _dev(go, 'grad_offsets'), _dev(ga, 'grad_attn_logits'), _dev(gc, 'grad_cam_logits'),
          b, n, q, hh, dh, nl, p, _lib.F32, _lib.PIXEL_MAJOR, 1 if raw_cam_weights else 0, _order_ptr(query_order, b * q),
          _opt(ws, 'workspace', None), ctypes.c_size_t(nbytes))
    return gv, gr, go, ga, gc


def match_cost_fwd(cls, box, gt_boxes, gt_labels, gt_start, max_gt, cls_weight=2.0, reg_weight=0.25, alpha=0.25, outs=None):
    """gd4d_match_cost_fwd.  cls (NL, B, Q, C), box (NL, B, Q, code) fp32; gt_boxes (sumG, 7..9) fp32, gt_labels (sumG)
    int32, gt_start (B + 1) int32 - all on the GPU; max_gt = largest per-sample count.  Returns the flat cost buffer
    (NL * Q * sumG): block (l, b) at Q * (l * sumG + gt_start[b]), shape (Q, G_b); every element is written (the blocks tile it).
    The focal term is the reference's fp32 formula -log(1 - p + 1e-12) with p = 1 / (1 + expf(-x)), ill-conditioned by construction
    once 1 - p loses its bits (x above ~6) and constant once p rounds to 1 (x above 24 ln 2).  outs = (cost,) may be the caller's."""
    nl, b, q, c = cls.shape
    sum_gt = gt_boxes.shape[0]
    cost = _out(outs[0] if outs is not None else None, (nl * q * sum_gt,), cls.device, 'outs[0]')
    _call('gd4d_match_cost_fwd', _dev(cls, 'cls', F32), _dev(box, 'box', F32), _dev(gt_boxes, 'gt_boxes', F32),
          _dev(gt_labels, 'gt_labels', I32), _dev(gt_start, 'gt_start', I32), _dev(cost, 'outs[0]', F32), nl, b, q, c, box.shape[-1],
          gt_boxes.shape[-1], sum_gt, int(max_gt), float(cls_weight), float(reg_weight), float(alpha))
    return cost


def head_loss_fwd_bwd(cls, box, assigned, gt_boxes, gt_labels, code_weights, avg_factors, alpha=0.25,
                      loss_cls_weight=2.0, loss_bbox_weight=0.25, outs=None):
    """gd4d_head_loss_fwd_bwd.  Returns (loss (NL, 2), grad_cls like cls, grad_box like box); outs may hold the caller's tensors in
    that order.  A matched row whose stored label is C (or outside [0, C]) is background for the focal term and keeps its box term;
    assigned outside [0, sumG) is background for both.  Box columns >= nk = min(gt_dim > 7 ? 10 : 8, code) get a zero gradient.

    Deviation from torch: the gradients are those of the two terms BEFORE their nan_to_num.  Where a layer's term is not finite (a NaN
    or infinite logit or box entry of that layer) torch's backward through nan_to_num zeroes that term's gradient in the whole layer
    (times the local derivative: NaN at the offending entry); here every other entry keeps its usual finite value, a NaN logit's own
    entry is NaN, a NaN box entry's 0 and a +/-inf box entry's its sign's.  Layers whose terms are finite equal torch's."""
    nl, b, q, c = cls.shape
    outs = tuple(outs) if outs is not None else (None, None, None)
    loss = _out(outs[0], (nl, 2), cls.device, 'outs[0]')
    gcls, gbox = _out(outs[1], cls.shape, cls.device, 'outs[1]'), _out(outs[2], box.shape, cls.device, 'outs[2]')
    _call('gd4d_head_loss_fwd_bwd', _dev(cls, 'cls', F32), _dev(box, 'box', F32), _dev(assigned, 'assigned', I32),
          _dev(gt_boxes, 'gt_boxes', F32), _dev(gt_labels, 'gt_labels', I32), _dev(code_weights, 'code_weights', F32),
          _dev(avg_factors, 'avg_factors', F32), _dev(loss, 'outs[0]', F32), _dev(gcls, 'outs[1]', F32), _dev(gbox, 'outs[2]', F32),
          nl, b, q, c, box.shape[-1], gt_boxes.shape[-1], gt_boxes.shape[0], float(alpha), float(loss_cls_weight), float(loss_bbox_weight))
    return loss, gcls, gbox


def linear_sum_assignment_batch(cost, problems, num_threads=8):
    """gd4d_linear_sum_assignment_batch (host).  cost: contiguous float32 numpy array; problems: list of
    (offset, rows, cols) into it.  Returns a list of int32 arrays (rows,): assigned column per row or -1."""
    import numpy as np
    lib = _lib.load()
    cost = np.ascontiguousarray(cost, dtype=np.float32)
    n = len(problems)
    offs = np.asarray([p[0] for p in problems], dtype=np.int64)
    rows = np.asarray([p[1] for p in problems], dtype=np.int32)
    cols = np.asarray([p[2] for p in problems], dtype=np.int32)
    if n and int((offs + rows.astype(np.int64) * cols).max()) > cost.size:
        raise ValueError('a problem reaches past the end of the cost buffer')
    out_off = np.concatenate([[0], np.cumsum(rows, dtype=np.int64)]).astype(np.int64)
    out = np.empty(int(out_off[-1]), dtype=np.int32)
    as_p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    code = lib.gd4d_linear_sum_assignment_batch(as_p(cost), as_p(offs), as_p(rows), as_p(cols), n, as_p(out),
                                                as_p(out_off), int(num_threads))
    _lib.check(code, 'gd4d_linear_sum_assignment_batch')
    return [out[out_off[i]:out_off[i + 1]] for i in range(n)]


def hungarian_assign_fwd(cost, gt_start, nl, b, q, sum_gt, max_gt, assigned=None, status=None, workspace=None):
    """gd4d_hungarian_assign_fwd: the assignment of every (layer, sample) block of match_cost_fwd's buffer on the device.  Returns
    (assigned (NL, B, Q) int32: index into the packed ground truth or -1, status (NL * B) int32: 0 solved / 1 NaN cost (bad label) /
    2 infeasible).  No host synchronisation."""
    return _assign_fwd('gd4d_hungarian_assign', cost, gt_start, nl, b, q, sum_gt, max_gt, assigned, status, workspace)


def _assign_fwd(stem, cost, gt_start, nl, b, q, sum_gt, max_gt, assigned, status, workspace):
    """hungarian_assign_fwd and lsa_dense_fwd: one contract, two kernels - lib.<stem>_fwd, its scratch sized by lib.<stem>_workspace_bytes."""
    dev = cost.device
    if assigned is None:
        assigned = torch.empty(nl, b, q, device=dev, dtype=I32)
    if status is None:
        status = torch.empty(nl * b, device=dev, dtype=I32)
    nbytes = int(getattr(_lib.load(), stem + '_workspace_bytes')(nl, b, q, max(int(max_gt), 1)))
    if workspace is None or workspace.numel() < nbytes:
        workspace = torch.empty(nbytes, device=dev, dtype=U8)
    _call(stem + '_fwd', _dev(cost, 'cost', F32), _dev(gt_start, 'gt_start', I32), _dev(assigned, 'assigned', I32),
          _dev(status, 'status', I32), _dev(workspace, 'workspace', U8), workspace.numel(), int(nl), int(b), int(q), int(sum_gt),
          int(max_gt))
    return assigned, status


def hungarian_assign_branches_fwd(costs, gt_start, nl, b, qs, ks, sum_gt, max_gt, want_copy=False, status=None, workspace=None):
    """gd4d_hungarian_assign_branches_fwd: H-DETR's one-to-one and one-to-many assignments in one launch.  costs: two match_cost_fwd
    buffers against the same packed, unrepeated ground truth (None for an absent branch, whose q is 0); qs, ks: the two branches' query
    counts and ground-truth multiplicities.  Returns (assigned, copies, status): assigned a list of two (NL, B, Q_t) int32 tensors (index
    into the packed unrepeated ground truth or -1; None for an absent branch), copies the same for the copy numbers (None unless
    want_copy), status (2, NL, B) int32 (0 solved / 1 NaN cost / 2 infeasible).  No host synchronisation."""
    lib = _lib.load()
    dev = gt_start.device
    qs, ks = [int(x) for x in qs], [int(x) for x in ks]
    assigned = [torch.empty(nl, b, q, device=dev, dtype=I32) if q else None for q in qs]
    copies = [torch.empty(nl, b, q, device=dev, dtype=I32) if q and want_copy else None for q in qs]
    if status is None:
        status = torch.zeros(2, nl, b, device=dev, dtype=I32)
    nbytes = int(lib.gd4d_hungarian_assign_branches_workspace_bytes(nl, b, qs[0], qs[1], max(int(max_gt), 1)))
    if workspace is None or workspace.numel() < nbytes:
        workspace = torch.empty(nbytes, device=dev, dtype=U8)
    _call('gd4d_hungarian_assign_branches_fwd', _opt(costs[0], 'cost0'), _opt(costs[1], 'cost1'), _dev(gt_start, 'gt_start', I32),
          _opt(assigned[0], 'assigned0', None), _opt(assigned[1], 'assigned1', None), _opt(copies[0], 'copy0', None),
          _opt(copies[1], 'copy1', None), _dev(status, 'status', I32), _dev(workspace, 'workspace', U8), workspace.numel(), int(nl), int(b),
          qs[0], qs[1], ks[0], ks[1], int(sum_gt), int(max_gt))
    return assigned, copies, status


def distill_match_cost_fwd(s_cls, s_box, t_cls, t_box, cls_weight=1.0, reg_weight=0.25, pseudo_gt=False, outs=None):
    """gd4d_distill_match_cost_fwd.  s_cls (NL, B, Qs, C), s_box (NL, B, Qs, code), t_cls (NL, B, Qt, C), t_box (NL, B, Qt, 10) fp32 on
    the GPU: the teacher head's logits and box codes.  pseudo_gt=True: t_cls the soft labels per sample, t_box (NL, B, Qt, 9) the
    denormalised boxes.  Returns the flat cost buffer (NL * B * Qs * Qt): block (l, b) at Qs * (l * B * Qt + b * Qt), shape (Qs, Qt).
    Without pseudo_gt the soft labels of EVERY sample are sigmoid(t_cls[l, 0]) (the reference's batch-0 indexing); the boxes are each
    sample's own.  outs = (cost,) may be the caller's."""
    nl, b, qs, c = s_cls.shape
    qt = t_cls.shape[2]
    if tuple(s_box.shape[:3]) != (nl, b, qs) or tuple(t_cls.shape) != (nl, b, qt, c) or tuple(t_box.shape) != (nl, b, qt, 9 if pseudo_gt else 10):
        raise ValueError('distill_match_cost_fwd: s_cls / s_box / t_cls / t_box shapes disagree')
    cost = _out(outs[0] if outs is not None else None, (nl * b * qs * qt,), s_cls.device, 'outs[0]')
    _call('gd4d_distill_match_cost_fwd', _dev(s_cls, 's_cls', F32), _dev(s_box, 's_box', F32), _dev(t_cls, 't_cls', F32),
          _dev(t_box, 't_box', F32), _dev(cost, 'outs[0]', F32), nl, b, qs, qt, c, s_box.shape[-1], 1 if pseudo_gt else 0, float(cls_weight),
          float(reg_weight))
    return cost


def lsa_dense_fwd(cost, gt_start, nl, b, q, sum_gt, max_gt, assigned=None, status=None, workspace=None):
    """gd4d_lsa_dense_fwd: hungarian_assign_fwd's contract (same buffers, same outputs and status words) solved by the dense-problem
    kernel.  Returns (assigned (NL, B, Q) int32, status (NL * B) int32).  No host synchronisation."""
    return _assign_fwd('gd4d_lsa_dense', cost, gt_start, nl, b, q, sum_gt, max_gt, assigned, status, workspace)


def distill_loss_fwd_bwd(s_cls, s_box, t_cls, t_box, assigned, code_weights, avg_factors, reweight_score=False,
                         loss_cls_weight=1.0, loss_reg_weight=1.0, outs=None):
    """gd4d_distill_loss_fwd_bwd.  Returns (loss (NL, 2), grad_s_cls like s_cls, grad_s_box like s_box); outs may hold the caller's
    tensors in that order.  Reference quirks kept: a matched row's soft labels are sigmoid(t_cls[l, 0, t]) - batch 0 for every sample;
    an unmatched row (assigned -1 or outside its sample's [b Qt, (b + 1) Qt)) has the label C in every class; with reweight_score the
    divisor sums max_c labels over rows with labels[:, 0] != 10 - the literal 10, so with C != 10 every unmatched row adds C - and is
    not clamped.  Box columns >= 10 get a zero gradient.

    Deviation from torch: the gradients are those of the two terms BEFORE their nan_to_num (see head_loss_fwd_bwd), and when a
    layer's reg divisor is 0 (reweight_score, C == 10, nothing matched) or not finite, grad_s_box[l, :, :, :10] is NaN in EVERY row
    (0 * inf), where torch leaves 0 in the rows the isfinite filter drops.  The loss values and every other layer equal torch's."""
    nl, b, qs, c = s_cls.shape
    qt = t_cls.shape[2]
    if tuple(assigned.shape) != (nl, b, qs) or tuple(t_box.shape) != (nl, b, qt, 10) or tuple(t_cls.shape) != (nl, b, qt, c):
        raise ValueError('distill_loss_fwd_bwd: shapes disagree')
    outs = tuple(outs) if outs is not None else (None, None, None)
    loss = _out(outs[0], (nl, 2), s_cls.device, 'outs[0]')
    gcls, gbox = _out(outs[1], s_cls.shape, s_cls.device, 'outs[1]'), _out(outs[2], s_box.shape, s_cls.device, 'outs[2]')
    _call('gd4d_distill_loss_fwd_bwd', _dev(s_cls, 's_cls', F32), _dev(s_box, 's_box', F32), _dev(t_cls, 't_cls', F32),
          _dev(t_box, 't_box', F32), _dev(assigned, 'assigned', I32), _dev(code_weights, 'code_weights', F32),
          _dev(avg_factors, 'avg_factors', F32), _dev(loss, 'outs[0]', F32), _dev(gcls, 'outs[1]', F32), _dev(gbox, 'outs[2]', F32),
          nl, b, qs, qt, c, s_box.shape[-1], 1 if reweight_score else 0, float(loss_cls_weight), float(loss_reg_weight))
    return loss, gcls, gbox


def lane_mask_loss(logits, targets, loss_weight, outs=None, workspace=None):
    """gd4d_lane_mask_loss: Sigmoid_ce_loss (losses/Sigmoid_ce_loss.py:39-43) of every decoder layer at once, forward and gradient.
    logits (L, R, C), targets (R, C) shared by the layers -> (loss (L,), dlogits (L, R, C)) with dlogits[l] = d loss[l] / d logits[l];
    loss[l] is already through the nan_to_num of petr_head_seg.py:785.

    Deviation from torch: a layer whose loss is not finite before the nan_to_num (a NaN or infinite logit) gets the nan_to_num value and
    an ALL-ZERO gradient; torch's backward leaves a NaN at the offending logit.  The other layers are unaffected bit for bit.
    outs = (loss, dlogits) and workspace (uint8, at least gd4d_lane_mask_loss_workspace_bytes) may be the caller's."""
    if logits.dim() != 3 or tuple(targets.shape) != tuple(logits.shape[1:]) or logits.numel() == 0:
        raise ValueError(f'lane_mask_loss: logits (L, R, C) and targets (R, C) expected, got {tuple(logits.shape)} and {tuple(targets.shape)}')
    nl, r, c = (int(s) for s in logits.shape)
    lp, tp = _dev(logits, 'logits', F32), _dev(targets, 'targets', F32)
    need = int(_lib.load().gd4d_lane_mask_loss_workspace_bytes(nl, r, c))
    if need == 0:
        raise _lib.Gd4dError(f'lane_mask_loss: {nl} layers of {r} x {c} are outside the kernel\'s limits (65535 layers, 2^40 elements)')
    loss, dlogits = outs if outs is not None else (None, None)
    loss = _out(loss, (nl,), logits.device, 'outs[0]')
    dlogits = _out(dlogits, (nl, r, c), logits.device, 'outs[1]')
    if workspace is None:
        workspace = torch.empty(need, device=logits.device, dtype=U8)
    elif workspace.numel() < need:
        raise ValueError(f'lane_mask_loss: workspace of at least {need} bytes expected, got {workspace.numel()}')
    _call('gd4d_lane_mask_loss', lp, tp, float(loss_weight), nl, r, c, _dev(loss, 'outs[0]', F32), _dev(dlogits, 'outs[1]', F32),
          _dev(workspace, 'workspace', U8), workspace.numel())
    return loss, dlogits


def lane_map_fwd(logits, gt_map=None, outs=None):
    """gd4d_lane_map_fwd: the map decode of Petr3D_seg.simple_test_pts (detectors/petr3d_seg.py:228-246) in one launch.  logits
    (B, g g, 768) -> prob (B, 3, 16 g, 16 g) = fp32 1 / (1 + exp(-x)) at '(h w) c h1 w2 -> c (h h1) (w w2)' and binary = prob >= 0.5 as
    fp32 0 / 1; with gt_map (B, 3, 16 g, 16 g) also sums (B, 3, 3) = sum(binary gt), sum(binary), sum(gt) per class and iou (B, 3) =
    (2 inter + 0.01) / (sum(binary) + sum(gt) + 0.01).  Returns (prob, binary) or (prob, binary, sums, iou); outs may hold the
    caller's tensors in that order."""
    g = int(round(logits.shape[1] ** 0.5)) if logits.dim() == 3 else 0
    if logits.dim() != 3 or logits.shape[0] < 1 or g < 1 or g * g != logits.shape[1] or logits.shape[2] != 768:
        raise ValueError(f'lane_map_fwd: logits (B, g g, 768) expected, got {tuple(logits.shape)}')
    b, shape = int(logits.shape[0]), (int(logits.shape[0]), 3, 16 * g, 16 * g)
    if gt_map is not None and tuple(gt_map.shape) != shape:
        raise ValueError(f'lane_map_fwd: gt_map must be {shape}, got {tuple(gt_map.shape)}')
    lp, gp = _dev(logits, 'logits', F32), _opt(gt_map, 'gt_map')
    outs = tuple(outs) if outs is not None else ()
    outs += (None,) * (4 - len(outs))
    prob, binary = _out(outs[0], shape, logits.device, 'outs[0]'), _out(outs[1], shape, logits.device, 'outs[1]')
    sums = iou = None
    if gt_map is not None:
        sums, iou = _out(outs[2], (b, 3, 3), logits.device, 'outs[2]'), _out(outs[3], (b, 3), logits.device, 'outs[3]')
    _call('gd4d_lane_map_fwd', lp, gp, b, g, _dev(prob, 'outs[0]', F32), _dev(binary, 'outs[1]', F32), _opt(sums, 'outs[2]'),
          _opt(iou, 'outs[3]'))
    return (prob, binary) if gt_map is None else (prob, binary, sums, iou)


def _feat_distill_levels(levels, name, like=None):
    """The per-level arguments of the feature-distillation entry points: fp32 (R, 256, H_l, W_l) maps with one R -> (pointer array,
    level_hw array, R)."""
    if not levels or any(t.dim() != 4 for t in levels) or any(t.shape[0] != levels[0].shape[0] or t.shape[1] != levels[0].shape[1] for t in levels):
        raise ValueError(f'{name}: levels (R, C, H_l, W_l) with the same R and C expected')
    if like is not None and [tuple(t.shape) for t in levels] != [tuple(t.shape) for t in like]:
        raise ValueError(f'{name}: the levels\' shapes differ from the other pyramid\'s')
    return _ptrs(levels, name), _levels(levels), int(levels[0].shape[0])


def feat_distill_stats_fwd(teacher, temperature=0.5):
    """gd4d_feat_distill_stats_fwd: teacher levels (R, 256, H_l, W_l) -> the attention maps of MixDistill.get_feat_distill_loss's
    'attention' type (mix_distill.py:131-135), one pass over each level: a_c[l] (R, H_l W_l) = 256 softmax_p(mean_c |t| / T) and
    a_s[l] (R, 256) = H W softmax_c(mean_p |t| / T)."""
    lib = _lib.load()
    tp, lv, r = _feat_distill_levels(teacher, 'teacher')
    nl, c, dev = len(teacher), int(teacher[0].shape[1]), teacher[0].device
    a_c = [torch.empty(r, t.shape[2] * t.shape[3], device=dev, dtype=F32) for t in teacher]
    a_s = [torch.empty(r, c, device=dev, dtype=F32) for t in teacher]
    ws = torch.empty(max(int(lib.gd4d_feat_distill_stats_workspace_bytes(lv, nl, r)), 16), device=dev, dtype=U8)
    cp = _ptrs(a_c, 'a_c')
    sp = _ptrs(a_s, 'a_s')
    _call('gd4d_feat_distill_stats_fwd', tp, lv, nl, r, c, float(temperature), cp, sp, _dev(ws, 'workspace', U8), ws.numel())
    return a_c, a_s


def feat_distill_fwd(student, teacher, weight, bias, loss_weight, a_c=None, a_s=None):
    """gd4d_feat_distill_fwd: student / teacher levels (R, 256, H_l, W_l), weight (L, 256, 256) and bias (L, 256) of the lateral 1x1
    convolutions -> (loss (1), [d loss / d student_l], d loss / d weight (L, 256, 256), d loss / d bias (L, 256)) of
    loss = loss_weight / L * sum_l mean(a_c a_s (conv_l(student_l) - teacher_l)^2); a_c / a_s from feat_distill_stats_fwd, or None for
    the vanilla type (plain mse).  The converted student map is never materialised."""
    lib = _lib.load()
    sp, lv, r = _feat_distill_levels(student, 'student')
    tp, _, _ = _feat_distill_levels(teacher, 'teacher', like=student)
    nl, c, dev = len(student), int(student[0].shape[1]), student[0].device
    if tuple(weight.shape) != (nl, c, c) or tuple(bias.shape) != (nl, c):
        raise ValueError(f'feat_distill_fwd: weight ({nl}, {c}, {c}) and bias ({nl}, {c}) expected')
    if (a_c is None) != (a_s is None):
        raise ValueError('feat_distill_fwd: both attention maps or neither')
    cp = ap = None
    if a_c is not None:
        if len(a_c) != nl or len(a_s) != nl or any(tuple(m.shape) != (r, s.shape[2] * s.shape[3]) for m, s in zip(a_c, student)) or \
                any(tuple(m.shape) != (r, c) for m in a_s):
            raise ValueError('feat_distill_fwd: a_c[l] (R, H_l W_l) and a_s[l] (R, C) expected')
        cp = _ptrs(a_c, 'a_c')
        ap = _ptrs(a_s, 'a_s')
    loss = torch.empty(1, device=dev, dtype=F32)
    gx = [torch.empty_like(s) for s in student]
    gw, gb = torch.empty_like(weight), torch.empty_like(bias)
    gp = _ptrs(gx, 'grad_student')
    ws = torch.empty(max(int(lib.gd4d_feat_distill_workspace_bytes(lv, nl, r)), 16), device=dev, dtype=U8)
    _call('gd4d_feat_distill_fwd', sp, tp, lv, nl, r, c, _dev(weight, 'weight', F32), _dev(bias, 'bias', F32), cp, ap, float(loss_weight),
          _dev(loss, 'loss', F32), gp, _dev(gw, 'grad_weight', F32), _dev(gb, 'grad_bias', F32), _dev(ws, 'workspace', U8), ws.numel())
    return loss, gx, gw, gb


class ChainOp(ctypes.Structure):
    """gd4d_chain_op (include/gd4d.h)."""
    _fields_ = [('kind', ctypes.c_int32), ('src', ctypes.c_int32), ('dst', ctypes.c_int32), ('res', ctypes.c_int32),
                ('K', ctypes.c_int32), ('N', ctypes.c_int32), ('flags', ctypes.c_int32), ('dst_col', ctypes.c_int32),
                ('ld0', ctypes.c_int32), ('ld1', ctypes.c_int32), ('ld2', ctypes.c_int32), ('ldg', ctypes.c_int32),
                ('eps', ctypes.c_float), ('reserved', ctypes.c_int32),
                ('p0', ctypes.c_void_p), ('p1', ctypes.c_void_p), ('p2', ctypes.c_void_p), ('gout', ctypes.c_void_p),
                ('p3', ctypes.c_void_p)]


CHAIN_LOAD, CHAIN_GEMM, CHAIN_LAYERNORM, CHAIN_ADD, CHAIN_REFINE, CHAIN_SMALL_LINEAR, CHAIN_HEADGEMM, CHAIN_SIGNAL, CHAIN_WAIT = 1, 2, 3, 4, 5, 6, 7, 8, 9
CHAIN_LN_BWD, CHAIN_DROPMASK = 10, 11
CHAIN_RELU, CHAIN_INV_SIGMOID, CHAIN_SIGMOID, CHAIN_EXACT, CHAIN_SRC2, CHAIN_SPLIT_OUT, CHAIN_MASK_P2, CHAIN_DROPOUT = 1, 2, 4, 8, 16, 32, 64, 128
CHAIN_SPLIT_KV, CHAIN_SPLIT_KV_KEEP, CHAIN_ADD_GOUT = 256, 512, 1024


def _rows(t, name):
    """(data pointer, row stride in elements) of a fp32 GPU tensor whose last dimension is dense and whose leading
    dimensions collapse to rows of one stride (a contiguous tensor or a last-dim slice of one)."""
    if t is None:
        return None, 0
    if not t.is_cuda or t.dtype != F32:
        raise _lib.Gd4dError(f'{name} must be a float32 GPU tensor')
    if t.dim() == 1:
        return t.data_ptr(), 0
    if t.stride(-1) != 1:
        raise ValueError(f'{name}: the last dimension must be dense')
    ld = t.stride(-2)
    for d in range(t.dim() - 2):
        if t.shape[d] != 1 and t.stride(d) != t.stride(d + 1) * t.shape[d + 1]:
            raise ValueError(f'{name}: rows must have one stride')
    return t.data_ptr(), ld


def chain_load(dst, x, x2=None, dst_col=0, inv_sigmoid=False, out=None):
    """buf[dst][:, dst_col ..] = f(x) (+ x2); out: the rows are also stored there."""
    p0, ld0 = _rows(x, 'x')
    p1, ld1 = _rows(x2, 'x2')
    g, ldg = _rows(out, 'out')
    return ChainOp(kind=CHAIN_LOAD, src=-1, dst=dst, res=-1, N=x.shape[-1], dst_col=dst_col, ld0=ld0, ld1=ld1, ldg=ldg,
                   flags=CHAIN_INV_SIGMOID if inv_sigmoid else 0, p0=p0, p1=p1, gout=g)


_CHAIN_IMAGES = {}
_CHAIN_EPOCH = [0]


def invalidate_chain_images():
    """The one rule for every value kept from parameters (_Stamp): chain_weight_image, value_proj_image, the stacked weights of
    chain_gemm_three_outputs, DepthNet's weight image, FeaturePositionEmbedding's weight splits, sine branch and kept embedding.
    Such a value is served while each source is the same live tensor (through its `_base`) with the same address, shape, dtype
    and version counter, and while this function has not been called since it was built; it is dropped when a source dies.
    Version counters miss writes through `.data` (p.data.copy_(), mmcv's EMA swap, an optimizer step inside a replayed graph):
    call this after such an update - the package's modules do it from train() / eval() and after load_state_dict."""
    for table in (_CHAIN_IMAGES, _VP_IMAGES, _STACKED):
        table.clear()
    _CHAIN_EPOCH[0] += 1


class _Stamp:
    """Whether a value built from the tensors `sources` (None: an absent one, e.g. a missing bias) still holds, by the rule of
    invalidate_chain_images; on_death (a weakref callback) runs when a source dies.  A copy (copy.deepcopy, pickle, torch.save of a module that
    keeps one) is never valid: it must not vouch for the original's tensors."""
    __slots__ = ('_refs', '_marks', '_epoch')

    def __init__(self, sources=(), on_death=None):
        self._refs = [weakref.ref(_base(t), on_death) for t in sources if t is not None]
        self._marks = [_mark(t) for t in sources]
        self._epoch = _CHAIN_EPOCH[0] if sources else -1

    def valid(self, sources):
        # (while the referents live, no other object has their id(): equal ids are the same tensors)
        return self._epoch == _CHAIN_EPOCH[0] and all(r() is not None for r in self._refs) and [_mark(t) for t in sources] == self._marks

    def __reduce__(self):
        return _Stamp, ()


def _base(t):
    return t if t._base is None else t._base


def _mark(t):
    return None if t is None else (id(_base(t)), t.data_ptr(), t.shape, t.dtype, t.device, t._version)


def _kept(table, key, sources, build):
    """table[key]: build()'s value of `sources`, rebuilt when the stamp it was kept with no longer holds; a source's death drops it."""
    hit = table.get(key)
    if hit is not None and hit[0].valid(sources):
        return hit[1]
    value = build()
    table[key] = (_Stamp(sources, lambda _r: table.pop(key, None)), value)
    return value


def kept_in_place(table, key, sources, build, owner, changed='parameter'):
    """_kept at a fixed address, for values a captured hipGraph reads (the weight images and folded constants of FPN, DCNv2, VoVNet):
    table[key] is served while its stamp holds and it lives on the device of the first source that is not None.  Otherwise build()
    runs under torch.no_grad() and, where an earlier value of the same device and shape is kept, is copied INTO that buffer, so a
    captured graph sees the new weights; under hipGraph capture it raises instead, in `owner`'s name.  The entry outlives its
    sources: the address is the point."""
    sources = tuple(sources)
    ent = table.get(key)
    dev = next(t for t in sources if t is not None).device
    if ent is not None and ent[0].valid(sources) and ent[1].device == dev:
        return ent[1]
    if dev.type == 'cuda' and torch.cuda.is_current_stream_capturing():       # (never asked of CPU tensors: there may be no GPU)
        raise RuntimeError(f'{type(owner).__name__} under hipGraph capture: call the module (or refresh_images) once eagerly first - '
                           f'its weight images are not on the device yet, or a {changed} changed since they were made')
    with torch.no_grad():
        value = build()
    if ent is not None and ent[1].device == value.device and ent[1].shape == value.shape:
        ent[1].copy_(value)
        value = ent[1]
    table[key] = (_Stamp(sources), value)
    return value


def chain_weight_image(weight, exact=False):
    """The bf16 hi / lo (exact: hi / mid / lo) MFMA-fragment image of a (N, K) fp32 weight (gd4d_chain_weight_image[_exact]),
    kept while the weight does not change (invalidate_chain_images) - one small launch after a load_state_dict or an optimizer
    step, none in steady-state inference."""
    if not weight.is_cuda or weight.dtype != F32 or weight.dim() != 2 or weight.stride(1) != 1 \
            or weight.stride(0) != weight.shape[1]:
        raise ValueError('chain weights must be dense (N, K) float32 GPU tensors')

    def build():
        lib = _lib.load()
        n, k = weight.shape
        nbytes = (lib.gd4d_chain_weight_image_exact_bytes if exact else lib.gd4d_chain_weight_image_bytes)(n, k)
        if nbytes == 0:
            raise _lib.Gd4dError(f'chain GEMM: K = {k} must be a multiple of 64')
        img = torch.empty(nbytes, device=weight.device, dtype=U8)
        with torch.cuda.device(weight.device):
            _call('gd4d_chain_weight_image_exact' if exact else 'gd4d_chain_weight_image', ctypes.c_void_p(weight.data_ptr()), n, k,
                  ctypes.c_void_p(img.data_ptr()))
        return img
    return _kept(_CHAIN_IMAGES, (weight.data_ptr(), tuple(weight.shape), bool(exact)), (weight,), build)


class ImageJob(ctypes.Structure):
    """gd4d_image_job (include/gd4d.h)."""
    _fields_ = [('seg', ctypes.c_void_p * 3), ('rows', ctypes.c_int32 * 3), ('cols', ctypes.c_int32), ('transposed', ctypes.c_int32),
                ('planes', ctypes.c_int32), ('frag0', ctypes.c_int32), ('reserved', ctypes.c_int32), ('image', ctypes.c_void_p)]


class WeightImage:
    """A chain GEMM operand made by an ImageSet: the image tensor and the (N, K) of the GEMM it serves (K already padded)."""

    def __init__(self, img, n, k, exact):
        self.img, self.n, self.k, self.exact = img, n, k, exact


class ImageSet:
    """The weight images of a TRAINING step's chains (gd4d_chain_weight_image_group): declared once (add / add_concat; the
    parameters' storage must stay where it is), rebuilt by ONE launch per step (refresh) into buffers whose addresses never
    change - a captured hipGraph replays the rebuild with the step, after every optimizer update."""

    def __init__(self, device):
        self.device = device
        self._jobs, self._keep, self._frags = [], [], 0
        self._table = None
        self.sources = []

    def _segments(self, tensors, cols):
        if not 1 <= len(tensors) <= 3:
            raise ValueError('an image stacks one to three row blocks')
        seg, rows = (ctypes.c_void_p * 3)(), (ctypes.c_int32 * 3)()
        for i, t in enumerate(tensors):
            if not t.is_cuda or t.dtype != F32 or not t.is_contiguous() or t.numel() % cols:
                raise ValueError('image sources must be dense float32 GPU tensors of `cols` columns')
            seg[i], rows[i] = t.data_ptr(), t.numel() // cols
            self.sources.append(t)
        return seg, rows, int(sum(rows))

    def add(self, tensors, transposed=False, exact=False):
        """Image of the row blocks `tensors` (each (r_i, cols)) stacked - or of the stack's transpose."""
        cols = tensors[0].shape[-1]
        seg, rows, r = self._segments(tensors, cols)
        n, k = (cols, r) if transposed else (r, cols)
        kp = (k + 63) // 64 * 64
        planes = 3 if exact else 2
        frags = (n + 15) // 16 * (kp // 32)
        img = torch.empty(frags * planes * 1024, device=self.device, dtype=U8)
        self._jobs.append(ImageJob(seg=seg, rows=rows, cols=cols, transposed=int(transposed), planes=planes, frag0=self._frags,
                                   image=img.data_ptr()))
        self._frags += frags
        self._table = None
        return WeightImage(img, n, kp, exact)

    def add_concat(self, vectors):
        """fp32 concatenation of 1-D tensors (a stacked bias), refreshed with the images."""
        seg, rows, r = self._segments(vectors, 1)
        out = torch.empty(r, device=self.device, dtype=F32)
        self._jobs.append(ImageJob(seg=seg, rows=rows, cols=1, transposed=0, planes=0, frag0=self._frags, image=out.data_ptr()))
        self._frags += (r + 63) // 64
        self._table = None
        return out

    def signature(self):
        return tuple(t.data_ptr() for t in self.sources)

    def finalize(self):
        """Upload the job table (a host-to-device copy: call it outside a graph capture; refresh() does it on first use)."""
        if self._table is None:
            arr = (ImageJob * len(self._jobs))(*self._jobs)
            raw = torch.frombuffer(bytearray(bytes(arr)), dtype=U8)
            self._table = raw.to(self.device)

    def refresh(self):
        self.finalize()
        if len(self._jobs) > 1024:
            raise _lib.Gd4dError('ImageSet: more than 1024 jobs (GD4D_IMAGE_JOBS_MAX) - split the set')
        with torch.cuda.device(self.device):
            _call('gd4d_chain_weight_image_group', ctypes.c_void_p(self._table.data_ptr()), len(self._jobs), self._frags)


def _image_of(weight, exact=False):
    """(image pointer, N, K) of a chain GEMM operand: a WeightImage of an ImageSet, or a weight tensor (cached image)."""
    if isinstance(weight, WeightImage):
        if weight.exact != bool(exact):
            raise ValueError('chain GEMM: the image was made for the other arithmetic (exact)')
        return weight.img.data_ptr(), weight.n, weight.k
    return chain_weight_image(weight, exact).data_ptr(), weight.shape[0], weight.shape[1]


def chain_dropout_args(p):
    """(threshold, scale) of a dropout with probability p as the chain operations take them (gd4d_mha_dropout.h)."""
    t = float(p) * 4294967296.0
    thresh = 0 if t <= 0 else (0xFFFFFFFF if t >= 4294967295.0 else int(t + 0.5))
    return thresh, 1.0 / (1.0 - float(p))


def chain_dropout_keep_mask(seed, m, n, p):
    """The (m, n) bool keep mask a chain GEMM with dropout=(seed, p) and N = n draws (restated with torch integer ops, as
    mha_dropout_keep_mask): for tests against torch with the same mask."""
    return mha_dropout_keep_mask(seed, 1, 1, m, n, p).view(m, n)


def chain_dropmask(src, dst, n, seed, p, out=None):
    """buf[dst] = (the keep mask of a forward GEMM with dropout=(seed, p), N = n) * buf[src] / (1 - p); out: also stored."""
    thresh, scale = chain_dropout_args(p)
    g, ldg = _rows(out, 'out')
    c_thresh = thresh - (1 << 32) if thresh >= (1 << 31) else thresh
    return ChainOp(kind=CHAIN_DROPMASK, src=src, dst=dst, res=-1, N=n, eps=scale, reserved=c_thresh, ldg=ldg, gout=g,
                   p0=_dev(seed, 'seed', torch.int64).value)


# Measurement switch (bench.py's `exact_gemms` figure; `with ops.all_exact():`): EVERY GEMM operation of the chains built while it is
# on uses six bf16 products (GD4D_CHAIN_EXACT, ~2^-24) - what fp32-class arithmetic on the query side costs.  HEADGEMM (value_proj
# of the aggregates) and the attention core's two products stay on three.
ALL_EXACT = [switches.flag('GD4D_CHAIN_ALL_EXACT')]          # (an import-time read: switches.py)


class all_exact:
    def __enter__(self):
        self.prev, ALL_EXACT[0] = ALL_EXACT[0], True

    def __exit__(self, *exc):
        ALL_EXACT[0] = self.prev


def chain_gemm(src, weight, bias=None, dst=-1, dst_col=0, relu=False, res=-1, out=None, sigmoid=False, exact=False, add=None,
               add2=None, mask=None, mask_scale=0., dropout=None):
    """act(buf[src] W^T + b) (+ buf[res]) (+ (add + add2)[m, :]) -> buf[dst] and / or out.  weight (N, K) contiguous rows.
    add / add2: global (M, N) tensors added in the epilogue (their sum first, then onto the result - what a LOAD of
    add + add2 into buf[res] would give, without the operation).  exact: fp32-class products (GD4D_CHAIN_EXACT) instead of
    split-bf16 x3 - for outputs that become reference points."""
    exact = exact or ALL_EXACT[0]
    img, n, k = _image_of(weight, exact)
    g, ldg = _rows(out, 'out')
    if mask is not None and (add is not None or add2 is not None):
        raise ValueError('chain_gemm: mask (a backward chain\'s ReLU) and global addends exclude each other')
    p2, ld2 = _rows(add if mask is None else mask, 'add')
    p3, ld3 = _rows(add2, 'add2')
    if p3 is not None and p2 is None:
        raise ValueError('chain_gemm: add2 without add')
    eps, reserved, flags = float(mask_scale) if mask is not None else 0., 0, 0
    if dropout is not None and float(dropout[1]) > 0.:      # (seed: (1,) int64 device tensor, p): nn.Dropout on the output
        if mask is not None or p3 is not None:
            raise ValueError('chain_gemm: dropout excludes mask and add2')
        thresh, eps = chain_dropout_args(dropout[1])
        reserved = thresh - (1 << 32) if thresh >= (1 << 31) else thresh
        p3, flags = _dev(dropout[0], 'seed', torch.int64).value, CHAIN_DROPOUT
    return ChainOp(kind=CHAIN_GEMM, src=src, dst=dst, res=res, K=k, N=n, dst_col=dst_col,
                   flags=(CHAIN_RELU if relu else 0) | (CHAIN_SIGMOID if sigmoid else 0) | (CHAIN_EXACT if exact else 0) |
                   (CHAIN_MASK_P2 if mask is not None else 0) | flags, ldg=ldg, eps=eps, reserved=reserved,
                   ld2=ld2, ld1=ld3, p0=img, p1=None if bias is None else bias.data_ptr(), p2=p2, p3=p3, gout=g)


class KVPlanes:
    """The attention core's K / V operands as split-bf16 planes in its MFMA fragment layout (GD4D_CHAIN_SPLIT_KV ->
    gd4d_mha_core_presplit_fwd; include/gd4d.h has the layouts): k (2, H, tiles, 64, 8), v (2, H, steps, 2, 64, 8) bf16."""

    def __init__(self, m, c, device, heads=8):
        self.m, self.c, self.heads = int(m), int(c), int(heads)
        self.tiles, self.steps = (self.m + 15) // 16, (self.m + 31) // 32
        self.k = torch.empty(2, heads, self.tiles, 64, 8, device=device, dtype=torch.bfloat16)
        self.v = torch.empty(2, heads, self.steps, 2, 64, 8, device=device, dtype=torch.bfloat16)

    def k_rows(self):
        """(2, tiles * 16, C): the planes as plain rows (tests)."""
        h, t = self.heads, self.tiles
        return self.k.view(2, h, t, 4, 16, 8).permute(0, 2, 4, 1, 3, 5).reshape(2, t * 16, h * 32)

    def v_rows(self):
        """(2, steps * 32, C): the planes as plain rows (tests)."""
        h, s = self.heads, self.steps
        # [plane][h][s][half][g][qi][t][r]  ->  key = 32 s + 16 t + 4 g + r, channel = 32 h + 16 half + qi
        return self.v.view(2, h, s, 2, 4, 16, 2, 4).permute(0, 2, 6, 4, 7, 1, 3, 5).reshape(2, s * 32, h * 32)


def chain_gemm_two_sources(src, src2, split, weight, bias, out, kv=None, keep_fp32=False):
    """One GEMM over a stacked weight (N, K) whose output columns [0, split) are computed from buf[src] and [split, N) from
    buf[src2] (split a multiple of 256): nn.MultiheadAttention's packed in-projection with q, k from x + pos and v from x.
    kv (KVPlanes, N = 768): the K and V columns are written as the attention core's split-bf16 operands INSTEAD of fp32 (out
    receives the Q columns only; keep_fp32 - a training step, whose attention backward reads fp32 rows: all columns)."""
    g, ldg = _rows(out, 'out')
    img, n, k = _image_of(weight, ALL_EXACT[0])
    op = ChainOp(kind=CHAIN_GEMM, src=src, dst=-1, res=src2, K=k, N=n, flags=CHAIN_SRC2 | (CHAIN_EXACT if ALL_EXACT[0] else 0), ld0=int(split),
                 ldg=ldg, p0=img, p1=None if bias is None else bias.data_ptr(), gout=g)
    if kv is not None:
        if n != 3 * kv.c or kv.c != 256 or kv.heads != 8:
            raise ValueError('kv planes: the packed in-projection of 256 channels, 8 heads')
        op.flags |= CHAIN_SPLIT_KV | (CHAIN_SPLIT_KV_KEEP if keep_fp32 else 0)
        op.p2, op.ld2 = kv.k.data_ptr(), kv.k[0].numel()
        op.p3, op.ld1 = kv.v.data_ptr(), kv.v[0].numel()
    return op


_STACKED = {}


def _stacked_linears(linears):
    """cat of the Linears' weights / biases (zeros for a missing bias), kept while none of them changes (invalidate_chain_images)."""
    def build():
        with torch.no_grad():
            w = torch.cat([m.weight for m in linears], 0).contiguous()
            b = torch.cat([m.bias if m.bias is not None else m.weight.new_zeros(m.weight.shape[0]) for m in linears], 0).contiguous()
        return w, b
    if len(_STACKED) > 256:                               # modules come and go in long-lived processes
        _STACKED.clear()
    return _kept(_STACKED, tuple(id(m) for m in linears), [t for m in linears for t in (m.weight, m.bias)], build)


def chain_gemm_three_outputs(src, linears, outs, stacked=None, exact=False):
    """Three nn.Linear of ONE input (buf[src]) as one GEMM over their stacked weights; column block i goes to outs[i] (M, N_i),
    dense rows.  The sums of a column do not depend on the operation it is part of: bit-identical to three chain_gemm.
    exact: fp32-class products (GD4D_CHAIN_EXACT) - one of the outputs are sampling offsets in metres, which a camera matrix turns
    into pixels before the visibility mask is decided."""
    if len(linears) != 3 or len(outs) != 3:
        raise ValueError('chain_gemm_three_outputs takes three Linears and three outputs')
    ptrs = [_rows(o, 'out') for o in outs]
    for (ptr, ld), m in zip(ptrs, linears):
        if ld != m.weight.shape[0]:
            raise ValueError('chain_gemm_three_outputs: every output must be dense, as wide as its Linear')
    if stacked is not None:                   # (WeightImage of the stacked weights, stacked bias) of an ImageSet
        img, n, k = _image_of(stacked[0], exact)
        b = stacked[1]
    else:
        w, b = _stacked_linears(linears)
        img, n, k = _image_of(w, exact)
    return ChainOp(kind=CHAIN_GEMM, src=src, dst=-1, res=-1, K=k, N=n, flags=CHAIN_SPLIT_OUT | (CHAIN_EXACT if exact else 0),
                   ldg=ptrs[0][1], ld2=ptrs[1][1], ld1=ptrs[2][1], p0=img, p1=b.data_ptr(),
                   gout=ptrs[0][0], p2=ptrs[1][0], p3=ptrs[2][0])


def chain_headgemm(agg, wsum, weight, bias=None, dst=-1, res=-1, out=None, addend=None):
    """value_proj of the per-head aggregates (cross_attn_agg_fwd's agg (..., Hh, K), wsum (..., Hh), contiguous) as a chain
    operation: v[m, n] = sum_k agg[m][h][k] W[n][k] + bias[n] wsum[m][h] (+ buf[res]) (+ addend[m, n]) -> buf[dst] and / or out.
    addend (M, N): a global tensor that is added - cross_attn_agg_coarse_fwd's pagg; excludes `out`."""
    heads, k = agg.shape[-2], agg.shape[-1]
    img, n, wk = _image_of(weight)
    if wk != k or n % heads or (n // heads) % 32 or wsum.numel() * k != agg.numel():
        raise ValueError('chain_headgemm: weight (N, K), agg (..., Hh, K), wsum (..., Hh) with (N / Hh) % 32 == 0')
    if addend is not None and (out is not None or dst < 0 or addend.shape[-1] != n):
        raise ValueError('chain_headgemm: an addend (M, N) goes with dst >= 0 and no `out`')
    g, ldg = _rows(out if addend is None else addend, 'out')
    return ChainOp(kind=CHAIN_HEADGEMM, src=-1, dst=dst, res=res, K=k, N=n, ld0=heads, ldg=ldg, p0=img,
                   flags=CHAIN_ADD_GOUT if addend is not None else 0,
                   p1=None if bias is None else bias.data_ptr(), p2=_dev(agg, 'agg', F32).value,
                   p3=_dev(wsum, 'wsum', F32).value, gout=g)


def chain_small_linear(src, weight, bias, dst, relu=False, inv_sigmoid=False, out=None):
    """buf[dst] = act(f(buf[src][:, :K]) W^T + b) for K <= 8; f = inverse_sigmoid with inv_sigmoid=True."""
    g, ldg = _rows(out, 'out')
    return ChainOp(kind=CHAIN_SMALL_LINEAR, src=src, dst=dst, res=-1, K=weight.shape[1], N=weight.shape[0], ldg=ldg, gout=g,
                   flags=(CHAIN_RELU if relu else 0) | (CHAIN_INV_SIGMOID if inv_sigmoid else 0), p0=weight.data_ptr(),
                   p1=None if bias is None else bias.data_ptr())


def chain_layernorm_bwd(src, x_buf, norm, dst=-1, relu=False, out=None, part=None):
    """Backward of chain_layernorm: buf[src] = gradient of the output; the forward's input = buf[x_buf], or - x_buf a tensor -
    its rows in global memory (no LOAD operation needed); dx -> buf[dst] (may be src) and / or out; part: (ceil(M / 16), 2, N)
    fp32 partial dgamma / dbeta (layernorm_bwd_reduce_group adds them)."""
    g, ldg = _rows(out, 'out')
    p3, ld3 = (None, 0) if isinstance(x_buf, int) else _rows(x_buf, 'x')
    return ChainOp(kind=CHAIN_LN_BWD, src=src, dst=dst, res=x_buf if isinstance(x_buf, int) else -1, N=norm.weight.shape[0],
                   eps=float(norm.eps), flags=CHAIN_RELU if relu else 0, ldg=ldg, ld1=ld3, p0=norm.weight.data_ptr(),
                   p1=norm.bias.data_ptr(), p2=None if part is None else _dev(part, 'part', F32).value, gout=g, p3=p3)


def chain_layernorm(src, norm, dst=-1, relu=False, out=None, dst2=-1, add=None):
    """LayerNorm of buf[src] -> buf[dst] and / or out; with dst2 and add: also buf[dst2] = result + add[m, :] (the ADD
    operation that would follow, e.g. x + query_pos for the next projection)."""
    g, ldg = _rows(out, 'out')
    p2, ld2 = _rows(add, 'add')
    if (p2 is None) != (dst2 < 0):
        raise ValueError('chain_layernorm: dst2 and add go together')
    return ChainOp(kind=CHAIN_LAYERNORM, src=src, dst=dst, res=dst2, N=norm.weight.shape[0], eps=float(norm.eps),
                   flags=CHAIN_RELU if relu else 0, ldg=ldg, ld2=ld2, p0=norm.weight.data_ptr(), p1=norm.bias.data_ptr(),
                   p2=p2, gout=g)


def chain_add(dst, src, n, res=-1, add=None, out=None):
    """buf[dst] = buf[src] (+ buf[res]) (+ add[m, :]); out: the sum is also stored there."""
    p2, ld2 = _rows(add, 'add')
    g, ldg = _rows(out, 'out')
    return ChainOp(kind=CHAIN_ADD, src=src, dst=dst, res=res, N=n, ld2=ld2, p2=p2, ldg=ldg, gout=g)


def chain_refine(src, ref, out, dst=-1):
    """Reference-point refinement of buf[src] (the reg branch's output) and `ref` into `out`; dst >= 0 also parks the
    refined points in buf[dst][:, 0:3]."""
    return ChainOp(kind=CHAIN_REFINE, src=src, dst=dst, res=-1, p0=ref.data_ptr(), gout=out.data_ptr())


def chain_signal(flags):
    """Two-program launches: publish this program's global outputs of its 16 rows to the other program (flags: int32 tensor
    of >= ceil(M / 16) zeros, one per row block)."""
    return ChainOp(kind=CHAIN_SIGNAL, src=-1, dst=-1, res=-1, gout=_dev(flags, 'flags', I32).value)


_HANDOFF = {}       # device index -> {'word': int32[1] on the device, 'pinned': int32[1] host, 'event': Event or None, 'placement': bool}


def _handoff_state(device):
    device = torch.device(device)
    idx = device.index if device.index is not None else torch.cuda.current_device()
    st = _HANDOFF.get(idx)
    if st is None:
        dev = torch.device('cuda', idx)
        st = _HANDOFF[idx] = {'word': None, 'dev': dev, 'pinned': None, 'event': None, 'placement': None}
    return st


def handoff_error_word(device):
    """The device's sticky error word of the SIGNAL / WAIT hand-offs between chain programs: a WAIT that gives up (~0.2 s
    unanswered) adds 1 to it and POISONS the rows it hands on (NaN), so a time-out is a wrong answer nobody can mistake for a right
    one, and check_handoff() / poll_handoff() turn it into an exception."""
    st = _handoff_state(device)
    if st['word'] is None:
        st['word'] = torch.zeros(1, device=st['dev'], dtype=I32)
    return st['word']


_HANDOFF_FLAGS = {}       # (device index, request slot key, rows, cols) -> int32 (rows, cols), zero between requests


def handoff_flags(device, rows, cols, slot_key):
    """The SIGNAL / WAIT flags of one request: (rows, cols) int32, zero when a request starts - the WAITing program takes every flag
    down again after it has seen it - so ONE persistent buffer per (device, request slot) serves every request and a replayed
    hipGraph holds no fill.  slot_key: functional.slot_key(device) - requests in flight on different streams get their own."""
    device = torch.device(device)
    key = (device.index, slot_key, int(rows), int(cols))
    buf = _HANDOFF_FLAGS.get(key)
    if buf is None:
        if torch.cuda.is_current_stream_capturing():
            return torch.zeros(rows, cols, device=device, dtype=I32)       # (first use inside a capture: this graph's own, filled per replay)
        buf = _HANDOFF_FLAGS[key] = torch.zeros(rows, cols, device=device, dtype=I32)
    return buf


def check_handoff(device=None):
    """Blocking: raises Gd4dError if a hand-off has timed out on `device` (default: every device used so far) since the last check.
    Call it where a host sync exists anyway - after a request's graph replay (or every N replays), at the end of a step."""
    sts = list(_HANDOFF.items()) if device is None else [(None, _handoff_state(device))]
    for _, st in sts:
        if st['word'] is None:
            continue
        n = int(st['word'].item())
        st['event'] = None
        if n:
            st['word'].zero_()
            for buf in _HANDOFF_FLAGS.values():          # a late SIGNAL may have raised a flag its WAIT no longer took down
                buf.zero_()
            # ... and the device builds its steps WITHOUT hand-offs from here on (handoff_enabled): the probe that allowed them covers
            # one launch shape on one stream at start-up - not a CU-masked stream, a later partition-mode change or the chain's own
            # resource footprint - and a time-out is the evidence that it did not hold.  (Graphs captured earlier keep theirs.)
            st['placement'] = False
            raise _lib.Gd4dError(f'{n} SIGNAL / WAIT hand-off(s) between chain programs timed out: the affected rows are NaN. '
                                 'GD4D_POS_ENCODER=dual / GD4D_TRAIN_REG_BESIDE=0 run the same step without hand-offs.')


def poll_handoff(device):
    """Non-blocking form for eager launches (not inside a graph capture): looks at the copy of the error word an earlier call
    requested, if it has arrived, and requests the next one - a time-out surfaces one call later at the latest, without a sync."""
    if torch.cuda.is_current_stream_capturing():
        return
    st = _handoff_state(device)
    if st['word'] is None:
        return
    if st['event'] is not None and st['event'].query():
        st['event'] = None
        if int(st['pinned'][0]) != 0:
            check_handoff(device)
    if st['event'] is None:
        if st['pinned'] is None:
            st['pinned'] = torch.zeros(1, dtype=I32).pin_memory()
        st['pinned'].copy_(st['word'], non_blocking=True)
        st['event'] = torch.cuda.Event()
        st['event'].record()


def handoff_placement_ok(device):
    """One-time self-test per device: the hand-offs publish their rows to the XCD's L2 only, so they need workgroup j and workgroup
    j + 8 k of a launch on the SAME XCD (what the dispatcher does today, not what any specification promises).
    gd4d_xcd_placement_probe records every workgroup's XCC id; False if the pattern does not hold (or cannot be probed because
    the first use falls inside a graph capture) - the callers then take the schedules without hand-offs."""
    st = _handoff_state(device)
    if st['placement'] is None:
        if torch.cuda.is_current_stream_capturing():
            import warnings
            warnings.warn('graph-detr4d_amd: first use inside a graph capture - the XCD placement self-test cannot run, the step is '
                          'built without SIGNAL / WAIT hand-offs (run one eager forward before capturing to get them)')
            return False
        idx = torch.device(device).index
        with torch.cuda.device(idx if idx is not None else torch.cuda.current_device()):
            blocks = 2048
            out = torch.full((blocks,), -1, device=st['dev'], dtype=I32)
            _call('gd4d_xcd_placement_probe', _dev(out, 'out', I32), blocks)
            ids = out.cpu()
        # (the probe's own shape: 2048 workgroups of one wave on the current stream; a time-out later on turns the hand-offs off
        #  for the device, check_handoff)
        st['placement'] = bool((ids >= 0).all() and (ids == ids[:8].repeat(blocks // 8)).all())
        if not st['placement']:
            import warnings
            warnings.warn('graph-detr4d_amd: workgroups j and j + 8 k do not share an XCD on this device - chain programs run '
                          'without SIGNAL / WAIT hand-offs')
    return st['placement']


def handoff_enabled(device, switch):
    """Whether a step may use hand-offs: the flag `switch` (GD4D_POS_ENCODER=dual / GD4D_TRAIN_REG_BESIDE=0 turn them off) and the
    placement self-test."""
    if not switches.flag(switch):
        return False
    return handoff_placement_ok(device)


def chain_wait(flags, errors=None):
    """Two-program launches: hold this program until the other program's workgroup of the same 16 rows has signalled on
    `flags`; errors: int32 tensor (1 element) that counts waits that gave up (handoff_error_word()).  A WAIT that gives up
    poisons what the program LOADs afterwards (NaN)."""
    return ChainOp(kind=CHAIN_WAIT, src=-1, dst=-1, res=-1, p0=_dev(flags, 'flags', I32).value,
                   gout=None if errors is None else _dev(errors, 'errors', I32).value)


class ChainGuest(ctypes.Structure):
    """gd4d_chain_guest (include/gd4d.h): value_proj of one decoder layer over a few pyramid levels, run by guest workgroups of a
    row-chain launch."""
    _fields_ = [('feats', ctypes.c_void_p * 8), ('level_hw', ctypes.c_int32 * 16), ('L', ctypes.c_int32), ('R', ctypes.c_int32),
                ('chlast', ctypes.c_int32), ('workgroups', ctypes.c_int32), ('image', ctypes.c_void_p), ('out', ctypes.c_void_p)]


_VP_IMAGES = {}


def value_proj_image(weight, bias=None):
    """gd4d_value_proj_image of a layer's value_proj (256, 256) weight and bias: the split-bf16 fragment image the guests of
    row_chain_fwd(..., guest=) stream through LDS, kept while neither changes (invalidate_chain_images)."""
    if not weight.is_cuda or weight.dtype != F32 or tuple(weight.shape) != (256, 256) or not weight.is_contiguous():
        raise ValueError('value_proj_image: a contiguous (256, 256) float32 GPU weight')
    if bias is not None and (bias.dtype != F32 or bias.numel() != 256 or not bias.is_contiguous() or bias.device != weight.device):
        raise ValueError('value_proj_image: bias (256) float32 on the weight\'s GPU')

    def build():
        lib = _lib.load()
        img = torch.empty(int(lib.gd4d_value_proj_image_bytes()), device=weight.device, dtype=U8)
        _call('gd4d_value_proj_image', _dev(weight, 'weight', F32), _opt(bias, 'bias'), _dev(img, 'image'))          # (_on_tensor_device: the weight's device is current)
        return img
    return _kept(_VP_IMAGES, (weight.data_ptr(), None if bias is None else bias.data_ptr()), (weight, bias), build)


def chain_guest(levels, image, out, workgroups=0):
    """A ChainGuest: project `levels` - (R, 256, H, W) / (B, N, 256, H, W) fp32, all contiguous (NCHW) or all stored channels-last -
    with the value_proj whose `image` this is into out (R, sum H W, 256) fp32."""
    chlast = [PyramidView.is_channels_last_level(t) and not t.is_contiguous() for t in levels]
    if any(chlast) != all(chlast) or (not any(chlast) and not all(t.is_contiguous() for t in levels)):
        raise ValueError('chain_guest: the levels must be all NCHW-contiguous or all channels-last')
    if any(t.dtype != F32 or not t.is_cuda or t.shape[-3] != 256 for t in levels) or len(levels) > 4:
        raise ValueError('chain_guest: up to 4 float32 GPU levels of 256 channels')
    r = levels[0].numel() // (256 * levels[0].shape[-1] * levels[0].shape[-2])
    s = sum(t.shape[-1] * t.shape[-2] for t in levels)
    if tuple(out.shape) != (r, s, 256) or out.dtype != F32 or not out.is_contiguous() or out.device != levels[0].device:
        raise ValueError(f'chain_guest: out must be ({r}, {s}, 256) float32, contiguous')
    g = ChainGuest()
    for i, t in enumerate(levels):
        g.feats[i] = t.data_ptr()
        g.level_hw[2 * i], g.level_hw[2 * i + 1] = int(t.shape[-2]), int(t.shape[-1])
    g.L, g.R, g.chlast, g.workgroups = len(levels), r, int(all(chlast)), int(workgroups)
    g.image, g.out = image.data_ptr(), out.data_ptr()
    g._keep = (levels, image, out)
    return g


def value_proj_guest_fwd(guest, max_cus=0):
    """gd4d_value_proj_guest_fwd: a ChainGuest's job as a launch of its own."""
    _call('gd4d_value_proj_guest_fwd', ctypes.byref(guest), int(max_cus))


def row_chain_fwd(program, m, guest=None, fills=None):
    """gd4d_row_chain_fwd: run the list of ChainOp over `m` rows in one launch (the tensors the operations point to must
    stay alive until the stream has run it - the callers keep them in locals / return them).  guest (ChainGuest): the launch
    also carries that value_proj job on the compute units the chain leaves idle (gd4d_row_chain_guest_fwd).  fills (training;
    PyramidGrad.take_fills): it carries those record fills of the pyramid gradient (gd4d_row_chain_fill_fwd)."""
    arr = (ChainOp * len(program))(*program)
    if fills is not None:       # (as guest workgroups of the chain launch)
        _call('gd4d_row_chain_fill_fwd', arr, len(program), None, 0, int(m), *_fill_args(fills), 0)
    elif guest is not None:
        _call('gd4d_row_chain_guest_fwd', arr, len(program), None, 0, int(m), ctypes.byref(guest))
    else:
        _call('gd4d_row_chain_fwd', arr, len(program), int(m))


def row_chain2_fwd(program_a, program_b, m, guest=None, fills=None):
    """gd4d_row_chain2_fwd: two independent programs over the same `m` rows in one launch (each on its own workgroups);
    guest / fills as row_chain_fwd."""
    a = (ChainOp * len(program_a))(*program_a)
    b = (ChainOp * len(program_b))(*program_b)
    if fills is not None:
        _call('gd4d_row_chain_fill_fwd', a, len(program_a), b, len(program_b), int(m), *_fill_args(fills), 0)
    elif guest is not None:
        _call('gd4d_row_chain_guest_fwd', a, len(program_a), b, len(program_b), int(m), ctypes.byref(guest))
    else:
        _call('gd4d_row_chain2_fwd', a, len(program_a), b, len(program_b), int(m))


def row_chain_choice(program_a, program_b=None, guest=False):
    """gd4d_row_chain_choice (no GPU): the name of the chain kernel's instantiation a launch of these program(s) runs - 'generic',
    a table entry ('in_proj', 'initial_reference', 'chain_a', 'chain_b', 'chain_b_last', 'head') or 'generic_train'.  The programs are
    validated as a launch validates them (Gd4dError)."""
    lib = _lib.load()
    a = (ChainOp * len(program_a))(*program_a)
    b = (ChainOp * len(program_b))(*program_b) if program_b else None
    code = lib.gd4d_row_chain_choice(a, len(program_a), b, len(program_b) if program_b else 0, int(bool(guest)))
    _lib.check(code if code < 0 else 0, 'gd4d_row_chain_choice')
    return lib.gd4d_row_chain_choice_name(code).decode()


def row_chain_specialise(on=None):
    """gd4d_row_chain_specialise: False sends every inference chain launch of the PROCESS to the generic kernel (an A/B: same bits),
    True (the default) uses the table of specialised instantiations; None only asks.  Returns the setting before the call."""
    return bool(_lib.load().gd4d_row_chain_specialise(-1 if on is None else int(bool(on))))


def gather_slice_group(ns=None):
    """gd4d_gather_slice_group / gd4d_gather_slice_group_get: how many consecutive slices a fine workgroup of
    cross_attn_agg_coarse_fwd gathers from one set of pairs - 1, 2, 4 or 8 (ValueError otherwise), for every later launch of the
    PROCESS (same bits for every value; a captured graph keeps what it was captured with); None only asks.  Returns the value
    before the call."""
    lib = _lib.load()
    if ns is None:
        return int(lib.gd4d_gather_slice_group_get())
    if ns not in (1, 2, 4, 8):
        raise ValueError('gather_slice_group: 1, 2, 4 or 8 slices per workgroup')
    return int(lib.gd4d_gather_slice_group(int(ns)))


def gather_walk(bq, blk, ns, block=-1, reverse=False):
    """gd4d_gather_walk / gd4d_gather_walk_dir (no GPU): (grid size, position, group) of workgroup `block` in the walk of
    cross_attn_agg_coarse_fwd over `bq` queries in blocks of `blk` with `ns` slices per workgroup; group 8 // ns is the projected
    rows' phase, position and group are -1 for a workgroup with nothing to do.  reverse: the walk of a reversed launch."""
    pos, group = ctypes.c_int(-1), ctypes.c_int(-1)
    if reverse:
        grid = _lib.load().gd4d_gather_walk_dir(int(bq), int(blk), int(ns), 1, int(block), ctypes.byref(pos), ctypes.byref(group))
    else:
        grid = _lib.load().gd4d_gather_walk(int(bq), int(blk), int(ns), int(block), ctypes.byref(pos), ctypes.byref(group))
    _lib.check(grid if grid < 0 else 0, 'gd4d_gather_walk')
    return grid, pos.value, group.value


_WALK_ALTERNATE = [True]


def gather_walk_alternate(on=None):
    """Whether fused_decoder.run_single reverses the gather's walk in every other layer (layer 0 walks forward), for the PROCESS - a
    dev switch for A/B runs from one build: the same bits either way; a captured graph and a recorded request program keep what they
    were made with.  None only asks.  Returns the setting before the call.  (Kept on this side of the library: the decoder reads
    it while it enqueues, where a call into the library is a launch.)"""
    was = _WALK_ALTERNATE[0]
    if on is not None:
        _WALK_ALTERNATE[0] = bool(on)
    return was


def mha_core_presplit_fwd(q, kv, num_heads, attn_mask=None, want_lse=False, dropout_p=0., seed=None):
    """gd4d_mha_core_presplit_fwd: the self-attention core (batch 1) on K / V planes a chain GEMM wrote (KVPlanes).
    q (M, 1, C); attn_mask, want_lse, dropout_p / seed as for mha_core_fwd.  Returns (M, 1, C) [, lse]; without dropout
    bit-identical to mha_core_fwd on the fp32 rows."""
    lq, b, c = q.shape
    _, _, _, _, _, _, kind, mptr, keep = _mha_args(q, q, q, num_heads, attn_mask)
    if b != 1 or lq != kv.m or c != kv.c or num_heads != kv.heads:
        raise ValueError('mha_core_presplit_fwd: batch 1, the planes of these rows')
    if not q.is_cuda or q.dtype != F32 or q.stride(2) != 1:
        raise _lib.Gd4dError('q must be a float32 GPU tensor with unit channel stride')
    d = c // num_heads
    out = torch.empty(lq, 1, c, device=q.device, dtype=F32)
    lse = torch.empty(lq, 1, num_heads, device=q.device, dtype=F32) if want_lse else None
    sptr = _mha_seed(dropout_p, seed, q.device)
    _call('gd4d_mha_core_presplit_fwd', ctypes.c_void_p(q.data_ptr()), ctypes.c_void_p(kv.k.data_ptr()), ctypes.c_void_p(kv.v.data_ptr()),
          _dev(out, 'out'), lq, num_heads, d, q.stride(0), c, kv.k[0].numel(), kv.v[0].numel(), mptr, kind, 1.0 / (d ** 0.5),
          _opt(lse, 'lse', None), float(dropout_p), sptr)
    return (out, lse) if want_lse else out


CROSS_MHA_MAX_SPLITS = 64


class CrossKV:
    """The keys and values of one cross-attention layer as split-bf16 planes in the MFMA fragment layout of gd4d_cross_mha_fwd
    (include/gd4d.h has the layouts): k (3 = hi | mid | lo, B, H, steps of 32 keys, 2, 64, 8) and v (2 = hi | lo, ...) bf16 - the
    scores are taken on six products, the second product on three.  cross_mha_pack_kv fills them.  train: the training form - v
    holds three planes too (gd4d_cross_mha_train_fwd takes P V on six products), vk (V as row fragments) and kv (K as column
    fragments), 3 planes each, are what gd4d_cross_mha_bwd reads beside k.  train='forward' / 'backward': only what that pass reads."""

    def __init__(self, lk, b, device, heads=8, train=False):
        self.lk, self.b, self.heads, self.c = int(lk), int(b), int(heads), 32 * int(heads)
        self.steps = (self.lk + 31) // 32
        if torch.device(device).type != 'cuda':
            raise _lib.Gd4dError('CrossKV must live on the GPU (no CPU fallback in graph-detr4d_amd)')
        self.k = torch.empty(3, self.b, heads, self.steps, 2, 64, 8, device=device, dtype=torch.bfloat16)
        if train not in (False, True, 'forward', 'backward'):
            raise ValueError("CrossKV: train is False, True, 'forward' or 'backward'")
        self.train = train
        self.v = None if train == 'backward' else torch.empty(3 if train else 2, self.b, heads, self.steps, 2, 64, 8, device=device,
                                                              dtype=torch.bfloat16)
        self.vk = torch.empty_like(self.k) if train in (True, 'backward') else None
        self.kv = torch.empty_like(self.k) if train in (True, 'backward') else None

    @property
    def plane(self):
        return self.k[0].numel()

    def k_rows(self):
        """(3, steps * 32, B, C): the planes as plain rows (tests)."""
        b, h, s = self.b, self.heads, self.steps
        # [plane][b][h][s][t][g][key % 16][c % 8]  ->  key = 32 s + 16 t + key % 16, channel = 32 h + 8 g + c % 8
        return self.k.view(3, b, h, s, 2, 4, 16, 8).permute(0, 3, 4, 6, 1, 2, 5, 7).reshape(3, s * 32, b, h * 32)

    def v_rows(self):
        """(2, steps * 32, B, C): the planes as plain rows (tests)."""
        b, h, s = self.b, self.heads, self.steps
        # [plane][b][h][s][half][g][d % 16][t][r]  ->  key = 32 s + 16 t + 4 g + r, channel = 32 h + 16 half + d % 16
        n = self.v.shape[0]
        return self.v.view(n, b, h, s, 2, 4, 16, 2, 4).permute(0, 3, 7, 5, 8, 1, 2, 4, 6).reshape(n, s * 32, b, h * 32)


def _rows_lbc(t, name):
    """The row stride of a float32 GPU tensor (L, B, C') addressed as rows l B + b: contiguous, or a last-dim slice of a wider one."""
    if not t.is_cuda or t.dtype != F32:
        raise _lib.Gd4dError(f'{name} must be a float32 GPU tensor')
    if t.dim() != 3 or t.stride(2) != 1 or t.stride(0) != t.stride(1) * t.shape[1]:
        raise ValueError(f'{name} must be row-strided (L, B, C)')
    return t.stride(1)


def cross_mha_pack_kv(k, v, kv=None, num_heads=8, train=False):
    """gd4d_cross_mha_pack_kv: k, v (Lk, B, C) float32 - contiguous, or the two halves of one (Lk, B, 2C) projection - split to bf16
    pieces once (k: hi / mid / lo, v: hi / lo), into the planes gd4d_cross_mha_fwd reads (pad keys of the last step written as zeros).  Returns the CrossKV.
    train (True, 'forward', 'backward'): gd4d_cross_mha_pack_kv_train - the training form, see CrossKV."""
    ldk, ldv = _rows_lbc(k, 'k'), _rows_lbc(v, 'v')
    lk, b, c = k.shape
    if tuple(v.shape) != (lk, b, c) or c != 32 * num_heads:
        raise ValueError('cross_mha_pack_kv: k and v (Lk, B, 32 heads)')
    if kv is None:
        kv = CrossKV(lk, b, k.device, num_heads, train=train)
    elif (kv.lk, kv.b, kv.heads) != (lk, b, num_heads) or getattr(kv, 'train', False) != train:
        raise ValueError('cross_mha_pack_kv: the planes were made for another shape or form')
    if train:
        _call('gd4d_cross_mha_pack_kv_train', ctypes.c_void_p(k.data_ptr()), ctypes.c_void_p(v.data_ptr()), ldk, ldv, _dev(kv.k, 'kv.k'),
              _opt(kv.v, 'kv.v', None), _opt(kv.vk, 'kv.vk', None), _opt(kv.kv, 'kv.kv', None), kv.plane, lk, b, num_heads, 32)
        return kv
    _call('gd4d_cross_mha_pack_kv', ctypes.c_void_p(k.data_ptr()), ctypes.c_void_p(v.data_ptr()), ldk, ldv, _dev(kv.k, 'kv.k'),
          _dev(kv.v, 'kv.v'), kv.plane, lk, b, num_heads, 32)
    return kv


class CrossMhaPlan:
    """cross_mha_plan's answer: q_tile queries per workgroup, `splits` key ranges of whole 32-key steps - ranges[i] = [first, last)
    keys of split i - and the launch's grid (query blocks, heads x splits, batch)."""

    def __init__(self, raw, lk):
        self.q_tile, self.splits, self.steps = raw[0], raw[1], raw[2]
        self.grid = (raw[3], raw[4], raw[5])
        self.ranges = [(32 * raw[6 + i], min(int(lk), 32 * raw[7 + i])) for i in range(self.splits)]

    @property
    def workgroups(self):
        return self.grid[0] * self.grid[1] * self.grid[2]


def cross_mha_plan(lq, lk, b, heads=8, q_tile=0, splits=0):
    """gd4d_cross_mha_plan (no GPU): how cross_mha_fwd divides (lq, lk, b, heads) among workgroups.  q_tile / splits: 0 = the
    library's choice (what a cross_mha_fwd call without them uses)."""
    raw = (ctypes.c_int32 * (7 + CROSS_MHA_MAX_SPLITS))()
    _lib.check(_lib.load().gd4d_cross_mha_plan(int(lq), int(lk), int(b), int(heads), int(q_tile), int(splits), raw), 'gd4d_cross_mha_plan')
    return CrossMhaPlan(list(raw), lk)


def _cross_mha_mask(key_padding_mask, b, lk):
    if key_padding_mask is None:
        return None, None
    if key_padding_mask.dtype not in (torch.bool, U8) or tuple(key_padding_mask.shape) != (b, lk):
        raise ValueError(f'key_padding_mask must be bool / uint8 ({b}, {lk})')
    key_padding_mask = key_padding_mask.contiguous().view(U8)
    return key_padding_mask, _dev(key_padding_mask, 'key_padding_mask', U8)


def cross_mha_fwd(q, kv, num_heads, key_padding_mask=None, want_lse=False, q_tile=0, splits=0, dropout_p=0., seed=None):
    """gd4d_cross_mha_fwd: softmax(q k^T / sqrt(32) + key-padding mask) v on the planes of `kv` (CrossKV).  q (Lq, B, C) float32,
    contiguous or a last-dim slice; key_padding_mask (B, Lk) bool / uint8, nonzero = ignore the key.  Returns (Lq, B, C) [, lse
    (Lq, B, heads)].  q_tile / splits: cross_mha_plan's (0 = the library's choice).  On training planes (cross_mha_pack_kv(train=True
    or 'forward')) it is gd4d_cross_mha_train_fwd: P V on six products, a 32-query tile, and with dropout_p and seed (mha_dropout_seed)
    dropout of the probabilities as mha_core_fwd draws it (mha_dropout_keep_mask rebuilds the mask)."""
    ldq = _rows_lbc(q, 'q')
    lq, b, c = q.shape
    if not isinstance(kv, CrossKV) or kv.v is None:
        raise TypeError('cross_mha_fwd: kv must be a CrossKV with the planes of the forward (cross_mha_pack_kv)')
    if b != kv.b or c != kv.c or num_heads != kv.heads:
        raise ValueError('cross_mha_fwd: the planes were made for another batch, width or head count')
    train = bool(getattr(kv, 'train', False))
    if dropout_p and not train:
        raise ValueError("cross_mha_fwd: dropout needs the training planes (cross_mha_pack_kv(train=True or 'forward'))")
    if train and not q_tile:
        q_tile = 32
    key_padding_mask, mptr = _cross_mha_mask(key_padding_mask, b, kv.lk)
    sptr = _mha_seed(dropout_p, seed, q.device)
    lib = _lib.load()
    ws_bytes = int(lib.gd4d_cross_mha_workspace_bytes(lq, kv.lk, b, num_heads, int(q_tile), int(splits)))
    ws = torch.empty(ws_bytes // 4, device=q.device, dtype=F32) if ws_bytes else None
    out = torch.empty(lq, b, c, device=q.device, dtype=F32)
    lse = torch.empty(lq, b, num_heads, device=q.device, dtype=F32) if want_lse else None
    args = (ctypes.c_void_p(q.data_ptr()), _dev(kv.k, 'kv.k'), _dev(kv.v, 'kv.v'), kv.plane, mptr, _dev(out, 'out'),
            _opt(lse, 'lse'), _opt(ws, 'workspace'), ws_bytes, lq, kv.lk, b, num_heads, 32, ldq, c, 1.0 / (32 ** 0.5), int(q_tile), int(splits))
    if train:
        _call('gd4d_cross_mha_train_fwd', *args, float(dropout_p), sptr)
    else:
        _call('gd4d_cross_mha_fwd', *args)
    return (out, lse) if want_lse else out


class CrossMhaBwdPlan:
    """cross_mha_bwd_plan's answer.  Query-side kernel: q_tile queries per workgroup, `splits` key ranges (ranges[i] = [first, last)
    keys), query_grid, query_block; key-side kernel: key_block keys per workgroup, key_grid, key_block_threads; workspace bytes of
    the query-side pack (pack_bytes, read by both kernels), of the split partials (partial_bytes) and their sum (workspace_bytes)."""

    def __init__(self, raw, lk):
        self.q_tile, self.splits, self.steps, self.query_steps = raw[0], raw[1], raw[2], raw[3]
        self.query_grid, self.query_block = (raw[4], raw[5], raw[6]), raw[7]
        self.key_block, self.key_grid, self.key_block_threads = raw[8], (raw[9], raw[10], raw[11]), raw[12]
        self.pack_bytes, self.partial_bytes, self.workspace_bytes = raw[13], raw[14], raw[15]
        self.ranges = [(32 * raw[16 + i], min(int(lk), 32 * raw[17 + i])) for i in range(self.splits)]

    def __repr__(self):
        return (f'CrossMhaBwdPlan(query side: grid {self.query_grid} x {self.query_block} threads, {self.q_tile} queries, {self.splits} splits; '
                f'key side: grid {self.key_grid} x {self.key_block_threads} threads, {self.key_block} keys; workspace {self.pack_bytes} + '
                f'{self.partial_bytes} bytes)')


def cross_mha_bwd_plan(lq, lk, b, heads=8, q_tile=0, splits=0):
    """gd4d_cross_mha_bwd_plan (no GPU): grids, blocks and workspace of cross_mha_bwd's two compute kernels."""
    raw = (ctypes.c_int64 * (17 + CROSS_MHA_MAX_SPLITS))()
    _lib.check(_lib.load().gd4d_cross_mha_bwd_plan(int(lq), int(lk), int(b), int(heads), int(q_tile), int(splits), raw),
               'gd4d_cross_mha_bwd_plan')
    return CrossMhaBwdPlan(list(raw), lk)


def cross_mha_bwd(grad_out, q, out, lse, kv, num_heads, key_padding_mask=None, dropout_p=0., seed=None, q_tile=0, splits=0,
                  packed_kv=False, workspace=None):
    """gd4d_cross_mha_bwd: the gradients of cross_mha_fwd's q, k and v from grad_out, q, out, lse (want_lse) and the training planes
    of k and v (cross_mha_pack_kv(train=True)); key_padding_mask, dropout_p and seed as in the forward.  Returns (dq (Lq, B, C), dk,
    dv (Lk, B, C)); packed_kv: (dq, dkv (Lk, B, 2C)) - dk | dv written as the two halves of one buffer, what the backward of a K|V
    projection takes.  Rows of masked keys are exact zeros.  A row whose keys are all masked has unspecified gradients.
    workspace: a float32 tensor of at least cross_mha_bwd_plan(...).workspace_bytes to use instead of a new one (its content does
    not matter: every element that is read is written first)."""
    ldq, ldo, ldg = _rows_lbc(q, 'q'), _rows_lbc(out, 'out'), _rows_lbc(grad_out, 'grad_out')
    lq, b, c = q.shape
    if not isinstance(kv, CrossKV) or kv.vk is None:
        raise TypeError('cross_mha_bwd: kv must be a CrossKV with the training planes (cross_mha_pack_kv(train=True))')
    if b != kv.b or c != kv.c or num_heads != kv.heads:
        raise ValueError('cross_mha_bwd: the planes were made for another batch, width or head count')
    if tuple(out.shape) != (lq, b, c) or tuple(grad_out.shape) != (lq, b, c) or tuple(lse.shape) != (lq, b, num_heads):
        raise ValueError('cross_mha_bwd: out, grad_out (Lq, B, C) and lse (Lq, B, heads) of the forward call')
    key_padding_mask, mptr = _cross_mha_mask(key_padding_mask, b, kv.lk)
    sptr = _mha_seed(dropout_p, seed, q.device)
    lib = _lib.load()
    ws_bytes = int(lib.gd4d_cross_mha_bwd_workspace_bytes(lq, kv.lk, b, num_heads, int(q_tile), int(splits)))
    ws = torch.empty(max(ws_bytes, 16) // 4, device=q.device, dtype=F32) if workspace is None else workspace
    if ws.dtype != F32 or ws.numel() * 4 < ws_bytes:
        raise ValueError(f'cross_mha_bwd: workspace must be float32 of at least {ws_bytes} bytes')
    dq = torch.empty(lq, b, c, device=q.device, dtype=F32)
    if packed_kv:
        dkv = torch.empty(kv.lk, b, 2 * c, device=q.device, dtype=F32)
        dk, dv, ldd = dkv[..., :c], dkv[..., c:], 2 * c
    else:
        dk = torch.empty(kv.lk, b, c, device=q.device, dtype=F32)
        dv = torch.empty(kv.lk, b, c, device=q.device, dtype=F32)
        ldd = c
    vp = lambda t: ctypes.c_void_p(t.data_ptr())    # noqa: E731
    _call('gd4d_cross_mha_bwd', vp(grad_out), vp(q), vp(out), _dev(lse, 'lse', F32), _dev(kv.k, 'kv.k'), _dev(kv.vk, 'kv.vk'),
          _dev(kv.kv, 'kv.kv'), kv.plane, mptr, _dev(dq, 'dq'), vp(dk), vp(dv), _dev(ws, 'workspace'), ws_bytes, lq, kv.lk, b, num_heads,
          32, ldg, ldq, ldo, c, ldd, ldd, 1.0 / (32 ** 0.5), float(dropout_p), sptr, int(q_tile), int(splits))
    return (dq, dkv) if packed_kv else (dq, dk, dv)


class RequestRef(ctypes.Structure):
    """gd4d_request_ref (include/gd4d.h)."""
    _fields_ = [('binding', ctypes.c_int32), ('reserved', ctypes.c_int32), ('value', ctypes.c_int64)]


class RequestPatch(ctypes.Structure):
    """gd4d_request_patch (include/gd4d.h)."""
    _fields_ = [('table', ctypes.c_int32), ('binding', ctypes.c_int32), ('offset', ctypes.c_int64), ('add', ctypes.c_int64)]


class RequestBinding(ctypes.Union):
    """gd4d_request_binding (include/gd4d.h)."""
    _fields_ = [('ptr', ctypes.c_void_p), ('scalar', ctypes.c_double)]


class RequestStep(ctypes.Structure):
    """gd4d_request_step (include/gd4d.h)."""
    _fields_ = [('kind', ctypes.c_int32), ('side', ctypes.c_int32), ('event', ctypes.c_int32), ('npatches', ctypes.c_int32),
                ('nops_a', ctypes.c_int32), ('nops_b', ctypes.c_int32), ('fbind', ctypes.c_int32 * 2),
                ('prog_a', ctypes.c_void_p), ('prog_b', ctypes.c_void_p), ('guest', ctypes.c_void_p), ('patches', ctypes.c_void_p),
                ('p', RequestRef * 10), ('i', ctypes.c_int32 * 10), ('l', ctypes.c_int64 * 2), ('f', ctypes.c_float * 2),
                ('table', ctypes.c_void_p * 5), ('table_bytes', ctypes.c_int64 * 5)]


(REQ_ROW_CHAIN, REQ_ROW_CHAIN2, REQ_ROW_CHAIN_GUEST, REQ_MHA_CORE, REQ_MHA_PRESPLIT, REQ_PLAN, REQ_AGG_COARSE, REQ_AGG_ITEMS,
 REQ_AGG_SLICED, REQ_SLICE_PLANAR, REQ_VALUE_PROJ_GUEST, REQ_QUERY_ORDER, REQ_EVENT_RECORD, REQ_STREAM_WAIT, REQ_COPY) = range(1, 16)


def _addr(a):
    """The address in a pointer argument as the wrappers above hand it to ctypes: None, c_void_p or int."""
    if a is None:
        return 0
    if isinstance(a, int):
        return a
    return a.value or 0


def tensor_extent(t):
    """[lo, hi): the bytes a strided tensor can touch."""
    span = sum((n - 1) * st for n, st in zip(t.shape, t.stride())) + 1 if t.numel() else 0
    return t.data_ptr(), t.data_ptr() + span * t.element_size()


class _Pending:
    """One recorded enqueue, addresses still raw (StepRecorder.steps resolves them against the bindings)."""

    def __init__(self, kind, side, **kw):
        self.kind, self.side, self.event = kind, side, 0
        self.prog_a = self.prog_b = self.guest = None
        self.p, self.i, self.l, self.f, self.tables, self.special, self.fbind = [], [], [], [], [], {}, [-1, -1]
        for k, v in kw.items():
            setattr(self, k, v)


_CHAIN_POINTERS = ('p0', 'p1', 'p2', 'gout', 'p3')


class StepRecorder:
    """What _lib.load() returns inside `with _lib.recording(rec)`: the library with every launching entry point of the decoder request
    turned into a step record.  The wrappers of this file - and so fused_decoder.run_single, functional.LateValues, the chain_*
    descriptors, the weight images, the hand-off flags - run unchanged; what they would have enqueued is what gd4d_decoder_request_run
    enqueues later (one description of the schedule).  Entry points that build a value kept from parameters (weight images) or probe the
    device run at once, as always; a launching entry point without a step kind raises.  Tensors the recorded code allocates must stay
    where they are for the life of the program: the caller records under a private memory pool that it keeps."""

    RUN_NOW = {'gd4d_chain_weight_image', 'gd4d_chain_weight_image_exact', 'gd4d_value_proj_image', 'gd4d_xcd_placement_probe'}

    def __init__(self, lib, main_stream):
        self._lib, self.main, self.side = lib, int(main_stream), None
        self.pending, self.events = [], 0

    def __getattr__(self, name):
        if name.startswith('gd4d_'):
            fn = getattr(self._lib, name)
            if name in self.RUN_NOW or not fn.argtypes or name.endswith('_bytes') or fn.restype is not ctypes.c_int:
                return fn
            raise _lib.Gd4dError(f'{name}: a request program (GD4D_REQUEST=1) has no step for this entry point - the route '
                                 'switches in force select a schedule it does not cover')
        raise AttributeError(name)

    # ---- streams and events -------------------------------------------------------------------------------------------
    def _side(self, handle):
        handle = int(_addr(handle))
        if handle == self.main:
            return 0
        if self.side not in (None, handle):
            raise _lib.Gd4dError('a request program runs on two streams: the caller\'s and one side stream')
        self.side = handle
        return 1

    def record_event(self, stream):
        """Event.record(stream): returns the event's id."""
        if self.events >= 64:
            raise _lib.Gd4dError('a request program holds at most 64 events')
        self.pending.append(_Pending(REQ_EVENT_RECORD, self._side(stream.cuda_stream), event=self.events))
        self.events += 1
        return self.events - 1

    def wait_event(self, stream, event):
        self.pending.append(_Pending(REQ_STREAM_WAIT, self._side(stream.cuda_stream), event=event))

    def copy(self, dst, src):
        if not (dst.is_contiguous() and src.is_contiguous()) or dst.numel() != src.numel() or dst.dtype != src.dtype:
            raise ValueError('request program: a copy step takes two dense tensors of one size')
        self.pending.append(_Pending(REQ_COPY, self._side(torch.cuda.current_stream(dst.device).cuda_stream),
                                     p=[dst.data_ptr(), src.data_ptr()], l=[dst.numel() * dst.element_size()]))

    # ---- the entry points ---------------------------------------------------------------------------------------------
    @staticmethod
    def _ops(arr, n):
        return None if arr is None or n == 0 else (ChainOp * n).from_buffer_copy(arr)

    @staticmethod
    def _guest(ref):
        return ChainGuest.from_buffer_copy(ref._obj)

    def gd4d_row_chain_fwd(self, a, na, m, stream):
        self.pending.append(_Pending(REQ_ROW_CHAIN, self._side(stream), prog_a=self._ops(a, na), i=[m]))
        return 0

    def gd4d_row_chain2_fwd(self, a, na, b, nb, m, stream):
        self.pending.append(_Pending(REQ_ROW_CHAIN2, self._side(stream), prog_a=self._ops(a, na), prog_b=self._ops(b, nb), i=[m]))
        return 0

    def gd4d_row_chain_guest_fwd(self, a, na, b, nb, m, guest, stream):
        self.pending.append(_Pending(REQ_ROW_CHAIN_GUEST, self._side(stream), prog_a=self._ops(a, na), prog_b=self._ops(b, nb), i=[m],
                                     guest=self._guest(guest)))
        return 0

    def gd4d_value_proj_guest_fwd(self, guest, max_cus, stream):
        self.pending.append(_Pending(REQ_VALUE_PROJ_GUEST, self._side(stream), guest=self._guest(guest), i=[max_cus]))
        return 0

    def gd4d_mha_core_fwd(self, q, k, v, mask, out, lq, lk, b, h, d, ldq, ldk, ldv, ldo, kind, scale, lse, drop_p, seed, stream):
        if _addr(lse) or drop_p:
            raise _lib.Gd4dError('request program: the attention core without lse / dropout (inference)')
        self.pending.append(_Pending(REQ_MHA_CORE, self._side(stream), p=[q, k, v, mask, out], i=[lq, lk, b, h, d, ldq, ldk, ldv, ldo, kind],
                                     f=[scale]))
        return 0

    def gd4d_mha_core_presplit_fwd(self, q, kp, vp, out, l, h, d, ldq, ldo, ks, vs, mask, kind, scale, lse, drop_p, seed, stream):
        if _addr(lse) or drop_p:
            raise _lib.Gd4dError('request program: the attention core without lse / dropout (inference)')
        self.pending.append(_Pending(REQ_MHA_PRESPLIT, self._side(stream), p=[q, kp, vp, out, mask], i=[l, h, d, ldq, ldo, kind], l=[ks, vs],
                                     f=[scale]))
        return 0

    def gd4d_cross_attn_plan_fwd(self, ref, off, att, cam, l2i, rng, img_h, img_w, lv, cs, pix, plan, plan_bytes, wsum, mask_out, uv_out,
                                 b, n, q, hh, nl, p, flags, order, stream):
        # lidar2img, img_h and img_w are the request's (functional.lidar2img_device / img_hw): bound by position, not by address
        self.pending.append(_Pending(REQ_PLAN, self._side(stream), p=[ref, off, att, cam, l2i, plan, wsum, mask_out, uv_out, order],
                                     special={4: 'lidar2img'}, fbind=['img_h', 'img_w'], f=[img_h, img_w], l=[pix, plan_bytes],
                                     i=[b, n, q, hh, nl, p, flags], tables=[(rng, False), (lv, False), (cs, False)]))
        return 0

    def gd4d_cross_attn_agg_items_coarse_fwd(self, ptrs, lv, cs, pix, sl, pp, pcs, plan, agg, wsum, pagg, b, n, q, hh, c, nl, p, dt, order,
                                             stream):
        self.pending.append(_Pending(REQ_AGG_COARSE, self._side(stream), p=[plan, agg, wsum, pagg, order], l=[pix, sl],
                                     i=[b, n, q, hh, c, nl, p, dt],
                                     tables=[(ptrs, True), (lv, False), (cs, False), (pp, True), (pcs, False)]))
        return 0

    def gd4d_cross_attn_agg_items_fwd(self, ptrs, lv, cs, pix, sl, plan, agg, wsum, b, n, q, hh, c, nl, p, dt, order, lo, cnt, stream):
        self.pending.append(_Pending(REQ_AGG_ITEMS, self._side(stream), p=[plan, agg, wsum, order], l=[pix, sl],
                                     i=[b, n, q, hh, c, nl, p, dt, lo, cnt], tables=[(ptrs, True), (lv, False), (cs, False)]))
        return 0

    def gd4d_cross_attn_agg_sliced_fwd(self, ptrs, sl, plan, agg, b, n, q, hh, c, nl, p, dt, order, lo, cnt, stream):
        self.pending.append(_Pending(REQ_AGG_SLICED, self._side(stream), p=[plan, agg, order], l=[sl],
                                     i=[b, n, q, hh, c, nl, p, dt, lo, cnt], tables=[(ptrs, True)]))
        return 0

    def gd4d_pyramid_slice_planar_fwd(self, feats, lv, out, r, c, nl, in_dt, out_dt, max_cus, stream):
        self.pending.append(_Pending(REQ_SLICE_PLANAR, self._side(stream), p=[out], i=[r, c, nl, in_dt, out_dt, max_cus],
                                     tables=[(feats, True), (lv, False)]))
        return 0

    def gd4d_query_order_fwd(self, ref, rng, order, b, q, stream):
        self.pending.append(_Pending(REQ_QUERY_ORDER, self._side(stream), p=[ref, order], i=[b, q], tables=[(rng, False)]))
        return 0

    # ---- resolution ---------------------------------------------------------------------------------------------------
    def steps(self, bindings, named):
        """The recorded enqueues as a (RequestStep * n) array plus everything it points to (keep both alive until
        gd4d_decoder_request_create has copied them).  bindings: {index: tensor} - an address inside a binding's extent becomes
        (index, offset), the base address of one wins over the extent of another (query and query_pos interleave as column slices of
        one tensor); named: {'lidar2img': index, 'img_h': index, 'img_w': index}."""
        exact = {t.data_ptr(): k for k, t in bindings.items()}
        extents = [(*tensor_extent(t), k) for k, t in bindings.items()]

        def find(addr):
            if addr == 0:
                return None
            if addr in exact:
                return exact[addr], 0
            for lo, hi, k in extents:
                if lo <= addr < hi:
                    return k, addr - lo
            return None

        keep, arr = [], (RequestStep * len(self.pending))()
        for s, pd in zip(arr, self.pending):
            s.kind, s.side, s.event = pd.kind, pd.side, pd.event
            patches = []
            for slot, prog in ((0, pd.prog_a), (1, pd.prog_b)):
                if prog is None:
                    continue
                for n, op in enumerate(prog):
                    for name in _CHAIN_POINTERS:
                        hit = find(getattr(op, name) or 0)
                        if hit is not None:
                            patches.append(RequestPatch(slot, hit[0], n * ctypes.sizeof(ChainOp) + getattr(ChainOp, name).offset, hit[1]))
                keep.append(prog)
                if slot == 0:
                    s.prog_a, s.nops_a = ctypes.addressof(prog), len(prog)
                else:
                    s.prog_b, s.nops_b = ctypes.addressof(prog), len(prog)
            if pd.guest is not None:
                g = pd.guest
                where = [(ChainGuest.feats.offset + 8 * n, g.feats[n] or 0) for n in range(g.L)] + \
                        [(ChainGuest.image.offset, g.image or 0), (ChainGuest.out.offset, g.out or 0)]
                for offset, addr in where:
                    hit = find(addr)
                    if hit is not None:
                        patches.append(RequestPatch(2, hit[0], offset, hit[1]))
                keep.append(g)
                s.guest = ctypes.addressof(g)
            for n, a in enumerate(pd.p):
                addr = int(_addr(a))
                hit = (named[pd.special[n]], 0) if n in pd.special else find(addr)
                s.p[n] = RequestRef(-1, 0, addr) if hit is None else RequestRef(hit[0], 0, hit[1])
            for n, v in enumerate(pd.i):
                s.i[n] = int(v)
            for n, v in enumerate(pd.l):
                s.l[n] = int(v)
            for n, v in enumerate(pd.f):
                s.f[n] = float(v)
            s.fbind[0], s.fbind[1] = [named[x] if isinstance(x, str) else -1 for x in pd.fbind]
            for n, (table, pointers) in enumerate(pd.tables):
                raw = bytes(table)
                buf = ctypes.create_string_buffer(raw, len(raw))
                if pointers:
                    for j in range(len(raw) // 8):
                        hit = find(int.from_bytes(raw[8 * j:8 * j + 8], 'little'))
                        if hit is not None:
                            patches.append(RequestPatch(3 + n, hit[0], 8 * j, hit[1]))
                keep.append(buf)
                s.table[n], s.table_bytes[n] = ctypes.addressof(buf), len(raw)
            if patches:
                parr = (RequestPatch * len(patches))(*patches)
                keep.append(parr)
                s.patches, s.npatches = ctypes.addressof(parr), len(patches)
        return arr, keep


def copy_into(dst, src):
    """dst.copy_(src) - or, while a request program is being recorded, its copy step."""
    rec = _lib.recorder()
    if rec is None:
        return dst.copy_(src)
    rec.copy(dst, src)
    return dst


def _weight_image(entry, nbytes, unsupported, weight, *dims, name='weight'):
    """The common tail of the convolutions' weight-image wrappers: nbytes (the entry's *_bytes; 0: a weight the kernel does not take, which
    raises `unsupported`) of device memory, filled by lib.<entry>(weight, *dims, image, stream)."""
    if nbytes == 0:
        raise _lib.Gd4dError(unsupported)
    img = torch.empty(nbytes, device=weight.device, dtype=U8)
    _call(entry, _dev(weight.contiguous(), name, F32), *dims, _dev(img, 'image', U8))
    return img


def depth_net_image(conv_w):
    """gd4d_depth_net_image: the camera-aware DepthNet's 3x3 weight (256, 256, 3, 3) fp32 -> its bf16 hi / lo fragment image for
    depth_conv_fwd (2.25 MB; remake it when the weight changes)."""
    c = int(conv_w.shape[0])
    nbytes = int(_lib.load().gd4d_depth_net_image_bytes(c)) if tuple(conv_w.shape) == (c, c, 3, 3) else 0
    return _weight_image('gd4d_depth_net_image', nbytes, f'depth_net_image: weight {tuple(conv_w.shape)}; the kernel takes (256, 256, 3, 3)',
                         conv_w, c, name='conv_w')


def cam_gate_fwd(intrinsics, ida00, fc1_w, fc1_b, fc2_w, fc2_b, se_reduce_w, se_reduce_b, se_expand_w, se_expand_b,
                 scale_depth_factor=1000.0, out=None):
    """gd4d_cam_gate_fwd: intrinsics (N, 4, 4), ida00 (1 or N) = ida[..., 0, 0] -> the camera gate (N, 256) =
    sigmoid(se(mlp(pixel_size * scale_depth_factor / aug_scale))) of DepthNet.forward (detr3d_head_pe_camaware.py:86-100).
    The weights as the modules hold them (mlp.fc1 (256, 1), 1x1 convolutions (256, 256, 1, 1))."""
    n = intrinsics.shape[0]
    if tuple(intrinsics.shape) != (n, 4, 4) or ida00.dim() != 1:
        raise ValueError('cam_gate_fwd: intrinsics (N, 4, 4) and ida00 (1 or N) expected')
    c = fc2_w.shape[0]
    out = _out(out, (n, c), intrinsics.device, 'cam_gate_fwd: out')
    w = [t.detach().contiguous() for t in (fc1_w, fc1_b, fc2_w, fc2_b, se_reduce_w, se_reduce_b, se_expand_w, se_expand_b)]
    names = ('fc1_w', 'fc1_b', 'fc2_w', 'fc2_b', 'se_reduce_w', 'se_reduce_b', 'se_expand_w', 'se_expand_b')
    _call('gd4d_cam_gate_fwd', _dev(intrinsics, 'intrinsics', F32), _dev(ida00, 'ida00', F32), int(n), int(ida00.shape[0]),
          float(scale_depth_factor), *[_dev(t, nm, F32) for t, nm in zip(w, names)], int(c), _dev(out, 'out', F32))
    return out


def depth_conv_fwd(feats, image, bias, bn_mean, bn_var, bn_weight, bn_bias, eps, gate, outs=None):
    """gd4d_depth_conv_fwd: L <= 4 levels (N, 256, H_l, W_l) fp32 NCHW -> relu(BN(conv3x3(x) + bias)) * gate[:, :, None, None]
    per level, all levels in one launch.  image = depth_net_image(reduce_conv[0].weight); BN with its running statistics;
    gate (N, 256) (cam_gate_fwd).  outs: the L (N, 256, H_l, W_l) tensors to write."""
    nl = len(feats)
    n = feats[0].shape[0]
    if any(f.dim() != 4 or f.shape[0] != n or f.shape[1] != feats[0].shape[1] for f in feats):
        raise ValueError('depth_conv_fwd: levels (N, C, H, W) with the same N and C expected')
    if outs is None:
        outs = [torch.empty(f.shape, device=f.device, dtype=F32) for f in feats]
    elif len(outs) != nl or any(tuple(o.shape) != tuple(f.shape) for o, f in zip(outs, feats)):
        raise ValueError('depth_conv_fwd: outs must match the levels\' shapes')
    fp = _ptrs(feats, 'feats')
    op = _ptrs(outs, 'outs')
    lv = _levels(feats)
    _call('gd4d_depth_conv_fwd', fp, op, lv, nl, int(n), int(feats[0].shape[1]), _dev(image, 'image', U8), _dev(bias, 'bias', F32),
          _dev(bn_mean, 'bn_mean', F32), _dev(bn_var, 'bn_var', F32), _dev(bn_weight, 'bn_weight', F32), _dev(bn_bias, 'bn_bias', F32),
          float(eps), _dev(gate, 'gate', F32))
    return outs


def _depth_levels(what, *lists):
    """The level table of a DepthNet training call: every list holds L (N, C, H_l, W_l) tensors of the same shapes."""
    first = lists[0]
    nl, n, c = len(first), first[0].shape[0], first[0].shape[1]
    if any(f.dim() != 4 or f.shape[0] != n or f.shape[1] != c for f in first):
        raise ValueError(f'{what}: levels (N, C, H, W) with the same N and C expected')
    for other in lists[1:]:
        if len(other) != nl or any(tuple(o.shape) != tuple(f.shape) for o, f in zip(other, first)):
            raise ValueError(f'{what}: every list must match the levels\' shapes')
    return nl, int(n), int(c), _levels(first)


def depth_net_image_t(conv_w):
    """gd4d_depth_net_image_mode(transposed = 1): the image of w'[ic, oc, 2 - ky, 2 - kx] = w[oc, ic, ky, kx], with which depth_conv_raw run
    on dy gives the input gradient (remake it when the weight changes, as depth_net_image)."""
    c = int(conv_w.shape[0])
    nbytes = int(_lib.load().gd4d_depth_net_image_bytes(c)) if tuple(conv_w.shape) == (c, c, 3, 3) else 0
    return _weight_image('gd4d_depth_net_image_mode', nbytes,
                         f'depth_net_image_t: weight {tuple(conv_w.shape)}; the kernel takes (256, 256, 3, 3)', conv_w, c, 1, name='conv_w')


def depth_conv_tiles(level_hw, n):
    """gd4d_depth_conv_tiles: the number of 16 x 16 tiles of the levels [(H, W), ...] with N cameras (the conv's grid)."""
    lv = _levels(level_hw)
    return int(_lib.load().gd4d_depth_conv_tiles(lv, len(level_hw), int(n)))


def depth_conv_raw(feats, image, bias=None, want_partials=False, outs=None, partials=None):
    """gd4d_depth_conv_raw: L <= 4 levels (N, 256, H_l, W_l) -> conv3x3 (+ bias) per level, one launch, no BatchNorm / ReLU / gate.
    want_partials: also returns the (tiles, 2, 256) per-tile mean / M2 partials depth_bn_stats merges (written into `partials` when
    given)."""
    lib = _lib.load()
    if outs is None:
        outs = [torch.empty(f.shape, device=f.device, dtype=F32) for f in feats]
    nl, n, c, lv = _depth_levels('depth_conv_raw', feats, outs)
    if want_partials:
        tiles = int(lib.gd4d_depth_conv_tiles(lv, nl, n))
        partials = _out(partials, (max(tiles, 1), 2, 256), feats[0].device, 'depth_conv_raw: partials')
    elif partials is not None:
        raise ValueError('depth_conv_raw: partials given without want_partials')
    _call('gd4d_depth_conv_raw', _ptrs(feats, 'feats'), _ptrs(outs, 'outs'), lv, nl, n, c, _dev(image, 'image', U8), _opt(bias, 'bias'),
          _opt(partials, 'partials'))
    return (outs, partials) if want_partials else outs


def depth_bn_stats(partials, level_hw, n, bn_weight, running_mean, running_var, momentum, eps, frozen=False):
    """gd4d_depth_bn_stats: stats (L, 3, 256) = mu, rstd, scale per level from depth_conv_raw's partials (frozen: from the running
    buffers, partials may be None); not frozen: running_mean / running_var are updated in place, level after level."""
    nl = len(level_hw)
    lv = _levels(level_hw)
    if not frozen and partials is None:
        raise ValueError('depth_bn_stats: partials are needed unless frozen')
    stats = torch.empty(nl, 3, 256, device=bn_weight.device, dtype=F32)
    _call('gd4d_depth_bn_stats', _opt(partials, 'partials'), lv, nl, int(n), int(bn_weight.shape[0]), _dev(bn_weight, 'bn_weight', F32),
          _dev(running_mean, 'running_mean', F32), _dev(running_var, 'running_var', F32), float(momentum), float(eps), int(bool(frozen)),
          _dev(stats, 'stats', F32))
    return stats


def depth_bn_act_fwd(ys, stats, bn_bias, gate, outs=None):
    """gd4d_depth_bn_act_fwd: out_l = relu((y_l - mu_l) scale_l + bn_bias) * gate[:, :, None, None] for L <= 4 levels."""
    if outs is None:
        outs = [torch.empty_like(y) for y in ys]
    nl, n, c, lv = _depth_levels('depth_bn_act_fwd', ys, outs)
    if tuple(stats.shape) != (nl, 3, c) or tuple(gate.shape) != (n, c):
        raise ValueError(f'depth_bn_act_fwd: stats ({nl}, 3, {c}) and gate ({n}, {c}) expected')
    _call('gd4d_depth_bn_act_fwd', _ptrs(ys, 'ys'), _ptrs(outs, 'outs'), lv, nl, n, c, _dev(stats, 'stats', F32),
          _dev(bn_bias, 'bn_bias', F32), _dev(gate, 'gate', F32))
    return outs


def depth_bn_bwd(douts, ys, stats, bn_bias, gate, frozen=False, outs=None, small=None, workspace=None):
    """gd4d_depth_bn_bwd: the BatchNorm / ReLU / gate backward of L <= 4 levels -> (dy list, dgamma, dbeta, dgate (N, 256), dbias),
    dgamma / dbeta / dgate / dbias summed over the levels of the call.  outs: the L dy maps to write; small: the (3 + N, 256) tensor
    whose rows become dgamma, dbeta, dbias and dgate; workspace: the kernel's scratch floats (defaults: new ones)."""
    lib = _lib.load()
    dys = [torch.empty_like(y) for y in ys] if outs is None else list(outs)
    nl, n, c, lv = _depth_levels('depth_bn_bwd', ys, douts, dys)
    if tuple(stats.shape) != (nl, 3, c) or tuple(gate.shape) != (n, c):
        raise ValueError(f'depth_bn_bwd: stats ({nl}, 3, {c}) and gate ({n}, {c}) expected')
    dev = ys[0].device
    ws = _out(workspace, (max(int(lib.gd4d_depth_bn_bwd_workspace_bytes(nl, n)) // 4, 1),), dev, 'depth_bn_bwd: workspace')
    small = _out(small, (3 + n, c), dev, 'depth_bn_bwd: small')
    dgamma, dbeta, dbias, dgate = small[0], small[1], small[2], small[3:]
    _call('gd4d_depth_bn_bwd', _ptrs(douts, 'douts'), _ptrs(ys, 'ys'), _ptrs(dys, 'dys'), lv, nl, n, c, _dev(stats, 'stats', F32),
          _dev(bn_bias, 'bn_bias', F32), _dev(gate, 'gate', F32), int(bool(frozen)), _dev(ws, 'workspace', F32),
          _dev(dgamma, 'dgamma', F32), _dev(dbeta, 'dbeta', F32), _dev(dgate, 'dgate', F32), _dev(dbias, 'dbias', F32))
    return dys, dgamma, dbeta, dgate, dbias


def depth_conv_wgrad(dys, feats, partitions=None, out=None, workspace=None):
    """gd4d_depth_conv_wgrad: dW (256, 256, 3, 3) = sum over L <= 4 levels, cameras and pixels of dy[oc, p] x[ic, p + tap], one launch
    plus the reduction over `partitions` partial sums (default: one workgroup per compute unit, at most one partition per tile).
    out / workspace: the dW tensor and the partial sums' scratch floats to use (defaults: new ones)."""
    lib = _lib.load()
    nl, n, c, lv = _depth_levels('depth_conv_wgrad', feats, dys)
    dev = feats[0].device
    if partitions is None:
        tiles = int(lib.gd4d_depth_conv_tiles(lv, nl, n))
        partitions = max(1, min(tiles, torch.cuda.get_device_properties(dev).multi_processor_count // 8))
    partitions = int(partitions)
    nbytes = int(lib.gd4d_depth_conv_wgrad_workspace_bytes(partitions))
    if nbytes == 0:
        raise ValueError(f'depth_conv_wgrad: partitions = {partitions}')
    ws = _out(workspace, (nbytes // 4,), dev, 'depth_conv_wgrad: workspace')
    dw = _out(out, (256, 256, 3, 3), dev, 'depth_conv_wgrad: out')
    _call('gd4d_depth_conv_wgrad', _ptrs(dys, 'dys'), _ptrs(feats, 'feats'), lv, nl, n, c, partitions, _dev(ws, 'workspace', F32),
          _dev(dw, 'dw', F32))
    return dw


_GRID_MASK_DTYPES = {F32: _lib.F32, torch.bfloat16: _lib.BF16, torch.float16: _lib.F16}
GRID_MASK_BLOCK_WORDS, GRID_MASK_STATE_WORDS = 8, 4


def _is_cl(t):
    """(N, 256, H, W) stored (N, H, W, 256)."""
    return t.dim() == 4 and t.permute(0, 2, 3, 1).is_contiguous()


def fpn_empty(n, h, w, device, channels_last=False):
    """An (N, 256, H, W) fp32 map for the neck's kernels to write: contiguous NCHW, or the same logical shape stored (N, H, W, 256)."""
    if channels_last:
        return torch.empty(n, h, w, 256, device=device, dtype=F32).permute(0, 3, 1, 2)
    return torch.empty(n, 256, h, w, device=device, dtype=F32)


def _fpn_map(t, name):
    """(device pointer, channels-last flag) of an (N, 256, H, W) fp32 map in either of the two layouts the neck's kernels take."""
    if not t.is_cuda:
        raise _lib.Gd4dError(f'{name} must live on the GPU (no CPU fallback in graph-detr4d_amd)')
    if t.dtype != F32 or t.dim() != 4:
        raise TypeError(f'{name} must be a float32 (N, C, H, W) map, got {t.dtype} {tuple(t.shape)}')
    if t.is_contiguous():
        return ctypes.c_void_p(t.data_ptr()), 0
    if _is_cl(t):
        return ctypes.c_void_p(t.data_ptr()), 1
    raise ValueError(f'{name} must be contiguous NCHW or channels-last')


def _fpn_lateral_image(name, weight, transposed):
    w = weight.reshape(weight.shape[0], -1)
    cout, cin = (int(v) for v in w.shape)
    ok = cout == 256 and (weight.dim() != 4 or tuple(weight.shape[2:]) == (1, 1))
    nbytes = int(_lib.load().gd4d_fpn_lateral_image_mode_bytes(cin, transposed)) if ok else 0
    entry, mode = ('gd4d_fpn_lateral_image_mode', (1,)) if transposed else ('gd4d_fpn_lateral_image', ())
    return _weight_image(entry, nbytes, f'{name}: weight {tuple(weight.shape)}; the kernel takes (256, Cin, 1, 1), Cin a multiple of 32 '
                         'in [32, 2048]', w, cin, cout, *mode)


def fpn_lateral_image(weight):
    """gd4d_fpn_lateral_image: a lateral's 1x1 weight (256, Cin[, 1, 1]) fp32 -> its bf16 hi / lo fragment image for fpn_lateral_fwd
    (Cin a multiple of 32 in [32, 2048]; remake it when the weight changes)."""
    return _fpn_lateral_image('fpn_lateral_image', weight, 0)


def fpn_lateral_fwd(x, image, bias, up=None, out=None, channels_last_out=False):
    """gd4d_fpn_lateral_fwd: x (N, Cin, H, W) fp32 NCHW -> (conv1x1(x) + bias) + nearest-upsampled `up` (the finished coarser lateral
    (N, 256, Hc, Wc), NCHW or channels-last; None: the coarsest level).  out: the (N, 256, H, W) map to write (either layout; default a
    new one, channels-last when channels_last_out)."""
    if x.dim() != 4:
        raise ValueError('fpn_lateral_fwd: x (N, Cin, H, W) expected')
    n, cin, h, w = (int(v) for v in x.shape)
    if out is None:
        out = fpn_empty(n, h, w, x.device, channels_last_out)
    elif tuple(out.shape) != (n, 256, h, w):
        raise ValueError(f'fpn_lateral_fwd: out must be ({n}, 256, {h}, {w})')
    op, out_cl = _fpn_map(out, 'out')
    up_ptr, up_cl, uh, uw = None, 0, 0, 0
    if up is not None:
        if up.dim() != 4 or up.shape[0] != n or up.shape[1] != 256:
            raise ValueError(f'fpn_lateral_fwd: up must be ({n}, 256, Hc, Wc)')
        up_ptr, up_cl = _fpn_map(up, 'up')
        uh, uw = int(up.shape[2]), int(up.shape[3])
    _call('gd4d_fpn_lateral_fwd', _dev(x, 'x', F32), n, cin, h, w, _dev(image, 'image', U8), _dev(bias, 'bias', F32), up_ptr, uh, uw, up_cl,
          op, 256, out_cl)
    return out


def fpn_conv_fwd(feats, images, biases, outs=None, channels_last_out=False):
    """gd4d_fpn_conv_fwd: L <= 4 NCHW levels (N, 256, H_l, W_l) -> conv3x3(x_l; images[l]) + biases[l] (pad 1, stride 1), one launch;
    images[l] = depth_net_image(weight_l), biases[l] (256) or None.  outs: the L maps to write, all NCHW or all channels-last."""
    nl = len(feats)
    if len(images) != nl or len(biases) != nl:
        raise ValueError('fpn_conv_fwd: one image and one bias (or None) per level')
    n = feats[0].shape[0]
    if any(f.dim() != 4 or f.shape[0] != n or f.shape[1] != feats[0].shape[1] for f in feats):
        raise ValueError('fpn_conv_fwd: levels (N, C, H, W) with the same N and C expected')
    if outs is None:
        outs = [fpn_empty(n, int(f.shape[2]), int(f.shape[3]), f.device, channels_last_out) for f in feats]
    elif len(outs) != nl or any(tuple(o.shape) != tuple(f.shape) for o, f in zip(outs, feats)):
        raise ValueError('fpn_conv_fwd: outs must match the levels\' shapes')
    maps = [_fpn_map(o, 'outs') for o in outs]
    # a one-pixel level is stored the same way in both layouts: it goes with whatever the other levels are
    layouts = {cl for o, (_, cl) in zip(outs, maps) if not (o.is_contiguous() and _is_cl(o))}
    if len(layouts) > 1:
        raise ValueError('fpn_conv_fwd: outs must be all NCHW or all channels-last')
    out_cl = layouts.pop() if layouts else 0
    fp = _ptrs(feats, 'feats')
    op = (ctypes.c_void_p * nl)(*[m[0].value for m in maps])
    ip = _ptrs(images, 'images', U8)
    bp = _ptrs(biases, 'biases', optional=True)
    lv = _levels(feats)
    _call('gd4d_fpn_conv_fwd', fp, op, lv, nl, int(n), int(feats[0].shape[1]), ip, bp, out_cl)
    return outs


def fpn_extra_conv_fwd(x, image, bias=None, relu_in=False, out=None, channels_last_out=False):
    """gd4d_fpn_extra_conv_fwd: x (N, 256, H, W) fp32, NCHW or channels-last -> conv3x3 stride 2 pad 1 of x (relu_in: of relu(x)) + bias,
    (N, 256, (H + 1) // 2, (W + 1) // 2); image = depth_net_image(weight)."""
    xp, x_cl = _fpn_map(x, 'x')
    n, c, h, w = (int(v) for v in x.shape)
    ho, wo = (h + 1) // 2, (w + 1) // 2
    if out is None:
        out = fpn_empty(n, ho, wo, x.device, channels_last_out)
    elif tuple(out.shape) != (n, 256, ho, wo):
        raise ValueError(f'fpn_extra_conv_fwd: out must be ({n}, 256, {ho}, {wo})')
    op, out_cl = _fpn_map(out, 'out')
    _call('gd4d_fpn_extra_conv_fwd', xp, n, c, h, w, x_cl, _dev(image, 'image', U8), _opt(bias, 'bias'), int(bool(relu_in)), op, out_cl)
    return out


def fpn_lateral_image_t(weight):
    """gd4d_fpn_lateral_image_mode(transposed = 1): a lateral's (256, Cin[, 1, 1]) weight -> the image of W^T with which fpn_lateral_dgrad
    gives the input gradient (the Cin output channels in blocks of 256, zeros beyond Cin; remake it when the weight changes)."""
    return _fpn_lateral_image('fpn_lateral_image_t', weight, 1)


def _fpn_grad_map(t, name, channels=256):
    if t.dim() != 4 or (channels is not None and t.shape[1] != channels):
        raise ValueError(f'{name} must be an (N, {channels if channels else "C"}, H, W) map, got {tuple(t.shape)}')
    return _dev(t, name, F32)


def fpn_lateral_dgrad(g, image_t, cin, out=None):
    """gd4d_fpn_lateral_dgrad: g (N, 256, H, W) fp32 NCHW, the lateral's gradient -> dx (N, Cin, H, W) = W^T g;
    image_t = fpn_lateral_image_t(weight).  out: the dx tensor to write (default a new one)."""
    lib = _lib.load()
    gp = _fpn_grad_map(g, 'g')
    n, _, h, w = (int(v) for v in g.shape)
    cin = int(cin)
    if int(lib.gd4d_fpn_lateral_image_mode_bytes(cin, 1)) != image_t.numel():
        raise ValueError(f'fpn_lateral_dgrad: image_t of {image_t.numel()} bytes is not the transposed image of a lateral with Cin = {cin}')
    dx = _out(out, (n, cin, h, w), g.device, 'fpn_lateral_dgrad: out')
    _call('gd4d_fpn_lateral_dgrad', gp, n, cin, h, w, _dev(image_t, 'image_t', U8), _dev(dx, 'dx', F32))
    return dx


def fpn_lateral_wgrad(g, x, partitions=None, outs=None, workspace=None):
    """gd4d_fpn_lateral_wgrad: g (N, 256, H, W), x (N, Cin, H, W) fp32 NCHW -> (dW (256, Cin, 1, 1), db (256)): the sums over cameras and
    pixels of g[oc, p] x[ic, p] and of g[oc, p], K split over `partitions` partial sums added in order (default: about two workgroups
    per compute unit, at most one partition per 64-pixel tile).  outs=(dW, db) / workspace: the tensors to write and the partial
    sums' scratch floats (defaults: new ones)."""
    lib = _lib.load()
    gp = _fpn_grad_map(g, 'g')
    xp = _fpn_grad_map(x, 'x', None)
    n, cin, h, w = (int(v) for v in x.shape)
    if tuple(g.shape) != (n, 256, h, w):
        raise ValueError(f'fpn_lateral_wgrad: g {tuple(g.shape)} for x {tuple(x.shape)}')
    if partitions is None:
        tiles = int(lib.gd4d_fpn_lateral_wgrad_tiles(n, h, w))
        chunks = (cin + 63) // 64
        cus = torch.cuda.get_device_properties(g.device).multi_processor_count
        partitions = max(1, min(tiles, (2 * cus + chunks - 1) // chunks))
    partitions = int(partitions)
    nbytes = int(lib.gd4d_fpn_lateral_wgrad_workspace_bytes(cin, partitions))
    if nbytes == 0:
        raise _lib.Gd4dError(f'fpn_lateral_wgrad: Cin = {cin} (a multiple of 32 in [32, 2048]), partitions = {partitions} (1 .. 4096)')
    o_dw, o_db = outs if outs is not None else (None, None)
    ws = _out(workspace, (nbytes // 4,), g.device, 'fpn_lateral_wgrad: workspace')
    dw = _out(o_dw, (256, cin, 1, 1), g.device, 'fpn_lateral_wgrad: dW')
    db = _out(o_db, (256,), g.device, 'fpn_lateral_wgrad: db')
    _call('gd4d_fpn_lateral_wgrad', gp, xp, n, cin, h, w, partitions, _dev(ws, 'workspace', F32), _dev(dw, 'dw', F32), _dev(db, 'db', F32))
    return dw, db


def fpn_topdown_bwd(g_fine, g_coarse):
    """gd4d_fpn_topdown_bwd: g_coarse (N, 256, Hc, Wc) += U^T g_fine (N, 256, H, W), IN PLACE: the adjoint of the forward's nearest
    upsampling add; every coarse pixel adds its children in row-major order.  Returns g_coarse."""
    fp, cp = _fpn_grad_map(g_fine, 'g_fine'), _fpn_grad_map(g_coarse, 'g_coarse')
    n, _, h, w = (int(v) for v in g_fine.shape)
    if g_coarse.shape[0] != n:
        raise ValueError('fpn_topdown_bwd: the two maps must hold the same cameras')
    _call('gd4d_fpn_topdown_bwd', fp, n, 256, h, w, cp, int(g_coarse.shape[2]), int(g_coarse.shape[3]))
    return g_coarse


def fpn_extra_conv_dgrad(dy, image_t, hw, mask=None, add=None, out=None):
    """gd4d_fpn_extra_conv_dgrad: dy (N, 256, (H + 1) // 2, (W + 1) // 2) -> the stride-2 level's input gradient (N, 256, H, W), hw = (H, W);
    image_t = depth_net_image_t(weight).  mask (N, 256, H, W): the result is kept where mask > 0 (the input the forward applied its
    ReLU to); add (N, 256, H, W): added after that (the level's own incoming gradient).  out: the dx tensor to write (default a new
    one)."""
    dp = _fpn_grad_map(dy, 'dy')
    n, h, w = int(dy.shape[0]), int(hw[0]), int(hw[1])
    if tuple(dy.shape[2:]) != ((h + 1) // 2, (w + 1) // 2):
        raise ValueError(f'fpn_extra_conv_dgrad: dy {tuple(dy.shape)} is not the stride-2 output of an ({h}, {w}) map')
    for t, name in ((mask, 'mask'), (add, 'add')):
        if t is not None and tuple(t.shape) != (n, 256, h, w):
            raise ValueError(f'fpn_extra_conv_dgrad: {name} must be ({n}, 256, {h}, {w})')
    dx = _out(out, (n, 256, h, w), dy.device, 'fpn_extra_conv_dgrad: out')
    _call('gd4d_fpn_extra_conv_dgrad', dp, n, 256, h, w, _dev(image_t, 'image_t', U8), _opt(mask, 'mask'), _opt(add, 'add'),
          _dev(dx, 'dx', F32))
    return dx


def fpn_extra_conv_wgrad(dy, x, relu_in=False, outs=None):
    """gd4d_fpn_extra_conv_wgrad: dy (N, 256, (H + 1) // 2, (W + 1) // 2), x (N, 256, H, W) fp32 NCHW -> (dW (256, 256, 3, 3), db (256)) of
    the stride-2 convolution (relu_in: of relu(x)).  outs=(dW, db): the tensors to write (default new ones)."""
    dp, xp = _fpn_grad_map(dy, 'dy'), _fpn_grad_map(x, 'x')
    n, _, h, w = (int(v) for v in x.shape)
    if tuple(dy.shape) != (n, 256, (h + 1) // 2, (w + 1) // 2):
        raise ValueError(f'fpn_extra_conv_wgrad: dy {tuple(dy.shape)} is not the stride-2 output of x {tuple(x.shape)}')
    o_dw, o_db = outs if outs is not None else (None, None)
    dw = _out(o_dw, (256, 256, 3, 3), x.device, 'fpn_extra_conv_wgrad: dW')
    db = _out(o_db, (256,), x.device, 'fpn_extra_conv_wgrad: db')
    _call('gd4d_fpn_extra_conv_wgrad', dp, xp, n, 256, h, w, int(bool(relu_in)), _dev(dw, 'dw', F32), _dev(db, 'db', F32))
    return dw, db


def fpn_bias_grad(g, out=None, workspace=None):
    """gd4d_fpn_bias_grad: g (N, 256, H, W) fp32 NCHW -> db (256), its channel sums in a fixed order.  out / workspace: the db tensor
    and the (N 256) scratch floats to use (defaults: new ones)."""
    gp = _fpn_grad_map(g, 'g')
    n, _, h, w = (int(v) for v in g.shape)
    ws = _out(workspace, (n * 256,), g.device, 'fpn_bias_grad: workspace')
    db = _out(out, (256,), g.device, 'fpn_bias_grad: out')
    _call('gd4d_fpn_bias_grad', gp, n, 256, h, w, _dev(ws, 'workspace', F32), _dev(db, 'db', F32))
    return db


def grid_mask_fwd(x, d=2, l=1, st_h=0, st_w=0, use_h=True, use_w=True, mode=0, offset=None, out=None, out_dtype=None, apply=True,
                  block=None, gen_offset=False):
    """gd4d_grid_mask_fwd: GridMask (models/utils/grid_mask.py:84-123, angle 0) on x (R, C, H, W) fp32 / fp16 / bf16 in one pass.
    out: None (a new tensor of out_dtype, default x's), a tensor, or x itself (in place).  Parameters by value, or `block`: the (8,)
    int32 device tensor {apply, d, l, st_h, st_w, seed_lo, seed_hi, step} the kernel reads at run time (grid_mask_draw fills it).
    offset: (H, W) fp32 device tensor; gen_offset=True: the per-pixel values of gd4d_grid_mask_rng.h from the block's seed and step."""
    if x.dim() != 4:
        raise ValueError(f'grid_mask_fwd: x (R, C, H, W) expected, got {tuple(x.shape)}')
    if x.dtype not in _GRID_MASK_DTYPES:
        raise TypeError(f'grid_mask_fwd: x must be float32, float16 or bfloat16, got {x.dtype}')
    xp = _dev(x, 'x')
    if out is None:
        out = torch.empty(x.shape, device=x.device, dtype=out_dtype or x.dtype)
    if out.shape != x.shape or out.dtype not in _GRID_MASK_DTYPES or (out_dtype is not None and out.dtype != out_dtype):
        raise ValueError(f'grid_mask_fwd: out must have x\'s shape and the dtype asked for, got {tuple(out.shape)} {out.dtype}')
    r, c, h, w = x.shape
    optr = _opt(offset, 'offset')
    if offset is not None and tuple(offset.shape) != (h, w):
        raise ValueError(f'grid_mask_fwd: offset ({h}, {w}) expected, got {tuple(offset.shape)}')
    bptr = None
    if block is not None:
        if block.numel() != GRID_MASK_BLOCK_WORDS:
            raise ValueError('grid_mask_fwd: block is the (8,) int32 parameter block')
        bptr = _dev(block, 'block', I32)
    _call('gd4d_grid_mask_fwd', xp, _dev(out, 'out'), _GRID_MASK_DTYPES[x.dtype], _GRID_MASK_DTYPES[out.dtype], r, c, h, w,
          int(bool(apply)), int(d), int(l), int(st_h), int(st_w), int(bool(use_h)), int(bool(use_w)), int(mode), optr, bptr,
          int(bool(gen_offset)))
    return out


def grid_mask_draw(state, block, h, ratio):
    """gd4d_grid_mask_draw: one step's draws from state (4,) int32 {seed_lo, seed_hi, step, thresh} into block (8,) int32; the step
    counter in `state` advances by one.  On the current stream, capturable."""
    if state.numel() != GRID_MASK_STATE_WORDS or block.numel() != GRID_MASK_BLOCK_WORDS:
        raise ValueError('grid_mask_draw: state (4,) and block (8,) int32 expected')
    _call('gd4d_grid_mask_draw', _dev(state, 'state', I32), _dev(block, 'block', I32), int(h), float(ratio))
    return block


# ---- DCNv2: the modulated deformable 3x3 convolution (gd4d_dcn.hip) ------------------------------------------------------------
DCN_OFFSET_CHANNELS = 27


def dcn_out_hw(h, w, stride):
    """The output size of the 3x3 convolution, pad 1."""
    return (int(h) - 1) // int(stride) + 1, (int(w) - 1) // int(stride) + 1


def _conv3x3_weight_image(name, entry, weight, takes, limits):
    """A (Cout, Cin, 3, 3) weight's image by lib.<entry>(weight, cin, cout, image, stream), sized by lib.<entry>_bytes(cin, cout)."""
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3):
        raise _lib.Gd4dError(f'{name}: weight {tuple(weight.shape)}; {takes} (Cout, Cin, 3, 3)')
    cout, cin = int(weight.shape[0]), int(weight.shape[1])
    nbytes = int(getattr(_lib.load(), entry + '_bytes')(cin, cout))
    return _weight_image(entry, nbytes, f'{name}: weight {tuple(weight.shape)}; {takes} {limits}', weight, cin, cout)


def dcn_weight_image(weight):
    """gd4d_dcn_weight_image: a 3x3 weight (Cout, Cin, 3, 3) fp32 -> its bf16 hi / lo fragment image.  Cin a multiple of 64 in [64, 512];
    Cout a multiple of 64 in [64, 512] (dcn_fwd) or 27 (dcn_offset_conv_fwd).  Remake it when the weight changes."""
    return _conv3x3_weight_image('dcn_weight_image', 'gd4d_dcn_weight_image', weight, 'the kernels take',
                                 'Cin a multiple of 64 in [64, 512] and Cout a multiple of 64 in [64, 512] (or 27, conv_offset)')


def _dcn_x(x, name):
    if x.dim() != 4:
        raise ValueError(f'{name}: x (N, Cin, H, W) expected')
    return (int(v) for v in x.shape)


def dcn_offset_conv_fwd(x, image, bias=None, stride=1, out=None):
    """gd4d_dcn_offset_conv_fwd: x (N, Cin, H, W) fp32 NCHW -> (N, 27, Ho, Wo): conv3x3(x; stride, pad 1) + bias with the sigmoid applied
    to channels 18..26 (18 offsets, 9 modulations); image = dcn_weight_image(conv_offset.weight)."""
    n, cin, h, w = _dcn_x(x, 'dcn_offset_conv_fwd')
    ho, wo = dcn_out_hw(h, w, stride)
    out = _out(out, (n, DCN_OFFSET_CHANNELS, ho, wo), x.device, 'dcn_offset_conv_fwd: out')
    _call('gd4d_dcn_offset_conv_fwd', _dev(x, 'x', F32), n, cin, h, w, int(stride), _dev(image, 'image', U8), _opt(bias, 'bias'),
          _dev(out, 'out', F32))
    return out


def dcn_fwd(x, offmask, image, cout, stride=1, scale=None, shift=None, relu=False, out=None):
    """gd4d_dcn_fwd: x (N, Cin, H, W), offmask (N, 27, Ho, Wo) (offsets, then modulations in [0, 1]) -> (N, cout, Ho, Wo), the modulated
    deformable 3x3 convolution (pad 1) with the weight of image = dcn_weight_image(weight), then * scale + shift per channel (each (cout)
    or None; shift alone is the bias) and ReLU when asked."""
    lib = _lib.load()
    n, cin, h, w = _dcn_x(x, 'dcn_fwd')
    ho, wo = dcn_out_hw(h, w, stride)
    if tuple(offmask.shape) != (n, DCN_OFFSET_CHANNELS, ho, wo):
        raise ValueError(f'dcn_fwd: offmask must be ({n}, {DCN_OFFSET_CHANNELS}, {ho}, {wo}), got {tuple(offmask.shape)}')
    for t, name in ((scale, 'scale'), (shift, 'shift')):
        if t is not None and tuple(t.shape) != (int(cout),):
            raise ValueError(f'dcn_fwd: {name} must be ({int(cout)},)')
    if int(lib.gd4d_dcn_weight_image_bytes(cin, int(cout))) != image.numel() or int(cout) == DCN_OFFSET_CHANNELS:
        raise _lib.Gd4dError(f'dcn_fwd: the image is not dcn_weight_image of a ({int(cout)}, {cin}, 3, 3) weight the kernel takes')
    out = _out(out, (n, int(cout), ho, wo), x.device, 'dcn_fwd: out')
    _call('gd4d_dcn_fwd', _dev(x, 'x', F32), _dev(offmask, 'offmask', F32), n, cin, int(cout), h, w, int(stride), _dev(image, 'image', U8),
          _opt(scale, 'scale'), _opt(shift, 'shift'), int(bool(relu)), _dev(out, 'out', F32))
    return out


# ---- DCNv2, training (gd4d_dcn_train.hip) ---------------------------------------------------------------------------------------
def dcn_weight_image_t(weight):
    """gd4d_dcn_weight_image_t: a 3x3 weight (Cout, Cin, 3, 3) fp32 -> the transposed bf16 hi / lo fragment image dcn_bwd_data reads
    (rows (tap, ci), K = Cout).  Cin and Cout multiples of 64 in [64, 512].  Remake it when the weight changes."""
    return _conv3x3_weight_image('dcn_weight_image_t', 'gd4d_dcn_weight_image_t', weight, 'the kernels take',
                                 'Cin and Cout multiples of 64 in [64, 512]')


def _dcn_bwd_args(name, dout, y, scale, x, offmask, cout, stride):
    n, cin, h, w = _dcn_x(x, name)
    ho, wo = dcn_out_hw(h, w, stride)
    cout = int(cout)
    if tuple(offmask.shape) != (n, DCN_OFFSET_CHANNELS, ho, wo):
        raise ValueError(f'{name}: offmask must be ({n}, {DCN_OFFSET_CHANNELS}, {ho}, {wo}), got {tuple(offmask.shape)}')
    if tuple(dout.shape) != (n, cout, ho, wo) or (y is not None and tuple(y.shape) != (n, cout, ho, wo)):
        raise ValueError(f'{name}: dout (and y) must be ({n}, {cout}, {ho}, {wo})')
    if scale is not None and tuple(scale.shape) != (cout,):
        raise ValueError(f'{name}: scale must be ({cout},)')
    return n, cin, cout, h, w, ho, wo


def dcn_bwd_data(dout, x, offmask, image_t, cout, stride=1, y=None, scale=None, sigmoid_grad=False, dx=None, want_dx=True, doff=None):
    """gd4d_dcn_bwd_data: the input and offset / modulation gradients of dcn_fwd in one pass.  dout (N, cout, Ho, Wo); y: the forward's
    output when it applied its ReLU (the mask y > 0), scale: the folded BatchNorm's, both optional; image_t = dcn_weight_image_t(weight).
    Returns (dx (N, Cin, H, W) or None, doff (N, 27, Ho, Wo)): doff[:18] the offset gradient, doff[18:] the modulation's - times m (1 - m)
    with sigmoid_grad (the gradient of conv_offset's raw output).  dx is ADDED into with float atomics (the one output whose last bits
    depend on the run): a given dx must hold zeros (or what to add to); by default a zeroed one is made.  doff: the tensor to write
    (default a new one)."""
    lib = _lib.load()
    n, cin, cout, h, w, ho, wo = _dcn_bwd_args('dcn_bwd_data', dout, y, scale, x, offmask, cout, stride)
    if int(lib.gd4d_dcn_weight_image_t_bytes(cin, cout)) != image_t.numel() or image_t.numel() == 0:
        raise _lib.Gd4dError(f'dcn_bwd_data: the image is not dcn_weight_image_t of a ({cout}, {cin}, 3, 3) weight the kernel takes')
    if dx is None and want_dx:
        dx = torch.zeros(n, cin, h, w, device=x.device, dtype=F32)
    elif dx is not None and tuple(dx.shape) != (n, cin, h, w):
        raise ValueError(f'dcn_bwd_data: dx must be ({n}, {cin}, {h}, {w})')
    doff = _out(doff, (n, DCN_OFFSET_CHANNELS, ho, wo), x.device, 'dcn_bwd_data: doff')
    _call('gd4d_dcn_bwd_data', _dev(dout, 'dout', F32), _opt(y, 'y'), _opt(scale, 'scale'), _dev(x, 'x', F32),
          _dev(offmask, 'offmask', F32), n, cin, cout, h, w, int(stride), _dev(image_t, 'image_t', U8), int(bool(sigmoid_grad)),
          _opt(dx, 'dx'), _dev(doff, 'doff', F32))
    return dx, doff


def _dcn_partitions(lib, dev, n, cin, h, w, stride, partitions, waves_per_block):
    if dev.type != 'cuda':
        raise _lib.Gd4dError('x must live on the GPU (no CPU fallback in graph-detr4d_amd)')
    if partitions is None:
        tiles = int(lib.gd4d_dcn_wgrad_tiles(n, h, w, int(stride)))
        blocks = 2 * torch.cuda.get_device_properties(dev).multi_processor_count * (4 // waves_per_block)
        partitions = max(1, min(tiles, blocks // (9 * cin // 32), 4096))
    return int(partitions)


def dcn_wgrad(dout, x, offmask, cout, stride=1, y=None, scale=None, partitions=None, outs=None, workspace=None):
    """gd4d_dcn_wgrad: (dW (cout, Cin, 3, 3), dbias (cout)) of dcn_fwd, the modulated samples recomputed as the forward forms them; y /
    scale as dcn_bwd_data.  One launch plus the reduction over `partitions` partial sums (default: about two workgroups per compute
    unit, at most one partition per 64-pixel tile).  outs=(dW, dbias) / workspace: the tensors to write and the partial sums' scratch
    floats (defaults: new ones)."""
    lib = _lib.load()
    n, cin, cout, h, w, ho, wo = _dcn_bwd_args('dcn_wgrad', dout, y, scale, x, offmask, cout, stride)
    partitions = _dcn_partitions(lib, x.device, n, cin, h, w, stride, partitions, 4)
    nbytes = int(lib.gd4d_dcn_wgrad_workspace_bytes(cin, cout, partitions))
    if nbytes == 0:
        raise _lib.Gd4dError(f'dcn_wgrad: Cin = {cin}, Cout = {cout}, partitions = {partitions}: the kernel takes channels that are multiples '
                             'of 64 in [64, 512] and 1..4096 partitions')
    o_dw, o_db = outs if outs is not None else (None, None)
    ws = _out(workspace, (nbytes // 4,), x.device, 'dcn_wgrad: workspace')
    dw = _out(o_dw, (cout, cin, 3, 3), x.device, 'dcn_wgrad: dW')
    db = _out(o_db, (cout,), x.device, 'dcn_wgrad: dbias')
    _call('gd4d_dcn_wgrad', _dev(dout, 'dout', F32), _opt(y, 'y'), _opt(scale, 'scale'), _dev(x, 'x', F32), _dev(offmask, 'offmask', F32),
          n, cin, cout, h, w, int(stride), partitions, _dev(ws, 'workspace', F32), _dev(dw, 'dw', F32), _dev(db, 'dbias', F32))
    return dw, db


def _dcn_doff(name, doff, x, stride):
    n, cin, h, w = _dcn_x(x, name)
    ho, wo = dcn_out_hw(h, w, stride)
    if tuple(doff.shape) != (n, DCN_OFFSET_CHANNELS, ho, wo):
        raise ValueError(f'{name}: doff must be ({n}, {DCN_OFFSET_CHANNELS}, {ho}, {wo}), got {tuple(doff.shape)}')
    return n, cin, h, w


def dcn_offset_conv_dgrad(doff, weight, dx, stride=1):
    """gd4d_dcn_offset_conv_dgrad: dx (N, Cin, H, W) += conv_transpose3x3(doff (N, 27, Ho, Wo), weight (27, Cin, 3, 3); stride, pad 1), in
    place: a plain read-modify-write (run it after dcn_bwd_data on the same stream).  Returns dx."""
    n, cin, h, w = _dcn_doff('dcn_offset_conv_dgrad', doff, dx, stride)
    if tuple(weight.shape) != (DCN_OFFSET_CHANNELS, cin, 3, 3):
        raise ValueError(f'dcn_offset_conv_dgrad: weight must be ({DCN_OFFSET_CHANNELS}, {cin}, 3, 3)')
    _call('gd4d_dcn_offset_conv_dgrad', _dev(doff, 'doff', F32), _dev(weight, 'weight', F32), n, cin, h, w, int(stride),
          _dev(dx, 'dx', F32))
    return dx


def dcn_offset_conv_wgrad(doff, x, stride=1, partitions=None, outs=None, workspace=None):
    """gd4d_dcn_offset_conv_wgrad: (dW (27, Cin, 3, 3), db (27)) of conv_offset from doff (N, 27, Ho, Wo) and its input x; `partitions` as
    dcn_wgrad, and so are outs=(dW, db) / workspace."""
    lib = _lib.load()
    n, cin, h, w = _dcn_doff('dcn_offset_conv_wgrad', doff, x, stride)
    partitions = _dcn_partitions(lib, x.device, n, cin, h, w, stride, partitions, 1)
    nbytes = int(lib.gd4d_dcn_offset_conv_wgrad_workspace_bytes(cin, partitions))
    if nbytes == 0:
        raise _lib.Gd4dError(f'dcn_offset_conv_wgrad: Cin = {cin}, partitions = {partitions}: the kernel takes Cin a multiple of 64 in '
                             '[64, 512] and 1..4096 partitions')
    o_dw, o_db = outs if outs is not None else (None, None)
    ws = _out(workspace, (nbytes // 4,), x.device, 'dcn_offset_conv_wgrad: workspace')
    dw = _out(o_dw, (DCN_OFFSET_CHANNELS, cin, 3, 3), x.device, 'dcn_offset_conv_wgrad: dW')
    db = _out(o_db, (DCN_OFFSET_CHANNELS,), x.device, 'dcn_offset_conv_wgrad: db')
    _call('gd4d_dcn_offset_conv_wgrad', _dev(doff, 'doff', F32), _dev(x, 'x', F32), n, cin, h, w, int(stride), partitions,
          _dev(ws, 'workspace', F32), _dev(dw, 'dw', F32), _dev(db, 'db', F32))
    return dw, db


# ---- VoVNet: 3x3 conv + frozen BN + ReLU, the OSA aggregation, eSE (gd4d_vovnet.hip) -------------------------------------------
OSA_MAX_SOURCES = 6


def conv3x3_image(weight):
    """gd4d_conv3x3_image: a 3x3 weight (Cout, Cin, 3, 3) fp32 -> its bf16 hi / lo fragment image.  Cin a multiple of 32 in [32, 1024],
    Cout a multiple of 32 in [32, 256].  Remake it when the weight changes."""
    return _conv3x3_weight_image('conv3x3_image', 'gd4d_conv3x3_image', weight, 'the kernel takes',
                                 'Cin a multiple of 32 in [32, 1024] and Cout a multiple of 32 in [32, 256]')


def conv3x3_bn_relu(x, image, cout, scale, shift, stride=1, out=None, m_blocks=0):
    """gd4d_conv3x3_bn_relu_fwd: x (N, Cin, H, W) fp32 NCHW -> relu(conv3x3(x; stride, pad 1) * scale + shift), (N, cout, Ho, Wo); image =
    conv3x3_image(weight), scale / shift (cout) the folded frozen BatchNorm.  m_blocks: 0, or the M tiling to force (1, 2, 3, 4, 5 or 7
    row blocks of 32 channels per workgroup, dividing cout / 32; the same bits either way)."""
    lib = _lib.load()
    n, cin, h, w = _dcn_x(x, 'conv3x3_bn_relu')
    cout = int(cout)
    ho, wo = dcn_out_hw(h, w, stride)
    for t, name in ((scale, 'scale'), (shift, 'shift')):
        if tuple(t.shape) != (cout,):
            raise ValueError(f'conv3x3_bn_relu: {name} must be ({cout},)')
    nbytes = int(lib.gd4d_conv3x3_image_bytes(cin, cout))
    if nbytes == 0 or nbytes != image.numel():
        raise _lib.Gd4dError(f'conv3x3_bn_relu: the image is not conv3x3_image of a ({cout}, {cin}, 3, 3) weight the kernel takes '
                             '(Cin a multiple of 32 in [32, 1024], Cout a multiple of 32 in [32, 256])')
    out = _out(out, (n, cout, ho, wo), x.device, 'conv3x3_bn_relu: out')
    _call('gd4d_conv3x3_bn_relu_fwd', _dev(x, 'x', F32), n, cin, h, w, int(stride), _dev(image, 'image', U8), cout,
          _dev(scale, 'scale', F32), _dev(shift, 'shift', F32), _dev(out, 'out', F32), int(m_blocks))
    return out


def osa_concat_image(weight):
    """gd4d_osa_concat_image: the aggregation's weight (Cout, K) or (Cout, K, 1, 1) fp32 -> its fragment image.  K a multiple of 32 in
    [32, 2304], Cout a multiple of 32 in [32, 1024]."""
    if weight.dim() == 4 and tuple(weight.shape[2:]) == (1, 1):
        weight = weight.reshape(weight.shape[0], weight.shape[1])
    if weight.dim() != 2:
        raise _lib.Gd4dError(f'osa_concat_image: weight {tuple(weight.shape)}; the kernel takes (Cout, K) or (Cout, K, 1, 1)')
    cout, k = int(weight.shape[0]), int(weight.shape[1])
    return _weight_image('gd4d_osa_concat_image', int(_lib.load().gd4d_osa_concat_image_bytes(k, cout)),
                         f'osa_concat_image: weight {tuple(weight.shape)}; the kernel takes K a multiple of 32 in [32, 2304] and Cout '
                         'a multiple of 32 in [32, 1024]', weight, k, cout)


def osa_concat_conv(sources, image, cout, scale, shift, out=None, partials=None, m_blocks=0):
    """gd4d_osa_concat_conv_fwd: relu((W . concat(sources)) * scale + shift) for 1..6 separate NCHW fp32 maps of the same (N, H, W), each
    with a multiple of 32 channels; the concatenation is never written.  Returns (out (N, cout, H, W), partials (N, tiles, cout)): each
    128-pixel tile's per-channel sum of the outputs, what ese_gate averages.  m_blocks: as conv3x3_bn_relu's."""
    lib = _lib.load()
    sources = list(sources)
    if not 1 <= len(sources) <= OSA_MAX_SOURCES:
        raise _lib.Gd4dError(f'osa_concat_conv: {len(sources)} sources; the kernel takes 1 to {OSA_MAX_SOURCES}')
    n, _, h, w = _dcn_x(sources[0], 'osa_concat_conv')
    for s in sources:
        if s.dim() != 4 or (int(s.shape[0]), int(s.shape[2]), int(s.shape[3])) != (n, h, w):
            raise ValueError(f'osa_concat_conv: every source must be ({n}, C_i, {h}, {w}), got {tuple(s.shape)}')
    chans = [int(s.shape[1]) for s in sources]
    cout = int(cout)
    for t, name in ((scale, 'scale'), (shift, 'shift')):
        if tuple(t.shape) != (cout,):
            raise ValueError(f'osa_concat_conv: {name} must be ({cout},)')
    nbytes = int(lib.gd4d_osa_concat_image_bytes(sum(chans), cout))
    if nbytes == 0 or nbytes != image.numel() or any(c % 32 for c in chans):
        raise _lib.Gd4dError(f'osa_concat_conv: sources of {chans} channels -> {cout}: the kernel takes multiples of 32, K up to 2304 and '
                             'Cout up to 1024, with image = osa_concat_image of the (Cout, K) weight')
    tiles = int(lib.gd4d_osa_concat_tiles(h, w))
    out = _out(out, (n, cout, h, w), sources[0].device, 'osa_concat_conv: out')
    partials = _out(partials, (n, tiles, cout), sources[0].device, 'osa_concat_conv: partials')
    ptrs = _ptrs(sources, 'sources')
    ch = (ctypes.c_int32 * len(sources))(*chans)
    _call('gd4d_osa_concat_conv_fwd', ptrs, ch, len(sources), n, h, w, _dev(image, 'image', U8), cout, _dev(scale, 'scale', F32),
          _dev(shift, 'shift', F32), _dev(out, 'out', F32), _dev(partials, 'partials', F32), int(m_blocks))
    return out, partials


def ese_gate(partials, hw, fc_weight, fc_bias, out=None):
    """gd4d_ese_gate_fwd: partials (N, tiles, C) of osa_concat_conv, hw = H W -> gate (N, C) = relu6(fc_weight mean + fc_bias + 3) / 6;
    fc_weight (C, C) or (C, C, 1, 1), C a multiple of 32 up to 1024."""
    if partials.dim() != 3:
        raise ValueError('ese_gate: partials (N, tiles, C) expected')
    n, tiles, c = (int(v) for v in partials.shape)
    if fc_weight.numel() != c * c or tuple(fc_weight.shape[:2]) != (c, c) or tuple(fc_bias.shape) != (c,):
        raise ValueError(f'ese_gate: fc_weight ({c}, {c}[, 1, 1]) and fc_bias ({c},) expected')
    if c % 32 or not 32 <= c <= 1024:
        raise _lib.Gd4dError(f'ese_gate: C = {c}; the kernel takes a multiple of 32 in [32, 1024]')
    out = _out(out, (n, c), partials.device, 'ese_gate: out')
    _call('gd4d_ese_gate_fwd', _dev(partials, 'partials', F32), n, tiles, c, int(hw), _dev(fc_weight, 'fc_weight', F32),
          _dev(fc_bias, 'fc_bias', F32), _dev(out, 'out', F32))
    return out


def ese_apply(xt, gate, identity=None, out=None):
    """gd4d_ese_apply_fwd: xt (N, C, H, W) * gate (N, C) (+ identity, xt's shape) -> out (a new tensor, or the one given: xt itself is
    allowed)."""
    n, c, h, w = _dcn_x(xt, 'ese_apply')
    if tuple(gate.shape) != (n, c):
        raise ValueError(f'ese_apply: gate must be ({n}, {c})')
    if identity is not None and identity.shape != xt.shape:
        raise ValueError(f'ese_apply: identity must have xt\'s shape {tuple(xt.shape)}, got {tuple(identity.shape)}')
    if out is None:
        out = torch.empty_like(xt)
    elif out.shape != xt.shape:
        raise ValueError(f'ese_apply: out must have xt\'s shape {tuple(xt.shape)}')
    _call('gd4d_ese_apply_fwd', _dev(xt, 'xt', F32), _dev(gate, 'gate', F32), _opt(identity, 'identity'), n, c, h * w,
          _dev(out, 'out', F32))
    return out


# ---- ResNet: the blocks' plain convolutions + frozen BN (+ identity) (+ ReLU) (gd4d_resnet.hip) ---------------------------------
_CONV1X1_LIMITS = 'K a multiple of 32 in [32, 2304] and Cout a multiple of 32 in [32, 2048]'
_CONV3X3_ACT_LIMITS = 'Cin a multiple of 32 in [32, 1024] and Cout a multiple of 32 in [32, 512]'


def conv1x1_image(weight):
    """gd4d_conv1x1_image: a 1x1 convolution's weight (Cout, K) or (Cout, K, 1, 1) fp32 -> its bf16 hi / lo fragment image.  K a multiple
    of 32 in [32, 2304], Cout a multiple of 32 in [32, 2048].  Remake it when the weight changes."""
    if weight.dim() == 4 and tuple(weight.shape[2:]) == (1, 1):
        weight = weight.reshape(weight.shape[0], weight.shape[1])
    if weight.dim() != 2:
        raise _lib.Gd4dError(f'conv1x1_image: weight {tuple(weight.shape)}; the kernel takes (Cout, K) or (Cout, K, 1, 1)')
    cout, k = int(weight.shape[0]), int(weight.shape[1])
    return _weight_image('gd4d_conv1x1_image', int(_lib.load().gd4d_conv1x1_image_bytes(k, cout)),
                         f'conv1x1_image: weight {tuple(weight.shape)}; the kernel takes {_CONV1X1_LIMITS}', weight, k, cout)


def conv3x3_act_image(weight):
    """gd4d_conv3x3_act_image: conv3x3_image for conv3x3_bn_act, whose Cout reaches 512: Cin a multiple of 32 in [32, 1024], Cout a
    multiple of 32 in [32, 512]; the same bytes as conv3x3_image where both take the weight."""
    return _conv3x3_weight_image('conv3x3_act_image', 'gd4d_conv3x3_act_image', weight, 'the kernel takes', _CONV3X3_ACT_LIMITS)


def _conv_bn_act(name, taps, x, image, cout, scale, shift, stride, identity, relu, out, m_blocks):
    lib = _lib.load()
    n, cin, h, w = _dcn_x(x, name)
    cout = int(cout)
    ho, wo = dcn_out_hw(h, w, stride)
    for t, what in ((scale, 'scale'), (shift, 'shift')):
        if tuple(t.shape) != (cout,):
            raise ValueError(f'{name}: {what} must be ({cout},)')
    if identity is not None and tuple(identity.shape) != (n, cout, ho, wo):
        raise ValueError(f'{name}: identity must be ({n}, {cout}, {ho}, {wo}), got {tuple(identity.shape)}')
    nbytes = int((lib.gd4d_conv3x3_act_image_bytes if taps == 9 else lib.gd4d_conv1x1_image_bytes)(cin, cout))
    if nbytes == 0 or nbytes != image.numel():
        made, shape, limits = ('conv3x3_act_image', f'({cout}, {cin}, 3, 3)', _CONV3X3_ACT_LIMITS) if taps == 9 else \
            ('conv1x1_image', f'({cout}, {cin})', _CONV1X1_LIMITS)
        raise _lib.Gd4dError(f'{name}: the image is not {made} of a {shape} weight the kernel takes ({limits})')
    out = _out(out, (n, cout, ho, wo), x.device, f'{name}: out')
    _call(f'gd4d_{name}_fwd', _dev(x, 'x', F32), n, cin, h, w, int(stride), _dev(image, 'image', U8), cout, _dev(scale, 'scale', F32),
          _dev(shift, 'shift', F32), _opt(identity, 'identity'), int(bool(relu)), _dev(out, 'out', F32), int(m_blocks))
    return out


def conv1x1_bn_act(x, image, cout, scale, shift, stride=1, identity=None, relu=True, out=None, m_blocks=0):
    """gd4d_conv1x1_bn_act_fwd: x (N, Cin, H, W) fp32 NCHW -> act(conv1x1(x; stride 1 or 2) * scale + shift (+ identity)), (N, cout, Ho,
    Wo); image = conv1x1_image(weight), scale / shift (cout) the folded frozen BatchNorm, identity an optional map of the result's shape
    (added before the ReLU), act the ReLU unless relu=False (a downsample branch).  m_blocks: as conv3x3_bn_relu's."""
    return _conv_bn_act('conv1x1_bn_act', 1, x, image, cout, scale, shift, stride, identity, relu, out, m_blocks)


def conv3x3_bn_act(x, image, cout, scale, shift, stride=1, identity=None, relu=True, out=None, m_blocks=0):
    """gd4d_conv3x3_bn_act_fwd: conv1x1_bn_act's counterpart for the 3x3 (pad 1); image = conv3x3_act_image(weight) (or conv3x3_image's:
    the same bytes).  With identity=None and relu=True it gives conv3x3_bn_relu's bits."""
    return _conv_bn_act('conv3x3_bn_act', 9, x, image, cout, scale, shift, stride, identity, relu, out, m_blocks)


# ---- VoVNet, training behind frozen BatchNorms (gd4d_vovnet_train.hip) ----------------------------------------------------------
def conv3x3_image_t(weight, scale=None):
    """gd4d_conv3x3_image_t: the image conv3x3_dgrad reads, of the (Cout, Cin, 3, 3) fp32 weight times scale[co] (the folded BatchNorm's;
    None: the weight as it is) - transposed, taps flipped.  Limits as conv3x3_image.  Remake it when the weight or the scale changes."""
    if scale is not None:
        weight = weight * scale.view(-1, 1, 1, 1)
    return _conv3x3_weight_image('conv3x3_image_t', 'gd4d_conv3x3_image_t', weight, 'the kernel takes',
                                 'Cin a multiple of 32 in [32, 1024] and Cout a multiple of 32 in [32, 256]')


def osa_concat_image_t(weight, scale=None):
    """gd4d_osa_concat_image_t: the image osa_concat_dgrad reads, of the aggregation's (Cout, K[, 1, 1]) weight times scale[co],
    transposed.  Limits as osa_concat_image."""
    if weight.dim() == 4 and tuple(weight.shape[2:]) == (1, 1):
        weight = weight.reshape(weight.shape[0], weight.shape[1])
    if weight.dim() != 2:
        raise _lib.Gd4dError(f'osa_concat_image_t: weight {tuple(weight.shape)}; the kernel takes (Cout, K) or (Cout, K, 1, 1)')
    cout, k = int(weight.shape[0]), int(weight.shape[1])
    if scale is not None:
        weight = weight * scale.view(-1, 1)
    return _weight_image('gd4d_osa_concat_image_t', int(_lib.load().gd4d_osa_concat_image_t_bytes(k, cout)),
                         f'osa_concat_image_t: weight {tuple(weight.shape)}; the kernel takes K a multiple of 32 in [32, 2304] and Cout '
                         'a multiple of 32 in [32, 1024]', weight, k, cout)


def conv3x3_dgrad(dz, image_t, cin, add=None, mask=None, add2=None, out=None, m_blocks=0):
    """gd4d_conv3x3_dgrad: dz (N, Cout, H, W) fp32 -> (conv3x3^T(dz) (+ add)) ([mask > 0]) (+ add2), (N, cin, H, W): the stride-1
    convolution's input gradient with image_t = conv3x3_image_t(weight, scale); add / mask / add2 optional maps of the result's shape
    (out may be add or add2).  m_blocks: as conv3x3_bn_relu's, dividing cin / 32; the same bits either way."""
    lib = _lib.load()
    n, cout, h, w = _dcn_x(dz, 'conv3x3_dgrad')
    cin = int(cin)
    nbytes = int(lib.gd4d_conv3x3_image_t_bytes(cin, cout))
    if nbytes == 0 or nbytes != image_t.numel():
        raise _lib.Gd4dError(f'conv3x3_dgrad: the image is not conv3x3_image_t of a ({cout}, {cin}, 3, 3) weight the kernel takes '
                             '(Cin a multiple of 32 in [32, 1024], Cout a multiple of 32 in [32, 256])')
    for t, name in ((add, 'add'), (mask, 'mask'), (add2, 'add2')):
        if t is not None and tuple(t.shape) != (n, cin, h, w):
            raise ValueError(f'conv3x3_dgrad: {name} must be ({n}, {cin}, {h}, {w})')
    out = _out(out, (n, cin, h, w), dz.device, 'conv3x3_dgrad: out')
    _call('gd4d_conv3x3_dgrad', _dev(dz, 'dz', F32), n, cin, cout, h, w, _dev(image_t, 'image_t', U8), _opt(add, 'add'), _opt(mask, 'mask'),
          _opt(add2, 'add2'), _dev(out, 'out', F32), int(m_blocks))
    return out


def osa_concat_dgrad(dz, image_t, channels, mask_last=None, outs=None, m_blocks=0):
    """gd4d_osa_concat_dgrad: dz (N, Cout, H, W) fp32 -> one map (N, channels[i], H, W) per source of the aggregation, the rows of source
    i of W^T dz with image_t = osa_concat_image_t(weight, scale); the concatenation's gradient is never written.  mask_last: the last
    map is zeroed where mask_last <= 0.  A forced m_blocks must divide every channels[i] / 32."""
    lib = _lib.load()
    n, cout, h, w = _dcn_x(dz, 'osa_concat_dgrad')
    chans = [int(c) for c in channels]
    if not 1 <= len(chans) <= OSA_MAX_SOURCES:
        raise _lib.Gd4dError(f'osa_concat_dgrad: {len(chans)} destinations; the kernel takes 1 to {OSA_MAX_SOURCES}')
    nbytes = int(lib.gd4d_osa_concat_image_t_bytes(sum(chans), cout))
    if nbytes == 0 or nbytes != image_t.numel() or any(c % 32 or c <= 0 for c in chans):
        raise _lib.Gd4dError(f'osa_concat_dgrad: {cout} -> maps of {chans} channels: the kernel takes multiples of 32, K up to 2304 and '
                             'Cout up to 1024, with image_t = osa_concat_image_t of the (Cout, K) weight')
    if mask_last is not None and tuple(mask_last.shape) != (n, chans[-1], h, w):
        raise ValueError(f'osa_concat_dgrad: mask_last must be ({n}, {chans[-1]}, {h}, {w})')
    if outs is None:
        outs = [torch.empty(n, c, h, w, device=dz.device, dtype=F32) for c in chans]
    elif [tuple(o.shape) for o in outs] != [(n, c, h, w) for c in chans]:
        raise ValueError('osa_concat_dgrad: outs must be one (N, channels[i], H, W) map per destination')
    _call('gd4d_osa_concat_dgrad', _dev(dz, 'dz', F32), n, cout, h, w, _dev(image_t, 'image_t', U8), _ptrs(outs, 'outs'),
          (ctypes.c_int32 * len(chans))(*chans), len(chans), _opt(mask_last, 'mask_last'), int(m_blocks))
    return list(outs)


def _vv_partitions(dev, tiles, chunks, partitions):
    """About two workgroups per compute unit, at most one partition per tile."""
    if dev.type != 'cuda':
        raise _lib.Gd4dError('the maps must live on the GPU (no CPU fallback in graph-detr4d_amd)')
    if partitions is None:
        partitions = max(1, min(tiles, 2 * torch.cuda.get_device_properties(dev).multi_processor_count // max(1, chunks), 4096))
    return int(partitions)


def _vv_wgrad_outputs(name, lib, weight, bn, cin, cout, taps, partitions, want, outs=None, workspace=None):
    if tuple(bn.shape) != (3, cout):
        raise ValueError(f'{name}: bn must be (3, {cout}): scale, rstd, mean')
    if weight.numel() != cout * cin * taps or int(weight.shape[0]) != cout:
        raise ValueError(f'{name}: weight of {cout} x {cin} x {taps} values expected, got {tuple(weight.shape)}')
    if not any(want):
        raise ValueError(f'{name}: nothing asked for')
    nbytes = int(lib.gd4d_conv_wgrad_workspace_bytes(cin, cout, taps, partitions))
    if nbytes == 0:
        raise _lib.Gd4dError(f'{name}: {cin} -> {cout} channels, partitions = {partitions}: the kernel takes multiples of 32 within the '
                             'forward\'s limits and 1..4096 partitions')
    dev = weight.device
    o_dw, o_dgamma, o_dbeta = outs if outs is not None else (None, None, None)
    ws = _out(workspace, (nbytes // 4,), dev, f'{name}: workspace')
    dw = _out(o_dw, weight.shape, dev, f'{name}: dW') if want[0] else None
    dgamma = _out(o_dgamma, (cout,), dev, f'{name}: dgamma') if want[1] else None
    dbeta = _out(o_dbeta, (cout,), dev, f'{name}: dbeta') if want[2] else None
    return ws, dw, dgamma, dbeta


def conv3x3_wgrad(dz, x, weight, bn, want=(True, True, True), partitions=None, outs=None, workspace=None):
    """gd4d_conv3x3_wgrad: the parameter gradients of relu(BN(conv3x3(x))) behind a frozen BatchNorm from dz (N, Cout, H, W), the
    gradient of the BatchNorm's output after the ReLU mask, and the convolution's input x (N, Cin, H, W): (dW (Cout, Cin, 3, 3), dgamma,
    dbeta), None where `want` says so.  weight: the unscaled fp32 weight; bn (3, Cout): scale = gamma rstd, rstd, mean.
    outs=(dW, dgamma, dbeta) / workspace: the tensors to write and the partial sums' scratch floats (defaults: new ones)."""
    lib = _lib.load()
    n, cout, h, w = _dcn_x(dz, 'conv3x3_wgrad')
    if x.dim() != 4 or (int(x.shape[0]), int(x.shape[2]), int(x.shape[3])) != (n, h, w):
        raise ValueError(f'conv3x3_wgrad: x {tuple(x.shape)} for dz {tuple(dz.shape)}')
    cin = int(x.shape[1])
    partitions = _vv_partitions(dz.device, int(lib.gd4d_conv3x3_wgrad_tiles(n, h, w)), cin // 32, partitions)
    ws, dw, dgamma, dbeta = _vv_wgrad_outputs('conv3x3_wgrad', lib, weight, bn, cin, cout, 9, partitions, want, outs, workspace)
    _call('gd4d_conv3x3_wgrad', _dev(dz, 'dz', F32), _dev(x, 'x', F32), n, cin, cout, h, w, partitions, _dev(ws, 'workspace', F32),
          _dev(weight, 'weight', F32), _dev(bn, 'bn', F32), _opt(dw, 'dw'), _opt(dgamma, 'dgamma'), _opt(dbeta, 'dbeta'))
    return dw, dgamma, dbeta


def osa_concat_wgrad(dz, dz_sums, sources, weight, bn, want=(True, True, True), partitions=None, outs=None, workspace=None):
    """gd4d_osa_concat_wgrad: conv3x3_wgrad's counterpart for the aggregation: sources are the L + 1 maps where they lie, dz_sums
    (N, Cout) dz's plane sums (ese_bwd's second result), weight (Cout, K[, 1, 1]).  Returns (dW of weight's shape, dgamma, dbeta);
    outs / workspace as conv3x3_wgrad's."""
    lib = _lib.load()
    n, cout, h, w = _dcn_x(dz, 'osa_concat_wgrad')
    sources = list(sources)
    if not 1 <= len(sources) <= OSA_MAX_SOURCES:
        raise _lib.Gd4dError(f'osa_concat_wgrad: {len(sources)} sources; the kernel takes 1 to {OSA_MAX_SOURCES}')
    for s in sources:
        if s.dim() != 4 or (int(s.shape[0]), int(s.shape[2]), int(s.shape[3])) != (n, h, w):
            raise ValueError(f'osa_concat_wgrad: every source must be ({n}, C_i, {h}, {w}), got {tuple(s.shape)}')
    if tuple(dz_sums.shape) != (n, cout):
        raise ValueError(f'osa_concat_wgrad: dz_sums must be ({n}, {cout})')
    chans = [int(s.shape[1]) for s in sources]
    k = sum(chans)
    if any(c % 32 for c in chans):
        raise _lib.Gd4dError(f'osa_concat_wgrad: sources of {chans} channels; the kernel takes multiples of 32')
    partitions = _vv_partitions(dz.device, int(lib.gd4d_osa_concat_wgrad_tiles(n, h, w)), ((k + 63) // 64) * ((cout + 255) // 256), partitions)
    ws, dw, dgamma, dbeta = _vv_wgrad_outputs('osa_concat_wgrad', lib, weight, bn, k, cout, 1, partitions, want, outs, workspace)
    _call('gd4d_osa_concat_wgrad', _dev(dz, 'dz', F32), _dev(dz_sums, 'dz_sums', F32), _ptrs(sources, 'sources'),
          (ctypes.c_int32 * len(chans))(*chans), len(chans), n, h, w, cout, partitions, _dev(ws, 'workspace', F32),
          _dev(weight, 'weight', F32), _dev(bn, 'bn', F32), _opt(dw, 'dw'), _opt(dgamma, 'dgamma'), _opt(dbeta, 'dbeta'))
    return dw, dgamma, dbeta


def ese_bwd(dout, xt, partials, gate, fc_weight, want_fc=(True, True), outs=None, workspace=None):
    """gd4d_ese_bwd: the backward of out = xt * gate (+ identity) with gate = ese_gate(partials, ...), up to the aggregation's BatchNorm
    output: returns (dz (N, C, H, W) = (dout gate + fc_w^T dv / HW) [xt > 0], its plane sums (N, C), dfc_w, dfc_b), where dv =
    (sum_hw dout xt) / 6 for 0 < gate < 1 and 0 at and beyond the clamp's corners; dfc_w / dfc_b are None where want_fc says so.
    outs=(dz, sums, dfc_w, dfc_b) / workspace: the tensors to write and the scratch floats (defaults: new ones)."""
    lib = _lib.load()
    n, c, h, w = _dcn_x(xt, 'ese_bwd')
    if dout.shape != xt.shape or tuple(gate.shape) != (n, c) or partials.dim() != 3 or (int(partials.shape[0]), int(partials.shape[2])) != (n, c):
        raise ValueError(f'ese_bwd: dout of xt\'s shape {tuple(xt.shape)}, gate ({n}, {c}) and partials ({n}, tiles, {c}) expected')
    if fc_weight.numel() != c * c or tuple(fc_weight.shape[:2]) != (c, c):
        raise ValueError(f'ese_bwd: fc_weight ({c}, {c}[, 1, 1]) expected')
    nbytes = int(lib.gd4d_ese_bwd_workspace_bytes(n, c))
    if nbytes == 0:
        raise _lib.Gd4dError(f'ese_bwd: C = {c}; the kernel takes a multiple of 32 in [32, 1024]')
    dev = xt.device
    o_dz, o_sums, o_w, o_b = outs if outs is not None else (None, None, None, None)
    ws = _out(workspace, (nbytes // 4,), dev, 'ese_bwd: workspace')
    dz, sums = _out(o_dz, xt.shape, dev, 'ese_bwd: dz'), _out(o_sums, (n, c), dev, 'ese_bwd: sums')
    dfc_w = _out(o_w, fc_weight.shape, dev, 'ese_bwd: dfc_w') if want_fc[0] else None
    dfc_b = _out(o_b, (c,), dev, 'ese_bwd: dfc_b') if want_fc[1] else None
    _call('gd4d_ese_bwd', _dev(dout, 'dout', F32), _dev(xt, 'xt', F32), _dev(partials, 'partials', F32), int(partials.shape[1]),
          _dev(gate, 'gate', F32), _dev(fc_weight, 'fc_weight', F32), n, c, h * w, _dev(ws, 'workspace', F32), _dev(dz, 'dz', F32),
          _dev(sums, 'dz_sums', F32), _opt(dfc_w, 'dfc_w'), _opt(dfc_b, 'dfc_b'))
    return dz, sums, dfc_w, dfc_b


# ---- ResNet, training behind frozen BatchNorms (gd4d_resnet_train.hip) ----------------------------------------------------------
_CONV1X1_T_LIMITS = 'Cin and Cout multiples of 32 in [32, 2048]'


def conv1x1_image_t(weight, scale=None):
    """gd4d_conv1x1_image_t: the image conv1x1_dgrad reads, of the (Cout, Cin[, 1, 1]) fp32 weight times scale[co] (the folded
    BatchNorm's; None: the weight as it is), transposed.  Cin and Cout multiples of 32 in [32, 2048]."""
    if weight.dim() == 4 and tuple(weight.shape[2:]) == (1, 1):
        weight = weight.reshape(weight.shape[0], weight.shape[1])
    if weight.dim() != 2:
        raise _lib.Gd4dError(f'conv1x1_image_t: weight {tuple(weight.shape)}; the kernel takes (Cout, Cin) or (Cout, Cin, 1, 1)')
    cout, cin = int(weight.shape[0]), int(weight.shape[1])
    if scale is not None:
        weight = weight * scale.view(-1, 1)
    return _weight_image('gd4d_conv1x1_image_t', int(_lib.load().gd4d_conv1x1_image_t_bytes(cin, cout)),
                         f'conv1x1_image_t: weight {tuple(weight.shape)}; the kernel takes {_CONV1X1_T_LIMITS}', weight, cin, cout)


def conv3x3_act_image_t(weight, scale=None):
    """gd4d_conv3x3_act_image_t: conv3x3_image_t for conv3x3_act_dgrad, whose Cout reaches 512 (limits as conv3x3_act_image)."""
    if scale is not None:
        weight = weight * scale.view(-1, 1, 1, 1)
    return _conv3x3_weight_image('conv3x3_act_image_t', 'gd4d_conv3x3_act_image_t', weight, 'the kernel takes', _CONV3X3_ACT_LIMITS)


def relu_mask_bwd(dout, out_map, out=None):
    """gd4d_relu_mask_bwd: dout where out_map > 0, else 0 (a ReLU's backward on its stored output); `out` may be dout."""
    if dout.shape != out_map.shape:
        raise ValueError(f'relu_mask_bwd: dout {tuple(dout.shape)} and the map {tuple(out_map.shape)} must have one shape')
    g = _out(out, dout.shape, dout.device, 'relu_mask_bwd: out')
    _call('gd4d_relu_mask_bwd', _dev(dout, 'dout', F32), _dev(out_map, 'out_map', F32), dout.numel(), _dev(g, 'out', F32))
    return g


def even_pixels_scatter(src, hw, out=None):
    """gd4d_even_pixels_scatter: src (N, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1) -> (N, C, H, W) with src[y / 2, x / 2] at the even
    (y, x) and zeros elsewhere: the adjoint of x[:, :, ::2, ::2]."""
    n, c, hs, ws = _dcn_x(src, 'even_pixels_scatter')
    h, w = int(hw[0]), int(hw[1])
    if dcn_out_hw(h, w, 2) != (hs, ws):
        raise ValueError(f'even_pixels_scatter: src {tuple(src.shape)} is not half of ({h}, {w})')
    out = _out(out, (n, c, h, w), src.device, 'even_pixels_scatter: out')
    _call('gd4d_even_pixels_scatter', _dev(src, 'src', F32), n * c, h, w, _dev(out, 'out', F32))
    return out


def _rt_dgrad(name, taps, dz, image_t, cin, hw, stride, add, mask, add2, add_even, out, m_blocks):
    lib = _lib.load()
    n, cout, hz, wz = _dcn_x(dz, name)
    cin, stride = int(cin), int(stride)
    h, w = (hz, wz) if hw is None else (int(hw[0]), int(hw[1]))
    if dcn_out_hw(h, w, stride) != (hz, wz):
        raise ValueError(f'{name}: dz {tuple(dz.shape)} is not the stride-{stride} output of an ({h}, {w}) map (hw= says which)')
    nbytes = int((lib.gd4d_conv3x3_act_image_t_bytes if taps == 9 else lib.gd4d_conv1x1_image_t_bytes)(cin, cout))
    if nbytes == 0 or nbytes != image_t.numel():
        made, limits = ('conv3x3_act_image_t', _CONV3X3_ACT_LIMITS) if taps == 9 else ('conv1x1_image_t', _CONV1X1_T_LIMITS)
        raise _lib.Gd4dError(f'{name}: the image is not {made} of a ({cout}, {cin}) weight the kernel takes ({limits})')
    for t, what in ((add, 'add'), (mask, 'mask'), (add2, 'add2')):
        if t is not None and tuple(t.shape) != (n, cin, h, w):
            raise ValueError(f'{name}: {what} must be ({n}, {cin}, {h}, {w}), got {tuple(t.shape)}')
    if add_even is not None and tuple(add_even.shape) != (n, cin) + dcn_out_hw(h, w, 2):
        raise ValueError(f'{name}: add_even must be {(n, cin) + dcn_out_hw(h, w, 2)}, got {tuple(add_even.shape)}')
    out = _out(out, (n, cin, h, w), dz.device, f'{name}: out')
    args = (_dev(image_t, 'image_t', U8), _opt(add, 'add'), _opt(mask, 'mask'), _opt(add2, 'add2'), _opt(add_even, 'add_even'),
            _dev(out, 'out', F32), int(m_blocks))
    if taps == 9:
        _call('gd4d_conv3x3_act_dgrad', _dev(dz, 'dz', F32), n, cin, cout, h, w, stride, *args)
    else:
        _call('gd4d_conv1x1_dgrad', _dev(dz, 'dz', F32), n, cin, cout, h, w, *args)
    return out


def conv1x1_dgrad(dz, image_t, cin, add=None, mask=None, add2=None, add_even=None, out=None, m_blocks=0):
    """gd4d_conv1x1_dgrad: dz (N, Cout, H, W) fp32 -> ((s W)^T dz (+ add)) ([mask > 0]) (+ add2) (+ add_even), (N, cin, H, W): a 1x1
    convolution's input gradient with image_t = conv1x1_image_t(weight, scale).  add / mask / add2: optional maps of the result's shape
    (out may be add or add2); add_even: an optional map of half its resolution, added at the pixels whose row and column are both
    even (a stride-2 downsample's gradient: that branch's own adjoint is this call on its half-resolution dz).  m_blocks: as
    conv3x3_bn_relu's, dividing cin / 32; the same bits either way."""
    return _rt_dgrad('conv1x1_dgrad', 1, dz, image_t, cin, None, 1, add, mask, add2, add_even, out, m_blocks)


def conv3x3_act_dgrad(dz, image_t, cin, hw=None, stride=1, add=None, mask=None, add2=None, add_even=None, out=None, m_blocks=0):
    """gd4d_conv3x3_act_dgrad: conv1x1_dgrad's counterpart for the 3x3 (pad 1) of stride 1 or 2 with image_t =
    conv3x3_act_image_t(weight, scale); hw = the result's (H, W), needed at stride 2 (dz is its stride-2 output's size)."""
    return _rt_dgrad('conv3x3_act_dgrad', 9, dz, image_t, cin, hw, stride, add, mask, add2, add_even, out, m_blocks)


def _rt_wgrad(name, taps, dz, x, weight, bn, stride, want, partitions, outs, workspace):
    lib = _lib.load()
    n, cout, hz, wz = _dcn_x(dz, name)
    stride = int(stride)
    if x.dim() != 4 or int(x.shape[0]) != n or dcn_out_hw(x.shape[2], x.shape[3], stride) != (hz, wz):
        raise ValueError(f'{name}: x {tuple(x.shape)} for dz {tuple(dz.shape)} at stride {stride}')
    cin, h, w = int(x.shape[1]), int(x.shape[2]), int(x.shape[3])
    if tuple(bn.shape) != (3, cout):
        raise ValueError(f'{name}: bn must be (3, {cout}): scale, rstd, mean')
    if weight.numel() != cout * cin * taps or int(weight.shape[0]) != cout:
        raise ValueError(f'{name}: weight of {cout} x {cin} x {taps} values expected, got {tuple(weight.shape)}')
    if not any(want):
        raise ValueError(f'{name}: nothing asked for')
    work = cin // 32 * -(-cout // 256) if taps == 9 else -(-cin // 64) * -(-cout // 256)
    partitions = _vv_partitions(dz.device, int(lib.gd4d_resnet_wgrad_tiles(taps, n, h, w, stride)), work, partitions)
    nbytes = int(lib.gd4d_resnet_wgrad_workspace_bytes(taps, cin, cout, n, h, w, stride, partitions))
    if nbytes == 0:
        raise _lib.Gd4dError(f'{name}: {cin} -> {cout} channels, stride {stride}, partitions = {partitions}: the kernel takes '
                             f'{_CONV3X3_ACT_LIMITS if taps == 9 else _CONV1X1_T_LIMITS}, stride 1 or 2 and 1..4096 partitions')
    dev = dz.device
    o_dw, o_dgamma, o_dbeta = outs if outs is not None else (None, None, None)
    ws = _out(workspace, (nbytes // 4,), dev, f'{name}: workspace')
    dw = _out(o_dw, weight.shape, dev, f'{name}: dW') if want[0] else None
    dgamma = _out(o_dgamma, (cout,), dev, f'{name}: dgamma') if want[1] else None
    dbeta = _out(o_dbeta, (cout,), dev, f'{name}: dbeta') if want[2] else None
    _call('gd4d_conv3x3_act_wgrad' if taps == 9 else 'gd4d_conv1x1_wgrad', _dev(dz, 'dz', F32), _dev(x, 'x', F32), n, cin, cout, h, w,
          stride, partitions, _dev(ws, 'workspace', F32), _dev(weight, 'weight', F32), _dev(bn, 'bn', F32), _opt(dw, 'dw'),
          _opt(dgamma, 'dgamma'), _opt(dbeta, 'dbeta'))
    return dw, dgamma, dbeta


def conv1x1_wgrad(dz, x, weight, bn, stride=1, want=(True, True, True), partitions=None, outs=None, workspace=None):
    """gd4d_conv1x1_wgrad: conv3x3_wgrad's counterpart for a ResNet block's 1x1 convolution of stride 1 or 2: dz (N, Cout, Ho, Wo), x
    (N, Cin, H, W) read in place at the pixels (stride yo, stride xo), weight (Cout, Cin[, 1, 1]) unscaled, bn (3, Cout).  Returns
    (dW of weight's shape, dgamma, dbeta), None where `want` says so; outs / workspace as conv3x3_wgrad's."""
    return _rt_wgrad('conv1x1_wgrad', 1, dz, x, weight, bn, stride, want, partitions, outs, workspace)


def conv3x3_act_wgrad(dz, x, weight, bn, stride=1, want=(True, True, True), partitions=None, outs=None, workspace=None):
    """gd4d_conv3x3_act_wgrad: conv3x3_wgrad at ResNet's widths (Cout up to 512) and strides (1 or 2: dz is the stride's output size;
    at stride 2 the workspace also holds dz zero-interleaved to x's resolution)."""
    return _rt_wgrad('conv3x3_act_wgrad', 9, dz, x, weight, bn, stride, want, partitions, outs, workspace)


def _first_tensor(args):
    for a in args:
        if torch.is_tensor(a):
            return a
        if isinstance(a, (list, tuple)) and a and torch.is_tensor(a[0]):
            return a[0]
    return None


def _on_tensor_device(fn):
    """Run `fn` with the device of its first tensor argument current: _stream() then hands the C ABI that device's
    current stream and the library's per-device state (CU count, LDS attributes) refers to the right GPU, also when
    one process drives several GPUs or the tensors live on a non-current device."""
    @functools.wraps(fn)
    def wrapped(*args, **kwargs):
        t = _first_tensor(args)
        if t is None or not t.is_cuda or t.device.index == torch.cuda.current_device():
            return fn(*args, **kwargs)
        with torch.cuda.device(t.device):
            return fn(*args, **kwargs)
    return wrapped


_HOST_ONLY = {'linear_sum_assignment_batch', 'cross_attn_plan_bytes', 'invalidate_chain_images', 'kept_in_place', 'chain_load', 'chain_gemm', 'chain_small_linear', 'chain_layernorm',
              'chain_add', 'chain_refine', 'row_chain_fwd', 'chain_weight_image', 'chain_layernorm_bwd', 'cross_mha_plan', 'cross_mha_bwd_plan', 'petr_keys_plan'}
for _name, _fn in list(globals().items()):
    if inspect.isfunction(_fn) and _fn.__module__ == __name__ and not _name.startswith('_') and _name not in _HOST_ONLY:
        globals()[_name] = _on_tensor_device(_fn)
del _name, _fn
