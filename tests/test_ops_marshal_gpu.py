"""What ops.py's wrappers hand the C ABI, argument by argument.  Nothing launches: under _lib.recording(stand-in) every launching
entry point stores its arguments and returns 0; the size queries (*_bytes, *_tiles, anything that does not return an int code) are
the library's own.  Every case pins the entry's name and argument count, every scalar by value and type, every table by its bytes,
every pointer (null, or the data_ptr() of a named input / a returned tensor) and the stream in the last place."""
import ctypes
import struct

import pytest
import torch

from graph_detr4d_amd import _lib, ops

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
RANGE = [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]
LEVELS = [(2, 3), (1, 2)]
IMG_H, IMG_W = 96, 160


class StandIn:
    def __init__(self):
        self.real, self.calls = _lib.load(), []

    def __getattr__(self, name):
        if not name.startswith('gd4d_'):
            raise AttributeError(name)
        fn = getattr(self.real, name)
        if name.endswith('_bytes') or name.endswith('_tiles') or fn.restype is not ctypes.c_int:
            return fn

        def stored(*args):
            self.calls.append((name, args))
            return 0
        return stored


def capture(fn, *args, **kwargs):
    """(the wrapper's return value, entry name, arguments) of the one launching call `fn` makes."""
    stand_in = StandIn()
    with _lib.recording(stand_in):
        ret = fn(*args, **kwargs)
    assert len(stand_in.calls) == 1, [n for n, _ in stand_in.calls]
    return (ret,) + stand_in.calls[0]


def addr(a):
    if a is None:
        return 0
    return a if isinstance(a, int) else (a.value or 0)


def is_ptr(a, t):
    """a: what a wrapper passes for a tensor - a c_void_p of its data_ptr()."""
    return isinstance(a, ctypes.c_void_p) and a.value == t.data_ptr() and t.is_cuda


def on_stream(a):
    return isinstance(a, ctypes.c_void_p) and addr(a) == torch.cuda.current_stream().cuda_stream


def ints(args, want):
    """The scalars are Python ints of these values (no bool, no numpy / torch scalar)."""
    return all(type(a) is int for a in args) and list(args) == list(want)


def i32_table(a, values):
    return isinstance(a, ctypes.Array) and a._type_ is ctypes.c_int32 and bytes(a) == struct.pack(f'<{len(values)}i', *values)


def f64_table(a, values):
    return isinstance(a, ctypes.Array) and a._type_ is ctypes.c_double and bytes(a) == struct.pack(f'<{len(values)}d', *values)


def ptr_table(a, addrs):
    return isinstance(a, ctypes.Array) and a._type_ is ctypes.c_void_p and bytes(a) == struct.pack(f'<{len(addrs)}Q', *addrs)


LV = [2, 3, 1, 2]


def rand(*shape, dtype=torch.float32):
    if dtype is torch.float32:
        return torch.rand(*shape, device=DEV)
    return torch.zeros(*shape, device=DEV, dtype=dtype)


def geometry(b=1):
    """B, N=2, Q=3, 2 heads, Dh=4, P=1 over LEVELS: value, ref, offsets, attn_logits, cam_logits, lidar2img."""
    return dict(value=rand(b * 2, 8, 2, 4), ref=rand(b, 3, 3), offsets=rand(b, 3, 2, 1, 3), attn=rand(b, 3, 2, 2, 1),
                cam=rand(b, 3, 2), l2i=rand(b, 2, 4, 4))


def camera_run(args, g):
    """ref, offsets, attn_logits, cam_logits, lidar2img, rng, img_h, img_w: eight arguments."""
    return (is_ptr(args[0], g['ref']) and is_ptr(args[1], g['offsets']) and is_ptr(args[2], g['attn']) and is_ptr(args[3], g['cam'])
            and is_ptr(args[4], g['l2i']) and f64_table(args[5], RANGE) and type(args[6]) is float and args[6] == float(IMG_H)
            and type(args[7]) is float and args[7] == float(IMG_W))


@pytest.mark.parametrize('with_res', [False, True])
def test_layernorm_fwd(with_res):
    x, gamma, beta = rand(2, 8), rand(8), rand(8)
    res = rand(2, 8) if with_res else None
    out, name, a = capture(ops.layernorm_fwd, x, gamma, beta, res=res)
    assert name == 'gd4d_layernorm_fwd' and len(a) == 10
    assert is_ptr(a[0], x) and (is_ptr(a[1], res) if with_res else a[1] is None) and is_ptr(a[2], gamma) and is_ptr(a[3], beta)
    assert is_ptr(a[4], out) and out.shape == x.shape and out.dtype == torch.float32
    assert ints(a[5:7], [2, 8]) and type(a[7]) is float and a[7] == 1e-5 and ints(a[8:9], [0])
    assert on_stream(a[9])


def test_linear_fwd_on_a_column_slice():
    buf, weight = rand(4, 32), rand(16, 8)
    x = buf[:, :16]
    out, name, a = capture(ops.linear_fwd, x, weight, relu=True, weight_kn=True)
    assert name == 'gd4d_linear_fwd' and len(a) == 18
    assert is_ptr(a[0], x) and a[0].value == buf.data_ptr() and a[1] is None and is_ptr(a[2], weight)
    assert a[3] is None and a[4] is None and a[5] is None and is_ptr(a[6], out) and tuple(out.shape) == (4, 8)
    assert ints(a[7:16], [4, 16, 8, 8, 1 | 8, 32, 8, 8, 8])                     # m, k, n, n_split, flags, ldx, three row strides
    assert a[16] is None and on_stream(a[17])


def test_cross_attn_fwd():
    g = geometry()
    order = torch.arange(3, device=DEV, dtype=torch.int32)
    (out, mask), name, a = capture(ops.cross_attn_fwd, g['value'], LEVELS, g['ref'], g['offsets'], g['attn'], g['cam'], g['l2i'], RANGE,
                                   IMG_H, IMG_W, want_mask=True, want_uv=False, query_order=order)
    assert name == 'gd4d_cross_attn_fwd' and len(a) == 25
    assert is_ptr(a[0], g['value']) and i32_table(a[1], LV) and camera_run(a[2:10], g)
    assert is_ptr(a[10], out) and tuple(out.shape) == (1, 3, 8) and is_ptr(a[11], mask) and a[12] is None
    assert tuple(mask.shape) == (1, 2, 3, 2, 1) and mask.dtype == torch.uint8
    assert ints(a[13:23], [1, 2, 3, 2, 4, 2, 1, _lib.F32, _lib.PIXEL_MAJOR, 0])
    assert is_ptr(a[23], order) and on_stream(a[24])


def pyramid(b=1):
    sp = rand(8, b * 2, 8, 32)
    return sp, ops.PyramidView.slice_planar(sp, LEVELS)


def test_cross_attn_plan_fwd_items():
    g = geometry()
    sp, view = pyramid()
    plan, name, a = capture(ops.cross_attn_plan_fwd, view, g['ref'], g['offsets'], g['attn'], g['cam'], g['l2i'], RANGE, IMG_H, IMG_W,
                            2, items=True)
    assert name == 'gd4d_cross_attn_plan_fwd' and len(a) == 25
    assert camera_run(a[0:8], g) and i32_table(a[8], LV)
    assert isinstance(a[9], ctypes.Array) and a[9]._type_ is ctypes.c_int64 and bytes(a[9]) == struct.pack('<2q', *view.cam_stride)
    nbytes = ops.cross_attn_plan_bytes(1, 2, 3, 2, 1)
    assert ints(a[10:11], [view.pix_stride]) and is_ptr(a[11], plan.buf) and ints(a[12:13], [nbytes]) and plan.buf.numel() == nbytes
    assert is_ptr(a[13], plan.wsum) and tuple(plan.wsum.shape) == (1, 3, 2) and a[14] is None and a[15] is None
    assert ints(a[16:23], [1, 2, 3, 2, 2, 1, ops.CA_PLAN_ITEMS]) and a[23] is None and on_stream(a[24])
    assert plan.items and plan.pyramid is view and plan.points == 1


@pytest.mark.parametrize('b', [1, 2])
def test_cross_attn_bwd(b):
    g = geometry(b)
    grad_out = rand(b, 3, 8)
    grads, name, a = capture(ops.cross_attn_bwd, g['value'], LEVELS, g['ref'], g['offsets'], g['attn'], g['cam'], g['l2i'], RANGE,
                             IMG_H, IMG_W, grad_out)
    assert name == 'gd4d_cross_attn_bwd' and len(a) == 30
    assert is_ptr(a[0], g['value']) and i32_table(a[1], LV) and camera_run(a[2:10], g) and is_ptr(a[10], grad_out)
    assert all(is_ptr(p, t) for p, t in zip(a[11:16], grads))
    assert [tuple(t.shape) for t in grads] == [(b * 2, 8, 2, 4), (b, 3, 3), (b, 3, 2, 1, 3), (b, 3, 2, 2, 1), (b, 3, 2)]
    assert ints(a[16:26], [b, 2, 3, 2, 4, 2, 1, _lib.F32, _lib.PIXEL_MAJOR, 0]) and a[26] is None
    nbytes = int(_lib.load().gd4d_cross_attn_bwd_workspace_bytes(b, 3, 2, 2, 1))
    assert isinstance(a[28], ctypes.c_size_t) and a[28].value == nbytes
    assert (a[27] is None) if nbytes == 0 else (isinstance(a[27], ctypes.c_void_p) and addr(a[27]) != 0)
    assert on_stream(a[29])


def test_detr3d_fwd_mask_only():
    feats = [rand(1, 2, 4, 2, 3), rand(1, 2, 4, 1, 2)]
    ref, attn, l2i = rand(1, 3, 3), rand(1, 3, 2, 1, 2), rand(1, 2, 4, 4)
    ret, name, a = capture(ops.detr3d_fwd, feats, ref, attn, l2i, RANGE, IMG_H, IMG_W, want_out=False, want_mask=True)
    assert name == 'gd4d_detr3d_fwd' and len(a) == 18
    assert ptr_table(a[0], [f.data_ptr() for f in feats]) and i32_table(a[1], LV)
    assert is_ptr(a[2], ref) and is_ptr(a[3], attn) and is_ptr(a[4], l2i) and f64_table(a[5], RANGE)
    assert type(a[6]) is float and a[6] == float(IMG_H) and type(a[7]) is float and a[7] == float(IMG_W)
    assert a[8] is None and is_ptr(a[9], ret['mask']) and a[10] is None and ret['out'] is None and ret['sampled'] is None
    assert tuple(ret['mask'].shape) == (1, 2, 3) and ret['mask'].dtype == torch.uint8
    assert ints(a[11:17], [1, 2, 3, 4, 2, 1]) and on_stream(a[17])


def test_query_order_fwd():
    ref = geometry()['ref']
    order, name, a = capture(ops.query_order_fwd, ref, RANGE)
    assert name == 'gd4d_query_order_fwd' and len(a) == 6
    assert is_ptr(a[0], ref) and f64_table(a[1], RANGE) and is_ptr(a[2], order) and ints(a[3:5], [1, 3]) and on_stream(a[5])
    assert order.dtype == torch.int32 and tuple(order.shape) == (3,)


def conv_levels():
    return [rand(1, 256, 2, 3), rand(1, 256, 1, 2)]


def test_fpn_conv_fwd_channels_last():
    feats = conv_levels()
    images = [rand(16, dtype=torch.uint8), rand(16, dtype=torch.uint8)]
    bias = rand(256)
    outs, name, a = capture(ops.fpn_conv_fwd, feats, images, [bias, None], channels_last_out=True)
    assert name == 'gd4d_fpn_conv_fwd' and len(a) == 10
    assert ptr_table(a[0], [f.data_ptr() for f in feats]) and ptr_table(a[1], [o.data_ptr() for o in outs]) and i32_table(a[2], LV)
    assert ints(a[3:6], [2, 1, 256]) and ptr_table(a[6], [i.data_ptr() for i in images]) and ptr_table(a[7], [bias.data_ptr(), 0])
    assert ints(a[8:9], [1]) and on_stream(a[9])
    for o, f in zip(outs, feats):
        assert o.shape == f.shape and o.dtype == torch.float32 and o.permute(0, 2, 3, 1).is_contiguous()


def test_depth_bn_bwd():
    ys, douts = conv_levels(), conv_levels()
    stats, bn_bias, gate = rand(2, 3, 256), rand(256), rand(1, 256)
    (dys, dgamma, dbeta, dgate, dbias), name, a = capture(ops.depth_bn_bwd, douts, ys, stats, bn_bias, gate)
    assert name == 'gd4d_depth_bn_bwd' and len(a) == 17
    assert ptr_table(a[0], [t.data_ptr() for t in douts]) and ptr_table(a[1], [t.data_ptr() for t in ys])
    assert ptr_table(a[2], [t.data_ptr() for t in dys]) and i32_table(a[3], LV) and ints(a[4:7], [2, 1, 256])
    assert is_ptr(a[7], stats) and is_ptr(a[8], bn_bias) and is_ptr(a[9], gate) and ints(a[10:11], [0])
    assert isinstance(a[11], ctypes.c_void_p) and addr(a[11]) != 0
    assert is_ptr(a[12], dgamma) and is_ptr(a[13], dbeta) and is_ptr(a[14], dgate) and is_ptr(a[15], dbias) and on_stream(a[16])
    base = dgamma.data_ptr()                                  # one (3 + N, C) allocation: dgamma, dbeta, dbias, then dgate's N rows
    assert [dbeta.data_ptr() - base, dbias.data_ptr() - base, dgate.data_ptr() - base] == [1024, 2048, 3072]
    assert tuple(dgate.shape) == (1, 256) and [d.shape for d in dys] == [y.shape for y in ys]


def test_hungarian_assign_branches_fwd_absent_branch():
    nl, b, sum_gt, max_gt = 1, 1, 2, 2
    cost0 = rand(nl * 3 * sum_gt)
    gt_start = torch.tensor([0, 2], device=DEV, dtype=torch.int32)
    (assigned, copies, status), name, a = capture(ops.hungarian_assign_branches_fwd, [cost0, None], gt_start, nl, b, (3, 0), (1, 4),
                                                  sum_gt, max_gt, want_copy=True)
    assert name == 'gd4d_hungarian_assign_branches_fwd' and len(a) == 19
    assert is_ptr(a[0], cost0) and a[1] is None and is_ptr(a[2], gt_start)
    assert is_ptr(a[3], assigned[0]) and a[4] is None and assigned[1] is None
    assert is_ptr(a[5], copies[0]) and a[6] is None and copies[1] is None and is_ptr(a[7], status)
    assert tuple(assigned[0].shape) == (1, 1, 3) and assigned[0].dtype == torch.int32 and tuple(status.shape) == (2, 1, 1)
    nbytes = int(_lib.load().gd4d_hungarian_assign_branches_workspace_bytes(nl, b, 3, 0, max_gt))
    assert isinstance(a[8], ctypes.c_void_p) and (addr(a[8]) != 0) == (nbytes != 0) and ints(a[9:10], [nbytes])
    assert ints(a[10:18], [1, 1, 3, 0, 1, 4, 2, 2]) and on_stream(a[18])
