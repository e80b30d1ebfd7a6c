"""Cases and the fp64 reference of the PETR head's training kernels (ops.petr_keys_train_fwd, ops.petr_keys_bwd_rows, ops.mlp2_wgrad),
built from petr_head_ref's pieces and torch autograd in float64 on the CPU.  Nothing here imports a kernel.

Cases (bs, n, h, w), each at an edge of the 128-row tile:
    (1, 3, 5, 7)    105 rows  less than one tile, cameras end inside 4-pixel groups
    (1, 1, 16, 8)   128 rows  exactly one tile
    (1, 3, 1, 43)   129 rows  one tile and one row
    (2, 3, 5, 7)    210 rows  bs = 2 interleaves the key rows
    (2, 3, 8, 10)   480 rows  4 tiles, with a partition that holds two
the last three with partitions 1, 3 (uneven tile lists) and 8 (empty partitions).  Cameras: synthetic.camera_rig(num_frames=1,
img_hw=(16 h, 16 w)), as test_petr_head_gpu.test_petr_keys_fwd_alone takes them.  Weights on the k / 64 grid, k in [-3, 3]
(test_petr_head_gpu._grid, restated: that module imports the kernels); dY, dkey_pos and dmemory on a k / 8 grid.

The ReLU margin condition.  A hidden unit whose fp64 pre-activation lies within TAU = 1e-3 of zero on any row can take the other
branch in split-bf16 arithmetic, legitimately.  So the first bias of every such unit is raised by 1 / 64, repeatedly, until none is
left (margin_bias); test_petr_head_train_cpu.py asserts the condition on the result, and that nothing is excluded from a comparison.
"""
import functools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import petr_head_ref as P  # noqa: E402

F64 = torch.float64
TAU = 1e-3
CASES = [(1, 3, 5, 7), (1, 1, 16, 8), (1, 3, 1, 43), (2, 3, 5, 7), (2, 3, 8, 10)]
PARTITIONS = {c: ((1, 3, 8) if i >= 2 else (1,)) for i, c in enumerate(CASES)}
CASE_PARTS = [(c, p) for c in CASES for p in PARTITIONS[c]]
SEED = {c: 0 for c in CASES}                     # added to the weights' seeds; a case that cannot meet the condition takes another


def grid(shape, seed, k, scale):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-k, k + 1, shape, generator=g).float() / scale


def mlp_weights(kind, seed=0):
    """(W1, b1, W2, b2) float32 on the k / 64 grid: 'pe' position_encoder 192 -> 1024 -> 256 (test_petr_head_gpu.mlps' seeds), 'adapt'
    adapt_pos3d 384 -> 1024 -> 256, 'gate' fpe.conv_reduce / conv_expand 256 -> 256 -> 256."""
    k1, h, s0 = dict(pe=(192, 1024, 1), adapt=(384, 1024, 21), gate=(256, 256, 5))[kind]
    s0 += 100 * seed
    return grid((h, k1), s0, 3, 64), grid((h,), s0 + 1, 3, 64), grid((256, h), s0 + 2, 3, 64), grid((256,), s0 + 3, 3, 64)


def pre_activation(x, w1, b1):
    return x.to(F64) @ w1.to(F64).t() + b1.to(F64)


def margin_bias(x, w1, b1, max_rounds=64):
    """b1 with every unit whose pre-activation comes within TAU of zero on a row of x raised by 1 / 64 until none is left, and the
    number of rounds it took."""
    b1 = b1.clone()
    xw = x.to(F64) @ w1.to(F64).t()
    for rounds in range(max_rounds + 1):
        bad = ((xw + b1.to(F64)).abs() < TAU).any(0)
        if not bool(bad.any()):
            return b1, rounds
        b1[bad] += 1.0 / 64
    raise AssertionError('margin_bias: the case cannot be brought inside the ReLU margin condition - change its seed')


def metas_for(bs, n, h, w):
    """img_metas of petr_head_ref's form for the case: camera 1 (where there is one) has its last 2 feature columns padded."""
    pad_hw = (16 * h, 16 * w)
    rig = np.asarray(__import__('graph_detr4d_amd.synthetic', fromlist=['x']).camera_rig(num_frames=1, img_hw=pad_hw), dtype=np.float64)
    l2i = rig[:bs * n].reshape(bs, n, 4, 4)
    metas = []
    for b in range(bs):
        shapes = [(pad_hw[0], pad_hw[1] - (32 if (b, c) == (0, 1) and w > 2 else 0), 3) for c in range(n)]
        metas.append(dict(lidar2img=[l2i[b, c] for c in range(n)], img_shape=shapes, pad_shape=[(pad_hw[0], pad_hw[1], 3)] * n))
    return metas, l2i


def rows(t):
    """(R, C, H, W) -> (R H W, C): the camera-major rows."""
    return t.flatten(2).transpose(1, 2).reshape(-1, t.shape[1])


def key_rows(t, bs, n):
    """(bs n S, C) camera-major rows -> (n S, bs, C) key rows; and back with from_key_rows."""
    s = t.shape[0] // (bs * n)
    return t.view(bs, n, s, -1).permute(1, 2, 0, 3).reshape(n * s, bs, -1)


def from_key_rows(t, bs, n):
    s = t.shape[0] // n
    return t.view(n, s, bs, -1).permute(2, 0, 1, 3).reshape(bs * n * s, -1)


@functools.lru_cache(maxsize=None)
def case(bs, n, h, w):
    """Everything a case's tests share, computed once: inputs (float32, what the kernels are handed) and the fp64 X of both MLPs."""
    r, s = bs * n, h * w
    m = r * s
    metas, l2i = metas_for(bs, n, h, w)
    seed = SEED[(bs, n, h, w)]
    c = dict(bs=bs, n=n, h=h, w=w, m=m, pad_hw=(16 * h, 16 * w), metas=metas)
    c['i2l'] = torch.from_numpy(np.linalg.inv(l2i)).float().view(r, 4, 4)
    c['x_fr'] = rows(P.frustum_inputs(metas, (h, w), 64, 1, P.POSITION_RANGE, dtype=F64))          # (M, 192) fp64
    mask = P.padding_masks(metas, (h, w))
    c['mask'] = mask
    c['x_sine'] = rows(P.sine3d(mask).flatten(0, 1)).float()                                       # (M, 384) as the kernel reads it
    c['x'] = grid((bs, n, 256, h, w), 11, 16, 8)
    c['sine'] = grid((r, s, 256), 12, 16, 8)
    c['dy'] = grid((m, 256), 31, 8, 8)
    c['dkey_pos'] = grid((n * s, bs, 256), 32, 8, 8)
    c['dmemory'] = grid((n * s, bs, 256), 33, 8, 8)
    inputs = dict(pe=c['x_fr'], adapt=c['x_sine'], gate=rows(c['x'].flatten(0, 1)))
    for kind, xin in inputs.items():
        w1, b1, w2, b2 = mlp_weights(kind, seed)
        b1, rounds = margin_bias(xin, w1, b1)
        c[kind] = dict(w1=w1, b1=b1, w2=w2, b2=b2, x=xin, rounds=rounds)
    return c


def mlp_forward(x, w1, b1, w2, b2):
    return torch.relu(pre_activation(x, w1, b1)) @ w2.to(F64).t() + b2.to(F64)


def mlp_grads(x, w1, b1, w2, dy):
    """dict(dw2, db2, dw1, db1) float64 of sum(y dy), y = relu(x W1^T + b1) W2^T + b2, by torch autograd."""
    p = [t.to(F64).clone().requires_grad_(True) for t in (w1, b1, w2)]
    b2 = torch.zeros(w2.shape[0], dtype=F64, requires_grad=True)
    y = torch.relu(x.to(F64) @ p[0].t() + p[1]) @ p[2].t() + b2
    (y * dy.to(F64)).sum().backward()
    return dict(dw2=p[2].grad, db2=b2.grad, dw1=p[0].grad, db1=p[1].grad)


def mlp_grads_explicit(x, w1, b1, w2, dy):
    """The same five gradients written out with a materialised hidden activation."""
    x, dy = x.to(F64), dy.to(F64)
    hid = torch.relu(pre_activation(x, w1, b1))
    dhid = (dy @ w2.to(F64)) * (hid > 0)
    return dict(dw2=dy.t() @ hid, db2=dy.sum(0), dw1=dhid.t() @ x, db1=dhid.sum(0))


def keys_reference(c, gate):
    """fp64: pe, logits (gate) and key_pos (key rows) of the forward launch on the case's inputs, `sine` being the case's sine tensor."""
    pe = mlp_forward(c['pe']['x'], *(c['pe'][k] for k in ('w1', 'b1', 'w2', 'b2')))
    logits = mlp_forward(c['gate']['x'], *(c['gate'][k] for k in ('w1', 'b1', 'w2', 'b2'))) if gate else None
    out = pe * torch.sigmoid(logits) if gate else pe
    out = out + c['sine'].to(F64).view(-1, 256)
    return pe, logits, key_rows(out, c['bs'], c['n'])


def rows_reference(c, pe, logits):
    """fp64: (dpe, dlogit, dsine, dx0) of key_pos = pe sigmoid(logits) + sine, memory = x^T from the case's dkey_pos / dmemory; pe,
    logits: the float32 tensors the kernel is handed (None, None: no gate)."""
    bs, n, h, w = c['bs'], c['n'], c['h'], c['w']
    g = from_key_rows(c['dkey_pos'].to(F64), bs, n)
    dx0 = from_key_rows(c['dmemory'].to(F64), bs, n).view(bs * n, h * w, 256).transpose(1, 2).reshape(bs * n, 256, h, w)
    if logits is None:
        return g, None, g, dx0
    s = torch.sigmoid(logits.to(F64))
    return g * s, g * pe.to(F64) * s * (1 - s), g, dx0
