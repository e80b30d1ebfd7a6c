"""Training PETR's cross-attention, without a GPU: the fp64 restatement under autograd against the gradient fixture captured from the
reference (tests/golden/petr_transformer_grads.npz), the host-side plan of the backward, argument checks of the new exports, and the
hip_train keyword's way through the registry."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import petr_grads as PG  # noqa: E402
import petr_ref as R  # noqa: E402
from golden_io import Golden  # noqa: E402
from petr_ref import petr_config  # noqa: E402

# The fixture is the reference's fp32 CPU run; its distance from fp64 on the same inputs, per tensor, as max error / max(1, max |value|).
# Observed: 1.2e-4 at worst - colsum of layer 1's self-attention out_proj.weight gradient, an error of 2^-13 on sums whose terms reach
# hundreds (rowsum of the same matrix: 567) and cancel; the input gradients are at 1.4e-7 (grad.x, values up to 0.23), biases and norms
# at 4e-6 - 1.3e-5 on values of 14 - 53.  The bound is about 4 x the worst, as the forward fixture's was set.
FIXTURE_REL = 5e-4


@pytest.fixture(scope='module')
def golden():
    return Golden('petr_transformer')


@pytest.fixture(scope='module')
def grads():
    return Golden('petr_transformer_grads')


def test_fp64_restatement_reproduces_the_fixture_gradients(golden, grads):
    g, m = golden, golden.meta
    sd = {k: v.double().requires_grad_(True) for k, v in g.state().items()}
    x, pos, qe = (g.t(k).double().requires_grad_(True) for k in ('x', 'pos_embed', 'query_embed'))
    out_dec, _, _ = R.transformer(sd, m['num_heads'], m['num_layers'], x, g.t('mask'), qe, pos)
    (out_dec * grads.t('G').double()).sum().backward()
    errs = PG.errors(PG.as_fixture(x, pos, qe, [(k, v.grad) for k, v in sd.items()]), grads)
    print(PG.table(errs, 'fp64 restatement against the fp32 reference fixture: max error (scale)'))
    worst, key = PG.worst_relative(errs)
    print(f'worst relative: {worst:.2e} ({key})')
    assert worst < FIXTURE_REL


def test_fixture_holds_every_parameter_and_zero_gradients_at_padded_pixels(golden, grads):
    sd = golden.state()
    for k, v in sd.items():
        if v.dim() == 1:
            assert tuple(grads.t('grad.' + k).shape) == tuple(v.shape)
        else:
            assert tuple(grads.t('rowsum.' + k).shape) == (v.shape[0],) and tuple(grads.t('colsum.' + k).shape) == (v.shape[1],)
    assert grads.arrays['G'].dtype.name == 'float16' and tuple(grads.t('G').shape) == tuple(golden.t('out_dec').shape)
    gx, gp, mask = grads.t('grad.x'), grads.t('grad.pos_embed'), golden.t('mask')
    pad = mask[:, :, None].expand_as(gx)
    assert bool(pad.any()) and bool((gx[pad] == 0).all()) and bool((gp[pad] == 0).all())
    assert float(gx[~pad].abs().min()) > 0


@pytest.mark.parametrize('lq,lk,b', [(900, 12000, 1), (1500, 48000, 2), (1, 1, 1), (65, 95, 2)])
def test_bwd_plan_is_consistent(lq, lk, b):
    from graph_detr4d_amd import _lib, ops
    p = ops.cross_mha_bwd_plan(lq, lk, b, 8)
    print(p)
    steps, qsteps = (lk + 31) // 32, (lq + 31) // 32
    assert p.q_tile == 32 and p.steps == steps and p.query_steps == qsteps and 1 <= p.splits <= ops.CROSS_MHA_MAX_SPLITS
    # the query side: every query in one workgroup per (head, split, batch); every key step in exactly one split
    assert p.query_grid == (qsteps, 8 * p.splits, b) and p.query_block == 256 and p.query_grid[0] * p.q_tile >= lq > (p.query_grid[0] - 1) * p.q_tile
    at = 0
    for first, last in p.ranges:
        assert first == at and first % 32 == 0 and (last % 32 == 0 or last == lk) and last > first
        at = last
    assert at == lk
    # the key side: every key in one workgroup per (head, batch), no split
    assert p.key_block == 64 and p.key_block_threads == 256 and p.key_grid == ((lk + 63) // 64, 8, b)
    assert p.key_grid[0] * p.key_block >= lk > (p.key_grid[0] - 1) * p.key_block
    # workspace: twelve query planes of bf16, Dq and lse per padded query and head; one dq partial per split
    lib = _lib.load()
    assert p.pack_bytes == 12 * lib.gd4d_cross_mha_plane_elems(lq, b, 8) * 2 + 2 * b * 8 * qsteps * 32 * 4
    assert p.partial_bytes == (p.splits * b * 8 * lq * 32 * 4 if p.splits > 1 else 0)
    assert p.workspace_bytes == p.pack_bytes + p.partial_bytes == lib.gd4d_cross_mha_bwd_workspace_bytes(lq, lk, b, 8, 0, 0)
    if (lq, lk, b) == (900, 12000, 1):
        assert p.key_grid == (188, 8, 1) and p.query_grid[0] * p.query_grid[1] >= 256
    forced = ops.cross_mha_bwd_plan(lq, lk, b, 8, q_tile=32, splits=5)
    assert forced.splits == 5 and forced.ranges[0][0] == 0 and forced.ranges[-1][1] == lk
    assert all(a[1] == c[0] for a, c in zip(forced.ranges, forced.ranges[1:]))
    for bad in (dict(q_tile=64), dict(q_tile=48), dict(splits=65)):
        with pytest.raises(_lib.Gd4dError):
            ops.cross_mha_bwd_plan(lq, lk, b, 8, **bad)


def test_training_exports_validate_before_any_gpu_work():
    """In the style of tests/test_abi.py: bad calls come back with an error code on a box without a GPU."""
    from graph_detr4d_amd import _lib
    lib = _lib.load()
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 96)()
    ptr = ctypes.c_void_p((ctypes.addressof(buf) + 63) & ~63)
    odd = ctypes.c_void_p(ptr.value + 4)
    EINVAL, EUNSUPPORTED, EALIGN, EWORKSPACE = -1, -2, -3, -5
    f = ctypes.c_float
    lk, b, h = 95, 2, 8
    plane = lib.gd4d_cross_mha_plane_elems(lk, b, h)
    assert lib.gd4d_cross_mha_bwd_plan(900, 6000, 1, 8, 0, 0, null) == EINVAL
    assert lib.gd4d_cross_mha_bwd_workspace_bytes(0, lk, b, h, 0, 0) == 0

    def fwd(q=ptr, kp=ptr, vp=ptr, stride=plane, out=ptr, ws=null, ws_bytes=0, lq=64, lk=lk, b=b, h=h, d=32, ldq=256, ldo=256,
            q_tile=0, splits=1, p=0.1, seed=ptr):
        return lib.gd4d_cross_mha_train_fwd(q, kp, vp, stride, null, out, null, ws, ws_bytes, lq, lk, b, h, d, ldq, ldo, f(0.17), q_tile,
                                            splits, f(p), seed, null)
    assert fwd(q=null) == EINVAL and fwd(kp=null) == EINVAL and fwd(vp=null) == EINVAL and fwd(out=null) == EINVAL
    assert fwd(lq=0) == EINVAL and fwd(ldq=128) == EINVAL and fwd(stride=plane - 8) == EINVAL
    assert fwd(p=1.0) == EINVAL and fwd(p=-0.1) == EINVAL and fwd(seed=null) == EINVAL
    assert fwd(d=64) == EUNSUPPORTED and fwd(h=4) == EUNSUPPORTED and fwd(q_tile=16) == EUNSUPPORTED and fwd(splits=65) == EUNSUPPORTED
    assert fwd(lq=70000, lk=70000, b=2, stride=lib.gd4d_cross_mha_plane_elems(70000, 2, h)) == EUNSUPPORTED      # 2 x 8 x 70000^2 >= 2^32
    assert fwd(q=odd) == EALIGN and fwd(kp=odd) == EALIGN and fwd(ldq=258) == EALIGN
    assert fwd(splits=3) == EWORKSPACE

    def pack(k=ptr, v=ptr, ldk=512, ldv=512, kp=ptr, vp=ptr, vk=ptr, kv=ptr, stride=plane, lk=lk, b=b, h=h, d=32):
        return lib.gd4d_cross_mha_pack_kv_train(k, v, ldk, ldv, kp, vp, vk, kv, stride, lk, b, h, d, null)
    assert pack(k=null) == EINVAL and pack(v=null) == EINVAL and pack(kp=null) == EINVAL
    assert pack(lk=0) == EINVAL and pack(ldk=128) == EINVAL and pack(ldv=255) == EINVAL and pack(stride=plane - 8) == EINVAL
    assert pack(d=16) == EUNSUPPORTED and pack(h=16) == EUNSUPPORTED
    assert pack(k=odd) == EALIGN and pack(kp=odd) == EALIGN and pack(vk=odd) == EALIGN and pack(kv=odd) == EALIGN
    assert pack(v=odd) == EALIGN and pack(ldv=514) == EALIGN and pack(ldk=514) == EALIGN

    need = lib.gd4d_cross_mha_bwd_workspace_bytes(64, lk, b, h, 0, 1)
    assert need == 12 * lib.gd4d_cross_mha_plane_elems(64, b, h) * 2 + 2 * b * h * 64 * 4

    def bwd(dout=ptr, q=ptr, out=ptr, lse=ptr, kp=ptr, vk=ptr, kv=ptr, stride=plane, dq=ptr, dk=ptr, dv=ptr, ws=ptr, ws_bytes=need,
            lq=64, lk=lk, b=b, h=h, d=32, ldg=256, ldq=256, ldo=256, ld_dq=256, ld_dk=512, ld_dv=512, p=0., seed=null, q_tile=0,
            splits=1):
        return lib.gd4d_cross_mha_bwd(dout, q, out, lse, kp, vk, kv, stride, null, dq, dk, dv, ws, ws_bytes, lq, lk, b, h, d, ldg, ldq,
                                      ldo, ld_dq, ld_dk, ld_dv, f(0.17), f(p), seed, q_tile, splits, null)
    for name in ('dout', 'q', 'out', 'lse', 'kp', 'vk', 'kv', 'dq', 'dk', 'dv'):
        assert bwd(**{name: null}) == EINVAL, name
    assert bwd(lq=0) == EINVAL and bwd(lk=0) == EINVAL and bwd(b=0) == EINVAL
    assert bwd(ldg=128) == EINVAL and bwd(ldq=255) == EINVAL and bwd(ldo=8) == EINVAL and bwd(ld_dq=128) == EINVAL
    assert bwd(ld_dk=255) == EINVAL and bwd(ld_dv=0) == EINVAL and bwd(stride=plane - 8) == EINVAL and bwd(stride=plane + 4) == EINVAL
    assert bwd(p=0.1) == EINVAL and bwd(p=1.0, seed=ptr) == EINVAL
    assert bwd(d=64) == EUNSUPPORTED and bwd(h=4) == EUNSUPPORTED and bwd(q_tile=64) == EUNSUPPORTED and bwd(splits=65) == EUNSUPPORTED
    assert bwd(dout=odd) == EALIGN and bwd(q=odd) == EALIGN and bwd(out=odd) == EALIGN and bwd(kp=odd) == EALIGN
    assert bwd(vk=odd) == EALIGN and bwd(kv=odd) == EALIGN and bwd(ws=odd) == EALIGN and bwd(ldg=258) == EALIGN and bwd(ldq=258) == EALIGN
    assert bwd(ws=null) == EWORKSPACE and bwd(ws_bytes=need - 4) == EWORKSPACE and bwd(splits=3) == EWORKSPACE


def test_hip_train_keyword_reaches_the_module():
    import graph_detr4d_amd as G
    m = G.build_attention(dict(type='PETRMultiheadAttention', embed_dims=256, num_heads=8, dropout=0.1, hip_train=True))
    assert m.hip_train is True and m.attn_drop == 0.1 and not m.torch_ops
    assert G.build_attention(dict(type='PETRMultiheadAttention', embed_dims=256, num_heads=8)).hip_train is False
    cfg = petr_config(2, 64)
    cfg['decoder']['transformerlayers']['attn_cfgs'][1]['hip_train'] = True
    model = G.build_transformer(cfg)
    for layer in model.decoder.layers:
        assert layer.attentions[1].hip_train is True and not hasattr(layer.attentions[0], 'hip_train')
    with pytest.raises(TypeError):                                        # other unknown keywords are still refused
        G.build_attention(dict(type='PETRMultiheadAttention', embed_dims=256, num_heads=8, hip_trains=True))


def test_training_ops_refuse_cpu_tensors():
    from graph_detr4d_amd import _lib, ops
    z = torch.zeros
    with pytest.raises(_lib.Gd4dError):
        ops.cross_mha_pack_kv(z(33, 1, 256), z(33, 1, 256), train=True)
    kv = object.__new__(ops.CrossKV)
    kv.lk, kv.b, kv.heads, kv.c, kv.steps = 33, 1, 8, 256, 2
    kv.k = z(3, 1, 8, 2, 2, 64, 8, dtype=torch.bfloat16)
    kv.v = kv.vk = kv.kv = z(2, 1, 8, 2, 2, 64, 8, dtype=torch.bfloat16)
    with pytest.raises(_lib.Gd4dError):
        ops.cross_mha_bwd(z(17, 1, 256), z(17, 1, 256), z(17, 1, 256), z(17, 1, 8), kv, 8)
