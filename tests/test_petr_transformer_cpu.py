"""PETR's transformer without a GPU: the fp64 restatement against the fixture captured from the reference, registry builds with the
reference's state-dict keys, the host-side plan of the long-key attention core, and argument checks of the new exports."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import petr_ref as R  # noqa: E402
from golden_io import Golden  # noqa: E402
from petr_ref import petr_config  # noqa: E402


@pytest.fixture(scope='module')
def golden():
    return Golden('petr_transformer')


def test_fp64_restatement_matches_the_reference_fixture(golden):
    """The fixture is the reference's fp32 run; its own rounding bounds the distance to fp64 by 1e-5.  Observed: 1.1e-6 on out_dec
    (values up to 2.8, three LayerNorms per layer), 4.4e-7 on the cross-attention output - the bounds below are 4x / 5x those."""
    g, m = golden, golden.meta
    out_dec, memory, cross0 = R.transformer(g.state(), m['num_heads'], m['num_layers'], g.t('x').float(), g.t('mask'),
                                            g.t('query_embed').float(), g.t('pos_embed').float())
    assert tuple(out_dec.shape) == (m['num_layers'], m['batch'], m['num_query'], m['embed_dims'])
    assert torch.equal(memory.float(), g.t('memory').float())
    e_out = float((out_dec - g.t('out_dec')).abs().max())
    e_cross = float((cross0 - g.t('cross0_out')).abs().max())
    print(f'out_dec {e_out:.2e}, cross-attention {e_cross:.2e}')
    assert e_out < 4e-6 and e_cross < 2e-6
    # the module alone, from its recorded input
    alone = R.attention(g.state(), 'decoder.layers.0.attentions.1.', m['num_heads'], g.t('cross0_query'),
                        g.t('x').float().permute(1, 3, 4, 0, 2).reshape(-1, m['batch'], 256), None,
                        query_pos=g.t('query_embed').float().unsqueeze(1).repeat(1, m['batch'], 1),
                        key_pos=g.t('pos_embed').float().permute(1, 3, 4, 0, 2).reshape(-1, m['batch'], 256),
                        key_padding_mask=g.t('mask').reshape(m['batch'], -1))
    assert float((alone - g.t('cross0_out')).abs().max()) < 2e-6


def test_fixture_mask_pads_three_columns_of_one_camera(golden):
    mask = golden.t('mask')
    assert mask.dtype == torch.bool and tuple(mask.shape) == (2, 2, 6, 10)
    assert mask[0, 1, :, 7:].all() and int(mask.sum()) == 18 and not mask[1].any()


def test_core_restatement_handles_masks_and_empty_rows():
    g = torch.Generator().manual_seed(3)
    q, k, v = (torch.randn(n, 2, 256, generator=g) for n in (5, 9, 9))
    mask = torch.zeros(2, 9, dtype=torch.bool)
    mask[0, 2:5] = True
    mask[1] = True
    out, lse = R.core(q, k, v, 8, mask)
    keep = ~mask[0]
    out0, lse0 = R.core(q[:, :1], k[keep][:, :1], v[keep][:, :1], 8)
    assert torch.allclose(out[:, :1], out0, atol=1e-12) and torch.allclose(lse[:, :1], lse0, atol=1e-12)
    assert torch.isnan(out[:, 1]).all() and torch.isinf(lse[:, 1]).all()
    want = torch.nn.functional.scaled_dot_product_attention(
        q.double().reshape(5, 2, 8, 32).permute(1, 2, 0, 3)[:1], k.double().reshape(9, 2, 8, 32).permute(1, 2, 0, 3)[:1],
        v.double().reshape(9, 2, 8, 32).permute(1, 2, 0, 3)[:1], attn_mask=keep[None, None, None, :])
    assert torch.allclose(out[:, 0], want[0].permute(1, 0, 2).reshape(5, 256), atol=1e-12)


def test_registry_builds_the_petrv2_block_with_the_reference_keys(golden):
    import graph_detr4d_amd as G
    for name, reg in (('PETRMultiheadAttention', G.ATTENTION), ('PETRTransformerDecoderLayer', G.TRANSFORMER_LAYER),
                      ('PETRTransformerDecoder', G.TRANSFORMER_LAYER_SEQUENCE), ('PETRTransformerEncoder', G.TRANSFORMER_LAYER_SEQUENCE),
                      ('PETRTransformer', G.TRANSFORMER)):
        assert name in reg and reg.get(name) is getattr(G, name)
    full = G.build_transformer(petr_config(6, 2048))                      # the config as shipped
    assert len(full.decoder.layers) == 6 and full.decoder.return_intermediate and full.encoder is None
    layer = full.decoder.layers[0]
    assert isinstance(layer.attentions[0], G.MultiheadAttention) and isinstance(layer.attentions[1], G.PETRMultiheadAttention)
    assert layer.use_checkpoint and layer.attentions[1].attn_drop == 0.1 and layer.attentions[1].dropout_layer.p == 0.1
    assert layer.ffns[0].layers[0][0].out_features == 2048
    small = G.build_transformer(petr_config(golden.meta['num_layers'], golden.meta['feedforward_channels']))
    sd = golden.state()
    small.load_state_dict(sd, strict=True)
    assert set(small.state_dict()) == set(sd)
    full.init_weights()
    w = full.decoder.layers[5].attentions[1].attn.out_proj
    assert float(w.bias.detach().abs().max()) == 0 and float(w.weight.detach().abs().max()) <= (6 / 512) ** 0.5


def test_encoder_and_plain_decoder_build():
    import graph_detr4d_amd as G
    layer = dict(type='BaseTransformerLayer', attn_cfgs=dict(type='PETRMultiheadAttention', embed_dims=256, num_heads=8),
                 feedforward_channels=64, operation_order=('norm', 'self_attn', 'norm', 'ffn'))
    enc = G.build_transformer_layer_sequence(dict(type='PETRTransformerEncoder', num_layers=1, transformerlayers=layer))
    assert enc.pre_norm and isinstance(enc.post_norm, torch.nn.LayerNorm) and 'post_norm.weight' in enc.state_dict()
    with pytest.raises(AssertionError):
        G.build_transformer_layer_sequence(dict(type='PETRTransformerEncoder', num_layers=1, transformerlayers=layer, post_norm_cfg=None))
    dec = G.build_transformer_layer_sequence(dict(type='PETRTransformerDecoder', num_layers=1, post_norm_cfg=None,
                                                  transformerlayers=petr_config(1, 64)['decoder']['transformerlayers']))
    assert dec.post_norm is None and not dec.return_intermediate
    with pytest.raises(AssertionError):                                   # the reference's asserts on the layer's order
        G.build_transformer_layer(dict(type='PETRTransformerDecoderLayer', attn_cfgs=dict(type='PETRMultiheadAttention', embed_dims=256,
                                       num_heads=8), feedforward_channels=64, operation_order=('self_attn', 'norm', 'ffn', 'norm')))


@pytest.mark.parametrize('b', [1, 2])
@pytest.mark.parametrize('lk', [1, 31, 32, 33, 95, 1000, 6000, 12000, 48000])
@pytest.mark.parametrize('lq', [1, 16, 17, 64, 65, 900])
def test_cross_mha_plan_covers_every_key_once(lq, lk, b):
    from graph_detr4d_amd import ops
    p = ops.cross_mha_plan(lq, lk, b, 8)
    steps = (lk + 31) // 32
    assert p.q_tile >= 64 and p.steps == steps and 1 <= p.splits <= ops.CROSS_MHA_MAX_SPLITS and len(p.ranges) == p.splits
    assert p.grid == ((lq + p.q_tile - 1) // p.q_tile, 8 * p.splits, b) and p.workgroups == p.grid[0] * p.grid[1] * p.grid[2]
    seen = torch.zeros(lk, dtype=torch.int32)
    at = 0
    for first, last in p.ranges:
        assert first == at and first % 32 == 0 and (last % 32 == 0 or last == lk)          # whole key steps, in order
        assert last > first                                                               # never empty: splits <= steps here
        seen[first:last] += 1
        at = last
    assert at == lk and bool((seen == 1).all())
    if lq == 900 and lk >= 6000 and b == 1:
        assert p.workgroups >= 256


def test_cross_mha_plan_forced_splits_and_refusals():
    from graph_detr4d_amd import _lib, ops
    p = ops.cross_mha_plan(65, 95, 1, 8, q_tile=32, splits=5)             # more splits than the 3 key steps: some are empty
    assert p.q_tile == 32 and p.splits == 5 and p.grid == (3, 40, 1)
    covered = [r for r in p.ranges if r[1] > r[0]]
    assert len(covered) == 3 and covered[0][0] == 0 and covered[-1][1] == 95
    assert all(a[1] == b[0] for a, b in zip(p.ranges, p.ranges[1:]))
    for bad in (dict(q_tile=48), dict(splits=65)):
        with pytest.raises(_lib.Gd4dError):
            ops.cross_mha_plan(900, 6000, 1, 8, **bad)
    with pytest.raises(_lib.Gd4dError):
        ops.cross_mha_plan(0, 6000, 1, 8)


def test_cross_mha_exports_validate_before_any_gpu_work():
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
    assert plane == b * h * 3 * 2 * 64 * 8 and lib.gd4d_cross_mha_plane_elems(0, b, h) == 0
    assert lib.gd4d_cross_mha_workspace_bytes(64, lk, b, h, 0, 1) == 0
    assert lib.gd4d_cross_mha_workspace_bytes(64, lk, b, h, 0, 3) == 3 * b * h * 64 * 34 * 4
    assert lib.gd4d_cross_mha_workspace_bytes(900, 12000, 1, h, 0, 0) == 4 * h * 900 * 34 * 4          # the plan: 4 splits
    assert lib.gd4d_cross_mha_plan(900, 6000, 1, 8, 0, 0, null) == EINVAL

    def fwd(q=ptr, kp=ptr, vp=ptr, stride=plane, out=ptr, ws=null, ws_bytes=0, lq=64, lk=lk, b=b, h=h, d=32, ldq=256, ldo=256,
            q_tile=0, splits=1):
        return lib.gd4d_cross_mha_fwd(q, kp, vp, stride, null, out, null, ws, ws_bytes, lq, lk, b, h, d, ldq, ldo, f(0.17), q_tile, splits, null)
    assert fwd(q=null) == EINVAL and fwd(kp=null) == EINVAL and fwd(vp=null) == EINVAL and fwd(out=null) == EINVAL
    assert fwd(lq=0) == EINVAL and fwd(lk=0) == EINVAL and fwd(b=0) == EINVAL
    assert fwd(ldq=128) == EINVAL and fwd(ldo=255) == EINVAL and fwd(stride=plane - 8) == EINVAL and fwd(stride=plane + 4) == EINVAL
    assert fwd(d=64) == EUNSUPPORTED and fwd(h=4) == EUNSUPPORTED and fwd(q_tile=16) == EUNSUPPORTED and fwd(splits=65) == EUNSUPPORTED
    assert fwd(q=odd) == EALIGN and fwd(kp=odd) == EALIGN and fwd(vp=odd) == EALIGN and fwd(ldq=258) == EALIGN
    assert fwd(splits=3) == EWORKSPACE and fwd(splits=3, ws=ptr, ws_bytes=64) == EWORKSPACE

    def pack(k=ptr, v=ptr, ldk=512, ldv=512, kp=ptr, vp=ptr, stride=plane, lk=lk, b=b, h=h, d=32):
        return lib.gd4d_cross_mha_pack_kv(k, v, ldk, ldv, kp, vp, stride, lk, b, h, d, null)
    assert pack(k=null) == EINVAL and pack(v=null) == EINVAL and pack(kp=null) == EINVAL and pack(vp=null) == EINVAL
    assert pack(lk=0) == EINVAL and pack(ldk=128) == EINVAL and pack(ldv=255) == EINVAL and pack(stride=plane - 8) == EINVAL
    assert pack(d=16) == EUNSUPPORTED and pack(h=16) == EUNSUPPORTED
    assert pack(k=odd) == EALIGN and pack(kp=odd) == EALIGN and pack(ldk=514) == EALIGN


def test_cross_mha_ops_refuse_cpu_tensors():
    from graph_detr4d_amd import _lib, ops
    z = torch.zeros
    with pytest.raises(_lib.Gd4dError):
        ops.CrossKV(33, 1, 'cpu')
    with pytest.raises(_lib.Gd4dError):
        ops.cross_mha_pack_kv(z(33, 1, 256), z(33, 1, 256))
    kv = object.__new__(ops.CrossKV)
    kv.lk, kv.b, kv.heads, kv.c, kv.steps = 33, 1, 8, 256, 2
    kv.k, kv.v = z(3, 1, 8, 2, 2, 64, 8, dtype=torch.bfloat16), z(2, 1, 8, 2, 2, 64, 8, dtype=torch.bfloat16)
    with pytest.raises(_lib.Gd4dError):
        ops.cross_mha_fwd(z(17, 1, 256), kv, 8)


def test_attention_module_refuses_cpu_tensors():
    import graph_detr4d_amd as G
    from graph_detr4d_amd import _lib
    m = G.build_attention(dict(type='PETRMultiheadAttention', embed_dims=256, num_heads=8)).eval()
    with pytest.raises(_lib.Gd4dError):
        with torch.no_grad():
            m(torch.zeros(4, 1, 256), torch.zeros(9, 1, 256))
