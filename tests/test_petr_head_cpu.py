"""PETRHead / PETRv2Head without a GPU: the fp64 restatement against the fixture captured from the reference, the state-dict keys and
module sharing of both classes, the refusals, PETRTransformer.forward_keys, and the host-side row map of gd4d_petr_keys_fwd."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import petr_head_ref as P  # noqa: E402
from golden_io import Golden  # noqa: E402


@pytest.fixture(scope='module')
def golden():
    return Golden('petr_head')


def _fixture_state(g, kind):
    keys = json.loads(bytes(g.arrays[kind + '.keys']).decode())
    shapes = json.loads(bytes(g.arrays[kind + '.shapes']).decode())
    return keys, shapes, P.state_dict(keys, shapes, shared=kind == 'v1')


def _metas(g, kind):
    ts = g.arrays[kind + '.timestamps'] if g.has(kind + '.timestamps') else None
    return P.img_metas(g.arrays[kind + '.lidar2img'].astype(np.float64), ts)


@pytest.fixture(scope='module')
def restated(golden):
    """The fp64 restatement of both heads, computed once."""
    out = {}
    for kind in ('v1', 'v2'):
        _, _, sd = _fixture_state(golden, kind)
        out[kind] = P.head_forward(sd, P.head_config(kind), golden.t(kind + '.feat').float(), _metas(golden, kind))
    return out


@pytest.mark.parametrize('kind', ['v1', 'v2'])
def test_parameter_rule_reproduces_the_fixture_sums(golden, kind):
    keys, shapes, sd = _fixture_state(golden, kind)
    sums = np.asarray([float(sd[k].double().sum()) for k in keys])
    sqs = np.asarray([float((sd[k].double() ** 2).sum()) for k in keys])
    assert np.array_equal(sums, golden.arrays[kind + '.sums']) and np.array_equal(sqs, golden.arrays[kind + '.sumsqs'])
    assert sum(int(np.prod(s)) for s in shapes) > 4_000_000
    assert torch.equal(golden.t(kind + '.feat').float(), P.features(P.KINDS[kind]['in_channels']))
    assert np.array_equal(golden.arrays[kind + '.lidar2img'].astype(np.float64), P.camera_matrices())


@pytest.mark.parametrize('kind', ['v1', 'v2'])
def test_fp64_restatement_matches_the_reference_fixture(golden, restated, kind):
    """The fixture is the reference's fp32 run.  x is exact (grid inputs and weights).  pos_embed: the reference's fp32 frustum feeds
    inverse_sigmoid, which amplifies one ulp of a coordinate near its clamps - compared under the rule of the head-PE test (entries
    with |value| < 8 within 2e-4, the share above 1e-2 below 1e-3).  Observed (docs/measurements_r38.md): pos_embed 6.6e-6 / 3.6e-6,
    query_embeds 2.7e-7 / 2.7e-7, all_cls_scores 6.4e-7 / 7.7e-7, all_bbox_preds 9.5e-6 / 9.2e-6 (values up to 51.2; the velocity
    columns divided by 0.4 - 0.5 s) for PETRHead / PETRv2Head; the bounds are about 4 x the larger of each pair."""
    g, r = golden, restated[kind]
    assert torch.equal(r['x'].float(), g.t(kind + '.x@512').float().div(512))
    d = (r['pos_embed'] - g.t(kind + '.pos_embed')).abs()
    e_pos, e_q = float(d.max()), float((r['query_embeds'] - g.t(kind + '.query_embeds')).abs().max())
    e_cls = float((r['all_cls_scores'] - g.t(kind + '.all_cls_scores')).abs().max())
    e_box = float((r['all_bbox_preds'] - g.t(kind + '.all_bbox_preds')).abs().max())
    print(f'{kind}: pos_embed {e_pos:.2e}, query_embeds {e_q:.2e}, cls {e_cls:.2e}, box {e_box:.2e}')
    assert float(d[g.t(kind + '.pos_embed').abs() < 8].max()) < 2e-4 and float((d > 1e-2).float().mean()) < 1e-3
    assert e_pos < 2.8e-5 and e_q < 1.1e-6 and e_cls < 3.2e-6 and e_box < 4e-5
    mask = g.t(kind + '.mask')
    assert mask.dtype == torch.bool and mask[0, 1, :, 7:].all() and int(mask.sum()) == 18


def test_reference_frustum_stays_inside_the_share_for_the_chosen_matrices(golden):
    """The pos_embed comparison on the GPU uses the head-PE rule (test_head_pe_gpu.py:44-45); here: the reference's own fp32 frustum
    inputs against the fp64 ones obey it for this fixture's cameras, so a failure there is the kernel's."""
    metas = _metas(golden, 'v1')
    lo = P.frustum_inputs(metas, (P.H, P.W), 64, 1, P.POSITION_RANGE, dtype=torch.float32)
    hi = P.frustum_inputs(metas, (P.H, P.W), 64, 1, P.POSITION_RANGE)
    d = (lo.double() - hi).abs()
    print(f'frustum inputs fp32 vs fp64: max {float(d.max()):.2e} where |x| < 8: {float(d[hi.abs() < 8].max()):.2e}, '
          f'share > 1e-2: {float((d > 1e-2).float().mean()):.2e}')
    assert float(d[hi.abs() < 8].max()) < 2e-4 and float((d > 1e-2).float().mean()) < 1e-3


@pytest.mark.parametrize('kind', ['v1', 'v2'])
def test_registry_builds_both_heads_with_the_reference_keys(golden, kind):
    import graph_detr4d_amd as G
    assert G.HEADS.get('PETRHead') is G.PETRHead and G.HEADS.get('PETRv2Head') is G.PETRv2Head
    keys, _, sd = _fixture_state(golden, kind)
    head = G.build_head(P.head_config(kind))
    assert set(head.state_dict()) == set(keys)
    head.load_state_dict(sd, strict=True)
    for k, v in head.state_dict().items():
        assert torch.equal(v, sd[k]), k
    shared = head.cls_branches[0] is head.cls_branches[5] and head.reg_branches[0] is head.reg_branches[5]
    assert shared == (kind == 'v1')
    if kind == 'v2':
        assert head.cls_branches[0][0].weight is not head.cls_branches[1][0].weight
        assert type(head.reg_branches[0]).__name__ == 'RegLayer' and len(head.reg_branches[0].task_heads) == 5
        assert 'fpe.conv_reduce.weight' in keys and 'reg_branches.3.task_heads.4.2.bias' in keys
    else:
        assert 'fpe.conv_reduce.weight' not in keys
        with pytest.raises(TypeError):
            G.PETRHead(**{**{k: v for k, v in P.head_config('v1').items() if k != 'type'}, 'with_fpe': True})


def test_petr_head_converts_version_1_keys(golden):
    import graph_detr4d_amd as G
    keys, _, sd = _fixture_state(golden, 'v1')
    old = {}
    for k, v in sd.items():
        k = k.replace('.attentions.0.', '.self_attn.').replace('.attentions.1.', '.multihead_attn.').replace('.decoder.post_norm.', '.decoder.norm.')
        old[k] = v
    assert set(old) != set(sd)
    head = G.build_head(P.head_config('v1'))
    head.load_state_dict(old, strict=True)                                # (a plain dict carries no version metadata: version None)
    assert torch.equal(head.transformer.decoder.post_norm.weight, sd['transformer.decoder.post_norm.weight'])
    assert torch.equal(head.transformer.decoder.layers[1].attentions[1].attn.in_proj_weight,
                       sd['transformer.decoder.layers.1.attentions.1.attn.in_proj_weight'])


@pytest.mark.parametrize('over', [dict(LID=False), dict(with_multiview=False), dict(with_position=False), dict(normedlinear=True),
                                  dict(depth_num=32)])
def test_uncovered_configurations_are_refused_at_construction(over):
    import graph_detr4d_amd as G
    from graph_detr4d_amd._lib import Gd4dError
    with pytest.raises(Gd4dError, match='torch_ops=True'):
        G.build_head(P.head_config('v2', **over))
    if 'normedlinear' not in over:                                        # the explicit choice builds (and has the reference's keys)
        head = G.build_head(P.head_config('v2', torch_ops=True, **over))
        assert ('position_encoder.0.weight' in head.state_dict()) == over.get('with_position', True)


def test_position_level_train_mode_and_autograd_are_refused_on_the_kernel_route(monkeypatch):
    import graph_detr4d_amd as G
    from graph_detr4d_amd import functional as Fn
    from graph_detr4d_amd._lib import Gd4dError
    monkeypatch.setattr(Fn, 'require_gpu', lambda t, name: None)          # (the refusals come before any kernel)
    head = G.build_head(P.head_config('v2', position_level=1))
    feats = [torch.zeros(1, 2, 256, 6, 10), torch.zeros(1, 2, 64, 3, 5)]
    metas = P.img_metas(np.tile(np.eye(4), (2, 2, 1, 1)))[:1]
    head.train()
    with pytest.raises(Gd4dError, match='torch_ops = True'):             # train mode
        head(feats, metas)
    head.eval()
    with pytest.raises(Gd4dError, match='torch_ops = True'):             # eval mode, autograd on (parameters require grad)
        head(feats, metas)
    with torch.no_grad(), pytest.raises(Gd4dError, match='position_level.*torch_ops=True'):
        head([feats[1], feats[0]], metas)                                 # level 1 is not the map input_proj reads
    odd = G.build_head(P.head_config('v2', in_channels=48))
    with torch.no_grad(), pytest.raises(Gd4dError, match='torch_ops = True'):
        odd.eval()([torch.zeros(1, 2, 48, 6, 10)], metas)


def test_loss_builds_the_existing_criterion_or_names_what_it_does_not_cover():
    import graph_detr4d_amd as G
    from graph_detr4d_amd._lib import Gd4dError
    assigner = dict(type='HungarianAssigner3D', cls_cost=dict(type='FocalLossCost', weight=2.0),
                    reg_cost=dict(type='BBox3DL1Cost', weight=0.25), iou_cost=dict(type='IoUCost', weight=0.0), pc_range=P.PC_RANGE)
    head = G.build_head(P.head_config('v1', train_cfg=dict(pts=dict(assigner=assigner))))
    crit = head.criterion()
    assert isinstance(crit, G.Detr3DCriterion) and crit.loss_cls_weight == 2.0 and crit.loss_bbox_weight == 0.25
    assert torch.equal(crit.code_weights, head.code_weights)
    default = {k: v for k, v in P.head_config('v1').items() if k not in ('loss_cls', 'loss_bbox', 'loss_iou', 'train_cfg')}
    with pytest.raises(Gd4dError, match='loss_cls.*loss_iou.*assigner'):
        G.build_head(default).loss([], [], {})                            # the reference's DETR defaults: CrossEntropy, GIoU, HungarianAssigner


def test_criterion_stays_out_of_the_state_dict_and_follows_code_weights(golden):
    """The criterion is built lazily at the first loss: it must not become a submodule (its code_weights would be a state-dict key the
    reference does not have), and it is a value of the head's code_weights - a reload or an in-place update shows in the next one."""
    import graph_detr4d_amd as G
    assigner = dict(type='HungarianAssigner3D', cls_cost=dict(type='FocalLossCost', weight=2.0),
                    reg_cost=dict(type='BBox3DL1Cost', weight=0.25), iou_cost=dict(type='IoUCost', weight=0.0), pc_range=P.PC_RANGE)
    keys, _, sd = _fixture_state(golden, 'v2')
    head = G.build_head(P.head_config('v2', train_cfg=dict(assigner=assigner)))
    first = head.criterion()
    assert head.criterion() is first
    assert set(head.state_dict()) == set(keys) and not any(isinstance(m, G.Detr3DCriterion) for m in head.modules())
    head.load_state_dict(sd, strict=True)                                  # (missing / unexpected keys would raise)
    fresh = G.build_head(P.head_config('v2', train_cfg=dict(assigner=assigner)))
    fresh.load_state_dict(head.state_dict(), strict=True)                  # a checkpoint saved after a loss loads into a fresh head
    other = dict(sd)
    other['code_weights'] = torch.tensor([1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.5, 0.5, 0.25, 0.25])
    head.load_state_dict(other, strict=True)
    second = head.criterion()
    assert second is not first and torch.equal(second.code_weights, other['code_weights'])
    with torch.no_grad():
        head.code_weights.mul_(2.0)
    assert torch.equal(head.criterion().code_weights, 2.0 * other['code_weights'])
    moved = head.to(torch.float64)                                         # a move replaces the parameter's storage: rebuilt as well
    assert moved.criterion().code_weights.device == moved.code_weights.device
    assert torch.equal(moved.criterion().code_weights.double(), moved.code_weights)
    assert set(moved.state_dict()) == set(keys)


def test_reg_layer_never_changes_route_on_its_own():
    from graph_detr4d_amd._lib import Gd4dError
    from graph_detr4d_amd.petr_head import RegLayer
    layer = RegLayer()
    x = torch.zeros(3, 256)
    with pytest.raises(Gd4dError, match='torch_ops = True'):              # train mode
        layer(x)
    layer.eval()
    with pytest.raises(Gd4dError, match='torch_ops = True'):              # autograd (its parameters require grad)
        layer(x)
    with torch.no_grad(), pytest.raises(Gd4dError, match='GPU'):          # the kernel route needs the GPU: no CPU detour
        layer(x)
    layer.torch_ops = True                                                 # the explicit choice: the reference's op sequence
    want = torch.cat([h(layer.reg_branch(x)) for h in layer.task_heads], -1)
    assert torch.equal(layer(x), want) and tuple(want.shape) == (3, 10)


def test_forward_keys_equals_forward_on_the_transformer_fixture():
    """On plain tensors (the decoder replaced by a recorder: the module needs a GPU): forward hands forward_keys exactly the rows its two
    copies make, and returns forward_keys' result.  The real decoder through both, on both routes: tests/test_petr_head_gpu.py."""
    import graph_detr4d_amd as G
    g = Golden('petr_transformer')
    model = G.build_transformer(P.R.petr_config(g.meta['num_layers'], g.meta['feedforward_channels']))
    model.load_state_dict(g.state(), strict=True)
    seen = []

    class Recorder(torch.nn.Module):
        embed_dims = 256

        def forward(self, query, key, value, key_pos, query_pos, key_padding_mask, reg_branch=None):
            seen.append((key, value, key_pos, query_pos, key_padding_mask))
            return (query_pos[None] + key.sum(0)[None, None] + key_pos.sum(0)[None, None]).repeat(2, 1, 1, 1)
    model.decoder = Recorder()
    x, pos, mask, qe = g.t('x').float(), g.t('pos_embed').float(), g.t('mask'), g.t('query_embed').float()
    out, memory = model(x, mask, qe, pos)
    keys = x.permute(1, 3, 4, 0, 2).reshape(-1, 2, 256)
    key_pos = pos.permute(1, 3, 4, 0, 2).reshape(-1, 2, 256)
    direct = model.forward_keys(keys, key_pos, mask.reshape(2, -1), qe)
    assert torch.equal(out, direct) and tuple(out.shape) == (2, 2, g.meta['num_query'], 256)
    assert torch.equal(memory, x)
    for a, b in zip(seen[0], seen[1]):
        assert torch.equal(a, b)
    assert seen[0][0] is seen[0][1]                                       # value is key: one K|V GEMM on the kernel route


@pytest.mark.parametrize('bs', [1, 2])
@pytest.mark.parametrize('n,h,w', [(3, 5, 7), (2, 6, 10), (1, 1, 1), (6, 20, 50)])
def test_row_map_and_grid_of_the_key_launch(bs, n, h, w):
    """gd4d_petr_keys_plan is the host function the launch takes its grid and row map from: every key row is written exactly once, and
    row (cam h w + pix) bs + b holds camera (b, cam)'s pixel pix - the layout of x.permute(1, 3, 4, 0, 2).reshape(n h w, bs, c)."""
    from graph_detr4d_amd import ops
    grid, per, rows = ops.petr_keys_plan(bs, n, h, w)
    m = bs * n * h * w
    assert per == 128 and grid == (m + 127) // 128 and len(rows) == m
    assert sorted(rows) == list(range(m))
    idx = torch.arange(m).reshape(bs, n, 1, h, w)                         # the input row of (b, cam, pix)
    want = idx.permute(1, 3, 4, 0, 2).reshape(-1)                         # want[key row] = input row
    got = torch.empty(m, dtype=torch.long)
    got[torch.tensor(rows)] = torch.arange(m)
    assert torch.equal(got, want)


def test_key_launch_argument_checks_return_before_any_gpu_work():
    import ctypes
    from graph_detr4d_amd import _lib, ops
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    rng = (ctypes.c_double * 6)(*P.POSITION_RANGE)
    call = lambda **kw: lib.gd4d_petr_keys_fwd(ptr, ptr, kw.get('bs', 1), 1, kw.get('c', 256), 2, 2, 32., 32., kw.get('d', 64), 1.0,      # noqa: E731
                                               rng, kw.get('img', ptr), None, kw.get('pe_h', 1024), None, None, 0, ptr, ptr, ptr, None)
    assert call(bs=0) == -1 and call(img=None) == -1                     # GD4D_EINVAL
    assert call(c=128) == -2 and call(d=32) == -2 and call(pe_h=512) == -2                                 # GD4D_EUNSUPPORTED
    assert lib.gd4d_petr_keys_plan(1, 1, 0, 4, None, None, None) == -1
    assert lib.gd4d_petr_keys_plan(4, 24, 8192, 8192, None, None, None) == -2
    with pytest.raises(_lib.Gd4dError):
        ops.petr_keys_plan(4, 24, 8192, 8192, want_rows=False)
