"""PETRHeadseg without a GPU: the fp64 restatement of the lane half against the fixture captured from the reference
(tests/golden/petr_head_seg.npz), the state-dict keys and module sharing, the version-1 key conversion in both transformers, the
refusals, the argument checks of the two lane entry points, and Sigmoid_ce_loss on the CPU."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import petr_head_ref as P  # noqa: E402
import petr_head_seg_ref as S  # noqa: E402
from golden_io import Golden  # noqa: E402


@pytest.fixture(scope='module')
def golden():
    return Golden('petr_head_seg')


def _fixture_state(g):
    keys = json.loads(bytes(g.arrays['keys']).decode())
    shapes = json.loads(bytes(g.arrays['shapes']).decode())
    return keys, shapes, S.state_dict(keys, shapes)


def _metas(g):
    return P.img_metas(g.arrays['lidar2img'].astype(np.float64), g.arrays['timestamps'])


@pytest.fixture(scope='module')
def restated(golden):
    """The fp64 restatement of the whole head, computed once."""
    _, _, sd = _fixture_state(golden)
    cfg = S.head_config()
    return S.head_forward(sd, cfg, P.features(cfg['in_channels']), _metas(golden))


def test_parameter_rule_reproduces_the_fixture_sums(golden):
    keys, shapes, sd = _fixture_state(golden)
    sums = np.asarray([float(sd[k].double().sum()) for k in keys])
    sqs = np.asarray([float((sd[k].double() ** 2).sum()) for k in keys])
    assert np.array_equal(sums, golden.arrays['sums']) and np.array_equal(sqs, golden.arrays['sumsqs'])
    assert np.array_equal(golden.arrays['lidar2img'].astype(np.float64), P.camera_matrices())
    assert golden.meta['num_lane'] == S.NUM_LANE and golden.meta['loss_weight'] == S.LOSS_WEIGHT


def test_fp64_restatement_matches_the_reference_fixture(golden, restated):
    """The bounds of tests/test_petr_head_cpu.py::test_fp64_restatement_matches_the_reference_fixture for PETRv2Head (the same front
    end, transformer and branches): pos_embed under the head-PE rule and 2.8e-5, the query embeddings 1.1e-6, the logits 3.2e-6, the
    boxes 4e-5.  all_lane_preds are logits behind the same two-layer decoder and a three-layer MLP: the classification bound."""
    g, r = golden, restated
    assert torch.equal(r['x'].float(), g.t('x@512').float().div(512))
    d = (r['pos_embed'] - g.t('pos_embed')).abs()
    err = {k: float((r[k] - g.t(k)).abs().max()) for k in ('query_embeds', 'query_embeds_lane', 'all_cls_scores', 'all_bbox_preds',
                                                           'all_lane_preds')}
    print(f'pos_embed {float(d.max()):.2e}, ' + ', '.join(f'{k} {v:.2e}' for k, v in err.items()))
    assert float(d[g.t('pos_embed').abs() < 8].max()) < 2e-4 and float((d > 1e-2).float().mean()) < 1e-3
    assert float(d.max()) < 2.8e-5 and err['query_embeds'] < 1.1e-6 and err['query_embeds_lane'] < 1.1e-6
    assert err['all_cls_scores'] < 3.2e-6 and err['all_bbox_preds'] < 4e-5 and err['all_lane_preds'] < 3.2e-6
    assert tuple(g.t('all_lane_preds').shape) == (P.LAYERS, P.BS, S.NUM_LANE, 768)
    assert float(g.t('all_lane_preds').abs().max()) > 0.1                    # (not a fixture of zeros)


@pytest.mark.parametrize('r,c', S.FIXTURE_LOSS_SHAPES)
def test_loss_restatement_matches_the_reference_fixture(golden, r, c):
    """The fixture is torch's fp32 formula on the edge inputs (+-90, a row without positives, a row of positives only).  The issue's
    bounds for the kernel hold the reference itself: 2e-6 relative on the loss (torch's fp32 formula sits near 1e-7 there), and
    1e-6 loss_weight w / (R C) absolute on every gradient."""
    x, t = S.loss_case(1, r, c)
    loss, grad, w = S.sigmoid_ce(x[0], t, S.LOSS_WEIGHT)
    got, got_grad = float(golden.arrays[f'loss.{r}x{c}'][0]), golden.t(f'loss.{r}x{c}.grad').double()
    rel = abs(got - float(loss)) / float(loss)
    excess = float(((got_grad - grad).abs() - 1e-6 * S.LOSS_WEIGHT * w / (r * c)).max())
    print(f'{r} x {c}: loss {float(loss):.6f}, fixture off by {rel:.1e} relative; gradient excess over the bound {excess:.1e}')
    assert rel < 2e-6 and excess <= 0
    assert int((w == 0).sum()) == c * (r // 3)                               # the all-positive rows (r % 3 == 2): pw = 0


@pytest.mark.parametrize('r,c', S.FIXTURE_LOSS_SHAPES)
def test_sigmoid_ce_loss_on_the_cpu_equals_the_fixture(golden, r, c):
    import graph_detr4d_amd as G
    crit = G.build_loss(dict(type='Sigmoid_ce_loss', loss_weight=S.LOSS_WEIGHT))
    assert isinstance(crit, G.Sigmoid_ce_loss) and not list(crit.parameters())
    x, t = S.loss_case(1, r, c)
    x = x[0].clone().requires_grad_(True)
    loss = crit(x, t)
    loss.backward()
    np.testing.assert_allclose(float(loss.detach()), float(golden.arrays[f'loss.{r}x{c}'][0]), rtol=1e-6, atol=0)
    torch.testing.assert_close(x.grad, golden.t(f'loss.{r}x{c}.grad'), rtol=1e-6, atol=1e-12)
    layers = crit.layers(x.detach()[None].repeat(3, 1, 1), t)                # the torch lines per layer, then nan_to_num
    assert tuple(layers.shape) == (3,) and torch.equal(layers[0], layers[2])
    np.testing.assert_allclose(float(layers[1]), float(loss.detach()), rtol=1e-6, atol=0)
    bad = x.detach()[None].repeat(2, 1, 1)
    bad[1, 0, 0] = float('nan')
    assert float(crit.layers(bad, t)[1]) == 0.0 and torch.equal(crit.layers(bad, t)[0], layers[0])


def test_registry_builds_the_head_with_the_reference_keys(golden):
    import graph_detr4d_amd as G
    assert G.HEADS.get('PETRHeadseg') is G.PETRHeadseg and G.LOSSES.get('Sigmoid_ce_loss') is G.Sigmoid_ce_loss
    keys, shapes, sd = _fixture_state(golden)
    head = G.build_head(S.head_config())
    own = head.state_dict()
    assert set(own) == set(keys)
    assert all(list(own[k].shape) == s for k, s in zip(keys, shapes))
    head.load_state_dict(sd, strict=True)
    for k, v in head.state_dict().items():
        assert torch.equal(v, sd[k]), k
    assert 'se.conv_reduce.weight' in keys and not any(k.startswith('fpe.') for k in keys)
    assert 'lane_branches.5.4.bias' in keys and 'query_embedding_lane.2.weight' in keys
    assert any(k.startswith('transformer_lane.decoder.layers.1.attentions.1.') for k in keys)
    assert isinstance(head.loss_lane_mask, G.Sigmoid_ce_loss)
    with pytest.raises(TypeError, match='with_se'):
        G.build_head(S.head_config(with_fpe=True))


def test_branches_are_shared_and_the_lane_points_are_a_plain_tensor(golden):
    import graph_detr4d_amd as G
    keys, _, _ = _fixture_state(golden)
    head = G.build_head(S.head_config())
    for branches in (head.lane_branches, head.cls_branches, head.reg_branches):
        assert len(branches) == 6 and all(b is branches[0] for b in branches)
    assert tuple(head.lane_branches[0][-1].weight.shape) == (768, 256)
    assert 'reference_points_lane' not in keys and 'reference_points_lane' not in head.state_dict()
    assert 'reference_points_lane' not in dict(head.named_parameters()) and 'reference_points_lane' not in dict(head.named_buffers())
    pts = head.reference_points_lane
    assert torch.is_tensor(pts) and not pts.requires_grad and pts.device == head.input_proj.weight.device
    assert torch.equal(pts.double(), S.lane_points(S.NUM_LANE).float().double())
    assert head.double().reference_points_lane.dtype == torch.float64        # it follows the module's moves
    nine = G.build_head(S.head_config(num_lane=9)).reference_points_lane      # 'ij' order: the first coordinate is the slow one
    assert tuple(nine.shape) == (9, 2) and torch.equal(nine[1], torch.tensor([0.5 / 3, 1.5 / 3]))
    from graph_detr4d_amd.petr_head import pos2posemb2d
    assert float((pos2posemb2d(nine).double() - S.pos2posemb2d(nine)).abs().max()) < 1e-5


def test_version_1_keys_convert_in_both_transformers(golden):
    import graph_detr4d_amd as G
    _, _, sd = _fixture_state(golden)
    old = {}
    for k, v in sd.items():
        k = k.replace('.attentions.0.', '.self_attn.').replace('.attentions.1.', '.multihead_attn.').replace('.decoder.post_norm.', '.decoder.norm.')
        old[k] = v
    assert sum(k not in sd for k in old if k.startswith('transformer.')) > 0
    assert sum(k not in sd for k in old if k.startswith('transformer_lane.')) > 0
    head = G.build_head(S.head_config())
    head.load_state_dict(old, strict=True)                                # (a plain dict carries no version metadata: version None)
    for t in ('transformer', 'transformer_lane'):
        mod = getattr(head, t)
        assert torch.equal(mod.decoder.post_norm.weight, sd[f'{t}.decoder.post_norm.weight'])
        assert torch.equal(mod.decoder.layers[1].attentions[1].attn.in_proj_weight,
                           sd[f'{t}.decoder.layers.1.attentions.1.attn.in_proj_weight'])
        assert torch.equal(mod.decoder.layers[0].attentions[0].attn.out_proj.bias,
                           sd[f'{t}.decoder.layers.0.attentions.0.attn.out_proj.bias'])


@pytest.mark.parametrize('num_lane', [2, 3, 8, 255, 0])
@pytest.mark.parametrize('torch_ops', [False, True])
def test_a_non_square_num_lane_is_refused_on_every_route(num_lane, torch_ops):
    import graph_detr4d_amd as G
    from graph_detr4d_amd._lib import Gd4dError
    with pytest.raises(Gd4dError, match='perfect square'):
        G.build_head(S.head_config(num_lane=num_lane, torch_ops=torch_ops))


@pytest.mark.parametrize('over', [dict(LID=False), dict(with_multiview=False), dict(with_position=False), dict(normedlinear=True),
                                  dict(depth_num=32)])
def test_uncovered_configurations_are_refused_at_construction(over):
    import graph_detr4d_amd as G
    from graph_detr4d_amd._lib import Gd4dError
    with pytest.raises(Gd4dError, match='torch_ops=True'):
        G.build_head(S.head_config(**over))
    if 'normedlinear' not in over:                                        # the explicit choice builds (and has the lane half)
        head = G.build_head(S.head_config(torch_ops=True, **over))
        assert ('position_encoder.0.weight' in head.state_dict()) == over.get('with_position', True)
        assert 'lane_branches.0.0.weight' in head.state_dict()


def test_train_mode_and_autograd_are_refused_on_the_kernel_route(monkeypatch):
    import graph_detr4d_amd as G
    from graph_detr4d_amd import functional as Fn
    from graph_detr4d_amd._lib import Gd4dError
    monkeypatch.setattr(Fn, 'require_gpu', lambda t, name: None)          # (the refusals come before any kernel)
    head = G.build_head(S.head_config())
    feats = [torch.zeros(1, 2, 64, 6, 10)]
    metas = P.img_metas(np.tile(np.eye(4), (2, 2, 1, 1)), P.timestamps())[:1]
    with pytest.raises(Gd4dError, match='torch_ops = True'):             # train mode
        head.train()(feats, metas)
    with pytest.raises(Gd4dError, match='torch_ops = True'):             # eval mode, autograd on (parameters require grad)
        head.eval()(feats, metas)


@pytest.mark.parametrize('torch_ops', [False, True])
def test_loss_refuses_a_batch_above_one_on_every_route(torch_ops):
    import graph_detr4d_amd as G
    from graph_detr4d_amd._lib import Gd4dError
    head = G.build_head(S.head_config(torch_ops=torch_ops))
    preds = dict(all_cls_scores=torch.zeros(2, 2, 40, 10), all_bbox_preds=torch.zeros(2, 2, 40, 10),
                 all_lane_preds=torch.zeros(2, 2, S.NUM_LANE, 768), enc_cls_scores=None, enc_bbox_preds=None)
    with pytest.raises(Gd4dError, match='batch size 2.*batch size 1 only'):
        head.loss([], [], preds, [torch.zeros(S.NUM_LANE, 768)] * 2)
    bare = G.build_head(S.head_config(loss_lane_mask=None))
    preds['all_lane_preds'] = preds['all_lane_preds'][:, :1]
    with pytest.raises(Gd4dError, match='loss_lane_mask'):
        bare.loss([], [], preds, [torch.zeros(S.NUM_LANE, 768)])


def test_the_criterion_stays_out_of_the_state_dict(golden):
    import graph_detr4d_amd as G
    assigner = dict(type='HungarianAssigner3D', cls_cost=dict(type='FocalLossCost', weight=2.0),
                    reg_cost=dict(type='BBox3DL1Cost', weight=0.25), iou_cost=dict(type='IoUCost', weight=0.0), pc_range=P.PC_RANGE)
    keys, _, _ = _fixture_state(golden)
    head = G.build_head(S.head_config(train_cfg=dict(assigner=assigner)))
    assert isinstance(head.criterion(), G.Detr3DCriterion) and head.criterion() is head.criterion()
    assert set(head.state_dict()) == set(keys) and not any(isinstance(m, G.Detr3DCriterion) for m in head.modules())


def test_get_lane_map_has_no_cpu_detour():
    import graph_detr4d_amd as G
    from graph_detr4d_amd._lib import Gd4dError
    preds = dict(all_lane_preds=torch.zeros(2, 1, S.NUM_LANE, 768))
    with pytest.raises(Gd4dError, match='torch_ops = True'):
        G.build_head(S.head_config()).get_lane_map(preds)
    head = G.build_head(S.head_config(torch_ops=True))                     # the explicit choice: the reference's op sequence
    x, gt = S.map_case(1, 2)
    binary, iou = head.get_lane_map(dict(all_lane_preds=x[None]), gt)
    _, want, _, want_iou = S.lane_map(x, gt)
    assert torch.equal(binary.long(), want) and float((iou.double() - want_iou).abs().max()) < 1e-6
    assert head.get_lane_map(dict(all_lane_preds=x[None]))[1] is None


def test_the_ops_refuse_cpu_tensors_and_bad_shapes():
    from graph_detr4d_amd import _lib, ops
    with pytest.raises(_lib.Gd4dError):
        ops.lane_mask_loss(torch.zeros(1, 2, 4), torch.zeros(2, 4), 1.0)
    with pytest.raises(_lib.Gd4dError):
        ops.lane_map_fwd(torch.zeros(1, 4, 768))
    with pytest.raises(ValueError):
        ops.lane_mask_loss(torch.zeros(1, 2, 4), torch.zeros(2, 5), 1.0)
    with pytest.raises(ValueError):
        ops.lane_map_fwd(torch.zeros(1, 5, 768))
    with pytest.raises(ValueError):
        ops.lane_map_fwd(torch.zeros(1, 4, 512))
    with pytest.raises(ValueError):
        ops.lane_map_fwd(torch.zeros(1, 4, 768), gt_map=torch.zeros(1, 3, 32, 16))


def test_lane_entry_points_validate_before_any_gpu_work(repo_root):
    import re
    from graph_detr4d_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(repo_root, 'include', 'gd4d.h')).read()
    for name in ('gd4d_lane_mask_loss_workspace_bytes', 'gd4d_lane_mask_loss', 'gd4d_lane_map_fwd'):
        assert name in _lib.SIGNATURES and re.search(rf'\b{name}\s*\(', hdr) and hasattr(lib, name)
    assert lib.gd4d_abi_version() == 56                                    # additive exports: the version stays
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 160)()
    ptr = ctypes.c_void_p((ctypes.addressof(buf) + 63) & ~63)
    odd = ctypes.c_void_p(ptr.value + 4)
    EINVAL, EUNSUPPORTED, EALIGN, EWORKSPACE = -1, -2, -3, -5
    # the workspace: L x ceil(R C / 4096) fp64 partials + R row weights, rounded up to 16 bytes; 0 outside the limits
    assert lib.gd4d_lane_mask_loss_workspace_bytes(6, 256, 768) == 6 * 48 * 8 + 256 * 4
    assert lib.gd4d_lane_mask_loss_workspace_bytes(1, 1, 1) == 16
    assert lib.gd4d_lane_mask_loss_workspace_bytes(0, 4, 4) == 0 and lib.gd4d_lane_mask_loss_workspace_bytes(70000, 4, 4) == 0
    loss = lambda logits=ptr, t=ptr, L=1, R=2, C=4, out=ptr, d=ptr, ws=ptr, nb=64: lib.gd4d_lane_mask_loss(      # noqa: E731
        logits, t, 1.0, L, R, C, out, d, ws, nb, null)
    assert loss(logits=null) == EINVAL and loss(t=null) == EINVAL and loss(out=null) == EINVAL and loss(d=null) == EINVAL
    assert loss(L=0) == EINVAL and loss(R=0) == EINVAL and loss(C=-1) == EINVAL
    assert loss(L=70000) == EUNSUPPORTED
    assert loss(ws=null) == EWORKSPACE and loss(nb=8) == EWORKSPACE
    assert loss(ws=odd) == EALIGN
    lane = lambda logits=ptr, gt=null, B=1, g=1, prob=ptr, binary=ptr, sums=null, iou=null: lib.gd4d_lane_map_fwd(     # noqa: E731
        logits, gt, B, g, prob, binary, sums, iou, null)
    assert lane(logits=null) == EINVAL and lane(prob=null) == EINVAL and lane(binary=null) == EINVAL
    assert lane(B=0) == EINVAL and lane(g=0) == EINVAL
    assert lane(gt=ptr) == EINVAL and lane(gt=ptr, sums=ptr) == EINVAL    # sums and iou are required with a ground-truth map
    assert lane(g=4096) == EUNSUPPORTED
    assert lane(logits=odd) == EALIGN and lane(prob=odd) == EALIGN and lane(gt=odd, sums=ptr, iou=ptr) == EALIGN
