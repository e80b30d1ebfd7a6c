"""Feature position embedding (HIP kernels + library 1x1 convs) against the reference-generated fixture and the oracle.
GPU only."""
import numpy as np
import pytest
import torch

from golden_io import Golden
from oracle import torch_oracle as O

pytestmark = pytest.mark.gpu


def _module(g):
    from graph_detr4d_amd import FeaturePositionEmbedding
    m = g.meta
    mod = FeaturePositionEmbedding(embed_dims=256, depth_num=m['depth_num'], depth_start=m['depth_start'],
                                   pc_range=m['pc_range'])
    own = ('position_encoder.', 'adapt_pos3d.', 'fpe.')
    mod.load_state_dict({k: v for k, v in g.state().items() if k.startswith(own)}, strict=True)   # the head's names
    return mod.cuda().eval()


def _metas(g):
    m = g.meta
    return [dict(lidar2img=[g.arrays['lidar2img'][i] for i in range(m['num_cams'])],
                 img_shape=[tuple(s) for s in m['img_shapes']], pad_shape=[tuple(m['pad_shape'])] * m['num_cams'])]


def test_frustum_input_and_mask_match_reference_pieces():
    from graph_detr4d_amd import ops
    import numpy as np
    g = Golden('head_pe')
    m = g.meta
    l2i = g.arrays['lidar2img'][None].astype(np.float64)
    i2l = torch.from_numpy(np.linalg.inv(l2i)).float().view(-1, 4, 4).cuda()
    for lvl, (h, w) in enumerate(m['levels']):
        x, outside = ops.frustum_pe_input_fwd(i2l, (h, w), m['pad_shape'][:2], m['depth_num'], m['depth_start'],
                                              m['pc_range'])
        c3, ref_out = O.frustum_points(l2i, (h, w), m['pad_shape'][:2], m['depth_num'], m['depth_start'], m['pc_range'])
        ref_x = O.inverse_sigmoid(c3.permute(0, 1, 4, 5, 3, 2).contiguous().view(-1, 3 * m['depth_num'], h, w))
        assert torch.equal(outside.cpu(), ref_out.permute(0, 1, 3, 2).reshape(-1, h, w))
        # inverse_sigmoid amplifies fp32 rounding of the coordinate near the clamps; compare where it is well conditioned
        d = (x.cpu() - ref_x).abs()
        assert d[ref_x.abs() < 8].max().item() < 2e-4
        assert (d > 1e-2).float().mean().item() < 1e-3
        mask = g.t(f'mask{lvl}').bool() | outside.view(1, -1, h, w).cpu()
        assert torch.equal(mask, g.t(f'coords_mask{lvl}').bool())


def test_sine_embedding_matches_reference():
    g = Golden('head_pe')
    mod = _module(g)
    for lvl in range(len(g.meta['levels'])):
        got = mod.sine_embedding(g.t(f'mask{lvl}').bool().cuda())
        torch.testing.assert_close(got.cpu(), g.t(f'sine{lvl}'), rtol=0, atol=2e-6)


def test_feature_position_embedding_matches_reference():
    g = Golden('head_pe')
    mod = _module(g)
    feats = [f.cuda() for f in g.feats()]
    with torch.no_grad():                                 # (with autograd on the module takes its training path)
        outs = mod(feats, _metas(g))                      # default: dense part on gd4d_gemm_bf16x3_fwd
        for lvl, o in enumerate(outs):
            torch.testing.assert_close(o.cpu(), g.t(f'out{lvl}'), rtol=2e-4, atol=2e-4)
        import os
        os.environ['GD4D_TORCH_OPS'] = '1'                # the 1x1 convolutions as torch ops
        try:
            for lvl, o in enumerate(mod(feats, _metas(g))):
                torch.testing.assert_close(o.cpu(), g.t(f'out{lvl}'), rtol=2e-4, atol=2e-4)
        finally:
            os.environ.pop('GD4D_TORCH_OPS')
        again = mod(feats, _metas(g))                     # second call: sine branch from the cache
    assert mod._sine_cache is not None
    for a, b in zip(outs, again):
        assert torch.equal(a, b)
    from graph_detr4d_amd._lib import Gd4dError
    with pytest.raises(Gd4dError):
        mod.cpu()([f.cpu() for f in feats], _metas(g))


def test_position_embedding_is_kept_per_camera_and_follows_the_matrices():
    """Inference keeps position_encoder(frustum) per camera, keyed by the camera's img2lidar matrix: a call with some matrices changed
    recomputes those cameras only and equals a fresh module bit for bit; a weight update drops the cache."""
    import copy
    from graph_detr4d_amd import ops
    g = Golden('head_pe')
    mod = _module(g)
    feats = [f.cuda() for f in g.feats()]
    metas = _metas(g)
    rows = []
    real, real_fr = ops.mlp2_bf16x3_fwd, ops.mlp2_frustum_fwd
    ops.mlp2_bf16x3_fwd = lambda x, *a, **k: (rows.append(x.shape[0]), real(x, *a, **k))[1]
    ops.mlp2_frustum_fwd = lambda i2l, shapes, *a, **k: (rows.append(i2l.shape[0] * sum(h * w for h, w in shapes)),
                                                         real_fr(i2l, shapes, *a, **k))[1]
    try:
        with torch.no_grad():
            first = mod(feats, metas)
            same = mod(feats, metas)
            assert len(rows) == 1, 'nothing changed: no camera recomputed'
            for a, b in zip(first, same):
                assert torch.equal(a, b)
            n = feats[0].shape[1]
            moved = copy.deepcopy(metas)
            for cam in (1, n - 1):                                        # two cameras get another pose
                m = np.array(moved[0]['lidar2img'][cam], dtype=np.float64)
                m[:3, 3] += np.array([0.7, -0.4, 0.2]) * (cam + 1)
                moved[0]['lidar2img'][cam] = m
            got = mod(feats, moved)
            s_tot = sum(f.shape[-2] * f.shape[-1] for f in feats)
            assert rows[-1] == 2 * s_tot, 'two cameras recomputed'
            fresh = _module(g)
            want = fresh(feats, moved)
            for a, b in zip(got, want):
                assert torch.equal(a, b)
            assert not torch.equal(got[0][:, 1], first[0][:, 1]) and torch.equal(got[0][:, 0], first[0][:, 0])
            run = copy.deepcopy(moved)                                    # a RUN of cameras: written in place, no scatter
            for cam in (2, 3):
                m = np.array(run[0]['lidar2img'][cam], dtype=np.float64)
                m[:3, 3] -= 0.3 * cam
                run[0]['lidar2img'][cam] = m
            got_run = mod(feats, run)
            assert rows[-1] == 2 * s_tot
            for a, b in zip(got_run, _module(g)(feats, run)):
                assert torch.equal(a, b)
            mod.position_encoder[2].bias.add_(0.5)                        # a weight update: everything is recomputed
            count = len(rows)
            upd = mod(feats, moved)
            assert len(rows) == count + 1 and rows[-1] == n * s_tot * feats[0].shape[0]
            assert not torch.equal(upd[0], got[0])
    finally:
        ops.mlp2_bf16x3_fwd, ops.mlp2_frustum_fwd = real, real_fr


@pytest.mark.parametrize('channels_last_out', [False, True])
def test_a_write_through_data_reaches_every_kept_value_after_invalidate(channels_last_out):
    """p.data.copy_() bumps no version counter: after ops.invalidate_chain_images() the weight splits, the sine branch and the kept
    per-camera embedding are rebuilt, and the output equals a fresh module's with the new weights bit for bit."""
    from graph_detr4d_amd import ops
    g = Golden('head_pe')
    feats = [f.cuda() for f in g.feats()]
    metas = _metas(g)
    mod = _module(g)
    mod.channels_last_out = channels_last_out
    torch.manual_seed(3)
    with torch.no_grad():
        before = mod(feats, metas)
        for p in (mod.position_encoder[0].weight, mod.adapt_pos3d[2].weight, mod.fpe.conv_expand.weight):
            p.data.copy_(torch.randn_like(p) * p.std())
            ops.invalidate_chain_images()
            got = mod(feats, metas)
            fresh = _module(g)
            fresh.load_state_dict(mod.state_dict())
            fresh.channels_last_out = channels_last_out
            for a, b, c in zip(got, fresh(feats, metas), before):
                assert torch.equal(a, b) and not torch.equal(a, c)
            before = got


@pytest.mark.parametrize('levels,r', [([(7, 9), (5, 3), (3, 3)], 3), ([(16, 28), (8, 14), (4, 7), (2, 4)], 2), ([(5, 5)], 1), ([(29, 50), (15, 25)], 5)])
def test_se_gate_and_fuse_as_one_kernel_matches_fp64(levels, r):
    """gd4d_mlp2_se_fuse_fwd on level sizes that put camera / level boundaries inside its groups of 4 pixels and its 128-row tiles (odd
    pixel counts per camera): out = feat + (pe * sigmoid(relu(feat W1^T + b1) W2^T + b2) + sine) against fp64, channels-last levels out."""
    from graph_detr4d_amd import ops
    torch.manual_seed(len(levels) * 10 + r)
    feats = [torch.randn(r, 256, h, w, device='cuda') for h, w in levels]
    s_tot = sum(h * w for h, w in levels)
    w1, b1 = torch.randn(256, 256, device='cuda') / 16, torch.randn(256, device='cuda')
    w2, b2 = torch.randn(256, 256, device='cuda') / 16, torch.randn(256, device='cuda')
    pe, sine = torch.randn(r, s_tot, 256, device='cuda'), torch.randn(r, s_tot, 256, device='cuda')
    outs = ops.mlp2_se_fuse_fwd(feats, ops.mlp2_image(w1, b1, w2), b2, pe, sine)
    again = ops.mlp2_se_fuse_fwd(feats, ops.mlp2_image(w1, b1, w2), b2, pe, sine)
    st = 0
    for f, o, o2 in zip(feats, outs, again):
        hw = f.shape[2] * f.shape[3]
        assert o.shape == f.shape and ops.PyramidView.is_channels_last_level(o) and torch.equal(o, o2)
        x = f.double().flatten(2).transpose(1, 2)                                       # (R, HW, C)
        gate = torch.relu(x @ w1.double().t() + b1.double()) @ w2.double().t() + b2.double()
        want = x + (pe[:, st:st + hw].double() * torch.sigmoid(gate) + sine[:, st:st + hw].double())
        got = o.permute(0, 2, 3, 1).reshape(r, hw, 256).double()
        assert (got - want).abs().max().item() < 2e-4 * max(1.0, want.abs().max().item())
        st += hw


def test_channels_last_output_holds_the_same_bits_and_is_gathered_in_place():
    """FeaturePositionEmbedding(channels_last_out=True): the (B, N, C, H, W) results equal the default's (1e-5) and the reference's
    fixture, their memory is (B, N, H, W, C), and the cross-attention reads them in place (no slice-planar copy) with the same output."""
    from graph_detr4d_amd import ops
    import graph_detr4d_amd as G
    g = Golden('head_pe')
    mod = _module(g)
    feats = [f.cuda() for f in g.feats()]
    with torch.no_grad():
        want = mod(feats, _metas(g))
        mod.channels_last_out = True
        got = mod(feats, _metas(g))
    for lvl, (a, b) in enumerate(zip(got, want)):
        # (the gate's two convolutions run in another kernel on this route - gd4d_mlp2_se_fuse_fwd: the same split-bf16 products,
        #  another summation order)
        assert a.shape == b.shape
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(a.cpu(), g.t(f'out{lvl}'), rtol=2e-4, atol=2e-4)
        assert ops.PyramidView.is_channels_last_level(a) and not ops.PyramidView.is_channels_last_level(b)
    fused = []
    real_se = ops.mlp2_se_fuse_fwd
    ops.mlp2_se_fuse_fwd = lambda *a, **k: (fused.append(1), real_se(*a, **k))[1]
    try:
        with torch.no_grad():
            again = mod(feats, _metas(g))
    finally:
        ops.mlp2_se_fuse_fwd = real_se
    assert fused and all(torch.equal(a, b) for a, b in zip(again, got)), 'one kernel for gate + fuse, run-to-run identical'
    copies = []
    real = ops.pyramid_slice_planar_fwd
    ops.pyramid_slice_planar_fwd = lambda *a, **k: (copies.append(1), real(*a, **k))[1]
    try:
        n = feats[0].shape[1]
        attn = G.build_attention(dict(type='Deform3DCrossAttn', num_cams=n, pc_range=g.meta['pc_range'], num_points=4, embed_dims=256,
                                      num_levels=len(feats))).cuda().eval()
        torch.manual_seed(0)
        q, b = 50, feats[0].shape[0]
        query, pos = torch.randn(q, b, 256, device='cuda'), torch.randn(q, b, 256, device='cuda')
        ref = torch.rand(b, q, 3, device='cuda')
        metas = _metas(g)
        with torch.no_grad():
            o_cl = attn(query, None, got, query_pos=pos, reference_points=ref, img_metas=metas)
            assert not copies, 'channels-last levels are gathered in place'
            o_nchw = attn(query, None, want, query_pos=pos, reference_points=ref, img_metas=metas)
            assert copies
    finally:
        ops.pyramid_slice_planar_fwd = real
    torch.testing.assert_close(o_cl, o_nchw, rtol=2e-5, atol=2e-5)


@pytest.mark.parametrize('route', ['hip', 'torch'])
def test_feature_position_embedding_trains(route, monkeypatch):
    """With autograd on, the stage equals the inference path and its gradients - to the feature maps (the backbone's),
    the two position MLPs and the SE gate - equal autograd of the oracle (a restatement of detr3d_head_pe.py:525-557).
    hip: forward and backward on the library's own kernels (_HeadPEFunction); torch: the 1x1 convolutions as torch ops."""
    import numpy as np
    from graph_detr4d_amd import head_pe, ops
    if route == 'torch':
        monkeypatch.setenv('GD4D_TORCH_OPS', '1')
    calls = []
    real = ops.gemm_tn_bf16x3
    monkeypatch.setattr(ops, 'gemm_tn_bf16x3', lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    g = Golden('head_pe')
    m = g.meta
    mod = _module(g)
    with torch.no_grad():
        want_out = mod([f.cuda() for f in g.feats()], _metas(g))
    feats = [f.cuda().requires_grad_() for f in g.feats()]
    outs = mod(feats, _metas(g))
    for o, w in zip(outs, want_out):
        torch.testing.assert_close(o, w, rtol=2e-4, atol=2e-4)
    gen = torch.Generator().manual_seed(3)
    probes = [torch.randn(o.shape, generator=gen) for o in outs]
    sum((o * p.cuda()).sum() for o, p in zip(outs, probes)).backward()
    # oracle, CPU autograd
    params = {k: v.clone().requires_grad_() for k, v in g.state().items() if k.startswith(('position_encoder.', 'adapt_pos3d.', 'fpe.'))}
    feats_c = [f.clone().requires_grad_() for f in g.feats()]
    l2i = torch.from_numpy(g.arrays['lidar2img'][None].astype(np.float64))
    o_outs, _ = O.feature_position_embedding(params, feats_c, l2i, [[tuple(s) for s in m['img_shapes']]], tuple(m['pad_shape']),
                                             m['depth_num'], m['depth_start'], m['pc_range'])
    sum((o * p).sum() for o, p in zip(o_outs, probes)).backward()
    for fg, fc in zip(feats, feats_c):
        torch.testing.assert_close(fg.grad.cpu(), fc.grad, rtol=1e-3, atol=1e-4)
    for name, prm in mod.named_parameters():
        want = params[name].grad
        assert prm.grad is not None, name
        tol = 2e-3 * max(1.0, want.abs().max().item())
        assert (prm.grad.cpu() - want).abs().max().item() < tol, name
    assert len(calls) == (5 if route == 'hip' else 0)          # the five weight gradients that are GEMMs over pixels


def test_head_pe_second_backward_is_refused():
    g = Golden('head_pe')
    mod = _module(g)
    feats = [f.cuda().requires_grad_() for f in g.feats()]
    loss = sum(o.sum() for o in mod(feats, _metas(g)))
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match='consumed'):
        loss.backward()


@pytest.mark.parametrize('rows,m,n,relu_b', [(1000, 256, 1024, False), (4099, 1024, 192, False), (777, 256, 256, True),
                                               (15, 128, 64, False), (70000, 1024, 384, False)])
def test_gemm_tn_bf16x3_matches_fp64(rows, m, n, relu_b):
    """C = A^T B and the column sums of A against fp64; ragged row counts (tail of 16, empty splits), every (M, N) the head
    uses; the same bits on a second run (fixed summation order)."""
    from graph_detr4d_amd import ops
    gen = torch.Generator().manual_seed(rows)
    a = torch.randn(rows, m, generator=gen).cuda()
    b = torch.randn(rows, n, generator=gen).cuda()
    c, col = ops.gemm_tn_bf16x3(a, b, relu_b=relu_b)
    bb = b.double().clamp_min(0) if relu_b else b.double()
    want = a.double().t() @ bb
    scale = (a.double().abs().t() @ bb.abs()).max().item()
    assert (c.double() - want).abs().max().item() < 1.5e-5 * scale          # 2^-16 per product (dropped lo x lo term)
    torch.testing.assert_close(col.double(), a.double().sum(0), rtol=1e-5, atol=1e-4 * rows ** 0.5)
    c2, col2 = ops.gemm_tn_bf16x3(a, b, relu_b=relu_b)
    assert torch.equal(c, c2) and torch.equal(col, col2)
    c3, none = ops.gemm_tn_bf16x3(a, b, relu_b=relu_b, want_colsum=False)
    assert none is None and torch.equal(c, c3)


def test_gemm_tn_rejects_unsupported_shapes():
    from graph_detr4d_amd import ops, _lib
    a, b = torch.randn(64, 100).cuda(), torch.randn(64, 64).cuda()
    with pytest.raises(_lib.Gd4dError):
        ops.gemm_tn_bf16x3(a, b)
    with pytest.raises(ValueError):
        ops.gemm_tn_bf16x3(torch.randn(64, 128).cuda(), torch.randn(63, 64).cuda())


def test_gemm_mask_out_is_the_gradient_at_a_relu():
    from graph_detr4d_amd import ops
    torch.manual_seed(5)
    dy, w = torch.randn(300, 256).cuda(), torch.randn(256, 1024).cuda() * 0.1          # y = h W^T, W (256, 1024)
    h = torch.relu(torch.randn(300, 1024)).cuda()
    want = (dy.double() @ w.double()) * (h > 0)
    got = h.clone()
    ops.gemm_bf16x3_fwd(dy, *ops.split_bf16_fwd(w.t().contiguous()), out=got, mask_out=True)
    torch.testing.assert_close(got.double(), want, rtol=1e-4, atol=1e-4)
    assert ((got == 0) | (h > 0)).all()
    with pytest.raises(ValueError):
        ops.gemm_bf16x3_fwd(dy, *ops.split_bf16_fwd(w.t().contiguous()), mask_out=True)


def test_se_fuse_chlast_bwd_equals_autograd():
    from graph_detr4d_amd import ops
    torch.manual_seed(1)
    r, c, sizes = 3, 256, [(9, 4), (5, 7)]
    s_tot = sum(h * w for h, w in sizes)
    gate, pe = (torch.randn(r, s_tot, c).cuda().requires_grad_() for _ in range(2))
    gouts = [torch.randn(r, c, h, w).cuda() for h, w in sizes]
    start, loss = 0, 0
    for (h, w), go in zip(sizes, gouts):
        sl = slice(start, start + h * w)
        val = (pe[:, sl] * torch.sigmoid(gate[:, sl])).transpose(1, 2).reshape(r, c, h, w)
        loss = loss + (val * go).sum()
        start += h * w
    loss.backward()
    g_buf, p_buf, ds = gate.detach().clone(), pe.detach().clone(), torch.empty(r, s_tot, c).cuda()
    start = 0
    for (h, w), go in zip(sizes, gouts):
        ops.se_fuse_chlast_bwd(go, g_buf, p_buf, ds, start)
        torch.testing.assert_close(ds[:, start:start + h * w], go.flatten(2).transpose(1, 2))
        start += h * w
    torch.testing.assert_close(g_buf, gate.grad, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(p_buf, pe.grad, rtol=1e-5, atol=1e-6)


def test_se_fuse_equals_torch():
    from graph_detr4d_amd import ops
    torch.manual_seed(0)
    f, g_, pe, s = (torch.randn(3, 256, 9, 4).cuda() for _ in range(4))
    got = ops.se_fuse_fwd(f, g_, pe, s)
    torch.testing.assert_close(got, f + (pe * torch.sigmoid(g_) + s), rtol=1e-6, atol=1e-6)


def test_head_outputs_match_reference_forward():
    """functional.head_outputs (cls / reg branches on the HIP linears + gd4d_box_head_fwd) against what the reference's
    Detr3DHeadPE.forward returned for the same decoder outputs."""
    import torch.nn as nn
    from graph_detr4d_amd import functional as Fn
    g = Golden('head_pe')
    m, sd = g.meta, g.state()
    nl = m['num_layers']

    def cls():
        return nn.Sequential(nn.Linear(256, 256), nn.LayerNorm(256), nn.ReLU(inplace=True),
                             nn.Linear(256, 256), nn.LayerNorm(256), nn.ReLU(inplace=True), nn.Linear(256, 10))

    def reg():
        return nn.Sequential(nn.Linear(256, 256), nn.ReLU(), nn.Linear(256, 256), nn.ReLU(), nn.Linear(256, 10))
    cls_b, reg_b = nn.ModuleList(cls() for _ in range(nl)), nn.ModuleList(reg() for _ in range(nl))
    cls_b.load_state_dict({k[len('cls_branches.'):]: v for k, v in sd.items() if k.startswith('cls_branches.')})
    reg_b.load_state_dict({k[len('reg_branches.'):]: v for k, v in sd.items() if k.startswith('reg_branches.')})
    cls_b.cuda().eval(), reg_b.cuda().eval()
    with torch.no_grad():
        got = Fn.head_outputs(g.t('hs').cuda(), g.t('init_reference').cuda(), g.t('inter_references').cuda(), cls_b,
                              reg_b, m['pc_range'])
    torch.testing.assert_close(got['all_cls_scores'].cpu(), g.t('all_cls_scores'), rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(got['all_bbox_preds'].cpu(), g.t('all_bbox_preds'), rtol=1e-4, atol=1e-4)


def test_with_detach_cuts_the_gradient_of_level_0_past_frames():
    """detr3d_head_pe.py:512-516 (`with_detach`, default True): level 0's cameras after the first six reach the stage
    detached - same outputs, no gradient to the backbone through them; every other (level, camera) keeps its gradient.
    with_detach=False restores it."""
    from graph_detr4d_amd import FeaturePositionEmbedding, synthetic
    img_hw, levels, n = (64, 112), [(8, 14), (4, 7)], 12
    rig = synthetic.camera_rig(2, img_hw)
    metas = synthetic.make_img_metas(rig, img_shape=(img_hw[0], img_hw[1], 3), pad_shape=(img_hw[0], img_hw[1], 3))
    gen = torch.Generator().manual_seed(5)
    base = [torch.randn(1, n, 256, h, w, generator=gen) for h, w in levels]
    probes = [torch.randn(1, n, 256, h, w, generator=gen).cuda() for h, w in levels]
    res = {}
    for detach in (True, False):
        mod = FeaturePositionEmbedding(pc_range=synthetic.PC_RANGE, with_detach=detach)
        synthetic.randomise_all_(mod, seed=9, std=0.04)
        mod = mod.cuda().eval()
        feats = [f.cuda().requires_grad_() for f in base]
        outs = mod(feats, metas)
        sum((o * p).sum() for o, p in zip(outs, probes)).backward()
        res[detach] = ([o.detach() for o in outs], [f.grad for f in feats])
    for a, b in zip(res[True][0], res[False][0]):
        assert torch.equal(a, b)                                        # values do not change
    g_det, g_full = res[True][1], res[False][1]
    assert float(g_det[0][:, 6:].abs().max()) == 0.0 and float(g_full[0][:, 6:].abs().max()) > 0
    assert torch.equal(g_det[0][:, :6], g_full[0][:, :6]) and torch.equal(g_det[1], g_full[1])
    assert FeaturePositionEmbedding(pc_range=synthetic.PC_RANGE).with_detach is True      # the head's default (:326)


@pytest.mark.parametrize('m,k1,h', [(1000, 192, 1024), (257, 192, 1024), (31, 64, 64), (4096, 256, 256), (300, 16, 32)])
def test_fused_two_layer_mlp_matches_fp64(m, k1, h):
    """gd4d_mlp2_bf16x3_fwd (relu(x W1^T + b1) W2^T + b2 with the hidden activation kept in registers) against fp64, at the
    position_encoder's shape (192 -> 1024 -> 256), the SE layer's (256 -> 256 -> 256), ragged row counts and the smallest shapes;
    within split-bf16 x 3 rounding of both products (the same bound as two gd4d_gemm_bf16x3_fwd calls); run-to-run identical."""
    from graph_detr4d_amd import ops
    torch.manual_seed(m + k1)
    x = torch.randn(m, k1)
    w1, b1 = torch.randn(h, k1) / k1 ** 0.5, torch.randn(h) * 0.1
    w2, b2 = torch.randn(256, h) / h ** 0.5, torch.randn(256) * 0.1
    want = (torch.relu(x.double() @ w1.double().t() + b1.double()) @ w2.double().t() + b2.double()).float()
    img = ops.mlp2_image(w1.cuda(), b1.cuda(), w2.cuda())
    got = ops.mlp2_bf16x3_fwd(x.cuda(), img, b2.cuda())
    torch.testing.assert_close(got.cpu(), want, rtol=2e-4, atol=2e-4)
    assert torch.equal(ops.mlp2_bf16x3_fwd(x.cuda(), img, b2.cuda()), got)
    hid = ops.gemm_bf16x3_fwd(x.cuda(), *ops.split_bf16_fwd(w1.cuda()), b1.cuda(), relu=True) if (h % 256 == 0 and k1 % 32 == 0) else None
    if hid is not None:                                  # ... and as close to fp64 as the two-GEMM route is
        two = ops.gemm_bf16x3_fwd(hid, *ops.split_bf16_fwd(w2.cuda()), b2.cuda())
        assert (got.cpu() - want).abs().max() <= 2 * (two.cpu() - want).abs().max() + 1e-6


@pytest.mark.parametrize('levels,r', [([(7, 9), (5, 3), (3, 3)], 3), ([(16, 28), (8, 14), (4, 7), (2, 4)], 6), ([(5, 5)], 1), ([(29, 50), (15, 25)], 5)])
def test_frustum_inputs_generated_inside_the_mlp_equal_the_two_kernels(levels, r):
    """gd4d_mlp2_frustum_fwd (the frustum coordinates generated in the MLP's prologue, no (R, S, 192) tensor) against
    gd4d_frustum_pe_input_fwd -> gd4d_mlp2_bf16x3_fwd: the same inputs operation for operation, the first product summed in another
    order (1e-4), and against fp64 on the frustum kernel's inputs (2e-4: the MLP's own bound); level sizes that put camera and level
    boundaries inside a 128-row tile; run-to-run identical; the rows of `out=` views."""
    from graph_detr4d_amd import ops, synthetic
    torch.manual_seed(len(levels) + r)
    rig = synthetic.camera_rig((r + 5) // 6)[:r].astype(np.float64)
    i2l = torch.from_numpy(np.linalg.inv(rig).astype(np.float32)).cuda()
    pad_hw = (928, 1600)
    w1, b1 = torch.randn(1024, 192) / 192 ** 0.5, torch.randn(1024) * 0.1
    w2, b2 = torch.randn(256, 1024) / 32, torch.randn(256) * 0.1
    s_tot = sum(h * w for h, w in levels)
    x = torch.empty(r, s_tot, 192, device='cuda')
    st = 0
    for h, w in levels:
        ops.frustum_pe_input_fwd(i2l, (h, w), pad_hw, 64, 1.0, synthetic.PC_RANGE, out=x, row_start=st)
        st += h * w
    two = ops.mlp2_bf16x3_fwd(x.view(r * s_tot, -1), ops.mlp2_image(w1.cuda(), b1.cuda(), w2.cuda()), b2.cuda()).view(r, s_tot, 256)
    img = ops.mlp2_frustum_image(w1.cuda(), b1.cuda(), w2.cuda())
    got = ops.mlp2_frustum_fwd(i2l, levels, pad_hw, 64, 1.0, synthetic.PC_RANGE, img, b2.cuda())
    assert got.shape == (r, s_tot, 256)
    torch.testing.assert_close(got, two, rtol=1e-5, atol=1e-4)
    want = (torch.relu(x.cpu().double().view(-1, 192) @ w1.double().t() + b1.double()) @ w2.double().t() + b2.double()).float()
    torch.testing.assert_close(got.cpu().view(-1, 256), want, rtol=2e-4, atol=2e-4)
    assert torch.equal(ops.mlp2_frustum_fwd(i2l, levels, pad_hw, 64, 1.0, synthetic.PC_RANGE, img, b2.cuda()), got)
    if r > 2:                                                     # a run of cameras written into their rows of a kept tensor
        kept = torch.full((r, s_tot, 256), float('nan'), device='cuda')
        ops.mlp2_frustum_fwd(i2l[1:3], levels, pad_hw, 64, 1.0, synthetic.PC_RANGE, img, b2.cuda(), out=kept[1:3])
        assert torch.equal(kept[1:3], got[1:3]) and torch.isnan(kept[0]).all()


@pytest.mark.parametrize('levels,r', [([(7, 9), (5, 3), (3, 3)], 3), ([(16, 28), (8, 14), (4, 7), (2, 4)], 6), ([(5, 5)], 1), ([(29, 50), (15, 25)], 5)])
def test_both_mlps_and_the_fuse_as_one_kernel_equal_the_two_kernels(levels, r):
    """gd4d_mlp2_pe_se_fwd (position_encoder(frustum) kept in registers while the SE gate's MLP runs, then the fuse) against
    gd4d_mlp2_frustum_fwd -> gd4d_mlp2_se_fuse_fwd: the same operations on the same operands - bit for bit, outputs and the optionally
    stored embedding; level sizes with camera / level boundaries inside tiles and groups; written into `outs` views."""
    from graph_detr4d_amd import ops, synthetic
    torch.manual_seed(len(levels) * 7 + r)
    rig = synthetic.camera_rig((r + 5) // 6)[:r].astype(np.float64)
    i2l = torch.from_numpy(np.linalg.inv(rig).astype(np.float32)).cuda()
    pad_hw = (928, 1600)
    w1, b1 = (torch.randn(1024, 192) / 192 ** 0.5).cuda(), (torch.randn(1024) * 0.1).cuda()
    w2, b2 = (torch.randn(256, 1024) / 32).cuda(), (torch.randn(256) * 0.1).cuda()
    v1, c1 = (torch.randn(256, 256) / 16).cuda(), (torch.randn(256) * 0.1).cuda()
    v2, c2 = (torch.randn(256, 256) / 16).cuda(), (torch.randn(256) * 0.1).cuda()
    feats = [torch.randn(r, 256, h, w).cuda() for h, w in levels]
    s_tot = sum(h * w for h, w in levels)
    sine = torch.randn(r, s_tot, 256).cuda()
    pe_img, se_img = ops.mlp2_frustum_image(w1, b1, w2), ops.mlp2_image(v1, c1, v2)
    pe = ops.mlp2_frustum_fwd(i2l, levels, pad_hw, 64, 1.0, synthetic.PC_RANGE, pe_img, b2)
    want = ops.mlp2_se_fuse_fwd(feats, se_img, c2, pe, sine)
    kept = torch.full_like(pe, float('nan'))
    got = ops.mlp2_pe_se_fwd(i2l, feats, pad_hw, 64, 1.0, synthetic.PC_RANGE, pe_img, b2, se_img, c2, sine, pe_out=kept)
    assert torch.equal(kept, pe)
    for a, b in zip(got, want):
        assert a.shape == b.shape and torch.equal(a, b)
    if r > 2:                                                     # a run of cameras, written into their rows of whole-rig outputs
        outs = [torch.full((r, h, w, 256), float('nan'), device='cuda') for h, w in levels]
        ops.mlp2_pe_se_fwd(i2l[1:3], [f[1:3] for f in feats], pad_hw, 64, 1.0, synthetic.PC_RANGE, pe_img, b2, se_img, c2, sine[1:3],
                           outs=[o[1:3] for o in outs])
        for o, b in zip(outs, want):
            assert torch.equal(o[1:3].permute(0, 3, 1, 2), b[1:3]) and torch.isnan(o[0]).all()


def test_cameras_that_keep_moving_go_through_one_kernel_and_nothing_is_lost(monkeypatch):
    """channels_last_out route: a camera whose matrix changed between the last two calls AND changes again is computed by
    gd4d_mlp2_pe_se_fwd (its embedding is not stored, its kept rows are stale); when it stops moving its rows are recomputed into the
    kept tensor once and then reused.  Every call equals a fresh module's output bit for bit; cache_position_embedding = False sends
    every camera through the one kernel."""
    import copy
    from graph_detr4d_amd import ops
    for name in ('GD4D_PE_FUSED', 'GD4D_PE_FRUSTUM'):             # (the default routes, whatever the caller's environment says)
        monkeypatch.delenv(name, raising=False)
    g = Golden('head_pe')
    feats = [f.cuda() for f in g.feats()]
    metas = _metas(g)
    n = feats[0].shape[1]
    s_tot = sum(f.shape[-2] * f.shape[-1] for f in feats)

    def module(keep=True):
        m = _module(g)
        m.channels_last_out, m.cache_position_embedding = True, keep
        return m

    def moved(step):
        mt = copy.deepcopy(metas)
        for cam in range(2, n):                                           # the "past frames": every camera from the third on
            m = np.array(mt[0]['lidar2img'][cam], dtype=np.float64)
            m[:3, 3] += np.array([0.5, -0.3, 0.1]) * step * (cam + 1)
            mt[0]['lidar2img'][cam] = m
        return mt

    calls = {'one': [], 'mlp': [], 'se': []}
    real = (ops.mlp2_pe_se_fwd, ops.mlp2_frustum_fwd, ops.mlp2_se_fuse_fwd)
    ops.mlp2_pe_se_fwd = lambda i2l, *a, **k: (calls['one'].append(i2l.shape[0]), real[0](i2l, *a, **k))[1]
    ops.mlp2_frustum_fwd = lambda i2l, *a, **k: (calls['mlp'].append(i2l.shape[0]), real[1](i2l, *a, **k))[1]
    ops.mlp2_se_fuse_fwd = lambda fl, *a, **k: (calls['se'].append(fl[0].shape[0]), real[2](fl, *a, **k))[1]

    def last():
        res = {k: list(v) for k, v in calls.items()}
        for v in calls.values():
            v.clear()
        return res
    try:
        with torch.no_grad():
            mod = module()
            want = {}
            for step in (0, 1, 2, 3):
                want[step] = [o.clone() for o in module()(feats, moved(step))]
            last()
            out0 = mod(feats, moved(0))
            assert last() == {'one': [], 'mlp': [n], 'se': [n]}            # first call: everything computed and kept
            out1 = mod(feats, moved(1))
            assert last() == {'one': [], 'mlp': [n - 2], 'se': [n]}        # first move: recomputed into the kept tensor
            out2 = mod(feats, moved(2))
            assert last() == {'one': [n - 2], 'mlp': [], 'se': [2]}        # moving: one kernel, nothing stored
            out3 = mod(feats, moved(3))
            assert last() == {'one': [n - 2], 'mlp': [], 'se': [2]}
            again = mod(feats, moved(3))                                   # stopped: stale rows recomputed into the kept tensor ...
            assert last() == {'one': [], 'mlp': [n - 2], 'se': [n]}
            still = mod(feats, moved(3))                                   # ... and reused
            assert last() == {'one': [], 'mlp': [], 'se': [n]}
            for got, step in ((out0, 0), (out1, 1), (out2, 2), (out3, 3), (again, 3), (still, 3)):
                for a, b in zip(got, want[step]):
                    assert ops.PyramidView.is_channels_last_level(a) and torch.equal(a, b)
            nokeep = module(keep=False)
            for step in (1, 2):
                got = nokeep(feats, moved(step))
                assert last() == {'one': [n], 'mlp': [], 'se': []}
                for a, b in zip(got, want[step]):
                    assert torch.equal(a, b)
            assert s_tot > 0
    finally:
        ops.mlp2_pe_se_fwd, ops.mlp2_frustum_fwd, ops.mlp2_se_fuse_fwd = real


def test_one_kernel_route_at_the_bench_size_equals_the_two_kernel_route(monkeypatch):
    """24 cameras on the R50 pyramid (739 800 pixels - the size bench.py's features_to_boxes runs): every camera through
    gd4d_mlp2_pe_se_fwd (cache_position_embedding = False) against the position MLP + SE gate / fuse kernels (GD4D_PE_FUSED=0) and
    against the module with its frustum tensor written and read (GD4D_PE_FRUSTUM=0): bit for bit / within the first product's
    summation order; the 5 780 tiles cross every camera and level boundary."""
    from graph_detr4d_amd import FeaturePositionEmbedding, ops, synthetic
    torch.manual_seed(5)
    n = 24
    rig = synthetic.camera_rig(4)
    metas = synthetic.make_img_metas(rig, batch=1)
    feats = [torch.randn(1, n, 256, h, w, device='cuda') * 0.5 for h, w in synthetic.R50_LEVELS]

    def run():
        mod = FeaturePositionEmbedding(pc_range=synthetic.PC_RANGE, channels_last_out=True)
        synthetic.randomise_all_(mod, seed=11, std=0.04)
        mod = mod.cuda().eval()
        mod.cache_position_embedding = False
        with torch.no_grad():
            return [o.clone() for o in mod(feats, metas)]
    for name in ('GD4D_PE_FUSED', 'GD4D_PE_FRUSTUM'):
        monkeypatch.delenv(name, raising=False)
    seen = []
    real = ops.mlp2_pe_se_fwd
    monkeypatch.setattr(ops, 'mlp2_pe_se_fwd', lambda i2l, *a, **k: (seen.append(i2l.shape[0]), real(i2l, *a, **k))[1])
    one = run()
    assert seen == [n]
    monkeypatch.setenv('GD4D_PE_FUSED', '0')
    two = run()
    assert seen == [n]
    for a, b in zip(one, two):
        assert ops.PyramidView.is_channels_last_level(a) and torch.equal(a, b)
    monkeypatch.setenv('GD4D_PE_FRUSTUM', '0')
    plain = run()
    for a, b in zip(one, plain):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=2e-4)
        assert (a - b).abs().mean().item() < 2e-6


@pytest.mark.parametrize('channels_last', [False, True])
def test_kept_embedding_across_streams_static_rig_and_updates(channels_last, monkeypatch):
    """(channels_last: the route with the one-kernel form for moving cameras, _forward_one_kernel - camera 1 alternates between two
    poses, so it is stored, then computed without being stored, then found stale.)
    The kept per-camera embedding is safe across streams: a call on another stream that finds every matrix unchanged (static rig)
    only READS the tensor - it must come after the stream that wrote it; an in-place update must come after every stream still
    reading it; a key change drops the tensor while readers may be queued.  Stress: two streams alternate calls (same rig, moved
    rig, weight update) with a long kernel queued in front of the writer each time; every result equals a fresh module's."""
    import copy
    for name in ('GD4D_PE_FUSED', 'GD4D_PE_FRUSTUM'):
        monkeypatch.delenv(name, raising=False)
    g = Golden('head_pe')

    def fresh():
        m = _module(g)
        m.channels_last_out = channels_last
        return m
    mod = fresh()
    feats = [f.cuda() for f in g.feats()]
    metas = _metas(g)
    moved = copy.deepcopy(metas)
    m = np.array(moved[0]['lidar2img'][1], dtype=np.float64)
    m[:3, 3] += np.array([0.9, -0.5, 0.3])
    moved[0]['lidar2img'][1] = m
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    big = torch.randn(4096, 4096, device='cuda')

    def busy(stream):                                             # ~ms of work queued on `stream` before the next call on it
        with torch.cuda.stream(stream):
            for _ in range(6):
                big @ big
    with torch.no_grad():
        want_static = [t.clone() for t in fresh()(feats, metas)]
        want_moved = [t.clone() for t in fresh()(feats, moved)]
        torch.cuda.synchronize()
        for rnd in range(4):
            busy(s1)
            with torch.cuda.stream(s1):
                a = mod(feats, metas if rnd % 2 == 0 else moved)     # writer: (re)computes or updates in place, behind the busy work
            with torch.cuda.stream(s2):
                b = mod(feats, metas if rnd % 2 == 0 else moved)     # reader on another stream: finds "unchanged" at once
            busy(s2)
            with torch.cuda.stream(s2):
                c = mod(feats, metas if rnd % 2 == 0 else moved)
            torch.cuda.synchronize()
            want = want_static if rnd % 2 == 0 else want_moved
            for got in (a, b, c):
                for x, y in zip(got, want):
                    assert torch.equal(x, y), rnd
        mod.train()
        assert mod._pe_cache is None and mod._split_cache is None    # a mode change drops the inference caches
        mod.eval()
