"""Camera-aware DepthNet (gd4d_depth_net.hip) against the reference fixture, an fp64 restatement at the bench's shape and the module's
own torch-op route.  GPU only."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from golden_io import Golden, sub
from test_depth_net_cpu import restated_gate

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
R50 = [(116, 200), (58, 100), (29, 50), (15, 25)]


def _fixture_module(g):
    from graph_detr4d_amd import DepthNet
    mod = DepthNet(256, 256, 80)
    mod.load_state_dict(sub(g.state(), 'depth_net.'), strict=True)
    return mod.to(DEV).eval()


def _fixture_metas(g):
    m = g.meta
    n = m['num_cams']
    return [dict(lidar2img=[g.arrays['lidar2img'][i] for i in range(n)], img_shape=[tuple(s) for s in m['img_shapes']],
                 pad_shape=[tuple(m['pad_shape'])] * n, intrinsics=[g.arrays['intrinsics'][i] for i in range(n)],
                 ida_mats=[g.t('ida')])]


def _fpe(g, channels_last_out=False):
    from graph_detr4d_amd import FeaturePositionEmbedding
    m = g.meta
    mod = FeaturePositionEmbedding(embed_dims=256, depth_num=m['depth_num'], depth_start=m['depth_start'], pc_range=m['pc_range'],
                                   channels_last_out=channels_last_out)
    own = ('position_encoder.', 'adapt_pos3d.', 'fpe.')
    mod.load_state_dict({k: v for k, v in g.state().items() if k.startswith(own)}, strict=True)
    return mod.to(DEV).eval()


def test_depth_net_matches_reference_fixture():
    """(a) forward per level (the reference's own call) and forward_levels against depth{l}; DepthNet -> FeaturePositionEmbedding
    (NCHW and channels-last out) against the head's hand-over out{l}."""
    g = Golden('head_pe_cam')
    mod = _fixture_module(g)
    metas = _fixture_metas(g)
    feats = [f.to(DEV) for f in g.feats()]
    mats = dict(intrin_mats=metas[0]['intrinsics'], ida_mats=metas[0]['ida_mats'])
    with torch.no_grad():
        per_level = [mod(f, mats) for f in feats]
        levels = mod.forward_levels(feats, metas)
        for lvl, (a, b) in enumerate(zip(per_level, levels)):
            ref = g.t(f'depth{lvl}')
            assert a.shape == ref.shape and b.shape == (1,) + tuple(ref.shape)
            torch.testing.assert_close(a.cpu(), ref, rtol=2e-4, atol=2e-4)
            torch.testing.assert_close(b[0].cpu(), ref, rtol=2e-4, atol=2e-4)
            assert torch.equal(a, b[0])                                    # one launch or one per level: the same arithmetic
        for cl in (False, True):
            outs = _fpe(g, channels_last_out=cl)(levels, metas)
            for lvl, o in enumerate(outs):
                torch.testing.assert_close(o.cpu(), g.t(f'out{lvl}'), rtol=2e-4, atol=2e-4)


def _random_module(seed, channels=256):
    from graph_detr4d_amd import DepthNet
    torch.manual_seed(seed)
    mod = DepthNet(channels, channels, 80)
    bn = mod.reduce_conv[1]
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(channels) * 0.3)
        bn.running_var.copy_(0.25 + 2 * torch.rand(channels))
        bn.weight.copy_(1 + 0.2 * torch.randn(channels))
        bn.bias.copy_(0.2 * torch.randn(channels))
        mod.reduce_conv[0].bias.copy_(0.1 * torch.randn(channels))
        for p in list(mod.mlp.parameters()) + list(mod.se.parameters()):
            p.copy_(torch.randn(p.shape) * 0.06)
    return mod.to(DEV).eval()


def _rig_metas(n, seed, ida_per_camera=False):
    from graph_detr4d_amd import synthetic
    rng = np.random.default_rng(seed)
    k = synthetic.camera_intrinsics(n // 6, (928, 1600))
    k[:, 0, 0] *= rng.uniform(0.8, 1.2, n).astype(np.float32)
    k[:, 1, 1] *= rng.uniform(0.8, 1.2, n).astype(np.float32)
    scales = rng.uniform(0.4, 1.1, n if ida_per_camera else 1)
    ida = [torch.tensor([[s, 0., -20.], [0., s, -40.], [0., 0., 1.]], dtype=torch.float32) for s in scales]
    return [dict(intrinsics=[k[i] for i in range(n)], ida_mats=ida)]


def _gate64(mod, metas):
    sd = {k: v.detach().double().cpu() for k, v in mod.state_dict().items()}
    intr = torch.from_numpy(np.stack(metas[0]['intrinsics'])).double()
    ida = torch.stack(metas[0]['ida_mats']).double()
    return restated_gate(sd, intr, ida)


def _samples(n, h, w, count, gen):
    """(camera, y, x) indices: every camera's four corners and points on each of its four borders, the rest random."""
    idx = []
    for c in range(n):
        for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):
            idx.append((c, y, x))
        for t in torch.randint(0, max(1, w), (6,), generator=gen).tolist():
            idx += [(c, 0, t), (c, h - 1, t)]
        for t in torch.randint(0, max(1, h), (6,), generator=gen).tolist():
            idx += [(c, t, 0), (c, t, w - 1)]
    rest = max(0, count - len(idx))
    idx += list(zip(torch.randint(0, n, (rest,), generator=gen).tolist(), torch.randint(0, h, (rest,), generator=gen).tolist(),
                    torch.randint(0, w, (rest,), generator=gen).tolist()))
    return torch.tensor(idx)


def _fp64_at(mod, x, gate64, idx):
    """relu(BN(conv3x3(x) + b)) * gate at the sampled (camera, y, x), in fp64."""
    sd = {k: v.detach().double() for k, v in mod.state_dict().items()}
    xp = F.pad(x, (1, 1, 1, 1))
    c, y, xx = idx[:, 0].to(x.device), idx[:, 1].to(x.device), idx[:, 2].to(x.device)
    taps = [xp[c, :, y + dy, xx + dx] for dy in range(3) for dx in range(3)]          # 9 x (S, 256)
    patch = torch.stack(taps, -1).double()                                         # (S, 256, 9)
    w = sd['reduce_conv.0.weight'].reshape(256, 256, 9)
    v = torch.einsum('sik,oik->so', patch, w) + sd['reduce_conv.0.bias']
    v = (v - sd['reduce_conv.1.running_mean']) / torch.sqrt(sd['reduce_conv.1.running_var'] + mod.reduce_conv[1].eps)
    v = v * sd['reduce_conv.1.weight'] + sd['reduce_conv.1.bias']
    return F.relu(v) * gate64.to(x.device)[idx[:, 0].to(x.device)]


def test_r50_pyramid_24_cameras_against_fp64_and_torch_route():
    """(b) 24 cameras x the R50 pyramid, random weights and BN statistics: >= 4096 sampled output pixels per level (every camera's
    borders and corners among them) within 2e-4 x max|ref| of an fp64 restatement; the whole tensor against the torch-op route."""
    n = 24
    mod = _random_module(5)
    metas = _rig_metas(n, 5)
    gen = torch.Generator().manual_seed(5)
    feats = [torch.randn(1, n, 256, h, w, generator=gen).to(DEV) for h, w in R50]
    gate64 = _gate64(mod, metas)
    with torch.no_grad():
        outs = mod.forward_levels(feats, metas)
        for f, o in zip(feats, outs):
            h, w = f.shape[-2:]
            idx = _samples(n, h, w, 4096, gen)
            assert len(idx) >= 4096
            ref = _fp64_at(mod, f[0], gate64, idx)
            got = o[0][idx[:, 0], :, idx[:, 1], idx[:, 2]].double()
            err = float((got - ref).abs().max())
            assert err <= 2e-4 * float(ref.abs().max()), (tuple(f.shape), err, float(ref.abs().max()))
        mod.torch_ops = True
        try:
            torch_outs = mod.forward_levels(feats, metas)
        finally:
            mod.torch_ops = False
        for o, t in zip(outs, torch_outs):
            assert float((o - t).abs().max()) <= 2e-4 * float(t.abs().max())


def test_ida_list_of_one_or_n_gives_the_reference_gate():
    """(c) the pipeline's single ida matrix broadcasts over the cameras; N matrices give each camera its own scale."""
    from graph_detr4d_amd import ops
    n = 12
    mod = _random_module(7)
    gen = torch.Generator().manual_seed(7)
    feats = [torch.randn(1, n, 256, h, w, generator=gen).to(DEV) for h, w in [(11, 19), (6, 10)]]
    with torch.no_grad():
        for per_cam in (False, True):
            metas = _rig_metas(n, 7 + per_cam, ida_per_camera=per_cam)
            assert len(metas[0]['ida_mats']) == (n if per_cam else 1)
            ref = _gate64(mod, metas).float()
            k_dev, ida_dev = mod.refresh_matrices(metas, DEV)
            fc1, fc2, cr, ce = mod.mlp.fc1, mod.mlp.fc2, mod.se.conv_reduce, mod.se.conv_expand
            ws = (fc1.weight, fc1.bias, fc2.weight, fc2.bias, cr.weight, cr.bias, ce.weight, ce.bias)
            assert ida_dev.shape == (n,)                                   # the module's buffer: one scale per camera either way
            torch.testing.assert_close(ops.cam_gate_fwd(k_dev, ida_dev, *ws).cpu(), ref, rtol=1e-5, atol=1e-5)
            if not per_cam:                                                # the kernel's broadcast of a single scale
                torch.testing.assert_close(ops.cam_gate_fwd(k_dev, ida_dev[:1], *ws).cpu(), ref, rtol=1e-5, atol=1e-5)
            assert float(ref.max() - ref.min()) > 0.05
            outs = mod.forward_levels(feats, metas)
            mod.torch_ops = True
            try:
                t_outs = mod.forward_levels(feats, metas)
            finally:
                mod.torch_ops = False
            for o, t in zip(outs, t_outs):
                assert float((o - t).abs().max()) <= 2e-4 * float(t.abs().max())
        one = _rig_metas(n, 9)
        many = [dict(intrinsics=one[0]['intrinsics'], ida_mats=one[0]['ida_mats'] * n)]
        for a, b in zip(mod.forward_levels(feats, one), mod.forward_levels(feats, many)):
            assert torch.equal(a, b)


def test_graph_captured_on_a_serves_b_after_refresh_matrices():
    """(d) a hipGraph captured on sample A, replayed after refresh_matrices(B), equals an eager call on B bit for bit."""
    from graph_detr4d_amd import functional as Fn
    n = 12
    mod = _random_module(11)
    gen = torch.Generator().manual_seed(11)
    feats = [torch.randn(1, n, 256, h, w, generator=gen).to(DEV) for h, w in [(29, 50), (15, 25), (8, 13), (4, 7)]]
    meta_a, meta_b = _rig_metas(n, 11), _rig_metas(n, 12, ida_per_camera=True)
    with torch.no_grad():
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s), Fn.request_slot(3):
            mod.forward_levels(feats, meta_a)                              # eager first: matrices and image on the device
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode='thread_local'), Fn.request_slot(3):
            captured = mod.forward_levels(feats, meta_a)
        graph.replay()
        torch.cuda.synchronize()
        with Fn.request_slot(99):
            eager_a = mod.forward_levels(feats, meta_a)
            eager_b = mod.forward_levels(feats, meta_b)
        for a, e in zip(captured, eager_a):
            assert torch.equal(a, e)
        with Fn.request_slot(3):
            mod.refresh_matrices(meta_b, DEV)
        graph.replay()
        torch.cuda.synchronize()
        for a, e, e_a in zip(captured, eager_b, eager_a):
            assert torch.equal(a, e)
            assert not torch.equal(e, e_a)                                 # B's cameras differ from A's


def _small_capture_case(seed):
    """One level, 2 cameras, a 17 x 18 map: 2 x 2 tiles of 16 x 16, ragged on both edges.  (module, metas, inputs A, inputs B)."""
    mod = _random_module(seed)
    six = _rig_metas(6, seed)[0]
    metas = [dict(intrinsics=six['intrinsics'][:2], ida_mats=six['ida_mats'])]
    gen = torch.Generator().manual_seed(seed)
    a, b = (torch.randn(1, 2, 256, 17, 18, generator=gen).to(DEV) for _ in range(2))
    return mod, metas, a, b


def test_graph_replay_follows_refresh_images_at_the_same_address():
    """A hipGraph captured on inputs A and replayed on inputs B equals the eager call on B; after an in-place weight edit,
    refresh_images() (outside the graph) makes the replay show the new weight - the image keeps its address."""
    from graph_detr4d_amd import functional as Fn
    mod, metas, a, b = _small_capture_case(21)
    static = a.clone()
    with torch.no_grad(), Fn.request_slot(3):
        mod.forward_levels([static], metas)                                # eager once: matrices and image on the device
        torch.cuda.synchronize()
        address = mod._image().data_ptr()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode='thread_local'):
            out, = mod.forward_levels([static], metas)
        static.copy_(b)
        graph.replay()
        eager, = mod.forward_levels([b], metas)
        assert torch.equal(out, eager)
        before = out.clone()
        mod.reduce_conv[0].weight.mul_(0.5)                                # in place: the version counter moves
        mod.refresh_images()
        graph.replay()
        eager, = mod.forward_levels([b], metas)
        assert torch.equal(out, eager) and not torch.equal(out, before)
        assert mod._image().data_ptr() == address
    torch.cuda.synchronize()


def test_a_stale_image_is_refused_under_capture():
    """After an in-place weight edit without refresh_images(), a capture raises instead of re-imaging inside the graph; a later eager
    call works (and re-images)."""
    from graph_detr4d_amd import functional as Fn
    mod, metas, a, _ = _small_capture_case(22)
    with torch.no_grad(), Fn.request_slot(3):
        first, = mod.forward_levels([a], metas)
        mod.reduce_conv[0].weight.mul_(0.5)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with pytest.raises(RuntimeError, match='once eagerly'):
            with torch.cuda.graph(graph, capture_error_mode='thread_local'):
                mod.forward_levels([a], metas)
        torch.cuda.synchronize()
        second, = mod.forward_levels([a], metas)
        assert torch.isfinite(second).all() and not torch.equal(first, second)
    torch.cuda.synchronize()


def test_output_follows_new_weights():
    """(e) load_state_dict, or an in-place change of a parameter: the next call uses the new weights."""
    n = 6
    mod = _random_module(13)
    other = _random_module(14)
    metas = _rig_metas(n, 13)
    gen = torch.Generator().manual_seed(13)
    feats = [torch.randn(1, n, 256, h, w, generator=gen).to(DEV) for h, w in [(20, 33), (10, 17)]]

    def both():
        with torch.no_grad():
            hip = mod.forward_levels(feats, metas)
            mod.torch_ops = True
            try:
                ref = mod.forward_levels(feats, metas)
            finally:
                mod.torch_ops = False
        for o, t in zip(hip, ref):
            assert float((o - t).abs().max()) <= 2e-4 * float(t.abs().max())
        return hip
    first = both()
    mod.load_state_dict(other.state_dict(), strict=True)
    second = both()
    with torch.no_grad():
        mod.reduce_conv[0].weight.mul_(-0.5)
    third = both()
    with torch.no_grad():
        mod.se.conv_expand.bias.add_(0.5)
        mod.reduce_conv[1].running_mean.add_(0.1)
    fourth = both()
    for a, b, c, d in zip(first, second, third, fourth):
        assert not torch.equal(a, b) and not torch.equal(b, c) and not torch.equal(c, d)


def test_a_write_through_data_reaches_the_weight_image_after_invalidate():
    """p.data.copy_() bumps no version counter: after ops.invalidate_chain_images() the 3x3 weight's image is rebuilt and the output
    equals a fresh module's with the new weight bit for bit."""
    from graph_detr4d_amd import ops
    n = 6
    mod = _random_module(13)
    metas = _rig_metas(n, 13)
    gen = torch.Generator().manual_seed(13)
    feats = [torch.randn(1, n, 256, h, w, generator=gen).to(DEV) for h, w in [(20, 33), (10, 17)]]
    with torch.no_grad():
        before = mod.forward_levels(feats, metas)
        mod.reduce_conv[0].weight.data.copy_(_random_module(14).reduce_conv[0].weight)
        ops.invalidate_chain_images()
        got = mod.forward_levels(feats, metas)
        fresh = _random_module(13)
        fresh.load_state_dict(mod.state_dict())
        for a, b, c in zip(got, fresh.forward_levels(feats, metas), before):
            assert torch.equal(a, b) and not torch.equal(a, c)


def test_training_needs_the_torch_route():
    """(f) train() without torch_ops raises; with torch_ops=True the module is the reference arithmetic with batch statistics and
    gradients reach every parameter the reference's forward uses (context_conv's output is discarded there too)."""
    from graph_detr4d_amd import DepthNet
    from graph_detr4d_amd._lib import Gd4dError
    n = 6
    mod = _random_module(17).train()
    metas = _rig_metas(n, 17)
    gen = torch.Generator().manual_seed(17)
    feats = [torch.randn(1, n, 256, h, w, generator=gen).to(DEV) for h, w in [(12, 20), (6, 10)]]
    with pytest.raises(Gd4dError, match='torch_ops'):
        mod.forward_levels(feats, metas)
    with torch.no_grad(), pytest.raises(Gd4dError, match='torch_ops'):
        mod.forward_levels(feats, metas)
    mod.eval()
    with pytest.raises(Gd4dError, match='torch_ops'):                     # eval, but autograd on: no HIP backward
        mod.forward_levels(feats, metas)
    sd = {k: v.detach().clone() for k, v in mod.state_dict().items()}
    tmod = DepthNet(256, 256, 80, torch_ops=True).to(DEV).train()
    tmod.load_state_dict(sd, strict=True)
    xs = [f.clone().requires_grad_(True) for f in feats]
    outs = tmod.forward_levels(xs, metas)
    gate = restated_gate({k: v.cpu() for k, v in sd.items()}, torch.from_numpy(np.stack(metas[0]['intrinsics'])),
                         torch.stack(metas[0]['ida_mats'])).to(DEV)
    bn_mean, bn_var = sd['reduce_conv.1.running_mean'].clone(), sd['reduce_conv.1.running_var'].clone()
    for f, o in zip(feats, outs):
        y = F.conv2d(f[0], sd['reduce_conv.0.weight'], sd['reduce_conv.0.bias'], padding=1)
        y = F.batch_norm(y, bn_mean.clone(), bn_var.clone(), sd['reduce_conv.1.weight'], sd['reduce_conv.1.bias'], training=True)
        torch.testing.assert_close(o[0], F.relu(y) * gate[:, :, None, None], rtol=2e-4, atol=2e-4)
    sum((o * o).sum() for o in outs).backward()
    for name, p in tmod.named_parameters():
        if name.startswith('context_conv.'):
            assert p.grad is None
        else:
            assert p.grad is not None and float(p.grad.abs().sum()) > 0, name
    assert all(x.grad is not None for x in xs)
    assert not torch.equal(tmod.reduce_conv[1].running_mean, sd['reduce_conv.1.running_mean'])   # batch statistics were taken


def test_unsupported_shapes_raise():
    """(g) channels other than 256 or fp64 maps raise and name the torch-op route."""
    from graph_detr4d_amd import DepthNet
    from graph_detr4d_amd._lib import Gd4dError
    metas = _rig_metas(6, 19)
    small = DepthNet(128, 128, 80).to(DEV).eval()
    with torch.no_grad():
        with pytest.raises(Gd4dError, match='torch_ops'):
            small.forward_levels([torch.randn(1, 6, 128, 8, 8, device=DEV)], metas)
        mod = _random_module(19)
        with pytest.raises(Gd4dError, match='torch_ops'):
            mod.forward_levels([torch.randn(1, 6, 256, 8, 8, device=DEV, dtype=torch.float64)], metas)
        small.torch_ops = True                                              # chosen: the torch layers serve it
        out = small.forward_levels([torch.randn(1, 6, 128, 8, 8, device=DEV)], metas)
        assert out[0].shape == (1, 6, 128, 8, 8)
        assert math.isfinite(float(out[0].sum()))
    assert os.environ.get('GD4D_TORCH_OPS') != '1'
