"""The FPN neck on the library's kernels (gd4d_fpn.hip, gd4d_fpn_conv_fwd) against the fp64 restatement (fpn_ref.py), the modules' own
torch-op route and the reference fixture; the bit-for-bit properties of the fused forms.  GPU only.

Shapes: N = 2 cameras; levels (13, 21), (7, 11), (4, 6) - ratios that are not 2, 273 pixels = four 64-pixel tiles and a tail that
crosses image rows, ragged 16 x 16 tiles with a second tile in x.  Tolerances: 1e-4 of the map's largest |entry| per kernel, 2e-4 per
module; fp32 storage of the fp64 reference is far below both."""
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import fpn_ref as R
from golden_io import Golden

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
N = 2
LEVELS = [(13, 21), (7, 11), (4, 6)]
KERNEL_TOL, MODULE_TOL = 1e-4, 2e-4


def _rand(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


@functools.lru_cache(maxsize=None)
def _lateral_case(in_channels):
    """Inputs, weights and the fp64 laterals (top-down adds included) of one pyramid; computed once."""
    xs = [_rand(N, c, h, w, seed=10 + i) for i, (c, (h, w)) in enumerate(zip(in_channels, LEVELS))]
    ws = [_rand(256, c, seed=20 + i, scale=c ** -0.5) for i, c in enumerate(in_channels)]
    bs = [_rand(256, seed=30 + i, scale=0.1) for i in range(len(in_channels))]
    lats = [None] * len(xs)
    for i in range(len(xs) - 1, -1, -1):
        lats[i] = R.lateral(xs[i], ws[i], bs[i], lats[i + 1] if i + 1 < len(xs) else None)
    return xs, ws, bs, lats


@functools.lru_cache(maxsize=None)
def _conv_case():
    xs = [_rand(N, 256, h, w, seed=40 + i) for i, (h, w) in enumerate(LEVELS)]
    ws = [_rand(256, 256, 3, 3, seed=50 + i, scale=2304 ** -0.5) for i in range(len(LEVELS))]
    bs = [_rand(256, seed=60 + i, scale=0.1) for i in range(len(LEVELS))]
    return xs, ws, bs, [R.conv3x3(x, w, b) for x, w, b in zip(xs, ws, bs)]


def _run_laterals(ops, xs, ws, bs, fused=True, channels_last=False):
    imgs = [ops.fpn_lateral_image(w.to(DEV)) for w in ws]
    lats = [None] * len(xs)
    for i in range(len(xs) - 1, -1, -1):
        up = lats[i + 1] if i + 1 < len(xs) else None
        lats[i] = ops.fpn_lateral_fwd(xs[i].to(DEV), imgs[i], bs[i].to(DEV), up=up if fused else None, channels_last_out=channels_last)
        if up is not None and not fused:
            lats[i] = lats[i] + F.interpolate(up, size=lats[i].shape[2:], mode='nearest')
    return lats


# ---- 1. kernel level ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('in_channels', [(64, 96, 160), (64, 96, 128)])       # start_level = 0; [32, 64, 96, 128] from start_level = 1
def test_lateral_kernel_against_fp64(in_channels):
    from graph_detr4d_amd import ops
    xs, ws, bs, ref = _lateral_case(in_channels)
    got = _run_laterals(ops, xs, ws, bs)
    for lvl, (g, r) in enumerate(zip(got, ref)):
        err = R.rel_err(g, r)
        print(f'lateral {in_channels} level {lvl}: {err:.2e}')
        assert g.shape == r.shape and err <= KERNEL_TOL


def test_lateral_kernel_long_k_walk():
    """Cin = 2048 on the (4, 6) level alone: 64 chunks through the double-buffered stage."""
    from graph_detr4d_amd import ops
    x, w, b = _rand(N, 2048, 4, 6, seed=70), _rand(256, 2048, seed=71, scale=2048 ** -0.5), _rand(256, seed=72, scale=0.1)
    got = ops.fpn_lateral_fwd(x.to(DEV), ops.fpn_lateral_image(w.to(DEV)), b.to(DEV))
    err = R.rel_err(got, R.lateral(x, w, b))
    print(f'lateral Cin = 2048: {err:.2e}')
    assert err <= KERNEL_TOL


def test_conv_kernel_per_level_weights_against_fp64():
    from graph_detr4d_amd import ops
    xs, ws, bs, ref = _conv_case()
    got = ops.fpn_conv_fwd([x.to(DEV) for x in xs], [ops.depth_net_image(w.to(DEV)) for w in ws], [b.to(DEV) for b in bs])
    for lvl, (g, r) in enumerate(zip(got, ref)):
        err = R.rel_err(g, r)
        print(f'conv3x3 level {lvl}: {err:.2e}')
        assert err <= KERNEL_TOL


@pytest.mark.parametrize('hw, relu_in', [((4, 6), False), ((2, 3), True), ((5, 7), False), ((13, 21), True)])
def test_extra_conv_kernel_against_fp64(hw, relu_in):
    """(4, 6) -> (2, 3); (2, 3) -> (1, 2) with the ReLU on read; an odd input (5, 7) -> (3, 4); (13, 21) -> (7, 11): a second tile."""
    from graph_detr4d_amd import ops
    x, w, b = _rand(N, 256, *hw, seed=80), _rand(256, 256, 3, 3, seed=81, scale=2304 ** -0.5), _rand(256, seed=82, scale=0.1)
    ref = R.conv3x3(x, w, b, stride=2, relu_in=relu_in)
    img = ops.depth_net_image(w.to(DEV))
    got = ops.fpn_extra_conv_fwd(x.to(DEV), img, b.to(DEV), relu_in=relu_in)
    assert tuple(got.shape) == (N, 256, (hw[0] + 1) // 2, (hw[1] + 1) // 2) == tuple(ref.shape)
    err = R.rel_err(got, ref)
    print(f'extra conv {hw} relu_in={relu_in}: {err:.2e}')
    assert err <= KERNEL_TOL
    # channels-last in and out: the same arithmetic on the same values
    x_cl = x.to(DEV).contiguous(memory_format=torch.channels_last)
    got_cl = ops.fpn_extra_conv_fwd(x_cl, img, b.to(DEV), relu_in=relu_in, channels_last_out=True)
    assert got_cl.permute(0, 2, 3, 1).is_contiguous() and torch.equal(got_cl, got)


# ---- 2. module level ------------------------------------------------------------------------------------------------------
FPN_CFG = dict(type='FPN', in_channels=[32, 64, 96, 128], out_channels=256, start_level=1, add_extra_convs='on_output', num_outs=5,
               relu_before_extra_convs=True)
CPFPN_CFG = dict(type='CPFPN', in_channels=[64, 96, 160], out_channels=256, start_level=0, add_extra_convs='on_output', num_outs=3,
                 relu_before_extra_convs=True)


def _module(cfg, seed=5, **kw):
    import graph_detr4d_amd as G
    torch.manual_seed(seed)
    mod = G.build_neck(dict(cfg, **kw))
    with torch.no_grad():
        for p in mod.parameters():
            if p.dim() == 1:
                p.copy_(_rand(*p.shape, seed=seed + 1, scale=0.1))
    return mod.to(DEV).eval()


def _inputs(cfg, seed=90):
    s = cfg['start_level']
    hw = [(26, 42)] * s + LEVELS                                              # (levels below start_level are not read)
    return [_rand(N, c, *hw[i], seed=seed + i) for i, c in enumerate(cfg['in_channels'])]


@pytest.mark.parametrize('cfg', [FPN_CFG, CPFPN_CFG], ids=['FPN', 'CPFPN'])
def test_module_against_its_torch_route_and_fp64(cfg):
    mod = _module(cfg)
    xs = _inputs(cfg)
    sd = {k: v.cpu() for k, v in mod.state_dict().items()}
    _, ref = R.fpn_forward(sd, xs, start_level=cfg['start_level'], num_outs=cfg['num_outs'], relu_before_extra_convs=True,
                           cp=cfg['type'] == 'CPFPN')
    with torch.no_grad():
        got = mod([x.to(DEV) for x in xs])
        mod.torch_ops = True
        tor = mod([x.to(DEV) for x in xs])
    assert len(got) == len(tor) == len(ref) == cfg['num_outs']
    for lvl, (g, t, r) in enumerate(zip(got, tor, ref)):
        e64, etor = R.rel_err(g, r), R.rel_err(g, t.cpu())
        print(f'{cfg["type"]} out {lvl} {tuple(g.shape)}: vs fp64 {e64:.2e}, vs torch route {etor:.2e}')
        assert g.shape == r.shape and e64 <= MODULE_TOL and etor <= MODULE_TOL


def test_cpfpn_against_the_reference_fixture():
    import graph_detr4d_amd as G
    g = Golden('fpn_cp')
    m = g.meta
    mod = G.CPFPN(**m['cfg'])
    mod.load_state_dict(g.state(), strict=True)
    mod = mod.to(DEV).eval()
    with torch.no_grad():
        outs = mod([g.t(f'in{i}').float().div(m['feat_scale']).to(DEV) for i in range(len(m['cfg']['in_channels']))])
    assert len(outs) == m['cfg']['num_outs']
    cs = m['chan_stride']
    for lvl, o in enumerate(outs):
        ref = g.t(f'out{lvl}')
        o = o.cpu()[:, ::cs] if lvl == 0 else o.cpu()                            # (the fixture keeps every cs-th channel of level 0)
        err = float((o - ref).abs().max() / ref.abs().max())
        print(f'CPFPN fixture out {lvl}: {err:.2e}')
        assert o.shape == ref.shape and err <= MODULE_TOL


# ---- 3. bit for bit -------------------------------------------------------------------------------------------------------
def test_fused_top_down_add_is_torchs_add_bit_for_bit():
    from graph_detr4d_amd import ops
    xs, ws, bs, _ = _lateral_case((64, 96, 160))
    fused = _run_laterals(ops, xs, ws, bs, fused=True)
    plain = _run_laterals(ops, xs, ws, bs, fused=False)
    for a, b in zip(fused, plain):
        assert torch.equal(a, b)


def test_one_launch_over_levels_is_one_launch_per_level_bit_for_bit():
    from graph_detr4d_amd import ops
    xs, ws, bs, _ = _conv_case()
    xs, bs = [x.to(DEV) for x in xs], [b.to(DEV) for b in bs]
    imgs = [ops.depth_net_image(w.to(DEV)) for w in ws]
    together = ops.fpn_conv_fwd(xs, imgs, bs)
    for x, img, b, t in zip(xs, imgs, bs, together):
        assert torch.equal(ops.fpn_conv_fwd([x], [img], [b])[0], t)
        assert torch.equal(ops.depth_conv_raw([x], img, b)[0], t)              # ... and the existing single-image entry point's bits


def test_channels_last_outputs_are_the_nchw_outputs_permuted():
    from graph_detr4d_amd import ops
    xs, ws, bs, _ = _lateral_case((64, 96, 160))
    for a, b in zip(_run_laterals(ops, xs, ws, bs), _run_laterals(ops, xs, ws, bs, channels_last=True)):
        assert a.is_contiguous() and b.permute(0, 2, 3, 1).is_contiguous() and torch.equal(a, b)
    cx, cw, cb, _ = _conv_case()
    cx, cb = [x.to(DEV) for x in cx], [b.to(DEV) for b in cb]
    imgs = [ops.depth_net_image(w.to(DEV)) for w in cw]
    for a, b in zip(ops.fpn_conv_fwd(cx, imgs, cb), ops.fpn_conv_fwd(cx, imgs, cb, channels_last_out=True)):
        assert b.permute(0, 2, 3, 1).is_contiguous() and torch.equal(a, b)
    for cfg in (FPN_CFG, CPFPN_CFG):
        xs = [x.to(DEV) for x in _inputs(cfg)]
        with torch.no_grad():
            nchw, cl = _module(cfg)(xs), _module(cfg, channels_last_out=True)(xs)
        for a, b in zip(nchw, cl):
            assert a.is_contiguous() and b.permute(0, 2, 3, 1).is_contiguous() and torch.equal(a, b)


def test_two_runs_give_the_same_bits():
    mod = _module(FPN_CFG)
    xs = [x.to(DEV) for x in _inputs(FPN_CFG)]
    with torch.no_grad():
        a = [o.clone() for o in mod(xs)]
        b = mod(xs)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


@pytest.mark.parametrize('cfg', [FPN_CFG, CPFPN_CFG], ids=['FPN', 'CPFPN'])
def test_graph_replay_on_new_inputs_and_after_a_weight_edit(cfg):
    """A hipGraph captured on inputs A and replayed on inputs B equals the eager call on B; after an in-place weight edit,
    refresh_images() (outside the graph) makes the replay show the new weights - the images keep their addresses."""
    from graph_detr4d_amd import functional as Fn
    mod = _module(cfg, channels_last_out=True)
    a, b = [x.to(DEV) for x in _inputs(cfg, seed=90)], [x.to(DEV) for x in _inputs(cfg, seed=190)]
    static = [x.clone() for x in a]
    with torch.no_grad(), Fn.request_slot(3):
        mod(static)                                                          # eager once: images and kept buffers exist
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode='thread_local'):
            outs = mod(static)
        for s, x in zip(static, b):
            s.copy_(x)
        graph.replay()
        eager = mod(b)
        for u, v in zip(outs, eager):
            assert torch.equal(u, v)
        before = [o.clone() for o in outs]
        for p in mod.parameters():
            p.mul_(0.5)                                                      # in place: the version counters move
        mod.refresh_images()
        graph.replay()
        eager = mod(b)
        for u, v in zip(outs, eager):
            assert torch.equal(u, v)
        assert not any(torch.equal(u, v) for u, v in zip(outs, before))      # (the edit is visible in every level)
    torch.cuda.synchronize()


# ---- 4. handing on to the decoder --------------------------------------------------------------------------------------
class _StubBackbone(nn.Module):
    """Four maps at strides 4 / 8 / 16 / 32 by average pooling and channel tiling: enough of a backbone for the plumbing."""

    def __init__(self, channels):
        super().__init__()
        self.channels = channels

    def forward(self, x):
        outs = []
        for i, c in enumerate(self.channels):
            f = F.avg_pool2d(x, 4 * 2 ** i, ceil_mode=True)
            outs.append(f.repeat(1, (c + 2) // 3, 1, 1)[:, :c].contiguous())
        return outs


def test_extractor_hands_channels_last_levels_to_the_decoder_in_place():
    from graph_detr4d_amd import ops
    from graph_detr4d_amd.plumbing import ImageFeatureExtractor
    neck = _module(dict(FPN_CFG, num_outs=4), channels_last_out=True)
    ext = ImageFeatureExtractor(_StubBackbone(FPN_CFG['in_channels']), neck, channels_last=True).to(DEV).eval()
    img = _rand(1, N, 3, 104, 168, seed=7).to(DEV)                             # strides 8 / 16 / 32: (13, 21), (7, 11), (4, 6)
    written = []
    hook = neck.register_forward_hook(lambda m, i, o: written.append([t.data_ptr() for t in o]))
    with torch.no_grad():
        levels = ext(img, [dict()])
        direct = neck(ext.img_backbone(img[0]))
    hook.remove()
    assert [tuple(f.shape) for f in levels] == [(1, N, 256, 13, 21), (1, N, 256, 7, 11), (1, N, 256, 4, 6), (1, N, 256, 2, 3)]
    assert all(ops.PyramidView.is_channels_last_level(f) for f in levels)
    view = ops.PyramidView.channels_last_levels(levels)                        # raises unless every level can be gathered in place
    assert view.ptrs == written[0] and view.rows == N                          # the memory the neck's kernels wrote: no copy since
    for f, d in zip(levels, direct):
        assert torch.equal(f[0], d)
