"""VoVNet on the library's kernels (gd4d_vovnet.hip) against the fp64 restatement (vovnet_ref.py), the reference's recorded maps
(tests/golden/vovnet_tiny.npz) and the modules' own torch-op route; the bit-for-bit properties (two runs, a captured graph).  GPU only.

Shapes: N = 2 images throughout.  13 x 21 is two pixel tiles in y (8 rows) and in x (16 columns), both ragged; 5 x 7 is one ragged tile;
26 x 37 -> 13 x 19 and 5 x 7 -> 3 x 4 are the even and odd stride-2 sizes.  The library picks the M tiling from the channel and the
tile count; at these sizes that is one row block per workgroup, so every case also runs with each of the six tilings (1, 2, 3, 4, 5, 7
row blocks) that divides its channel count forced - 32, 64, 192, 128 / 256, 160, 224 reach all six - and must give the same bits.  (1024, 224) and the 2144-channel aggregation are stage 5's own shapes.
Tolerances: 1e-4 of the map's largest |entry| per kernel, 2e-4 per module, accumulated linearly over the OSA modules for a
whole network.  The function is continuous: no entry is excluded."""
import ctypes
import functools

import pytest
import torch

import vovnet_ref as R
from golden_io import Golden

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
N = 2
KERNEL_TOL, MODULE_TOL = 1e-4, 2e-4
FEATS = ('stem', 'stage2', 'stage3', 'stage4', 'stage5')
# (cin, cout, stride, h, w)
CONV_CASES = [(64, 64, 1, 13, 21), (64, 128, 2, 26, 37), (128, 128, 1, 5, 7), (256, 160, 1, 13, 21), (160, 160, 1, 5, 7),
              (224, 224, 1, 13, 21), (512, 192, 1, 5, 7), (768, 224, 1, 5, 7), (32, 32, 2, 5, 7), (1024, 224, 1, 5, 7)]
# (source channels, cout, h, w, the first source is a slice of a larger buffer)
OSA_CASES = [((128,) * 6, 256, 13, 21, False), ((256,) + (160,) * 5, 512, 13, 21, True), ((512,) + (192,) * 5, 768, 5, 7, False),
             ((768,) + (224,) * 5, 1024, 5, 7, False), ((64,), 32, 5, 7, False), ((1024,) + (224,) * 5, 1024, 5, 7, False)]


def _rand(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _tilings(cout):
    return [mt for mt in (1, 2, 3, 4, 5, 7) if (cout // 32) % mt == 0]


def _scale_shift(c, seed):
    return 1.5 + 0.1 * _rand(c, seed=seed), _rand(c, seed=seed + 1, scale=0.5)


# ---- 1. kernels ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _conv_case(cin, cout, stride, h, w):
    x = _rand(N, cin, h, w, seed=1)
    weight = _rand(cout, cin, 3, 3, seed=2, scale=(9 * cin) ** -0.5)
    scale, shift = _scale_shift(cout, 3)
    return x, weight, scale, shift, R.folded_conv_relu(x, weight, scale, shift, stride)


@pytest.mark.parametrize('case', CONV_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_conv3x3_bn_relu_against_fp64(case):
    from graph_detr4d_amd import ops
    cin, cout, stride, h, w = case
    x, weight, scale, shift, ref = _conv_case(*case)
    image = ops.conv3x3_image(weight.to(DEV))
    run = lambda: ops.conv3x3_bn_relu(x.to(DEV), image, cout, scale.to(DEV), shift.to(DEV), stride=stride)
    out = run()
    torch.cuda.synchronize()
    assert tuple(out.shape) == tuple(ref.shape) == (N, cout, (h - 1) // stride + 1, (w - 1) // stride + 1)
    err = R.rel_err(out, ref)
    zeros = float((ref == 0).double().mean())
    print(f'conv3x3_bn_relu {case}: rel_err {err:.3e}, {zeros:.2f} of the outputs are 0')
    assert zeros > 0.2                                                      # the ReLU is exercised
    assert err <= KERNEL_TOL
    assert torch.equal(out, run())                                          # no atomics: two runs give the same bits
    for mt in _tilings(cout):                                               # ... and so does every M tiling
        assert torch.equal(out, ops.conv3x3_bn_relu(x.to(DEV), image, cout, scale.to(DEV), shift.to(DEV), stride=stride, m_blocks=mt)), mt


@functools.lru_cache(maxsize=None)
def _osa_case(chans, cout, h, w):
    srcs = [_rand(N, c, h, w, seed=10 + i) for i, c in enumerate(chans)]
    k = sum(chans)
    weight = _rand(cout, k, 1, 1, seed=20, scale=k ** -0.5)
    scale, shift = _scale_shift(cout, 21)
    ref = R.folded_conv_relu(torch.cat(srcs, dim=1), weight, scale, shift)
    return srcs, weight, scale, shift, ref


@pytest.mark.parametrize('case', OSA_CASES, ids=lambda c: f'{c[0][0]}+{len(c[0]) - 1}x{c[0][-1]}-{c[1]}-{c[2]}x{c[3]}')
def test_osa_concat_conv_against_fp64(case):
    from graph_detr4d_amd import ops
    chans, cout, h, w, sliced = case
    srcs, weight, scale, shift, ref = _osa_case(chans, cout, h, w)
    dsrcs = [s.to(DEV) for s in srcs]
    if sliced:                                                              # its own base pointer inside a larger buffer
        big = torch.full((N + 1, chans[0], h, w), float('nan'), device=DEV)
        big[1:] = dsrcs[0]
        dsrcs[0] = big[1:]
        assert dsrcs[0].is_contiguous() and dsrcs[0].data_ptr() != big.data_ptr()
    image = ops.osa_concat_image(weight.to(DEV))
    run = lambda: ops.osa_concat_conv(dsrcs, image, cout, scale.to(DEV), shift.to(DEV))
    out, partials = run()
    torch.cuda.synchronize()
    assert tuple(out.shape) == tuple(ref.shape)
    assert tuple(partials.shape) == (N, (h * w + 127) // 128, cout)
    err = R.rel_err(out, ref)
    mean_ref = ref.mean(dim=(2, 3))
    mean = partials.cpu().double().sum(dim=1) / (h * w)
    err_mean = float((mean - mean_ref).abs().max() / mean_ref.abs().max())
    print(f'osa_concat_conv {chans} -> {cout} at {h} x {w}: rel_err {err:.3e}, pool mean {err_mean:.3e}')
    assert err <= KERNEL_TOL
    assert err_mean <= KERNEL_TOL
    out2, partials2 = run()
    assert torch.equal(out, out2) and torch.equal(partials, partials2)
    for mt in _tilings(cout):
        out2, partials2 = ops.osa_concat_conv(dsrcs, image, cout, scale.to(DEV), shift.to(DEV), m_blocks=mt)
        assert torch.equal(out, out2) and torch.equal(partials, partials2), mt


@functools.lru_cache(maxsize=None)
def _ese_case(c, h, w):
    xt = torch.relu(_rand(N, c, h, w, seed=30))
    identity = _rand(N, c, h, w, seed=31)
    fc_w = _rand(c, c, 1, 1, seed=32, scale=c ** -0.5)
    fc_b = _rand(c, seed=33, scale=0.5)
    fc_b[0::7], fc_b[3::7] = 8.0, -8.0                                     # gates of exactly 1 and exactly 0
    gate = R.ese_gate(xt.double().mean(dim=(2, 3)), fc_w, fc_b)
    return xt, identity, fc_w, fc_b, gate


@pytest.mark.parametrize('hw', [(5, 7), (13, 21)], ids=lambda v: f'{v[0]}x{v[1]}')
@pytest.mark.parametrize('c', [256, 1024])
def test_ese_gate_and_apply_against_fp64(c, hw):
    from graph_detr4d_amd import ops
    h, w = hw
    assert (h * w) % 4 != 0
    xt, identity, fc_w, fc_b, gate_ref = _ese_case(c, h, w)
    assert (gate_ref == 0).any() and (gate_ref == 1).any() and ((gate_ref > 0) & (gate_ref < 1)).any()
    # the partials as the aggregation leaves them: per-channel sums over tiles of 128 consecutive pixels
    flat = xt.reshape(N, c, h * w)
    partials = torch.stack([t.sum(dim=2) for t in flat.split(128, dim=2)], dim=1).contiguous()
    dxt, did = xt.to(DEV), identity.to(DEV)
    gate = ops.ese_gate(partials.to(DEV), h * w, fc_w.to(DEV), fc_b.to(DEV))
    torch.cuda.synchronize()
    err = R.rel_err(gate, gate_ref)
    print(f'ese_gate C = {c}, HW = {h * w}: rel_err {err:.3e}')
    assert err <= KERNEL_TOL
    assert torch.equal(gate.cpu() == 0, gate_ref == 0) and torch.equal(gate.cpu() == 1, gate_ref == 1)
    assert torch.equal(gate, ops.ese_gate(partials.to(DEV), h * w, fc_w.to(DEV), fc_b.to(DEV)))
    for ident in (None, did):
        ref = xt.double() * gate.cpu().double()[:, :, None, None] + (0 if ident is None else identity.double())
        out = ops.ese_apply(dxt, gate, identity=ident)
        torch.cuda.synchronize()
        err = R.rel_err(out, ref)
        print(f'ese_apply C = {c}, HW = {h * w}, identity {ident is not None}: rel_err {err:.3e}')
        assert err <= KERNEL_TOL
        assert torch.equal(out, ops.ese_apply(dxt, gate, identity=ident))
        alias = dxt.clone()
        assert ops.ese_apply(alias, gate, identity=ident, out=alias) is alias
        assert torch.equal(alias, out)                                      # out aliasing xt


# ---- 2. one OSA module through the classes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('identity', [False, True], ids=['plain', 'identity'])
def test_osa_module_against_fp64(identity):
    from graph_detr4d_amd import vovnet
    in_ch, stage_ch, concat_ch = (256, 160, 256) if identity else (128, 128, 256)
    m = R.randomize_(vovnet._OSA_module(in_ch, stage_ch, concat_ch, 5, 'OSA3_2', identity=identity), seed=40).eval()
    x = torch.relu(_rand(N, in_ch, 13, 21, seed=41))
    ref, gates = R.osa_module(m.state_dict(), '', 'OSA3_2', x, identity, return_gate=True)
    assert (gates == 0).any() and (gates == 1).any() and ((gates > 0) & (gates < 1)).any()
    m = m.to(DEV)
    with torch.no_grad():
        out = m(x.to(DEV))
        torch.cuda.synchronize()
        err = R.rel_err(out, ref)
        print(f'_OSA_module identity={identity}: rel_err {err:.3e}')
        assert err <= MODULE_TOL
        assert torch.equal(out, m(x.to(DEV)))


# ---- 3. whole networks -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _golden():
    return Golden('vovnet_tiny')


@pytest.fixture
def tiny(monkeypatch):
    """A builder of the tiny-spec network with the fixture's state dict, on the GPU; the spec is in the package's table for the test."""
    from graph_detr4d_amd import vovnet
    g = _golden()
    monkeypatch.setitem(vovnet._STAGE_SPECS, g.meta['spec_name'], g.meta['spec'])

    def build(cls_name='VoVNetCP', **kw):
        net = getattr(vovnet, cls_name)(g.meta['spec_name'], out_features=FEATS, **kw).eval()
        net.load_state_dict(g.state(), strict=True)
        return net.to(DEV)
    return build


def _image(g):
    return g.t('img').float() / g.meta['feat_scale']


def test_fixture_network_against_the_recorded_maps(tiny):
    """The tiny-spec VoVNetCP with the fixture's state dict, on the kernel route, against the reference's recorded maps.  The bound at
    stage s is 2e-4 x (OSA modules up to s); the stem, three convolutions, has the bound of one module."""
    from graph_detr4d_amd import functional as Fn
    g = _golden()
    sd, cs = g.state(), g.meta['chan_stride']
    net = tiny()
    x = _image(g).to(DEV)
    with torch.no_grad():
        outs = net(x)
        again = net(x)
        with Fn.torch_ops_for(net):
            torch_outs = net(x)
    torch.cuda.synchronize()
    fp64 = R.vovnet(sd, _image(g))
    for s, (f, o, o2, t) in enumerate(zip(FEATS, outs, again, torch_outs), start=1):
        pick = (lambda m: m[:, ::cs]) if f in ('stem', 'stage2') else (lambda m: m)
        bound = MODULE_TOL * max(1, R.modules_up_to(sd, s))
        err = R.rel_err(pick(o), g.t(f))
        print(f'fixture {f}: kernels against the recording {err:.3e} (bound {bound:.1e}); against fp64: kernels '
              f'{R.rel_err(o, fp64[f]):.3e}, torch ops {R.rel_err(t, fp64[f]):.3e}')
        assert list(o.shape) == g.meta['shapes'][f]
        assert err <= bound
        assert torch.equal(o, o2)
    named = tiny('VoVNet')
    with torch.no_grad():
        d = named(x)
    assert list(d) == list(FEATS) and all(torch.equal(d[f], o) for f, o in zip(FEATS, outs))


@functools.lru_cache(maxsize=None)
def _v99():
    """(the four-feature VoVNetCP, the two-feature VoVNetCP, the four-feature VoVNet), the three sharing their layers."""
    from graph_detr4d_amd import VoVNet, VoVNetCP
    four = ('stage2', 'stage3', 'stage4', 'stage5')
    net = R.randomize_(VoVNetCP('V-99-eSE', out_features=four), seed=70).eval().to(DEV)
    others = [VoVNetCP('V-99-eSE', out_features=('stage4', 'stage5')).eval(), VoVNet('V-99-eSE', out_features=four).eval()]
    for o in others:
        for name in ('stem', 'stage2', 'stage3', 'stage4', 'stage5'):
            setattr(o, name, getattr(net, name))
    return (net, *others)


def test_v99_against_its_torch_route():
    from graph_detr4d_amd import functional as Fn
    net, net2, named = _v99()
    x = _rand(N, 3, 52, 84, seed=71).to(DEV)
    with torch.no_grad():
        outs = net(x)
        again = net(x)
        two = net2(x)
        d = named(x)
        with Fn.torch_ops_for(net):
            want = net(x)
    torch.cuda.synchronize()
    assert [tuple(o.shape) for o in outs] == [(N, 256, 13, 21), (N, 512, 6, 10), (N, 768, 3, 5), (N, 1024, 1, 2)]   # ceil_mode
    modules = (1, 4, 13, 16)                                                # OSA modules up to stages 2, 3, 4, 5
    for o, o2, t, k in zip(outs, again, want, modules):
        err = R.rel_err(o, t.cpu())
        print(f'V-99 after {k} modules: kernels against the torch-op route {err:.3e} (bound {MODULE_TOL * k:.1e}), largest entry '
              f'{float(t.abs().max()):.3e}')
        assert torch.isfinite(t).all() and float(t.abs().max()) > 0
        assert err <= MODULE_TOL * k
        assert torch.equal(o, o2)
    assert len(two) == 2 and torch.equal(two[0], outs[2]) and torch.equal(two[1], outs[3])
    assert list(d) == ['stage2', 'stage3', 'stage4', 'stage5'] and all(torch.equal(d[f'stage{i + 2}'], outs[i]) for i in range(4))


def test_graph_capture_replay_and_weight_edit(tiny):
    """Capturing before any eager call raises; after one, a hipGraph captured on input A and replayed on input B equals the eager call on
    B bit for bit; an in-place weight edit followed by an eager call changes the output."""
    g = _golden()
    net = tiny()
    a = _image(g).to(DEV)
    b = _rand(*a.shape, seed=80).to(DEV)
    static = a.clone()
    with torch.no_grad():
        graph = torch.cuda.CUDAGraph()
        with pytest.raises(RuntimeError, match='once eagerly'):
            with torch.cuda.graph(graph, capture_error_mode='thread_local'):
                net(static)
        torch.cuda.synchronize()
        net(static)                                                         # eager once: the images exist
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode='thread_local'):
            outs = net(static)
        static.copy_(b)
        graph.replay()
        eager = net(b)
        assert all(torch.equal(o, e) for o, e in zip(outs, eager))
        for p in net.parameters():
            p.mul_(0.5)                                                     # in place: the version counters move
        edited = net(b)
        assert not torch.equal(edited[-1], eager[-1])
        graph.replay()                                                      # the eager call rebuilt the images into the same buffers
        assert all(torch.equal(o, e) for o, e in zip(outs, edited))
    torch.cuda.synchronize()


# ---- 4. the C ABI's error codes ------------------------------------------------------------------------------------------------
def test_abi_error_codes():
    from graph_detr4d_amd import _lib
    lib = _lib.load()
    invalid, unsupported, misaligned = -1, -2, -3                            # GD4D_EINVAL, GD4D_EUNSUPPORTED, GD4D_EALIGN
    ptr = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    x = torch.zeros(N, 64, 5, 7, device=DEV)
    x48 = torch.zeros(N, 48, 5, 7, device=DEV)
    out = torch.zeros(N, 64, 5, 7, device=DEV)
    vec = torch.ones(64, device=DEV)
    image = torch.zeros(64 * 64 * 9 * 4 + 16, dtype=torch.uint8, device=DEV)
    assert lib.gd4d_conv3x3_image_bytes(48, 64) == 0 and lib.gd4d_conv3x3_image_bytes(64, 64) == 64 * 64 * 9 * 4
    assert lib.gd4d_conv3x3_bn_relu_fwd(ptr(x48), N, 48, 5, 7, 1, ptr(image), 64, ptr(vec), ptr(vec), ptr(out), 0, None) == unsupported
    assert lib.gd4d_conv3x3_bn_relu_fwd(ptr(x), N, 64, 5, 7, 1, ptr(image), 64, ptr(vec), ptr(vec), ptr(out), 3, None) == unsupported   # 3 does not divide 2
    assert lib.gd4d_conv3x3_bn_relu_fwd(ptr(x), N, 64, 5, 7, 3, ptr(image), 64, ptr(vec), ptr(vec), ptr(out), 0, None) == unsupported
    assert lib.gd4d_conv3x3_bn_relu_fwd(None, N, 64, 5, 7, 1, ptr(image), 64, ptr(vec), ptr(vec), ptr(out), 0, None) == invalid
    assert lib.gd4d_conv3x3_bn_relu_fwd(ptr(x), N, 64, 5, 7, 1, ptr(image, 4), 64, ptr(vec), ptr(vec), ptr(out), 0, None) == misaligned
    assert lib.gd4d_conv3x3_image(ptr(x), 64, 64, ptr(image, 4), None) == misaligned
    partials = torch.zeros(N, 1, 64, device=DEV)
    chans = (ctypes.c_int32 * 2)(64, 64)
    srcs = (ctypes.c_void_p * 2)(x.data_ptr(), None)
    osa_image = torch.zeros(128 * 64 * 4 + 16, dtype=torch.uint8, device=DEV)
    args = lambda s, img: (s, chans, 2, N, 5, 7, img, 64, ptr(vec), ptr(vec), ptr(out), ptr(partials), 0, None)
    assert lib.gd4d_osa_concat_conv_fwd(*args(srcs, ptr(osa_image))) == invalid                          # a NULL source
    srcs = (ctypes.c_void_p * 2)(x.data_ptr(), x.data_ptr())
    assert lib.gd4d_osa_concat_conv_fwd(*args(srcs, ptr(osa_image, 4))) == misaligned
    chans[1] = 48
    assert lib.gd4d_osa_concat_conv_fwd(*args(srcs, ptr(osa_image))) == unsupported
    torch.cuda.synchronize()
