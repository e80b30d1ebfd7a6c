"""ResNet's plain convolutions on the library's kernels (gd4d_resnet.hip; `plain_kernels=True`) against the fp64 restatement
(resnet_ref.py) and the modules' own torch-op route; the bit-for-bit properties (two runs, every M tiling, the stride-2 pointwise
against the stride-1 kernel on the subsampled input, a captured graph).  GPU only.  mmdet is not installed and the reference repository
holds no ResNet: there is no golden fixture.

Shapes (resnet_cases.py): N = 2; 13 x 21 is two ragged tiles each way, 5 x 7 one ragged tile, 26 x 37 -> 13 x 19 and 5 x 7 -> 3 x 4 the
even and odd stride-2 sizes.  Every case also runs with each M tiling (1, 2, 3, 4, 5, 7 row blocks) that divides its channel count.
Tolerances: 1e-4 of the map's largest |entry| per kernel, 2e-4 per block (test_vovnet_gpu.py), accumulated linearly over the
blocks for a network.  No entry is excluded."""
import ctypes

import pytest
import torch

import resnet_cases as C
import resnet_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
N = C.N
KERNEL_TOL, MODULE_TOL = 1e-4, 2e-4
DCN = dict(type='DCNv2', deform_groups=1, fallback_on_stride=False)
FROZEN = dict(type='BN', requires_grad=False)


def _tilings(cout):
    return [mt for mt in (1, 2, 3, 4, 5, 7) if (cout // 32) % mt == 0]


# ---- 1, 2. kernels ---------------------------------------------------------------------------------------------------------
def _kernel_case(taps, case):
    from graph_detr4d_amd import ops
    cin, cout, stride, identity, relu, h, w = case
    x, weight, scale, shift, ident, ref = C.conv_case(taps, *case)
    name, make, run_op = ('conv3x3_bn_act', ops.conv3x3_act_image, ops.conv3x3_bn_act) if taps == 9 else \
        ('conv1x1_bn_act', ops.conv1x1_image, ops.conv1x1_bn_act)
    image = make(weight.to(DEV))
    dx, dscale, dshift, dident = x.to(DEV), scale.to(DEV), shift.to(DEV), None if ident is None else ident.to(DEV)
    run = lambda inp=dx, s=stride, **kw: run_op(inp, image, cout, dscale, dshift, stride=s, identity=dident, relu=relu, **kw)  # noqa: E731
    out = run()
    torch.cuda.synchronize()
    assert tuple(out.shape) == tuple(ref.shape) == (N, cout, (h - 1) // stride + 1, (w - 1) // stride + 1)
    err = R.rel_err(out, ref)
    zeros = float((ref == 0).double().mean())
    print(f'{name} {C.case_id(case)}: rel_err {err:.3e}, {zeros:.2f} of the outputs are 0')
    assert err <= KERNEL_TOL
    if relu:
        assert zeros > 0.2                                                  # the ReLU is exercised
    else:
        assert float((ref < 0).double().mean()) > 0.2                       # ... and where it is off, negative outputs come through
    assert torch.equal(out, run())                                          # no atomics: two runs give the same bits
    for mt in _tilings(cout):                                               # ... and so does every M tiling
        assert torch.equal(out, run(m_blocks=mt)), mt
    return out, run, dx


@pytest.mark.parametrize('case', C.CONV1X1_CASES, ids=C.case_id)
def test_conv1x1_bn_act_against_fp64(case):
    out, run, dx = _kernel_case(1, case)
    if case[2] == 2:                                                        # the same K walk as the stride-1 kernel's on the subsampled map
        assert torch.equal(out, run(dx[:, :, ::2, ::2].contiguous(), 1))


@pytest.mark.parametrize('case', C.CONV3X3_CASES, ids=C.case_id)
def test_conv3x3_bn_act_against_fp64(case):
    _kernel_case(9, case)


def test_conv3x3_bn_act_gives_conv3x3_bn_relu_its_bits():
    from graph_detr4d_amd import ops
    cin, cout, stride, h, w = 64, 128, 2, 26, 37
    x, weight = C.rand(N, cin, h, w, seed=1).to(DEV), C.rand(cout, cin, 3, 3, seed=2, scale=(9 * cin) ** -0.5).to(DEV)
    scale, shift = (t.to(DEV) for t in C.scale_shift(cout, 3))
    image = ops.conv3x3_image(weight)
    assert torch.equal(image, ops.conv3x3_act_image(weight))
    want = ops.conv3x3_bn_relu(x, image, cout, scale, shift, stride=stride)
    assert float((want == 0).float().mean()) > 0.2
    assert torch.equal(ops.conv3x3_bn_act(x, image, cout, scale, shift, stride=stride, identity=None, relu=True), want)


# ---- 3. blocks ---------------------------------------------------------------------------------------------------------------
def _block(kind, inplanes, planes, stride=1, dcn=None, seed=40):
    """A stage's first block as ResNet builds it (with the downsample where the shapes ask for one), plain_kernels=True, randomised."""
    import graph_detr4d_amd as G
    blk = G.ResNet._make_stage(inplanes, planes, 1, stride, 1, FROZEN, dcn, False, False, getattr(G, kind), True)[0]
    return R.randomize_(blk, seed).eval()


# (block, inplanes, planes, stride, has a downsample, h, w)
BLOCK_CASES = [('Bottleneck', 64, 64, 1, True, 13, 21), ('Bottleneck', 256, 128, 2, True, 26, 37), ('Bottleneck', 512, 128, 1, False, 13, 21),
               ('BasicBlock', 64, 128, 2, True, 26, 37), ('BasicBlock', 128, 128, 1, False, 13, 21)]


@pytest.mark.parametrize('case', BLOCK_CASES, ids=lambda c: f'{c[0]}-{c[1]}-{c[2]}-s{c[3]}')
def test_block_against_fp64(case):
    kind, inplanes, planes, stride, down, h, w = case
    blk = _block(kind, inplanes, planes, stride)
    assert (blk.downsample is not None) == down and blk.plain_kernels
    x = torch.relu(C.rand(N, inplanes, h, w, seed=41))
    ref = (R.bottleneck if kind == 'Bottleneck' else R.basic_block)(blk.state_dict(), '', x, stride)
    blk = blk.to(DEV)
    with torch.no_grad():
        out = blk(x.to(DEV))
        torch.cuda.synchronize()
        err = R.rel_err(out, ref)
        print(f'{kind}({inplanes}, {planes}, stride={stride}): rel_err {err:.3e}, {float((ref == 0).double().mean()):.2f} of the outputs are 0')
        assert tuple(out.shape) == tuple(ref.shape) == (N, planes * blk.expansion, (h - 1) // stride + 1, (w - 1) // stride + 1)
        assert err <= MODULE_TOL
        assert torch.equal(out, blk(x.to(DEV)))


def test_dcn_bottleneck_against_its_torch_route():
    from graph_detr4d_amd import functional as Fn
    blk = _block('Bottleneck', 1024, 256, dcn=DCN, seed=42).to(DEV)
    assert blk.with_dcn and blk.downsample is None and [k for k, _, _ in blk._plain_layers()] == ['conv1', 'conv3']
    x = torch.relu(C.rand(N, 1024, 13, 21, seed=43)).to(DEV)
    with torch.no_grad():
        out = blk(x)
        with Fn.torch_ops_for(blk):
            assert blk.conv2.torch_ops
            want = blk(x)
        assert not blk.conv2.torch_ops
        torch.cuda.synchronize()
        err = R.rel_err(out, want.cpu())
        print(f'Bottleneck with DCN, plain_kernels=True, against its torch-op route: rel_err {err:.3e}')
        assert tuple(out.shape) == (N, 1024, 13, 21) and float(want.abs().max()) > 0
        assert err <= MODULE_TOL
        assert torch.equal(out, blk(x))


# ---- 4. whole networks -------------------------------------------------------------------------------------------------------
NETS = {'r50': (dict(depth=50), (256, 512, 1024, 2048), (3, 7, 13, 16)),
        'r50_dcn': (dict(depth=50, dcn=DCN, stage_with_dcn=(False, False, True, True)), (256, 512, 1024, 2048), (3, 7, 13, 16)),
        'r18': (dict(depth=18, norm_cfg=dict(type='BN2d', requires_grad=False)), (64, 128, 256, 512), (2, 4, 6, 8))}


@pytest.mark.parametrize('name', list(NETS))
def test_network_against_its_torch_route(name):
    import graph_detr4d_amd as G
    from graph_detr4d_amd import functional as Fn
    kw, chans, blocks = NETS[name]
    kw = dict(dict(norm_cfg=FROZEN), **kw)
    net = R.randomize_(G.ResNet(plain_kernels=True, **kw), seed=70).eval().to(DEV)
    stock = G.ResNet(**kw).eval()
    stock.load_state_dict(net.state_dict(), strict=True)
    stock = stock.to(DEV)
    assert [R.blocks_up_to(net.state_dict(), i) for i in (1, 2, 3, 4)] == list(blocks)
    x = C.rand(N, 3, 52, 84, seed=71).to(DEV)
    with torch.no_grad():
        outs = net(x)
        again = net(x)
        with Fn.torch_ops_for(net):
            want = net(x)
        plain = stock(x)
    torch.cuda.synchronize()
    assert [tuple(o.shape) for o in outs] == [(N, c, h, w) for c, (h, w) in zip(chans, ((13, 21), (7, 11), (4, 6), (2, 3)))]
    for o, o2, t, s, k in zip(outs, again, want, plain, blocks):
        err, err_stock = R.rel_err(o, t.cpu()), R.rel_err(s, t.cpu())
        print(f'{name} after {k} blocks: kernels against the torch-op route {err:.3e}, plain_kernels=False {err_stock:.3e} '
              f'(bound {MODULE_TOL * k:.1e}), largest entry {float(t.abs().max()):.3e}')
        assert torch.isfinite(t).all() and torch.isfinite(o).all() and float(t.abs().max()) > 0
        assert err <= MODULE_TOL * k
        assert err_stock <= MODULE_TOL * k
        assert torch.equal(o, o2)


# ---- 5. capture ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['r18', 'r50_two_stages'])
def test_graph_capture_replay_and_weight_edit(name):
    """Capturing before any eager call raises; after one, a hipGraph captured on input A and replayed on input B equals the eager call on
    B bit for bit; an in-place weight edit followed by an eager call changes the output, and the next replay shows it."""
    import graph_detr4d_amd as G
    kw = dict(depth=18) if name == 'r18' else dict(depth=50, num_stages=2, strides=(1, 2), dilations=(1, 1), out_indices=(0, 1))
    net = R.randomize_(G.ResNet(plain_kernels=True, norm_cfg=FROZEN, **kw), seed=80).eval().to(DEV)
    a, b = C.rand(N, 3, 52, 84, seed=81).to(DEV), C.rand(N, 3, 52, 84, seed=82).to(DEV)
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


# ---- 6. the C ABI's error codes ----------------------------------------------------------------------------------------------
def test_abi_error_codes():
    from graph_detr4d_amd import _lib
    lib = _lib.load()
    invalid, unsupported, misaligned = -1, -2, -3                            # GD4D_EINVAL, GD4D_EUNSUPPORTED, GD4D_EALIGN
    ptr = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)               # noqa: E731
    x = torch.zeros(N, 64, 5, 7, device=DEV)
    x48 = torch.zeros(N, 48, 5, 7, device=DEV)
    out = torch.zeros(N, 64, 5, 7, device=DEV)
    vec = torch.ones(64, device=DEV)
    image = torch.zeros(64 * 64 * 9 * 4 + 16, dtype=torch.uint8, device=DEV)
    assert lib.gd4d_conv1x1_image_bytes(48, 64) == 0 and lib.gd4d_conv1x1_image_bytes(2048, 2048) == 2048 * 2048 * 4
    assert lib.gd4d_conv1x1_image_bytes(2304, 2048) == 2304 * 2048 * 4 and lib.gd4d_conv1x1_image_bytes(64, 2080) == 0
    assert lib.gd4d_conv3x3_act_image_bytes(512, 512) == 512 * 512 * 9 * 4 and lib.gd4d_conv3x3_act_image_bytes(64, 544) == 0
    assert lib.gd4d_conv3x3_image_bytes(512, 512) == 0                       # VoVNet's entry points keep their limits
    for fwd in (lib.gd4d_conv1x1_bn_act_fwd, lib.gd4d_conv3x3_bn_act_fwd):
        def call(xp=ptr(x), cin=64, stride=1, img=ptr(image), scale=ptr(vec), outp=ptr(out), mt=0):
            return fwd(xp, N, cin, 5, 7, stride, img, 64, scale, ptr(vec), None, 1, outp, mt, None)
        assert call(xp=None) == invalid and call(img=None) == invalid and call(scale=None) == invalid and call(outp=None) == invalid
        assert call(xp=ptr(x48), cin=48) == unsupported
        assert call(stride=3) == unsupported
        assert call(mt=3) == unsupported                                    # 3 does not divide 2
        assert call(img=ptr(image, 4)) == misaligned
    assert lib.gd4d_conv1x1_image(None, 64, 64, ptr(image), None) == invalid
    assert lib.gd4d_conv1x1_image(ptr(x), 64, 64, None, None) == invalid
    assert lib.gd4d_conv1x1_image(ptr(x), 48, 64, ptr(image), None) == unsupported
    assert lib.gd4d_conv1x1_image(ptr(x), 64, 64, ptr(image, 4), None) == misaligned
    torch.cuda.synchronize()
