"""DCNv2 on the library's kernels (gd4d_dcn.hip) against the fp64 restatement (dcn_ref.py) and the modules' own torch-op route; the
bit-for-bit properties (two runs, a captured graph).  GPU only.

Shapes: N = 2 images; inputs 13 x 21 (ragged 16-pixel tiles, a second tile in x; with 512 output channels the tile is 16 x 8: a second
tile in y too), 5 x 7, and 26 x 37 for stride 2 (-> 13 x 19: an even and an odd size, the last tap of the last column off the image
in x only).  Channels (256, 256), (512, 512), (256, 512): both kernel shapes, both weight-image geometries; (64, 128): output channels
padded to 256.  Offsets: normal with sigma = 2 px, and dcn_ref.crafted_offsets's planes (one image per plane).
Tolerances: 1e-4 of the map's largest |entry| per kernel, 2e-4 per module.  The function is continuous: no entry is excluded."""
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import dcn_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
N = 2
KERNEL_TOL, MODULE_TOL = 1e-4, 2e-4
# (cin, cout, stride, h, w)
KERNEL_CASES = [(256, 256, 1, 13, 21), (256, 256, 1, 5, 7), (256, 256, 2, 26, 37), (512, 512, 1, 13, 21), (512, 512, 2, 26, 37),
                (256, 512, 1, 5, 7), (256, 512, 2, 26, 37), (64, 128, 1, 5, 7)]
CRAFTED_CASES = [(256, 256, 1, 5, 7), (256, 256, 1, 13, 21), (256, 256, 2, 26, 37), (512, 512, 1, 5, 7)]


def _rand(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


@functools.lru_cache(maxsize=None)
def _kernel_case(cin, cout, stride, h, w):
    """Inputs, a sigma = 2 offset map, modulations in (0, 1) and the fp64 result; computed once."""
    ho, wo = R.out_hw(h, w, stride)
    x = _rand(N, cin, h, w, seed=1)
    weight = _rand(cout, cin, 3, 3, seed=2, scale=(9 * cin) ** -0.5)
    offset = _rand(N, 18, ho, wo, seed=3, scale=2.0)
    mask = torch.rand(N, 9, ho, wo, generator=torch.Generator().manual_seed(4))
    return x, weight, offset, mask, R.dcn_ref(x, offset, mask, weight, None, stride)


@functools.lru_cache(maxsize=None)
def _crafted_case(cin, cout, stride, h, w):
    """One image per crafted plane (the same random image under each), and the fp64 result."""
    planes = R.crafted_offsets(h, w, stride)
    names = list(planes)
    ho, wo = R.out_hw(h, w, stride)
    x = _rand(1, cin, h, w, seed=5).expand(len(names), -1, -1, -1).contiguous()
    weight = _rand(cout, cin, 3, 3, seed=6, scale=(9 * cin) ** -0.5)
    offset = torch.cat([planes[k] for k in names])
    mask = torch.rand(len(names), 9, ho, wo, generator=torch.Generator().manual_seed(7))
    return names, x, weight, offset, mask, R.dcn_ref(x, offset, mask, weight, None, stride)


def _run_kernel(x, weight, offset, mask, stride, **kw):
    from graph_detr4d_amd import ops
    image = ops.dcn_weight_image(weight.to(DEV))
    out = ops.dcn_fwd(x.to(DEV), torch.cat((offset, mask), dim=1).to(DEV), image, weight.shape[0], stride=stride, **kw)
    torch.cuda.synchronize()
    return out


# ---- 1. kernels ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', KERNEL_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_dcn_kernel_against_fp64(case):
    cin, cout, stride, h, w = case
    x, weight, offset, mask, ref = _kernel_case(*case)
    out = _run_kernel(x, weight, offset, mask, stride)
    assert tuple(out.shape) == tuple(ref.shape)
    err = R.rel_err(out, ref)
    print(f'dcn_fwd {case}: rel_err {err:.3e}')
    assert err <= KERNEL_TOL
    again = _run_kernel(x, weight, offset, mask, stride)
    assert torch.equal(out, again)                                          # no atomics: two runs give the same bits


@pytest.mark.parametrize('case', CRAFTED_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_dcn_kernel_crafted_offsets(case):
    cin, cout, stride, h, w = case
    names, x, weight, offset, mask, ref = _crafted_case(*case)
    out = _run_kernel(x, weight, offset, mask, stride).cpu()
    for i, name in enumerate(names):
        if float(ref[i].abs().max()) == 0.0:                                # nothing inside the image: exactly zero
            print(f'dcn_fwd {case} {name}: reference is zero, max |out| {float(out[i].abs().max()):.3e}')
            assert float(out[i].abs().max()) == 0.0, name
            continue
        err = R.rel_err(out[i], ref[i])
        print(f'dcn_fwd {case} {name}: rel_err {err:.3e}')
        assert err <= KERNEL_TOL, name
    assert {'zero', 'integers', 'at_minus_1', 'at_h_minus_1', 'at_h_and_w', 'plus_1000', 'minus_1000', 'corner_tl', 'corner_tr',
            'corner_bl', 'corner_br'} == set(names)


def test_dcn_kernel_epilogue_scale_shift_relu():
    case = (256, 256, 1, 13, 21)
    x, weight, offset, mask, ref = _kernel_case(*case)
    scale, shift = _rand(256, seed=8) + 1.5, _rand(256, seed=9)
    want = F.relu(ref * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1))
    out = _run_kernel(x, weight, offset, mask, 1, scale=scale.to(DEV), shift=shift.to(DEV), relu=True)
    err = R.rel_err(out, want)
    print(f'dcn_fwd scale / shift / relu: rel_err {err:.3e}')
    assert err <= KERNEL_TOL and float((out == 0).float().mean()) > 0.2
    plain = _run_kernel(x, weight, offset, mask, 1, shift=shift.to(DEV))
    assert R.rel_err(plain, ref + shift.double().view(1, -1, 1, 1)) <= KERNEL_TOL


@pytest.mark.parametrize('case', [(256, 1, 13, 21), (256, 2, 26, 37), (512, 1, 5, 7), (512, 2, 26, 37), (64, 1, 5, 7)],
                         ids=lambda c: 'x'.join(map(str, c)))
def test_offset_conv_kernel_against_fp64(case):
    from graph_detr4d_amd import ops
    cin, stride, h, w = case
    x = _rand(N, cin, h, w, seed=11)
    weight = _rand(27, cin, 3, 3, seed=12, scale=2.0 * (9 * cin) ** -0.5)                    # offsets of sigma ~ 2 px
    bias = _rand(27, seed=13, scale=0.5)
    off, msk = R.offset_conv_ref(x, weight, bias, stride)
    ref = torch.cat((off, msk), dim=1)
    out = ops.dcn_offset_conv_fwd(x.to(DEV), ops.dcn_weight_image(weight.to(DEV)), bias.to(DEV), stride=stride)
    torch.cuda.synchronize()
    assert tuple(out.shape) == tuple(ref.shape)
    err = R.rel_err(out, ref)
    err_mask = R.rel_err(out[:, 18:], msk)
    print(f'dcn_offset_conv_fwd {case}: rel_err {err:.3e} (modulation planes alone {err_mask:.3e})')
    assert err <= KERNEL_TOL and err_mask <= KERNEL_TOL
    assert torch.equal(out, ops.dcn_offset_conv_fwd(x.to(DEV), ops.dcn_weight_image(weight.to(DEV)), bias.to(DEV), stride=stride))


# ---- 2. modules ------------------------------------------------------------------------------------------------------------
def _pack(cin, cout, stride, seed=20, bias=True):
    import graph_detr4d_amd as G
    torch.manual_seed(seed)
    m = G.ModulatedDeformConv2dPack(cin, cout, 3, stride=stride, padding=1, bias=bias)
    with torch.no_grad():
        m.conv_offset.weight.normal_(std=2.0 * (9 * cin) ** -0.5)
        m.conv_offset.bias.normal_(std=0.5)
        if bias:
            m.bias.normal_(std=0.2)
    return m.eval()


def _bn(c, seed=30):
    torch.manual_seed(seed)
    bn = nn.BatchNorm2d(c).eval()
    with torch.no_grad():
        bn.running_mean.normal_(std=0.3)
        bn.running_var.uniform_(0.5, 2.0)
        bn.weight.normal_(mean=1.0, std=0.3)
        bn.bias.normal_(std=0.3)
    return bn


@pytest.mark.parametrize('case', [(256, 256, 1, 13, 21), (256, 256, 2, 26, 37), (512, 512, 1, 5, 7), (512, 512, 2, 26, 37)],
                         ids=lambda c: 'x'.join(map(str, c)))
def test_pack_forward_and_bn_relu(case):
    from graph_detr4d_amd import functional as Fn
    cin, cout, stride, h, w = case
    m, bn = _pack(cin, cout, stride), _bn(cout)
    x = _rand(N, cin, h, w, seed=21)
    off, msk = R.offset_conv_ref(x, m.conv_offset.weight.detach(), m.conv_offset.bias.detach(), stride)
    ref = R.dcn_ref(x, off, msk, m.weight.detach(), m.bias.detach(), stride)
    ref_bn = F.relu(bn.double()(ref))
    bn.float()
    m, bn = m.to(DEV), bn.to(DEV)
    with torch.no_grad():
        out, out_bn = m(x.to(DEV)), m.forward_bn_relu(x.to(DEV), bn)
        with Fn.torch_ops_for(m):
            t_out, t_bn = m(x.to(DEV)), m.forward_bn_relu(x.to(DEV), bn)
    torch.cuda.synchronize()
    errs = dict(fwd_fp64=R.rel_err(out, ref), bn_relu_fp64=R.rel_err(out_bn, ref_bn), fwd_torch=R.rel_err(out, t_out.cpu()),
                bn_relu_torch=R.rel_err(out_bn, t_bn.cpu()))
    print(f'pack {case}: ' + ', '.join(f'{k} {v:.3e}' for k, v in errs.items()))
    assert all(v <= MODULE_TOL for v in errs.values()), errs
    with torch.no_grad():
        assert torch.equal(out, m(x.to(DEV))) and torch.equal(out_bn, m.forward_bn_relu(x.to(DEV), bn))


def test_caller_supplied_offset_and_mask():
    import graph_detr4d_amd as G
    case = (256, 256, 1, 13, 21)
    x, weight, offset, mask, ref = _kernel_case(*case)
    m = G.ModulatedDeformConv2d(256, 256, 3, padding=1, bias=False).eval()
    with torch.no_grad():
        m.weight.copy_(weight)
        out = m.to(DEV)(x.to(DEV), offset.to(DEV), mask.to(DEV))
    assert R.rel_err(out, ref) <= MODULE_TOL


def test_zero_init_pack_is_half_the_convolution():
    import graph_detr4d_amd as G
    torch.manual_seed(40)
    m = G.ModulatedDeformConv2dPack(256, 256, 3, stride=1, padding=1, bias=False).eval()
    x = _rand(N, 256, 13, 21, seed=41)
    ref = 0.5 * F.conv2d(x.double(), m.weight.detach().double(), None, padding=1)
    with torch.no_grad():
        out = m.to(DEV)(x.to(DEV))
    err = R.rel_err(out, ref)
    print(f'zero-initialised pack against 0.5 x conv2d: rel_err {err:.3e}')
    assert err <= KERNEL_TOL


def test_default_route_refuses_train_and_autograd_on_the_gpu():
    from graph_detr4d_amd._lib import Gd4dError
    m = _pack(256, 256, 1).to(DEV)
    x = torch.zeros(1, 256, 5, 7, device=DEV)
    with pytest.raises(Gd4dError, match='torch_ops'):
        m(x)                                                                # autograd on, parameters require grad
    m.train()
    with torch.no_grad(), pytest.raises(Gd4dError, match='train'):
        m(x)
    m.torch_ops = True
    out = m(x.requires_grad_(True))                                         # the chosen route trains
    out.sum().backward()
    assert m.weight.grad is not None and m.conv_offset.weight.grad is not None and x.grad is not None


def test_graph_replay_on_new_inputs_and_after_a_weight_edit():
    """A hipGraph captured on input A and replayed on input B equals the eager call on B; after an in-place edit of every parameter,
    refresh_images() (outside the graph) makes the replay show the new weights - images and folded constants keep their addresses."""
    m, bn = _pack(256, 256, 2).to(DEV), _bn(256).to(DEV)
    a, b = _rand(N, 256, 26, 37, seed=50).to(DEV), _rand(N, 256, 26, 37, seed=51).to(DEV)
    static = a.clone()
    with torch.no_grad():
        m.forward_bn_relu(static, bn)                                        # eager once: the images exist
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode='thread_local'):
            out = m.forward_bn_relu(static, bn)
        static.copy_(b)
        graph.replay()
        assert torch.equal(out, m.forward_bn_relu(b, bn))
        before = out.clone()
        for p in list(m.parameters()) + list(bn.parameters()):
            p.mul_(0.5)                                                      # in place: the version counters move
        m.refresh_images()
        graph.replay()
        assert torch.equal(out, m.forward_bn_relu(b, bn))
        assert not torch.equal(out, before)
    torch.cuda.synchronize()


def test_bottleneck_with_dcn_against_its_torch_route():
    import graph_detr4d_amd as G
    from graph_detr4d_amd import functional as Fn
    torch.manual_seed(60)
    blk = G.Bottleneck(1024, 256, stride=1, norm_cfg=dict(type='BN', requires_grad=False), dcn=dict(type='DCNv2', deform_groups=1,
                                                                                                  fallback_on_stride=False)).eval()
    with torch.no_grad():
        blk.conv2.conv_offset.weight.normal_(std=2.0 * (9 * 256) ** -0.5)
        blk.conv2.conv_offset.bias.normal_(std=0.5)
        for bn in (blk.bn1, blk.bn2, blk.bn3):
            bn.running_mean.normal_(std=0.3)
            bn.running_var.uniform_(0.5, 2.0)
            bn.weight.normal_(mean=1.0, std=0.3)
            bn.bias.normal_(std=0.3)
    blk = blk.to(DEV)
    x = _rand(N, 1024, 13, 21, seed=61).to(DEV)
    with torch.no_grad():
        out = blk(x)
        with Fn.torch_ops_for(blk.conv2):
            want = blk(x)
    err = R.rel_err(out, want.cpu())
    print(f'Bottleneck with DCN against its torch-op route: rel_err {err:.3e}')
    assert tuple(out.shape) == (N, 1024, 13, 21) and err <= MODULE_TOL
