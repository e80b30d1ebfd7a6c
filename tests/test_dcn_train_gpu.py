"""DCNv2 training on the library's kernels (gd4d_dcn_train.hip, dcn.py's hip_train) against fp64 autograd through dcn_ref (the arbiter:
floor-based corners, the right derivative at integer sample coordinates - never grid_sample).  GPU only.

N = 2 images; the shapes are the smallest that take each path (see each list).  Tolerances: KERNEL_TOL = 1e-4 of a gradient map's
largest |entry| per kernel, BWD_TOL = 1e-3 relative Frobenius per module.  dX is accumulated with float atomics: it is the one output
compared between two runs with a tolerance instead of bit for bit."""
import copy
import functools

import pytest
import torch
import torch.nn as nn

import dcn_ref as R
import dcn_train_ref as T

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
N = 2
KERNEL_TOL, BWD_TOL = 1e-4, 1e-3
# (cin, cout, stride, h, w): one chunk and one ragged tile; a second tile, ragged; stride 2 with an odd output and the last tap off
# the image; the 32-pixel-tile geometry (Cout > 256); both together; output channels below the forward's padding
KERNEL_CASES = [(64, 64, 1, 5, 7), (256, 256, 1, 13, 21), (256, 256, 2, 26, 37), (512, 512, 1, 13, 21), (256, 512, 2, 26, 37),
                (64, 128, 1, 5, 7)]
CRAFTED_CASES = [(256, 256, 1, 5, 7), (256, 256, 2, 26, 37), (512, 512, 1, 5, 7)]
PLANES = {'zero', 'integers', 'at_minus_1', 'at_h_minus_1', 'at_h_and_w', 'plus_1000', 'minus_1000', 'corner_tl', 'corner_tr', 'corner_bl',
          'corner_br'}


def _rand(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


@functools.lru_cache(maxsize=None)
def _kernel_case(cin, cout, stride, h, w):
    """Inputs (offsets normal with sigma = 2 px, modulations uniform in (0, 1)), a `y` whose sign is the ReLU mask, and the two fp64
    references (plain; scale + mask); computed once."""
    ho, wo = R.out_hw(h, w, stride)
    x = _rand(N, cin, h, w, seed=1)
    weight = _rand(cout, cin, 3, 3, seed=2, scale=(9 * cin) ** -0.5)
    offset = _rand(N, 18, ho, wo, seed=3, scale=2.0)
    mask = torch.rand(N, 9, ho, wo, generator=torch.Generator().manual_seed(4))
    dout, y, scale = _rand(N, cout, ho, wo, seed=5), _rand(N, cout, ho, wo, seed=6), _rand(cout, seed=7) + 1.5
    plain = T.autograd(x, offset, mask, weight, dout, stride)
    masked = T.autograd(x, offset, mask, weight, dout, stride, scale, y > 0)
    return x, weight, offset, mask, dout, y, scale, plain, masked


def _run_kernels(x, weight, offset, mask, dout, stride, y=None, scale=None, sigmoid_grad=False, partitions=None):
    from graph_detr4d_amd import ops
    d = lambda t: None if t is None else t.to(DEV)                                                               # noqa: E731
    om = torch.cat((offset, mask), dim=1).to(DEV)
    image_t = ops.dcn_weight_image_t(weight.to(DEV))
    dx, doff = ops.dcn_bwd_data(d(dout), d(x), om, image_t, weight.shape[0], stride=stride, y=d(y), scale=d(scale), sigmoid_grad=sigmoid_grad)
    dw, db = ops.dcn_wgrad(d(dout), d(x), om, weight.shape[0], stride=stride, y=d(y), scale=d(scale), partitions=partitions)
    torch.cuda.synchronize()
    return dict(x=dx, doff=doff, weight=dw, bias=db)


def _check(got, ref, what, tol=KERNEL_TOL):
    errs = dict(x=R.rel_err(got['x'], ref['x']), doff=R.rel_err(got['doff'], torch.cat((ref['offset'], ref['mask']), dim=1)),
                offset=R.rel_err(got['doff'][:, :18], ref['offset']), mask=R.rel_err(got['doff'][:, 18:], ref['mask']),
                weight=R.rel_err(got['weight'], ref['weight']), bias=R.rel_err(got['bias'], ref['bias']))
    print(f'{what}: ' + ', '.join(f'{k} {v:.3e}' for k, v in errs.items()))
    assert all(v <= tol for v in errs.values()), (what, errs)


# ---- 1. kernels ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', KERNEL_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_dcn_backward_kernels_against_fp64(case):
    cin, cout, stride, h, w = case
    x, weight, offset, mask, dout, y, scale, plain, masked = _kernel_case(*case)
    _check(_run_kernels(x, weight, offset, mask, dout, stride), plain, f'dcn backward {case} plain')
    # the ReLU mask is the y handed to the kernel, and the same y > 0 went to the reference: no entry is excluded
    _check(_run_kernels(x, weight, offset, mask, dout, stride, y=y, scale=scale), masked, f'dcn backward {case} scale + relu')


@pytest.mark.parametrize('case', CRAFTED_CASES, ids=lambda c: 'x'.join(map(str, c)))
def test_dcn_backward_kernels_crafted_offsets(case):
    """One image per crafted plane.  `zero` and `integers` are the convention test: every sample coordinate is an integer."""
    cin, cout, stride, h, w = case
    planes = R.crafted_offsets(h, w, stride)
    names = list(planes)
    assert PLANES == set(names)                                            # no plane may be skipped
    ho, wo = R.out_hw(h, w, stride)
    x = _rand(1, cin, h, w, seed=11).expand(len(names), -1, -1, -1).contiguous()
    weight = _rand(cout, cin, 3, 3, seed=12, scale=(9 * cin) ** -0.5)
    offset = torch.cat([planes[k] for k in names])
    mask = torch.rand(len(names), 9, ho, wo, generator=torch.Generator().manual_seed(13))
    dout = _rand(len(names), cout, ho, wo, seed=14)
    ref = T.autograd(x, offset, mask, weight, dout, stride)
    got = _run_kernels(x, weight, offset, mask, dout, stride)
    got = {k: v.cpu() for k, v in got.items()}
    maps = dict(x=(got['x'], ref['x']), offset=(got['doff'][:, :18], ref['offset']), mask=(got['doff'][:, 18:], ref['mask']))
    for i, name in enumerate(names):
        for key, (g, r) in maps.items():
            if float(r[i].abs().max()) == 0.0:                              # exactly zero in the reference: exactly zero here
                print(f'dcn backward {case} {name} {key}: reference is zero, max |got| {float(g[i].abs().max()):.3e}')
                assert float(g[i].abs().max()) == 0.0, (name, key)
            else:
                err = R.rel_err(g[i], r[i])
                print(f'dcn backward {case} {name} {key}: rel_err {err:.3e}')
                assert err <= KERNEL_TOL, (name, key, err)
        if name in ('plus_1000', 'minus_1000', 'at_h_and_w'):
            assert all(float(r[i].abs().max()) == 0.0 for _, r in maps.values()), name
        if name == 'at_minus_1':
            assert float(ref['offset'][i].abs().max()) == 0.0
    for key in ('weight', 'bias'):
        err = R.rel_err(got[key], ref[key])
        print(f'dcn backward {case} all planes {key}: rel_err {err:.3e}')
        assert err <= KERNEL_TOL, key


@functools.lru_cache(maxsize=None)
def _offset_conv_case(cin, stride, h, w, integers):
    ho, wo = R.out_hw(h, w, stride)
    if integers:
        g = torch.Generator().manual_seed(21)
        x = torch.randint(-3, 4, (N, cin, h, w), generator=g).float()
        weight = torch.randint(-2, 3, (27, cin, 3, 3), generator=g).float()
        do = torch.randint(-3, 4, (N, 27, ho, wo), generator=g).float()
    else:
        x, weight, do = _rand(N, cin, h, w, seed=22), _rand(27, cin, 3, 3, seed=23, scale=(9 * cin) ** -0.5), _rand(N, 27, ho, wo, seed=24)
    xx, ww, bb = x.double().requires_grad_(True), weight.double().requires_grad_(True), torch.zeros(27, dtype=torch.float64, requires_grad=True)
    (torch.nn.functional.conv2d(xx, ww, bb, stride=stride, padding=1) * do.double()).sum().backward()
    return x, weight, do, xx.grad, ww.grad, bb.grad


@pytest.mark.parametrize('case', [(64, 1, 5, 7), (256, 1, 5, 7), (512, 1, 5, 7), (64, 2, 26, 37), (256, 2, 26, 37), (512, 2, 26, 37)],
                         ids=lambda c: 'x'.join(map(str, c)))
def test_offset_conv_backward_kernels_against_fp64(case):
    from graph_detr4d_amd import ops
    cin, stride, h, w = case
    for integers in (False, True):
        x, weight, do, rx, rw, rb = _offset_conv_case(*case, integers)
        base = _rand(N, cin, h, w, seed=25) if not integers else torch.ones(N, cin, h, w)
        dx = ops.dcn_offset_conv_dgrad(do.to(DEV), weight.to(DEV), base.to(DEV).clone(), stride=stride)      # ADDED into dx
        dw, db = ops.dcn_offset_conv_wgrad(do.to(DEV), x.to(DEV), stride=stride)
        torch.cuda.synchronize()
        if integers:                                                        # small integers: every product and sum is exact
            assert torch.equal(dx.cpu().double(), rx + 1.0) and torch.equal(dw.cpu().double(), rw) and torch.equal(db.cpu().double(), rb)
        else:
            errs = (R.rel_err(dx.cpu().double() - base.double(), rx), R.rel_err(dw, rw), R.rel_err(db, rb))
            print(f'conv_offset backward {case}: dgrad {errs[0]:.3e}, dW_off {errs[1]:.3e}, db_off {errs[2]:.3e}')
            assert all(e <= KERNEL_TOL for e in errs), errs


def test_two_runs_only_dx_comes_from_atomics():
    """Every output has a fixed summation order except dX, the float atomics' output: bit for bit / 1e-6 relative Frobenius."""
    from graph_detr4d_amd import ops
    case = (256, 256, 2, 26, 37)
    x, weight, offset, mask, dout, y, scale, _, _ = _kernel_case(*case)
    off_w = _rand(27, 256, 3, 3, seed=31, scale=(9 * 256) ** -0.5).to(DEV)
    runs = []
    for _ in range(2):
        got = _run_kernels(x, weight, offset, mask, dout, 2, y=y, scale=scale, sigmoid_grad=True)
        got['off_weight'], got['off_bias'] = ops.dcn_offset_conv_wgrad(got['doff'], x.to(DEV), stride=2)
        got['x_offset_term'] = ops.dcn_offset_conv_dgrad(got['doff'], off_w, torch.zeros_like(got['x']), stride=2)
        torch.cuda.synchronize()
        runs.append(got)
    for key in ('doff', 'weight', 'bias', 'off_weight', 'off_bias', 'x_offset_term'):
        assert torch.equal(runs[0][key], runs[1][key]), key
    err = T.rel_fro(runs[0]['x'], runs[1]['x'].cpu())
    print(f'dX (atomics) between two runs: relative Frobenius {err:.3e}')
    assert err <= 1e-6


def test_weight_gradient_partitions():
    from graph_detr4d_amd import ops
    case = (256, 256, 1, 13, 21)
    x, weight, offset, mask, dout, y, scale, plain, _ = _kernel_case(*case)
    om = torch.cat((offset, mask), dim=1).to(DEV)
    xd, dd = x.to(DEV), dout.to(DEV)
    do = _rand(N, 27, 13, 21, seed=41).to(DEV)
    xx, ww = x.double(), torch.zeros(27, 256, 3, 3, dtype=torch.float64, requires_grad=True)
    bb = torch.zeros(27, dtype=torch.float64, requires_grad=True)
    (torch.nn.functional.conv2d(xx, ww, bb, padding=1) * do.cpu().double()).sum().backward()
    tiles = N * ((13 * 21 + 63) // 64)
    results = {}
    for parts in (1, None, tiles + 6):                                      # more partitions than tiles: the extra ones write zeros
        a, b = ops.dcn_wgrad(dd, xd, om, 256, partitions=parts), ops.dcn_offset_conv_wgrad(do, xd, partitions=parts)
        a2, b2 = ops.dcn_wgrad(dd, xd, om, 256, partitions=parts), ops.dcn_offset_conv_wgrad(do, xd, partitions=parts)
        torch.cuda.synchronize()
        assert all(torch.equal(u, v) for u, v in zip(a + b, a2 + b2)), parts
        errs = (R.rel_err(a[0], plain['weight']), R.rel_err(a[1], plain['bias']), R.rel_err(b[0], ww.grad), R.rel_err(b[1], bb.grad))
        print(f'partitions {parts}: dW {errs[0]:.3e}, dbias {errs[1]:.3e}, dW_off {errs[2]:.3e}, db_off {errs[3]:.3e}')
        assert all(e <= KERNEL_TOL for e in errs), (parts, errs)
        results[parts] = a + b
    for parts in (None, tiles + 6):
        for u, v in zip(results[1], results[parts]):
            assert T.rel_fro(v, u.cpu()) <= 1e-6, parts


# ---- 2. modules ------------------------------------------------------------------------------------------------------------
def _pack(seed=50, randomise=True, cin=256, cout=256, stride=2):
    import graph_detr4d_amd as G
    torch.manual_seed(seed)
    m = G.ModulatedDeformConv2dPack(cin, cout, 3, stride=stride, padding=1, bias=False, hip_train=True)
    if randomise:
        with torch.no_grad():
            m.conv_offset.weight.normal_(std=2.0 * (9 * cin) ** -0.5)
            m.conv_offset.bias.normal_(std=0.5)
    return m.train()


def _bn(c, seed=51):
    torch.manual_seed(seed)
    bn = nn.BatchNorm2d(c).eval()
    with torch.no_grad():
        bn.running_mean.normal_(std=0.3)
        bn.running_var.uniform_(0.5, 2.0)
        bn.weight.normal_(mean=1.0, std=0.3)
        bn.bias.normal_(std=0.3)
    for p in bn.parameters():
        p.requires_grad = False
    return bn


def _bn_scale(bn):
    return (bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)).cpu()


def _pack_step(m, bn, x, r):
    for p in m.parameters():
        p.grad = None
    xd = x.to(DEV).requires_grad_(True)
    out = m.forward_bn_relu(xd, bn)
    (out * r.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return out.detach(), xd.grad


@pytest.mark.parametrize('fresh', [False, True], ids=['random_conv_offset', 'fresh_zero_conv_offset'])
def test_pack_trains_behind_a_frozen_batchnorm(fresh):
    """train() mode, forward_bn_relu, loss (out * r).sum().  The fresh Pack has conv_offset zero: every offset is exactly 0, and
    conv_offset's gradients must follow the right-derivative convention of the fp64 reference."""
    m, bn = _pack(randomise=not fresh), _bn(256)
    x, r = _rand(N, 256, 26, 37, seed=52), _rand(N, 256, 13, 19, seed=53)
    off, _ = R.offset_conv_ref(x, m.conv_offset.weight.detach(), m.conv_offset.bias.detach(), 2)
    std = float(off.std())
    print(f'offsets: standard deviation {std:.3f} px')
    assert (std == 0.0 and float(off.abs().max()) == 0.0) if fresh else 0.5 <= std <= 3.0
    scale = _bn_scale(bn)
    m, bn = m.to(DEV), bn.to(DEV)
    out, dx = _pack_step(m, bn, x, r)
    assert float((out == 0).float().mean()) > 0.2
    ref = T.autograd_pack(x, m.weight.detach().cpu(), m.conv_offset.weight.detach().cpu(), m.conv_offset.bias.detach().cpu(), r, 2, scale,
                          (out > 0).cpu())                                  # the ReLU mask of the HIP forward's own output
    errs = dict(x=T.rel_fro(dx, ref['x']), weight=T.rel_fro(m.weight.grad, ref['weight']),
                off_weight=T.rel_fro(m.conv_offset.weight.grad, ref['off_weight']), off_bias=T.rel_fro(m.conv_offset.bias.grad, ref['off_bias']))
    print(f'pack (fresh={fresh}): ' + ', '.join(f'{k} {v:.3e}' for k, v in errs.items()))
    assert float(ref['off_weight'].abs().max()) > 0 and all(v <= BWD_TOL for v in errs.values()), errs


def test_caller_supplied_offset_and_mask_gradients_to_all_five():
    import graph_detr4d_amd as G
    case = (256, 256, 1, 13, 21)
    x, weight, offset, mask, dout, _, _, plain, _ = _kernel_case(*case)
    m = G.ModulatedDeformConv2d(256, 256, 3, padding=1, bias=True, hip_train=True).train()
    with torch.no_grad():
        m.weight.copy_(weight)
    m = m.to(DEV)
    xs = [t.to(DEV).requires_grad_(True) for t in (x, offset, mask)]
    (m(*xs) * dout.to(DEV)).sum().backward()
    errs = dict(x=T.rel_fro(xs[0].grad, plain['x']), offset=T.rel_fro(xs[1].grad, plain['offset']), mask=T.rel_fro(xs[2].grad, plain['mask']),
                weight=T.rel_fro(m.weight.grad, plain['weight']), bias=T.rel_fro(m.bias.grad, plain['bias']))
    print('ModulatedDeformConv2d: ' + ', '.join(f'{k} {v:.3e}' for k, v in errs.items()))
    assert all(v <= BWD_TOL for v in errs.values()), errs


def test_frozen_parameters_dtype_and_refusals():
    from graph_detr4d_amd._lib import Gd4dError
    m, bn = _pack().to(DEV), _bn(256).to(DEV)
    x, r = _rand(N, 256, 26, 37, seed=52), _rand(N, 256, 13, 19, seed=53)
    _, dx = _pack_step(m, bn, x, r)
    full = dict(weight=m.weight.grad.clone(), off_w=m.conv_offset.weight.grad.clone(), off_b=m.conv_offset.bias.grad.clone())
    # a frozen weight: no gradient for it, the others unchanged bit for bit (dX apart: atomics)
    m.weight.requires_grad = False
    _, dx2 = _pack_step(m, bn, x, r)
    assert m.weight.grad is None and torch.equal(m.conv_offset.weight.grad, full['off_w']) and torch.equal(m.conv_offset.bias.grad, full['off_b'])
    assert T.rel_fro(dx2, dx.cpu()) <= 1e-6
    m.weight.requires_grad = True
    for p in m.conv_offset.parameters():
        p.requires_grad = False
    _, dx3 = _pack_step(m, bn, x, r)
    assert m.conv_offset.weight.grad is None and m.conv_offset.bias.grad is None and torch.equal(m.weight.grad, full['weight'])
    assert T.rel_fro(dx3, dx.cpu()) <= 1e-6
    for p in m.conv_offset.parameters():
        p.requires_grad = True
    # an fp16 input gets an fp16 gradient
    xh = x.to(DEV).half().requires_grad_(True)
    m.forward_bn_relu(xh, bn).sum().backward()
    assert xh.grad.dtype == torch.float16 and tuple(xh.grad.shape) == tuple(xh.shape)
    # a BatchNorm whose parameters require grad is refused, and the message names the other route
    bn.weight.requires_grad = True
    with pytest.raises(Gd4dError, match='torch_ops=True'):
        m.forward_bn_relu(x.to(DEV), bn)
    bn.weight.requires_grad = False
    # capture with gradients wanted is refused
    static = x.to(DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(Gd4dError, match='capture'):
        with torch.cuda.graph(graph, capture_error_mode='thread_local'):
            m.forward_bn_relu(static, bn)
    torch.cuda.synchronize()


# ---- 3. backbone -----------------------------------------------------------------------------------------------------------
def test_bottleneck_trains_against_its_torch_route_in_fp64():
    import graph_detr4d_amd as G
    torch.manual_seed(60)
    blk = G.Bottleneck(256, 64, stride=2, norm_cfg=dict(type='BN', requires_grad=False), hip_train=True,
                       downsample=nn.Sequential(nn.Conv2d(256, 256, 1, stride=2, bias=False), nn.BatchNorm2d(256)),
                       dcn=dict(type='DCNv2', deform_groups=1, fallback_on_stride=False)).train()
    with torch.no_grad():
        blk.conv2.conv_offset.weight.normal_(std=2.0 * (9 * 64) ** -0.5)      # random, non-zero: the offsets are not integers
        blk.conv2.conv_offset.bias.normal_(std=0.5)
        for bn in (b for b in blk.modules() if isinstance(b, nn.BatchNorm2d)):
            bn.eval()                                                        # norm_eval=True
            bn.running_mean.normal_(std=0.3)
            bn.running_var.uniform_(0.5, 2.0)
            bn.weight.normal_(mean=1.0, std=0.3)
            bn.bias.normal_(std=0.3)
            for p in bn.parameters():
                p.requires_grad = False
    ref = copy.deepcopy(blk).double()
    ref.conv2.torch_ops = True
    x, r = _rand(N, 256, 16, 16, seed=61), _rand(N, 256, 8, 8, seed=62)
    xr = x.double().requires_grad_(True)
    (ref(xr) * r.double()).sum().backward()
    blk = blk.to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    (blk(xd) * r.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    errs = {'input': T.rel_fro(xd.grad, xr.grad)}
    for (name, p), (_, q) in zip(blk.named_parameters(), ref.named_parameters()):
        if p.requires_grad:
            errs[name] = T.rel_fro(p.grad, q.grad)
        else:
            assert p.grad is None
    print('Bottleneck with DCN, hip_train against fp64 torch ops: ' + ', '.join(f'{k} {v:.3e}' for k, v in errs.items()))
    assert 'conv2.conv_offset.weight' in errs and all(v <= BWD_TOL for v in errs.values()), errs


def test_small_resnet_trains():
    """(BatchNorm parameters frozen as in every config - the folded epilogue needs that - and zero_init_residual off, so that the
    blocks' own convolutions see a gradient at initialisation.)"""
    import graph_detr4d_amd as G
    torch.manual_seed(70)
    r = G.ResNet(50, num_stages=2, strides=(1, 2), dilations=(1, 1), out_indices=(0, 1), dcn=dict(type='DCNv2'), stage_with_dcn=(False, True),
                 norm_cfg=dict(type='BN', requires_grad=False), zero_init_residual=False, hip_train=True).to(DEV).train()
    outs = r(_rand(N, 3, 64, 64, seed=71).to(DEV))
    assert [tuple(o.shape) for o in outs] == [(N, 256, 16, 16), (N, 512, 8, 8)]
    sum((o * o).sum() for o in outs).backward()
    torch.cuda.synchronize()
    for name, p in r.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, name
        else:
            assert p.grad is None, name
    assert any(n.endswith('conv_offset.weight') for n, p in r.named_parameters() if p.requires_grad)
