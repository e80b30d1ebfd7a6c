"""Training of the FPN neck on the library's kernels (fpn.py hip_train=True; gd4d_fpn_train.hip, the two dgrad kinds of gd4d_fpn.hip)
against the fp64 backward (fpn_train_ref.py) and the modules' own torch-op route.  GPU only.

Shapes as in test_fpn_gpu.py: N = 2 cameras, levels (13, 21), (7, 11), (4, 6); loss sum_k (out_k * r_k).sum() with fixed random r_k.
Tolerances are the project's: 1e-4 of a gradient map's largest |entry| per kernel (KERNEL_TOL), 1e-3 relative Frobenius
per module (BWD_TOL of test_depth_net_train_gpu.py).  Every measured error is printed."""
import functools

import pytest
import torch

import fpn_ref as R
import fpn_train_ref as T
from test_fpn_gpu import CPFPN_CFG, FPN_CFG, LEVELS, N, _inputs, _module, _rand

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
KERNEL_TOL, BWD_TOL, MASK_BAND, MASK_SHARE = 1e-4, 1e-3, 2e-4, 1e-3


def _d(t):
    return t.to(DEV).contiguous()


# ---- 1. kernel level ------------------------------------------------------------------------------------------------------
LATERAL_CASES = [(32, N, (13, 21)), (96, N, (13, 21)), (160, N, (7, 11)), (2048, N, (4, 6)), (96, 3, (1, 2))]


@functools.lru_cache(maxsize=None)
def _lateral_case(cin, n, hw):
    g, x = _rand(n, 256, *hw, seed=300 + cin), _rand(n, cin, *hw, seed=301 + cin)
    w = _rand(256, cin, seed=302 + cin, scale=cin ** -0.5)
    dx = torch.einsum('ok,nohw->nkhw', w.double(), g.double())
    dw = torch.einsum('nohw,nkhw->ok', g.double(), x.double())
    return g, x, w, dx, dw, g.double().sum((0, 2, 3))


@pytest.mark.parametrize('cin, n, hw', LATERAL_CASES)
def test_lateral_dgrad_and_wgrad_against_fp64(cin, n, hw):
    """Cin = 32 / 96: a ragged channel block (dgrad) and a half-empty 64-channel chunk (wgrad); 546 = 2 x 273 pixels: a pixel tail and
    fewer tiles than default partitions; Cin = 2048 on (4, 6): eight channel blocks, 32 chunks; N = 3 on (1, 2): two-pixel tiles."""
    from graph_detr4d_amd import ops
    g, x, w, dx, dw, db = _lateral_case(cin, n, hw)
    got_dx = ops.fpn_lateral_dgrad(_d(g), ops.fpn_lateral_image_t(_d(w)), cin)
    got_dw, got_db = ops.fpn_lateral_wgrad(_d(g), _d(x))
    assert tuple(got_dx.shape) == tuple(x.shape) and tuple(got_dw.shape) == (256, cin, 1, 1) and tuple(got_db.shape) == (256,)
    errs = R.rel_err(got_dx, dx), R.rel_err(got_dw.reshape(256, cin), dw), R.rel_err(got_db, db)
    print(f'lateral Cin = {cin} N = {n} {hw}: dgrad {errs[0]:.2e}, wgrad {errs[1]:.2e}, bias {errs[2]:.2e}')
    assert max(errs) <= KERNEL_TOL


def test_lateral_wgrad_partitions():
    """One partition against the default count: the same sum in another association (1e-6 relative Frobenius); each bit-equal to
    itself across two runs; more partitions than tiles (the empty ones write zeros)."""
    from graph_detr4d_amd import ops
    g, x, _, _, dw, _ = _lateral_case(96, N, (13, 21))
    g, x = _d(g), _d(x)
    a, b = ops.fpn_lateral_wgrad(g, x, partitions=1), ops.fpn_lateral_wgrad(g, x)
    many = ops.fpn_lateral_wgrad(g, x, partitions=37)                          # 10 tiles
    for u, v in zip(ops.fpn_lateral_wgrad(g, x, partitions=1) + ops.fpn_lateral_wgrad(g, x), a + b):
        assert torch.equal(u, v)
    e_w, e_b, e_m = T.rel_fro(a[0], b[0].cpu()), T.rel_fro(a[1], b[1].cpu()), T.rel_fro(many[0], b[0].cpu())
    print(f'lateral wgrad partitions 1 vs default: dW {e_w:.2e}, db {e_b:.2e}; 37 vs default: {e_m:.2e}')
    assert e_w <= 1e-6 and e_b <= 1e-6 and e_m <= 1e-6
    assert R.rel_err(many[0].reshape(256, 96), dw) <= KERNEL_TOL


@pytest.mark.parametrize('fine, coarse', [((13, 21), (7, 11)), ((7, 11), (4, 6)), ((8, 12), (4, 6)), ((13, 21), (4, 6))])
def test_topdown_adjoint(fine, coarse):
    from graph_detr4d_amd import ops
    gf, gc = _rand(N, 256, *fine, seed=400), _rand(N, 256, *coarse, seed=401)
    ref = gc.double() + T.upsample_adjoint(gf, coarse)
    buf = _d(gc)
    got = ops.fpn_topdown_bwd(_d(gf), buf)
    assert got.data_ptr() == buf.data_ptr()                                    # in place
    err = R.rel_err(got, ref)
    print(f'top-down adjoint {fine} -> {coarse}: {err:.2e}')
    assert err <= KERNEL_TOL
    gi = torch.randint(-8, 9, gf.shape, generator=torch.Generator().manual_seed(402)).float()
    ci = torch.randint(-8, 9, gc.shape, generator=torch.Generator().manual_seed(403)).float()
    exact = ci.double() + T.upsample_adjoint(gi, coarse)
    assert torch.equal(ops.fpn_topdown_bwd(_d(gi), _d(ci)).cpu().double(), exact)   # integers: exact


@functools.lru_cache(maxsize=None)
def _extra_case(hw, relu_in):
    ho, wo = (hw[0] + 1) // 2, (hw[1] + 1) // 2
    x, w, dy = _rand(N, 256, *hw, seed=500), _rand(256, 256, 3, 3, seed=501, scale=2304 ** -0.5), _rand(N, 256, ho, wo, seed=502)
    add = _rand(N, 256, *hw, seed=503)
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    b64 = torch.zeros(256, dtype=torch.float64, requires_grad=True)
    (R.conv3x3(x64, w64, b64, stride=2, relu_in=relu_in) * dy.double()).sum().backward()
    return x, w, dy, add, x64.grad, w64.grad, b64.grad


@pytest.mark.parametrize('hw, relu_in', [((4, 6), False), ((2, 3), True), ((5, 7), False), ((13, 21), True)])
def test_extra_conv_dgrad_and_wgrad_against_fp64(hw, relu_in):
    """(4, 6) -> (2, 3); (2, 3) -> (1, 2) with the ReLU mask; an odd input (5, 7) -> (3, 4); (13, 21) -> (7, 11): a second tile."""
    from graph_detr4d_amd import ops
    x, w, dy, add, dx, dw, db = _extra_case(hw, relu_in)
    img_t = ops.depth_net_image_t(_d(w))
    got_dx = ops.fpn_extra_conv_dgrad(_d(dy), img_t, hw, mask=_d(x) if relu_in else None)
    got_sum = ops.fpn_extra_conv_dgrad(_d(dy), img_t, hw, mask=_d(x) if relu_in else None, add=_d(add))
    got_dw, got_db = ops.fpn_extra_conv_wgrad(_d(dy), _d(x), relu_in=relu_in)
    errs = R.rel_err(got_dx, dx), R.rel_err(got_dw, dw), R.rel_err(got_db, db)
    print(f'extra conv {hw} relu_in={relu_in}: dgrad {errs[0]:.2e}, wgrad {errs[1]:.2e}, bias {errs[2]:.2e}')
    assert max(errs) <= KERNEL_TOL
    assert torch.equal(got_sum, _d(add) + got_dx)                             # the fused add is torch's add
    if relu_in:
        assert bool((got_dx[_d(x) <= 0] == 0).all())                           # nothing passes where the forward's ReLU cut


def test_conv3x3_dgrad_all_levels_in_one_launch():
    """The stride-1 input gradient is gd4d_fpn_conv_fwd on the transposed, tap-flipped images: against fp64, and one launch over the
    three levels bit-equal to one launch per level."""
    from graph_detr4d_amd import ops
    dys = [_rand(N, 256, h, w, seed=600 + i) for i, (h, w) in enumerate(LEVELS)]
    ws = [_rand(256, 256, 3, 3, seed=610 + i, scale=2304 ** -0.5) for i in range(len(LEVELS))]
    imgs = [ops.depth_net_image_t(_d(w)) for w in ws]
    together = ops.fpn_conv_fwd([_d(d) for d in dys], imgs, [None] * len(dys))
    for lvl, (dy, w, img, got) in enumerate(zip(dys, ws, imgs, together)):
        x64 = torch.zeros(dy.shape, dtype=torch.float64, requires_grad=True)
        (R.conv3x3(x64, w) * dy.double()).sum().backward()
        err = R.rel_err(got, x64.grad)
        print(f'conv3x3 dgrad level {lvl}: {err:.2e}')
        assert err <= KERNEL_TOL
        assert torch.equal(ops.fpn_conv_fwd([_d(dy)], [img], [None])[0], got)


def test_bias_grad_against_fp64():
    from graph_detr4d_amd import ops
    g = _rand(N, 256, 13, 21, seed=700)
    got = ops.fpn_bias_grad(_d(g))
    err = R.rel_err(got, g.double().sum((0, 2, 3)))
    print(f'bias grad (13, 21): {err:.2e}')
    assert err <= KERNEL_TOL and torch.equal(got, ops.fpn_bias_grad(_d(g)))


# ---- 2. module level ------------------------------------------------------------------------------------------------------
def _rs(cfg):
    sizes = list(LEVELS)
    while len(sizes) < cfg['num_outs']:
        sizes.append(((sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2))
    return [_rand(N, 256, *s, seed=800 + i) for i, s in enumerate(sizes)]


def _step(mod, xs, rs, grad_inputs=True):
    s = mod.start_level
    xg = [x.to(DEV).requires_grad_(grad_inputs and i >= s) for i, x in enumerate(xs)]
    outs = mod(xg)
    sum((o * r.to(DEV)).sum() for o, r in zip(outs, rs)).backward()
    return outs, xg


@functools.lru_cache(maxsize=None)
def _module_case(name):
    """One hip_train step in train() mode, its torch-op twin and the fp64 backward with the device's ReLU mask; computed once."""
    cfg = FPN_CFG if name == 'FPN' else CPFPN_CFG
    xs, rs = _inputs(cfg), _rs(cfg)
    mod = _module(cfg, hip_train=True)
    sd = {k: v.detach().cpu().clone() for k, v in mod.state_dict().items()}
    with torch.no_grad():
        infer = [o.clone() for o in mod([x.to(DEV) for x in xs])]            # eval(): the inference kernels
    outs, xg = _step(mod.train(), xs, rs)
    twin = _module(cfg, torch_ops=True)
    twin.load_state_dict(sd)
    _, xt = _step(twin.train(), xs, rs)
    ref_cfg = dict(start_level=cfg['start_level'], num_outs=cfg['num_outs'], relu_before_extra_convs=True, cp=name == 'CPFPN')
    masks = {3: outs[3].detach().cpu() > 0} if name == 'FPN' else None
    o64, p64, x64 = T.backward(sd, xs, rs, relu_masks=masks, **ref_cfg)
    o64_free = T.forward({k: v.double() for k, v in sd.items()}, [x.double() for x in xs], **ref_cfg)
    return dict(cfg=cfg, xs=xs, rs=rs, mod=mod, sd=sd, infer=infer, outs=[o.detach() for o in outs], xg=xg, twin=twin, xt=xt, p64=p64,
                x64=x64, o64=o64_free, grads={k: p.grad.clone() for k, p in mod.named_parameters()})


@pytest.mark.parametrize('name', ['FPN', 'CPFPN'])
def test_module_trains_on_the_kernels(name):
    c = _module_case(name)
    for a, b in zip(c['outs'], c['infer']):
        assert torch.equal(a, b)                                               # the node's forward is the inference kernels' bits
    s = c['cfg']['start_level']
    for k, p in c['twin'].named_parameters():
        e64, etor = T.rel_fro(c['grads'][k], c['p64'][k]), T.rel_fro(c['grads'][k], p.grad.cpu())
        print(f'{name} d {k}: vs fp64 {e64:.2e}, vs torch route {etor:.2e}')
        assert c['grads'][k].shape == p.shape and e64 <= BWD_TOL and etor <= BWD_TOL, k
    for i, (x, t, r) in enumerate(zip(c['xg'], c['xt'], c['x64'])):
        if i < s:
            assert x.grad is None and r is None                                # below start_level: not read, no gradient
            continue
        e64, etor = T.rel_fro(x.grad, r), T.rel_fro(x.grad, t.grad.cpu())
        print(f'{name} d input {i}: vs fp64 {e64:.2e}, vs torch route {etor:.2e}')
        assert x.grad.shape == x.shape and e64 <= BWD_TOL and etor <= BWD_TOL


def test_relu_mask_of_the_device_forward_is_the_fp64_mask_but_for_a_band():
    c = _module_case('FPN')
    dev_map, ref_map = c['outs'][3].cpu().double(), c['o64'][3]
    differ = (dev_map > 0) != (ref_map > 0)
    band = MASK_BAND * float(ref_map.abs().max())
    count, worst = int(differ.sum()), float(ref_map[differ].abs().max()) if bool(differ.any()) else 0.0
    print(f'ReLU mask: {count} of {differ.numel()} entries differ from the fp64 mask, the largest |fp64 entry| among them {worst:.2e} '
          f'(band {band:.2e}); fp64 entries inside the band: {int((ref_map.abs() <= band).sum())}')
    assert differ.numel() == 3072 and worst <= band and count <= MASK_SHARE * differ.numel()


def test_levels_that_need_no_gradient():
    c = _module_case('FPN')
    cfg, xs, rs = c['cfg'], c['xs'], c['rs']
    mod = _module(cfg, hip_train=True)
    mod.load_state_dict(c['sd'])
    _, xg = _step(mod, xs, rs, grad_inputs=False)                              # eval(), autograd on: parameters require grad
    assert all(x.grad is None for x in xg)
    for k, p in mod.named_parameters():
        assert torch.equal(p.grad, c['grads'][k]), k                           # ... and are the train() step's, bit for bit
    frozen = _module(cfg, hip_train=True)
    frozen.load_state_dict(c['sd'])
    for p in frozen.parameters():
        p.requires_grad_(False)
    _, xf = _step(frozen, xs, rs)
    assert all(p.grad is None for p in frozen.parameters())
    for i, (a, b) in enumerate(zip(xf, c['xg'])):
        assert (a.grad is None and b.grad is None) if i < cfg['start_level'] else torch.equal(a.grad, b.grad)
    # one frozen lateral, one input without grad: only those two gradients are missing
    part = _module(cfg, hip_train=True)
    part.load_state_dict(c['sd'])
    part.lateral_convs[1].conv.weight.requires_grad_(False)
    xp = [x.to(DEV).requires_grad_(i in (1, 3)) for i, x in enumerate(xs)]
    sum((o * r.to(DEV)).sum() for o, r in zip(part(xp), rs)).backward()
    assert part.lateral_convs[1].conv.weight.grad is None and xp[2].grad is None
    assert torch.equal(part.lateral_convs[1].conv.bias.grad, c['grads']['lateral_convs.1.conv.bias'])
    assert torch.equal(xp[1].grad, c['xg'][1].grad) and torch.equal(xp[3].grad, c['xg'][3].grad)


def test_gradients_accumulate_and_repeat():
    c = _module_case('FPN')
    mod = _module(c['cfg'], hip_train=True)
    mod.load_state_dict(c['sd'])
    _, x1 = _step(mod.train(), c['xs'], c['rs'])
    for k, p in mod.named_parameters():
        assert torch.equal(p.grad, c['grads'][k]), k                           # two runs, two modules: the same bits
    for a, b in zip(x1, c['xg']):
        assert (a.grad is None and b.grad is None) or torch.equal(a.grad, b.grad)
    _step(mod, c['xs'], c['rs'])
    for k, p in mod.named_parameters():
        assert torch.equal(p.grad, c['grads'][k] + c['grads'][k]), k           # a second backward adds to .grad


@pytest.mark.parametrize('name', ['FPN', 'CPFPN'])
def test_channels_last_outputs_give_the_same_gradients(name):
    c = _module_case(name)
    mod = _module(c['cfg'], hip_train=True, channels_last_out=True)
    mod.load_state_dict(c['sd'])
    outs, xg = _step(mod.train(), c['xs'], c['rs'])
    for a, b in zip(outs, c['outs']):
        assert a.permute(0, 2, 3, 1).is_contiguous() and torch.equal(a, b)
    for k, p in mod.named_parameters():
        assert torch.equal(p.grad, c['grads'][k]), k
    for a, b in zip(xg, c['xg']):
        assert (a.grad is None and b.grad is None) or torch.equal(a.grad, b.grad)
