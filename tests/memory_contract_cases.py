"""The rows of the memory-contract tests and their fp64 references, computed once per process on the CPU with the reference modules
the families' own tests use.  test_memory_contract_gpu.py runs the kernels on them inside guarded buffers (guarded.py);
test_memory_contract_cpu.py checks on the references alone that every ReLU-bearing row exercises its ReLU and that every family has
an exact-tile and a tile-plus-one size.

Sizes: the smallest at which each tiling can go wrong - one pixel, one pixel short of a tile, exactly a tile, one pixel more.
Channels: the smallest count each weight-image packer takes, and one that needs a second row block."""
import functools

import torch

import dcn_ref
import dcn_train_ref
import fpn_ref
import fpn_train_ref
import resnet_cases
import resnet_ref
import vovnet_ref
import vovnet_train_ref
from depth_net_train_ref import forward64

N = 2
# 16 x 16 tiles (DN_T, DT_T, DCN_TW): the DepthNet conv, the FPN 3x3, the DCN kernels
T16 = [(1, 1), (16, 16), (17, 16), (16, 17), (1, 33)]
# 64 flat pixels (FPN_PX, DW_PX): the FPN lateral and its gradients, the DCN weight gradients
PX64 = [(1, 1), (7, 9), (8, 8), (5, 13)]
# 128 flat pixels (VV_PIX) and 8 x 16 output tiles (VV_TY x VV_TX): the VoVNet and ResNet convolutions
PX128 = [(1, 1), (1, 127), (8, 16), (3, 43)]
TILE8X16 = [(1, 1), (8, 16), (9, 17)]
# stride 2, input sizes: outputs (1, 1), (1, 1), (8, 16), (8, 16), (9, 17) - both input parities of an exact tile, and one pixel more
S2 = [(1, 1), (2, 2), (15, 31), (16, 32), (17, 33)]
# one launch over several levels: an exact level in the middle of the tile prefix table and a one-tile level last
MULTI = ((17, 16), (16, 16), (1, 1))
# family -> (pixels or (rows, columns) of a tile, the sizes of the family's rows as the OUTPUT map the tiling cuts)
TILINGS = {}


def rand(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def hw_id(hw):
    return f'{hw[0]}x{hw[1]}'


def out_hw(h, w, stride):
    return (h - 1) // stride + 1, (w - 1) // stride + 1


# ---- ResNet --------------------------------------------------------------------------------------------------------------------
_FLAGS = [(False, True), (True, True), (False, False), (True, False)]            # (identity, relu)
_CHANNELS = [(32, 32), (64, 64)]                                                 # one row block of 32, and a second


def _resnet_rows(taps, stride, sizes):
    rows = []
    for i, hw in enumerate(sizes):
        for j, (cin, cout) in enumerate(_CHANNELS):
            identity, relu = _FLAGS[(i + 2 * j) % 4]
            rows.append((taps, cin, cout, stride, identity, relu, *hw))
    return rows


# (taps, cin, cout, stride, identity, relu, h, w): the pointwise kernel walks 128 flat pixels, the 3x3 cuts 8 x 16 output tiles
RESNET_ROWS = _resnet_rows(1, 1, PX128) + _resnet_rows(1, 2, S2) + _resnet_rows(9, 1, TILE8X16) + _resnet_rows(9, 2, S2)
TILINGS['resnet'] = ((8, 16), [out_hw(r[6], r[7], r[3]) for r in RESNET_ROWS])


def resnet_id(r):
    return f'conv{"3x3" if r[0] == 9 else "1x1"}-' + resnet_cases.case_id(r[1:])


@functools.lru_cache(maxsize=None)
def resnet_case(taps, cin, cout, stride, identity, relu, h, w):
    """(x, weight, scale, shift, identity or None, the fp64 reference).  The seeds differ per row so that no two rows share an input."""
    k = 3 if taps == 9 else 1
    seed = 1000 + 7 * h + 3 * w + cin + stride
    x = rand(N, cin, h, w, seed=seed)
    weight = rand(cout, cin, k, k, seed=seed + 1, scale=(taps * cin) ** -0.5)
    scale, shift = resnet_cases.scale_shift(cout, seed + 2)
    ho, wo = out_hw(h, w, stride)
    ident = rand(N, cout, ho, wo, seed=seed + 4) if identity else None
    return x, weight, scale, shift, ident, resnet_ref.folded_conv_act(x, weight, scale, shift, stride, ident, relu)


# ---- VoVNet --------------------------------------------------------------------------------------------------------------------
# (cin, cout, stride, h, w)
VOV_CONV_ROWS = [(c, c, 1, *hw) for hw in TILE8X16 for c in (32, 64)] + [(c, c, 2, *hw) for hw in S2 for c in (32, 64)]
# (source channels, cout, h, w): one source and one row block; two sources and a second row block
VOV_OSA_ROWS = [(ch, co, *hw) for hw in PX128 for ch, co in (((32,), 32), ((64, 32), 64))]
# (channels, h, w)
VOV_ESE_ROWS = [(c, *hw) for hw in PX128 for c in (32, 64)]
TILINGS['vovnet'] = ((8, 16), [out_hw(r[3], r[4], r[2]) for r in VOV_CONV_ROWS] + [r[2:] for r in VOV_OSA_ROWS])


def bn(c, seed):
    """test_vovnet_train_gpu._bn's statistics: gamma, beta, running mean, running var."""
    g = torch.Generator().manual_seed(seed)
    return (1.0 + 0.25 * (torch.rand(c, generator=g) - 0.5), 0.5 * torch.randn(c, generator=g), 0.2 * torch.randn(c, generator=g),
            0.75 + 0.5 * torch.rand(c, generator=g))


@functools.lru_cache(maxsize=None)
def vov_conv_case(cin, cout, stride, h, w):
    """Forward: (x, weight, scale, shift, ref); and for stride 1 the training half: bn, dz, the (dW, dgamma, dbeta) references."""
    seed = 2000 + 7 * h + 3 * w + cin + stride
    x = torch.relu(rand(N, cin, h, w, seed=seed))
    weight = rand(cout, cin, 3, 3, seed=seed + 1, scale=(2.0 / (9 * cin)) ** 0.5)
    scale, shift = resnet_cases.scale_shift(cout, seed + 2)
    c = dict(x=x, weight=weight, scale=scale, shift=shift, ref=vovnet_ref.folded_conv_relu(x, weight, scale, shift, stride))
    if stride == 1:
        stats = bn(cout, seed + 4)
        dz = rand(N, cout, h, w, seed=seed + 5) * (rand(N, cout, h, w, seed=seed + 6) > 0)
        c.update(bn=stats, dz=dz, grads=vovnet_train_ref.conv_param_grads(dz.double(), x.double(), weight, *stats))
    return c


@functools.lru_cache(maxsize=None)
def vov_osa_case(chans, cout, h, w):
    seed = 3000 + 7 * h + 3 * w + cout
    srcs = [torch.relu(rand(N, c, h, w, seed=seed + i)) for i, c in enumerate(chans)]
    k = sum(chans)
    weight = rand(cout, k, 1, 1, seed=seed + 10, scale=(2.0 / k) ** 0.5)
    scale, shift = resnet_cases.scale_shift(cout, seed + 11)
    stats = bn(cout, seed + 13)
    dz = rand(N, cout, h, w, seed=seed + 14) * (rand(N, cout, h, w, seed=seed + 15) > 0)
    cat = torch.cat(srcs, dim=1)
    return dict(srcs=srcs, weight=weight, scale=scale, shift=shift, ref=vovnet_ref.folded_conv_relu(cat, weight, scale, shift),
                bn=stats, dz=dz, grads=vovnet_train_ref.conv_param_grads(dz.double(), cat.double(), weight, *stats))


@functools.lru_cache(maxsize=None)
def vov_ese_case(c, h, w):
    """test_vovnet_gpu._ese_case / test_vovnet_train_gpu.test_ese_bwd's inputs: gates of exactly 0, exactly 1 and in between."""
    seed = 4000 + 7 * h + 3 * w + c
    xt = torch.relu(rand(N, c, h, w, seed=seed))
    identity, dout = rand(N, c, h, w, seed=seed + 1), rand(N, c, h, w, seed=seed + 2)
    fc_w = rand(c, c, 1, 1, seed=seed + 3, scale=c ** -0.5)
    fc_b = rand(c, seed=seed + 4, scale=0.5)
    fc_b[0::7], fc_b[3::7] = 8.0, -8.0
    flat = xt.reshape(N, c, h * w)
    partials = torch.stack([t.sum(dim=2) for t in flat.split(128, dim=2)], dim=1).contiguous()
    gate = vovnet_ref.ese_gate(xt.double().mean(dim=(2, 3)), fc_w, fc_b)
    return dict(xt=xt, identity=identity, dout=dout, fc_w=fc_w, fc_b=fc_b, partials=partials, gate=gate)


# ---- FPN -----------------------------------------------------------------------------------------------------------------------
# (cin, h, w, with `up`, channels-last out)
FPN_LATERAL_ROWS = [(cin, *hw, up, cl) for i, hw in enumerate(PX64) for j, cin in enumerate((32, 64))
                    for up, cl in ([(False, False), (True, True)] if (i + j) % 2 == 0 else [(True, False), (False, True)])]
# (levels, channels-last out)
FPN_CONV_ROWS = [(lv, cl) for lv in [(hw,) for hw in T16] + [MULTI] for cl in (False, True)]
# (h, w of the input, relu_in, channels-last in and out)
FPN_EXTRA_ROWS = [(*hw, bool(i % 2), cl) for i, hw in enumerate(S2) for cl in (False, True)]
# (cin, h, w): dgrad, wgrad, bias gradient
FPN_LATERAL_GRAD_ROWS = [(cin, *hw) for hw in PX64 for cin in (32, 64)]
# (fine, coarse)
FPN_TOPDOWN_ROWS = [(hw, ((hw[0] + 1) // 2, (hw[1] + 1) // 2)) for hw in PX64] + [((16, 16), (8, 8)), ((17, 16), (9, 8))]
TILINGS['fpn'] = (64, [r[1:3] for r in FPN_LATERAL_ROWS])
TILINGS['fpn_conv'] = ((16, 16), [hw for lv, _ in FPN_CONV_ROWS for hw in lv] + [out_hw(r[0], r[1], 2) for r in FPN_EXTRA_ROWS])


@functools.lru_cache(maxsize=None)
def fpn_lateral_case(cin, h, w):
    seed = 5000 + 7 * h + 3 * w + cin
    x, wt, b = rand(N, cin, h, w, seed=seed), rand(256, cin, seed=seed + 1, scale=cin ** -0.5), rand(256, seed=seed + 2, scale=0.1)
    up = rand(N, 256, (h + 1) // 2, (w + 1) // 2, seed=seed + 3)
    g = rand(N, 256, h, w, seed=seed + 4)
    return dict(x=x, w=wt, b=b, up=up, g=g, plain=fpn_ref.lateral(x, wt, b), with_up=fpn_ref.lateral(x, wt, b, up),
                dx=torch.einsum('ok,nohw->nkhw', wt.double(), g.double()), dw=torch.einsum('nohw,nkhw->ok', g.double(), x.double()),
                db=g.double().sum((0, 2, 3)))


@functools.lru_cache(maxsize=None)
def fpn_conv_case(levels):
    seed = 5500 + 7 * levels[0][0] + 3 * levels[0][1] + len(levels)
    xs = [rand(N, 256, h, w, seed=seed + i) for i, (h, w) in enumerate(levels)]
    ws = [rand(256, 256, 3, 3, seed=seed + 10 + i, scale=2304 ** -0.5) for i in range(len(levels))]
    bs = [rand(256, seed=seed + 20 + i, scale=0.1) for i in range(len(levels))]
    return xs, ws, bs, [fpn_ref.conv3x3(x, w, b) for x, w, b in zip(xs, ws, bs)]


@functools.lru_cache(maxsize=None)
def fpn_extra_case(h, w, relu_in):
    """test_fpn_train_gpu._extra_case: forward and the fp64 autograd gradients of the stride-2 convolution."""
    seed = 6000 + 7 * h + 3 * w
    ho, wo = (h + 1) // 2, (w + 1) // 2
    x, wt, b = rand(N, 256, h, w, seed=seed), rand(256, 256, 3, 3, seed=seed + 1, scale=2304 ** -0.5), rand(256, seed=seed + 2, scale=0.1)
    dy, add = rand(N, 256, ho, wo, seed=seed + 3), rand(N, 256, h, w, seed=seed + 4)
    x64, w64, b64 = x.double().requires_grad_(True), wt.double().requires_grad_(True), b.double().requires_grad_(True)
    ref = fpn_ref.conv3x3(x64, w64, b64, stride=2, relu_in=relu_in)
    (ref * dy.double()).sum().backward()
    return dict(x=x, w=wt, b=b, dy=dy, add=add, ref=ref.detach(), dx=x64.grad, dw=w64.grad, db=b64.grad)


@functools.lru_cache(maxsize=None)
def fpn_topdown_case(fine, coarse):
    seed = 6500 + 7 * fine[0] + 3 * fine[1]
    gf, gc = rand(N, 256, *fine, seed=seed), rand(N, 256, *coarse, seed=seed + 1)
    return gf, gc, gc.double() + fpn_train_ref.upsample_adjoint(gf, coarse)


# ---- DCN -----------------------------------------------------------------------------------------------------------------------
# the crafted planes of dcn_ref.crafted_offsets, two per row (image 0, image 1): samples exactly on the border, at -1, at H and W
DCN_PLANE_PAIRS = [('at_minus_1', 'at_h_minus_1'), ('corner_br', 'at_h_and_w'), ('integers', 'corner_tl'), ('corner_tr', 'corner_bl'),
                   ('zero', 'at_h_minus_1')]
# (cin, cout, stride, h, w, the planes of the two images)
DCN_ROWS = [(cin, 64, s, *hw, DCN_PLANE_PAIRS[(i + j) % len(DCN_PLANE_PAIRS)])
            for s, sizes in ((1, T16), (2, S2)) for i, hw in enumerate(sizes) for j, cin in enumerate((64, 128))]
# (cin, stride, h, w): the offset convolution; (cin, cout, stride, h, w, planes): the 64-flat-pixel weight gradients
DCN_OFFSET_ROWS = [(cin, s, *hw) for s, sizes in ((1, T16), (2, S2)) for hw in sizes for cin in (64, 128)] + \
    [(64, 1, *hw) for hw in PX64[1:]]                                              # its weight gradient walks 64 flat pixels
DCN_WGRAD_ROWS = [(64, 64, 1, *hw, DCN_PLANE_PAIRS[i % len(DCN_PLANE_PAIRS)]) for i, hw in enumerate(PX64)] + \
    [(128, 64, 2, 15, 15, DCN_PLANE_PAIRS[0]), (64, 64, 2, 16, 16, DCN_PLANE_PAIRS[1])]          # -> (8, 8): 64 output pixels
TILINGS['dcn'] = ((16, 16), [out_hw(r[3], r[4], r[2]) for r in DCN_ROWS])
TILINGS['dcn_wgrad'] = (64, [out_hw(r[3], r[4], r[2]) for r in DCN_WGRAD_ROWS])


def dcn_id(r):
    return f'{r[0]}-{r[1]}-s{r[2]}-{r[3]}x{r[4]}-{r[5][0]}+{r[5][1]}'


@functools.lru_cache(maxsize=None)
def dcn_case(cin, cout, stride, h, w, planes):
    """Inputs with the crafted offsets of `planes` (one image each), the fp64 forward and the fp64 autograd gradients (plain, and
    behind a folded BatchNorm's scale and a ReLU mask y > 0)."""
    seed = 7000 + 7 * h + 3 * w + cin + stride
    crafted = dcn_ref.crafted_offsets(h, w, stride)
    ho, wo = out_hw(h, w, stride)
    x = rand(N, cin, h, w, seed=seed)
    weight = rand(cout, cin, 3, 3, seed=seed + 1, scale=(9 * cin) ** -0.5)
    offset = torch.cat([crafted[k] for k in planes])
    mask = torch.rand(N, 9, ho, wo, generator=torch.Generator().manual_seed(seed + 2))
    dout, y, scale = rand(N, cout, ho, wo, seed=seed + 3), rand(N, cout, ho, wo, seed=seed + 4), rand(cout, seed=seed + 5) + 1.5
    return dict(x=x, weight=weight, offset=offset, mask=mask, dout=dout, y=y, scale=scale,
                ref=dcn_ref.dcn_ref(x, offset, mask, weight, None, stride),
                plain=dcn_train_ref.autograd(x, offset, mask, weight, dout, stride),
                masked=dcn_train_ref.autograd(x, offset, mask, weight, dout, stride, scale, y > 0))


@functools.lru_cache(maxsize=None)
def dcn_offset_case(cin, stride, h, w):
    """test_dcn_gpu.test_offset_conv_kernel_against_fp64's inputs and test_dcn_train_gpu._offset_conv_case's gradients."""
    seed = 7500 + 7 * h + 3 * w + cin + stride
    ho, wo = out_hw(h, w, stride)
    x = rand(N, cin, h, w, seed=seed)
    weight = rand(27, cin, 3, 3, seed=seed + 1, scale=2.0 * (9 * cin) ** -0.5)
    bias = rand(27, seed=seed + 2, scale=0.5)
    do, base = rand(N, 27, ho, wo, seed=seed + 3), rand(N, cin, h, w, seed=seed + 4)
    off, msk = dcn_ref.offset_conv_ref(x, weight, bias, stride)
    xx, ww, bb = x.double().requires_grad_(True), weight.double().requires_grad_(True), bias.double().requires_grad_(True)
    (torch.nn.functional.conv2d(xx, ww, bb, stride=stride, padding=1) * do.double()).sum().backward()
    return dict(x=x, weight=weight, bias=bias, do=do, base=base, ref=torch.cat((off, msk), dim=1), dx=xx.grad, dw=ww.grad, db=bb.grad)


# ---- DepthNet ------------------------------------------------------------------------------------------------------------------
# (levels, frozen): batch statistics need more than the two values per channel a (1, 1) level of two cameras has - with two, xhat
# is +-1 and every gradient through the statistics cancels to zero - so the lone (1, 1) level runs frozen only
DEPTH_ROWS = [((hw,), frozen) for hw in T16 for frozen in ((True,) if hw == (1, 1) else (False, True))] + [(MULTI, False), (MULTI, True)]
TILINGS['depth_net'] = ((16, 16), [hw for lv, _ in DEPTH_ROWS for hw in lv])
DEPTH_EPS, DEPTH_MOMENTUM = 1e-5, 0.1


def depth_id(r):
    return '+'.join(hw_id(hw) for hw in r[0]) + ('-frozen' if r[1] else '')


@functools.lru_cache(maxsize=None)
def depth_params():
    """test_depth_net_train_gpu._module's distributions for the 3x3, its bias and the BatchNorm; a gate (N, 256) in (0, 1)."""
    g = torch.Generator().manual_seed(8000)
    r = lambda *s: torch.randn(*s, generator=g)                                                     # noqa: E731
    return dict(w=r(256, 256, 3, 3) * 2304 ** -0.5, b=0.1 * r(256), mean=0.3 * r(256), var=0.25 + 2 * torch.rand(256, generator=g),
                gamma=1 + 0.2 * r(256), beta=0.2 * r(256), gate=torch.sigmoid(r(N, 256)))


@functools.lru_cache(maxsize=None)
def depth_case(levels, frozen):
    """Per level: x, the cotangent r and forward64's dict (batch statistics, or frozen: the running ones)."""
    p = depth_params()
    seed = 8100 + 7 * levels[0][0] + 3 * levels[0][1] + len(levels)
    xs = [rand(N, 256, h, w, seed=seed + i) for i, (h, w) in enumerate(levels)]
    rs = [rand(N, 256, h, w, seed=seed + 10 + i) for i, (h, w) in enumerate(levels)]
    fwd = [forward64(x, p['w'], p['b'], p['gamma'], p['beta'], p['gate'], DEPTH_EPS, running=(p['mean'], p['var']) if frozen else None)
           for x in xs]
    return xs, rs, fwd


@functools.lru_cache(maxsize=None)
def cam_gate_case():
    """Two cameras' intrinsics, one augmentation scale, the gate's weights; the reference is test_depth_net_cpu.restated_gate."""
    from test_depth_net_cpu import restated_gate
    g = torch.Generator().manual_seed(8500)
    intr = torch.eye(4).repeat(N, 1, 1)
    for i, f in enumerate((600.0, 1500.0)):
        intr[i, 0, 0], intr[i, 1, 1], intr[i, 0, 2], intr[i, 1, 2] = f, f * 1.05, 800.0, 450.0
    ida = torch.tensor([[[0.8, 0., -20.], [0., 0.8, -40.], [0., 0., 1.]]])
    shapes = {'mlp.fc1.weight': (256, 1), 'mlp.fc1.bias': (256,), 'mlp.fc2.weight': (256, 256), 'mlp.fc2.bias': (256,),
              'se.conv_reduce.weight': (256, 256, 1, 1), 'se.conv_reduce.bias': (256,), 'se.conv_expand.weight': (256, 256, 1, 1),
              'se.conv_expand.bias': (256,)}
    sd = {k: torch.randn(*s, generator=g) * 0.06 for k, s in shapes.items()}
    ref = restated_gate({k: v.double() for k, v in sd.items()}, intr.double(), ida.double())
    return intr, ida[:, 0, 0].contiguous(), sd, ref


# ---- dense rows ----------------------------------------------------------------------------------------------------------------
DENSE_M = [1, 127, 128, 129]
# (K, N) of linear_fwd: a full tile; N = 248 and K = 3, the ragged sizes of test_dense_gpu.py
LINEAR_KN = [(256, 256), (256, 248), (3, 256)]
TILINGS['dense'] = (128, [(1, m) for m in DENSE_M])
GEMM_KN = (32, 256)              # test_gemm_gpu.test_gemm_bf16x3_matches_fp64's smallest K and N
MLP2_K1_H = (16, 32)             # test_head_pe_gpu.test_fused_two_layer_mlp_matches_fp64's smallest shapes
HEADS = 8
LN_C = 256


@functools.lru_cache(maxsize=None)
def linear_case(m, k, n):
    """test_dense_gpu.test_linear_matches_fp64's inputs."""
    g = torch.Generator().manual_seed(9000 + m + k + n)
    x, w, b = torch.randn(m, k, generator=g), torch.randn(n, k, generator=g) * 0.1, torch.randn(n, generator=g)
    w[min(3, n - 1), min(2, k - 1)] = 2.5
    return x, w, b, torch.nn.functional.linear(x.double(), w.double(), b.double())


@functools.lru_cache(maxsize=None)
def dense_case(m):
    """The inputs and fp64 references of the other dense rows at M rows, as the tests named beside each build them."""
    F = torch.nn.functional
    g = torch.Generator().manual_seed(9100 + m)
    r = lambda *s: torch.randn(*s, generator=g)                                                     # noqa: E731
    c = {}
    # gemm_bf16x3_fwd with its ReLU (test_gemm_gpu.py); `scale` is the magnitude of the products summed, which its bound takes
    k, n = GEMM_KN
    a, w, b = r(m, k), r(n, k) * 0.1, r(n)
    w[3, 2] = 2.5
    c['gemm'] = dict(a=a, w=w, b=b, ref=(a.double() @ w.double().t() + b.double()).relu(),
                     scale=(a.double().abs() @ w.double().abs().t()).max().item())
    # mlp2_bf16x3_fwd (test_head_pe_gpu.py): relu(x W1^T + b1) W2^T + b2, the hidden activation kept for the ReLU condition
    k1, h = MLP2_K1_H
    x, w1, b1, w2, b2 = r(m, k1), r(h, k1) / k1 ** 0.5, r(h) * 0.1, r(256, h) / h ** 0.5, r(256) * 0.1
    hidden = torch.relu(x.double() @ w1.double().t() + b1.double())
    c['mlp2'] = dict(x=x, w1=w1, b1=b1, w2=w2, b2=b2, hidden=hidden, ref=(hidden @ w2.double().t() + b2.double()).float())
    # value_proj_heads_fwd (test_cross_attn_late_gpu.test_value_proj_heads_matches_fp64)
    dh = 256 // HEADS
    agg, wsum, w, b = r(m, HEADS, 256), torch.rand(m, HEADS, generator=g), r(256, 256) * 0.06, r(256)
    ref = torch.einsum('mhc,hdc->mhd', agg.double(), w.double().view(HEADS, dh, 256)) + b.double().view(HEADS, dh) * wsum.double().unsqueeze(-1)
    c['heads'] = dict(agg=agg, wsum=wsum, w=w, b=b, ref=ref.reshape(m, 256))
    # layernorm_fwd / layernorm_bwd (test_dense_gpu.py): plain, with the ReLU, with a residual; the gradients by fp64 autograd
    x, res, gamma, beta, dy = r(m, LN_C) * 3 + 0.5, r(m, LN_C), r(LN_C), r(LN_C) * 0.5, r(m, LN_C)
    ln = dict(x=x, res=res, gamma=gamma, beta=beta, dy=dy, fwd={}, bwd={})
    for relu, with_res in ((False, False), (True, False), (False, True)):
        y = F.layer_norm((x + res if with_res else x).double(), (LN_C,), gamma.double(), beta.double())
        ln['fwd'][relu, with_res] = y.relu() if relu else y
    for relu in (False, True):
        xd, gd, bd = x.double().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
        y = F.layer_norm(xd, (LN_C,), gd, bd)
        (y.relu() if relu else y).backward(dy.double())
        ln['bwd'][relu] = (xd.grad, gd.grad, bd.grad)
    c['ln'] = ln
    return c


# ---- the conditions test_memory_contract_cpu.py asserts ---------------------------------------------------------------------------
def relu_references():
    """(id, fp64 reference) of every row whose last operation is a ReLU."""
    for r in RESNET_ROWS:
        if r[5]:
            yield 'resnet ' + resnet_id(r), resnet_case(*r)[5]
    for r in VOV_CONV_ROWS:
        yield 'vovnet conv3x3_bn_relu ' + 'x'.join(map(str, r)), vov_conv_case(*r)['ref']
    for r in VOV_OSA_ROWS:
        yield f'vovnet osa_concat_conv {r}', vov_osa_case(*r)['ref']
    for r in DEPTH_ROWS:
        for hw, f in zip(r[0], depth_case(*r)[2]):
            yield f'depth_net {depth_id(r)} level {hw_id(hw)}', f['out']
    for m in DENSE_M:
        c = dense_case(m)
        yield f'gemm_bf16x3_fwd M = {m}', c['gemm']['ref']
        yield f'mlp2_bf16x3_fwd M = {m}, the hidden activation', c['mlp2']['hidden']
        yield f'layernorm_fwd M = {m} with its ReLU', c['ln']['fwd'][True, False]


def has_exact_and_plus_one(tile, sizes):
    """A size that is a whole number of tiles, and one that is a whole number of tiles plus one pixel (flat pixels, or in either
    direction of a two-dimensional tile)."""
    if isinstance(tile, int):
        flat = [h * w for h, w in sizes]
        return any(p % tile == 0 for p in flat), any(p > tile and p % tile == 1 for p in flat)
    th, tw = tile
    exact = any(h % th == 0 and w % tw == 0 for h, w in sizes)
    plus = any((h > th and h % th == 1 and w % tw in (0, 1)) or (w > tw and w % tw == 1 and h % th in (0, 1)) for h, w in sizes)
    return exact, plus
