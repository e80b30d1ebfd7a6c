"""The new kernels of gd4d_resnet_train.hip under the memory contract (contract.py / guarded.py), at the edge sizes of
test_resnet_train_gpu.py (resnet_train_cases.py): every input embedded in NaNs, every output and every weight-gradient workspace in a
guarded NaN buffer, the pads intact, the results finite and within KERNEL_TOL of the fp64 reference's largest |entry|, and a second launch
into fresh buffers gives the same bits.  GPU only."""
import pytest
import torch

import resnet_train_cases as C
import resnet_train_ref as T
from contract import as_input, contract, err

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
N = C.N


def _scale(bn):
    return (bn[0] * torch.rsqrt(bn[3] + T.EPS)).to(DEV)


def _dgrad(taps, cin, cout, stride, h, w, even):
    from graph_detr4d_amd import ops
    weight, bn, dz, operands, variants = C.dgrad_case(taps, cin, cout, stride, h, w, even)
    build = ops.conv3x3_act_image_t if taps == 9 else ops.conv1x1_image_t
    image_t = as_input(build(weight.to(DEV), _scale(bn)))
    ddz = as_input(dz)
    dev = {k: as_input(v) for k, v in operands.items()}
    name = 'mask+add2+add_even' if even else 'add+mask+add2'                   # every operand the case has
    names, ref = variants[name]

    def launch(run):
        out = run.out((N, cin, h, w))
        kw = {k: dev[k] for k in names}
        if taps == 9:
            return {'dx': ops.conv3x3_act_dgrad(ddz, image_t, cin, hw=(h, w), stride=stride, out=out, **kw)}
        return {'dx': ops.conv1x1_dgrad(ddz, image_t, cin, out=out, **kw)}

    what = f'dgrad taps {taps} {(cin, cout, stride, h, w)} {name}'
    contract(what, launch, lambda res: err(what, res['dx'], ref, C.KERNEL_TOL, T.rel_err))


@pytest.mark.parametrize('case', C.PW_DGRAD_CASES, ids=C.case_id)
def test_conv1x1_dgrad_contract(case):
    cin, cout, h, w, even = case
    _dgrad(1, cin, cout, 1, h, w, even)


@pytest.mark.parametrize('case', C.C3_DGRAD_CASES, ids=C.case_id)
def test_conv3x3_act_dgrad_contract(case):
    cin, cout, stride, h, w, even = case
    _dgrad(9, cin, cout, stride, h, w, even)


@pytest.mark.parametrize('case', C.WGRAD_CASES, ids=C.case_id)
def test_wgrad_contract(case):
    from graph_detr4d_amd import _lib, ops
    taps, cin, cout, stride, h, w = case
    x, weight, bn, dz, refs = C.wgrad_case(*case)
    wgrad = ops.conv3x3_act_wgrad if taps == 9 else ops.conv1x1_wgrad
    dx, ddz, dweight, dbn = as_input(x), as_input(dz), as_input(weight), as_input(C.bn_stats(bn))
    lib = _lib.load()
    tiles = int(lib.gd4d_resnet_wgrad_tiles(taps, N, h, w, stride))
    for parts in (1, tiles + 3):                                               # one partition; more partitions than tiles
        floats = int(lib.gd4d_resnet_wgrad_workspace_bytes(taps, cin, cout, N, h, w, stride, parts)) // 4
        assert floats > 0

        def launch(run):
            outs = (run.out(weight.shape), run.out((cout,)), run.out((cout,)))
            got = wgrad(ddz, dx, dweight, dbn, stride=stride, partitions=parts, outs=outs, workspace=run.out((floats,)))
            return dict(zip(('dW', 'dgamma', 'dbeta'), got))

        what = f'wgrad {case}, {parts} partitions of {tiles} tiles'

        def check(res):
            for k, r in zip(('dW', 'dgamma', 'dbeta'), refs):
                err(f'{what} {k}', res[k], r, C.KERNEL_TOL, T.rel_err)
        contract(what, launch, check)


def test_mask_and_scatter_contract():
    from graph_detr4d_amd import ops
    dout, out = C.rand(N, 32, 9, 11, seed=1), torch.relu(C.rand(N, 32, 9, 11, seed=2))
    d_dout, d_out = as_input(dout), as_input(out)
    contract('relu_mask_bwd', lambda run: {'g': ops.relu_mask_bwd(d_dout, d_out, out=run.out(dout.shape))},
             lambda res: err('relu_mask_bwd', res['g'], dout * (out > 0), 0.0, T.rel_err))
    for h, w in ((9, 11), (8, 12), (1, 1)):
        src = C.rand(N, 32, *C.half(h, w), seed=3)
        ref = torch.zeros(N, 32, h, w)
        ref[:, :, ::2, ::2] = src
        d_src = as_input(src)
        contract(f'even_pixels_scatter {h} x {w}', lambda run: {'out': ops.even_pixels_scatter(d_src, (h, w), out=run.out((N, 32, h, w)))},
                 lambda res: err(f'even_pixels_scatter {h} x {w}', res['out'], ref, 0.0, T.rel_err))
