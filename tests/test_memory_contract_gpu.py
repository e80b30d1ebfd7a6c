"""The memory contract of the convolution families and the dense rows: what the value tests cannot see because it lies outside the map
they compare.  Every row of memory_contract_cases.py runs on N = 2 images (an over-run of image 0 falls into image 1, where the value
check sees it; an over-run of image 1 falls into the guard) with
  - every floating-point input embedded in NaNs (guarded.embedded): a read past an input that is then multiplied by zero is a NaN;
  - every output the wrapper lets the caller supply inside a guarded buffer (guarded.guarded), itself pre-filled with NaN: a store
    past the end flips the guard, an element never written stays NaN; the workspaces of the partitioned weight gradients likewise;
  - one run checked against the family's fp64 reference with THE BOUND THE FAMILY'S OWN TEST ASSERTS (imported from it, or copied with
    the test named), a second run into fresh buffers that must give the same bits (every kernel here documents a fixed summation
    order; dcn_bwd_data's dX, the float atomics' output, is compared as test_dcn_train_gpu.py compares it).
Every guarded buffer of a launch must be among the pointers the library was handed, and every returned tensor must lie inside one: a
wrapper that ignores a supplied out= / outs= / workspace= fails here instead of passing on a buffer nobody guards.
No new tolerance is introduced here, with one deviation in the measure: under batch statistics the (1, 1) level of the multi-level
DepthNet row has two values per channel, its dy / dx references are zero up to rounding, and their errors (and the dbias bound) are
taken against the frozen form of the same gradient - the size of the terms that cancel - with DepthNet's own BWD_TOL
(test_depth_net_kernels).  GPU only; every test is a handful of launches on maps of at most a few thousand pixels."""
import math

import pytest
import torch

import dcn_ref
import dcn_train_ref
import fpn_ref
import memory_contract_cases as C
import resnet_ref
import vovnet_ref
import vovnet_train_ref
from contract import DEV, Handed as _Handed, Run as _Run, as_input as _in, contract as _contract, err as _err  # noqa: F401
from depth_net_train_ref import backward64, rel_fro
from guarded import embedded
from test_dcn_gpu import KERNEL_TOL as DCN_TOL
from test_dcn_train_gpu import KERNEL_TOL as DCN_TRAIN_TOL
from test_depth_net_train_gpu import BWD_TOL as DEPTH_BWD_TOL, FWD_TOL as DEPTH_FWD_TOL
from test_fpn_gpu import KERNEL_TOL as FPN_TOL
from test_fpn_train_gpu import KERNEL_TOL as FPN_TRAIN_TOL
from test_resnet_gpu import KERNEL_TOL as RESNET_TOL
from test_vovnet_gpu import KERNEL_TOL as VOVNET_TOL
from test_vovnet_train_gpu import KERNEL_TOL as VOVNET_TRAIN_TOL

pytestmark = pytest.mark.gpu
N = C.N


# ---- the harness (contract.py) and what only this file needs of it ------------------------------------------------------------------
def _partitioned(what, tiles, default, launch, check, agree):
    """A partitioned weight gradient at 1 partition, the default count and more partitions than tiles (partition_range then yields
    empty partitions, whose workspace slab must still be defined): launch(run, partitions), its workspace guarded and NaN-filled
    every time.  `default` restates the wrapper's own choice so that its workspace can be sized: the wrapper called without
    a count must give that run's bits.  All three meet the bound; the first and the last agree with each other to it: agree(name,
    got, ref)."""
    results = {}
    assert 1 <= default <= max(1, tiles)
    for parts in dict.fromkeys((1, default, tiles + 5)):
        results[parts] = _contract(f'{what}, partitions {parts}', lambda run, p=parts: launch(run, p), check)
    own = _contract(f'{what}, partitions left to the wrapper', lambda run: launch(run, None), check)
    for k, t in own.items():
        assert torch.equal(t, results[default][k]), f'{what} {k}: the wrapper\'s default is not {default} partitions'
    for k, t in results[tiles + 5].items():
        agree(f'{what} {k}: {tiles + 5} partitions against 1', t, results[1][k].cpu())
    return results[default]


def _cus():
    return torch.cuda.get_device_properties(DEV).multi_processor_count


def _workspace(run, lib_bytes, *args):
    """A guarded, NaN-filled workspace of the size the library asks for."""
    nbytes = int(lib_bytes(*args))
    assert nbytes > 0 and nbytes % 4 == 0, (args, nbytes)
    return run.out((nbytes // 4,))


def _lib():
    from graph_detr4d_amd import _lib as L
    return L.load()


def test_the_harness_fails_on_each_kind_of_error():
    """Torch ops on the device standing in for a kernel, inside memory this test allocated: a store one element past the output, an
    element never written, a zero-weighted read of the element past an input, a second run with other bits, and a result that is
    not the buffer supplied each fail _contract; the correct stand-in passes."""
    x = torch.arange(1., 13.).view(3, 4)
    dx = _in(x)
    whole = torch.empty(0, device=DEV).set_(dx.untyped_storage())               # the input with its surroundings
    start = dx.storage_offset()
    calls = []

    def kernel(kind):
        def launch(run):
            out = run.out((3, 4))
            out.copy_(dx * 2)
            if kind == 'stray store':
                run.guards[-1][1].buffer[out.storage_offset() + 12] = 0.0
            elif kind == 'unwritten':
                out[2, 3] = float('nan')
            elif kind == 'zero-weighted read past the input':
                out[2, 3] += 0.0 * whole[start + 12]
            elif kind == 'other bits':
                calls.append(1)
                out[0, 0] += 4e-7 * len(calls)                                  # within the bound both times, other bits
            return dict(out=out.clone() if kind == 'ignores the supplied output' else out)
        return launch
    check = lambda res: _err('stand-in', res['out'], x.double() * 2, 1e-6, resnet_ref.rel_err)      # noqa: E731
    _contract('correct', kernel('correct'), check, native=False)
    for kind in ('stray store', 'unwritten', 'zero-weighted read past the input', 'other bits', 'ignores the supplied output'):
        with pytest.raises(AssertionError):
            _contract(kind, kernel(kind), check, native=False)
    with pytest.raises(AssertionError, match='never handed to the library'):     # a buffer the library never received
        _contract('not handed over', kernel('correct'), check)


# ---- ResNet ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('row', C.RESNET_ROWS, ids=C.resnet_id)
def test_resnet_conv_bn_act(row):
    from graph_detr4d_amd import ops
    taps, cin, cout, stride, identity, relu, h, w = row
    x, weight, scale, shift, ident, ref = C.resnet_case(*row)
    make, op = (ops.conv3x3_act_image, ops.conv3x3_bn_act) if taps == 9 else (ops.conv1x1_image, ops.conv1x1_bn_act)
    image = make(weight.to(DEV))
    dx, dscale, dshift, dident = _in(x), _in(scale), _in(shift), _in(ident)
    what = f'{op.__name__} {C.resnet_id(row)}'
    _contract(what, lambda run: dict(out=op(dx, image, cout, dscale, dshift, stride=stride, identity=dident, relu=relu, out=run.out(ref.shape))),
              lambda res: _err(what, res['out'], ref, RESNET_TOL, resnet_ref.rel_err))


# ---- VoVNet ----------------------------------------------------------------------------------------------------------------------
def _bn_dev(gamma, beta, mean, var):
    """test_vovnet_train_gpu._bn_dev: scale = gamma rstd, rstd, mean."""
    rstd = torch.rsqrt(var + vovnet_ref.EPS)
    return torch.stack((gamma * rstd, rstd, mean)).contiguous()


def _wgrad_check(what, names, refs, tol, metric):
    return lambda res: [_err(f'{what} {k}', res[k], r, tol, metric) for k, r in zip(names, refs)]


@pytest.mark.parametrize('row', C.VOV_CONV_ROWS, ids=lambda r: 'x'.join(map(str, r)))
def test_vovnet_conv3x3_bn_relu_and_wgrad(row):
    from graph_detr4d_amd import ops
    cin, cout, stride, h, w = row
    c = C.vov_conv_case(*row)
    image = ops.conv3x3_image(c['weight'].to(DEV))
    dx, dscale, dshift = _in(c['x']), _in(c['scale']), _in(c['shift'])
    what = f'conv3x3_bn_relu {row}'
    _contract(what, lambda run: dict(out=ops.conv3x3_bn_relu(dx, image, cout, dscale, dshift, stride=stride, out=run.out(c['ref'].shape))),
              lambda res: _err(what, res['out'], c['ref'], VOVNET_TOL, vovnet_ref.rel_err))
    if stride != 1:
        return                                                                   # (the training kernels are the stride-1 layers')
    lib = _lib()
    ddz, dweight, dbn = _in(c['dz']), _in(c['weight']), _in(_bn_dev(*c['bn']))
    names = ('dW', 'dgamma', 'dbeta')
    what = f'conv3x3_wgrad {row}'

    def launch(run, parts):
        ws = None if parts is None else _workspace(run, lib.gd4d_conv_wgrad_workspace_bytes, cin, cout, 9, parts)
        outs = (run.out(c['weight'].shape), run.out((cout,)), run.out((cout,)))
        return dict(zip(names, ops.conv3x3_wgrad(ddz, dx, dweight, dbn, partitions=parts, outs=outs, workspace=ws)))
    tiles = int(lib.gd4d_conv3x3_wgrad_tiles(N, h, w))
    _partitioned(what, tiles, ops._vv_partitions(torch.device(DEV), tiles, cin // 32, None), launch,
                 _wgrad_check(what, names, c['grads'], VOVNET_TRAIN_TOL, vovnet_train_ref.rel_err),
                 lambda n, a, b: _err(n, a, b, VOVNET_TRAIN_TOL, vovnet_train_ref.rel_err))


@pytest.mark.parametrize('row', C.VOV_OSA_ROWS, ids=lambda r: '+'.join(map(str, r[0])) + f'-{r[1]}-{r[2]}x{r[3]}')
def test_vovnet_osa_concat_conv_and_wgrad(row):
    from graph_detr4d_amd import ops
    chans, cout, h, w = row
    c = C.vov_osa_case(*row)
    lib = _lib()
    image = ops.osa_concat_image(c['weight'].to(DEV))
    dsrcs, dscale, dshift = [_in(s) for s in c['srcs']], _in(c['scale']), _in(c['shift'])
    tiles = (h * w + 127) // 128
    assert int(lib.gd4d_osa_concat_tiles(h, w)) == tiles
    what = f'osa_concat_conv {row}'

    def check(res):
        _err(what, res['out'], c['ref'], VOVNET_TOL, vovnet_ref.rel_err)
        mean_ref = c['ref'].mean(dim=(2, 3))                                     # test_vovnet_gpu.test_osa_concat_conv_against_fp64
        mean = res['partials'].cpu().double().sum(dim=1) / (h * w)
        _err(f'{what} pool mean', mean, mean_ref, VOVNET_TOL, lambda a, b: float((a - b).abs().max() / b.abs().max()))
    fwd = _contract(what, lambda run: dict(zip(('out', 'partials'), ops.osa_concat_conv(
        dsrcs, image, cout, dscale, dshift, out=run.out(c['ref'].shape), partials=run.out((N, tiles, cout))))), check)
    assert tuple(fwd['partials'].shape) == (N, tiles, cout)
    ddz, dweight, dbn = _in(c['dz']), _in(c['weight']), _in(_bn_dev(*c['bn']))
    dsums = _in(c['dz'].to(DEV).sum(dim=(2, 3)))
    names = ('dW', 'dgamma', 'dbeta')
    what = f'osa_concat_wgrad {row}'

    def launch(run, parts):
        ws = None if parts is None else _workspace(run, lib.gd4d_conv_wgrad_workspace_bytes, sum(chans), cout, 1, parts)
        outs = (run.out(c['weight'].shape), run.out((cout,)), run.out((cout,)))
        return dict(zip(names, ops.osa_concat_wgrad(ddz, dsums, dsrcs, dweight, dbn, partitions=parts, outs=outs, workspace=ws)))
    wtiles = int(lib.gd4d_osa_concat_wgrad_tiles(N, h, w))
    chunks = ((sum(chans) + 63) // 64) * ((cout + 255) // 256)
    _partitioned(what, wtiles, ops._vv_partitions(torch.device(DEV), wtiles, chunks, None), launch,
                 _wgrad_check(what, names, c['grads'], VOVNET_TRAIN_TOL, vovnet_train_ref.rel_err),
                 lambda n, a, b: _err(n, a, b, VOVNET_TRAIN_TOL, vovnet_train_ref.rel_err))


@pytest.mark.parametrize('row', C.VOV_ESE_ROWS, ids=lambda r: f'{r[0]}-{r[1]}x{r[2]}')
def test_vovnet_ese_gate_apply_and_bwd(row):
    from graph_detr4d_amd import ops
    ch, h, w = row
    c = C.vov_ese_case(*row)
    lib = _lib()
    dpart, dfc_w, dfc_b, dxt, dident, ddout = (_in(c[k]) for k in ('partials', 'fc_w', 'fc_b', 'xt', 'identity', 'dout'))
    what = f'ese_gate {row}'

    def check_gate(res):
        _err(what, res['gate'], c['gate'], VOVNET_TOL, vovnet_ref.rel_err)
        got = res['gate'].cpu()
        assert torch.equal(got == 0, c['gate'] == 0) and torch.equal(got == 1, c['gate'] == 1)
    gate = _contract(what, lambda run: dict(gate=ops.ese_gate(dpart, h * w, dfc_w, dfc_b, out=run.out((N, ch)))), check_gate)['gate']
    dgate = _in(gate)
    for ident in (None, dident):
        ref = c['xt'].double() * gate.cpu().double()[:, :, None, None] + (0 if ident is None else c['identity'].double())
        what = f'ese_apply {row} identity {ident is not None}'
        _contract(what, lambda run: dict(out=ops.ese_apply(dxt, dgate, identity=ident, out=run.out(ref.shape))),
                  lambda res: _err(what, res['out'], ref, VOVNET_TOL, vovnet_ref.rel_err))
    # the device's own gate: its branches are the ones taken (test_vovnet_train_gpu.test_ese_bwd_against_fp64)
    ref_dz, ref_w, ref_b = vovnet_train_ref.ese_backward(c['dout'].double(), c['xt'].double(), gate.cpu().double(), c['fc_w'])
    refs = dict(dz=ref_dz, sums=ref_dz.sum(dim=(2, 3)), dfc_w=ref_w, dfc_b=ref_b)
    what = f'ese_bwd {row}'

    def launch(run):
        outs = (run.out(ref_dz.shape), run.out((N, ch)), run.out(c['fc_w'].shape), run.out((ch,)))
        ws = _workspace(run, lib.gd4d_ese_bwd_workspace_bytes, N, ch)
        return dict(zip(refs, ops.ese_bwd(ddout, dxt, dpart, dgate, dfc_w, outs=outs, workspace=ws)))
    _contract(what, launch, lambda res: [_err(f'{what} {k}', res[k], r, VOVNET_TRAIN_TOL, vovnet_train_ref.rel_err) for k, r in refs.items()])


# ---- FPN -------------------------------------------------------------------------------------------------------------------------
def _cl(t):
    """The same values stored (N, H, W, C)."""
    return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


@pytest.mark.parametrize('row', C.FPN_LATERAL_ROWS, ids=lambda r: f'{r[0]}-{r[1]}x{r[2]}' + ('-up' if r[3] else '') + ('-cl' if r[4] else ''))
def test_fpn_lateral_fwd(row):
    from graph_detr4d_amd import ops
    cin, h, w, with_up, cl = row
    c = C.fpn_lateral_case(cin, h, w)
    image = ops.fpn_lateral_image(c['w'].to(DEV))
    dx, db = _in(c['x']), _in(c['b'])
    dup = embedded(_cl(c['up'].to(DEV)) if cl else c['up'].to(DEV)) if with_up else None       # (the finished coarser lateral's layout)
    ref = c['with_up'] if with_up else c['plain']
    what = f'fpn_lateral_fwd {row}'

    def launch(run):
        out = ops.fpn_lateral_fwd(dx, image, db, up=dup, out=run.out(ref.shape, channels_last=cl))
        assert ops._is_cl(out) == cl or h * w == 1
        return dict(out=out)
    _contract(what, launch, lambda res: _err(what, res['out'], ref, FPN_TOL, fpn_ref.rel_err))


@pytest.mark.parametrize('row', C.FPN_CONV_ROWS, ids=lambda r: '+'.join(C.hw_id(hw) for hw in r[0]) + ('-cl' if r[1] else ''))
def test_fpn_conv_fwd(row):
    from graph_detr4d_amd import ops
    levels, cl = row
    xs, ws, bs, refs = C.fpn_conv_case(levels)
    images = [ops.depth_net_image(w.to(DEV)) for w in ws]
    dxs, dbs = [_in(x) for x in xs], [_in(b) for b in bs]
    what = f'fpn_conv_fwd {row}'
    got = _contract(what, lambda run: {f'level {i}': o for i, o in enumerate(ops.fpn_conv_fwd(
        dxs, images, dbs, outs=[run.out(r.shape, channels_last=cl) for r in refs]))},
        lambda res: [_err(f'{what} level {i}', res[f'level {i}'], r, FPN_TOL, fpn_ref.rel_err) for i, r in enumerate(refs)])
    # the wrapper's own maps: the same bits (a one-pixel level is both layouts at once and goes with the others)
    own = ops.fpn_conv_fwd(dxs, images, dbs, channels_last_out=cl)
    assert all(torch.equal(o, got[f'level {i}']) and (ops._is_cl(o) == cl or o.shape[2] * o.shape[3] == 1) for i, o in enumerate(own))


@pytest.mark.parametrize('row', C.FPN_EXTRA_ROWS, ids=lambda r: f'{r[0]}x{r[1]}' + ('-relu_in' if r[2] else '') + ('-cl' if r[3] else ''))
def test_fpn_extra_conv_fwd_dgrad_wgrad(row):
    from graph_detr4d_amd import ops
    h, w, relu_in, cl = row
    c = C.fpn_extra_case(h, w, relu_in)
    image = ops.depth_net_image(c['w'].to(DEV))
    dx, db = _in(c['x']), _in(c['b'])
    dx_in = embedded(_cl(c['x'].to(DEV))) if cl else dx
    what = f'fpn_extra_conv_fwd {row}'
    _contract(what, lambda run: dict(out=ops.fpn_extra_conv_fwd(dx_in, image, db, relu_in=relu_in, out=run.out(c['ref'].shape, channels_last=cl))),
              lambda res: _err(what, res['out'], c['ref'], FPN_TOL, fpn_ref.rel_err))
    if cl:
        return                                                                   # (the gradients are NCHW only)
    image_t = ops.depth_net_image_t(c['w'].to(DEV))
    ddy, dadd = _in(c['dy']), _in(c['add'])
    mask = dx if relu_in else None
    for add in (None, dadd):
        ref = c['dx'] + (0 if add is None else c['add'].double())
        what = f'fpn_extra_conv_dgrad {row} add {add is not None}'
        got = _contract(what, lambda run: dict(dx=ops.fpn_extra_conv_dgrad(ddy, image_t, (h, w), mask=mask, add=add, out=run.out(ref.shape))),
                        lambda res: _err(what, res['dx'], ref, FPN_TRAIN_TOL, fpn_ref.rel_err))['dx']
        if relu_in and add is None:
            assert bool((got[c['x'].to(DEV) <= 0] == 0).all())                   # nothing passes where the forward's ReLU cut
    what = f'fpn_extra_conv_wgrad {row}'
    _contract(what, lambda run: dict(zip(('dW', 'db'), ops.fpn_extra_conv_wgrad(ddy, dx, relu_in=relu_in,
                                                                                outs=(run.out((256, 256, 3, 3)), run.out((256,)))))),
              lambda res: [_err(f'{what} {k}', res[k], c[r], FPN_TRAIN_TOL, fpn_ref.rel_err) for k, r in (('dW', 'dw'), ('db', 'db'))])


@pytest.mark.parametrize('row', C.FPN_LATERAL_GRAD_ROWS, ids=lambda r: f'{r[0]}-{r[1]}x{r[2]}')
def test_fpn_lateral_dgrad_wgrad_bias_grad(row):
    from graph_detr4d_amd import ops
    cin, h, w = row
    c = C.fpn_lateral_case(cin, h, w)
    lib = _lib()
    image_t = ops.fpn_lateral_image_t(c['w'].to(DEV))
    dg, dx = _in(c['g']), _in(c['x'])
    what = f'fpn_lateral_dgrad {row}'
    _contract(what, lambda run: dict(dx=ops.fpn_lateral_dgrad(dg, image_t, cin, out=run.out(c['dx'].shape))),
              lambda res: _err(what, res['dx'], c['dx'], FPN_TRAIN_TOL, fpn_ref.rel_err))
    what = f'fpn_lateral_wgrad {row}'
    refs = dict(dW=c['dw'].reshape(256, cin, 1, 1), db=c['db'])

    def launch(run, parts):
        ws = None if parts is None else _workspace(run, lib.gd4d_fpn_lateral_wgrad_workspace_bytes, cin, parts)
        return dict(zip(refs, ops.fpn_lateral_wgrad(dg, dx, partitions=parts, outs=(run.out((256, cin, 1, 1)), run.out((256,))), workspace=ws)))
    tiles, chunks = int(lib.gd4d_fpn_lateral_wgrad_tiles(N, h, w)), (cin + 63) // 64
    _partitioned(what, tiles, max(1, min(tiles, (2 * _cus() + chunks - 1) // chunks)), launch,
                 lambda res: [_err(f'{what} {k}', res[k], r, FPN_TRAIN_TOL, fpn_ref.rel_err) for k, r in refs.items()],
                 lambda n, a, b: _err(n, a, b, FPN_TRAIN_TOL, fpn_ref.rel_err))       # "partial sums added in order"
    what = f'fpn_bias_grad {row}'
    _contract(what, lambda run: dict(db=ops.fpn_bias_grad(dg, out=run.out((256,)), workspace=run.out((N * 256,)))),
              lambda res: _err(what, res['db'], c['db'], FPN_TRAIN_TOL, fpn_ref.rel_err))


@pytest.mark.parametrize('row', C.FPN_TOPDOWN_ROWS, ids=lambda r: f'{C.hw_id(r[0])}-to-{C.hw_id(r[1])}')
def test_fpn_topdown_bwd_in_place(row):
    from graph_detr4d_amd import ops
    fine, coarse = row
    gf, gc, ref = C.fpn_topdown_case(fine, coarse)
    dgf, dgc = _in(gf), gc.to(DEV)
    what = f'fpn_topdown_bwd {row}'

    def launch(run):
        buf = run.out(gc.shape, holds=dgc)
        got = ops.fpn_topdown_bwd(dgf, buf)
        assert got.data_ptr() == buf.data_ptr()
        return dict(g_coarse=got)
    _contract(what, launch, lambda res: _err(what, res['g_coarse'], ref, FPN_TRAIN_TOL, fpn_ref.rel_err))


# ---- DCN -------------------------------------------------------------------------------------------------------------------------
def _per_image(what, planes, got, ref, tol):
    """test_dcn_gpu.test_dcn_kernel_crafted_offsets: an image whose reference is exactly zero is exactly zero here."""
    got = got.cpu()
    for i, name in enumerate(planes):
        if float(ref[i].abs().max()) == 0.0:
            assert float(got[i].abs().max()) == 0.0, f'{what} {name}: the reference is zero'
        else:
            _err(f'{what} {name}', got[i], ref[i], tol, dcn_ref.rel_err)


@pytest.mark.parametrize('row', C.DCN_OFFSET_ROWS, ids=lambda r: f'{r[0]}-s{r[1]}-{r[2]}x{r[3]}')
def test_dcn_offset_conv_fwd_dgrad_wgrad(row):
    from graph_detr4d_amd import ops
    cin, stride, h, w = row
    c = C.dcn_offset_case(*row)
    lib = _lib()
    image = ops.dcn_weight_image(c['weight'].to(DEV))
    dx, dbias, ddo, dweight = _in(c['x']), _in(c['bias']), _in(c['do']), _in(c['weight'])
    what = f'dcn_offset_conv_fwd {row}'
    _contract(what, lambda run: dict(out=ops.dcn_offset_conv_fwd(dx, image, dbias, stride=stride, out=run.out(c['ref'].shape))),
              lambda res: _err(what, res['out'], c['ref'], DCN_TOL, dcn_ref.rel_err))
    what = f'dcn_offset_conv_dgrad {row}'
    base = c['base'].to(DEV)

    def dgrad(run):
        buf = run.out(base.shape, holds=base)                                   # ADDED into dx, in place
        got = ops.dcn_offset_conv_dgrad(ddo, dweight, buf, stride=stride)
        assert got.data_ptr() == buf.data_ptr()
        return dict(dx=got)
    _contract(what, dgrad, lambda res: _err(what, res['dx'].cpu().double() - c['base'].double(), c['dx'], DCN_TRAIN_TOL, dcn_ref.rel_err))
    what = f'dcn_offset_conv_wgrad {row}'
    refs = dict(dW=c['dw'], db=c['db'])

    def launch(run, parts):
        ws = None if parts is None else _workspace(run, lib.gd4d_dcn_offset_conv_wgrad_workspace_bytes, cin, parts)
        return dict(zip(refs, ops.dcn_offset_conv_wgrad(ddo, dx, stride=stride, partitions=parts, outs=(run.out((27, cin, 3, 3)), run.out((27,))),
                                                        workspace=ws)))
    _partitioned(what, int(lib.gd4d_dcn_wgrad_tiles(N, h, w, stride)),
                 ops._dcn_partitions(lib, torch.device(DEV), N, cin, h, w, stride, None, 1), launch,
                 lambda res: [_err(f'{what} {k}', res[k], r, DCN_TRAIN_TOL, dcn_ref.rel_err) for k, r in refs.items()],
                 lambda n, a, b: _err(n, a, b, DCN_TRAIN_TOL, dcn_ref.rel_err))


def _dcn_inputs(c):
    om = torch.cat((c['offset'], c['mask']), dim=1)
    return _in(c['x']), _in(om), _in(c['dout']), _in(c['y']), _in(c['scale'])


@pytest.mark.parametrize('row', C.DCN_ROWS, ids=C.dcn_id)
def test_dcn_fwd_and_bwd_data_crafted_offsets(row):
    from graph_detr4d_amd import ops
    cin, cout, stride, h, w, planes = row
    c = C.dcn_case(*row)
    image, image_t = ops.dcn_weight_image(c['weight'].to(DEV)), ops.dcn_weight_image_t(c['weight'].to(DEV))
    dx, dom, ddout, dy, dscale = _dcn_inputs(c)
    ho, wo = C.out_hw(h, w, stride)
    what = f'dcn_fwd {C.dcn_id(row)}'
    _contract(what, lambda run: dict(out=ops.dcn_fwd(dx, dom, image, cout, stride=stride, out=run.out(c['ref'].shape))),
              lambda res: _per_image(what, planes, res['out'], c['ref'], DCN_TOL))
    for name, kw, ref in (('plain', {}, c['plain']), ('scale + relu', dict(y=dy, scale=dscale), c['masked'])):
        what = f'dcn_bwd_data {C.dcn_id(row)} {name}'

        def launch(run, want_dx=True):
            dxo = run.out(c['x'].shape, holds=torch.zeros(c['x'].shape, device=DEV)) if want_dx else None   # added into: zeros
            return dict(zip(('dx', 'doff'), ops.dcn_bwd_data(ddout, dx, dom, image_t, cout, stride=stride, dx=dxo, want_dx=want_dx,
                                                             doff=run.out((N, 27, ho, wo)), **kw)))

        def check(res):
            _per_image(f'{what} dx', planes, res['dx'], ref['x'], DCN_TRAIN_TOL)
            _per_image(f'{what} offset', planes, res['doff'][:, :18], ref['offset'], DCN_TRAIN_TOL)
            _per_image(f'{what} mask', planes, res['doff'][:, 18:], ref['mask'], DCN_TRAIN_TOL)
        both = _contract(what, launch, check, atomics=('dx',))
        only = _contract(f'{what} want_dx=False', lambda run: launch(run, False), lambda res: None)
        assert set(only) == {'doff'} and torch.equal(only['doff'], both['doff'])


@pytest.mark.parametrize('row', C.DCN_WGRAD_ROWS, ids=C.dcn_id)
def test_dcn_wgrad(row):
    from graph_detr4d_amd import ops
    cin, cout, stride, h, w, planes = row
    c = C.dcn_case(*row)
    lib = _lib()
    dx, dom, ddout, dy, dscale = _dcn_inputs(c)
    for name, kw, ref in (('plain', {}, c['plain']), ('scale + relu', dict(y=dy, scale=dscale), c['masked'])):
        what = f'dcn_wgrad {C.dcn_id(row)} {name}'
        refs = dict(dW=ref['weight'], dbias=ref['bias'])

        def launch(run, parts):
            ws = None if parts is None else _workspace(run, lib.gd4d_dcn_wgrad_workspace_bytes, cin, cout, parts)
            return dict(zip(refs, ops.dcn_wgrad(ddout, dx, dom, cout, stride=stride, partitions=parts, workspace=ws,
                                                outs=(run.out((cout, cin, 3, 3)), run.out((cout,))), **kw)))
        _partitioned(what, int(lib.gd4d_dcn_wgrad_tiles(N, h, w, stride)),
                     ops._dcn_partitions(lib, torch.device(DEV), N, cin, h, w, stride, None, 4), launch,
                     lambda res: [_err(f'{what} {k}', res[k], r, DCN_TRAIN_TOL, dcn_ref.rel_err) for k, r in refs.items()],
                     lambda n, a, b: _err(n, a, b, DCN_TRAIN_TOL, dcn_ref.rel_err))


# ---- DepthNet --------------------------------------------------------------------------------------------------------------------
def _max_err(got, ref):
    """test_depth_net_train_gpu.test_forward_train_mode's measure."""
    return float((got.double().cpu() - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize('row', C.DEPTH_ROWS, ids=C.depth_id)
def test_depth_net_kernels(row):
    """The launches of DepthNet's training node in its order (depth_net.py), every output guarded: depth_conv_raw (with partials unless
    frozen), depth_bn_stats, depth_bn_act_fwd, depth_bn_bwd, depth_conv_wgrad, the transposed-image data gradient; frozen also
    depth_conv_fwd, the inference launch, which must give the same map."""
    from graph_detr4d_amd import ops
    levels, frozen = row
    p = C.depth_params()
    xs, rs, fwd = C.depth_case(levels, frozen)
    lib = _lib()
    nl = len(levels)
    image, image_t = ops.depth_net_image(p['w'].to(DEV)), ops.depth_net_image_t(p['w'].to(DEV))
    dxs, drs = [_in(x) for x in xs], [_in(r) for r in rs]
    dbias, dgamma, dbeta, dgate, dmean, dvar = (_in(p[k]) for k in ('b', 'gamma', 'beta', 'gate', 'mean', 'var'))
    shapes = [x.shape for x in xs]
    tiles = ops.depth_conv_tiles(levels, N)
    tag = C.depth_id(row)

    def outs_of(run):
        return [run.out(s) for s in shapes]

    def per_level(res, key, refs, bound, metric, what):
        for i, (hw, r) in enumerate(zip(levels, refs)):
            _err(f'{what} {C.hw_id(hw)}', res[f'{key}{i}'], r, bound, metric)

    def named(key, tensors):
        return {f'{key}{i}': t for i, t in enumerate(tensors)}

    # y = conv + bias (and the per-tile partials)
    def raw(run):
        if frozen:
            return named('y', ops.depth_conv_raw(dxs, image, dbias, outs=outs_of(run)))
        ys, partials = ops.depth_conv_raw(dxs, image, dbias, want_partials=True, outs=outs_of(run), partials=run.out((max(tiles, 1), 2, 256)))
        return dict(named('y', ys), partials=partials)
    res = _contract(f'depth_conv_raw {tag}', raw,
                    lambda res: per_level(res, 'y', [f['y'] for f in fwd], DEPTH_FWD_TOL, _max_err, f'depth_conv_raw {tag}'))
    ys = [_in(res[f'y{i}']) for i in range(nl)]
    rm, rv = p['mean'].to(DEV).clone(), p['var'].to(DEV).clone()
    stats = ops.depth_bn_stats(None if frozen else _in(res['partials']), levels, N, dgamma, rm, rv, 0.0 if frozen else C.DEPTH_MOMENTUM,
                               C.DEPTH_EPS, frozen=frozen)
    dstats = _in(stats)
    outs = _contract(f'depth_bn_act_fwd {tag}', lambda run: named('out', ops.depth_bn_act_fwd(ys, dstats, dbeta, dgate, outs=outs_of(run))),
                     lambda res: per_level(res, 'out', [f['out'] for f in fwd], DEPTH_FWD_TOL, _max_err, f'depth_bn_act_fwd {tag}'))
    if frozen:
        _contract(f'depth_conv_fwd {tag}',
                  lambda run: named('out', ops.depth_conv_fwd(dxs, image, dbias, dmean, dvar, dgamma, dbeta, C.DEPTH_EPS, dgate, outs=outs_of(run))),
                  lambda res: per_level(res, 'out', [f['out'] for f in fwd], DEPTH_FWD_TOL, _max_err, f'depth_conv_fwd {tag}'))
    # the backward of the forward the DEVICE computed: its own ReLU mask (test_depth_net_train_gpu.py)
    bwd = [backward64(f, r, outs[f'out{i}'].cpu() > 0) for i, (f, r) in enumerate(zip(fwd, rs))]
    # a level with two values per channel under batch statistics: xhat = +-1, dy is the difference of terms that cancel to zero, so
    # its error is measured against the size of those terms (the frozen form of the same gradient) where that is the larger
    floor = [backward64(dict(f, frozen=True), r, outs[f'out{i}'].cpu() > 0) if not frozen and N * h * w == 2 else None
             for i, (f, r, (h, w)) in enumerate(zip(fwd, rs, levels))]

    def fro(i, key):
        def metric(got, ref):
            scale = ref.norm() if floor[i] is None else max(ref.norm(), floor[i][key].norm())
            return float((got.detach().double().cpu() - ref).norm() / scale)
        return metric

    def bn_bwd(run):
        small = run.out((3 + N, 256))
        ws = run.out((max(int(lib.gd4d_depth_bn_bwd_workspace_bytes(nl, N)) // 4, 1),))
        dys, g_gamma, g_beta, g_gate, g_bias = ops.depth_bn_bwd(drs, ys, dstats, dbeta, dgate, frozen=frozen, outs=outs_of(run), small=small,
                                                                workspace=ws)
        return dict(named('dy', dys), dgamma=g_gamma, dbeta=g_beta, dgate=g_gate, dbias=g_bias)

    def check_bn_bwd(res):
        for i, hw in enumerate(levels):
            _err(f'depth_bn_bwd {tag} dy {C.hw_id(hw)}', res[f'dy{i}'], bwd[i]['dy'], DEPTH_BWD_TOL, fro(i, 'dy'))
        for key, name in (('dgamma', 'dgamma'), ('dbeta', 'dbeta'), ('dgate', 'dg')):
            _err(f'depth_bn_bwd {tag} {key}', res[key], sum(b[name] for b in bwd), DEPTH_BWD_TOL, rel_fro)
        db = res['dbias'].double().cpu()
        if frozen:
            _err(f'depth_bn_bwd {tag} dbias', db, sum(b['db'] for b in bwd), DEPTH_BWD_TOL, rel_fro)
        else:                                  # zero up to rounding with batch statistics: test_depth_net_train_gpu's absolute bound
            bound = 1e-3 * sum(b['dy'].abs().sum((0, 2, 3)) / (N * h * w) if f is None else f['dy'].abs().sum((0, 2, 3)) / (N * h * w)
                               for b, f, (h, w) in zip(bwd, floor, levels))
            assert bool((db.abs() <= bound).all()), f'depth_bn_bwd {tag} dbias: {float(db.abs().max()):.2e}'
    res = _contract(f'depth_bn_bwd {tag}', bn_bwd, check_bn_bwd)
    dys = [_in(res[f'dy{i}']) for i in range(nl)]
    _contract(f'depth_conv_raw (transposed image) {tag}', lambda run: named('dx', ops.depth_conv_raw(dys, image_t, outs=outs_of(run))),
              lambda res: [_err(f'data gradient {tag} {C.hw_id(hw)}', res[f'dx{i}'], bwd[i]['dx'], DEPTH_BWD_TOL, fro(i, 'dx'))
                           for i, hw in enumerate(levels)])
    ref_dw = sum(b['dW'] for b in bwd)

    def wgrad(run, parts):
        ws = None if parts is None else _workspace(run, lib.gd4d_depth_conv_wgrad_workspace_bytes, parts)
        return dict(dW=ops.depth_conv_wgrad(dys, dxs, partitions=parts, out=run.out((256, 256, 3, 3)), workspace=ws))
    _partitioned(f'depth_conv_wgrad {tag}', tiles, max(1, min(tiles, _cus() // 8)), wgrad,
                 lambda res: _err(f'depth_conv_wgrad {tag}', res['dW'], ref_dw, DEPTH_BWD_TOL, rel_fro),
                 lambda n, a, b: _err(n, a, b, DEPTH_BWD_TOL, rel_fro))


def test_cam_gate_fwd():
    from graph_detr4d_amd import ops
    intr, ida00, sd, ref = C.cam_gate_case()
    keys = ('mlp.fc1.weight', 'mlp.fc1.bias', 'mlp.fc2.weight', 'mlp.fc2.bias', 'se.conv_reduce.weight', 'se.conv_reduce.bias',
            'se.conv_expand.weight', 'se.conv_expand.bias')
    dintr, dida, ws = _in(intr), _in(ida00), [_in(sd[k]) for k in keys]

    def check(res):                            # test_depth_net_gpu.py: rtol = atol = 1e-5 against the fp64 restatement
        torch.testing.assert_close(res['gate'].cpu(), ref.float(), rtol=1e-5, atol=1e-5)
    _contract('cam_gate_fwd', lambda run: dict(gate=ops.cam_gate_fwd(dintr, dida, *ws, out=run.out((N, 256)))), check)
    assert float(ref.max() - ref.min()) > 0.05


# ---- dense rows ------------------------------------------------------------------------------------------------------------------
def _abs_err(got, ref):
    return float((got.double().cpu() - ref).abs().max())


@pytest.mark.parametrize('m', C.DENSE_M)
def test_dense_rows(m):
    """The inputs and references are memory_contract_cases.py's; each bound is the one of the test named there."""
    from graph_detr4d_amd import ops
    for k, n in C.LINEAR_KN:                   # test_dense_gpu.test_linear_matches_fp64's bound
        x, w, b, ref = C.linear_case(m, k, n)
        dx, dw, db = _in(x), _in(w), _in(b)
        what = f'linear_fwd M = {m}, K = {k}, N = {n}'
        _contract(what, lambda run: dict(out=ops.linear_fwd(dx, dw, db, out=run.out((m, n)))),
                  lambda res: _err(what, res['out'], ref, 2e-5 * max(1.0, math.sqrt(k) / 4), _abs_err))
    c = C.dense_case(m)
    g = c['gemm']                              # test_gemm_gpu.test_gemm_bf16x3_matches_fp64's bound
    hi, lo = ops.split_bf16_fwd(g['w'].to(DEV))
    da, dhi, dlo, db = _in(g['a']), embedded(hi), embedded(lo), _in(g['b'])
    what = f'gemm_bf16x3_fwd M = {m}'
    _contract(what, lambda run: dict(out=ops.gemm_bf16x3_fwd(da, dhi, dlo, db, relu=True, out=run.out((m, C.GEMM_KN[1])))),
              lambda res: _err(what, res['out'], g['ref'], 4e-5 * max(1.0, g['scale'] / 8), _abs_err))
    p = c['mlp2']                              # test_head_pe_gpu.test_fused_two_layer_mlp_matches_fp64: rtol = atol = 2e-4
    img = ops.mlp2_image(p['w1'].to(DEV), p['b1'].to(DEV), p['w2'].to(DEV))
    dx, db2 = _in(p['x']), _in(p['b2'])
    _contract(f'mlp2_bf16x3_fwd M = {m}', lambda run: dict(out=ops.mlp2_bf16x3_fwd(dx, img, db2, out=run.out((m, 256)))),
              lambda res: torch.testing.assert_close(res['out'].cpu(), p['ref'], rtol=2e-4, atol=2e-4))
    v = c['heads']                             # test_cross_attn_late_gpu.test_value_proj_heads_matches_fp64: < 2e-5
    dagg, dwsum, dw, db = _in(v['agg']), _in(v['wsum']), _in(v['w']), _in(v['b'])
    what = f'value_proj_heads_fwd M = {m}'
    _contract(what, lambda run: dict(out=ops.value_proj_heads_fwd(dagg, dwsum, dw, db, out=run.out((m, 256)))),
              lambda res: _err(what, res['out'], v['ref'], 2e-5, _abs_err))
    # test_dense_gpu.test_layernorm_matches_aten (< 2e-5) and test_layernorm_bwd_matches_fp64 (dx < 5e-5, dgamma / dbeta < 1e-3 ...)
    ln = c['ln']
    dx, dr, dgam, dbet, ddy = (_in(ln[k]) for k in ('x', 'res', 'gamma', 'beta', 'dy'))
    for (relu, with_res), ref in ln['fwd'].items():
        what = f'layernorm_fwd M = {m} relu {relu} res {with_res}'
        _contract(what, lambda run: dict(out=ops.layernorm_fwd(dx, dgam, dbet, res=dr if with_res else None, relu=relu, out=run.out((m, C.LN_C)))),
                  lambda res: _err(what, res['out'], ref, 2e-5, _abs_err))
    for relu, (rx, rg, rb) in ln['bwd'].items():
        what = f'layernorm_bwd M = {m} relu {relu}'
        small = 1e-3 * max(1.0, math.sqrt(m) / 30)

        def check(res):
            _err(f'{what} dx', res['dx'], rx, 5e-5, _abs_err)
            _err(f'{what} dgamma', res['dgamma'], rg, small, _abs_err)
            _err(f'{what} dbeta', res['dbeta'], rb, small, _abs_err)
        _contract(what, lambda run: dict(zip(('dx', 'dgamma', 'dbeta'), ops.layernorm_bwd(
            dx, dgam, dbet, ddy, relu=relu, outs=(run.out((m, C.LN_C)), run.out((C.LN_C,)), run.out((C.LN_C,)))))), check)
