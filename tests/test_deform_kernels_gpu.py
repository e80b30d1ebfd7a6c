"""Deform3DCrossAttn's kernels (gd4d_cross_attn*.hip: plan, gathers, value projection per head, projected-value backward, raw-pyramid
backward with its bucket sort) through ops.*, against the fp64 arbiter of tests/deform_cases.py on its cases: samples in the half-pixel
band beyond each border and corner of the maps at both ends of every pyramid allocation, a sample behind a camera, samples two cameras
share, a query nobody sees, samples whose cell touches the coarsest map only, 32 queries inside one coarse cell, batch 2 with the
reference's row pairing, 4 heads on 3 levels with a one-row coarsest map.  Every entry of every output is compared.

Tolerance rule (detr3d_cases.FACTOR): the same operation evaluated in fp32 by torch on the CPU - the oracle for the projected-value
kernels, the raw association (gather raw pixels, then W agg + b wsum per head) for the raw-pyramid ones - has an error against fp64 per
output; a kernel gets 4 x that, computed at run time and printed beside the kernel's error (docs/measurements_r42.md holds the table).
Masks are compared bit for bit; the row of a query nobody sees and the gradients of everything no visible sample feeds are exactly 0.

The memory contract of the same launches (contract.py, the discipline of test_memory_contract_gpu.py) on `batch2` and `narrow`: inputs
embedded in NaN, pyramid copies and every output inside guarded buffers - PyramidGrad's own through alloc=, its records and sorted
records sized from the counts to the record."""
import pytest
import torch

import contract as K
import deform_cases as D
import detr3d_ref as R
from graph_detr4d_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = K.DEV
GEOM = (D.PC_RANGE, D.IMG_H, D.IMG_W)
NAMES = list(D.SHAPES)
U8, I32 = torch.uint8, torch.int32


def _dev(cs, embed=False, feats=None):
    """The case on the device; embed: every tensor inside NaNs (guarded.embedded)."""
    put = K.as_input if embed else (lambda t: t.to(DEV).contiguous())
    feats = cs.feats if feats is None else feats
    d = dict(feats=[put(f) for f in feats], ref=put(cs.ref), offsets=put(cs.offsets), attn=put(cs.attn), cam=put(cs.cam),
             l2i=put(cs.lidar2img), w_v=put(cs.w_v), b_v=put(cs.b_v), gout=put(cs.grad_out), gout2=put(cs.grad_out2),
             value=put(D.value32(cs, feats)), embed=embed)
    if coarse_ok(cs):
        d['coarse'] = put(D.value32(cs, feats, slice(2, None)).reshape(cs.B * cs.N, -1, D.C))
    d['args'] = (d['ref'], d['offsets'], d['attn'], d['cam'], d['l2i'], *GEOM)
    return d


def coarse_ok(cs):
    """gd4d_cross_attn_agg_items_coarse_fwd and the record count riding in the gather: 8 heads on 4 levels."""
    return cs.Hh == 8 and cs.L == 4


def _o(run):
    """shape -> a guarded output of the run, or None (the wrapper allocates)."""
    return (lambda shape, **kw: None) if run is None else run.out


def _zeros(run, shape, dtype=torch.float32):
    z = torch.zeros(shape, device=DEV, dtype=dtype)
    return z if run is None else run.out(shape, holds=z, dtype=dtype)


# ---- the routes ---------------------------------------------------------------------------------------------------------------------
def route_fwd(cs, d, order, run=None, head_major=False, value=None):
    o = _o(run)
    value = d['value'] if value is None else value
    if head_major:
        value = value.permute(0, 2, 1, 3).contiguous()
    vis = (cs.B, cs.N, cs.Q, cs.Hh, cs.P)
    out, mask, uv = ops.cross_attn_fwd(value, cs.levels, *d['args'], out=o((cs.B, cs.Q, D.C)), head_major=head_major, query_order=order,
                                       mask_out=o(vis, dtype=U8), uv_out=o(vis + (2,)), want_mask=True, want_uv=True)
    return dict(out=out, mask=mask, uv=uv)


def route_agg(cs, d, order, fused=False, dtype=torch.float32):
    """gd4d_cross_attn_agg_fwd (B = 1) + gd4d_value_proj_heads_fwd, or value_proj in the gather's epilogue."""
    cl, shp = ops.pyramid_channels_last_fwd(d['feats'], out_dtype=dtype)
    if fused:
        out, mask = ops.cross_attn_agg_fwd(cl, shp, *d['args'], cs.Hh, want_mask=True, query_order=order, vp_weight=d['w_v'], vp_bias=d['b_v'])
        return dict(out=out, mask=mask)
    agg, wsum, mask = ops.cross_attn_agg_fwd(cl, shp, *d['args'], cs.Hh, want_mask=True, query_order=order)
    return dict(out=ops.value_proj_heads_fwd(agg, wsum, d['w_v'], d['b_v']), mask=mask, wsum=wsum)


def pyramid(cs, d, source, run=None, dtype=torch.float32):
    o = _o(run)
    rows, s = cs.B * cs.N, sum(h * w for h, w in cs.levels)
    if source == 'planar':
        sp, shp = ops.pyramid_slice_planar_fwd(d['feats'], out=o((8, rows, s, 32), dtype=dtype), out_dtype=dtype)
        return ops.PyramidView.slice_planar(sp, shp)
    if source == 'pixel_major':
        cl, shp = ops.pyramid_channels_last_fwd(d['feats'], out=o((rows, s, D.C), dtype=dtype), out_dtype=dtype)
        return ops.PyramidView.pixel_major(cl, shp)
    levels = [f.reshape(rows, *f.shape[-3:]).to(dtype).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2) for f in d['feats']]
    return ops.PyramidView.channels_last_levels([K.embedded(t) for t in levels] if d['embed'] else levels)


def _plan(cs, d, pyr, order, run, items=False, both=False):
    o = _o(run)
    vis = (cs.B, cs.N, cs.Q, cs.Hh, cs.P)
    seed = None
    if run is not None and not both:                        # (both=True takes no buffer from outside: its plan stays the allocator's)
        nbytes = ops.cross_attn_plan_bytes(cs.B, cs.N, cs.Q, cs.Hh, cs.P)
        seed = ops.Plan(run.out((nbytes,), dtype=U8), order, pyr, cs.B, cs.Q, cs.Hh, run.out((cs.B, cs.Q, cs.Hh)))
    return ops.cross_attn_plan_fwd(pyr, *d['args'], cs.Hh, plan=seed, query_order=order, items=items, both=both, want_mask=True,
                                   want_uv=True, mask_out=o(vis, dtype=U8), uv_out=o(vis + (2,)))


def route_sliced(cs, d, pyr, order, form='pairs', run=None):
    """plan + gd4d_cross_attn_agg_sliced_fwd / _items_fwd (+ the record count riding) + gd4d_value_proj_heads_fwd."""
    o = _o(run)
    plan, mask, uv = _plan(cs, d, pyr, order, run, items=form == 'items', both=form.startswith('both'))
    if form == 'both+count':
        agg = ops.cross_attn_agg_sliced_fwd(plan, agg=o((cs.B, cs.Q, cs.Hh, D.C)), count=(ops.PyramidGrad(pyr, 1, cs.B, cs.Q, cs.Hh), 0))
        assert agg is not None, 'the gather refused to carry the record count'
    else:
        agg = ops.cross_attn_agg_sliced_fwd(plan, agg=o((cs.B, cs.Q, cs.Hh, D.C)))
    out = ops.value_proj_heads_fwd(agg, plan.wsum, d['w_v'], d['b_v'], out=o((cs.B, cs.Q, D.C)))
    return dict(out=out, agg=agg, wsum=plan.wsum, mask=mask, uv=uv)


def route_coarse(cs, d, pyr, order, run=None):
    """Levels 0, 1 gathered raw, levels 2, 3 from this layer's projected rows: value_proj_heads_fwd(agg, wsum of the fine levels) + pagg."""
    o = _o(run)
    plan, mask, uv = _plan(cs, d, pyr, order, run, items=True)
    agg, pagg = ops.cross_attn_agg_coarse_fwd(plan, ops.CoarseValues(d['coarse'], cs.levels[2:]), agg=o((cs.B, cs.Q, cs.Hh, D.C)),
                                              pagg=o((cs.B, cs.Q, D.C)))
    proj = ops.value_proj_heads_fwd(agg, plan.wsum, d['w_v'], d['b_v'], out=o((cs.B, cs.Q, D.C)))
    return dict(proj=proj, pagg=pagg, agg=agg, wsum_fine=plan.wsum, mask=mask, uv=uv)


def projected_backward(cs, d, order, run=None):
    o = _o(run)
    outs = ws = None
    if run is not None:
        outs = (_zeros(run, d['value'].shape), o((cs.B, cs.Q, 3)), o((cs.B, cs.Q, cs.Hh, cs.P, 3)), o((cs.B, cs.Q, cs.Hh, cs.L, cs.P)),
                o((cs.B, cs.Q, cs.N)))
        nbytes = int(_lib.load().gd4d_cross_attn_bwd_workspace_bytes(cs.B, cs.Q, cs.Hh, cs.L, cs.P))
        ws = o((nbytes,), dtype=U8) if nbytes else None
    res = ops.cross_attn_bwd(d['value'], cs.levels, *d['args'], d['gout'], query_order=order, outs=outs, workspace=ws)
    return dict(zip(('grad_value', 'grad_ref', 'grad_offsets', 'grad_attn_logits', 'grad_cam_logits'), res))


def chain_rule(cs, grad_value):
    """grad_value -> the pyramid's gradient through value_proj, in fp64 on the host (test_cross_attn_sliced_bwd_gpu._projected_backward)."""
    gflat = grad_value.cpu().reshape(cs.B * cs.N, -1, D.C).double() @ cs.w_v.double()
    out, s = [], 0
    for h, w in cs.levels:
        out.append(gflat[:, s:s + h * w].permute(0, 2, 1).reshape(cs.B, cs.N, D.C, h, w))
        s += h * w
    return out


def raw_backward(cs, d, order, layers=1, riding=False, run=None, short=0):
    """The route training runs, as test_cross_attn_sliced_bwd_gpu._raw_backward composes it; layer 1 is fed grad_out2.  riding: the
    records' slots are handed out in the forward gather's launch.  With a run every buffer is guarded, PyramidGrad's own through alloc=,
    `records` and `sorted` sized from the counts (8 bytes per record) less `short` records."""
    o = _o(run)
    b, n, q, hh, nl = cs.B, cs.N, cs.Q, cs.Hh, cs.L
    pyr = pyramid(cs, d, 'planar', run)
    sink = None

    def alloc(what, shape, dtype, zero):
        if what in ('records', 'sorted'):
            shape = (8 * max(int(sink.count.sum()) - (short if what == 'records' else 0), 1),)
        return _zeros(run, shape, dtype) if zero else run.out(shape, dtype=dtype)
    sink = ops.PyramidGrad(pyr, layers, b, q, hh, alloc=None if run is None else alloc)
    status = _zeros(run, (1,), I32)
    first = None
    for layer in range(layers):
        gout = d['gout'] if layer == 0 else d['gout2']
        plan, _, _ = _plan(cs, d, pyr, order, run, both=riding)
        if riding:
            assert ops.cross_attn_agg_sliced_fwd(plan, count=(sink, layer)) is not None, 'the gather refused to carry the record count'
        gagg, beta = ops.value_proj_heads_bwd(gout, d['w_v'], d['b_v'], hh, grad_agg=sink.grad_agg_rows(layer), beta=o((b, q, hh)))
        dpart = ops.cross_attn_dot_sliced(plan, gagg, dpart=o((ops.cross_attn_dot_bytes(b, n, q, hh, cs.P),), dtype=U8))
        outs = ws = None
        if run is not None:
            outs = (o((b, q, 3)), o((b, q, hh, cs.P, 3)), o((b, q, hh, nl, cs.P)), o((b, q, n)))
            nbytes = int(_lib.load().gd4d_cross_attn_bwd_workspace_bytes(b, q, hh, nl, cs.P))
            ws = o((nbytes,), dtype=U8) if nbytes else None
        res = ops.cross_attn_plan_bwd(plan, dpart, beta, *d['args'], status=status, outs=outs, workspace=ws)
        if not riding:
            sink.add_layer(layer, plan)
        first = res if first is None else first
    grads = None if run is None else [o((b * n, D.C, h, w)) for h, w in cs.levels]
    gfeats = sink.finish(grads=grads)
    res = dict(zip(('grad_ref', 'grad_offsets', 'grad_attn_logits', 'grad_cam_logits'), first), status=status)
    res['grad_feats' if layers == 1 else 'grad_feats2'] = gfeats
    return res


# ---- the checks ---------------------------------------------------------------------------------------------------------------------
def _cpu(x):
    return [_cpu(e) for e in x] if isinstance(x, (list, tuple)) else x.cpu()


def _hold(label, kernel, host):
    """Print the kernel's error next to the fp32 host error and the bound, then assert every bound."""
    late = []
    for key, e in kernel.items():
        bound = D.FACTOR * host[key]
        print(f'FIG | {label} | {key} | {e:.2e} | {host[key]:.2e} | {e / host[key] if host[key] else float("nan"):.2f}')
        if not e <= bound:
            late.append(f'{key}: {e:.2e} > {bound:.2e}')
    assert not late, f'{label}: ' + '; '.join(late)


def check_forward(cs, label, res, want, host, out_want=None):
    got = {k: _cpu(v) for k, v in res.items()}
    if 'proj' in got:
        got['out'] = got['proj'] + got['pagg']
    assert torch.equal(got['mask'].bool(), want['mask']), f'{label}: mask differs from the arbiter'
    nobody = D.of_kind(cs, 'nobody')
    assert bool((got['out'][:, nobody] == 0).all()), f'{label}: the row of a query nobody sees'
    for key in ('wsum', 'wsum_fine', 'agg'):
        assert key not in got or bool((got[key][:, nobody] == 0).all()), f'{label}: {key} of a query nobody sees'
    ref = want if out_want is None else dict(out=out_want)
    _hold(label, D.figures(cs, {k: got.get(k) for k in ('out', 'wsum', 'wsum_fine') if k in ref}, ref), host)
    return got


def exact_zeros(cs, label, got, want):
    """What no visible sample feeds is exactly zero, in the arbiter and in the kernel: grad_ref / grad_offsets of a query (a sample)
    that no camera sees, grad_cam_logits of a (camera, query) without a visible sample (through the reference's view of the (Q, N)
    logits as (N, Q)), grad_attn_logits of a (batch, query, head) whose softmax feeds no visible sample of the rows paired with it."""
    vis = want['mask']                                                              # (B, N, Q, Hh, P)
    b, n = cs.B, cs.N
    rows = vis.reshape(b * n, *vis.shape[2:])
    live = torch.stack([rows[bb::b].flatten(3).any(3).any(0) for bb in range(b)])   # (B, Q, Hh): rows i with i % B == bb
    dead = {'grad_ref': ~vis.permute(0, 2, 1, 3, 4).flatten(2).any(2), 'grad_offsets': ~vis.any(1), 'grad_attn_logits': ~live}
    cam_dead = ~vis.flatten(3).any(3)                                               # (B, N, Q)
    for src in (want, got):
        for key, sel in dead.items():
            assert bool(sel.any()) and bool((src[key].reshape(want[key].shape)[sel] == 0).all()), f'{label}: {key} that nothing feeds'
        assert bool((src['grad_cam_logits'].reshape(b, n, cs.Q)[cam_dead] == 0).all()), f'{label}: grad_cam_logits that nothing feeds'


def check_backward(cs, label, res, want, host):
    got = {k: _cpu(v) for k, v in res.items()}
    if 'status' in got:
        assert int(got.pop('status')) == 0, f'{label}: an item count of the backward disagrees with the plan'
    if 'grad_value' in got:
        got['grad_feats'] = chain_rule(cs, got['grad_value'])
    exact_zeros(cs, label, got, want)
    _hold(label, D.figures(cs, got, want), host)
    return got


def block_alone(name, raw, run_route):
    cs = D.case(name)
    sub = D.subset(cs, cs.block)
    want, host = D.reference(name, raw=raw, block_only=True)
    got = {k: _cpu(v) for k, v in run_route(sub, _dev(sub)).items()}
    gf = chain_rule(sub, got['grad_value']) if 'grad_value' in got else got['grad_feats']
    assert len(D.block_pixels(cs)) >= 1
    fig = R.rel_err(D.block_grad(sub, gf), D.block_grad(sub, want['grad_feats']))
    _hold(f'{name} {"raw" if raw else "projected"} backward', {'block grad_feats': fig}, host)


# ---- values -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_forward_routes(name):
    """Every forward route against the one fp64 out, with and without the locality order (scheduling only: the same bits)."""
    cs = D.case(name)
    D.check_case(cs)
    want, host_p = D.reference(name)
    _, host_r = D.reference(name, raw=True)
    d = _dev(cs)
    plain = {}
    for tag, order in (('plain', None), ('order', ops.query_order_fwd(d['ref'], D.PC_RANGE))):
        routes = {'fwd pixel-major': (host_p, lambda: route_fwd(cs, d, order)),
                  'fwd head-major': (host_p, lambda: route_fwd(cs, d, order, head_major=True))}
        if cs.B == 1:                                       # (gd4d_cross_attn_agg_fwd refuses B > 1: test_b2_is_refused)
            routes['agg + heads'] = (host_r, lambda: route_agg(cs, d, order))
            routes['agg fused value_proj'] = (host_r, lambda: route_agg(cs, d, order, fused=True))
        for source in ('planar', 'pixel_major', 'nhwc'):
            routes[f'pairs {source}'] = (host_r, lambda s=source: route_sliced(cs, d, pyramid(cs, d, s), order))
        routes['items planar'] = (host_r, lambda: route_sliced(cs, d, pyramid(cs, d, 'planar'), order, 'items'))
        routes['items nhwc'] = (host_r, lambda: route_sliced(cs, d, pyramid(cs, d, 'nhwc'), order, 'items'))
        routes['both planar'] = (host_r, lambda: route_sliced(cs, d, pyramid(cs, d, 'planar'), order, 'both'))
        if coarse_ok(cs):
            routes['both + count planar'] = (host_r, lambda: route_sliced(cs, d, pyramid(cs, d, 'planar'), order, 'both+count'))
            routes['coarse planar'] = (host_r, lambda: route_coarse(cs, d, pyramid(cs, d, 'planar'), order))
        for label, (host, launch) in routes.items():
            got = check_forward(cs, f'{name} | {label} {tag}', launch(), want, host)
            if tag == 'plain':
                plain[label] = got
            else:
                assert torch.equal(got['out'], plain[label]['out']), f'{label}: the locality order changed the result'


@pytest.mark.parametrize('name', NAMES)
def test_forward_bf16_storage(name):
    """One bf16 run per route that stores bf16: the projected value rounded (gd4d_cross_attn_fwd), the pyramid rounded (the copies'
    out_dtype) - against the arbiter fed the same rounded tensors, as test_fused_kernel_bf16_values does; the budget is the fp32
    host's on those inputs."""
    cs = D.case(name)
    want, _ = D.reference(name)
    bf = torch.bfloat16
    d = _dev(cs)
    out16, host = D.reference_bf16(name, 'value')
    check_forward(cs, f'{name} | bf16 value fwd', route_fwd(cs, d, None, value=D.bf16_value(cs).to(DEV)), want, host, out16)
    out16, host = D.reference_bf16(name, 'feats')
    d = _dev(cs, feats=[f.bfloat16().float() for f in cs.feats])                  # (rounding twice changes nothing; the coarse rows follow)
    routes = {'pairs planar': lambda: route_sliced(cs, d, pyramid(cs, d, 'planar', dtype=bf), None),
              'items pixel_major': lambda: route_sliced(cs, d, pyramid(cs, d, 'pixel_major', dtype=bf), None, 'items'),
              'pairs nhwc': lambda: route_sliced(cs, d, pyramid(cs, d, 'nhwc', dtype=bf), None)}
    if cs.B == 1:
        routes['agg + heads'] = lambda: route_agg(cs, d, None, dtype=bf)
    if coarse_ok(cs):
        routes['coarse planar'] = lambda: route_coarse(cs, d, pyramid(cs, d, 'planar', dtype=bf), None)
    for label, launch in routes.items():
        check_forward(cs, f'{name} | bf16 pyramid {label}', launch(), want, host, out16)


@pytest.mark.parametrize('name', NAMES)
def test_projected_value_backward(name):
    """gd4d_cross_attn_bwd: all five gradients against fp64 autograd, the pyramid's through value_proj's chain rule in fp64."""
    cs = D.case(name)
    want, host = D.reference(name)
    d = _dev(cs)
    order = ops.query_order_fwd(d['ref'], D.PC_RANGE)
    got = check_backward(cs, f'{name} | projected backward', projected_backward(cs, d, order), want, host)
    again = check_backward(cs, f'{name} | projected backward plain', projected_backward(cs, d, None), want, host)
    for key in ('grad_ref', 'grad_offsets', 'grad_attn_logits', 'grad_cam_logits'):                 # fixed order; grad_value: atomic adds
        assert torch.equal(got[key], again[key]), f'{key} differs between two calls'
    block_alone(name, False, lambda sub, dd: projected_backward(sub, dd, None))


@pytest.mark.parametrize('name', NAMES)
def test_raw_pyramid_backward(name):
    """The route training runs, with one layer and with two on one pyramid (the second fed grad_out2: the fp64 sum of both layers'
    gradients), and with the record count riding in the forward gather."""
    cs = D.case(name)
    want, host = D.reference(name, raw=True)
    d = _dev(cs)
    order = ops.query_order_fwd(d['ref'], D.PC_RANGE)
    one = check_backward(cs, f'{name} | raw backward', raw_backward(cs, d, order), want, host)
    two = check_backward(cs, f'{name} | raw backward 2 layers', raw_backward(cs, d, order, layers=2), want, host)
    for key in ('grad_ref', 'grad_offsets', 'grad_attn_logits', 'grad_cam_logits'):                 # test_query_side_gradients_are_bit_reproducible
        assert torch.equal(one[key], two[key]), f'{key} differs between two calls'
    check_backward(cs, f'{name} | raw backward plain', raw_backward(cs, d, None), want, host)
    if coarse_ok(cs):
        check_backward(cs, f'{name} | raw backward count in gather', raw_backward(cs, d, order, riding=True), want, host)
        check_backward(cs, f'{name} | raw backward 2 layers count in gather', raw_backward(cs, d, order, layers=2, riding=True), want, host)
    block_alone(name, True, lambda sub, dd: raw_backward(sub, dd, None))


# ---- the memory contract of the same launches -----------------------------------------------------------------------------------------
def _results(res, *drop):
    return {k: v for k, v in res.items() if k not in drop}


@pytest.mark.parametrize('name', ['batch2', 'narrow'])
def test_memory_contract_forward(name):
    cs = D.case(name)
    want, host_p = D.reference(name)
    _, host_r = D.reference(name, raw=True)
    e = _dev(cs, embed=True)
    order = ops.query_order_fwd(e['ref'], D.PC_RANGE)
    what = f'{name} | contract fwd pixel-major'
    K.contract(what, lambda run: route_fwd(cs, e, order, run), lambda res: check_forward(cs, what, res, want, host_p))
    for source, form in (('planar', 'pairs'), ('planar', 'items'), ('pixel_major', 'pairs'), ('pixel_major', 'items'), ('nhwc', 'pairs'),
                         ('nhwc', 'items')):
        what = f'{name} | contract {form} {source}'
        K.contract(what, lambda run: route_sliced(cs, e, pyramid(cs, e, source, run), order, form, run),
                   lambda res: check_forward(cs, what, res, want, host_r))
    if coarse_ok(cs):
        what = f'{name} | contract coarse planar'
        K.contract(what, lambda run: route_coarse(cs, e, pyramid(cs, e, 'planar', run), order, run),
                   lambda res: check_forward(cs, what, res, want, host_r))
        # the gather that carries the record count is launched beside ops._call (its wrapper reads the return code first) and both=True
        # takes no plan buffer from outside (wsum stays the wrapper's): guards, finiteness, bounds and bits of the rest, without the
        # "handed to the library" clause
        what = f'{name} | contract both + count planar'
        K.contract(what, lambda run: _results(route_sliced(cs, e, pyramid(cs, e, 'planar', run), order, 'both+count', run), 'wsum'),
                   lambda res: check_forward(cs, what, res, want, host_r), native=False)


@pytest.mark.parametrize('name', ['batch2', 'narrow'])
def test_memory_contract_backward(name):
    """Query-side gradients: the same bits over two runs (every partial sum has its slot and a fixed order).  grad_value (atomic adds)
    and the pyramid's gradient (the atomic slot hand-out of the bucket fill, test_query_side_gradients_are_bit_reproducible): two runs
    agree to ATOMICS_TOL."""
    cs = D.case(name)
    want, host_p = D.reference(name)
    _, host_r = D.reference(name, raw=True)
    e = _dev(cs, embed=True)
    order = ops.query_order_fwd(e['ref'], D.PC_RANGE)
    what = f'{name} | contract projected backward'
    K.contract(what, lambda run: projected_backward(cs, e, order, run), lambda res: check_backward(cs, what, res, want, host_p),
               atomics=('grad_value',))
    for layers in (1, 2):
        what = f'{name} | contract raw backward {layers} layers'

        def launch(run):
            res = raw_backward(cs, e, order, layers=layers, run=run)
            key = 'grad_feats' if layers == 1 else 'grad_feats2'
            return dict(_results(res, key), **{f'{key}[{l}]': g for l, g in enumerate(res[key])})

        def check(res):
            key = 'grad_feats' if layers == 1 else 'grad_feats2'
            check_backward(cs, what, dict({k: v for k, v in res.items() if '[' not in k}, **{key: [res[f'{key}[{l}]'] for l in range(cs.L)]}),
                           want, host_r)
        K.contract(what, launch, check, atomics=tuple(f'grad_feats{"" if layers == 1 else "2"}[{l}]' for l in range(cs.L)))
