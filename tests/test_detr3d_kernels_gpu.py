"""The four entry points of gd4d_detr3d.hip (gd4d_detr3d_fwd / _bwd, gd4d_detr3d_v2_fwd / _bwd) as kernels, through ops.*, against the
fp64 restatement tests/detr3d_ref.py (autograd for the gradients) on the cases of tests/detr3d_cases.py: channel counts below, at and
above the workgroup size, a head width that is no power of two, 1 to 4 levels, batch 2, samples beyond each border and each corner of the
map, cameras behind the point, offsets of +-3e9 pixels, and 32 queries whose atomic adds meet on the same pixels.  Every entry of every
output is compared; nothing is excluded.

Tolerance rule: the same restatement is evaluated in fp32 by torch on the CPU; its error against fp64, per output tensor and over the
tensor's largest |entry| (grad_logits / grad_offsets: per (query, camera, head) row, detr3d_ref.row_rel_err), is the error of honest
fp32 arithmetic for this operation and these inputs.  A kernel gets 4 x that (its sums run in another order; expf and the division
differ from the host's by an ulp or two).  The bound is computed at run time and printed beside the kernel's error; as measured on one
MI355X and its host (fp32 host error -> bound, then the kernel's error; the largest kernel / host ratio is 1.7; the host's figure moves
in its third digit from one CPU to another; docs/measurements_r35.md):

    base    v1 out               2.65e-06 -> 1.06e-05   (kernel 2.64e-06)
    base    v1 sampled           4.86e-06 -> 1.94e-05   (kernel 4.98e-06)
    base    v1 grad_ref          1.55e-06 -> 6.19e-06   (kernel 1.48e-06)
    base    v1 grad_logits       5.74e-06 -> 2.30e-05   (kernel 7.47e-06)
    base    v1 grad_feats[0]     3.00e-06 -> 1.20e-05   (kernel 3.79e-06)
    base    v1 grad_feats[1]     1.60e-06 -> 6.41e-06   (kernel 1.72e-06)
    base    v1 grad_feats[2]     7.59e-07 -> 3.04e-06   (kernel 7.71e-07)
    base    v1 grad_feats[3]     4.51e-07 -> 1.80e-06   (kernel 4.19e-07)
    base    v1 block grad_feats  5.68e-07 -> 2.27e-06   (kernel 4.97e-07)
    narrow  v1 out               1.06e-06 -> 4.23e-06   (kernel 1.39e-06)
    narrow  v1 sampled           1.81e-06 -> 7.25e-06   (kernel 2.02e-06)
    narrow  v1 grad_ref          3.28e-07 -> 1.31e-06   (kernel 2.10e-07)
    narrow  v1 grad_logits       3.17e-06 -> 1.27e-05   (kernel 3.08e-06)
    narrow  v1 grad_feats[0]     1.02e-06 -> 4.09e-06   (kernel 1.25e-06)
    narrow  v1 grad_feats[1]     6.19e-07 -> 2.48e-06   (kernel 6.24e-07)
    narrow  v1 grad_feats[2]     3.25e-07 -> 1.30e-06   (kernel 4.90e-07)
    narrow  v1 block grad_feats  3.49e-07 -> 1.40e-06   (kernel 3.65e-07)
    ragged  v1 out               1.89e-07 -> 7.56e-07   (kernel 1.89e-07)
    ragged  v1 sampled           1.05e-06 -> 4.21e-06   (kernel 1.05e-06)
    ragged  v1 grad_ref          4.60e-07 -> 1.84e-06   (kernel 4.60e-07)
    ragged  v1 grad_logits       6.05e-07 -> 2.42e-06   (kernel 4.11e-07)
    ragged  v1 grad_feats[0]     1.44e-07 -> 5.78e-07   (kernel 2.12e-07)
    ragged  v1 block grad_feats  2.10e-07 -> 8.39e-07   (kernel 1.82e-07)
    wide    v1 out               4.70e-06 -> 1.88e-05   (kernel 4.68e-06)
    wide    v1 sampled           5.64e-06 -> 2.25e-05   (kernel 5.64e-06)
    wide    v1 grad_ref          4.66e-07 -> 1.86e-06   (kernel 5.02e-07)
    wide    v1 grad_logits       1.13e-05 -> 4.53e-05   (kernel 1.13e-05)
    wide    v1 grad_feats[0]     3.18e-06 -> 1.27e-05   (kernel 3.16e-06)
    wide    v1 grad_feats[1]     1.50e-06 -> 6.02e-06   (kernel 1.52e-06)
    wide    v1 block grad_feats  1.57e-06 -> 6.27e-06   (kernel 1.57e-06)
    base    v2 out               3.65e-06 -> 1.46e-05   (kernel 3.64e-06)
    base    v2 grad_ref          9.80e-07 -> 3.92e-06   (kernel 8.89e-07)
    base    v2 grad_logits       2.38e-05 -> 9.51e-05   (kernel 2.38e-05)
    base    v2 grad_offsets      1.06e-05 -> 4.24e-05   (kernel 1.09e-05)
    base    v2 grad_feats[0]     3.62e-06 -> 1.45e-05   (kernel 3.62e-06)
    base    v2 grad_feats[1]     1.29e-06 -> 5.16e-06   (kernel 1.32e-06)
    base    v2 grad_feats[2]     7.23e-07 -> 2.89e-06   (kernel 8.15e-07)
    base    v2 grad_feats[3]     5.24e-07 -> 2.10e-06   (kernel 5.21e-07)
    base    v2 block grad_feats  4.69e-07 -> 1.88e-06   (kernel 4.76e-07)
    narrow  v2 out               1.44e-06 -> 5.75e-06   (kernel 1.25e-06)
    narrow  v2 grad_ref          7.75e-07 -> 3.10e-06   (kernel 8.35e-07)
    narrow  v2 grad_logits       8.28e-06 -> 3.31e-05   (kernel 7.47e-06)
    narrow  v2 grad_offsets      5.59e-06 -> 2.24e-05   (kernel 4.72e-06)
    narrow  v2 grad_feats[0]     1.16e-06 -> 4.63e-06   (kernel 1.17e-06)
    narrow  v2 grad_feats[1]     4.70e-07 -> 1.88e-06   (kernel 4.69e-07)
    narrow  v2 grad_feats[2]     4.96e-07 -> 1.99e-06   (kernel 3.66e-07)
    narrow  v2 block grad_feats  5.00e-07 -> 2.00e-06   (kernel 3.88e-07)
    ragged  v2 out               1.59e-07 -> 6.35e-07   (kernel 1.99e-07)
    ragged  v2 grad_ref          4.12e-07 -> 1.65e-06   (kernel 4.51e-07)
    ragged  v2 grad_logits       0.00e+00 -> 0.00e+00   (kernel 0.00e+00)
    ragged  v2 grad_offsets      4.78e-07 -> 1.91e-06   (kernel 7.93e-07)
    ragged  v2 grad_feats[0]     1.72e-07 -> 6.87e-07   (kernel 2.85e-07)
    ragged  v2 block grad_feats  1.18e-07 -> 4.71e-07   (kernel 1.39e-07)
    wide    v2 out               4.82e-06 -> 1.93e-05   (kernel 4.84e-06)

Masks are compared bit for bit; rows of an invisible camera and grad_ref of a query that no camera sees are exactly 0; everything but
grad_feats (atomic adds) is the same bits over two runs."""
import ctypes

import pytest
import torch

import detr3d_cases as D
import detr3d_ref as R
from graph_detr4d_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GEOM = (D.PC_RANGE, D.IMG_H, D.IMG_W)
NAMES = list(D.SHAPES)
V2_TRAINABLE = [n for n in NAMES if D.SHAPES[n][2] <= 256]


def _dev(cs):
    return dict(feats=[f.to(DEV) for f in cs.feats], ref=cs.ref.to(DEV), l2i=cs.lidar2img.to(DEV), logits=cs.logits.to(DEV),
                logits_v2=cs.logits_v2.to(DEV), offsets=cs.offsets.to(DEV), grad_out=cs.grad_out.to(DEV))


def _cpu(x):
    if isinstance(x, (list, tuple)):
        return [_cpu(e) for e in x]
    return None if x is None else x.cpu()


def v1_fwd(d, **want):
    return {k: _cpu(v) for k, v in ops.detr3d_fwd(d['feats'], d['ref'], d['logits'], d['l2i'], *GEOM, **want).items()}


def v1_bwd(d, **want):
    gf, gl, gr = ops.detr3d_bwd(d['feats'], d['ref'], d['logits'], d['l2i'], *GEOM, d['grad_out'], **want)
    return dict(grad_feats=_cpu(gf), grad_logits=_cpu(gl), grad_ref=_cpu(gr))


def v2_fwd(d, cs, want_mask=True):
    r = ops.detr3d_v2_fwd(d['feats'], d['ref'], d['logits_v2'], d['offsets'], d['l2i'], *GEOM, cs.Hh, want_mask=want_mask)
    return dict(out=_cpu(r[0]), mask=_cpu(r[1])) if want_mask else dict(out=_cpu(r))


def v2_bwd(d, cs, **want):
    gf, gl, go, gr = ops.detr3d_v2_bwd(d['feats'], d['ref'], d['logits_v2'], d['offsets'], d['l2i'], *GEOM, cs.Hh, d['grad_out'], **want)
    return dict(grad_feats=_cpu(gf), grad_logits=_cpu(gl), grad_offsets=_cpu(go), grad_ref=_cpu(gr))


def _hold(label, kernel, host):
    """Print the kernel's error next to the fp32 host error and the bound, then assert every bound."""
    late = []
    for key, err in kernel.items():
        bound = D.FACTOR * host[key]
        print(f'{label:>10} {key:<16} kernel {err:.2e}   fp32 host {host[key]:.2e}   bound {bound:.2e}')
        if not err <= bound:
            late.append(f'{key}: {err:.2e} > {bound:.2e}')
    assert not late, f'{label}: ' + '; '.join(late)


def _same_bits(a, b, keys):
    for key in keys:
        assert torch.equal(a[key], b[key]), f'{key} differs between two calls'


@pytest.mark.parametrize('name', NAMES)
def test_v1_forward(name):
    cs = D.case(name)
    D.check_case(cs)
    want, host = D.reference(name, 'v1')
    d = _dev(cs)
    got = v1_fwd(d, want_out=True, want_mask=True, want_sampled=True)
    assert torch.equal(got['mask'].bool(), want['mask']), 'mask differs from the restatement'
    behind = [i for i, kind in enumerate(cs.kinds) if kind == 'behind']
    assert bool((want['sampled'][:, :, behind, 0] == 0).all()) and bool((got['sampled'][:, :, behind, 0] == 0).all())
    _hold(f'{name} v1', D.figures(cs, 'v1', got, want), host)
    _same_bits(got, v1_fwd(d, want_out=True, want_mask=True, want_sampled=True), ('out', 'mask', 'sampled'))
    only_mask = v1_fwd(d, want_out=False, want_mask=True)
    assert only_mask['out'] is None and only_mask['sampled'] is None and torch.equal(only_mask['mask'], got['mask'])
    only_sampled = v1_fwd(d, want_out=False, want_sampled=True)
    assert only_sampled['out'] is None and only_sampled['mask'] is None and torch.equal(only_sampled['sampled'], got['sampled'])
    only_out = v1_fwd(d)
    assert only_out['mask'] is None and only_out['sampled'] is None and torch.equal(only_out['out'], got['out'])


def _exact_zeros(cs, got, want):
    unseen = ~want['mask'].permute(0, 2, 1)                                       # (B, Q, N)
    assert bool(unseen.any()) and bool(unseen.all(2).any())
    assert bool((got['grad_logits'].reshape(cs.B, cs.Q, cs.N, -1)[unseen] == 0).all()), 'grad_logits of an invisible camera'
    if 'grad_offsets' in got:
        assert bool((got['grad_offsets'][unseen] == 0).all()), 'grad_offsets of an invisible camera'
    assert bool((got['grad_ref'][unseen.all(2)] == 0).all()), 'grad_ref of a query that no camera sees'


def _block_alone(name, variant, run):
    cs = D.case(name)
    sub = D.subset(cs, cs.block)
    want, host = D.reference(name, variant, block_only=True)
    got = run(_dev(sub), sub)
    assert len(D.block_pixels(cs)) >= 1
    _hold(f'{name} {variant}', {'block grad_feats': R.rel_err(D.block_grad(sub, got), D.block_grad(sub, want))}, host)


@pytest.mark.parametrize('name', NAMES)
def test_v1_backward(name):
    cs = D.case(name)
    D.check_case(cs)
    want, host = D.reference(name, 'v1')
    d = _dev(cs)
    got = v1_bwd(d)
    _exact_zeros(cs, got, want)
    _hold(f'{name} v1', D.figures(cs, 'v1', got, want), host)
    again = v1_bwd(d)
    _same_bits(got, again, ('grad_logits', 'grad_ref'))
    _hold(f'{name} v1 #2', D.figures(cs, 'v1', dict(grad_feats=again['grad_feats']), want), host)
    no_feats = v1_bwd(d, want_feats=False)
    assert no_feats['grad_feats'] is None
    _same_bits(got, no_feats, ('grad_logits', 'grad_ref'))
    no_ref = v1_bwd(d, want_ref=False)
    assert no_ref['grad_ref'] is None
    _same_bits(got, no_ref, ('grad_logits',))
    _hold(f'{name} v1 -ref', D.figures(cs, 'v1', dict(grad_feats=no_ref['grad_feats']), want), host)
    _block_alone(name, 'v1', lambda dd, sub: v1_bwd(dd))


@pytest.mark.parametrize('name', NAMES)
def test_v2_forward(name):
    """`wide` (C = 320) runs here although the backward refuses it (test_refusals_and_error_codes)."""
    cs = D.case(name)
    D.check_case(cs)
    want, host = D.reference(name, 'v2')
    d = _dev(cs)
    got = v2_fwd(d, cs)
    assert torch.equal(got['mask'].bool(), want['mask']), 'mask differs from the restatement'
    _hold(f'{name} v2', D.figures(cs, 'v2', got, want), host)
    _same_bits(got, v2_fwd(d, cs), ('out', 'mask'))
    _same_bits(got, v2_fwd(d, cs, want_mask=False), ('out',))


@pytest.mark.parametrize('name', V2_TRAINABLE)
def test_v2_backward(name):
    cs = D.case(name)
    D.check_case(cs)
    want, host = D.reference(name, 'v2')
    d = _dev(cs)
    got = v2_bwd(d, cs)
    _exact_zeros(cs, got, want)
    _hold(f'{name} v2', D.figures(cs, 'v2', got, want), host)
    again = v2_bwd(d, cs)
    _same_bits(got, again, ('grad_logits', 'grad_offsets', 'grad_ref'))
    _hold(f'{name} v2 #2', D.figures(cs, 'v2', dict(grad_feats=again['grad_feats']), want), host)
    no_feats = v2_bwd(d, cs, want_feats=False)
    assert no_feats['grad_feats'] is None
    _same_bits(got, no_feats, ('grad_logits', 'grad_offsets', 'grad_ref'))
    no_ref = v2_bwd(d, cs, want_ref=False)
    assert no_ref['grad_ref'] is None
    _same_bits(got, no_ref, ('grad_logits', 'grad_offsets'))
    _hold(f'{name} v2 -ref', D.figures(cs, 'v2', dict(grad_feats=no_ref['grad_feats']), want), host)
    _block_alone(name, 'v2', lambda dd, sub: v2_bwd(dd, sub))


def test_refusals_and_error_codes():
    """Every refusal below is a host-side check that returns before a launch; the first call of each entry point is a valid one (0)."""
    lib = _lib.load()
    invalid, unsupported = -1, -2                                               # GD4D_EINVAL, GD4D_EUNSUPPORTED
    b, n, q, c, hh, nl = 1, 2, 3, 8, 2, 2
    hw = [(2, 3), (1, 2)]
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())                               # noqa: E731
    z = lambda *shape: torch.zeros(*shape, device=DEV)                          # noqa: E731
    feats, gfeats = [z(b, n, c, h, w) for h, w in hw], [z(b, n, c, h, w) for h, w in hw]
    # tables of 9 entries: a level count of 9 must be refused before any of them is read, and reads nothing foreign if it is not
    table = lambda ts: (ctypes.c_void_p * 9)(*[ts[i % nl].data_ptr() for i in range(9)])    # noqa: E731
    level_hw = (ctypes.c_int32 * 18)(*[x for i in range(9) for x in hw[i % nl]])
    holed = table(feats)
    holed[1] = None
    rng = (ctypes.c_double * 6)(*D.PC_RANGE)
    ref, l2i = z(b, q, 3) + 0.5, torch.eye(4, device=DEV).expand(b, n, 4, 4).contiguous()
    lg1, lg2, off = z(b, q, n, 1, nl), z(b, q, n, hh, nl * nl), z(b, q, n, hh, nl, nl, 2)
    out, mask, sampled, gout = z(b, q, c), torch.zeros(b, n, q, dtype=torch.uint8, device=DEV), z(b, c, q, n, 1, nl), z(b, q, c)
    gl1, gl2, goff, gref = z(b, q, n, 1, nl), z(b, q, n, hh, nl * nl), z(b, q, n, hh, nl, nl, 2), z(b, q, 3)
    base = dict(feats=table(feats), level_hw=level_hw, ref=ptr(ref), lidar2img=ptr(l2i), pc_range=rng, out=ptr(out), mask=ptr(mask),
                sampled=ptr(sampled), grad_out=ptr(gout), grad_feats=table(gfeats), grad_ref=ptr(gref), offsets=ptr(off),
                grad_offsets=ptr(goff), N=n, C=c, L=nl, Hh=hh)

    def fwd(P=1, **kw):
        a = {**base, 'logits': ptr(lg1), **kw}
        return lib.gd4d_detr3d_fwd(a['feats'], a['level_hw'], a['ref'], a['logits'], a['lidar2img'], a['pc_range'], 64.0, 112.0, a['out'],
                                   a['mask'], a['sampled'], b, a['N'], q, a['C'], a['L'], P, None)

    def bwd(P=1, **kw):
        a = {**base, 'logits': ptr(lg1), 'grad_logits': ptr(gl1), **kw}
        return lib.gd4d_detr3d_bwd(a['feats'], a['level_hw'], a['ref'], a['logits'], a['lidar2img'], a['pc_range'], 64.0, 112.0,
                                   a['grad_out'], a['grad_feats'], a['grad_logits'], a['grad_ref'], b, a['N'], q, a['C'], a['L'], P, None)

    def fwd2(P=nl, **kw):
        a = {**base, 'logits': ptr(lg2), **kw}
        return lib.gd4d_detr3d_v2_fwd(a['feats'], a['level_hw'], a['ref'], a['logits'], a['offsets'], a['lidar2img'], a['pc_range'], 64.0,
                                      112.0, a['out'], a['mask'], b, a['N'], q, a['C'], a['Hh'], a['L'], P, None)

    def bwd2(**kw):
        a = {**base, 'logits': ptr(lg2), 'grad_logits': ptr(gl2), **kw}
        return lib.gd4d_detr3d_v2_bwd(a['feats'], a['level_hw'], a['ref'], a['logits'], a['offsets'], a['lidar2img'], a['pc_range'], 64.0,
                                      112.0, a['grad_out'], a['grad_feats'], a['grad_logits'], a['grad_offsets'], a['grad_ref'], b, a['N'],
                                      q, a['C'], a['L'], a['Hh'], None)

    required = {fwd: ('feats', 'level_hw', 'ref', 'logits', 'lidar2img', 'pc_range'),
                bwd: ('feats', 'level_hw', 'ref', 'logits', 'lidar2img', 'pc_range', 'grad_out', 'grad_logits'),
                fwd2: ('feats', 'level_hw', 'ref', 'logits', 'offsets', 'lidar2img', 'pc_range', 'out'),
                bwd2: ('feats', 'level_hw', 'ref', 'logits', 'offsets', 'lidar2img', 'pc_range', 'grad_out', 'grad_logits', 'grad_offsets')}
    for call, names in required.items():
        assert call() == 0
        for name in names:
            assert call(**{name: None}) == invalid, f'{call.__name__}: a null {name}'
        assert call(feats=holed) == invalid, f'{call.__name__}: a null level'
        assert call(L=9) == unsupported, f'{call.__name__}: L above GD4D_MAX_LEVELS'
        assert call(N=257) == unsupported, f'{call.__name__}: 257 cameras'
    assert fwd(out=None, mask=None, sampled=None) == invalid                    # nothing asked for
    assert fwd(out=None, sampled=None) == 0 and bwd(grad_feats=None, grad_ref=None) == 0 and bwd2(grad_feats=None, grad_ref=None) == 0
    assert fwd(P=2) == unsupported and bwd(P=2) == unsupported
    assert fwd2(P=nl + 1) == unsupported and fwd2(P=1) == unsupported
    assert fwd2(Hh=3) == unsupported and bwd2(Hh=3) == invalid                  # 8 channels over 3 heads: refused by both
    assert bwd2(C=320, Hh=8) == unsupported                                     # no launch: the small buffers are never touched
    torch.cuda.synchronize()


def test_v2_module_refuses_to_train_wider_than_256(monkeypatch):
    import graph_detr4d_amd as G
    monkeypatch.delenv('GD4D_TORCH_OPS', raising=False)
    n, q = 2, 5
    mod = G.build_attention(dict(type='Detr3DCrossAttenV2', num_cams=n, pc_range=D.PC_RANGE, num_levels=2, num_points=2,
                                 embed_dims=320)).to(DEV).train()
    feats = [torch.zeros(1, n, 320, 4, 7, device=DEV), torch.zeros(1, n, 320, 2, 4, device=DEV)]
    metas = [dict(lidar2img=[torch.eye(4).numpy()] * n, img_shape=[(D.IMG_H, D.IMG_W, 3)] * n)]
    query = torch.zeros(q, 1, 320, device=DEV, requires_grad=True)
    with pytest.raises(_lib.Gd4dError, match='embed_dims = 320'):
        mod(query, None, feats, reference_points=torch.rand(1, q, 3, device=DEV), img_metas=metas)
