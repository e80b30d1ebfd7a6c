"""The query front end of the cross-attention kernels (csrc/gd4d_cross_attn_shared.h): every kernel that projects a query's
sampling points takes visibility, image coordinates, item lists and corner weights from one set of helpers, so

  * mask and uv of gd4d_cross_attn_fwd, gd4d_cross_attn_agg_fwd and gd4d_cross_attn_plan_fwd (pairs and items form) are the
    same bytes, and on rows built by hand ON the decision boundaries (u = 0, u = 1, v = 0, v = 1, depth = eps and the next float
    above it, a sample half a pixel outside either edge of a level) they are what plain fp32 arithmetic on the CPU says;
  * the plan's item counts are the mask's sums, and the plan's backward counts the same items (its status word stays 0);
  * wsum of the pairs plan and of the items gather are the same bits;
  * the two backward routes (gd4d_cross_attn_bwd on projected values, plan + gather-dot + gd4d_cross_attn_plan_bwd on the raw
    pyramid) agree on grad_ref and grad_offsets to the tolerance of test_raw_backward_matches_projected_backward.

Shapes are the smallest that reach every path: levels (6, 10), (3, 5), (2, 3), (1, 2) (on the one-row level no corner has a
row below), fewer candidates than a wave (6 cameras), more than a wave (17 cameras: the compaction loop runs twice and the
projection loop more than once per wave), a query count that is no multiple of 8 with a locality order, two samples, and
4 heads x 1 level (16 logits: the plan's one-thread softmax next to gd4d_cross_attn_fwd's shuffles).  GPU only."""
import numpy as np
import pytest
import torch

from graph_detr4d_amd import ops, synthetic

pytestmark = pytest.mark.gpu
DEV = 'cuda'
PC_RANGE = synthetic.PC_RANGE
IMG_H, IMG_W = 900, 1600
LEVELS = [(6, 10), (3, 5), (2, 3), (1, 2)]
EPS = np.float32(1e-5)
EPS_UP = np.nextafter(EPS, np.float32(1))

# Points in the frame of a camera whose lidar2img is the identity (cx = X, cy = Y, cz = Z), and whether they are visible:
# strict compares, so a point ON the image border or AT the depth threshold is not.  All of them are exact in fp32, and so is
# every step of their projection (1600 / 1600, 450 / 900, 25 / 16 / 1600 = 2^-10 ...).
BOUNDARY_POINTS = [
    ((0.0, 450.0, 1.0), False),             # u == 0: u * W - 0.5 is exactly -0.5 on every level
    ((1600.0, 450.0, 1.0), False),          # u == 1: u * W - 0.5 is exactly W - 0.5
    ((800.0, 0.0, 1.0), False),             # v == 0
    ((800.0, 900.0, 1.0), False),           # v == 1
    ((800.0, 450.0, 1.0), True),            # the image centre
    ((1.5625, 450.0, 1.0), True),           # u = 2^-10: column -1 | 0 on every level (x0 off the map)
    ((1598.4375, 450.0, 1.0), True),        # u = 1 - 2^-10: column W - 1 | W (x0 + 1 off the map)
    ((800.0, 0.87890625, 1.0), True),       # v = 2^-10: row -1 | 0
    ((800.0, 899.12109375, 1.0), True),     # v = 1 - 2^-10: row H - 1 | H
    ((400.0, 225.0, 1.0), True),            # u = v = 0.25: on the (1, 2) level x = 0 exactly (dx = 0)
    ((512.0 * float(EPS), 256.0 * float(EPS), float(EPS)), False),             # depth == eps: `>` fails
    ((512.0 * float(EPS_UP), 256.0 * float(EPS_UP), float(EPS_UP)), True),     # the next float above eps
    ((800.0, 450.0, -1.0), False),          # behind the camera
    ((3200.0, 900.0, 2.0), False),          # u == 1 at depth 2
]
# ref at which ref * (hi - lo) + lo is exactly (0, 0, 0) for PC_RANGE (51.2 + -51.2, 0.625 * 8 - 5): the point IS its offset
REF_ORIGIN = (0.5, 0.5, 0.625)


def _case(heads, levels, b, n, q, seed, boundary=True):
    gen = torch.Generator().manual_seed(seed)
    hw = LEVELS[:levels]
    feats = [torch.randn(b, n, 256, h, w, generator=gen) for h, w in hw]
    l2i = torch.from_numpy(synthetic.camera_rig((n + 5) // 6)[:n]).unsqueeze(0).repeat(b, 1, 1, 1).contiguous()
    ref = torch.rand(b, q, 3, generator=gen)
    offsets = torch.randn(b, q, heads, 4, 3, generator=gen) * 2.0
    if boundary:                                                   # camera 0 of sample 0 looks along +z with unit intrinsics;
        l2i[0, 0] = torch.eye(4)                                   # query 0 carries the boundary points, one per (head, point)
        assert q >= 2 and heads * 4 >= len(BOUNDARY_POINTS)
        pts = torch.tensor([p for p, _ in BOUNDARY_POINTS], dtype=torch.float32)
        for qq, shift in ((0, 0), (1, 5)):                         # ... and query 1 the same ones in other (head, point) slots
            ref[0, qq] = torch.tensor(REF_ORIGIN)
            flat = offsets[0, qq].view(-1, 3)
            flat[(torch.arange(len(pts)) + shift) % flat.shape[0]] = pts
    attn = torch.randn(b, q, heads, levels, 4, generator=gen)
    cam = torch.randn(b, q, n, generator=gen)
    w_v = torch.randn(256, 256, generator=gen) / 16
    b_v = torch.randn(256, generator=gen)
    gout = torch.randn(b, q, 256, generator=gen)
    to = lambda t: t.to(DEV)                                                                             # noqa: E731
    return dict(hw=hw, feats=[to(f) for f in feats], l2i=to(l2i), ref=to(ref), offsets=to(offsets), attn=to(attn), cam=to(cam),
                w_v=to(w_v), b_v=to(b_v), gout=to(gout), heads=heads, b=b, n=n, q=q, boundary=boundary)


def _cpu_projection(c):
    """mask (B, N, Q, Hh, P) and uv (B, N, Q, Hh, P, 2) in plain numpy fp32, one rounding per operation, in the reference's order:
    p = ref * scale + lo (two roundings), X = p + offset, c = ((m0 X + m1 Y) + m2 Z) + m3, u = (cx / max(cz, eps)) / W."""
    f = np.float32
    ref, off, l2i = c['ref'].cpu().numpy(), c['offsets'].cpu().numpy(), c['l2i'].cpu().numpy()
    scale = [f(PC_RANGE[k + 3] - PC_RANGE[k]) for k in range(3)]
    lo = [f(PC_RANGE[k]) for k in range(3)]
    X, Y, Z = [((ref[:, None, :, None, None, k] * scale[k]) + lo[k]) + off[:, None, :, :, :, k] for k in range(3)]   # (B, 1, Q, Hh, P)
    m = l2i[:, :, None, None, None]                                                                     # (B, N, 1, 1, 1, 4, 4)
    cx, cy, cz = [((m[..., r, 0] * X + m[..., r, 1] * Y) + m[..., r, 2] * Z) + m[..., r, 3] for r in range(3)]
    assert cx.dtype == np.float32
    zc = np.maximum(cz, EPS)
    u, v = (cx / zc) / f(IMG_W), (cy / zc) / f(IMG_H)
    mask = (cz > EPS) & (u > 0) & (u < 1) & (v > 0) & (v < 1)
    return mask, np.stack([u, v], -1)


def _same_bytes(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _front_ends(c, order):
    """mask / uv of every forward kernel that projects, and the two plans (pairs, items) with their gathers' results."""
    b, n, hh = c['b'], c['n'], c['heads']
    args = (c['ref'], c['offsets'], c['attn'], c['cam'], c['l2i'], PC_RANGE, IMG_H, IMG_W)
    flat = torch.cat([f.flatten(3).permute(0, 1, 3, 2) for f in c['feats']], 2).reshape(b * n, -1, 256)          # (R, S, 256)
    val = (flat @ c['w_v'].t() + c['b_v']).view(b * n, -1, hh, 256 // hh).contiguous()
    got = {}
    _, got['fwd_mask'], got['fwd_uv'] = ops.cross_attn_fwd(val, c['hw'], *args, want_mask=True, want_uv=True, query_order=order)
    if b == 1:                                                                 # the one-workgroup-per-query aggregate refuses B > 1
        _, _, got['agg_mask'], got['agg_uv'] = ops.cross_attn_agg_fwd(flat.contiguous(), c['hw'], *args, hh, want_mask=True, want_uv=True,
                                                                      query_order=order)
    sp, hw = ops.pyramid_slice_planar_fwd(c['feats'])
    pyr = ops.PyramidView.slice_planar(sp, hw)
    pairs, got['pairs_mask'], got['pairs_uv'] = ops.cross_attn_plan_fwd(pyr, *args, hh, want_mask=True, want_uv=True, query_order=order)
    items, got['items_mask'], got['items_uv'] = ops.cross_attn_plan_fwd(pyr, *args, hh, want_mask=True, want_uv=True, query_order=order,
                                                                        items=True)
    items.wsum.fill_(float('nan'))                                             # the items gather must write every row
    agg_items = ops.cross_attn_agg_sliced_fwd(items)
    agg_pairs = ops.cross_attn_agg_sliced_fwd(pairs)
    return got, pairs, items, agg_pairs, agg_items, val


def _hdr_by_query(plan, order):
    """(B*Q, Hh) item counts of a plan; the header is stored by position of the locality order, kPlanHdr = 16 ints each."""
    bq, hh = plan.b * plan.q, plan.num_heads
    hdr = plan.buf[:bq * 16 * 4].view(torch.int32).view(bq, 16)[:, :hh]
    if order is None:
        return hdr
    out = torch.empty_like(hdr)
    out[order.long()] = hdr
    return out


CASES = [(8, 4, 1, 6, 17, True), (8, 4, 1, 17, 9, False), (8, 4, 2, 3, 5, False), (4, 1, 1, 6, 17, False)]
_RESULTS = {}


def _run(case):
    """One case's kernels, run once and shared by the tests below (nothing below modifies what it returns)."""
    if case not in _RESULTS:
        heads, levels, b, n, q, ordered = case
        c = _case(heads, levels, b, n, q, seed=200 + heads + levels + b + n + q)
        order = ops.query_order_fwd(c['ref'], PC_RANGE) if ordered else None
        _RESULTS[case] = (c, order) + _front_ends(c, order)
    return _RESULTS[case]


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'Hh%d-L%d-B%d-N%d-Q%d%s' % (c[:5] + ('-ordered' if c[5] else '',)))
def test_every_forward_kernel_writes_the_same_mask_and_uv(case):
    c, order, got, pairs, items, agg_pairs, agg_items, _ = _run(case)
    names = [k[:-5] for k in got if k.endswith('_mask')]
    assert len(names) == (4 if c['b'] == 1 else 3)
    for name in names[1:]:
        assert _same_bytes(got[name + '_mask'], got[names[0] + '_mask']), f'mask of {name} differs from {names[0]}'
        assert _same_bytes(got[name + '_uv'], got[names[0] + '_uv']), f'uv of {name} differs from {names[0]}'
    want_mask, want_uv = _cpu_projection(c)
    mask = got['fwd_mask'].cpu().numpy().astype(bool)
    assert np.array_equal(mask, want_mask), 'mask differs from fp32 arithmetic on the CPU'
    assert np.array_equal(got['fwd_uv'].cpu().numpy().view(np.uint32), want_uv.view(np.uint32)), 'uv differs from fp32 arithmetic on the CPU'
    # the rows built by hand: what the rule says, written down (camera 0 is the identity)
    flat = mask[0, 0].reshape(c['q'], -1)
    for qq, shift in ((0, 0), (1, 5)):
        for i, (point, visible) in enumerate(BOUNDARY_POINTS):
            assert flat[qq, (i + shift) % flat.shape[1]] == visible, (qq, point)
    assert mask.any() and not mask.all()


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'Hh%d-L%d-B%d-N%d-Q%d%s' % (c[:5] + ('-ordered' if c[5] else '',)))
def test_plan_counts_are_the_masks_sums_and_wsum_is_one_set_of_bits(case):
    c, order, got, pairs, items, agg_pairs, agg_items, _ = _run(case)
    b, n, q, hh = c['b'], c['n'], c['q'], c['heads']
    want = got['pairs_mask'].to(torch.int32).sum(dim=(1, 4)).view(b * q, hh)           # (B, N, Q, Hh, P) -> per (query, head)
    assert torch.equal(_hdr_by_query(pairs, order), want)
    assert torch.equal(_hdr_by_query(items, order), want)
    assert int(want.max()) > 0
    assert not torch.isnan(items.wsum).any()
    assert _same_bytes(items.wsum, pairs.wsum), 'wsum of the items gather differs from the pairs plan\'s'
    assert _same_bytes(agg_items, agg_pairs), 'items gather and pairs gather disagree'


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'Hh%d-L%d-B%d-N%d-Q%d%s' % (c[:5] + ('-ordered' if c[5] else '',)))
def test_plan_backward_counts_the_plans_items_and_agrees_with_the_projected_backward(case):
    c, order, got, pairs, items, agg_pairs, agg_items, val = _run(case)
    hh = c['heads']
    args = (c['ref'], c['offsets'], c['attn'], c['cam'], c['l2i'], PC_RANGE, IMG_H, IMG_W)
    status = torch.zeros(1, device=DEV, dtype=torch.int32)
    gagg, beta = ops.value_proj_heads_bwd(c['gout'], c['w_v'], c['b_v'], hh)
    dpart = ops.cross_attn_dot_sliced(pairs, gagg)
    gr, go, ga, gc = ops.cross_attn_plan_bwd(pairs, dpart, beta, *args, status=status)
    assert int(status.item()) == 0, 'an item count of the backward disagrees with the plan'
    assert all(bool(torch.isfinite(t).all()) for t in (gr, go, ga, gc))
    if c['b'] == 1:                                                # both routes apply (4 points per head everywhere here)
        _, gr_p, go_p, _, _ = ops.cross_attn_bwd(val, c['hw'], *args, c['gout'], query_order=order)
        rel = lambda a, e: ((a.double() - e.double()).abs().max() / e.double().abs().max().clamp(min=1e-12)).item()   # noqa: E731
        # the tolerance of tests/test_cross_attn_sliced_bwd_gpu.py::test_raw_backward_matches_projected_backward, on all queries and
        # on the random ones alone (the point at depth eps + 1 ulp has a gradient of 1e10 that would hide every other row)
        for rows in (slice(None), slice(2, None)):
            e_r, e_o = rel(gr[:, rows], gr_p[:, rows]), rel(go[:, rows], go_p[:, rows])
            print(f'rows {rows}: grad_ref {e_r:.2e} grad_offsets {e_o:.2e}')
            assert e_r < 2e-4 and e_o < 2e-4
