"""gd4d_cross_attn_agg_items_coarse_fwd with NS = 2, 4, 8 slices per fine workgroup (ops.gather_slice_group) against NS = 1: agg,
wsum and pagg bit for bit - on the slice-planar copy, on channels-last levels read in place and on bf16 values - over plans that
hold an empty head, an odd count, a multi-step head (more than 32 items) and a last partial pass; and a 2-layer decoder, eager and
replayed from a captured graph.  Every comparison is exact.  GPU only."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
LEVELS = [(5, 7), (3, 4), (2, 3), (1, 2)]
CAMS, HEADS, POINTS = 12, 8, 4
FAR = 1.0e4                                   # metres: an offset that takes a point out of every image


def make_inputs(q):
    """12 cameras: eleven copies of the rig's camera 0 and its camera 3 (which looks the other way), so that a point camera 0 sees is
    seen eleven times.  Query 0 sits in the middle of camera 0's image with small offsets, except: head 0's four points are
    nowhere (no item), one point of head 1 is nowhere (3 x 11 = 33 items: odd, a second step, a last pass of one item); its other
    heads have 44 items (a second step, a last pass of four).  The other queries are random."""
    from graph_detr4d_amd import synthetic
    from oracle import torch_oracle as O
    g = torch.Generator().manual_seed(100 + q)
    rig = torch.from_numpy(synthetic.camera_rig(1))
    l2i = torch.stack([rig[0]] * (CAMS - 1) + [rig[3]]).unsqueeze(0).contiguous()
    # a reference point camera 0 sees near the middle of its image (and camera 3 does not): searched on a grid, on the host
    axis = torch.linspace(0.05, 0.95, 19)
    grid = torch.stack(torch.meshgrid(axis, axis, torch.tensor([0.5]), indexing='ij'), -1).reshape(1, -1, 3)
    uv, seen = O.project(O.denormalise(grid, synthetic.PC_RANGE), l2i, 900, 1600)
    centred = seen[0, 0] & ~seen[0, CAMS - 1] & ((uv[0, 0] - 0.5).abs().amax(-1) < 0.2)
    assert bool(centred.any())
    score = (uv[0, 0] - 0.5).abs().amax(-1).masked_fill(~centred, 9.)
    ref = torch.rand(1, q, 3, generator=g)
    ref[0, 0] = grid[0, int(score.argmin())]
    offsets = torch.randn(1, q, HEADS, POINTS, 3, generator=g) * 2.0
    offsets[0, 0] = torch.randn(HEADS, POINTS, 3, generator=g) * 0.2
    offsets[0, 0, 0] = FAR
    offsets[0, 0, 1, 2] = FAR
    attn = torch.randn(1, q, HEADS, len(LEVELS), POINTS, generator=g)
    cam = torch.randn(1, q, CAMS, generator=g)
    feats = [torch.randn(1, CAMS, 256, h, w, generator=g) for h, w in LEVELS]
    w_v, b_v = torch.randn(256, 256, generator=g) * 0.06, torch.randn(256, generator=g)
    return dict(l2i=l2i, ref=ref, offsets=offsets, attn=attn, cam=cam, feats=feats, w_v=w_v, b_v=b_v)


_CASES = {}


def _case(q):
    """The inputs of a query count on the device and the projected coarse levels: made once, shared by the layouts, left unchanged."""
    from graph_detr4d_amd import ops
    if q not in _CASES:
        c = {k: ([t.to(DEV) for t in v] if isinstance(v, list) else v.to(DEV)) for k, v in make_inputs(q).items()}
        coarse_levels = [f.contiguous() for f in c['feats'][2:]]
        c['coarse'] = ops.CoarseValues(ops.value_proj_fwd(coarse_levels, c['w_v'], c['b_v']), [tuple(f.shape[-2:]) for f in coarse_levels])
        _CASES[q] = c
    return _CASES[q]


def _pyramid(layout, feats):
    from graph_detr4d_amd import ops
    if layout == 'planar':
        sp, shp = ops.pyramid_slice_planar_fwd(feats)
        return ops.PyramidView.slice_planar(sp, shp)
    if layout == 'bf16':
        sp, shp = ops.pyramid_slice_planar_fwd(feats, out_dtype=torch.bfloat16)
        return ops.PyramidView.slice_planar(sp, shp)
    nhwc = [f.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3) for f in feats]
    return ops.PyramidView.channels_last_levels(nhwc)


def _gather(plan, coarse, q):
    from graph_detr4d_amd import ops
    agg = torch.full((1, q, HEADS, 256), float('nan'), device=DEV)
    pagg = torch.full((1, q, 256), float('nan'), device=DEV)
    plan.wsum.fill_(float('nan'))                                   # the gather writes every row of all three
    ops.cross_attn_agg_coarse_fwd(plan, coarse, agg=agg, pagg=pagg)
    torch.cuda.synchronize()
    return agg, plan.wsum.clone(), pagg


@pytest.mark.parametrize('q', [1, 9, 37])
@pytest.mark.parametrize('layout', ['planar', 'channels_last', 'bf16'])
def test_slice_groups_equal_one_slice_per_workgroup(layout, q):
    from graph_detr4d_amd import ops, synthetic
    c = _case(q)
    pyr = _pyramid(layout, c['feats'])
    order = ops.query_order_fwd(c['ref'], synthetic.PC_RANGE)
    plan = ops.cross_attn_plan_fwd(pyr, c['ref'], c['offsets'], c['attn'], c['cam'], c['l2i'], synthetic.PC_RANGE, 900, 1600, HEADS,
                                   query_order=order, items=True)
    # the plan's own counts: its header holds 16 ints per position, the first 8 the heads' item counts
    counts = plan.buf[:q * 64].view(torch.int32).view(q, 16)[:, :HEADS].cpu()
    assert bool((counts == 0).any()), 'a head with no visible item'
    assert bool((counts % 2 == 1).any()), 'a head with an odd count'
    assert bool((counts > 32).any()), 'a head with more than 32 items: a second step'
    assert bool(((counts > 0) & (counts % 8 != 0)).any()), 'a last partial pass (a pass is 8 items x 2 levels)'
    assert int(counts.max()) <= CAMS * POINTS
    was = ops.gather_slice_group()
    try:
        ops.gather_slice_group(1)
        want = _gather(plan, c['coarse'], q)
        assert all(bool(torch.isfinite(t).all()) for t in want)
        assert bool((want[1] == 0).any()) and bool((want[0].abs().amax(-1) > 0).any())
        for ns in (2, 4, 8):
            ops.gather_slice_group(ns)
            got = _gather(plan, c['coarse'], q)
            for name, a, b in zip(('agg', 'wsum', 'pagg'), got, want):
                assert torch.equal(a, b), (name, ns, layout, q)
    finally:
        ops.gather_slice_group(was)


def test_two_layer_decoder_equal_for_every_group_size_and_replayed(monkeypatch):
    """A 2-layer decoder at 64 queries, 6 cameras, a small pyramid: every returned tensor equal for NS = 1, the default and the other
    values; a graph captured under the default replays to the eager result - and keeps doing so after the setting has changed."""
    import bench
    import graph_detr4d_amd as G
    from graph_detr4d_amd import ops, synthetic
    tr, regs = bench.build_decoder(G, 6, 2, 'fp32', 77)
    tr, regs = tr.to(DEV).eval(), regs.to(DEV).eval()
    feats = [f.to(DEV) for f in synthetic.feature_pyramid(6, [(29, 50), (15, 25), (8, 13), (4, 7)], seed=5)]
    qe = torch.randn(64, 512, generator=torch.Generator().manual_seed(9)).to(DEV)
    metas = synthetic.make_img_metas(synthetic.camera_rig(1), batch=1)
    seen = []
    orig = ops._call

    def spy(entry, *args):
        seen.append(entry)
        return orig(entry, *args)
    monkeypatch.setattr(ops, '_call', spy)

    def run():
        with torch.no_grad():
            return tr(feats, qe, reg_branches=regs, img_metas=metas)
    default = ops.gather_slice_group()
    try:
        outs = {}
        for ns in (1, default, 2, 4, 8):
            ops.gather_slice_group(ns)
            outs[ns] = [t.clone() for t in run()]
            torch.cuda.synchronize()
        assert seen.count('gd4d_cross_attn_agg_items_coarse_fwd') >= 2 * 5          # the gather under test is the step's gather
        assert len(outs[1]) == 3 and all(bool(torch.isfinite(t).all()) for t in outs[1])
        for ns, out in outs.items():
            for a, b in zip(out, outs[1]):
                assert torch.equal(a, b), ns
        ops.gather_slice_group(default)
        run()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode='thread_local'):
            captured = run()
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(captured, outs[default]):
            assert torch.equal(a, b)
        ops.gather_slice_group(8 if default != 8 else 1)                            # read at launch: the captured graph keeps its kernels
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(captured, outs[default]):
            assert torch.equal(a, b)
    finally:
        ops.gather_slice_group(default)
