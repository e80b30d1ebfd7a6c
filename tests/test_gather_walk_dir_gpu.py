"""gd4d_cross_attn_agg_items_coarse_fwd walked forward and reversed (ops.cross_attn_agg_coarse_fwd(reverse=)): agg, wsum and pagg bit for
bit, on the inputs of tests/test_gather_slice_group_gpu.py - 12 cameras, levels 5x7, 3x4, 2x3, 1x2, plans with an empty head, an odd
count, a multi-step head and a last partial pass - over the slice-planar copy, channels-last levels in place and bf16 values, for every
slice-group size; and a 2-layer decoder: alternation by layer on and off, a captured graph's replay, and the request program
(GD4D_REQUEST=1).  Every comparison is exact.  GPU only."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'


def _gather(plan, coarse, q, reverse):
    from graph_detr4d_amd import ops
    agg = torch.full((1, q, 8, 256), float('nan'), device=DEV)
    pagg = torch.full((1, q, 256), float('nan'), device=DEV)
    plan.wsum.fill_(float('nan'))                                   # the gather writes every row of all three
    ops.cross_attn_agg_coarse_fwd(plan, coarse, agg=agg, pagg=pagg, reverse=reverse)
    torch.cuda.synchronize()
    return agg, plan.wsum.clone(), pagg


@pytest.mark.parametrize('q', [1, 9, 37])
@pytest.mark.parametrize('layout', ['planar', 'channels_last', 'bf16'])
def test_reversed_walk_sums_the_same_bits(layout, q):
    import test_gather_slice_group_gpu as base
    from graph_detr4d_amd import ops, synthetic
    c = base._case(q)
    pyr = base._pyramid(layout, c['feats'])
    order = ops.query_order_fwd(c['ref'], synthetic.PC_RANGE)
    plan = ops.cross_attn_plan_fwd(pyr, c['ref'], c['offsets'], c['attn'], c['cam'], c['l2i'], synthetic.PC_RANGE, 900, 1600, base.HEADS,
                                   query_order=order, items=True)
    was = ops.gather_slice_group()
    try:
        for ns in (was, 1, 4, 8):
            ops.gather_slice_group(ns)
            want = _gather(plan, c['coarse'], q, False)
            assert all(bool(torch.isfinite(t).all()) for t in want)
            assert bool((want[0].abs().amax(-1) > 0).any())
            got = _gather(plan, c['coarse'], q, True)
            for name, a, b in zip(('agg', 'wsum', 'pagg'), got, want):
                assert torch.equal(a, b), (name, ns, layout, q)
    finally:
        ops.gather_slice_group(was)


def test_two_layer_decoder_alternating_replayed_and_as_a_request_program(monkeypatch):
    """A 2-layer decoder at 64 queries, 6 cameras, a small pyramid: layer 1 walks reversed under the default and forward with the switch
    off, every returned tensor equal; a graph captured under the default replays to the eager result; the request program too."""
    import bench
    import graph_detr4d_amd as G
    from graph_detr4d_amd import fused_decoder, ops, synthetic
    tr, regs = bench.build_decoder(G, 6, 2, 'fp32', 77)
    tr, regs = tr.to(DEV).eval(), regs.to(DEV).eval()
    feats = [f.to(DEV) for f in synthetic.feature_pyramid(6, [(29, 50), (15, 25), (8, 13), (4, 7)], seed=5)]
    qe = torch.randn(64, 512, generator=torch.Generator().manual_seed(9)).to(DEV)
    metas = synthetic.make_img_metas(synthetic.camera_rig(1), batch=1)
    directions = []
    orig = ops.cross_attn_agg_coarse_fwd

    def spy(plan, coarse, agg=None, pagg=None, reverse=False):
        directions.append(bool(reverse))
        return orig(plan, coarse, agg=agg, pagg=pagg, reverse=reverse)
    monkeypatch.setattr(ops, 'cross_attn_agg_coarse_fwd', spy)
    monkeypatch.setenv('GD4D_REQUEST', '0')

    def run():
        with torch.no_grad():
            out = [t.clone() for t in tr(feats, qe, reg_branches=regs, img_metas=metas)]
        torch.cuda.synchronize()
        return out
    was = ops.gather_walk_alternate()
    try:
        ops.gather_walk_alternate(False)
        plain = run()
        assert directions == [False, False]                         # the gather under test is the step's gather, once per layer
        ops.gather_walk_alternate(True)
        del directions[:]
        alternating = run()
        assert directions == [False, True]
        assert len(plain) == 3 and all(bool(torch.isfinite(t).all()) for t in plain)
        for a, b in zip(alternating, plain):
            assert torch.equal(a, b)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode='thread_local'):
            with torch.no_grad():
                captured = tr(feats, qe, reg_branches=regs, img_metas=metas)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(captured, plain):
            assert torch.equal(a, b)
        entered = []
        orig_run = fused_decoder.RequestProgram.run
        monkeypatch.setattr(fused_decoder.RequestProgram, 'run', lambda self, *a: (entered.append(1), orig_run(self, *a))[1])
        monkeypatch.setenv('GD4D_REQUEST', '1')
        del directions[:]
        first = run()                                               # records the program (the recorder stands in for the library), runs it
        again = run()                                               # the kept program alone
        assert entered == [1, 1], 'the call did not take the request program'
        assert directions == [False, True]                          # recorded once, with layer 1 reversed
        for a, b, w in zip(first, again, plain):
            assert torch.equal(a, w) and torch.equal(b, w)
    finally:
        ops.gather_walk_alternate(was)
