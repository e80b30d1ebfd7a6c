#!/usr/bin/env python
"""Times the matching of Detr4D_Distiller's instance term: 6 layers x B problems of 900 x 900 (B = 1, 2), two seeded families
('independent': student and teacher boxes unrelated; 'noise': student = teacher + noise, query order permuted), four routes:

  host      the cost blocks to the host, gd4d_linear_sum_assignment_batch (8 threads), the matches back;
  sap       gd4d_hungarian_assign_fwd (one workgroup per problem, scipy's loop from zero duals);
  dense     gd4d_lsa_dense_fwd (warm start + shortest augmenting paths);
  term      the whole term - cost, dense assignment, loss forward + backward - replayed as ONE captured graph.

Device events around >= --reps replays after --warmup.  Prints one JSON line per (B, family).

    python tools/bench_distill_match.py [--reps 20] [--warmup 2] [--out results/distill_match.json]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from graph_detr4d_amd import distill, get_instance_distill_loss, ops  # noqa: E402

CFG = dict(loss_cls_distill=dict(type='DistillCrossEntropyLoss', use_sigmoid=True, loss_weight=1.0),
           loss_reg_distill=dict(type='L1Loss', loss_weight=0.25), reweight_score=False)


def inputs(family, b, seed, nl=6, q=900, dev='cuda'):
    """head outputs whose distillation cost is the family's: box codes drawn so that the first 8 entries carry the geometry"""
    g = torch.Generator(device=dev).manual_seed(seed)
    t_cls = torch.randn(nl, b, q, 10, device=dev, generator=g) * 2 - 1
    t_box = torch.randn(nl, b, q, 10, device=dev, generator=g) * 0.5
    if family == 'independent':
        s_cls = torch.randn(nl, b, q, 10, device=dev, generator=g) * 2 - 1
        s_box = torch.randn(nl, b, q, 10, device=dev, generator=g) * 0.5
    else:
        perm = torch.argsort(torch.rand(nl, b, q, device=dev, generator=g), dim=-1)
        idx = perm[..., None].expand(-1, -1, -1, 10)
        s_cls = torch.gather(t_cls, 2, idx) + 0.05 * torch.randn(nl, b, q, 10, device=dev, generator=g)
        s_box = torch.gather(t_box, 2, idx) + 0.05 * torch.randn(nl, b, q, 10, device=dev, generator=g)
    return t_cls, t_box, s_cls, s_box


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return {'ms_events': e0.elapsed_time(e1) / reps, 'ms_wall': (time.perf_counter() - t0) * 1e3 / reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--batches', default='1,2')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    rows = []
    for b in [int(x) for x in a.batches.split(',')]:
        for family in ('independent', 'noise'):
            t_cls, t_box, s_cls, s_box = inputs(family, b, seed=17 + b)
            nl, q = 6, 900
            cost = ops.distill_match_cost_fwd(s_cls, s_box, t_cls, t_box, 1.0, 0.25)
            start = torch.arange(0, (b + 1) * q, q, dtype=torch.int32, device='cuda')
            ws = torch.empty(int(ops._lib.load().gd4d_hungarian_assign_workspace_bytes(nl, b, q, q)), dtype=torch.uint8, device='cuda')
            wd = torch.empty(int(ops._lib.load().gd4d_lsa_dense_workspace_bytes(nl, b, q, q)), dtype=torch.uint8, device='cuda')
            asg = distill.DistillHungarianAssigner3D(cls_cost=dict(type='DistillCrossEntropyLossCost', weight=1.0),
                                                     reg_cost=dict(type='BBox3DL1Cost', weight=0.25))
            res = {'batch': b, 'family': family, 'problems': nl * b, 'size': [q, q], 'reps': a.reps}
            res['host'] = timed(lambda: asg._solve(cost, nl, b, q, q, True), a.reps, a.warmup)
            res['sap'] = timed(lambda: ops.hungarian_assign_fwd(cost, start, nl, b, q, b * q, q, workspace=ws), a.reps, a.warmup)
            res['dense'] = timed(lambda: ops.lsa_dense_fwd(cost, start, nl, b, q, b * q, q, workspace=wd), a.reps, a.warmup)
            a_sap, st_sap = ops.hungarian_assign_fwd(cost, start, nl, b, q, b * q, q, workspace=ws)
            a_den, st_den = ops.lsa_dense_fwd(cost, start, nl, b, q, b * q, q, workspace=wd)
            res['dense_equals_sap'] = bool(torch.equal(a_sap, a_den)) and int(st_den.abs().sum()) == 0
            cw = torch.tensor([1.0] * 8 + [0.2, 0.2], device='cuda')
            avg = distill.distill_normalisers(b, q, q, device='cuda')
            sg, bg = s_cls.clone().requires_grad_(), s_box.clone().requires_grad_()

            def term():
                out = get_instance_distill_loss(dict(all_cls_scores=t_cls, all_bbox_preds=t_box), dict(all_cls_scores=sg, all_bbox_preds=bg),
                                                code_weights=cw, avg_factors=avg, distill_assigner=asg, **CFG)
                torch.stack(list(out.values())).sum().backward()
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                term()
            torch.cuda.current_stream().wait_stream(s)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                term()
            res['term_graph'] = timed(graph.replay, a.reps, a.warmup)
            asg.check_status()
            print(json.dumps(res), flush=True)
            rows.append(res)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
