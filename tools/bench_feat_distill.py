"""Times MixDistill's feature-distillation term, forward + backward, at the shipped size - 24 cameras x the R50 pyramid (116 x 200 ...
15 x 25), 256 channels - on both routes of FeatureDistillLoss: the HIP route (gd4d_feat_distill.hip) and the torch-op route (nn.Conv2d,
the reference's ops, autograd), which is the baseline.  hipEvents around each step, warm-up, the median; the peak of the allocator above
what the inputs and parameters hold.  One JSON line per (type, route).

  python tools/bench_feat_distill.py [--cams 24] [--steps 20] [--warmup 5] [--types vanilla attention]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

R50 = [(116, 200), (58, 100), (29, 50), (15, 25)]


def measure(mod, teacher, student, steps, warmup):
    params = list(mod.parameters())

    def step():
        for p in params + student:
            p.grad = None
        mod(teacher, student)['feat_loss'].backward()
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    for p in params + student:
        p.grad = None
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    times = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times), (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cams', type=int, default=24)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--types', nargs='+', default=['vanilla', 'attention'])
    args = ap.parse_args()
    from graph_detr4d_amd import FeatureDistillLoss
    dev = 'cuda:0'
    g = torch.Generator().manual_seed(0)
    teacher = [(torch.randn(1, args.cams, 256, h, w, generator=g) * (0.25 + 2.0 * torch.rand(1, args.cams, 256, 1, 1, generator=g))).to(dev)
               for h, w in R50]
    student = [torch.randn(1, args.cams, 256, h, w, generator=g).to(dev).requires_grad_() for h, w in R50]
    pyramid_mb = sum(t.numel() for t in teacher) * 4 / 2 ** 20
    for kind in args.types:
        torch.manual_seed(1)
        mod = FeatureDistillLoss(dict(type=kind, loss_weight=1.0)).to(dev)
        losses = {}
        for route in ('hip', 'torch_ops'):
            mod.torch_ops = route == 'torch_ops'
            med, best, peak = measure(mod, teacher, student, args.steps, args.warmup)
            losses[route] = float(mod(teacher, student)['feat_loss'].detach())
            print(json.dumps(dict(bench='feat_distill', type=kind, route=route, cams=args.cams, levels=R50, median_ms=round(med, 3),
                                  min_ms=round(best, 3), peak_extra_mb=round(peak, 1), pyramid_mb=round(pyramid_mb, 1),
                                  loss=losses[route], steps=args.steps, warmup=args.warmup)), flush=True)
        print(json.dumps(dict(bench='feat_distill', type=kind, loss_rel_diff=abs(losses['hip'] - losses['torch_ops']) / abs(losses['torch_ops']))),
              flush=True)


if __name__ == '__main__':
    main()
