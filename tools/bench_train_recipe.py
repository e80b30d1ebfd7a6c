#!/usr/bin/env python
"""Timing of the optimizer step alone, captured in a hipGraph and replayed: FlatGradAllReducer.adamw_step (gd4d_adamw_flat) against
TrainRecipe.step (gd4d_adamw_recipe_flat: static loss scale 512, cosine schedule with linear warmup, two parameter groups), with and
without zero_grads, and a skipped step (an inf in the gradients), at n = the decoder's flat buffer (~5.5 M elements, 22 MB) and
n = 82.5 M (330 MB, the full-model size dist.preflight plans all-reduces for).  Device events around each replay, medians of --iters
replays after --warmup; the whole measurement is repeated --repeats times and the spread of the medians is reported.

    python tools/bench_train_recipe.py [--iters 30] [--warmup 5] [--repeats 5] [--json OUT]

The step moves 28 bytes per element (read p, g, m, v; write p, m, v; + 4 with zero_grads) plus 4 for the norm pass; a skipped step
reads g twice (8 bytes, + 4 with zero_grads).  `GBps` is bytes / median.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from graph_detr4d_amd import TrainRecipe, dist as D  # noqa: E402

OPTIMIZER = dict(type='AdamW', lr=2e-4, paramwise_cfg=dict(custom_keys={'img_backbone': dict(lr_mult=0.1)}), weight_decay=0.01)
OPTIMIZER_CONFIG = dict(grad_clip=dict(max_norm=35, norm_type=2))
LR_CONFIG = dict(policy='CosineAnnealing', warmup='linear', warmup_iters=500, warmup_ratio=1.0 / 3, min_lr_ratio=1e-3)


def replay_ms(graph, iters, warmup, before=None):
    times = []
    for i in range(warmup + iters):
        if before is not None:
            before()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        graph.replay()
        e.record()
        e.synchronize()
        if i >= warmup:
            times.append(s.elapsed_time(e))
    times.sort()
    return times[len(times) // 2]


def capture(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()                                                                   # (one eager call: allocations and lazy loads done)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def setup(n):
    """Two parameters (a 'backbone' tenth and the rest) over one flat buffer of n elements, gradients of unit scale x 512."""
    class M(torch.nn.Module):
        def __init__(self):
            super().__init__()
            k = max(4, n // 10 // 4 * 4)
            self.img_backbone = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(k, device='cuda') * 0.02)])
            self.head = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(n - k, device='cuda') * 0.02)])
    model = M()
    red = D.FlatGradAllReducer(list(model.parameters()), align=4)
    red.bind()
    return model, red


def measure(n, iters, warmup):
    res = {}
    n = n // 4 * 4                                                             # (no padding: the buffers have n elements)
    grads = torch.randn(n, device='cuda') * 1e-3 * 512.0
    # parent
    model, red = setup(n)
    red.adamw_state()

    def fill(r):
        return lambda: r.flat[:r.numel].copy_(grads[:r.numel])
    g = capture(lambda: red.adamw_step(lr=2e-4, weight_decay=0.01, max_norm=35.0))
    res['parent_adamw_step_ms'] = replay_ms(g, iters, warmup, fill(red))
    del g, model, red
    for key, zero in (('recipe_step_ms', False), ('recipe_step_zero_grads_ms', True)):
        model, red = setup(n)
        rec = TrainRecipe(red, model.named_parameters(), optimizer=OPTIMIZER, optimizer_config=OPTIMIZER_CONFIG, lr_config=LR_CONFIG,
                          fp16=dict(loss_scale=512.), max_epochs=24, iters_per_epoch=1000)
        rec.state()
        assert len(rec.ranges) == 2
        g = capture(lambda: rec.step(zero_grads=zero))
        res[key] = replay_ms(g, iters, warmup, fill(red))
        assert int(rec.found_inf) == 0 and int(rec.skipped_steps) == 0
        if zero:                                                               # the skipped step: an inf among the gradients
            def poisoned():
                fill(red)()
                red.flat[n // 2] = float('inf')
            res['recipe_skipped_step_zero_grads_ms'] = replay_ms(g, iters, warmup, poisoned)
            assert int(rec.found_inf) == 1 and int(rec.skipped_steps) == iters + warmup
        del g, model, red, rec
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--sizes', type=int, nargs='+', default=[5_500_000, 82_500_000])
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    bytes_per = {'parent_adamw_step_ms': 32, 'recipe_step_ms': 32, 'recipe_step_zero_grads_ms': 36, 'recipe_skipped_step_zero_grads_ms': 12}
    out = {}
    for n in a.sizes:
        runs = [measure(n, a.iters, a.warmup) for _ in range(a.repeats)]
        out[f'n{n}'] = r = {}
        for key in runs[0]:
            vals = sorted(x[key] for x in runs)
            med = vals[len(vals) // 2]
            r[key] = dict(median_ms=med, min_ms=vals[0], max_ms=vals[-1], GBps=bytes_per[key] * n / med / 1e6)
        print(f'n={n}: ' + ', '.join(f'{k}={v["median_ms"]:.4f} [{v["min_ms"]:.4f}, {v["max_ms"]:.4f}] ms {v["GBps"]:.0f} GB/s'
                                     for k, v in r.items()), flush=True)
    line = json.dumps(dict(device=torch.cuda.get_device_name(0), iters=a.iters, warmup=a.warmup, repeats=a.repeats, results=out))
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
