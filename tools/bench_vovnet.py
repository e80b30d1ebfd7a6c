#!/usr/bin/env python
"""GPU time of the VoVNet-99 backbone (graph_detr4d_amd.VoVNetCP, spec 'V-99-eSE') on the library's kernels beside the module's own
torch-op route (the reference's op sequence on MIOpen's fp32 convolutions) on the same GPU, weights and inputs: per piece (stem, stages
2-5) and for the whole forward, at 6 and at 24 cameras of 3 x 320 x 800.  Prints ONE JSON line.

    python tools/bench_vovnet.py [--cams 6,24] [--hw 320 800] [--reps 7] [--window-ms 200] [--hip-only]
    python tools/bench_vovnet.py --train [--cams 6] ...     one training step (forward + backward) instead, see bench_train

Timing: each piece runs on the input the kernel route hands it (computed once).  After a warm-up of both routes on every shape, a WINDOW
is k consecutive calls between two device events, k chosen from the warm-up so that a window lasts at least --window-ms; the two routes'
windows alternate, and the figure is the median over --reps windows of the window's time per call.  `tflop` counts 2 K Cout per output
pixel over the piece's convolutions and the eSE matvecs, from the shapes (hooks on the torch-op route's layers); the kernels run three
bf16 products per multiply-add (split-bf16 x 3), so `hip_bf16_fraction_of_spec` is 3 x that over the time, against the MI355X's
2.5 PFLOP/s dense bf16 spec - a whole-piece rate including stem_1, the pooling and the eSE passes, not one kernel's share of peak.
`rel_err` is the largest difference of the two routes' outputs over the largest entry, at the timed size.  `total_hip_host_enqueue_ms`
is the host's time to enqueue one forward of the kernel route (no synchronise in the timed region).
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import graph_detr4d_amd as G  # noqa: E402
from graph_detr4d_amd import functional as Fn  # noqa: E402

BF16_SPEC = 2.5e15
PIECES = ('stem', 'stage2', 'stage3', 'stage4', 'stage5')


def event_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def windows(fns, reps, window_ms, clock=event_ms):
    """name -> (median ms per call over `reps` windows, calls per window, the windows' spread (max - min) / median); the callables'
    windows alternate."""
    calls = {}
    for k, f in fns.items():
        f()
        once = clock(f, 2)                                                   # warm, and the estimate that sizes the window
        calls[k] = max(1, min(200, math.ceil(window_ms / max(once, 1e-3))))
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            ts[k].append(clock(f, calls[k]))
    return {k: (float(np.median(v)), calls[k], float((max(v) - min(v)) / np.median(v))) for k, v in ts.items()}


def host_enqueue_ms(fn, reps):
    """Median host time to ENQUEUE one call (no synchronise inside the timed region; the queue is drained before each): the route
    decision, the kept-value look-ups, the ctypes calls and the allocations.  Below the GPU time it is hidden behind the kernels."""
    ts = []
    for _ in range(max(reps, 5)):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
        torch.cuda.synchronize()
    return float(np.median(ts))


def make_net(seed, dev):
    """V-99 with He-scaled convolutions and random frozen BatchNorm statistics (the activations keep their scale through 16 modules)."""
    torch.manual_seed(seed)
    net = G.VoVNetCP('V-99-eSE', out_features=('stage4', 'stage5'), norm_eval=True).eval()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight)
                if m.bias is not None:
                    m.bias.normal_(std=0.5)
            elif isinstance(m, nn.BatchNorm2d):
                m.running_mean.normal_(std=0.2)
                m.running_var.uniform_(0.75, 1.25)
                m.weight.uniform_(0.9, 1.1)
                m.bias.normal_(std=0.2)
    return net.to(dev)


def count_flop(piece, x):
    """2 K Cout per output element over the piece's convolutions, by hooks on one torch-op-route call."""
    total = [0]

    def hook(m, inp, out):
        total[0] += 2 * out.numel() * (m.in_channels // m.groups) * m.kernel_size[0] * m.kernel_size[1]
    handles = [m.register_forward_hook(hook) for m in piece.modules() if isinstance(m, nn.Conv2d)]
    with torch.no_grad(), Fn.torch_ops_for(*routed(piece)):
        piece(x)
    for h in handles:
        h.remove()
    return total[0]


def routed(module):
    return [m for m in module.modules() if hasattr(m, '_kernel_limits')]


def bench(net, cams, hw, reps, window_ms, routes=('hip', 'torch'), dev='cuda', clock=event_ms):
    x = torch.randn(cams, 3, *hw, device=dev, generator=torch.Generator(dev).manual_seed(cams))
    pieces = {p: getattr(net, p) for p in PIECES}

    def call(module, inp, route):
        def f():
            with torch.no_grad():
                if route == 'torch':
                    with Fn.torch_ops_for(*routed(module)):
                        return module(inp)
                return module(inp)
        return f
    # each piece's input, from the first route (the kernels, unless only the torch-op route runs)
    inputs, cur = {}, x
    for p in PIECES:
        inputs[p] = cur
        cur = call(pieces[p], cur, routes[0])()
    out = {'cams': cams, 'hw': list(hw), 'pieces': []}
    for p in PIECES:
        flop = count_flop(pieces[p], inputs[p])
        rec = {'piece': p, 'in_shape': list(inputs[p].shape), 'tflop': flop / 1e12}
        res = windows({r: call(pieces[p], inputs[p], r) for r in routes}, reps, window_ms, clock)
        for r, (ms, calls, spread) in res.items():
            rec[f'{r}_ms'], rec[f'{r}_calls_per_window'], rec[f'{r}_spread'] = ms, calls, spread
        if 'hip' in res:
            rec['hip_bf16_fraction_of_spec'] = 3 * flop / (res['hip'][0] * 1e-3) / BF16_SPEC
        if len(routes) == 2:
            a, b = (call(pieces[p], inputs[p], r)() for r in routes)
            rec['rel_err'] = float((a - b).abs().max() / b.abs().max())
        out['pieces'].append(rec)
    res = windows({r: call(net, x, r) for r in routes}, reps, window_ms, clock)
    for r, (ms, calls, spread) in res.items():
        out[f'total_{r}_ms'], out[f'total_{r}_calls_per_window'], out[f'total_{r}_spread'] = ms, calls, spread
    if 'hip' in routes and dev != 'cpu':
        out['total_hip_host_enqueue_ms'] = host_enqueue_ms(call(net, x, 'hip'), reps)
    out['total_tflop'] = sum(rec['tflop'] for rec in out['pieces'])
    if len(routes) == 2:
        a, b = (call(net, x, r)() for r in routes)
        out['total_rel_err'] = [float((u - v).abs().max() / v.abs().max()) for u, v in zip(a, b)]
        out['hip_over_torch'] = out['total_hip_ms'] / out['total_torch_ms']
    return out


def bench_train(net, cams, hw, reps, window_ms, dev='cuda'):
    """Forward + backward of the backbone as every config trains it (train() mode, norm_eval=True, every parameter trained, the images
    need no gradient) with a fixed cotangent per output: hip_train=True beside the torch-op route, each with with_cp on and off - four
    cases whose windows alternate in one process.  Per case the median ms per step and the peak allocated memory of one step above what
    is allocated between steps; `stem_*`: the stem's step alone (under hip_train it runs its own torch layers: what leaving it there
    costs)."""
    from graph_detr4d_amd import vovnet
    net.train()
    x = torch.randn(cams, 3, *hw, device=dev, generator=torch.Generator(dev).manual_seed(cams))
    osa = [m for m in net.modules() if isinstance(m, vovnet._OSA_module)]
    with torch.no_grad():
        couts = [torch.randn(o.shape, device=dev, generator=torch.Generator(dev).manual_seed(i)) for i, o in enumerate(net(x))]

    def step(route, with_cp, module=net, inp=x, cot=couts):
        def f():
            net.torch_ops, net.hip_train = route == 'torch', route == 'hip'
            for m in osa:
                m.with_cp = with_cp
            module.zero_grad(set_to_none=True)
            out = module(inp)
            torch.autograd.backward(out, cot)
        return f
    cases = {f'{r}_cp{int(c)}': step(r, c) for r in ('hip', 'torch') for c in (True, False)}
    out = {'cams': cams, 'hw': list(hw), 'mode': 'train'}
    for k, (ms, calls, spread) in windows(cases, reps, window_ms).items():
        out[f'{k}_ms'], out[f'{k}_calls_per_window'], out[f'{k}_spread'] = ms, calls, spread
    for k, f in cases.items():
        f()
        net.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        f()
        torch.cuda.synchronize()
        out[f'{k}_peak_mb'] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    with torch.no_grad():
        y = net.stem(x)
    gy = torch.randn(y.shape, device=dev, generator=torch.Generator(dev).manual_seed(99))
    stem = {f'stem_{r}': step(r, True, net.stem, x, [gy]) for r in ('hip', 'torch')}
    for k, (ms, calls, spread) in windows(stem, reps, window_ms).items():
        out[f'{k}_ms'], out[f'{k}_spread'] = ms, spread
    out['stem_share_of_hip_cp1'] = out['stem_hip_ms'] / out['hip_cp1_ms']
    out['hip_over_torch_cp1'], out['hip_over_torch_cp0'] = out['hip_cp1_ms'] / out['torch_cp1_ms'], out['hip_cp0_ms'] / out['torch_cp0_ms']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cams', default='6,24')
    ap.add_argument('--hw', type=int, nargs=2, default=(320, 800))
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--window-ms', type=float, default=200.0)
    ap.add_argument('--hip-only', action='store_true')
    ap.add_argument('--train', action='store_true', help='time one training step: hip_train=True beside the torch-op route, with_cp on and off')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_vovnet.py needs a GPU: a CPU timing says nothing about the kernels')
    net = make_net(0, 'cuda')
    routes = ('hip',) if args.hip_only else ('hip', 'torch')
    if args.train:
        print(json.dumps({'device': torch.cuda.get_device_name(0), 'spec': 'V-99-eSE', 'reps': args.reps, 'window_ms': args.window_ms,
                          'runs': [bench_train(net, int(c), tuple(args.hw), args.reps, args.window_ms) for c in args.cams.split(',')]}))
        return
    res = {'device': torch.cuda.get_device_name(0), 'spec': 'V-99-eSE', 'reps': args.reps, 'window_ms': args.window_ms,
           'runs': [bench(net, int(c), tuple(args.hw), args.reps, args.window_ms, routes) for c in args.cams.split(',')]}
    print(json.dumps(res))


if __name__ == '__main__':
    main()
