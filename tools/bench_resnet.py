#!/usr/bin/env python
"""GPU time of the ResNet backbones (graph_detr4d_amd.ResNet) with `plain_kernels=True` - the blocks' plain convolutions on the library's
kernels, frozen BatchNorm, residual and ReLU in their epilogues - beside `plain_kernels=False` of the same commit (stock torch layers on
MIOpen's fp32 convolutions; a DCN conv2 on the library's kernels on both routes) on the same GPU, weights and inputs: ResNet-50 with DCN
in stages 3 and 4, ResNet-50 without, ResNet-18; per piece (the stem with its pooling, layer1 .. layer4) and for the whole forward, eager
and as a captured hipGraph, at 6 and at 24 cameras of 3 x 320 x 800.  Prints ONE JSON line.

    python tools/bench_resnet.py [--nets r50_dcn,r50,r18] [--cams 6,24] [--hw 320 800] [--reps 7] [--window-ms 200]

Timing (tools/bench_vovnet.py's): under torch.no_grad(), each piece runs on the input the kernel route hands it (computed once).  After
a warm-up of both routes, a WINDOW is k consecutive calls between two device events, k chosen from the warm-up so that a window lasts at
least --window-ms; the two routes' windows alternate, and the figure is the median over --reps windows of the window's time per call.
`graph_*`: the whole forward captured once per route and replayed in the same windows.  `tflop` counts 2 K Cout per output pixel over
the piece's convolutions (a DCN conv2 as its plain 3x3 plus conv_offset).  `rel_err` is the largest difference of the two routes'
outputs over the largest entry, at the timed size.

    python tools/bench_resnet.py --train [--nets ...] [--cams 6,24] ...     one training step (forward + backward) instead: bench_train
"""
import argparse
import json
import os
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import graph_detr4d_amd as G  # noqa: E402
from bench_vovnet import host_enqueue_ms, windows  # noqa: E402

DCN = dict(type='DCNv2', deform_groups=1, fallback_on_stride=False)
NETS = {'r50_dcn': dict(depth=50, dcn=DCN, stage_with_dcn=(False, False, True, True)), 'r50': dict(depth=50), 'r18': dict(depth=18)}
PIECES = ('stem', 'layer1', 'layer2', 'layer3', 'layer4')
ROUTES = ('kernels', 'stock')


def make_nets(name, seed, dev):
    """{'kernels': plain_kernels=True, 'stock': plain_kernels=False} on the same weights: He-scaled convolutions, random frozen BatchNorm
    statistics, gamma around 1 (the zero-initialised last BatchNorm of a block too: the residual branch carries values).  A DCN's
    conv_offset keeps its zero weight and gets a random bias: offsets of about two pixels.  (With random conv_offset weights the offsets
    follow the untrained activations' scale, hundreds of pixels: the samples land outside the map and a last-bit difference of the two
    routes moves them across pixel borders.)"""
    kw = dict(NETS[name], norm_cfg=dict(type='BN', requires_grad=False), norm_eval=True)
    torch.manual_seed(seed)
    nets = {'kernels': G.ResNet(plain_kernels=True, **kw).eval(), 'stock': G.ResNet(**kw).eval()}
    with torch.no_grad():
        for name_, m in nets['kernels'].named_modules():
            if name_.endswith('conv_offset'):
                m.weight.zero_()                                            # mmdet's initial value; the bias alone gives offsets of
                m.bias.normal_(std=2.0)                                     # a few pixels, whatever the activations' scale
            elif hasattr(m, 'weight') and m.weight is not None and m.weight.dim() == 4:
                nn.init.kaiming_normal_(m.weight)
            elif isinstance(m, nn.BatchNorm2d):
                m.running_mean.normal_(std=0.2)
                m.running_var.uniform_(0.75, 1.25)
                m.weight.uniform_(0.9, 1.1)
                m.bias.normal_(std=0.2)
    nets['stock'].load_state_dict(nets['kernels'].state_dict(), strict=True)
    return {k: v.to(dev) for k, v in nets.items()}


def piece(net, p):
    return (lambda x: net.maxpool(net.relu(net.bn1(net.conv1(x))))) if p == 'stem' else getattr(net, p)


def count_flop(module, x):
    """2 K Cout per output pixel over the convolutions of one call of the stock route, by hooks.  A DCN conv2 is entered through
    forward_bn_relu, not as a module call: it is counted at its block, whose output has its pixels (conv3 has stride 1)."""
    total = [0]

    def hook(m, inp, out):
        pixels = out.numel() // out.shape[1]
        if isinstance(m, G.Bottleneck):
            total[0] += 2 * pixels * (m.conv2.weight.numel() + m.conv2.conv_offset.weight.numel())
        else:
            total[0] += 2 * pixels * m.weight.numel()
    hooked = [m for m in module.modules() if isinstance(m, nn.Conv2d) or (isinstance(m, G.Bottleneck) and m.with_dcn)]
    handles = [m.register_forward_hook(hook) for m in hooked]
    with torch.no_grad():
        module(x)
    for h in handles:
        h.remove()
    return total[0]


def captured(net, x):
    """A replay of the whole forward captured on x (one eager call first: the weight images exist)."""
    with torch.no_grad():
        net(x)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode='thread_local'):
            outs = net(x)
    return graph.replay, outs


def bench(name, nets, cams, hw, reps, window_ms, dev='cuda'):
    x = torch.randn(cams, 3, *hw, device=dev, generator=torch.Generator(dev).manual_seed(cams))

    def call(fn, inp):
        def f():
            with torch.no_grad():
                return fn(inp)
        return f
    inputs, cur = {}, x
    for p in PIECES:
        inputs[p] = cur
        cur = call(piece(nets['kernels'], p), cur)()
    out = {'net': name, 'cams': cams, 'hw': list(hw), 'pieces': []}
    for p in PIECES:
        rec = {'piece': p, 'in_shape': list(inputs[p].shape)}
        if p != 'stem':
            rec['tflop'] = count_flop(getattr(nets['stock'], p), inputs[p]) / 1e12
        fns = {r: call(piece(nets[r], p), inputs[p]) for r in ROUTES}
        for r, (ms, calls, spread) in windows(fns, reps, window_ms).items():
            rec[f'{r}_ms'], rec[f'{r}_calls_per_window'], rec[f'{r}_spread'] = ms, calls, spread
        a, b = (fns[r]() for r in ROUTES)
        rec['rel_err'] = float((a - b).abs().max() / b.abs().max())
        rec['kernels_over_stock'] = rec['kernels_ms'] / rec['stock_ms']
        out['pieces'].append(rec)
    fns = {r: call(nets[r], x) for r in ROUTES}
    for r, (ms, calls, spread) in windows(fns, reps, window_ms).items():
        out[f'total_{r}_ms'], out[f'total_{r}_calls_per_window'], out[f'total_{r}_spread'] = ms, calls, spread
    out['kernels_over_stock'] = out['total_kernels_ms'] / out['total_stock_ms']
    a, b = (fns[r]() for r in ROUTES)
    out['total_rel_err'] = [float((u - v).abs().max() / v.abs().max()) for u, v in zip(a, b)]
    out['total_kernels_host_enqueue_ms'] = host_enqueue_ms(fns['kernels'], reps)
    out['total_stock_host_enqueue_ms'] = host_enqueue_ms(fns['stock'], reps)
    replays = {}
    for r in ROUTES:
        replays[r], outs = captured(nets[r], x)
        replays[r]()
        torch.cuda.synchronize()
        out[f'graph_{r}_equals_eager'] = all(torch.equal(u, v) for u, v in zip(outs, fns[r]()))
    assert out['graph_kernels_equals_eager'], f'{name}: the kernel route\'s replay differs from its eager call'
    for r, (ms, calls, spread) in windows(replays, reps, window_ms).items():
        out[f'graph_{r}_ms'], out[f'graph_{r}_calls_per_window'], out[f'graph_{r}_spread'] = ms, calls, spread
    out['graph_kernels_over_stock'] = out['graph_kernels_ms'] / out['graph_stock_ms']
    return out


def make_train_nets(name, seed, dev):
    """make_nets' two networks as the configs train them: frozen_stages=1, norm_eval=True, frozen BatchNorm parameters, train() mode;
    'kernels' with plain_train=True.  hip_train=True on the DCN layers of BOTH (the default route's stock layers around the DCN's own
    training kernels is what the same commit offers without the switch)."""
    kw = dict(NETS[name], norm_cfg=dict(type='BN', requires_grad=False), norm_eval=True, frozen_stages=1)
    hip = 'dcn' in kw
    eval_nets = make_nets(name, seed, 'cpu')
    nets = {'kernels': G.ResNet(plain_kernels=True, plain_train=True, hip_train=hip, **kw), 'stock': G.ResNet(hip_train=hip, **kw)}
    for r, net in nets.items():
        net.load_state_dict(eval_nets['kernels'].state_dict(), strict=True)
        nets[r] = net.to(dev).train()
    return nets


def kernel_times(fn):
    """{kernel name: (calls, total ms)} of one call of fn, the library's GEMM, weight-gradient and elementwise kernels only, by
    torch.profiler; {} with the reason under 'error' where the profiler is not available."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        rows = {}
        for e in prof.key_averages():
            total = getattr(e, 'device_time_total', None)
            total = getattr(e, 'cuda_time_total', 0.0) if total is None else total
            if any(t in e.key for t in ('gd4d', 'vv_gemm', 'rt_', 'vt_', 'dcn_')) and total > 0:
                rows[e.key[:160]] = [int(e.count), total / 1e3]
        return rows
    except Exception as exc:                                                    # noqa: BLE001  (a tool: report, do not die)
        return {'error': repr(exc)}


def bench_train(name, nets, cams, hw, reps, window_ms, dev='cuda'):
    """Forward + backward of the backbone (the images need no gradient, layer1 and the stem are frozen) with a fixed cotangent on the
    outputs of layer2 .. layer4: plain_train=True beside the default route's stock torch layers, alternating windows.  Per route the
    median ms per step, the peak allocated memory of one step above what is allocated between steps, and the HIP route's kernels."""
    x = torch.randn(cams, 3, *hw, device=dev, generator=torch.Generator(dev).manual_seed(cams))
    with torch.no_grad():
        couts = [torch.randn(o.shape, device=dev, generator=torch.Generator(dev).manual_seed(i)) for i, o in enumerate(nets['stock'](x))]

    def step(net):
        def f():
            net.zero_grad(set_to_none=True)
            outs = net(x)
            torch.autograd.backward(outs[1:], couts[1:])
        return f
    fns = {r: step(nets[r]) for r in ROUTES}
    out = {'net': name, 'cams': cams, 'hw': list(hw), 'mode': 'train'}
    for r, (ms, calls, spread) in windows(fns, reps, window_ms).items():
        out[f'{r}_ms'], out[f'{r}_calls_per_window'], out[f'{r}_spread'] = ms, calls, spread
    out['kernels_over_stock'] = out['kernels_ms'] / out['stock_ms']
    grads = {}
    for r, f in fns.items():
        f()
        grads[r] = {k: p.grad.clone() for k, p in nets[r].named_parameters() if p.grad is not None}
        nets[r].zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        f()
        torch.cuda.synchronize()
        out[f'{r}_peak_mb'] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    assert set(grads['kernels']) == set(grads['stock'])
    out['grad_rel_err_max'] = max(float((grads['kernels'][k] - v).abs().max() / v.abs().max().clamp(min=1e-30)) for k, v in grads['stock'].items())
    out['kernels_host_enqueue_ms'] = host_enqueue_ms(fns['kernels'], reps)
    out['stock_host_enqueue_ms'] = host_enqueue_ms(fns['stock'], reps)
    out['kernel_times_ms'] = kernel_times(fns['kernels'])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nets', default='r50_dcn,r50,r18')
    ap.add_argument('--cams', default='6,24')
    ap.add_argument('--hw', type=int, nargs=2, default=(320, 800))
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--window-ms', type=float, default=200.0)
    ap.add_argument('--train', action='store_true', help='time one training step: plain_train=True beside the default route')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_resnet.py needs a GPU: a CPU timing says nothing about the kernels')
    runs = []
    for name in args.nets.split(','):
        nets = make_train_nets(name, 0, 'cuda') if args.train else make_nets(name, 0, 'cuda')
        for c in args.cams.split(','):
            if args.train:
                runs.append(bench_train(name, nets, int(c), tuple(args.hw), args.reps, args.window_ms))
                print(f'{name} at {c} cameras, one training step: kernels {runs[-1]["kernels_ms"]:.2f} ms, stock {runs[-1]["stock_ms"]:.2f} ms',
                      file=sys.stderr)
                continue
            runs.append(bench(name, nets, int(c), tuple(args.hw), args.reps, args.window_ms))
            print(f'{name} at {c} cameras: kernels {runs[-1]["total_kernels_ms"]:.2f} ms, stock {runs[-1]["total_stock_ms"]:.2f} ms', file=sys.stderr)
        del nets
        torch.cuda.empty_cache()
    print(json.dumps({'device': torch.cuda.get_device_name(0), 'reps': args.reps, 'window_ms': args.window_ms, 'runs': runs}))


if __name__ == '__main__':
    main()
