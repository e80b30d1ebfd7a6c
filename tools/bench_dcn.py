#!/usr/bin/env python
"""GPU time of DCNv2 (graph_detr4d_amd.ModulatedDeformConv2dPack) on the library's kernels beside the module's own torch-op route (nine
grid_sample calls and an einsum, fp32: the only way this platform could run the layer before the kernels existed) on the same GPU and
inputs, the two routes alternated call by call; and the two kernels on their own.  Prints ONE JSON line.

    python tools/bench_dcn.py [--reps 10] [--cams 24] [--hip-only] [--train]

Workload: the nine DCN layers of an R50 with stage_with_dcn=(False, False, True, True) for a 928 x 1600 image - stage 3 (256
channels): 116 x 200 -> 58 x 100 at stride 2 once, 58 x 100 at stride 1 five times; stage 4 (512 channels): 58 x 100 -> 29 x 50 at stride
2 once, 29 x 50 at stride 1 twice - each as relu(bn2(conv2(x))) with a frozen BatchNorm (forward_bn_relu), N = cameras.  Offsets are
those of a conv_offset with random weights (sigma ~ 2 px), not zeros: the gather is not a regular halo read.
Timing: device events around each call, after a warm-up of every shape; medians.  FLOP from shapes: 2 x 9 Cin Cout per output pixel
for the main kernel, 2 x 9 Cin 27 for conv_offset; the kernels run three bf16 products per multiply-add (split-bf16 x 3), so the rate
of bf16 products is 3x that, against the MI355X's 2.5 PFLOP/s dense bf16 spec (gd4d_depth_conv_fwd, the same GEMM without the gather:
0.40-0.41 of it).  `extra_bytes`: what each route allocates above its input and output per call (torch.cuda.max_memory_allocated).

--train: forward + backward of the same layers in train() mode behind the frozen BatchNorm (loss = <out, r>), `hip_train=True` beside the
torch-op route (what training took before the backward kernels), same process, inputs and timing loop; each route's peak bytes above
the input, the output and the gradients it returns; and the backward's kernels on their own (data, weight gradient, the two
conv_offset kernels), the data kernel's rate beside the forward kernel's on the same shape (the same FLOP count: K = Cout instead of
9 Cin, M = 9 Cin instead of Cout).
"""
import argparse
import contextlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import graph_detr4d_amd as G  # noqa: E402
from graph_detr4d_amd import functional as Fn  # noqa: E402
from graph_detr4d_amd import ops  # noqa: E402

BF16_SPEC = 2.5e15
# (name, channels, input (h, w), stride, how many such layers an R50 has)
LAYERS = [('stage3_s2', 256, (116, 200), 2, 1), ('stage3_s1', 256, (58, 100), 1, 5), ('stage4_s2', 512, (58, 100), 2, 1),
          ('stage4_s1', 512, (29, 50), 1, 2)]


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(fns, reps):
    """Median ms of each callable, interleaved call by call (the same host / clock conditions for all)."""
    for f in fns.values():
        f()
        f()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            ts[k].append(event_ms(f))
    return {k: float(np.median(v)) for k, v in ts.items()}


def extra_bytes(fn, keep):
    """Peak bytes allocated during fn() above what is live before it, less the result it returns (`keep` bytes)."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    del out
    return int(peak - base - keep)


def layer(name, c, hw, stride, count, n, reps, hip_only):
    torch.manual_seed(hash(name) % 1000)
    m = G.ModulatedDeformConv2dPack(c, c, 3, stride=stride, padding=1, bias=False).cuda().eval()
    bn = torch.nn.BatchNorm2d(c).cuda().eval()
    with torch.no_grad():
        m.conv_offset.weight.normal_(std=2.0 * (9 * c) ** -0.5)
        m.conv_offset.bias.normal_(std=0.5)
        bn.running_mean.normal_(std=0.3)
        bn.running_var.uniform_(0.5, 2.0)
    x = torch.randn(n, c, *hw, device='cuda')
    ho, wo = ops.dcn_out_hw(*hw, stride)
    px = n * ho * wo
    flop, off_flop = 2 * 9 * c * c * px, 2 * 9 * c * 27 * px
    out = {'layer': name, 'channels': c, 'in_hw': list(hw), 'stride': stride, 'count_in_r50': count, 'cams': n,
           'tflop': flop / 1e12, 'offset_tflop': off_flop / 1e12}

    def hip():
        with torch.no_grad():
            return m.forward_bn_relu(x, bn)

    def tor():
        with torch.no_grad(), Fn.torch_ops_for(m):
            return m.forward_bn_relu(x, bn)
    fns = {'hip': hip} if hip_only else {'hip': hip, 'torch': tor}
    for k, v in alternate(fns, reps).items():
        out[f'{k}_ms'] = v
    keep = 4 * n * c * ho * wo
    out['hip_extra_bytes'] = extra_bytes(hip, keep)
    if not hip_only:
        out['torch_extra_bytes'] = extra_bytes(tor, keep)
        err = float((hip() - tor()).abs().max() / tor().abs().max())
        out['hip_vs_torch_rel_err'] = err
    # the two kernels on their own
    with torch.no_grad():
        m.refresh_images()
        om = ops.dcn_offset_conv_fwd(x, m._offset_image(), m.conv_offset.bias.detach(), stride=stride)
        scale, shift = m._folded(bn)
        y = ops.dcn_fwd(x, om, m._weight_image(), c, stride=stride, scale=scale, shift=shift, relu=True)
        t = alternate({'offset_conv': lambda: ops.dcn_offset_conv_fwd(x, m._offset_image(), m.conv_offset.bias.detach(), stride=stride, out=om),
                       'dcn': lambda: ops.dcn_fwd(x, om, m._weight_image(), c, stride=stride, scale=scale, shift=shift, relu=True, out=y)},
                      reps)
    out['offset_conv_kernel_ms'] = t['offset_conv']
    out['dcn_kernel_ms'] = t['dcn']
    out['dcn_kernel_bf16_pflops'] = 3 * flop / t['dcn'] / 1e12
    out['dcn_kernel_fraction_of_spec'] = 3 * flop / (t['dcn'] * 1e-3) / BF16_SPEC
    out['offset_conv_kernel_bf16_pflops'] = 3 * off_flop / t['offset_conv'] / 1e12
    return out


def layer_train(name, c, hw, stride, count, n, reps, hip_only):
    torch.manual_seed(hash(name) % 1000)
    m = G.ModulatedDeformConv2dPack(c, c, 3, stride=stride, padding=1, bias=False, hip_train=True).cuda().train()
    bn = torch.nn.BatchNorm2d(c).cuda().eval()
    for p in bn.parameters():
        p.requires_grad = False
    with torch.no_grad():
        m.conv_offset.weight.normal_(std=2.0 * (9 * c) ** -0.5)
        m.conv_offset.bias.normal_(std=0.5)
        bn.running_mean.normal_(std=0.3)
        bn.running_var.uniform_(0.5, 2.0)
    x = torch.randn(n, c, *hw, device='cuda', requires_grad=True)
    ho, wo = ops.dcn_out_hw(*hw, stride)
    r = torch.randn(n, c, ho, wo, device='cuda')
    px = n * ho * wo
    flop = 2 * 9 * c * c * px
    out = {'layer': name, 'channels': c, 'in_hw': list(hw), 'stride': stride, 'count_in_r50': count, 'cams': n, 'tflop': flop / 1e12}

    def step(torch_route):
        def f():
            x.grad = None
            for p in m.parameters():
                p.grad = None
            with (Fn.torch_ops_for(m) if torch_route else contextlib.nullcontext()):
                y = m.forward_bn_relu(x, bn)
            y.backward(r)
            return y
        return f
    fns = {'hip_train': step(False)} if hip_only else {'hip_train': step(False), 'torch_train': step(True)}
    for k, v in alternate(fns, reps).items():
        out[f'{k}_ms'] = v
    x.grad = None
    for p in m.parameters():
        p.grad = None
    keep = 4 * (n * c * ho * wo + x.numel() + sum(p.numel() for p in m.parameters()))       # the output and the gradients returned
    for k, f in fns.items():
        out[f'{k}_extra_bytes'] = extra_bytes(f, keep)
        x.grad = None
        for p in m.parameters():
            p.grad = None
    # the backward's kernels on their own, and the forward kernel on the same shape
    with torch.no_grad():
        xd = x.detach()
        om = ops.dcn_offset_conv_fwd(xd, m._offset_image(), m.conv_offset.bias.detach(), stride=stride)
        scale, shift = m._folded(bn)
        y = ops.dcn_fwd(xd, om, m._weight_image(), c, stride=stride, scale=scale, shift=shift, relu=True)
        image_t, off_w = m._weight_image_t(), m.conv_offset.weight.detach()
        dx, doff = ops.dcn_bwd_data(r, xd, om, image_t, c, stride=stride, y=y, scale=scale, sigmoid_grad=True)
        t = alternate({
            'fwd': lambda: ops.dcn_fwd(xd, om, m._weight_image(), c, stride=stride, scale=scale, shift=shift, relu=True, out=y),
            'data': lambda: ops.dcn_bwd_data(r, xd, om, image_t, c, stride=stride, y=y, scale=scale, sigmoid_grad=True, dx=dx),
            'data_no_dx': lambda: ops.dcn_bwd_data(r, xd, om, image_t, c, stride=stride, y=y, scale=scale, sigmoid_grad=True, want_dx=False),
            'wgrad': lambda: ops.dcn_wgrad(r, xd, om, c, stride=stride, y=y, scale=scale),
            'offset_dgrad': lambda: ops.dcn_offset_conv_dgrad(doff, off_w, dx, stride=stride),
            'offset_wgrad': lambda: ops.dcn_offset_conv_wgrad(doff, xd, stride=stride)}, reps)
    for k, v in t.items():
        out[f'{k}_kernel_ms'] = v
    out['fwd_kernel_fraction_of_spec'] = 3 * flop / (t['fwd'] * 1e-3) / BF16_SPEC
    out['data_kernel_fraction_of_spec'] = 3 * flop / (t['data'] * 1e-3) / BF16_SPEC
    out['wgrad_kernel_fraction_of_spec'] = 3 * flop / (t['wgrad'] * 1e-3) / BF16_SPEC
    out['dx_atomic_bytes'] = 4 * 4 * 9 * c * px                             # at most four 4-byte adds per (tap, channel, pixel)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--cams', type=int, default=24)
    ap.add_argument('--hip-only', action='store_true')
    ap.add_argument('--train', action='store_true', help='forward + backward: hip_train=True beside the torch-op route')
    ap.add_argument('--layers', default='', help='comma-separated layer names (default: all four shapes)')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_dcn.py needs a GPU: a CPU timing says nothing about the kernels')
    specs = [s for s in LAYERS if not args.layers or s[0] in args.layers.split(',')]
    if args.train:
        res = {'device': torch.cuda.get_device_name(0), 'reps': args.reps, 'mode': 'train',
               'layers': [layer_train(*spec, args.cams, args.reps, args.hip_only) for spec in specs]}
        for route in ('hip_train',) if args.hip_only else ('hip_train', 'torch_train'):
            res[f'nine_layers_{route}_ms'] = sum(l[f'{route}_ms'] * l['count_in_r50'] for l in res['layers'])
        print(json.dumps(res))
        return
    res = {'device': torch.cuda.get_device_name(0), 'reps': args.reps,
           'layers': [layer(*spec, args.cams, args.reps, args.hip_only) for spec in specs]}
    for route in ('hip',) if args.hip_only else ('hip', 'torch'):
        res[f'nine_layers_{route}_ms'] = sum(l[f'{route}_ms'] * l['count_in_r50'] for l in res['layers'])
    res['nine_layers_tflop'] = sum((l['tflop'] + l['offset_tflop']) * l['count_in_r50'] for l in res['layers'])
    print(json.dumps(res))


if __name__ == '__main__':
    main()
