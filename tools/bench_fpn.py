#!/usr/bin/env python
"""GPU time of the neck (graph_detr4d_amd.FPN / CPFPN) on the library's kernels beside the module's own torch-op route (nn.Conv2d +
F.interpolate in fp32: what a user ran before the kernels existed) on the same GPU and inputs, the two routes alternated call by
call; and each kernel on its own.  Prints ONE JSON line.

    python tools/bench_fpn.py [--reps 20] [--cams 24 12] [--hip-only]
    python tools/bench_fpn.py --train [--reps 10] [--cams 24 12]

--train: forward + backward of `hip_train=True` beside `torch_ops=True` (the module's torch layers under autograd: how the neck was
trained before the backward kernels existed) on the same inputs, alternated call by call, every parameter and input requiring grad;
and each backward kernel on its own.  The input gradient of a lateral does 2 Cin 256 FLOP per pixel, its weight gradient the same; the
top-down adjoint and the lateral weight gradient are also given as bytes (adjoint: the finer map read, the coarser read and written;
weight gradient: x once and the lateral's gradient once per 64-channel chunk of Cin, which is what the kernel reads) against 8 TB/s.

Workloads: the R50 pyramid (inputs (N, 512, 116, 200), (N, 1024, 58, 100), (N, 2048, 29, 50); mmdet FPN, start_level=1, one extra
level) and the VoVNet CPFPN shapes (in_channels [256, 512, 768, 1024] at strides 4 .. 32 of a 928 x 1600 image).
Timing: device events around each call, after a warm-up of every shape; medians.  FLOP counts from shapes (2 Cin 256 per lateral
pixel, 2 x 2304 x 256 per 3x3 pixel); the kernels run three bf16 products per multiply-add (split-bf16 x 3), so their rate of bf16
products is 3x that, against the MI355X's 2.5 PFLOP/s dense bf16 spec.  The lateral's bytes are its input, its output and the
coarser lateral it reads, against 8 TB/s of HBM.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import graph_detr4d_amd as G  # noqa: E402
from graph_detr4d_amd import ops  # noqa: E402

BF16_SPEC, HBM_SPEC = 2.5e15, 8.0e12
R50 = dict(cls='FPN', cfg=dict(in_channels=[256, 512, 1024, 2048], out_channels=256, start_level=1, add_extra_convs='on_output',
                               num_outs=4, relu_before_extra_convs=True),
           hw=[(232, 400), (116, 200), (58, 100), (29, 50)])
VOV = dict(cls='CPFPN', cfg=dict(in_channels=[256, 512, 768, 1024], out_channels=256, start_level=0, add_extra_convs='on_output',
                                 num_outs=4, relu_before_extra_convs=True),
           hw=[(232, 400), (116, 200), (58, 100), (29, 50)])


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


def workload(spec, n, reps, hip_only):
    cfg, s = spec['cfg'], spec['cfg']['start_level']
    torch.manual_seed(n)
    mod = getattr(G, spec['cls'])(**cfg).cuda().eval()
    xs = [torch.randn(n, c, *hw, device='cuda') if i >= s else torch.empty(n, c, 1, 1, device='cuda')
          for i, (c, hw) in enumerate(zip(cfg['in_channels'], spec['hw']))]
    used = list(zip(cfg['in_channels'], spec['hw']))[s:]
    lat_flop = sum(2 * c * 256 * n * h * w for c, (h, w) in used)
    conv_px = n * (sum(h * w for _, (h, w) in used) if spec['cls'] == 'FPN' else used[0][1][0] * used[0][1][1])
    conv_flop = 2 * 2304 * 256 * conv_px
    out = {'cams': n, 'lateral_tflop': lat_flop / 1e12, 'conv3x3_tflop': conv_flop / 1e12}

    def run(m):
        def f():
            with torch.no_grad():
                m(xs)
        return f
    fns = {'hip': run(mod)}
    mod_cl = getattr(G, spec['cls'])(**cfg, channels_last_out=True).cuda().eval()
    fns['hip_channels_last_out'] = run(mod_cl)
    if not hip_only:
        tor = getattr(G, spec['cls'])(**cfg, torch_ops=True).cuda().eval()
        fns['torch'] = run(tor)
    for k, v in alternate(fns, reps).items():
        out[f'{k}_forward_ms'] = v
    out['hip_forward_bf16_pflops'] = 3 * (lat_flop + conv_flop) / out['hip_forward_ms'] / 1e12
    out['hip_forward_fraction_of_spec'] = 3 * (lat_flop + conv_flop) / (out['hip_forward_ms'] * 1e-3) / BF16_SPEC

    # the kernels on their own, in the module's launch order
    with torch.no_grad():
        lat_img, conv_img = mod._all_images()
        lats, per = [None] * len(used), {}
        for i in range(len(used) - 1, -1, -1):
            x, b = xs[i + s], mod.lateral_convs[i].conv.bias.detach()
            up = lats[i + 1] if i + 1 < len(used) else None
            lats[i] = ops.fpn_lateral_fwd(x, lat_img[i], b, up=up)
            per[f'lateral{i}'] = (lambda x=x, img=lat_img[i], b=b, up=up, o=lats[i]: ops.fpn_lateral_fwd(x, img, b, up=up, out=o))
        nconv = len(used) if spec['cls'] == 'FPN' else 1
        biases = [m.conv.bias.detach() for m in mod.fpn_convs]
        outs = ops.fpn_conv_fwd(lats[:nconv], conv_img[:nconv], biases[:nconv])
        per['conv3x3'] = lambda: ops.fpn_conv_fwd(lats[:nconv], conv_img[:nconv], biases[:nconv], outs=outs)
        if len(mod.fpn_convs) > nconv:
            ex = ops.fpn_extra_conv_fwd(outs[-1], conv_img[nconv], biases[nconv])
            per['extra'] = lambda: ops.fpn_extra_conv_fwd(outs[-1], conv_img[nconv], biases[nconv], out=ex)
        t = alternate(per, reps)
    kern = {}
    for i, (c, (h, w)) in enumerate(used):
        ms = t[f'lateral{i}']
        flop = 2 * c * 256 * n * h * w
        nbytes = 4 * n * h * w * (c + 256) + (4 * n * 256 * used[i + 1][1][0] * used[i + 1][1][1] if i + 1 < len(used) else 0)
        kern[f'lateral{i}'] = {'cin': c, 'hw': [h, w], 'ms': ms, 'bf16_pflops': 3 * flop / ms / 1e12,
                               'fraction_of_spec': 3 * flop / (ms * 1e-3) / BF16_SPEC, 'gbytes': nbytes / 1e9,
                               'tbytes_per_s': nbytes / (ms * 1e-3) / 1e12, 'fraction_of_hbm': nbytes / (ms * 1e-3) / HBM_SPEC}
    kern['conv3x3'] = {'pixels': conv_px, 'ms': t['conv3x3'], 'bf16_pflops': 3 * conv_flop / t['conv3x3'] / 1e12,
                       'fraction_of_spec': 3 * conv_flop / (t['conv3x3'] * 1e-3) / BF16_SPEC}
    if 'extra' in t:
        kern['extra'] = {'ms': t['extra']}
    out['kernels'] = kern
    return out


def rate(flop, ms):
    return {'ms': ms, 'bf16_pflops': 3 * flop / ms / 1e12, 'fraction_of_spec': 3 * flop / (ms * 1e-3) / BF16_SPEC}


def traffic(nbytes, ms):
    return {'gbytes': nbytes / 1e9, 'tbytes_per_s': nbytes / (ms * 1e-3) / 1e12, 'fraction_of_hbm': nbytes / (ms * 1e-3) / HBM_SPEC}


def train_workload(spec, n, reps):
    cfg, s = spec['cfg'], spec['cfg']['start_level']
    torch.manual_seed(n)
    hip = getattr(G, spec['cls'])(**cfg, hip_train=True).cuda().train()
    tor = getattr(G, spec['cls'])(**cfg, torch_ops=True).cuda().train()
    tor.load_state_dict(hip.state_dict())
    xs = [torch.randn(n, c, *hw, device='cuda').requires_grad_(i >= s) if i >= s else torch.empty(n, c, 1, 1, device='cuda')
          for i, (c, hw) in enumerate(zip(cfg['in_channels'], spec['hw']))]
    used = list(zip(cfg['in_channels'], spec['hw']))[s:]
    with torch.no_grad():
        rs = [torch.randn_like(o) for o in tor(xs)]

    def step(m):
        def f():
            for p in m.parameters():
                p.grad = None
            for x in xs:
                x.grad = None
            outs = m(xs)
            torch.autograd.backward(outs, rs)
        return f
    out = {'cams': n}
    for k, v in alternate({'hip_train': step(hip), 'torch': step(tor)}, reps).items():
        out[f'{k}_fwd_bwd_ms'] = v

    # the backward kernels on their own, on gradients of the right shapes
    nconv = len(used) if spec['cls'] == 'FPN' else 1
    with torch.no_grad():
        lat_t, conv_t = hip._all_images_t()
        gls = [torch.randn(n, 256, *hw, device='cuda') for _, hw in used]
        per = {}
        for i, (c, hw) in enumerate(used):
            x = xs[i + s].detach()
            per[f'lateral{i}_dgrad'] = lambda g=gls[i], img=lat_t[i], c=c: ops.fpn_lateral_dgrad(g, img, c)
            per[f'lateral{i}_wgrad'] = lambda g=gls[i], x=x: ops.fpn_lateral_wgrad(g, x)
            if i + 1 < len(used):
                per[f'topdown{i}'] = lambda g=gls[i], c=gls[i + 1]: ops.fpn_topdown_bwd(g, c)
        per['conv3x3_dgrad'] = lambda: ops.fpn_conv_fwd(gls[:nconv], conv_t[:nconv], [None] * nconv)
        per['conv3x3_wgrad'] = lambda: [ops.depth_conv_wgrad([g], [l]) for g, l in zip(gls[:nconv], gls[:nconv])]
        per['conv3x3_bias'] = lambda: [ops.fpn_bias_grad(g) for g in gls[:nconv]]
        if len(hip.fpn_convs) > nconv:
            h, w = used[-1][1]
            dy = torch.randn(n, 256, (h + 1) // 2, (w + 1) // 2, device='cuda')
            per['extra_dgrad'] = lambda: ops.fpn_extra_conv_dgrad(dy, conv_t[nconv], (h, w), add=gls[-1])
            per['extra_wgrad'] = lambda: ops.fpn_extra_conv_wgrad(dy, gls[-1])
        t = alternate(per, reps)
    kern = {}
    for i, (c, (h, w)) in enumerate(used):
        px, flop = n * h * w, 2 * c * 256 * n * h * w
        kern[f'lateral{i}_dgrad'] = dict(rate(flop, t[f'lateral{i}_dgrad']), cin=c, hw=[h, w])
        chunks = (c + 63) // 64
        kern[f'lateral{i}_wgrad'] = dict(rate(flop, t[f'lateral{i}_wgrad']), **traffic(4 * px * (c + 256 * chunks), t[f'lateral{i}_wgrad']))
        if i + 1 < len(used):
            hc, wc = used[i + 1][1]
            kern[f'topdown{i}'] = dict(ms=t[f'topdown{i}'], **traffic(4 * n * 256 * (h * w + 2 * hc * wc), t[f'topdown{i}']))
    conv_px = n * sum(h * w for _, (h, w) in used[:nconv])
    kern['conv3x3_dgrad'] = dict(rate(2 * 2304 * 256 * conv_px, t['conv3x3_dgrad']), pixels=conv_px)
    kern['conv3x3_wgrad'] = dict(rate(2 * 2304 * 256 * conv_px, t['conv3x3_wgrad']), launches=nconv)
    kern['conv3x3_bias'] = {'ms': t['conv3x3_bias'], 'launches': nconv}
    for k in ('extra_dgrad', 'extra_wgrad'):
        if k in t:
            kern[k] = {'ms': t[k]}
    out['kernels'] = kern
    out['slowest_kernel'] = max(kern, key=lambda k: kern[k]['ms'])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--cams', type=int, nargs='+', default=[24, 12])
    ap.add_argument('--hip-only', action='store_true')
    ap.add_argument('--train', action='store_true', help='forward + backward: hip_train=True beside torch_ops=True')
    a = ap.parse_args()
    if a.train:
        res = {'metric': 'neck forward + backward ms per sample (B = 1), hip_train=True against the module\'s torch-op route'}
        for n in a.cams:
            res[f'r50_fpn_cams{n}'] = train_workload(R50, n, a.reps)
        res[f'vov_cpfpn_cams{a.cams[0]}'] = train_workload(VOV, a.cams[0], a.reps)
        print(json.dumps(res))
        return
    res = {'metric': 'neck forward ms per sample (B = 1), kernels against the module\'s torch-op route'}
    for n in a.cams:
        res[f'r50_fpn_cams{n}'] = workload(R50, n, a.reps, a.hip_only)
    res[f'vov_cpfpn_cams{a.cams[0]}'] = workload(VOV, a.cams[0], a.reps, a.hip_only)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
