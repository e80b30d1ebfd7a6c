#!/usr/bin/env python
"""GPU time of the camera-aware DepthNet (graph_detr4d_amd.DepthNet.forward_levels: gd4d_cam_gate_fwd + ONE gd4d_depth_conv_fwd
launch) at the bench's R50 pyramid, 24 and 12 cameras, beside the module's torch-op route (nn.Conv2d / BatchNorm2d / MLP / SE, the
reference arithmetic) on the same GPU and inputs, the two routes alternated in the same run; and the camera-aware head's whole
feature stage (DepthNet + FeaturePositionEmbedding(channels_last_out=True)).  Prints ONE JSON line.

    python tools/bench_depth_net.py [--reps 20] [--hip-only]
    python tools/bench_depth_net.py --train [--reps 10] [--hip-only]

--train: forward + backward of forward_levels in train() mode (loss = sum of the outputs times fixed random tensors; gradients to
every parameter and to the input maps) at 12 and 24 cameras, `hip_train=True` against `torch_ops=True` (the only training route
without it), alternated call by call on the same inputs; also each route's peak memory above what is resident before the call
(torch.cuda.max_memory_allocated).  The weight gradient's share of the bf16 spec is read from a kernel trace, not from here.

Timing: device events around each call, after a warm-up of every shape; medians.  FLOP counts from shapes: the convolution
needs 2 * 9 * 256 * 256 FLOP per output pixel; the kernel runs three bf16 products per multiply-add (split-bf16 x 3), so its rate of
bf16 products is 3x that, against the MI355X's 2.5 PFLOP/s dense bf16 spec.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import graph_detr4d_amd as G  # noqa: E402
from graph_detr4d_amd import synthetic  # noqa: E402

BF16_SPEC = 2.5e15
R50 = [(116, 200), (58, 100), (29, 50), (15, 25)]


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


def module(seed):
    torch.manual_seed(seed)
    mod = G.DepthNet(256, 256, 80)
    bn = mod.reduce_conv[1]
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(256) * 0.3)
        bn.running_var.copy_(0.25 + 2 * torch.rand(256))
    return mod.cuda().eval()


def metas_for(n):
    rig = synthetic.camera_rig(n // 6)
    metas = synthetic.make_img_metas(rig)
    metas[0]['intrinsics'] = list(synthetic.camera_intrinsics(n // 6, (928, 1600)))
    metas[0]['ida_mats'] = [torch.tensor([[0.48, 0., 0.], [0., 0.48, -32.], [0., 0., 1.]])]
    return metas


def train_main(a):
    res = {'metric': 'DepthNet.forward_levels forward + backward ms per sample, train() mode (B = 1, R50 pyramid)', 'levels': R50}
    for n in (12, 24):
        feats = [f.requires_grad_() for f in synthetic.feature_pyramid(n, levels=R50, device='cuda')]
        metas = metas_for(n)
        torch.manual_seed(n)
        rs = [torch.randn(f.shape[1:], device='cuda') for f in feats]
        mods = {'hip': module(0).train()}
        mods['hip'].hip_train = True
        if not a.hip_only:
            mods['torch'] = module(0).train()
            mods['torch'].torch_ops = True

        def step(mod):
            def run():
                for p in mod.parameters():
                    p.grad = None
                for f in feats:
                    f.grad = None
                outs = mod.forward_levels(feats, metas)
                sum((o[0] * r).sum() for o, r in zip(outs, rs)).backward()
            return run
        fns = {k: step(m) for k, m in mods.items()}
        t = alternate(fns, a.reps)
        pixels = n * sum(h * w for h, w in R50)
        out = {'cams': n, 'pixels': pixels, 'tflop_per_conv_pass': 2 * 9 * 256 * 256 * pixels / 1e12}
        for k, f in fns.items():
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            f()
            torch.cuda.synchronize()
            out[f'{k}_fwd_bwd_ms'] = t[k]
            out[f'{k}_peak_mib_above_resident'] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
        res[f'cams{n}'] = out
        del feats, rs, mods, fns
        torch.cuda.empty_cache()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=None)
    ap.add_argument('--train', action='store_true', help='forward + backward in train() mode: hip_train=True beside torch_ops=True')
    ap.add_argument('--hip-only', action='store_true', help='only the library\'s route (what a rocprofv3 run should see)')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_depth_net.py needs a GPU')
    if a.reps is None:
        a.reps = 10 if a.train else 20
    if a.train:
        return train_main(a)
    mod = module(0)
    res = {'metric': 'DepthNet.forward_levels ms per sample (B = 1, R50 pyramid)', 'levels': R50}
    with torch.no_grad():
        for n in (24, 12):
            feats = synthetic.feature_pyramid(n, levels=R50, device='cuda')
            metas = metas_for(n)
            pixels = n * sum(h * w for h, w in R50)
            flop = 2 * 9 * 256 * 256 * pixels

            def torch_route():
                mod.torch_ops = True
                try:
                    return mod.forward_levels(feats, metas)
                finally:
                    mod.torch_ops = False
            fns = {'hip': lambda: mod.forward_levels(feats, metas)}
            if not a.hip_only:
                fns['torch'] = torch_route
            t = alternate(fns, a.reps)
            out = {'cams': n, 'pixels': pixels, 'tflop_per_sample': flop / 1e12, 'hip_ms': t['hip'],
                   'bf16_product_pflops': 3 * flop / (t['hip'] * 1e-3) / 1e15,
                   'share_of_bf16_spec': 3 * flop / (t['hip'] * 1e-3) / BF16_SPEC}
            if 'torch' in t:
                out['torch_ops_ms'] = t['torch']
                out['torch_ops_fp32_tflops'] = flop / (t['torch'] * 1e-3) / 1e12
                hip, ref = fns['hip'](), torch_route()
                out['max_rel_diff_vs_torch_ops'] = max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(hip, ref))
            if n == 24:                                                   # the camera-aware head's whole feature stage
                fpe = G.FeaturePositionEmbedding(pc_range=synthetic.PC_RANGE, channels_last_out=True).cuda().eval()
                stage = {'hip': lambda: fpe(mod.forward_levels(feats, metas), metas)}
                if not a.hip_only:
                    stage['torch'] = lambda: fpe(torch_route(), metas)
                st = alternate(stage, a.reps)
                out['stage_depth_net_plus_pe_ms'] = st['hip']
                if 'torch' in st:
                    out['stage_torch_ops_depth_net_plus_pe_ms'] = st['torch']
                fpe_only = alternate({'pe': lambda: fpe(feats, metas)}, a.reps)
                out['pe_alone_ms'] = fpe_only['pe']
                del fpe
            res[f'cams{n}'] = out
            del feats
            torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
