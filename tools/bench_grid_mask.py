"""Times GridMask at the two image sizes of the configs - 24 x 3 x 320 x 800 and 24 x 3 x 900 x 1600 -, fp32 -> fp32 and fp32 -> fp16,
on three routes that alternate call by call: the eager HIP route (host draws, one kernel), the device-draw route (draw kernel + apply
kernel, nothing from the host) and the torch-op route (the reference's op sequence: host mask, PIL, upload, multiply - the yardstick).
The detector's module (use_h, use_w, mode 1, ratio 0.5) with prob = 1, so every call applies a mask.  Per call: hipEvents around it
(device time) and the host's wall time from issue to return (the torch-op route's cost is mostly there); medians.  The bytes the kernel
must move are the kept elements read once plus every element written once; the kept share is counted from an output.
One JSON line per (size, out dtype, route).

  python tools/bench_grid_mask.py [--steps 30] [--warmup 5] [--sizes 320x800 900x1600]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--cams', type=int, default=24)
    ap.add_argument('--sizes', nargs='+', default=['320x800', '900x1600'])
    args = ap.parse_args()
    from graph_detr4d_amd import GridMask
    dev = 'cuda:0'
    for size in args.sizes:
        h, w = (int(v) for v in size.split('x'))
        x = (torch.rand(args.cams, 3, h, w, generator=torch.Generator().manual_seed(0)) + 0.25).to(dev)
        for out_dtype in (None, torch.float16):
            kw = dict(rotate=1, offset=False, ratio=0.5, mode=1, prob=1.0, out_dtype=out_dtype)
            routes = dict(hip_eager=GridMask(True, True, **kw).train(),
                          hip_device_draw=GridMask(True, True, **kw).device_draw(1234).train(),
                          torch_ops=GridMask(True, True, torch_ops=True, **kw).train())
            dev_ms, host_ms, kept = {k: [] for k in routes}, {k: [] for k in routes}, {k: [] for k in routes}
            np.random.seed(0)
            for it in range(args.warmup + args.steps):
                for name, mod in routes.items():
                    torch.cuda.synchronize()
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0 = time.perf_counter()
                    a.record()
                    y = mod(x)
                    b.record()
                    t1 = time.perf_counter()
                    b.synchronize()
                    if it >= args.warmup:
                        dev_ms[name].append(a.elapsed_time(b))
                        host_ms[name].append((t1 - t0) * 1e3)
                        if it == args.warmup:
                            kept[name].append(float((y != 0).float().mean()))
                    del y
            so = 4 if out_dtype is None else 2
            for name in routes:
                med = statistics.median(dev_ms[name])
                must = x.numel() * (4 * kept[name][0] + so)
                print(json.dumps(dict(bench='grid_mask', size=size, planes=args.cams * 3, out='fp32' if out_dtype is None else 'fp16', route=name,
                                      device_median_ms=round(med, 4), device_min_ms=round(min(dev_ms[name]), 4),
                                      host_median_ms=round(statistics.median(host_ms[name]), 4), kept_share=round(kept[name][0], 3),
                                      must_move_mb=round(must / 1e6, 1), tb_per_s=round(must / (med * 1e-3) / 1e12, 3), steps=args.steps,
                                      warmup=args.warmup)), flush=True)


if __name__ == '__main__':
    main()
