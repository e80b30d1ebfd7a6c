"""Host time of an eager decoder request, three ways, in one process: the Python loop (GD4D_REQUEST=0, what every caller gets
today), the request program (GD4D_REQUEST=1: one gd4d_decoder_request_run per request) and the hipGraph replay (the floor: no
host work per launch at all).  bench.py's default workload - 6 layers, 900 queries, 24 cameras, R50 pyramid, fp32, one request at
a time on one stream.

The quantity is host-bound, so a window is wall clock around N requests with ONE synchronisation at its end; the two eager routes
alternate window by window (neighbours on the box disturb both alike) and the figure of a route is the median of its windows, with
min / max.  `host_us` is the enqueue alone (the same loop without the closing synchronise in the timed part); `parts_us` splits
the program route's per-request host work.

    python tools/bench_request.py [--samples 200] [--windows 7] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def window(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return (t2 - t0) / n * 1e3, (t1 - t0) / n * 1e6          # ms per request (synchronised), host us per request (enqueue)


def summary(xs):
    return {'median': statistics.median(xs), 'min': min(xs), 'max': max(xs), 'windows': len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--samples', type=int, default=200, help='requests per window')
    ap.add_argument('--windows', type=int, default=7, help='windows per route (>= 5)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import bench
    import graph_detr4d_amd as G
    from graph_detr4d_amd import functional as Fn
    from graph_detr4d_amd import fused_decoder, ops, synthetic
    dev = torch.device('cuda', 0)
    tr, regs = bench.build_decoder(G, 24, 6, 'fp32', 1002)
    tr, regs = tr.to(dev), regs.to(dev)
    feats = [f.to(dev) for f in synthetic.feature_pyramid(24, synthetic.R50_LEVELS, seed=1002)]
    qe = torch.randn(900, 512, generator=torch.Generator().manual_seed(1005)).to(dev)
    metas = synthetic.make_img_metas(synthetic.camera_rig(4), batch=1)
    stream = torch.cuda.Stream(dev)

    def request():
        return tr(feats, qe, reg_branches=regs, img_metas=metas)

    def route(on):
        os.environ['GD4D_REQUEST'] = '1' if on else '0'

    with torch.no_grad(), torch.cuda.stream(stream), Fn.request_slot(0):
        route(False)
        want = request()
        route(True)
        got = request()
        torch.cuda.synchronize()
        assert torch.equal(want[0], got[0]) and torch.equal(want[2], got[2]), 'the two routes disagree'
        route(False)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream, capture_error_mode='thread_local'):
            static = request()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static[0], want[0])
        for on in (False, True):                                  # warm-up of everything a window touches
            route(on)
            window(request, 20)
        window(graph.replay, 20)
        ms = {'off': [], 'on': [], 'graph': []}
        host = {'off': [], 'on': [], 'graph': []}
        for _ in range(max(5, a.windows)):
            for name, on, fn in (('off', False, request), ('on', True, request), ('graph', False, graph.replay)):
                route(on)
                m, h = window(fn, a.samples)
                ms[name].append(m)
                host[name].append(h)
        ops.check_handoff()
        # where the program route's host time goes
        route(True)
        request()
        prog = [p for p in fused_decoder._PROGRAMS[tr.decoder].values() if p.valid(regs)][-1]
        query_pos, query = torch.split(qe, 256, dim=1)

        def clock(fn, n=2000):
            t0 = time.perf_counter()
            for _ in range(n):
                fn()
            return (time.perf_counter() - t0) / n * 1e6
        parts = {
            'stamp_check': clock(lambda: prog.valid(regs)),
            'lidar2img_device': clock(lambda: Fn.lidar2img_device(metas, qe)),
            'two_output_allocations': clock(lambda: (torch.empty(prog.out_shape, device=dev), torch.empty(prog.ref_shape, device=dev))),
            'applicable_checks': clock(lambda: fused_decoder.takes_single_stream_loop(
                tr.decoder, query.unsqueeze(1), feats, query_pos[None, :, :3], regs, None, query_pos.unsqueeze(1))),
            'request_covers_whole': clock(lambda: fused_decoder.request_covers(
                tr.decoder, query.unsqueeze(1), None, regs, dict(key=None, value=feats, query_pos=query_pos.unsqueeze(1), img_metas=metas))),
            'late_values_applicable': clock(lambda: Fn.LateValues.applicable([l.attentions[1] for l in tr.decoder.layers], feats)),
            'img_hw': clock(lambda: Fn.img_hw(metas)),
            'initial_reference_launch': clock(lambda: fused_decoder.initial_reference(tr.reference_points, query_pos), 200),
        }
        torch.cuda.synchronize()
        t_run = clock(lambda: prog.run(query.unsqueeze(1), query_pos.unsqueeze(1), want[1], feats, metas, None), 200)
        torch.cuda.synchronize()
        parts['program_run_whole'] = t_run
    res = {
        'workload': '6 layers, 900 queries, 24 cameras, R50 pyramid, fp32, one request at a time',
        'samples_per_window': a.samples,
        'eager_ms_per_sample': {k: summary(v) for k, v in ms.items()},
        'host_us_per_sample': {k: summary(v) for k, v in host.items()},
        'steps_in_program': prog.nsteps,
        'parts_us': parts,
        'gain_ms': statistics.median(ms['off']) - statistics.median(ms['on']),
        'switch_off_spread_ms': max(ms['off']) - min(ms['off']),
        'gap_to_graph_ms': statistics.median(ms['on']) - statistics.median(ms['graph']),
    }
    res['accepted'] = res['gain_ms'] > res['switch_off_spread_ms']
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
