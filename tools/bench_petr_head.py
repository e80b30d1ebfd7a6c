#!/usr/bin/env python
"""GPU time of the key side of PETRv2Head (6 cameras, 6 000 - 24 000 keys, batch 1) on gd4d_petr_keys_fwd beside the same result composed
from the kernels the library had before plus torch, and of a whole head call on the kernel route beside torch_ops=True.  Prints ONE JSON
line per key count.

    python tools/bench_petr_head.py [--keys 6000,12000,24000] [--rounds 7] [--window-ms 100] [--timeout 240]
    python tools/bench_petr_head.py --one 12000 ...      one key count in this process (what the driver starts)

Without --one the script is a driver that has not touched the GPU: it starts one fresh child process per key count, each under its
own time limit (--timeout seconds), and stops at the first child that fails or runs out of time.

Variants, their windows interleaved in one process (tools/bench_cross_mha.py's windows: k consecutive calls between two device events,
k sized so that a window lasts --window-ms; median, min and max over --rounds windows, microseconds per call):
  keys               gd4d_petr_keys_fwd with the gate: memory and key_pos as (n h w, 1, 256) rows
  keys_no_gate       the same without a gate image (PETRHead)
  composed           gd4d_mlp2_frustum_fwd -> (R, S, 256); the gate as two GEMMs (gd4d_value_proj_fwd over the NCHW map, gd4d_gemm_bf16x3_fwd
                     with the ReLU on its input); sigmoid, product and sum on torch; PETRTransformer._camera_pixels_first of x and of the
                     result (at batch 1 torch makes the second a view of the channels-last rows: the composed form's best case)
  composed_parts     the same, timed piece by piece (frustum, gate, fuse, copies)
  head / head_torch_ops    a whole PETRv2Head call (with_fpe, with_time, with_multi; 900 queries, the 6-layer transformer of the shipped
                     configs), kernel route and torch_ops=True, same module
`max_abs_diff_*` compares the variants' outputs at the timed size.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
SHAPES = {6000: (20, 50), 12000: (25, 80), 24000: (40, 100)}          # per camera, 6 cameras
POSITION_RANGE = [-61.2, -61.2, -10.0, 61.2, 61.2, 10.0]
PC_RANGE = [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]


def head_config(**over):
    """The head block of projects/configs/petrv2/petrv2_vovnet_gridmask_p4_800x320.py."""
    layer = dict(type='PETRTransformerDecoderLayer',
                 attn_cfgs=[dict(type='MultiheadAttention', embed_dims=256, num_heads=8, dropout=0.1),
                            dict(type='PETRMultiheadAttention', embed_dims=256, num_heads=8, dropout=0.1)],
                 feedforward_channels=2048, ffn_dropout=0.1, with_cp=True,
                 operation_order=('self_attn', 'norm', 'cross_attn', 'norm', 'ffn', 'norm'))
    cfg = dict(type='PETRv2Head', num_classes=10, in_channels=256, num_query=900, LID=True, with_position=True, with_multiview=True,
               with_fpe=True, with_time=True, with_multi=True, position_range=POSITION_RANGE, normedlinear=False,
               transformer=dict(type='PETRTransformer', decoder=dict(type='PETRTransformerDecoder', return_intermediate=True, num_layers=6,
                                                                     transformerlayers=layer)),
               bbox_coder=dict(type='NMSFreeCoder', post_center_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0], pc_range=PC_RANGE, max_num=300,
                               voxel_size=[0.2, 0.2, 8], num_classes=10),
               positional_encoding=dict(type='SinePositionalEncoding3D', num_feats=128, normalize=True), train_cfg=None)
    cfg.update(over)
    return cfg


def bench(keys, rounds, window_ms):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import graph_detr4d_amd as G
    from bench_cross_mha import windows
    from graph_detr4d_amd import ops, synthetic
    from graph_detr4d_amd.petr_transformer import PETRTransformer
    dev, n = 'cuda', 6
    h, w = SHAPES[keys]
    s = h * w
    pad_hw = (16 * h, 16 * w)
    torch.manual_seed(keys)
    head = G.build_head(head_config()).to(dev).eval()
    head.init_weights()
    l2i = np.asarray(synthetic.camera_rig(num_frames=1, img_hw=pad_hw), dtype=np.float64)
    metas = [dict(lidar2img=[l2i[i] for i in range(n)], img_shape=[(pad_hw[0], pad_hw[1], 3)] * n, pad_shape=[(pad_hw[0], pad_hw[1], 3)] * n,
                  timestamp=[0.0] * 6 + [0.5] * 6)]
    feat = torch.randn(1, n, 256, h, w, device=dev)
    with torch.no_grad():
        x = head._input_proj(feat)
        pe = head._helper()
        masks, _ = pe.padding_masks(metas, [feat])
        sine = pe._sine_branch(masks, chlast=True)
        img = head._images()
        i2l = pe._matrices_device(pe._img2lidar(metas), torch.device(dev, torch.cuda.current_device()))
        pe2b, cr, ce = head.position_encoder[2].bias, head.fpe.conv_reduce, head.fpe.conv_expand
        memory = torch.empty(n * s, 1, 256, device=dev)
        key_pos = torch.empty(n * s, 1, 256, device=dev)
        wr = cr.weight.view(256, 256).contiguous()
        we = ops.split_bf16_fwd(ce.weight.view(256, 256).contiguous())
        xf = x.flatten(0, 1).contiguous()
        bufs = {}

        def frustum():
            bufs['pe'] = ops.mlp2_frustum_fwd(i2l, [(h, w)], pad_hw, 64, 1, POSITION_RANGE, img['pe'], pe2b)

        def gate():
            g1 = ops.value_proj_fwd([xf], wr, cr.bias.contiguous())
            bufs['gate'] = ops.gemm_bf16x3_fwd(g1.view(n * s, -1), *we, ce.bias, relu_in=True).view(n, s, 256)

        def fuse():
            bufs['pos'] = bufs['pe'] * torch.sigmoid(bufs['gate']) + sine

        def copies():
            bufs['memory'] = PETRTransformer._camera_pixels_first(x)
            bufs['key_pos'] = PETRTransformer._camera_pixels_first(bufs['pos'].view(1, n, h, w, 256).permute(0, 1, 4, 2, 3))

        def composed():
            frustum(), gate(), fuse(), copies()
        fns = {'keys': lambda: ops.petr_keys_fwd(x, i2l, pad_hw, 64, 1, POSITION_RANGE, img['pe'], pe2b, sine, img['se'], ce.bias,
                                                 memory=memory, key_pos=key_pos),
               'keys_no_gate': lambda: ops.petr_keys_fwd(x, i2l, pad_hw, 64, 1, POSITION_RANGE, img['pe'], pe2b, sine, memory=memory,
                                                         key_pos=key_pos),
               'composed': composed, 'composed_frustum': frustum, 'composed_gate': gate, 'composed_fuse': fuse, 'composed_copies': copies}

        def call(torch_ops):
            head.torch_ops = torch_ops
            try:
                return head([feat], metas)
            finally:
                head.torch_ops = False
        fns['head'] = lambda: call(False)
        fns['head_torch_ops'] = lambda: call(True)
        composed()
        res = windows(fns, rounds, window_ms)
        fns['keys']()
        composed()
        a, b = call(False), call(True)
        out = dict(device=torch.cuda.get_device_name(0), keys=keys, cameras=n, h=h, w=w, rounds=rounds, window_ms=window_ms,
                   launch=dict(zip(('workgroups', 'rows_per_workgroup'), ops.petr_keys_plan(1, n, h, w, want_rows=False)[:2])), variants=res,
                   memory_equal=bool(torch.equal(memory, bufs['memory'])),
                   max_abs_diff_key_pos_vs_composed=float((key_pos - bufs['key_pos']).abs().max()),
                   max_abs_diff_head_cls_vs_torch_ops=float((a['all_cls_scores'] - b['all_cls_scores']).abs().max()),
                   max_abs_diff_head_box_vs_torch_ops=float((a['all_bbox_preds'] - b['all_bbox_preds']).abs().max()))
    out['keys_over_composed'] = res['keys']['median_us'] / res['composed']['median_us']
    out['head_over_torch_ops'] = res['head']['median_us'] / res['head_torch_ops']['median_us']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--keys', default='6000,12000,24000')
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--window-ms', type=float, default=100.0)
    ap.add_argument('--timeout', type=float, default=240.0, help='driver: seconds each key count\'s process may take')
    ap.add_argument('--one', type=int, default=0, help='measure this key count in this process')
    args = ap.parse_args()
    if args.one:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit('bench_petr_head.py needs a GPU: a CPU timing says nothing about the kernels')
        if args.one not in SHAPES:
            raise SystemExit(f'key counts with a shape here: {sorted(SHAPES)}')
        print(json.dumps(bench(args.one, args.rounds, args.window_ms)), flush=True)
        return
    for keys in args.keys.split(','):
        cmd = [sys.executable, os.path.abspath(__file__), '--one', keys, '--rounds', str(args.rounds), '--window-ms', str(args.window_ms)]
        try:
            rc = subprocess.run(cmd, cwd=ROOT, timeout=args.timeout).returncode
        except subprocess.TimeoutExpired:
            raise SystemExit(f'keys = {keys}: no result within {args.timeout} s - stopping here')
        if rc != 0:
            raise SystemExit(f'keys = {keys}: exit status {rc} - stopping here')


if __name__ == '__main__':
    main()
