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

    python tools/bench_petr_head.py --train [--keys 6000,12000,48000] [--kinds PETRHead,PETRv2Head]

--train: forward + backward, one child process per (kind, key count), eval mode with autograd on (no dropout, with_cp inactive - the
setting of the gradient tests), the variants' windows alternating in one process as above:
  head_hip / head_torch_ops      a whole head call and the backward of sum(outputs G), hip_train=True beside torch_ops=True of the same
                                 commit (the same parameters)
  keys_hip / keys_torch_ops      the key side alone: autograd.PetrKeysFunction and its backward from fixed dmemory / dkey_pos, beside the
                                 reference's op sequence for the same two tensors on torch (input_proj, position_embeding, the gate,
                                 adapt_pos3d over the sine encoding, the two permute copies)
  pe_wgrad / pe_wgrad_composed   position_encoder's weight gradients alone: gd4d_mlp2_wgrad with the frustum generated, beside the
                                 kernels the library had before - ops.frustum_pe_input_fwd, two ops.gemm_bf16x3_fwd (one masked), two
                                 ops.gemm_tn_bf16x3
  adapt_wgrad                    gd4d_mlp2_wgrad over the (rows, 384) sine expansion
peak_bytes_*: torch.cuda.max_memory_allocated over one forward + backward of each head route, above what was allocated before it.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
SHAPES = {6000: (20, 50), 12000: (25, 80), 24000: (40, 100), 48000: (80, 100)}          # per camera, 6 cameras
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


def bench_train(keys, kind, rounds, window_ms):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import graph_detr4d_amd as G
    from bench_cross_mha import windows
    from graph_detr4d_amd import ops, synthetic
    from graph_detr4d_amd import petr_head as PH
    from graph_detr4d_amd.autograd import PetrKeysFunction
    from graph_detr4d_amd.petr_transformer import PETRTransformer
    dev, n = 'cuda', 6
    h, w = SHAPES[keys]
    s = h * w
    pad_hw = (16 * h, 16 * w)
    torch.manual_seed(keys)
    v1 = dict(type='PETRHead', with_fpe=False, with_time=False, with_multi=False) if kind == 'PETRHead' else {}
    cfg = {k: v for k, v in head_config(**v1).items() if kind != 'PETRHead' or k not in ('with_fpe', 'with_time', 'with_multi')}
    hip = G.build_head(dict(cfg, hip_train=True)).to(dev).eval()
    hip.init_weights()
    ref = G.build_head(dict(cfg, torch_ops=True)).to(dev).eval()
    ref.load_state_dict(hip.state_dict())
    l2i = np.asarray(synthetic.camera_rig(num_frames=1, img_hw=pad_hw), dtype=np.float64)
    metas = [dict(lidar2img=[l2i[i] for i in range(n)], img_shape=[(pad_hw[0], pad_hw[1], 3)] * n, pad_shape=[(pad_hw[0], pad_hw[1], 3)] * n,
                  timestamp=[0.0] * 6 + [0.5] * 6)]
    feat = torch.randn(1, n, 256, h, w, device=dev, requires_grad=True)
    gm, gk = torch.randn(n * s, 1, 256, device=dev), torch.randn(n * s, 1, 256, device=dev)
    weights = {}

    def step(head):
        for p in head.parameters():
            p.grad = None
        feat.grad = None
        outs = head([feat], metas)
        if not weights:
            weights.update({k: torch.randn_like(outs[k]) for k in ('all_cls_scores', 'all_bbox_preds')})
        sum((outs[k] * weights[k]).sum() for k in weights).backward()
        return outs

    def keys_hip():
        feat.grad = None
        pe = hip._helper()
        masks, _ = pe.padding_masks(metas, [feat])
        ip_image, ip_scale = hip._input_proj_image()
        img = hip._images()
        conv = hip.input_proj
        geom = dict(i2l=pe._matrices_device(pe._img2lidar(metas), feat.device).clone(), pad_hw=pad_hw, depth_num=64, depth_start=hip.depth_start,
                    position_range=POSITION_RANGE, xs=hip._sine_expansion(masks), ip_image=ip_image, ip_scale=ip_scale, pe_image=img['pe'],
                    se_image=img['se'], ip_image_t=lambda: hip._keep('input_proj_t', [conv.weight], lambda: ops.fpn_lateral_image_t(conv.weight.detach())))
        seqs = [hip.position_encoder, hip.adapt_pos3d] + ([(hip.fpe.conv_reduce, None, hip.fpe.conv_expand)] if hip.with_fpe else [])
        params = [conv.weight, conv.bias] + [p for q in seqs for c in (q[0], q[2]) for p in (c.weight, c.bias)]
        params += [None] * (14 - len(params))
        memory, key_pos = PetrKeysFunction.apply(feat, geom, *params)
        torch.autograd.backward([memory, key_pos], [gm, gk])
        return memory, key_pos

    def keys_torch():
        feat.grad = None
        x = ref.input_proj(feat.flatten(0, 1)).view(1, n, 256, h, w)
        masks = torch.zeros(1, n, h, w, dtype=torch.bool, device=dev)
        sin_embed = PH._sine_encoding(masks, ref.positional_encoding)
        pos_embed, _ = ref.position_embeding([feat], metas, masks)
        if ref.with_fpe:
            pos_embed = (pos_embed.flatten(0, 1) * ref.fpe.gate_logits(x.flatten(0, 1)).sigmoid()).view(x.size())
        pos_embed = pos_embed + ref.adapt_pos3d(sin_embed.flatten(0, 1)).view(x.size())
        memory, key_pos = PETRTransformer._camera_pixels_first(x), PETRTransformer._camera_pixels_first(pos_embed)
        torch.autograd.backward([memory, key_pos], [gm, gk])
        return memory, key_pos

    pe0, pe2 = hip.position_encoder[0], hip.position_encoder[2]
    a0, a2 = hip.adapt_pos3d[0], hip.adapt_pos3d[2]
    flat = lambda c: c.weight.detach().view(c.out_channels, c.in_channels).contiguous()      # noqa: E731
    i2l = hip._helper()._matrices_device(hip._helper()._img2lidar(metas), feat.device)
    dy = torch.randn(n * s, 256, device=dev)
    w0, w2 = flat(pe0), flat(pe2)
    frustum = (i2l, (h, w), pad_hw, 64, hip.depth_start, POSITION_RANGE)
    with torch.no_grad():
        masks, _ = hip._helper().padding_masks(metas, [feat])
        xs = hip._sine_expansion(masks).view(n * s, 384)

    def pe_wgrad():
        return ops.mlp2_wgrad(dy, w0, pe0.bias.detach(), w2, frustum=frustum)

    def pe_wgrad_composed():                                # the parent's kernels: what it takes without gd4d_mlp2_wgrad
        fr = torch.empty(n, s, 192, device=dev)
        ops.frustum_pe_input_fwd(i2l, (h, w), pad_hw, 64, hip.depth_start, POSITION_RANGE, out=fr)
        x = fr.view(n * s, 192)
        hid = ops.gemm_bf16x3_fwd(x, *ops.split_bf16_fwd(w0), pe0.bias.detach(), relu=True)
        dw2, db2 = ops.gemm_tn_bf16x3(dy, hid)
        ops.gemm_bf16x3_fwd(dy, *ops.split_bf16_fwd(w2.t().contiguous()), out=hid, mask_out=True)
        dw1, db1 = ops.gemm_tn_bf16x3(hid, x)
        return dw2, db2, dw1, db1

    fns = {'head_hip': lambda: step(hip), 'head_torch_ops': lambda: step(ref), 'keys_hip': keys_hip, 'keys_torch_ops': keys_torch,
           'pe_wgrad': pe_wgrad, 'pe_wgrad_composed': pe_wgrad_composed,
           'adapt_wgrad': lambda: ops.mlp2_wgrad(dy, flat(a0), a0.bias.detach(), flat(a2), x=xs)}
    res = windows(fns, rounds, window_ms)
    peak = {}
    for name, head in (('hip', hip), ('torch_ops', ref)):
        step(head)
        torch.cuda.synchronize()
        for p in head.parameters():
            p.grad = None
        feat.grad = None
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        step(head)
        torch.cuda.synchronize()
        peak[name] = int(torch.cuda.max_memory_allocated() - before)
    a, b = step(hip), step(ref)
    ga = {k: p.grad.clone() for k, p in hip.named_parameters() if p.grad is not None}
    step(ref)
    gb = {k: p.grad for k, p in ref.named_parameters() if p.grad is not None}
    key_side = ('input_proj.', 'position_encoder.', 'adapt_pos3d.', 'fpe.')      # (weights: a last bias's gradient can be zero identically)
    fro = max(float((ga[k] - gb[k]).norm() / gb[k].norm()) for k in gb if k.startswith(key_side) and k.endswith('weight'))
    g1, g2 = pe_wgrad(), pe_wgrad_composed()
    out = dict(device=torch.cuda.get_device_name(0), mode='train', kind=kind, keys=keys, cameras=n, h=h, w=w, rounds=rounds, window_ms=window_ms,
               variants=res, peak_bytes_hip=peak['hip'], peak_bytes_torch_ops=peak['torch_ops'],
               max_abs_diff_head_cls_vs_torch_ops=float((a['all_cls_scores'] - b['all_cls_scores']).detach().abs().max()),
               worst_rel_fro_key_side_weight_grad_vs_torch_ops=fro,
               max_rel_diff_pe_wgrad_vs_composed=max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(g1, g2)),
               head_hip_over_torch_ops=res['head_hip']['median_us'] / res['head_torch_ops']['median_us'],
               keys_hip_over_torch_ops=res['keys_hip']['median_us'] / res['keys_torch_ops']['median_us'],
               pe_wgrad_over_composed=res['pe_wgrad']['median_us'] / res['pe_wgrad_composed']['median_us'])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--keys', default='')
    ap.add_argument('--train', action='store_true', help='forward + backward: hip_train=True beside torch_ops=True (see the docstring)')
    ap.add_argument('--kinds', default='PETRHead,PETRv2Head', help='--train: the head classes to measure')
    ap.add_argument('--kind', default='PETRv2Head', help='--train --one: the head class of this process')
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
        if args.train:
            print(json.dumps(bench_train(args.one, args.kind, args.rounds, args.window_ms)), flush=True)
        else:
            print(json.dumps(bench(args.one, args.rounds, args.window_ms)), flush=True)
        return
    key_list = args.keys or ('6000,12000,48000' if args.train else '6000,12000,24000')
    for kind in (args.kinds.split(',') if args.train else [None]):
        for keys in key_list.split(','):
            cmd = [sys.executable, os.path.abspath(__file__), '--one', keys, '--rounds', str(args.rounds), '--window-ms', str(args.window_ms)]
            if args.train:
                cmd += ['--train', '--kind', kind]
            try:
                rc = subprocess.run(cmd, cwd=ROOT, timeout=args.timeout).returncode
            except subprocess.TimeoutExpired:
                raise SystemExit(f'keys = {keys}: no result within {args.timeout} s - stopping here')
            if rc != 0:
                raise SystemExit(f'keys = {keys}: exit status {rc} - stopping here')


if __name__ == '__main__':
    main()
