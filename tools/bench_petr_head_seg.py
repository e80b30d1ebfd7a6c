#!/usr/bin/env python
"""GPU time of PETRHeadseg at the size of projects/configs/petrv2/petrv2_BEVseg.py - 12 cameras x 20 x 50 = 12 000 keys, in_channels 256,
900 + 256 queries, two 6-layer decoders, batch 1 - and of its two lane kernels beside the torch sequences they replace.  Prints ONE
JSON line.

    python tools/bench_petr_head_seg.py [--train] [--rounds 7] [--window-ms 100] [--timeout 300]
    python tools/bench_petr_head_seg.py --one ...       the measurement in this process (what the driver starts)

Without --one the script is a driver that has not touched the GPU: it starts one fresh child process under a time limit (--timeout
seconds).  The variants' windows alternate in one process (tools/bench_cross_mha.py's windows: k consecutive calls between two device
events, k sized so that a window lasts --window-ms; median, min and max over --rounds windows, microseconds per call):
  head / head_torch_ops          a whole head call in eval mode without autograd, kernel route beside torch_ops=True of the same module
  lane_map / lane_map_torch      gd4d_lane_map_fwd with a ground-truth map (one launch) beside the reference's sequence on torch
                                 (view, permute, sigmoid, two masked assignments, the IoU's products and sums)
--train adds (eval mode with autograd on: no dropout, with_cp inactive - the setting of the gradient tests):
  step_hip / step_torch_ops      forward, loss() and backward of the sum of its terms, hip_train=True beside torch_ops=True of the same
                                 commit and parameters
  lane_loss / lane_loss_torch    Sigmoid_ce_loss over the six layers' (256, 768) logits, forward + backward: ONE gd4d_lane_mask_loss call
                                 (three launches) and the scaling of its gradient, beside the torch formula per layer with nan_to_num
                                 and autograd's backward
`max_abs_diff_*` / `max_rel_diff_*` compare the variants' results at the timed size.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
CAMERAS, H, W, NUM_LANE = 12, 20, 50, 256
POSITION_RANGE = [-61.2, -61.2, -10.0, 61.2, 61.2, 10.0]
PC_RANGE = [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]


def head_config(**over):
    """The head block of projects/configs/petrv2/petrv2_BEVseg.py:40-125."""
    layer = dict(type='PETRTransformerDecoderLayer',
                 attn_cfgs=[dict(type='MultiheadAttention', embed_dims=256, num_heads=8, dropout=0.1),
                            dict(type='PETRMultiheadAttention', embed_dims=256, num_heads=8, dropout=0.1)],
                 feedforward_channels=2048, ffn_dropout=0.1, with_cp=True,
                 operation_order=('self_attn', 'norm', 'cross_attn', 'norm', 'ffn', 'norm'))
    transformer = dict(type='PETRTransformer', decoder=dict(type='PETRTransformerDecoder', return_intermediate=True, num_layers=6,
                                                            transformerlayers=layer))
    assigner = dict(type='HungarianAssigner3D', cls_cost=dict(type='FocalLossCost', weight=2.0), reg_cost=dict(type='BBox3DL1Cost', weight=0.25),
                    iou_cost=dict(type='IoUCost', weight=0.0), pc_range=PC_RANGE)
    cfg = dict(type='PETRHeadseg', num_classes=10, in_channels=256, num_query=900, num_lane=NUM_LANE, LID=True, with_position=True,
               with_multiview=True, with_se=True, with_time=True, with_multi=True, position_range=POSITION_RANGE, normedlinear=False,
               transformer=transformer, transformer_lane=transformer,
               bbox_coder=dict(type='NMSFreeCoder', post_center_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0], pc_range=PC_RANGE, max_num=300,
                               voxel_size=[0.2, 0.2, 8], num_classes=10),
               positional_encoding=dict(type='SinePositionalEncoding3D', num_feats=128, normalize=True),
               loss_cls=dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=2.0),
               loss_bbox=dict(type='L1Loss', loss_weight=0.25), loss_iou=dict(type='GIoULoss', loss_weight=0.0),
               loss_lane_mask=dict(type='Sigmoid_ce_loss', loss_weight=1.0), train_cfg=dict(pts=dict(assigner=assigner)))
    cfg.update(over)
    return cfg


def bench(train, rounds, window_ms):
    import numpy as np
    import torch
    import torch.nn.functional as F
    sys.path.insert(0, ROOT)
    import graph_detr4d_amd as G
    from bench_cross_mha import windows
    from graph_detr4d_amd import ops, synthetic
    dev, n, g = 'cuda', CAMERAS, 16
    pad_hw = (16 * H, 16 * W)
    torch.manual_seed(12000)
    head = G.build_head(head_config(hip_train=train)).to(dev).eval()
    head.init_weights()
    rig = np.asarray(synthetic.camera_rig(num_frames=2, img_hw=pad_hw), dtype=np.float64)[:n]
    metas = [dict(lidar2img=[rig[i] for i in range(n)], img_shape=[(pad_hw[0], pad_hw[1], 3)] * n, pad_shape=[(pad_hw[0], pad_hw[1], 3)] * n,
                  timestamp=[0.0] * 6 + [0.5] * 6)]
    feat = torch.randn(1, n, 256, H, W, device=dev, requires_grad=train)
    gt_map = (torch.rand(1, 3, 16 * g, 16 * g, device=dev) < 0.3).float()
    target = (torch.rand(NUM_LANE, 768, device=dev) < 0.1).float()
    logits = torch.randn(6, NUM_LANE, 768, device=dev)

    def call(torch_ops):
        head.torch_ops = torch_ops
        try:
            with torch.no_grad():
                return head([feat], metas)
        finally:
            head.torch_ops = False

    def lane_map_torch(x=logits[-1:]):
        f_lane = x.view(1, g, g, 3, 16, 16).permute(0, 3, 1, 4, 2, 5).reshape(1, 3, 16 * g, 16 * g).sigmoid()
        f_lane[f_lane >= 0.5] = 1
        f_lane[f_lane < 0.5] = 0
        p, t = f_lane.flatten(2), gt_map.flatten(2)
        return f_lane, (2 * (p * t).sum(dim=2) + 0.01) / (p.sum(dim=2) + t.sum(dim=2) + 0.01)

    fns = {'head': lambda: call(False), 'head_torch_ops': lambda: call(True),
           'lane_map': lambda: ops.lane_map_fwd(logits[-1:], gt_map), 'lane_map_torch': lane_map_torch}
    out = dict(device=torch.cuda.get_device_name(0), mode='train' if train else 'eval', keys=n * H * W, cameras=n, h=H, w=W, num_query=900,
               num_lane=NUM_LANE, rounds=rounds, window_ms=window_ms)
    if train:
        ref = G.build_head(head_config(torch_ops=True)).to(dev).eval()
        ref.load_state_dict(head.state_dict())
        boxes = torch.randn(30, 9, device=dev)
        boxes[:, 0:2] *= 30.
        boxes[:, 3:6] = boxes[:, 3:6].abs() * 2 + 0.3
        labels = torch.randint(0, 10, (30,), device=dev)

        def step(h):
            for p in h.parameters():
                p.grad = None
            feat.grad = None
            outs = h([feat], metas)
            losses = h.loss([boxes], [labels], outs, [target])
            sum(losses.values()).backward()
            return outs, losses
        lg = logits.clone().requires_grad_(True)
        crit = head.loss_lane_mask

        def lane_loss():
            lg.grad = None
            loss = crit.layers(lg, target)
            loss.sum().backward()
            return loss

        def lane_loss_torch():
            lg.grad = None
            pos_weight = (target == 0).float().sum(dim=1) / (target == 1).float().sum(dim=1).clamp(min=1.0)
            loss = []
            for x in lg:                                     # per layer, as loss_single does it (petr_head_seg.py:782-785)
                weight = target * pos_weight.unsqueeze(1) + (1 - target)
                loss.append(torch.nan_to_num(F.binary_cross_entropy_with_logits(x, target, reduction='mean', weight=weight)))
            loss = torch.stack(loss)
            loss.sum().backward()
            return loss
        fns.update({'step_hip': lambda: step(head), 'step_torch_ops': lambda: step(ref), 'lane_loss': lane_loss,
                    'lane_loss_torch': lane_loss_torch})
    res = windows(fns, rounds, window_ms)
    a, b = call(False), call(True)
    m, mt = ops.lane_map_fwd(logits[-1:], gt_map), lane_map_torch()
    out.update(variants=res, head_over_torch_ops=res['head']['median_us'] / res['head_torch_ops']['median_us'],
               lane_map_over_torch=res['lane_map']['median_us'] / res['lane_map_torch']['median_us'],
               max_abs_diff_head_cls_vs_torch_ops=float((a['all_cls_scores'] - b['all_cls_scores']).abs().max()),
               max_abs_diff_head_lane_vs_torch_ops=float((a['all_lane_preds'] - b['all_lane_preds']).abs().max()),
               lane_map_binary_equal=bool(torch.equal(m[1], mt[0])), max_abs_diff_lane_map_iou=float((m[3] - mt[1]).abs().max()))
    if train:
        la = lane_loss().detach().clone()
        ga = lg.grad.clone()
        lb = lane_loss_torch().detach()
        (_, l_hip), (_, l_ref) = step(head), step(ref)
        out.update(step_hip_over_torch_ops=res['step_hip']['median_us'] / res['step_torch_ops']['median_us'],
                   lane_loss_over_torch=res['lane_loss']['median_us'] / res['lane_loss_torch']['median_us'],
                   max_rel_diff_lane_loss=float(((la - lb).abs() / lb.abs()).max()),
                   max_rel_diff_lane_loss_grad=float((ga - lg.grad).abs().max() / lg.grad.abs().max()),
                   max_rel_diff_step_losses=max(float((l_hip[k] - l_ref[k]).abs() / l_ref[k].abs().clamp(min=1e-12)) for k in l_ref))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--train', action='store_true', help='add forward + loss + backward: hip_train=True beside torch_ops=True, and the lane loss')
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--window-ms', type=float, default=100.0)
    ap.add_argument('--timeout', type=float, default=300.0, help='driver: seconds the measuring process may take')
    ap.add_argument('--one', action='store_true', help='measure in this process')
    args = ap.parse_args()
    if args.one:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit('bench_petr_head_seg.py needs a GPU: a CPU timing says nothing about the kernels')
        print(json.dumps(bench(args.train, args.rounds, args.window_ms)), flush=True)
        return
    cmd = [sys.executable, os.path.abspath(__file__), '--one', '--rounds', str(args.rounds), '--window-ms', str(args.window_ms)]
    cmd += ['--train'] if args.train else []
    try:
        rc = subprocess.run(cmd, cwd=ROOT, timeout=args.timeout).returncode
    except subprocess.TimeoutExpired:
        raise SystemExit(f'no result within {args.timeout} s')
    if rc != 0:
        raise SystemExit(f'exit status {rc}')


if __name__ == '__main__':
    main()
