#!/usr/bin/env python
"""Generate tests/golden/petr_head_seg.npz: PETRHeadseg (PETRv2's head plus the BEV map branch) and Sigmoid_ce_loss captured from the
reference itself.

    python tools/gen_golden_petr_head_seg.py      # needs the reference checkout (GD4D_REFERENCE_ROOT); never run on the GPU box

The reference's dense_heads/petr_head_seg.py and losses/Sigmoid_ce_loss.py are imported unmodified under tools/refstub.py's stand-ins
(refstub.load_petr_head_seg); what is recorded is their fp32 CPU arithmetic in eval mode.  The one thing the reference cannot do on a
box without a GPU is the `.cuda()` at petr_head_seg.py:369 (reference_points_lane): it is neutralised HERE, by making Tensor.cuda the
identity while the head is constructed, not in the reference.  Parameters come from the closed-form rule of tests/petr_head_ref.py
(lane_branches is one shared module, drawn under N = 0, like the other branches), inputs from its features / camera_matrices /
img_metas / timestamps; the config is the v2 fixture's plus num_lane=4, with_se=True, transformer_lane equal to transformer and
train_cfg=None (tests/petr_head_seg_ref.py:head_config).  Recorded (data only, no reference source):
  - keys / shapes / sums / sumsqs of the state dict;
  - x (as int16 x 512, exact), mask, pos_embed and query_embeds as the forward hook of `transformer` sees them, and the same four as
    `transformer_lane`'s hook sees them - x / mask / pos_embed must be the same tensors, the query embedding is the lane one;
  - all_cls_scores, all_bbox_preds, all_lane_preds;
  - for Sigmoid_ce_loss: loss and d loss / d inputs on the edge inputs petr_head_seg_ref.loss_case gives for FIXTURE_LOSS_SHAPES.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)
import refstub  # noqa: E402
import petr_head_ref as P  # noqa: E402
import petr_head_seg_ref as S  # noqa: E402


def build_head(cls):
    cfg = S.head_config()
    cfg.pop('type')
    real = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self             # petr_head_seg.py:369, on a box without a GPU
    try:
        head = cls(**cfg).eval()
    finally:
        torch.Tensor.cuda = real
    return cfg, head


def capture_head(seg, arrays, l2i):
    cfg, head = build_head(seg.PETRHeadseg)
    assert type(head.transformer_lane).__module__.startswith(refstub._PKG), 'the transformers must be the reference\'s own'
    assert type(head.loss_lane_mask).__name__ == 'Sigmoid_ce_loss'
    assert head.lane_branches[0] is head.lane_branches[5] and tuple(head.reference_points_lane.shape) == (S.NUM_LANE, 2)
    sd = head.state_dict()
    keys = list(sd.keys())
    assert 'reference_points_lane' not in keys and 'se.conv_reduce.weight' in keys
    with torch.no_grad():
        for k in keys:
            sd[k].copy_(S.draw(k, tuple(sd[k].shape)))
    metas = P.img_metas(l2i, P.timestamps())
    feat = P.features(cfg['in_channels'])
    seen = {}

    def recorder(tag):
        def record(mod, args, out):
            seen[tag] = dict(x=args[0].detach().clone(), mask=args[1].detach().clone(), query_embeds=args[2].detach().clone(),
                             pos_embed=args[3].detach().clone())
        return record
    hooks = [head.transformer.register_forward_hook(recorder('det')), head.transformer_lane.register_forward_hook(recorder('lane'))]
    with torch.no_grad():
        outs = head([feat.clone()], metas)
    for h in hooks:
        h.remove()
    assert outs['enc_cls_scores'] is None and outs['enc_bbox_preds'] is None
    for k in ('x', 'mask', 'pos_embed'):
        assert torch.equal(seen['det'][k], seen['lane'][k]), k
    arrays['keys'] = np.frombuffer(json.dumps(keys).encode(), dtype=np.uint8)
    arrays['shapes'] = np.frombuffer(json.dumps([list(sd[k].shape) for k in keys]).encode(), dtype=np.uint8)
    arrays['sums'] = np.asarray([float(sd[k].double().sum()) for k in keys])
    arrays['sumsqs'] = np.asarray([float((sd[k].double() ** 2).sum()) for k in keys])
    xq = np.round(seen['det']['x'].numpy().astype(np.float64) * 512)
    assert np.array_equal(xq / 512, seen['det']['x'].numpy().astype(np.float64)) and np.abs(xq).max() < 32768
    arrays['x@512'] = xq.astype(np.int16)
    arrays['mask'] = seen['det']['mask'].numpy()
    arrays['pos_embed'] = seen['det']['pos_embed'].numpy()
    arrays['query_embeds'] = seen['det']['query_embeds'].numpy()
    arrays['query_embeds_lane'] = seen['lane']['query_embeds'].numpy()
    arrays['lidar2img'] = l2i.astype(np.float32)
    arrays['timestamps'] = P.timestamps()
    for name in ('all_cls_scores', 'all_bbox_preds', 'all_lane_preds'):
        arrays[name] = outs[name].numpy()
    print(len(keys), 'tensors,', sum(v.numel() for v in sd.values()), 'parameters; |lane| <=', float(outs['all_lane_preds'].abs().max()),
          '|cls| <=', float(outs['all_cls_scores'].abs().max()))


def capture_loss(loss_mod, arrays):
    crit = loss_mod.Sigmoid_ce_loss(loss_weight=S.LOSS_WEIGHT)
    for r, c in S.FIXTURE_LOSS_SHAPES:
        x, t = S.loss_case(1, r, c)
        x = x[0].clone().requires_grad_(True)
        loss = crit(x, t)
        loss.backward()
        arrays[f'loss.{r}x{c}'] = loss.detach().numpy().reshape(1)
        arrays[f'loss.{r}x{c}.grad'] = x.grad.numpy()
        print(f'Sigmoid_ce_loss {r} x {c}: {float(loss.detach()):.6f}')


def main():
    l2i = P.camera_matrices()          # (imports the package BEFORE the stand-ins exist: its registry shim must not mirror into them)
    seg, loss_mod = refstub.load_petr_head_seg()
    arrays = {}
    capture_head(seg, arrays, l2i)
    capture_loss(loss_mod, arrays)
    meta = dict(layers=P.LAYERS, feedforward_channels=P.FFN, num_query=P.QUERIES, num_lane=S.NUM_LANE, batch=P.BS, num_cams=P.CAMS, h=P.H,
                w=P.W, pad_hw=list(P.PAD_HW), pc_range=P.PC_RANGE, position_range=P.POSITION_RANGE, loss_weight=S.LOSS_WEIGHT)
    arrays['meta'] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    out = os.path.join(ROOT, 'tests', 'golden', 'petr_head_seg.npz')
    np.savez_compressed(out, **arrays)
    print(f'{out}: {len(arrays) - 1} arrays, {os.path.getsize(out)} bytes')
    assert os.path.getsize(out) < (1 << 20)


if __name__ == '__main__':
    main()
