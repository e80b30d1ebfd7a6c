#!/usr/bin/env python
"""Generate tests/golden/petr_head.npz: PETRHead and PETRv2Head (with_fpe, with_time, with_multi) captured from the reference itself.

    python tools/gen_golden_petr_head.py      # needs the reference checkout (GD4D_REFERENCE_ROOT); never run on the GPU box

The reference's dense_heads/petr_head.py and petrv2_head.py are imported unmodified under tools/refstub.py's stand-ins
(refstub.load_petr_head); what is recorded is their fp32 CPU arithmetic in eval mode.  The heads hold about 4 M parameters - too many
to commit - so every parameter comes from a closed-form rule of the tensor's name and flat index (draw() below; tests/petr_head_ref.py
restates it) and the fixture stores, per tensor, its name, shape, sum and sum of squares.  Recorded (data only, no reference source),
per head `v1.` / `v2.`:
  - keys / shapes / sums / sumsqs of the state dict;
  - the inputs: feat (2, 2, C, 6, 10) on the k / 8 grid as float16 (C = 256 for PETRHead, 64 for PETRv2Head), lidar2img (2, 2, 4, 4)
    float32 (the package's synthetic rig, as the head-PE fixture), the timestamps; camera 1 of sample 0 has its last 3 columns padded;
  - x = input_proj(feat) as int16 x 512 (exact: grid inputs and weights), pos_embed (2, 2, 256, 6, 10) and query_embeds (40, 256) float32,
    mask (2, 2, 6, 10) bool;
  - all_cls_scores (2, 2, 40, 10) and all_bbox_preds (2, 2, 40, 10) float32.
"""
import json
import os
import re
import sys
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)
import refstub  # noqa: E402
import petr_head_ref as P  # noqa: E402  (the configs, inputs and camera matrices: data, shared with the tests)


def draw(name, shape, shared=False):
    """The parameter rule, restated (tests/petr_head_ref.py:draw is the other copy)."""
    n = int(np.prod(shape))
    if shared:                                                 # PETRHead: ONE branch object under six names
        name = re.sub(r'^(cls|reg)_branches\.\d+\.', r'\1_branches.0.', name)
    if name == 'code_weights':
        return torch.tensor(([1.0] * 8 + [0.2, 0.2])[:n], dtype=torch.float32).reshape(shape)
    m32 = np.uint64(0xFFFFFFFF)
    h = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(zlib.crc32(name.encode()))) & m32
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(2246822519)) & m32
    h ^= h >> np.uint64(13)
    if name == 'reference_points.weight':
        v = ((h % np.uint64(15)).astype(np.float32) + 1.0) / 16.0
    else:
        v = ((h % np.uint64(7)).astype(np.float32) - 3.0) / 64.0
        if len(shape) == 1 and name.endswith('.weight'):
            v = v + 1.0
    return torch.from_numpy(v.astype(np.float32)).reshape(tuple(shape))


def capture(kind, cls, arrays, l2i):
    cfg = P.head_config(kind)
    cfg.pop('type')
    head = cls(**cfg).eval()
    assert type(head.transformer).__module__.startswith(refstub._PKG), 'the transformer must be the reference\'s own'
    sd = head.state_dict()
    keys = list(sd.keys())
    with torch.no_grad():
        for k in keys:
            sd[k].copy_(draw(k, tuple(sd[k].shape), shared=kind == 'v1'))
    for name, mod in head.named_modules():                       # the rule's "+ 1" tensors are exactly the LayerNorm gains
        if isinstance(mod, torch.nn.LayerNorm):
            assert float(mod.weight.min()) > 0.9, name
    metas = P.img_metas(l2i, P.timestamps() if cfg.get('with_time') else None)
    feat = P.features(cfg['in_channels'])
    seen = {}

    def record(mod, args, out):
        seen.update(x=args[0].detach().clone(), mask=args[1].detach().clone(), query_embeds=args[2].detach().clone(),
                    pos_embed=args[3].detach().clone())
    hook = head.transformer.register_forward_hook(record)
    with torch.no_grad():
        outs = head([feat.clone()], metas)
    hook.remove()
    assert outs['enc_cls_scores'] is None and outs['enc_bbox_preds'] is None
    p = kind + '.'
    arrays[p + 'keys'] = np.frombuffer(json.dumps(keys).encode(), dtype=np.uint8)
    arrays[p + 'shapes'] = np.frombuffer(json.dumps([list(sd[k].shape) for k in keys]).encode(), dtype=np.uint8)
    arrays[p + 'sums'] = np.asarray([float(sd[k].double().sum()) for k in keys])
    arrays[p + 'sumsqs'] = np.asarray([float((sd[k].double() ** 2).sum()) for k in keys])
    f16 = feat.numpy().astype(np.float16)
    assert np.array_equal(f16.astype(np.float32), feat.numpy())
    arrays[p + 'feat'] = f16
    arrays[p + 'lidar2img'] = l2i.astype(np.float32)
    assert np.array_equal(arrays[p + 'lidar2img'].astype(np.float64), l2i)
    if cfg.get('with_time'):
        arrays[p + 'timestamps'] = P.timestamps()
    xq = np.round(seen['x'].numpy().astype(np.float64) * 512)
    assert np.array_equal(xq / 512, seen['x'].numpy().astype(np.float64)) and np.abs(xq).max() < 32768
    arrays[p + 'x@512'] = xq.astype(np.int16)
    arrays[p + 'mask'] = seen['mask'].numpy()
    arrays[p + 'pos_embed'] = seen['pos_embed'].numpy()
    arrays[p + 'query_embeds'] = seen['query_embeds'].numpy()
    arrays[p + 'all_cls_scores'] = outs['all_cls_scores'].numpy()
    arrays[p + 'all_bbox_preds'] = outs['all_bbox_preds'].numpy()
    print(kind, len(keys), 'tensors,', sum(v.numel() for v in sd.values()), 'parameters; |pos_embed| <=',
          float(seen['pos_embed'].abs().max()), '|cls| <=', float(outs['all_cls_scores'].abs().max()))


def main():
    l2i = P.camera_matrices()          # (imports the package BEFORE the stand-ins exist: its registry shim must not mirror into them)
    v1, v2 = refstub.load_petr_head()
    arrays = {}
    capture('v1', v1.PETRHead, arrays, l2i)
    capture('v2', v2.PETRv2Head, arrays, l2i)
    meta = dict(layers=P.LAYERS, feedforward_channels=P.FFN, num_query=P.QUERIES, batch=P.BS, num_cams=P.CAMS, h=P.H, w=P.W,
                pad_hw=list(P.PAD_HW), pc_range=P.PC_RANGE, position_range=P.POSITION_RANGE)
    arrays['meta'] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    out = os.path.join(ROOT, 'tests', 'golden', 'petr_head.npz')
    np.savez_compressed(out, **arrays)
    print(f'{out}: {len(arrays) - 1} arrays, {os.path.getsize(out)} bytes')
    assert os.path.getsize(out) < (1 << 20)


if __name__ == '__main__':
    main()
