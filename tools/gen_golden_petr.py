#!/usr/bin/env python
"""Generate tests/golden/petr_transformer.npz: a small PETRTransformer run captured from the reference itself.

    python tools/gen_golden_petr.py      # needs the reference checkout (GD4D_REFERENCE_ROOT); never run on the GPU box

The reference's models/utils/petr_transformer.py is imported unmodified under tools/refstub.py's stand-ins for mmcv / mmdet; its
PETRMultiheadAttention wraps torch's own nn.MultiheadAttention, so what is recorded is the reference's arithmetic (fp32, CPU, eval
mode).  Recorded (data only, no reference source):
  - the state dict of a 2-layer PETRTransformer (256 dims, 8 heads, feedforward_channels 128; the config block of
    projects/configs/petrv2/petrv2_vovnet_gridmask_p4_800x320.py otherwise), `sd.<key>` as float16: every parameter is drawn on the
    k / 64 grid (LayerNorm weights 1 + k / 64), which float16 holds exactly;
  - the inputs: x and pos_embed (2, 2, 256, 6, 10) on the k / 8 grid as float16, query_embed (40, 256) likewise, mask (2, 2, 6, 10)
    bool - the last 3 columns of camera 1 in batch 0 padded, nothing in batch 1;
  - the outputs: out_dec (2, 2, 40, 256), memory (2, 2, 256, 6, 10; as float16, it is x), and for decoder layer 0 the
    cross-attention module's own input query and output (40, 2, 256).
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import refstub  # noqa: E402

DIMS, HEADS, FFN, LAYERS, QUERIES, BS, CAMS, H, W = 256, 8, 128, 2, 40, 2, 2, 6, 10


def config():
    return dict(type='PETRTransformer', decoder=dict(
        type='PETRTransformerDecoder', return_intermediate=True, num_layers=LAYERS,
        transformerlayers=dict(
            type='PETRTransformerDecoderLayer',
            attn_cfgs=[dict(type='MultiheadAttention', embed_dims=DIMS, num_heads=HEADS, dropout=0.1),
                       dict(type='PETRMultiheadAttention', embed_dims=DIMS, num_heads=HEADS, dropout=0.1)],
            feedforward_channels=FFN, ffn_dropout=0.1, with_cp=True,
            operation_order=('self_attn', 'norm', 'cross_attn', 'norm', 'ffn', 'norm'))))


def main():
    refstub.load_petr_transformer()
    model = refstub.TRANSFORMER.build(config())
    model.init_weights()
    model.eval()
    g = torch.Generator().manual_seed(20240917)
    grid = lambda shape, k, scale: torch.randint(-k, k + 1, shape, generator=g).float() / scale      # noqa: E731
    with torch.no_grad():
        for name, p in model.named_parameters():
            p.copy_(grid(p.shape, 3, 64))
            if ('norms.' in name or 'post_norm' in name) and name.endswith('weight'):
                p.add_(1.0)
    x = grid((BS, CAMS, DIMS, H, W), 16, 8)
    pos = grid((BS, CAMS, DIMS, H, W), 16, 8)
    query_embed = grid((QUERIES, DIMS), 16, 8)
    mask = torch.zeros(BS, CAMS, H, W, dtype=torch.bool)
    mask[0, 1, :, W - 3:] = True
    seen = {}
    cross = model.decoder.layers[0].attentions[1]
    assert type(cross).__name__ == 'PETRMultiheadAttention'
    hook = cross.register_forward_hook(lambda m, inp, out: seen.update(query=inp[0].detach().clone(), out=out.detach().clone()))
    with torch.no_grad():
        out_dec, memory = model(x, mask, query_embed, pos)
    hook.remove()
    assert tuple(out_dec.shape) == (LAYERS, BS, QUERIES, DIMS) and tuple(memory.shape) == (BS, CAMS, DIMS, H, W)
    f16 = lambda t: t.numpy().astype(np.float16)                                                      # noqa: E731
    arrays = {}
    for k, v in model.state_dict().items():
        a = f16(v)
        assert np.array_equal(a.astype(np.float32), v.numpy()), k
        arrays['sd.' + k] = a
    for k, v in (('x', x), ('pos_embed', pos), ('query_embed', query_embed), ('memory', memory)):
        a = f16(v.contiguous())
        assert np.array_equal(a.astype(np.float32), v.contiguous().numpy()), k
        arrays[k] = a
    arrays['mask'] = mask.numpy()
    arrays['out_dec'] = out_dec.contiguous().numpy()
    arrays['cross0_query'] = seen['query'].numpy()
    arrays['cross0_out'] = seen['out'].numpy()
    meta = dict(embed_dims=DIMS, num_heads=HEADS, feedforward_channels=FFN, num_layers=LAYERS, num_query=QUERIES, batch=BS,
                num_cams=CAMS, h=H, w=W)
    arrays['meta'] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    out = os.path.join(ROOT, 'tests', 'golden', 'petr_transformer.npz')
    np.savez_compressed(out, **arrays)
    print(f'{out}: {len(arrays) - 1} arrays, {os.path.getsize(out)} bytes')


if __name__ == '__main__':
    main()
