#!/usr/bin/env python
"""Generate tests/golden/petr_transformer_grads.npz: the gradients of the run recorded in tests/golden/petr_transformer.npz, from the
reference itself.

    python tools/gen_golden_petr_train.py      # needs the reference checkout (GD4D_REFERENCE_ROOT); never run on the GPU box

The reference's models/utils/petr_transformer.py is imported unmodified under tools/refstub.py's stand-ins, loaded with the state dict
of the committed fixture and run on its inputs in EVAL mode with autograd on (fp32, CPU): dropout is off and with_cp is inactive, so
the gradients are a function of the fixture alone.  The loss is (out_dec * G).sum() with G drawn on the k / 8 grid (|k| <= 16) from a
fixed seed.  Recorded (data only, no reference source):
  - `G` as float16 (exact);
  - `grad.x`, `grad.pos_embed` (2, 2, 256, 6, 10) and `grad.query_embed` (40, 256) in float32;
  - `grad.<key>` in float32 for every bias and LayerNorm parameter;
  - for every weight matrix `rowsum.<key>` (its gradient summed over dim 1) and `colsum.<key>` (over dim 0) in float32 - the full
    matrices do not fit below 1 MiB.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import refstub  # noqa: E402
from gen_golden_petr import config  # noqa: E402

G_SEED = 20240918


def loss_weights(shape):
    g = torch.Generator().manual_seed(G_SEED)
    return torch.randint(-16, 17, shape, generator=g).float() / 8


def main():
    fix = np.load(os.path.join(ROOT, 'tests', 'golden', 'petr_transformer.npz'))
    refstub.load_petr_transformer()
    model = refstub.TRANSFORMER.build(config())
    sd = {k[3:]: torch.from_numpy(fix[k].astype(np.float32)) for k in fix.files if k.startswith('sd.')}
    model.load_state_dict(sd, strict=True)
    model.eval()
    x, pos, query_embed = (torch.from_numpy(fix[k].astype(np.float32)).requires_grad_(True) for k in ('x', 'pos_embed', 'query_embed'))
    mask = torch.from_numpy(fix['mask'])
    out_dec, _ = model(x, mask, query_embed, pos)
    assert np.array_equal(out_dec.detach().numpy(), fix['out_dec']), 'the run does not reproduce the fixture'
    G = loss_weights(out_dec.shape)
    (out_dec * G).sum().backward()
    arrays = {'G': G.numpy().astype(np.float16)}
    assert np.array_equal(arrays['G'].astype(np.float32), G.numpy())
    for name, t in (('x', x), ('pos_embed', pos), ('query_embed', query_embed)):
        arrays['grad.' + name] = t.grad.numpy()
    for name, p in model.named_parameters():
        g = p.grad
        assert g is not None, name
        if g.dim() == 1:
            arrays['grad.' + name] = g.numpy()
        else:
            arrays['rowsum.' + name] = g.sum(1).numpy()
            arrays['colsum.' + name] = g.sum(0).numpy()
    meta = dict(fixture='petr_transformer', loss='(out_dec * G).sum()', g_seed=G_SEED)
    arrays['meta'] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    out = os.path.join(ROOT, 'tests', 'golden', 'petr_transformer_grads.npz')
    np.savez_compressed(out, **arrays)
    print(f'{out}: {len(arrays) - 1} arrays, {os.path.getsize(out)} bytes')


if __name__ == '__main__':
    main()
