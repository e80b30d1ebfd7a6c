#!/usr/bin/env python
"""Generate tests/golden/grid_mask.npz: GridMask outputs captured from the reference itself.

    python tools/gen_golden_grid_mask.py      # needs the reference checkout (GD4D_REFERENCE_ROOT); never run on the GPU box

The reference's models/utils/grid_mask.py is imported unmodified at run time (it needs torch, numpy and PIL only);
`torch.Tensor.cuda` is patched to the identity for the call, so its `GridMask.forward` runs on the host.  Recorded (data only, no
reference source): per shape the input - on the k/8 grid, stored as int8 `x_<H>x<W>@q` -, per case the np.random seed, the constructor
arguments, whether the gate returned the input, the output (`y<i>@q` int8 on the same grid - a 0/1 mask keeps it there -, `y<i>`
float32 with an offset map, nothing when the gate returned the input), the drawn (d, l, st_h, st_w) - recovered by replaying np.random
in the documented order and checked against the reference's own `self.l` -, and the next np.random.rand() after the call (the state
the reference leaves behind).
"""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from refstub import REFERENCE_ROOT  # noqa: E402

SCALE = 8                                                   # inputs live on the k/8 grid, |k| <= 16
SHAPES = [(2, 3, 12, 20), (1, 3, 5, 7), (2, 3, 33, 70)]
# (use_h, use_w, offset, mode, prob): both modes, each axis alone, offset on and off
VARIANTS = [(True, True, False, 1, 1.0), (True, True, False, 0, 1.0), (True, False, False, 0, 1.0), (False, True, False, 1, 1.0),
            (True, True, True, 0, 1.0), (True, True, True, 1, 1.0)]


def load_reference():
    path = os.path.join(REFERENCE_ROOT, 'projects', 'mmdet3d_plugin', 'models', 'utils', 'grid_mask.py')
    if not os.path.isfile(path):
        raise FileNotFoundError(f'reference not present at {path} (build container only)')
    spec = importlib.util.spec_from_file_location('_ref_grid_mask', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def replay_draws(seed, prob, h, w, ratio, offset):
    """np.random in the reference's order (:85, 91, 94-95, 107, 118) -> (gate passed, d, l, st_h, st_w, next rand())."""
    np.random.seed(seed)
    if np.random.rand() > prob:
        return False, 0, 0, 0, 0, float(np.random.rand())
    d = int(np.random.randint(2, h))
    l = min(max(int(d * ratio + 0.5), 1), d - 1)
    st_h, st_w = int(np.random.randint(d)), int(np.random.randint(d))
    np.random.randint(1)
    if offset:
        np.random.rand(h, w)
    return True, d, l, st_h, st_w, float(np.random.rand())


def find_seed(want, prob, h, w, used):
    """The smallest unused seed whose draws satisfy `want(d, hh, passed)`."""
    for seed in range(10000):
        passed, d, _, _, _, _ = replay_draws(seed, prob, h, w, 0.5, False)
        if seed not in used and want(d, int(1.5 * h), passed):
            return seed
    raise RuntimeError('no seed found')


def main():
    ref = load_reference()
    cases, used, arrays = [], set(), {}
    rng = np.random.RandomState(1234)
    inputs = {shape: rng.randint(-16, 17, size=shape).astype(np.int8) for shape in SHAPES}

    def add(shape, use_h, use_w, offset, mode, prob, seed, tag):
        used.add(seed)
        n, c, h, w = shape
        x = inputs[shape].astype(np.float32) / SCALE
        m = ref.GridMask(use_h, use_w, rotate=1, offset=offset, ratio=0.5, mode=mode, prob=prob)
        m.train()
        saved = torch.Tensor.cuda
        torch.Tensor.cuda = lambda self, *a, **k: self
        try:
            np.random.seed(seed)
            xt = torch.from_numpy(x.copy())
            yt = m(xt)
            nxt = float(np.random.rand())
        finally:
            torch.Tensor.cuda = saved
        passed, d, l, st_h, st_w, nxt2 = replay_draws(seed, prob, h, w, 0.5, offset)
        assert nxt == nxt2 and passed == (yt is not xt), (tag, 'the replay of np.random left the reference\'s order')
        if passed:
            assert m.l == l
        i = len(cases)
        if passed and offset:
            arrays[f'y{i}'] = yt.numpy().copy()
        elif passed:
            q = yt.numpy() * SCALE
            assert np.array_equal(q, np.round(q)) and np.abs(q).max() <= 127
            arrays[f'y{i}@q'] = q.astype(np.int8)
        cases.append(dict(tag=tag, seed=seed, shape=list(shape), use_h=use_h, use_w=use_w, offset=offset, mode=mode, prob=prob,
                          applied=bool(passed), d=d, l=l, st_h=st_h, st_w=st_w, next_rand=nxt))

    for shape in SHAPES:
        h, w = shape[-2:]
        for k, (use_h, use_w, offset, mode, prob) in enumerate(VARIANTS):
            if offset and h * w > 1000:                  # offset maps are random floats: the small shapes only
                continue
            seed = find_seed(lambda d, hh, passed: passed, prob, h, w, used)
            add(shape, use_h, use_w, offset, mode, prob, seed, f'{h}x{w}_v{k}')
        # the undrawn second band (d > hh / 2), the smallest period, and a gate that returns the input
        add(shape, True, True, False, 1, 1.0, find_seed(lambda d, hh, passed: passed and 2 * d > hh, 1.0, h, w, used), f'{h}x{w}_wide')
        add(shape, True, True, False, 0, 1.0, find_seed(lambda d, hh, passed: passed and d == 2, 1.0, h, w, used), f'{h}x{w}_d2')
        add(shape, True, True, False, 1, 0.3, find_seed(lambda d, hh, passed: not passed, 0.3, h, w, used), f'{h}x{w}_gate')
    assert any(c['applied'] and 2 * c['d'] > int(1.5 * c['shape'][2]) for c in cases) and any(c['applied'] and c['d'] == 2 for c in cases)
    for shape, x in inputs.items():
        arrays[f'x_{shape[2]}x{shape[3]}@q'] = x
    arrays['meta'] = np.frombuffer(json.dumps(dict(cases=cases, ratio=0.5, rotate=1, scale=SCALE)).encode(), dtype=np.uint8)
    out = os.path.join(ROOT, 'tests', 'golden', 'grid_mask.npz')
    np.savez_compressed(out, **arrays)
    print(f'{out}: {len(cases)} cases, {os.path.getsize(out)} bytes')


if __name__ == '__main__':
    main()
