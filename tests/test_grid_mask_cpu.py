"""GridMask without a GPU: the numpy restatements (tests/grid_mask_ref.py) against each other and against vectors captured from the
reference's own `GridMask.forward` (tools/gen_golden_grid_mask.py), the module's host draw against the reference's np.random order,
the device route's draw contract on its host restatement, the C ABI's argument checks, and the module's surface."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from grid_mask_ref import (M32, apply_ref, device_draw_ref, device_offset_ref, device_step_ref, fixture_cases, mask_closed,
                           mask_literal, prob_threshold)

NEW_EXPORTS = ('gd4d_grid_mask_fwd', 'gd4d_grid_mask_draw')
CASES = fixture_cases()
IDS = [c['tag'] for c in CASES]


def replay_offset(c):
    """The offset map the reference drew in case `c`: np.random in its order (grid_mask.py:85, 91, 94-95, 107, 118)."""
    h, w = c['shape'][-2:]
    np.random.seed(c['seed'])
    np.random.rand()
    d = np.random.randint(2, h)
    assert (d, np.random.randint(d), np.random.randint(d)) == (c['d'], c['st_h'], c['st_w'])
    np.random.randint(1)
    return (2 * (np.random.rand(h, w) - 0.5)).astype(np.float32)


def test_closed_form_equals_the_literal_loops_on_every_small_size():
    total = wide = 0
    for h in range(3, 13):
        for w in range(3, 13):
            hh = int(1.5 * h)
            for d in range(2, h):
                ls = sorted({1, d - 1, min(max(int(d * 0.5 + 0.5), 1), d - 1)})
                for l in ls:
                    for st_h in range(d):
                        for st_w in range(d):
                            a = mask_closed(h, w, d, l, st_h, st_w)
                            assert np.array_equal(a, mask_literal(h, w, d, l, st_h, st_w)), (h, w, d, l, st_h, st_w)
                            total += 1
                            wide += 2 * d > hh
                # one axis alone and the inverted mask: once per (h, w, d), at the starts that reach furthest into the crop
                for use_h, use_w, mode in ((True, False, 0), (False, True, 1), (True, True, 1)):
                    for st in (0, d - 1):
                        a = mask_closed(h, w, d, ls[-1], st, d - 1 - st, use_h, use_w, mode)
                        assert np.array_equal(a, mask_literal(h, w, d, ls[-1], st, d - 1 - st, use_h, use_w, mode))
    assert total > 20000 and wide / total > 0.05, (total, wide)            # d > hh / 2: the band the reference never draws


def test_undrawn_second_band_is_not_masked():
    # h = 12: hh = 18, d = 11 draws ONE band (18 // 11); with st_h = 0 a second would start at Y = 11, i.e. y = 8, inside the crop
    m = mask_closed(12, 12, 11, 6, 0, 0, True, False, 0)
    assert m[:3].sum() == 0 and m[3:].min() == 1                            # rows Y = 3..5 of band 0, nothing at y = 8


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_restatements_reproduce_the_reference(c):
    h, w = c['shape'][-2:]
    if not c['applied']:
        assert c['y'] is None
        return
    off = replay_offset(c) if c['offset'] else None
    for fn in (mask_closed, mask_literal):
        mask = fn(h, w, c['d'], c['l'], c['st_h'], c['st_w'], c['use_h'], c['use_w'], c['mode'])
        assert np.array_equal(apply_ref(c['x'], mask, off), c['y'])
    assert 0 < float((c['y'] == 0).mean()) < 1 or c['offset']


def test_fixture_covers_what_it_should():
    applied = [c for c in CASES if c['applied']]
    assert any(2 * c['d'] > int(1.5 * c['shape'][2]) for c in applied) and any(c['d'] == 2 for c in applied)
    assert {c['mode'] for c in applied} == {0, 1} and any(c['offset'] for c in applied) and any(not c['applied'] for c in CASES)
    assert any(c['use_h'] and not c['use_w'] for c in applied) and any(c['use_w'] and not c['use_h'] for c in applied)


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_host_draw_follows_the_reference(c):
    from graph_detr4d_amd import GridMask
    h, w = c['shape'][-2:]
    m = GridMask(c['use_h'], c['use_w'], rotate=1, offset=c['offset'], ratio=0.5, mode=c['mode'], prob=c['prob'])
    np.random.seed(c['seed'])
    draw = m.host_draw(h, w)
    assert float(np.random.rand()) == c['next_rand']                       # np.random is left where the reference leaves it
    if not c['applied']:
        assert draw is None
        return
    assert (draw['d'], draw['l'], draw['st_h'], draw['st_w'], draw['angle']) == (c['d'], c['l'], c['st_h'], c['st_w'], 0)
    assert m.l == c['l']
    assert (draw['offset'] is not None) == c['offset']
    if c['offset']:
        assert draw['offset'].dtype == np.float32 and np.array_equal(draw['offset'], replay_offset(c))


def test_host_draw_in_eval_mode_consumes_one_rand_and_returns_none():
    from graph_detr4d_amd import GridMask
    m = GridMask(True, True, prob=1.0).eval()
    np.random.seed(3)
    assert m.host_draw(12, 20) is None
    after = float(np.random.rand())
    np.random.seed(3)
    np.random.rand()
    assert after == float(np.random.rand())


@pytest.mark.parametrize('h', [3, 4, 320, 900])
def test_device_draw_contract(h):
    seed, steps, prob = 0x1234_5678_9ABC_DEF0 ^ h, 10000, 0.7
    thresh = prob_threshold(prob)
    assert thresh == int(0.7 * 2 ** 32 + 0.5)
    hits, ds = 0, set()
    state = [seed & M32, seed >> 32, 0, thresh]
    for step in range(steps):
        block, after = device_step_ref(state, h, 0.5)
        assert after == [state[0], state[1], step + 1, thresh] and block[5:] == state[:3]        # the counter advances by one
        state = after
        apply, d, l, st_h, st_w = block[:5]
        assert tuple(block[:5]) == device_draw_ref(seed, step, thresh, h, 0.5)
        assert apply in (0, 1) and 2 <= d < h and 1 <= l <= d - 1 and 0 <= st_h < d and 0 <= st_w < d
        assert l == min(max(int(d * 0.5 + 0.5), 1), d - 1)
        hits += apply
        ds.add(d)
    # the gate: a binomial (steps, prob) count, within five standard deviations (fixed seed: deterministic)
    assert abs(hits - steps * prob) <= 5 * math.sqrt(steps * prob * (1 - prob)), hits
    assert h > 4 or ds == set(range(2, h))                                  # the small heights: every period is drawn
    if h >= 320:
        assert len(ds) > 0.9 * (h - 2) and min(ds) <= 3 and max(ds) >= h - 2
    assert device_draw_ref(seed, 0, M32, h, 0.5)[0] == 1 and device_draw_ref(seed, 0, 0, h, 0.5)[0] == 0          # prob >= 1 / <= 0
    assert device_draw_ref(seed, 5, thresh, h, 0.5) != device_draw_ref(seed + 1, 5, thresh, h, 0.5) or h <= 4


def test_device_offset_values():
    o = device_offset_ref(99, 7, 33, 70)
    assert o.dtype == np.float32 and o.shape == (33, 70) and o.min() >= -1 and o.max() < 1
    assert abs(float(o.mean())) < 5 / math.sqrt(3 * o.size) and len(np.unique(o)) > 0.99 * o.size          # uniform on [-1, 1): sd 1/sqrt 3
    assert not np.array_equal(o, device_offset_ref(99, 8, 33, 70)) and not np.array_equal(o, device_offset_ref(98, 7, 33, 70))


def test_step_counter_wraps():
    _, after = device_step_ref([1, 2, M32, 0], 12, 0.5)
    assert after == [1, 2, 0, 0]


def test_new_exports_in_header_lib_and_library(repo_root):
    from graph_detr4d_amd import _lib
    hdr = open(os.path.join(repo_root, 'include', 'gd4d.h')).read()
    lib = _lib.load()
    assert lib.gd4d_abi_version() == 56 and _lib.ABI_VERSION == 56          # additive exports: the version stays
    for name in NEW_EXPORTS:
        assert name in _lib.SIGNATURES and re.search(rf'\b{name}\s*\(', hdr)
        assert hasattr(lib, name)


def test_entry_points_validate_before_any_gpu_work():
    from graph_detr4d_amd import _lib
    lib = _lib.load()
    EINVAL, EUNSUPPORTED = -1, -2
    F32, BF16, F16 = _lib.F32, _lib.BF16, _lib.F16
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 96)()
    ptr = ctypes.c_void_p((ctypes.addressof(buf) + 63) & ~63)
    other = ctypes.c_void_p(ptr.value + 64)

    def fwd(x=ptr, out=other, it=F32, ot=F32, r=2, c=3, h=12, w=20, apply=1, d=5, l=2, st_h=0, st_w=4, use_h=1, use_w=1, mode=1,
            offset=null, block=null, gen=0):
        return lib.gd4d_grid_mask_fwd(x, out, it, ot, r, c, h, w, apply, d, l, st_h, st_w, use_h, use_w, mode, offset, block, gen, null)
    assert fwd(x=null) == EINVAL and fwd(out=null) == EINVAL
    assert fwd(r=0) == EINVAL and fwd(c=0) == EINVAL and fwd(w=0) == EINVAL
    assert fwd(h=2) == EINVAL                                               # randint(2, h) needs h >= 3
    assert fwd(d=1) == EINVAL and fwd(d=0) == EINVAL
    assert fwd(l=0) == EINVAL and fwd(l=5) == EINVAL                        # l in [1, d - 1]
    assert fwd(st_h=-1) == EINVAL and fwd(st_h=5) == EINVAL and fwd(st_w=-1) == EINVAL and fwd(st_w=5) == EINVAL
    assert fwd(mode=2) == EINVAL
    for it, ot in ((F16, F32), (BF16, F32), (F16, BF16), (BF16, F16), (3, 3), (F32, 7), (-1, F32)):
        assert fwd(it=it, ot=ot) == EUNSUPPORTED, (it, ot)
    assert fwd(out=ptr, ot=F16) == EINVAL and fwd(out=ptr, ot=BF16) == EINVAL                     # in place with another dtype
    assert fwd(gen=1) == EINVAL and fwd(gen=1, block=ptr, offset=ptr) == EINVAL                   # generated offsets need the block alone
    assert fwd(h=65536, w=32768) == EUNSUPPORTED and fwd(r=32768, c=4096, h=16) == EUNSUPPORTED   # H W / R C H >= 2^31

    def draw(state=ptr, block=other, h=12, ratio=0.5):
        return lib.gd4d_grid_mask_draw(state, block, h, ratio, null)
    assert draw(state=null) == EINVAL and draw(block=null) == EINVAL and draw(h=2) == EINVAL
    assert draw(ratio=-0.5) == EINVAL and draw(ratio=float('nan')) == EINVAL


def test_module_surface():
    from graph_detr4d_amd import GridMask, plumbing
    from graph_detr4d_amd._lib import Gd4dError
    m = GridMask(True, True, rotate=1, offset=False, ratio=0.5, mode=1, prob=0.7)
    assert list(m.state_dict()) == [] and list(m.parameters()) == [] and list(m.buffers()) == []
    assert (m.use_h, m.use_w, m.rotate, m.offset, m.ratio, m.mode, m.st_prob, m.prob) == (True, True, 1, False, 0.5, 1, 0.7, 0.7)
    m.set_prob(3, 12)
    assert m.prob == 0.7 * 3 / 12 and m.st_prob == 0.7
    with pytest.raises(Gd4dError, match='torch_ops=True'):
        GridMask(True, True, rotate=2)
    assert GridMask(True, True, rotate=2, torch_ops=True).rotate == 2
    with pytest.raises(Gd4dError, match='GPU'):
        m(torch.zeros(1, 3, 5, 7))                                          # no CPU fallback
    with pytest.raises(ValueError):
        GridMask(True, True, out_dtype=torch.float64)
    with pytest.raises(ValueError):
        GridMask(True, True, out_dtype=torch.float16, inplace=True)
    ext = plumbing.ImageFeatureExtractor(torch.nn.Identity())
    assert ext.grid_mask is None and not any(isinstance(s, GridMask) for s in ext.modules())
    on = plumbing.ImageFeatureExtractor(torch.nn.Identity(), use_grid_mask=True).grid_mask
    assert isinstance(on, GridMask) and (on.use_h, on.use_w, on.rotate, on.offset, on.ratio, on.mode, on.prob) == (True, True, 1, False, 0.5, 1, 0.7)
    assert plumbing.ImageFeatureExtractor(torch.nn.Identity(), grid_mask=m).grid_mask is m


@pytest.mark.parametrize('c', [c for c in CASES if c['shape'][2] == 12], ids=[c['tag'] for c in CASES if c['shape'][2] == 12])
def test_torch_ops_route_is_the_reference_on_the_host(c):
    """torch_ops=True is the reference's op sequence and is device-agnostic: under the fixture's seed it gives the fixture's output."""
    from graph_detr4d_amd import GridMask
    m = GridMask(c['use_h'], c['use_w'], rotate=1, offset=c['offset'], ratio=0.5, mode=c['mode'], prob=c['prob'], torch_ops=True)
    x = torch.from_numpy(c['x'].copy())
    np.random.seed(c['seed'])
    y = m(x)
    assert float(np.random.rand()) == c['next_rand']
    if not c['applied']:
        assert y is x
    else:
        assert torch.equal(y, torch.from_numpy(c['y']))
