"""GridMask on the GPU: gd4d_grid_mask_fwd / gd4d_grid_mask_draw and the module against the reference's recorded outputs
(tests/golden/grid_mask.npz) and the numpy restatement (tests/grid_mask_ref.py).  A 0/1 mask and a cast are exact, so every comparison
is torch.equal."""
import numpy as np
import pytest
import torch

from grid_mask_ref import (M32, apply_ref, device_draw_ref, device_offset_ref, device_step_ref, fixture_cases, mask_closed,
                           prob_threshold)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CASES = fixture_cases()
SHAPES = [(1, 3, 5, 7), (2, 3, 12, 20), (3, 1, 33, 70)]


def images(shape, seed=0, dtype=torch.float32):
    """Finite, non-zero values (a zero in the output is then the mask's)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(shape, generator=g) + 0.25
    return (x * (torch.randint(0, 2, shape, generator=g) * 2 - 1)).to(dtype)


def expect(x, d, l, st_h, st_w, use_h=True, use_w=True, mode=0, offset=None):
    h, w = x.shape[-2:]
    mask = mask_closed(h, w, d, l, st_h, st_w, use_h, use_w, mode)
    return torch.from_numpy(apply_ref(x.float().numpy(), mask, offset))


def param_sets(h):
    """d = 2, d = h - 1, starts 0 and d - 1, and a middle one."""
    out = []
    for d in sorted({2, h - 1, max(2, h // 2)}):
        l = min(max(int(d * 0.5 + 0.5), 1), d - 1)
        for st_h, st_w in ((0, d - 1), (d - 1, 0)):
            out.append((d, l, st_h, st_w))
        out.append((d, d - 1, d // 2, d // 2))
    return out


def block_of(params, apply=1, words=(0, 0, 0)):
    return torch.tensor([apply, *params, *words], dtype=torch.int32, device=DEV)


def signed(v):
    return v - (1 << 32) if v >= (1 << 31) else v


@pytest.mark.parametrize('c', CASES, ids=[c['tag'] for c in CASES])
def test_module_reproduces_the_reference(c):
    from graph_detr4d_amd import GridMask
    m = GridMask(c['use_h'], c['use_w'], rotate=1, offset=c['offset'], ratio=0.5, mode=c['mode'], prob=c['prob']).train()
    x = torch.from_numpy(c['x'].copy()).to(DEV)
    np.random.seed(c['seed'])
    y = m(x)
    assert float(np.random.rand()) == c['next_rand']
    if not c['applied']:
        assert y is x                                                       # the gate returns the very same tensor
        return
    assert y is not x and y.dtype == torch.float32
    assert torch.equal(y.cpu(), torch.from_numpy(c['y']))
    assert torch.equal(x.cpu(), torch.from_numpy(c['x']))                   # out of place: the input is untouched


@pytest.mark.parametrize('shape', SHAPES + [(3, 3, 701, 8), (8, 3, 701, 8)], ids=str)
def test_kernel_equals_the_restatement(shape):
    """Odd plane counts, widths that are no multiple of 4, one and several workgroups; the two tall shapes make a wave take 3 and 8
    rows, across plane ends (701 is no multiple of either)."""
    from graph_detr4d_amd import ops
    h, w = shape[-2:]
    x = images(shape, 1)
    xd = x.to(DEV)
    off = (torch.rand(h, w, generator=torch.Generator().manual_seed(2)) * 2 - 1)
    offd = off.to(DEV)
    sets = param_sets(h) if h < 100 else param_sets(h)[::3]
    for (d, l, st_h, st_w) in sets:
        for mode, use_h, use_w, with_off in ((0, True, True, False), (1, True, True, False), (0, True, False, False), (1, False, True, False),
                                             (0, True, True, True), (1, True, True, True)):
            y = ops.grid_mask_fwd(xd, d, l, st_h, st_w, use_h, use_w, mode, offset=offd if with_off else None)
            want = expect(x, d, l, st_h, st_w, use_h, use_w, mode, off.numpy() if with_off else None)
            assert torch.equal(y.cpu(), want), (shape, d, l, st_h, st_w, mode, use_h, use_w, with_off)


@pytest.mark.parametrize('shape', [(2, 3, 12, 20), (3, 1, 33, 70)], ids=str)
def test_unaligned_views(shape):
    """A storage offset of one element: the 16-byte form cannot be used on the input, the output or either; results do not change."""
    from graph_detr4d_amd import ops
    n = int(np.prod(shape))
    x = images(shape, 3)
    buf = torch.zeros(n + 1, device=DEV)
    view = buf[1:].view(shape)
    view.copy_(x)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    d, l, st_h, st_w = param_sets(shape[2])[1]
    want = expect(x, d, l, st_h, st_w, mode=1)
    assert torch.equal(ops.grid_mask_fwd(view, d, l, st_h, st_w, mode=1).cpu(), want)             # unaligned in, aligned out
    obuf = torch.full((n + 1,), 7.0, device=DEV)
    ops.grid_mask_fwd(x.to(DEV), d, l, st_h, st_w, mode=1, out=obuf[1:].view(shape))              # aligned in, unaligned out
    assert torch.equal(obuf[1:].view(shape).cpu(), want) and float(obuf[0]) == 7.0
    ops.grid_mask_fwd(view, d, l, st_h, st_w, mode=1, out=view)                                   # in place on the view
    assert torch.equal(view.cpu(), want) and float(buf[0]) == 0.0


@pytest.mark.parametrize('pair', [(torch.float32, torch.float32), (torch.float32, torch.float16), (torch.float32, torch.bfloat16),
                                  (torch.float16, torch.float16), (torch.bfloat16, torch.bfloat16)], ids=str)
@pytest.mark.parametrize('shape', [(2, 3, 12, 20), (3, 2, 9, 32), (1, 3, 5, 7)], ids=str)
def test_dtype_pairs(pair, shape):
    """W = 32 takes the 16-byte form for the 16-bit inputs too (8 elements per lane), 20 only for fp32, 7 for none."""
    from graph_detr4d_amd import ops
    tin, tout = pair
    h, w = shape[-2:]
    x = (images(shape, 4) * 3.1415926).to(tin)                              # fp32 values that are NOT representable in 16 bits: the cast rounds
    off = torch.rand(h, w, generator=torch.Generator().manual_seed(5)) * 2 - 1
    for (d, l, st_h, st_w) in param_sets(h)[:4]:
        for mode in (0, 1):
            for with_off in (False, True):
                y = ops.grid_mask_fwd(x.to(DEV), d, l, st_h, st_w, mode=mode, out_dtype=tout, offset=off.to(DEV) if with_off else None)
                want = expect(x, d, l, st_h, st_w, mode=mode, offset=off.numpy() if with_off else None).to(tout)
                assert y.dtype == tout and torch.equal(y.cpu(), want), (pair, shape, d, mode, with_off)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16, torch.bfloat16], ids=str)
def test_in_place_equals_out_of_place(dtype):
    from graph_detr4d_amd import ops
    for shape in ((2, 3, 12, 20), (3, 2, 9, 32), (1, 3, 5, 7)):
        h, w = shape[-2:]
        off = (torch.rand(h, w, generator=torch.Generator().manual_seed(6)) * 2 - 1).to(DEV)
        for (d, l, st_h, st_w) in param_sets(h)[:3]:
            for mode in (0, 1):
                for o in (None, off):
                    x = images(shape, 7, dtype).to(DEV)
                    y = ops.grid_mask_fwd(x, d, l, st_h, st_w, mode=mode, offset=o)
                    z = ops.grid_mask_fwd(x, d, l, st_h, st_w, mode=mode, offset=o, out=x)
                    assert z is x and torch.equal(x, y)


def test_by_value_and_through_the_block_give_the_same_bits():
    from graph_detr4d_amd import ops
    for shape in SHAPES:
        x = images(shape, 8).to(DEV)
        for params in param_sets(shape[2]):
            for mode in (0, 1):
                a = ops.grid_mask_fwd(x, *params, mode=mode)
                b = ops.grid_mask_fwd(x, 2, 1, 0, 0, mode=mode, block=block_of(params))          # the values in the call are ignored
                assert torch.equal(a, b)


@pytest.mark.parametrize('out_dtype', [None, torch.float16, torch.bfloat16], ids=str)
def test_apply_zero_in_the_block(out_dtype):
    from graph_detr4d_amd import ops
    for shape in ((2, 3, 12, 20), (1, 3, 5, 7)):
        x = (images(shape, 9) * 3.1415926).to(DEV)
        blk = block_of((5 if shape[2] > 5 else 2, 1, 1, 1), apply=0)
        y = ops.grid_mask_fwd(x, block=blk, mode=1, out_dtype=out_dtype)
        assert torch.equal(y, x.to(out_dtype or torch.float32))            # a copy (and the cast)
        if out_dtype is None:
            keep = x.clone()
            ops.grid_mask_fwd(x, block=blk, mode=1, out=x)
            assert torch.equal(x, keep)                                     # in place: nothing changes
            assert torch.equal(ops.grid_mask_fwd(x, 2, 1, 0, 0, apply=False), keep)             # by value as well


@pytest.mark.parametrize('mode', [0, 1])
def test_backward_is_grad_times_mask(mode):
    from graph_detr4d_amd import GridMask
    shape = (2, 3, 12, 20)
    m = GridMask(True, True, mode=mode, prob=1.0, offset=bool(mode)).train()                      # mode 1 also with an offset: it has no gradient
    g = images(shape, 10).to(DEV)
    grads = []
    for _ in range(2):
        x = images(shape, 11).to(DEV).requires_grad_(True)
        np.random.seed(21)
        y = m(x)
        assert y.requires_grad
        y.backward(g)
        grads.append(x.grad.clone())
    np.random.seed(21)
    dr = m.host_draw(12, 20)
    mask = torch.from_numpy(mask_closed(12, 20, dr['d'], dr['l'], dr['st_h'], dr['st_w'], True, True, mode))
    assert torch.equal(grads[0].cpu(), g.cpu() * mask) and 0 < float(mask.mean()) < 1
    assert torch.equal(grads[0], grads[1])


@pytest.mark.parametrize('offset', [False, True])
def test_device_draw_eager(offset):
    from graph_detr4d_amd import GridMask
    seed, shape = 0xC0FFEE_0000_0000 + 12345, (2, 3, 12, 20)
    h, w = shape[-2:]
    m = GridMask(True, True, offset=offset, mode=1, prob=0.7).device_draw(seed).train()
    state = [seed & M32, seed >> 32, 0, prob_threshold(0.7)]
    applied = 0
    for step in range(8):
        x = images(shape, 30 + step)
        y = m(x.to(DEV))
        st, blk = m.device_state()
        want_block, state = device_step_ref(state, h, 0.5)
        assert blk.cpu().tolist() == [signed(v) for v in want_block]
        assert [v & M32 for v in st.cpu().tolist()] == state
        apply, d, l, st_h, st_w = want_block[:5]
        applied += apply
        off = device_offset_ref(seed, step, h, w) if offset else None
        want = expect(x, d, l, st_h, st_w, mode=1, offset=off) if apply else x
        assert torch.equal(y.cpu(), want), step
    assert 0 < applied < 8                                                  # this seed's first eight steps hold both decisions
    m.set_prob(0, 10)                                                       # prob 0: the threshold word is rewritten, nothing applies
    torch.cuda.synchronize()
    assert m.device_state()[0].cpu().tolist()[3] == 0
    x = images(shape, 50).to(DEV)
    assert torch.equal(m(x), x)
    assert m.eval()(x) is x


def test_device_draw_captured_graph_draws_a_new_mask_each_replay():
    from graph_detr4d_amd import GridMask
    seed, shape = 0x5EED_0000_0042, (2, 3, 12, 20)
    h, w = shape[-2:]
    m = GridMask(True, True, mode=1, prob=1.0, out_dtype=torch.float16).device_draw(seed).train()
    static_x = torch.zeros(shape, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m(static_x)                                                         # warm-up: step 0
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                           # one stream: draw, then apply
        static_y = m(static_x)
    torch.cuda.synchronize()
    first = m.device_state()[0].cpu().tolist()[2]
    assert first == 1                                                       # capturing runs nothing
    draws = [device_draw_ref(seed, first + k, M32, h, 0.5) for k in range(3)]
    assert len(set(draws)) >= 2                                             # this seed: the three steps do not all share one mask
    masks = []
    for k in range(3):
        x = images(shape, 60 + k)
        static_x.copy_(x.to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        blk = m.device_state()[1].cpu().tolist()
        assert tuple(blk[:5]) == draws[k] and blk[7] == first + k
        _, d, l, st_h, st_w = draws[k]
        assert torch.equal(static_y.cpu(), expect(x, d, l, st_h, st_w, mode=1).to(torch.float16))
        masks.append(static_y.cpu() != 0)
    assert m.device_state()[0].cpu().tolist()[2] == first + 3
    assert sum(not torch.equal(masks[i], masks[j]) for i, j in ((0, 1), (0, 2), (1, 2))) >= 1


def test_feature_extractor_applies_the_mask_in_training_only():
    from graph_detr4d_amd import GridMask, plumbing

    class OneConv(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.conv = torch.nn.Conv2d(3, 4, 3, padding=1)
            self.seen = None

        def forward(self, x):
            self.seen = x
            return [self.conv(x)]

    ext = plumbing.ImageFeatureExtractor(OneConv(), use_grid_mask=True).to(DEV).train()
    img = images((1, 2, 3, 12, 20), 70).to(DEV)
    np.random.seed(0)                                                       # rand() = 0.5488 <= 0.7: the gate passes
    feats = ext(img, [dict()])
    assert len(feats) == 1 and tuple(feats[0].shape) == (1, 2, 4, 12, 20)
    ref = GridMask(True, True, rotate=1, offset=False, ratio=0.5, mode=1, prob=0.7).train()
    np.random.seed(0)
    want = ref(img.view(2, 3, 12, 20))
    assert want is not img and torch.equal(ext.img_backbone.seen, want) and not torch.equal(want, img.view(2, 3, 12, 20))
    ext.eval()
    ext(img, [dict()])
    assert torch.equal(ext.img_backbone.seen, img.view(2, 3, 12, 20)) and ext.img_backbone.seen.data_ptr() == img.data_ptr()
