"""gd4d_adamw_flat / gd4d_adamw_recipe_flat at sizes that are no multiple of 4, through ctypes on 16-byte-aligned buffers.  Python reaches
both only through FlatGradAllReducer(align=4), whose buffers always end on a quad: the `cnt < 4` tails of the two apply kernels, the
scalar tails of the two norm kernels and a range table whose last range ends on a ragged n never run there.  The arbiter is torch's own
clip_grad_norm_ + torch.optim.AdamW in fp64, tolerances as tests/test_head_loss_gpu.py::test_flat_adamw_with_clipping_equals_torch
(norm rtol 1e-5; parameters rtol 1e-5, atol 2e-7).  GPU only."""
import ctypes

import numpy as np
import pytest
import torch

# the word offsets of gd4d_recipe_state (include/gd4d.h) as the package names them
from graph_detr4d_amd.recipe import _F32_NORM, _F32_SCALE, _I32_FOUND_INF, _I64_SKIPPED, _I64_STEPS

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 7, 1025, 524289]
GUARD, SENTINEL = 64, 777.0
# the hyper-parameters as the fp32 values the kernels receive, so the fp64 arbiter evaluates the same function
LR, B1, B2, EPS = (float(np.float32(v)) for v in (2e-4, 0.9, 0.999, 1e-8))
MAX_NORM = 35.0


class _Buffers:
    """p, g, m, v as the first n elements of longer, 16-byte-aligned device buffers whose remaining GUARD elements hold a sentinel:
    a tail that reads or writes a whole quad shows in the guard."""

    def __init__(self, n, seed, pinned=()):
        self.n = n
        gen = torch.Generator().manual_seed(seed)
        self.full = [torch.full((n + GUARD,), SENTINEL).cuda() for _ in range(4)]
        self.p, self.g, self.m, self.v = (t[:n] for t in self.full)
        self.p.copy_(torch.randn(n, generator=gen))
        for i in pinned:                               # parameters of known size where a test reasons about one element
            self.p[i] = 0.1
        self.m.zero_()
        self.v.zero_()
        assert all(t.data_ptr() % 16 == 0 for t in self.full)

    def guards_intact(self):
        return all(bool((t[self.n:] == SENTINEL).all()) for t in self.full)


def _grad(n, step, gen):
    # large enough for the clip to bite on even steps, small enough not to on odd ones
    return torch.randn(n, generator=gen) * (300.0 if step % 2 == 0 else 0.01)


def _arbiter(p0, groups, weight_decay):
    """torch.optim.AdamW over fp64 copies of the slices [begin, end) of p0, one param group per slice."""
    params = [p0[b:e].double().clone().requires_grad_(True) for b, e, _, _ in groups]
    opt = torch.optim.AdamW([dict(params=[q], lr=LR * lm, weight_decay=weight_decay * dm) for q, (_, _, lm, dm) in zip(params, groups)],
                            lr=LR, betas=(B1, B2), eps=EPS, weight_decay=weight_decay)
    return params, opt


def _arbiter_step(params, opt, groups, g):
    for q, (b, e, _, _) in zip(params, groups):
        q.grad = g[b:e].double().clone()
    norm = torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
    opt.step()
    return norm, torch.cat([q.detach() for q in params])


def _assert_close(got, want, what, atol=2e-7):
    torch.testing.assert_close(got.double().cpu(), want, rtol=1e-5, atol=atol, msg=lambda m: f'{what}: {m}')


@pytest.mark.parametrize('n', SIZES)
def test_adamw_flat_ragged_sizes(n):
    from graph_detr4d_amd import _lib
    lib = _lib.load()
    buf = _Buffers(n, n)
    state = torch.zeros(2, device='cuda')
    ws = torch.empty(int(lib.gd4d_adamw_flat_workspace_bytes()), device='cuda', dtype=torch.uint8)
    groups = [(0, n, 1.0, 1.0)]
    params, opt = _arbiter(buf.p.cpu(), groups, 0.01)
    gen = torch.Generator().manual_seed(100 + n)
    for step in range(3):
        g = _grad(n, step, gen)
        buf.g.copy_(g)
        code = lib.gd4d_adamw_flat(buf.p.data_ptr(), buf.g.data_ptr(), buf.m.data_ptr(), buf.v.data_ptr(), state.data_ptr(),
                                   ws.data_ptr(), ws.numel(), n, LR, B1, B2, EPS, 0.01, MAX_NORM,
                                   torch.cuda.current_stream().cuda_stream)
        _lib.check(code, 'gd4d_adamw_flat')
        want_norm, want_p = _arbiter_step(params, opt, groups, g)
        assert float(state[0]) == step + 1
        torch.testing.assert_close(state[1].double().cpu(), want_norm, rtol=1e-5, atol=0)
        _assert_close(buf.p, want_p, f'n {n} step {step} parameters')
        st = opt.state[params[0]]
        _assert_close(buf.m, st['exp_avg'], f'n {n} step {step} exp_avg')
        _assert_close(buf.v, st['exp_avg_sq'], f'n {n} step {step} exp_avg_sq', atol=1e-30)     # a sum of positives: relative
        assert torch.equal(buf.g.cpu(), g), 'gd4d_adamw_flat does not write the gradients'
        assert buf.guards_intact(), 'an element past n was written'


# ---- the recipe variant ----
SCALE = 512.0
WD = 0.5                       # large enough for decay_mult to show: lr * wd = 1e-4 per step against rtol 1e-5
MULTS = [(0.1, 1.0), (1.0, 0.0), (2.5, 3.0)]


def _ranges(n):
    """Up to three ranges over [0, n), every range starting on a quad (the entry point's rule), the last ending on the ragged n;
    for n = 1025 / 524289 the inner borders (340, 684 / 174764, 349528) are no multiple of a block's 1024-element stride."""
    quads = (n + 3) // 4
    k = min(3, quads)
    cuts = [4 * (quads * i // k) for i in range(k)] + [n]
    return [(cuts[i], cuts[i + 1], *MULTS[i + 3 - k]) for i in range(k)]


class _Recipe:
    def __init__(self, n, ranges, zero_grads):
        from graph_detr4d_amd import _lib, recipe as R
        self.lib, self._lib, self.n = _lib.load(), _lib, n
        c = self.cfg = R.RecipeConfig()
        c.base_lr, c.policy, c.by_epoch, c.warmup = LR, R.LR_FIXED, 1, R.WARMUP_NONE
        c.iters_per_epoch = c.max_epochs = c.max_iters = 1
        c.warmup_ratio, c.gamma = 0.1, 0.1
        c.beta1, c.beta2, c.eps, c.weight_decay, c.max_norm = B1, B2, EPS, WD, MAX_NORM
        c.init_scale, c.growth_factor, c.backoff_factor, c.growth_interval, c.dynamic_scale = SCALE, 2.0, 0.5, 2000, 0
        c.zero_grads = int(zero_grads)
        self.host = (R.RecipeRange * len(ranges))(*[R.RecipeRange(*r) for r in ranges])
        self.table = torch.frombuffer(bytearray(bytes(self.host)), dtype=torch.uint8).cuda()
        words = torch.zeros(int(self.lib.gd4d_adamw_recipe_flat_state_bytes()) // 4, dtype=torch.int32)
        words.view(torch.float32)[_F32_SCALE] = SCALE
        self.i32 = words.cuda()
        self.f32, self.i64 = self.i32.view(torch.float32), self.i32.view(torch.int64)
        self.ws = torch.empty(int(self.lib.gd4d_adamw_recipe_flat_workspace_bytes()), device='cuda', dtype=torch.uint8)

    def step(self, buf):
        code = self.lib.gd4d_adamw_recipe_flat(buf.p.data_ptr(), buf.g.data_ptr(), buf.m.data_ptr(), buf.v.data_ptr(), self.i32.data_ptr(),
                                               self.i32.numel() * 4, self.ws.data_ptr(), self.ws.numel(), self.n, ctypes.byref(self.cfg),
                                               self.host, self.table.data_ptr(), len(self.host),
                                               torch.cuda.current_stream().cuda_stream)
        self._lib.check(code, 'gd4d_adamw_recipe_flat')

    counters = property(lambda self: (int(self.i64[_I64_STEPS]), int(self.i64[_I64_SKIPPED]), int(self.i32[_I32_FOUND_INF])))


@pytest.mark.parametrize('n', SIZES)
def test_adamw_recipe_flat_ragged_sizes_and_ranges(n):
    """Three steps, zero_grads on the middle one.  Every element against the arbiter with ITS range's lr_mult / decay_mult; the
    elements on both sides of each border, and the last ragged one, by name.  That the named elements can tell the ranges apart is
    shown on the first step, where Adam's update is lr * lr_mult * sign(g) and the decay p * lr * lr_mult * wd * decay_mult with p set
    to 0.1 there: 2.0e-5 + 1e-6, 2.0e-4 + 0, 5.0e-4 + 7.5e-5 for the three ranges.  Under the multipliers of the NEXT range the
    arbiter moves such an element by at least 1.79e-4 more or less (1.8e-4 -+ 1e-6, 3.0e-4 -+ 7.5e-5, 4.8e-4 -+ 7.4e-5); the tolerance
    there is 1.2e-6, so agreeing with the own range's arbiter excludes the neighbour's.  decay_mult shows in the whole-buffer
    comparison: 7.5e-4 |p| per step in the last range against rtol 1e-5."""
    ranges = _ranges(n)
    assert ranges[0][0] == 0 and ranges[-1][1] == n and all(a[1] == b[0] and b[0] % 4 == 0 for a, b in zip(ranges, ranges[1:]))
    assert len(ranges) == (1 if n < 5 else 2 if n < 9 else 3)
    named = sorted({i for b, e, _, _ in ranges for i in (b, e - 1)})          # first and last element of every range
    buf = _Buffers(n, 2 * n, pinned=named)
    rec = _Recipe(n, ranges, zero_grads=False)
    params, opt = _arbiter(buf.p.cpu(), ranges, WD)
    rotated = [(b, e, *MULTS[(MULTS.index((lm, dm)) + 1) % 3]) for b, e, lm, dm in ranges]
    params_rot, opt_rot = _arbiter(buf.p.cpu(), rotated, WD)
    gen = torch.Generator().manual_seed(200 + n)
    for step in range(3):
        rec.cfg.zero_grads = int(step == 1)
        g = _grad(n, step, gen)
        buf.g.copy_(g * SCALE)                                                # what backward of the scaled loss leaves (exact: 2^9)
        rec.step(buf)
        want_norm, want_p = _arbiter_step(params, opt, ranges, g)
        _, rot_p = _arbiter_step(params_rot, opt_rot, rotated, g)
        assert rec.counters == (step + 1, 0, 0) and float(rec.f32[_F32_SCALE]) == SCALE
        torch.testing.assert_close(rec.f32[_F32_NORM].double().cpu(), want_norm, rtol=1e-5, atol=0)
        got_p = buf.p.double().cpu()
        for i in named:                                                       # by name: both sides of each border, the ragged end
            tol = 1e-5 * abs(float(want_p[i])) + 2e-7
            assert abs(float(got_p[i]) - float(want_p[i])) <= tol, f'n {n} step {step}: element {i} (ranges {ranges})'
            if step == 0:
                assert abs(float(rot_p[i]) - float(want_p[i])) > 1.7e-4 > 100 * tol, f'element {i}: the multipliers do not show'
        _assert_close(buf.p, want_p, f'n {n} step {step} parameters')
        _assert_close(buf.m, torch.cat([opt.state[q]['exp_avg'] for q in params]), f'n {n} step {step} exp_avg')
        _assert_close(buf.v, torch.cat([opt.state[q]['exp_avg_sq'] for q in params]), f'n {n} step {step} exp_avg_sq', atol=1e-30)
        if step == 1:
            assert bool((buf.g == 0).all()), 'zero_grads on an applied step: an element of g (the tail?) is not zero'
        else:
            assert torch.equal(buf.g.cpu(), g * SCALE)
        assert buf.guards_intact(), 'an element past n was written'


@pytest.mark.parametrize('zero_grads', [False, True])
@pytest.mark.parametrize('n', [7, 1025, 524289])
def test_adamw_recipe_flat_inf_in_the_last_ragged_element(n, zero_grads):
    """One applied step, then a step whose only non-finite gradient is the LAST element (in the scalar tail of the norm kernel): it
    must be found, the step skipped (p, m, v and Adam's step count bit for bit as before), and with zero_grads the whole gradient
    buffer - the tail included - zeroed on the skipped path; then an applied step again, whose tail is zeroed as well."""
    ranges = _ranges(n)
    buf = _Buffers(n, 3 * n)
    rec = _Recipe(n, ranges, zero_grads)
    params, opt = _arbiter(buf.p.cpu(), ranges, WD)
    gen = torch.Generator().manual_seed(300 + n)
    g = _grad(n, 1, gen)
    buf.g.copy_(g * SCALE)
    rec.step(buf)
    _, want_p = _arbiter_step(params, opt, ranges, g)
    assert rec.counters == (1, 0, 0)
    _assert_close(buf.p, want_p, 'first step')
    before = [t.clone() for t in (buf.p, buf.m, buf.v)]
    bad = _grad(n, 1, gen) * SCALE
    bad[n - 1] = float('inf')
    buf.g.copy_(bad)
    rec.step(buf)
    assert rec.counters == (1, 1, 1), 'the inf in the last element was not found'
    assert not np.isfinite(float(rec.f32[_F32_NORM]))
    for a, b in zip(before, (buf.p, buf.m, buf.v)):
        assert torch.equal(a, b)
    if zero_grads:
        assert bool((buf.g == 0).all()), 'skipped step: the gradient tail is not zero'
    else:
        assert torch.equal(buf.g.cpu(), bad)
    assert buf.guards_intact()
    g = _grad(n, 0, gen)
    buf.g.copy_(g * SCALE)
    rec.step(buf)
    _, want_p = _arbiter_step(params, opt, ranges, g)
    assert rec.counters == (2, 1, 0)
    _assert_close(buf.p, want_p, 'the step after the skipped one')
    assert bool((buf.g == 0).all()) if zero_grads else torch.equal(buf.g.cpu(), g * SCALE)
    assert buf.guards_intact()
