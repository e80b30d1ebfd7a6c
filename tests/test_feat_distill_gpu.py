"""MixDistill's feature-distillation loss on gd4d_feat_distill.hip: the reference's fixtures, ragged pixel tails against the fp64
restatement (tests/feat_distill_ref.py), the bias and weight paths with an exactly-zero loss, run-to-run bits, the torch-op route and a
captured graph.  GPU only; a few seconds in all (the largest level is 16 x 29 on 3 cameras).

Tolerances: the loss at the kernels' 1e-4 relative; gradients at the training tests' relative Frobenius error <= 1e-3 against fp64;
the two routes of the module against each other at 2e-4 (of the loss / of a gradient's largest entry)."""
import functools

import numpy as np
import pytest
import torch

from feat_distill_ref import feat_distill_ref
from golden_io import Golden

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
# 1 x 1 (a single pixel), 1 x 2, 5 x 7 (less than one 64-pixel tile), 15 x 25 = 375 (5 tiles + 55), 16 x 29 = 464 (7 tiles + 16; the weight
# gradient's 32-pixel chunks: 14 + 16)
RAGGED = [(1, 2), (5, 7), (15, 25), (16, 29), (1, 1)]


def _frob(got, ref):
    ref = np.asarray(ref, dtype=np.float64).ravel()
    return float(np.linalg.norm(got.detach().double().cpu().numpy().ravel() - ref) / np.linalg.norm(ref))


def _module(kind, loss_weight, num_levels, seed, torch_ops=False):
    from graph_detr4d_amd import FeatureDistillLoss
    torch.manual_seed(seed)
    return FeatureDistillLoss(dict(type=kind, loss_weight=loss_weight), num_levels=num_levels, torch_ops=torch_ops).to(DEV)


def _pyramids(levels, r, seed, batch=1):
    """Teacher magnitudes vary by camera, channel and pixel: neither attention softmax is near uniform."""
    g = torch.Generator().manual_seed(seed)
    n = r // batch
    teacher, student = [], []
    for h, w in levels:
        t = torch.randn(batch, n, 256, h, w, generator=g)
        t = t * (0.25 + 2.0 * torch.rand(batch, n, 256, 1, 1, generator=g)) * (0.25 + 2.0 * torch.rand(batch, n, 1, h, w, generator=g))
        teacher.append(t)
        student.append(torch.randn(batch, n, 256, h, w, generator=g))
    return teacher, student


def _run(mod, teacher, student):
    """One forward + backward: (loss, [d student_l], [d weight_l], [d bias_l]), the module's .grad fields left untouched."""
    s = [x.to(DEV).requires_grad_() for x in student]
    loss = mod([x.to(DEV) for x in teacher], s)['feat_loss']
    nl = len(teacher)
    params = [mod.lateral_convs[l].weight for l in range(nl)] + [mod.lateral_convs[l].bias for l in range(nl)]
    grads = torch.autograd.grad(loss, s + params)
    return loss.detach(), list(grads[:nl]), list(grads[nl:2 * nl]), list(grads[2 * nl:])


def _check(got, ref, what):
    loss, gx, gw, gb = got
    rloss, rx, rw, rb = ref
    err = abs(float(loss) - rloss) / abs(rloss)
    figures = [f'loss {err:.2e}']
    fails = [] if err <= 1e-4 else [f'loss {err:.2e}']
    for l in range(len(rx)):
        for name, a, b in ((f'dx{l}', gx[l], rx[l]), (f'dw{l}', gw[l], rw[l]), (f'db{l}', gb[l], rb[l])):
            e = _frob(a, b)
            figures.append(f'{name} {e:.2e}')
            if not e <= 1e-3:
                fails.append(f'{name} {e:.2e}')
    print(what, ' '.join(figures))
    assert not fails, (what, fails)


@pytest.mark.parametrize('name', ['feat_distill_vanilla', 'feat_distill_attention'])
def test_reference_fixtures(name):
    torch.manual_seed(11)
    g = Golden(name)
    m = g.meta
    nl = len(m['levels'])
    mod = _module(m['type'], m['loss_weight'], nl, 11)
    mod.load_state_dict({k: g.t(k) for k in g.arrays if k.startswith('lateral_convs.')}, strict=True)
    got = _run(mod, [g.t(f'teacher{l}') for l in range(nl)], [g.t(f'student{l}') for l in range(nl)])
    ref = (float(g.t('feat_loss')), [g.arrays[f'grad_student{l}'] for l in range(nl)], [g.arrays[f'grad_weight{l}'] for l in range(nl)],
           [g.arrays[f'grad_bias{l}'] for l in range(nl)])
    assert got[0].dim() == 0 and got[1][0].shape == g.t('student0').shape and got[2][0].shape == (256, 256, 1, 1)
    _check(got, ref, name)


@functools.lru_cache(maxsize=None)
def _ragged_case(kind):
    """Inputs, conv state and the fp64 reference of the ragged case, computed once per type and shared (never modified)."""
    teacher, student = _pyramids(RAGGED, 3, 21)
    mod = _module(kind, 1.5, len(RAGGED), 22)
    w = [c.weight.detach().cpu().numpy() for c in mod.lateral_convs]
    b = [c.bias.detach().cpu().numpy() for c in mod.lateral_convs]
    ref = feat_distill_ref([t.numpy() for t in teacher], [s.numpy() for s in student], w, b, kind, 1.5)
    return teacher, student, mod, ref


@pytest.mark.parametrize('kind', ['vanilla', 'attention'])
def test_ragged_pixel_tails(kind):
    torch.manual_seed(23)
    teacher, student, mod, ref = _ragged_case(kind)
    got = _run(mod, teacher, student)
    _check(got, ref, f'ragged {kind}')
    # each camera's slice on its own: a tile that spilled into the next camera would be lost in the whole tensor's norm at the small
    # levels' sizes, not here
    for l, (h, w) in enumerate(RAGGED):
        for cam in range(3):
            e = _frob(got[1][l][0, cam], ref[1][l][0, cam])
            assert e <= 1e-3, (kind, l, cam, e)
            assert float(np.abs(ref[1][l][0, cam]).max()) > 0


def test_bias_and_weight_paths_give_exact_zeros():
    """Level 0: zero weight, non-zero bias - the converted student is the bias.  Level 1: identity weight, zero bias - it is the student
    itself; the student's values are multiples of 1/8 below 64, which a bf16 hi + lo pair holds exactly, and every output is ONE
    product, so the split-bf16 product returns them exactly.  With the teacher equal to the converted student every difference is an
    exact 0: loss and all gradients are 0 bit for bit (vanilla).  Then the teacher is moved by 0.5: every difference is 0.5 exactly."""
    torch.manual_seed(31)
    g = torch.Generator().manual_seed(31)
    mod = _module('vanilla', 3.0, 2, 31)
    bias = torch.randn(256, generator=g)
    with torch.no_grad():
        mod.lateral_convs[0].weight.zero_()
        mod.lateral_convs[0].bias.copy_(bias)
        mod.lateral_convs[1].weight.copy_(torch.eye(256).view(256, 256, 1, 1))
        mod.lateral_convs[1].bias.zero_()
    student = [torch.randn(1, 3, 256, 5, 7, generator=g), torch.randint(-511, 512, (1, 3, 256, 9, 11), generator=g) / 8.0]
    teacher = [bias.view(1, 1, 256, 1, 1).expand(1, 3, 256, 5, 7).contiguous(), student[1].clone()]
    loss, gx, gw, gb = _run(mod, teacher, student)
    assert float(loss) == 0.0
    for t in gx + gw + gb:
        assert torch.count_nonzero(t) == 0
    loss, gx, gw, gb = _run(mod, [t + 0.5 for t in teacher], student)
    assert abs(float(loss) - 3.0 * 0.25) <= 1e-6 * 0.75                   # (0.25 + 0.25) / 2 levels * loss_weight
    for l, hw in enumerate((35, 99)):
        want = -3.0 / (2 * 3 * 256 * hw)                                     # 2 coef (s - t) = -coef, summed over cameras and pixels
        torch.testing.assert_close(gb[l], torch.full_like(gb[l], want * 3 * hw), rtol=1e-5, atol=0)


@pytest.mark.parametrize('kind', ['vanilla', 'attention'])
def test_two_runs_give_the_same_bits(kind):
    torch.manual_seed(41)
    teacher, student, mod, _ = _ragged_case(kind)
    a, b = _run(mod, teacher, student), _run(mod, teacher, student)
    assert torch.equal(a[0], b[0])
    for x, y in zip(a[1] + a[2] + a[3], b[1] + b[2] + b[3]):
        assert torch.equal(x, y)


@pytest.mark.parametrize('kind', ['vanilla', 'attention'])
def test_torch_op_route_agrees(kind):
    from graph_detr4d_amd import functional as Fn
    torch.manual_seed(51)
    teacher, student, mod, _ = _ragged_case(kind)
    hip = _run(mod, teacher, student)
    with Fn.torch_ops_for(mod):
        ops = _run(mod, teacher, student)
    assert abs(float(hip[0]) - float(ops[0])) <= 2e-4 * abs(float(ops[0]))
    for x, y in zip(hip[1] + hip[2] + hip[3], ops[1] + ops[2] + ops[3]):
        assert x.shape == y.shape
        assert float((x - y).abs().max()) <= 2e-4 * float(y.abs().max())


@pytest.mark.parametrize('kind', ['vanilla', 'attention'])
def test_captured_graph_replays_on_new_inputs(kind):
    torch.manual_seed(61)
    levels = [(5, 7), (9, 11), (1, 1)]
    mod = _module(kind, 2.0, len(levels), 61)
    t0, s0 = _pyramids(levels, 2, 62)
    t1, s1 = _pyramids(levels, 2, 63)
    st = [x.to(DEV) for x in t0]
    ss = [x.to(DEV).requires_grad_() for x in s0]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):                                                   # warm-up outside the capture (no .grad is written)
            torch.autograd.grad(mod(st, ss)['feat_loss'], ss + list(mod.parameters()))
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                            # forward + backward, one capture stream
        loss = mod(st, ss)['feat_loss']
        loss.backward()
    want = _run(mod, t1, s1)                                                 # eager, on inputs the capture never saw
    with torch.no_grad():
        for dst, src in zip(st + ss, t1 + s1):
            dst.copy_(src)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(loss.detach(), want[0])
    nl = len(levels)
    for l in range(nl):
        assert torch.equal(ss[l].grad, want[1][l])
        assert torch.equal(mod.lateral_convs[l].weight.grad, want[2][l])
        assert torch.equal(mod.lateral_convs[l].bias.grad, want[3][l])
    assert float(want[0]) > 0 and float(want[1][0].abs().max()) > 0


def test_teacher_that_requires_grad_is_refused():
    torch.manual_seed(71)
    mod = _module('attention', 1.0, 1, 71)
    t, s = _pyramids([(3, 5)], 2, 72)
    with pytest.raises(ValueError, match='detached'):
        mod([t[0].to(DEV).requires_grad_()], [s[0].to(DEV).requires_grad_()])
    out = mod([t[0].to(DEV)], [s[0].to(DEV).requires_grad_()])
    assert list(out) == ['feat_loss']
