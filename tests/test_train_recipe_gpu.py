"""TrainRecipe.step (gd4d_adamw_recipe_flat: schedule, loss scale, skip-on-overflow, clip, per-group AdamW from device state) against
adamw_step (bit for bit where the two coincide), against torch.amp.GradScaler + clip_grad_norm_ + torch.optim.AdamW as arbiter,
inside a replayed hipGraph, across a save / resume and across two ranks.  GPU only."""
import copy
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

OPTIMIZER = dict(type='AdamW', lr=2e-4, paramwise_cfg=dict(custom_keys={'0.': dict(lr_mult=0.1)}), weight_decay=0.01)   # '0.': the first Linear
OPTIMIZER_CONFIG = dict(grad_clip=dict(max_norm=35, norm_type=2))
LR_CONFIG = dict(policy='CosineAnnealing', warmup='linear', warmup_iters=3, warmup_ratio=1.0 / 3, min_lr_ratio=1e-3)
FP16 = dict(loss_scale=512.)
SMALL_RUN = dict(max_epochs=4, iters_per_epoch=2)


def _net(seed=0):
    torch.manual_seed(seed)
    # (no normalisation after the last Linear: see test_flat_adamw_with_clipping_equals_torch)
    return torch.nn.Sequential(torch.nn.Linear(64, 96), torch.nn.LayerNorm(96), torch.nn.ReLU(), torch.nn.Linear(96, 33)).cuda()


def _recipe(net, **kw):
    from graph_detr4d_amd import TrainRecipe, dist as D
    red = D.FlatGradAllReducer(list(net.parameters()), align=4)
    red.bind()
    args = dict(optimizer=OPTIMIZER, optimizer_config=OPTIMIZER_CONFIG, lr_config=LR_CONFIG, fp16=FP16, **SMALL_RUN)
    args.update(kw)
    return TrainRecipe(red, net.named_parameters(), **args), red


def _input(step, inf=False):
    x = torch.randn(16, 64, device='cuda') * (300.0 if step % 2 == 0 else 0.01)
    if inf:
        x[2, 7] = float('inf')
    return x


def _ulps(a, b):
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


def test_fixed_rate_scale_one_is_adamw_step_bit_for_bit():
    """The regression anchor, tolerance zero: fp16=None (scale 1), policy 'fixed', one group - the same arithmetic in the same order
    as gd4d_adamw_flat (x 1.0 is exact), five steps on test_flat_adamw_with_clipping_equals_torch's network."""
    from graph_detr4d_amd import dist as D
    net = _net()
    ref = copy.deepcopy(net)
    rec, red = _recipe(net, optimizer=dict(type='AdamW', lr=2e-4, weight_decay=0.01), lr_config=dict(policy='fixed'), fp16=None)
    red_ref = D.FlatGradAllReducer(list(ref.parameters()), align=4)
    red_ref.bind()
    for step in range(5):
        x = _input(step)
        red.zero_grad()
        red_ref.zero_grad()
        rec.scale(net(x).square().sum()).backward()
        ref(x).square().sum().backward()
        rec.step()
        red_ref.adamw_step(lr=2e-4, weight_decay=0.01, max_norm=35.0)
        m, v = rec.state()[:2]
        assert torch.equal(rec.last_grad_norm, red_ref.last_grad_norm)
        assert torch.equal(red.flat_params, red_ref.flat_params)
        assert torch.equal(m, red_ref._adam[0]) and torch.equal(v, red_ref._adam[1])
        assert int(rec.optimizer_steps) == int(red_ref._adam[2][0]) == step + 1 and int(rec.found_inf) == 0
        assert float(rec.lr) == float(np.float32(2e-4)) and float(rec.loss_scale) == 1.0


def _arbiter(net, rec, red):
    """torch's own recipe on the CPU, seeded from the device: parameters, Adam's moments and step count."""
    arb = copy.deepcopy(net).cpu()
    params = list(arb.parameters())
    opt = torch.optim.AdamW([dict(params=params[:2]), dict(params=params[2:])], lr=2e-4, weight_decay=0.01)
    m, v = rec.state()[:2]
    t = float(int(rec.optimizer_steps))
    for p, off in zip(params, red._offsets):
        opt.state[p] = dict(step=torch.tensor(t), exp_avg=m[off:off + p.numel()].view_as(p).cpu().clone(),
                            exp_avg_sq=v[off:off + p.numel()].view_as(p).cpu().clone())
    return arb, params, opt


def test_reference_recipe_against_torch_with_a_skipped_step():
    """The reference's four dicts (warmup_iters 3, 2 iterations per epoch, 4 epochs; lr_mult 0.1 on the first Linear; static scale
    512) against GradScaler('cpu', init_scale=512.) + clip_grad_norm_ + AdamW with two param groups whose lr is set from
    recipe.lr_at(it), then scaler.update(512.).  The arbiter receives the device's scaled gradients, so only the optimizer is compared.
    Eight iterations, an inf in the input of iteration 4: that step is skipped on both sides.  Tolerances: tests/test_head_loss_gpu.py's
    for this comparison over five applied steps (norm rtol 1e-5; parameters rtol 1e-5, atol 2e-7); the arbiter is re-seeded from the
    device after the skipped iteration, so no window has more than five applied steps.  The lr word: within 2 fp32 ulps of
    float32(lr_at(it)) - one for a last-bit difference of the double cosine, one for the order of the multiplies."""
    net = _net()
    rec, red = _recipe(net)
    assert [(b, e) for b, e, _, _ in rec.ranges] == [(0, 64 * 96 + 96), (64 * 96 + 96, red.numel)]
    assert len(rec.ranges) == 2 and rec.ranges[0][2:] == (0.1, 1.0) and rec.ranges[1][2:] == (1.0, 1.0)
    rec.state()
    arb, params, opt = _arbiter(net, rec, red)
    scaler = torch.amp.GradScaler('cpu', init_scale=512.)
    applied = 0
    for it in range(8):
        rec.scale(net(_input(it, inf=(it == 4))).square().sum()).backward()
        assert float(rec.loss_scale) == 512.0
        for p, q in zip(params, net.parameters()):
            p.grad = q.grad.detach().cpu().clone()
        before = [t.clone() for t in (red.flat_params,) + tuple(rec.state()[:2])]
        before_arb = [p.detach().clone() for p in params]
        rec.step(zero_grads=True)
        lr = rec.lr_at(it)
        opt.param_groups[0]['lr'], opt.param_groups[1]['lr'] = lr * 0.1, lr
        scaler.scale(torch.zeros(()))
        scaler.unscale_(opt)
        want_norm = torch.nn.utils.clip_grad_norm_(params, 35.0)
        scaler.step(opt)
        scaler.update(512.)
        assert scaler.get_scale() == 512.0 and float(rec.loss_scale) == 512.0
        print(f'it {it}: lr word {float(rec.lr):.9e} want {lr:.9e} ulps {_ulps(float(rec.lr), lr)} norm {float(rec.last_grad_norm):.6e} '
              f'want {float(want_norm):.6e} found_inf {int(rec.found_inf)}')
        assert _ulps(float(rec.lr), lr) <= 2
        assert int(rec.iteration) == it + 1
        assert bool((red.flat[:red.numel] == 0).all())                         # zero_grads
        if it == 4:
            assert not np.isfinite(float(rec.last_grad_norm)) and not bool(torch.isfinite(want_norm))
            assert int(rec.found_inf) == 1 and int(rec.skipped_steps) == 1 and int(rec.optimizer_steps) == 4
            for a, b in zip(before, (red.flat_params,) + tuple(rec.state()[:2])):
                assert torch.equal(a, b)
            for a, p in zip(before_arb, params):                               # the arbiter skipped as well
                assert torch.equal(a, p) and float(opt.state[p]['step']) == 4.0
            arb, params, opt = _arbiter(net, rec, red)                         # next window
            applied = 0
            continue
        applied += 1
        assert applied <= 5 and int(rec.found_inf) == 0
        torch.testing.assert_close(rec.last_grad_norm.cpu(), want_norm, rtol=1e-5, atol=0)
        for q, p in zip(net.parameters(), params):
            torch.testing.assert_close(q.detach().cpu(), p.detach(), rtol=1e-5, atol=2e-7)
    assert int(rec.optimizer_steps) == 7 and int(rec.skipped_steps) == 1 and int(rec.iteration) == 8


def test_dynamic_scale_follows_gradscaler_and_a_step_unscales_with_the_scale_it_was_seeded_with():
    net = _net()
    rec, red = _recipe(net, fp16=dict(loss_scale=dict(init_scale=1024., growth_interval=3)))
    rec.state()
    dummy = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([dummy], lr=0.0)
    scaler = torch.amp.GradScaler('cpu', init_scale=1024., growth_interval=3)
    scales = []
    for it in range(10):
        overflow = it in (2, 7)
        seeded = float(rec.loss_scale)
        rec.scale(net(_input(it, inf=overflow)).square().sum()).backward()
        grads = red.flat[:red.numel].double().clone()
        rec.step(zero_grads=True)
        dummy.grad = torch.full((1,), float('inf') if overflow else 1.0)
        scaler.scale(torch.zeros(()))
        scaler.unscale_(opt)
        scaler.step(opt)
        scaler.update()
        scales.append(float(rec.loss_scale))
        assert float(rec.loss_scale) == scaler.get_scale(), (it, scales)       # powers of two: exactly
        assert int(rec.growth_tracker) == scaler._get_growth_tracker()
        assert int(rec.found_inf) == int(overflow) and float(rec.scale_in_use) == seeded
        if not overflow:                                                       # the norm is of grad / the scale of THIS iteration
            torch.testing.assert_close(rec.last_grad_norm.double().cpu(), (grads / seeded).norm().cpu(), rtol=1e-5, atol=0)
    assert scales == [1024., 1024., 512., 512., 512., 1024., 1024., 512., 512., 512.]
    assert int(rec.skipped_steps) == 2 and int(rec.optimizer_steps) == 8


def test_replayed_graph_follows_schedule_and_skips():
    """state(), then ONE captured scale -> backward -> step(zero_grads=True) (no fill of the gradient buffer in the graph) replayed
    eight times, an inf in the static input of the fifth: equal to eight eager steps on a copy (rtol 1e-5, atol 1e-7 as
    test_flat_adamw_inside_a_replayed_graph_keeps_its_state); the lr word changes from replay to replay."""
    net = _net(1)
    ref = copy.deepcopy(net)
    rec, red = _recipe(net)
    rec_ref, red_ref = _recipe(ref)
    x = torch.randn(16, 64, device='cuda')
    clean = x.clone()

    def step(model, r):
        r.scale(model(x).square().sum()).backward()
        r.step(zero_grads=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        net(x).square().sum().backward()                          # warm-up of autograd on the capture stream (no optimizer step)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    red.zero_grad()
    g_bad = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match=r'state\(\)'):
        with torch.cuda.graph(g_bad, capture_error_mode='thread_local'):
            step(net, rec)
    torch.cuda.synchronize()
    rec.state()
    red.zero_grad()
    versions = [p._version for p in net.parameters()]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode='thread_local'):
        step(net, rec)
    rates = []
    for it in range(8):
        x.copy_(clean)
        if it == 4:
            x[2, 7] = float('inf')
        graph.replay()
        rates.append(float(rec.lr))
        assert int(rec.found_inf) == int(it == 4)
    for it in range(8):
        x.copy_(clean)
        if it == 4:
            x[2, 7] = float('inf')
        step(ref, rec_ref)
        assert _ulps(rates[it], float(rec_ref.lr)) == 0
    torch.cuda.synchronize()
    for p, r in zip(net.parameters(), ref.parameters()):
        torch.testing.assert_close(p, r, rtol=1e-5, atol=1e-7)
    assert len(set(rates)) >= 4, rates
    assert (int(rec.iteration), int(rec.optimizer_steps), int(rec.skipped_steps)) == (8, 7, 1)
    assert bool((red.flat[:red.numel] == 0).all())
    red.after_replays()
    assert all(p._version > v for p, v in zip(net.parameters(), versions))


def test_state_dict_resumes_bit_for_bit():
    net = _net(2)
    rec, red = _recipe(net, fp16=dict(loss_scale=dict(init_scale=1024., growth_interval=2)))
    torch.manual_seed(5)
    xs = [_input(i, inf=(i == 1)) for i in range(6)]

    def run(model, r, inputs):
        for x in inputs:
            r.scale(model(x).square().sum()).backward()
            r.step(zero_grads=True)
    run(net, rec, xs[:3])
    sd = rec.state_dict()
    assert (sd['iteration'], sd['optimizer_steps'], sd['skipped_steps'], sd['loss_scale']) == (3, 2, 1, 512.0)
    snapshot = copy.deepcopy(net)
    run(net, rec, xs[3:])
    rec2, red2 = _recipe(snapshot, fp16=dict(loss_scale=dict(init_scale=1024., growth_interval=2)))
    rec2.load_state_dict(sd)
    run(snapshot, rec2, xs[3:])
    assert torch.equal(red.flat_params, red2.flat_params)
    for a, b in zip(rec.state()[:3], rec2.state()[:3]):                        # exp_avg, exp_avg_sq, every state word
        assert torch.equal(a, b)
    assert (int(rec2.iteration), int(rec2.optimizer_steps), int(rec2.skipped_steps)) == (6, 5, 1)
    rec2.set_progress(4)
    assert int(rec2.iteration) == 4


def test_two_ranks_take_the_same_decision(repo_root, tmp_path):
    """Two processes on the one GPU over gloo; rank 1's local gradient has an inf, rank 0's does not.  After reduce() both see it,
    both skip, the parameters stay equal (and unchanged); the next iteration both step.  Each rank under its own time limit."""
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    procs, outs = [], []
    for rank in range(2):
        out = str(tmp_path / f'rank{rank}.json')
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE='2', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY='0')
        procs.append(subprocess.Popen(['timeout', '-k', '10', '240', sys.executable, os.path.join(repo_root, 'tests', 'train_recipe_rank.py'), out],
                                      cwd=repo_root, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
        outs.append(out)
    logs = [p.communicate()[0] for p in procs]
    assert [p.returncode for p in procs] == [0, 0], logs
    r0, r1 = (json.load(open(o)) for o in outs)
    assert (r0['rank'], r1['rank'], r0['world']) == (0, 1, 2) and r0['initial'] == r1['initial']
    a0, a1 = r0['steps'][0], r1['steps'][0]
    assert a0['local_finite'] and not a1['local_finite']
    for a in (a0, a1):
        assert (a['found_inf'], a['skipped_steps'], a['optimizer_steps'], a['iteration']) == (1, 1, 0, 1) and a['grads_zero']
        assert a['params'] == r0['initial']
    b0, b1 = r0['steps'][1], r1['steps'][1]
    for b in (b0, b1):
        assert (b['found_inf'], b['skipped_steps'], b['optimizer_steps'], b['iteration']) == (0, 1, 1, 2)
    assert b0['params'] == b1['params'] != r0['initial']
