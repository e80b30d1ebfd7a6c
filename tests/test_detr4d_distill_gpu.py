"""Detr4D_Distiller's instance term on the device: gd4d_distill_match_cost_fwd, gd4d_lsa_dense_fwd and gd4d_distill_loss_fwd_bwd
against the reference fixtures and the host solver, and the whole term inside one captured graph.  GPU only."""
import numpy as np
import pytest
import torch

from golden_io import Golden

pytestmark = pytest.mark.gpu
CASES = ['detr4d_distill_b1_rw', 'detr4d_distill_b2', 'detr4d_distill_fewer_teacher', 'detr4d_distill_degenerate']


def _cfg(m):
    return dict(loss_cls_distill=dict(type='DistillCrossEntropyLoss', use_sigmoid=True, loss_weight=m['loss_cls_weight']),
                loss_reg_distill=dict(type='L1Loss', loss_weight=m['loss_reg_weight']), reweight_score=m['reweight_score'],
                code_weights=m['code_weights'], pc_range=m['pc_range'])


def _unpack(assigned, b, qt):
    """solver output (b * Qt + t, or -1) -> the reference's gt_inds (t + 1, or 0)"""
    a = assigned.long().cpu()
    off = (torch.arange(b) * qt).view(1, b, 1)
    return torch.where(a >= 0, a - off + 1, torch.zeros_like(a))


@pytest.mark.parametrize('name', CASES)
def test_cost_assignment_loss_and_gradients_match_reference(name):
    from graph_detr4d_amd import get_instance_distill_loss, ops
    g = Golden(name)
    m = g.meta
    nl, b, qs, qt = m['num_layers'], m['batch'], m['num_student'], m['num_teacher']
    t_cls, t_box = g.t('t_cls').cuda(), g.t('t_box').cuda()
    s_cls, s_box = g.t('s_cls').cuda().requires_grad_(), g.t('s_box').cuda().requires_grad_()
    cost = ops.distill_match_cost_fwd(s_cls.detach(), s_box.detach(), t_cls, t_box, 1.0, 0.25).cpu()
    for l in range(nl):
        for i in range(b):
            off = qs * (l * b * qt + i * qt)
            got, want = cost[off:off + qs * qt].view(qs, qt), g.t(f'cost_l{l}_b{i}')
            assert torch.equal(torch.isinf(got), torch.isinf(want))
            fin = torch.isfinite(want)
            torch.testing.assert_close(got[fin], want[fin], rtol=1e-5, atol=1e-5)
    out = get_instance_distill_loss(dict(all_cls_scores=t_cls, all_bbox_preds=t_box), dict(all_cls_scores=s_cls, all_bbox_preds=s_box),
                                    **_cfg(m))
    get_instance_distill_loss.last_assigner.check_status()
    gt_inds = _unpack(get_instance_distill_loss.last_assigned, b, qt)
    for l in range(nl):
        for i in range(b):
            assert torch.equal(gt_inds[l, i], g.t(f'assigned_l{l}_b{i}').long())
    keys = m['loss_keys']
    got = torch.stack([out[k] for k in keys]).cpu()
    torch.testing.assert_close(got, g.t('losses'), rtol=1e-5, atol=1e-5)
    sum(out.values()).backward()
    for t, ref in ((s_cls.grad, g.t('grad_s_cls')), (s_box.grad, g.t('grad_s_box'))):
        torch.testing.assert_close(t.cpu(), ref, rtol=0, atol=1e-4 * float(ref.abs().max()))
    assert t_cls.grad is None and t_box.grad is None


def family_costs(n_problems, rows, cols, family, seed, dev='cuda'):
    """seeded L1 costs between 8-d points: 'independent' student / teacher, or 'noise' (student = teacher + noise, rows permuted)"""
    g = torch.Generator(device=dev).manual_seed(seed)
    t = torch.randn(n_problems, cols, 8, device=dev, generator=g)
    if family == 'independent':
        s = torch.randn(n_problems, rows, 8, device=dev, generator=g)
    else:
        perm = torch.argsort(torch.rand(n_problems, cols, device=dev, generator=g), dim=1)[:, :rows]
        s = torch.gather(t, 1, perm[..., None].expand(-1, -1, 8)) + 0.05 * torch.randn(n_problems, rows, 8, device=dev, generator=g)
    # (one problem at a time, summed explicitly: a batched torch.cdist of this size came back partly zero on the GPU)
    return torch.stack([(s[i][:, None, :] - t[i][None, :, :]).abs().sum(-1) for i in range(n_problems)]).contiguous()


def _solve_both(cost):
    """(device assignment, host assignment) of P problems (P, Q, G) in hungarian_assign_fwd's layout (one layer, P samples)."""
    from graph_detr4d_amd import ops
    p, q, gcols = cost.shape
    flat = cost.permute(0, 1, 2).reshape(-1).contiguous()             # block b at Q * (b * G) = (Q, G) row-major
    start = torch.arange(0, (p + 1) * gcols, gcols, dtype=torch.int32, device=cost.device)
    dev_a, status = ops.lsa_dense_fwd(flat, start, 1, p, q, p * gcols, gcols)
    host = ops.linear_sum_assignment_batch(flat.cpu().numpy(), [(q * b * gcols, q, gcols) for b in range(p)], num_threads=8)
    host = torch.from_numpy(np.stack(host)).view(1, p, q)
    host = torch.where(host >= 0, host + (torch.arange(p) * gcols).view(1, p, 1).int(), host)
    return dev_a.cpu(), status.cpu(), host


@pytest.mark.parametrize('family', ['independent', 'noise'])
def test_dense_solver_equals_host_solver_900(family):
    for chunk in range(5):                                                # 5 x 52 = 260 problems per family
        cost = family_costs(52, 900, 900, family, seed=100 * chunk + (family == 'noise'))
        dev_a, status, host = _solve_both(cost)
        assert (status == 0).all()
        if not torch.equal(dev_a, host):
            c = cost.cpu().double()
            bad = [i for i in range(cost.shape[0]) if not torch.equal(dev_a[0, i], host[0, i])]
            tot = [(i, float(c[i, torch.arange(900), dev_a[0, i].long() - i * 900].sum()),
                    float(c[i, torch.arange(900), host[0, i].long() - i * 900].sum())) for i in bad]
            raise AssertionError(f'{family} chunk {chunk}: problems {bad} differ; (problem, device total, host total) {tot}')


@pytest.mark.parametrize('shape', [(900, 300), (300, 900), (1, 1), (2, 2), (37, 64)])
def test_dense_solver_rectangular(shape):
    cost = family_costs(6, shape[0], shape[1], 'independent', seed=shape[0] * 7 + shape[1])
    dev_a, status, host = _solve_both(cost)
    assert (status == 0).all()
    assert torch.equal(dev_a, host)


def test_dense_solver_ties_reach_the_optimum():
    g = torch.Generator(device='cuda').manual_seed(5)
    cost = torch.randint(0, 4, (8, 200, 200), generator=g, device='cuda').float()
    dev_a, status, host = _solve_both(cost)
    assert (status == 0).all()
    c = cost.cpu()
    for b in range(8):
        cols_d, cols_h = dev_a[0, b].long() - b * 200, host[0, b].long() - b * 200
        assert sorted(cols_d.tolist()) == list(range(200))
        td = float(c[b, torch.arange(200), cols_d].double().sum())
        th = float(c[b, torch.arange(200), cols_h].double().sum())
        assert abs(td - th) <= 1e-9 * max(abs(th), 1.0)


def test_dense_solver_nan_sets_status_1_and_spares_neighbours():
    cost = family_costs(3, 64, 64, 'independent', seed=9)
    cost[1, 5, 7] = float('nan')
    from graph_detr4d_amd import ops
    flat = cost.reshape(-1).contiguous()
    start = torch.arange(0, 4 * 64, 64, dtype=torch.int32, device='cuda')
    a, st = ops.lsa_dense_fwd(flat, start, 1, 3, 64, 192, 64)
    assert st.cpu().tolist() == [0, 1, 0]
    assert (a[0, 1] == -1).all()
    ok = cost.clone()
    ok[1] = 0
    a2, _ = ops.lsa_dense_fwd(ok.reshape(-1).contiguous(), start, 1, 3, 64, 192, 64)
    assert torch.equal(a[0, 0], a2[0, 0]) and torch.equal(a[0, 2], a2[0, 2])


def _term_inputs(seed, nl=6, b=2, q=900, dev='cuda'):
    g = torch.Generator(device=dev).manual_seed(seed)
    t_cls = torch.randn(nl, b, q, 10, device=dev, generator=g) * 2 - 1
    t_box = torch.randn(nl, b, q, 10, device=dev, generator=g) * 0.5
    s_cls = torch.randn(nl, b, q, 10, device=dev, generator=g) * 2 - 1
    s_box = torch.randn(nl, b, q, 10, device=dev, generator=g) * 0.5
    return t_cls, t_box, s_cls, s_box


CFG = dict(loss_cls_distill=dict(type='DistillCrossEntropyLoss', use_sigmoid=True, loss_weight=1.0),
           loss_reg_distill=dict(type='L1Loss', loss_weight=0.25), reweight_score=True)


def test_whole_term_in_one_captured_graph_equals_eager():
    from graph_detr4d_amd import distill, get_instance_distill_loss
    ins = [t.clone() for t in _term_inputs(1)]
    cw = torch.tensor([1.0] * 8 + [0.2, 0.2], device='cuda')
    avg = distill.distill_normalisers(2, 900, 900, device='cuda')
    asg = distill.DistillHungarianAssigner3D(cls_cost=dict(type='DistillCrossEntropyLossCost', weight=1.0),
                                             reg_cost=dict(type='BBox3DL1Cost', weight=0.25))

    def step():
        out = get_instance_distill_loss(dict(all_cls_scores=ins[0], all_bbox_preds=ins[1]), dict(all_cls_scores=ins[2], all_bbox_preds=ins[3]),
                                        code_weights=cw, avg_factors=avg, distill_assigner=asg, **CFG)
        return torch.stack(list(out.values())), get_instance_distill_loss.last_assigned
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()                                                            # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_loss, g_assigned = step()
    second = _term_inputs(2)
    for dst, src in zip(ins, second):
        dst.copy_(src)
    graph.replay()
    torch.cuda.synchronize()
    asg.check_status()
    e_loss, e_assigned = step()
    assert torch.equal(g_assigned, e_assigned)
    assert torch.equal(g_loss, e_loss)
    assert (g_assigned >= 0).all()


def test_device_route_equals_host_route():
    from graph_detr4d_amd import get_instance_distill_loss
    t_cls, t_box, s_cls, s_box = _term_inputs(3, nl=6, b=2, q=300)
    outs = []
    for host in (False, True):
        out = get_instance_distill_loss(dict(all_cls_scores=t_cls, all_bbox_preds=t_box), dict(all_cls_scores=s_cls, all_bbox_preds=s_box),
                                        host=host, **CFG)
        outs.append((torch.stack(list(out.values())).cpu(), get_instance_distill_loss.last_assigned.cpu()))
    assert torch.equal(outs[0][1], outs[1][1])
    assert torch.equal(outs[0][0], outs[1][0])


def test_assign_per_problem_matches_fixture():
    from graph_detr4d_amd import DistillHungarianAssigner3D
    from test_detr4d_distill_cpu import denormalize
    g = Golden('detr4d_distill_b2')
    asg = DistillHungarianAssigner3D(cls_cost=dict(type='DistillCrossEntropyLossCost', weight=1.0),
                                     reg_cost=dict(type='BBox3DL1Cost', weight=0.25))
    for l in range(g.meta['num_layers']):
        for i in range(g.meta['batch']):
            soft = g.t('t_cls')[l, 0].sigmoid().cuda()
            r = asg.assign(g.t('s_box')[l, i].cuda(), g.t('s_cls')[l, i].cuda(), denormalize(g.t('t_box')[l, i]).cuda(), soft)
            assert torch.equal(r.gt_inds.cpu(), g.t(f'assigned_l{l}_b{i}').long())
