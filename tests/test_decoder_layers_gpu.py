"""Every layer of ONE real multi-layer decoder call against the oracle, on every multi-layer route (GPU only).

The teacher-forced tests (tests/test_full_size_gpu.py) isolate a layer but cannot see the work that crosses layer boundaries
inside the six-layer call: chain B computing the NEXT layer's in-projection, the second program of chain A (reg branch of
layer l - 1 + refinement), position_encoder(l) handed to chain B through SIGNAL / WAIT flags (or the dual schedule), the query
order computed once for all layers, per-layer weight images and ping-pong buffers.  Here the oracle is STEPPED from what the
call returned (tests/decoder_step.py): layer l of the oracle runs on the call's states[l - 1] / refs[l - 1] and must give its
states[l] / refs[l] to one layer's rounding - the tolerances of the teacher-forced tests.  The visibility masks the call's
gathers used are recorded (decoder_step.MaskSpy) so that exactly the rows with a flipped mask bit are excluded (<= 2).

Eager calls only: a graph replayed on another sample is bit-identical to eager (tests/test_modules_gpu.py and bench.py's
check).  The last test is the free-running yardstick of tools/freerun_parity.py."""
import copy
import importlib.util
import os

import pytest
import torch

import bench
import graph_detr4d_amd as G
from graph_detr4d_amd import fused_decoder, fused_train, ops, synthetic
from oracle import torch_oracle as O

from config_cases import decoder_cfg, oracle_params, reg_branches
from decoder_step import MaskSpy, step_check

pytestmark = pytest.mark.gpu
DEV = 'cuda'
PC = synthetic.PC_RANGE
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Case:
    """A decoder, its reg branches, one sample, and the oracle's view of them (CPU)."""

    def __init__(self, tr, regs, feats, qe, metas, oracle_kw=None):
        torch.set_num_threads(16)
        self.sd, self.layer_params = oracle_params(tr)
        self.regs_cpu = None if regs is None else copy.deepcopy(regs)
        self.feats, self.qe, self.metas = feats, qe, metas
        self.oracle_kw = {**dict(cross='Deform3DCrossAttn', num_heads=8, num_points=4), **(oracle_kw or {})}
        self.tr, self.regs = tr.to(DEV).eval(), None if regs is None else regs.to(DEV).eval()
        self.feats_d = [f.to(DEV) for f in feats]
        self.qe_d = qe.to(DEV)

    def split(self, qe):
        query_pos, query = (t.unsqueeze(1).contiguous() for t in torch.split(qe, qe.shape[1] // 2, dim=1))  # (Q, 1, C)
        return query, query_pos

    def init_ref(self, query_pos):
        with torch.no_grad():
            return torch.nn.functional.linear(query_pos.permute(1, 0, 2), self.sd['reference_points.weight'],
                                              self.sd['reference_points.bias']).sigmoid()

    def check(self, states, init_ref, refs, masks, label, qe=None):
        query, query_pos = self.split(self.qe if qe is None else qe)
        torch.testing.assert_close(init_ref.detach().cpu(), self.init_ref(query_pos), rtol=1e-5, atol=1e-5)
        return step_check(self.layer_params, self.regs_cpu, query, query_pos, self.feats, self.metas, PC, states, init_ref,
                          refs, masks=masks, label=label, **self.oracle_kw)


class _Calls:
    """Counts the fused loops a call takes (run_single: the single-stream loop; run: the multi-stream one)."""

    def __init__(self, monkeypatch):
        self.single, self.run = [], []
        orig_single, orig_run = fused_decoder.run_single, fused_decoder.run

        def single(*a, **k):
            self.single.append(1)
            return orig_single(*a, **k)

        def run(*a, **k):
            self.run.append(1)
            return orig_run(*a, **k)
        monkeypatch.setattr(fused_decoder, 'run_single', single)
        monkeypatch.setattr(fused_decoder, 'run', run)


# ----------------------------------------------------------------------------------------------- 900 queries x 24 cameras
@pytest.fixture(scope='module')
def timed():
    """bench.py's timed configuration: build_decoder(G, 24, 6, 'fp32', 1002) and its reg branches, the R50 pyramid, 900 queries."""
    n = 24
    tr, regs = bench.build_decoder(G, n, 6, 'fp32', 1002)
    feats = synthetic.feature_pyramid(n, synthetic.R50_LEVELS, seed=79)
    qe = torch.randn(900, 512, generator=torch.Generator().manual_seed(8))
    metas = synthetic.make_img_metas(synthetic.camera_rig(4), batch=1)
    return _Case(tr, regs, feats, qe, metas)


ROUTES = {
    # name: (environment, run_single taken, gather kinds recorded)
    'default': ({}, True, 'cross_attn_plan_fwd'),
    'pos-encoder-dual': ({'GD4D_POS_ENCODER': 'dual'}, True, 'cross_attn_plan_fwd'),
    'chain-exact': ({}, True, 'cross_attn_plan_fwd'),
    'coarse-off': ({'GD4D_COARSE': '0'}, True, 'cross_attn_plan_fwd'),
    'channels-last': ({}, True, 'cross_attn_plan_fwd'),
    'agg-rows': ({'GD4D_AGG': 'rows'}, True, 'cross_attn_agg_fwd'),
    'project-early': ({'GD4D_PROJECT': 'early'}, False, 'cross_attn_fwd'),
}


@pytest.mark.parametrize('route', list(ROUTES))
def test_six_layer_call_900q_24cams_steps_the_oracle(timed, route, monkeypatch):
    """(a) default: run_single, sliced plan, coarse-projected levels 2-3, position_encoder hand-off, x3 chains;
    (b) GD4D_POS_ENCODER=dual; (c) chain-exact: every chain GEMM on six bf16 products (ops.all_exact(), the switch behind
    GD4D_CHAIN_ALL_EXACT); (d) GD4D_COARSE=0; (e) channels-last levels gathered in place; (f) GD4D_AGG=rows: the pixel-major
    copy and gd4d_cross_attn_agg_fwd; (g) GD4D_PROJECT=early: LateValues refuses it, so the call takes the multi-stream run()
    with pre-projected values (_preproject_values), the position encoder on the aux stream and cross-stream events."""
    env, single, kind = ROUTES[route]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    calls = _Calls(monkeypatch)
    feats_d = timed.feats_d
    if route == 'channels-last':
        feats_d = [f.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3) for f in timed.feats_d]
        assert all(ops.PyramidView.is_channels_last_level(f) for f in feats_d)
    copies = []
    real_copy = ops.pyramid_slice_planar_fwd
    monkeypatch.setattr(ops, 'pyramid_slice_planar_fwd', lambda *a, **k: (copies.append(1), real_copy(*a, **k))[1])
    with torch.no_grad(), MaskSpy() as spy:
        if route == 'chain-exact':
            with ops.all_exact():
                states, init_ref, refs = timed.tr(feats_d, timed.qe_d, reg_branches=timed.regs, img_metas=timed.metas)
        else:
            states, init_ref, refs = timed.tr(feats_d, timed.qe_d, reg_branches=timed.regs, img_metas=timed.metas)
        torch.cuda.synchronize()
    del feats_d
    assert len(calls.run) == 1 and len(calls.single) == int(single), (calls.run, calls.single)
    assert spy.kinds == [kind] * 6, spy.kinds
    assert bool(copies) == (route in ('default', 'pos-encoder-dual', 'chain-exact', 'coarse-off')), copies
    assert states.shape == (6, 900, 1, 256) and refs.shape == (6, 1, 900, 3)
    timed.check(states, init_ref, refs, spy.masks, f'900x24 {route}')


def test_six_layer_call_900q_24cams_student_and_teacher_queries_step_the_oracle(timed, monkeypatch):
    """configs[4]: Detr3DTransformer.forward_shared - a student and a teacher query set through the decoder over ONE pyramid
    (one channels-last copy shared by both passes).  Both passes are stepped, every layer."""
    calls = _Calls(monkeypatch)
    qe_t = torch.randn(905, 512, generator=torch.Generator().manual_seed(46)) * 0.5
    with torch.no_grad(), MaskSpy() as spy:
        outs = timed.tr.forward_shared(timed.feats_d, [timed.qe_d, qe_t.to(DEV)], reg_branches=timed.regs, img_metas=timed.metas)
        torch.cuda.synchronize()
    assert len(outs) == 2 and len(spy.masks) == 12 and len(calls.run) == 2
    for i, ((states, init_ref, refs), qe) in enumerate(zip(outs, (timed.qe, qe_t))):
        timed.check(states, init_ref, refs, spy.masks[6 * i:6 * i + 6], f'forward_shared set {i}', qe=qe)


def test_training_forward_900q_24cams_six_layers_steps_the_oracle(timed):
    """fused_train.DecoderTrainFunction's forward (autograd on, eval mode, reg branches on): its out_all / ref_all stepped against
    the oracle.  The backward of the same call is stepped layer by layer against the fp64 oracle in
    tests/test_train_layers_gpu.py."""
    before = fused_train.CALLS[0]
    with torch.enable_grad(), MaskSpy() as spy:
        states, init_ref, refs = timed.tr(timed.feats_d, timed.qe_d, reg_branches=timed.regs, img_metas=timed.metas)
        torch.cuda.synchronize()
    assert fused_train.CALLS[0] == before + 1, 'the call must take the row-chain training forward'
    assert states.requires_grad and spy.kinds == ['cross_attn_plan_fwd'] * 6, spy.kinds
    timed.check(states.detach(), init_ref.detach(), refs.detach(), spy.masks, '900x24 training forward')


# ----------------------------------------------------------------------------------------------- VoVNet-99 pyramid
def test_six_layer_call_vovnet_pyramid_steps_the_oracle(monkeypatch):
    """configs[3]'s size: 24 cameras, 232 x 400 ... 29 x 50, 900 queries, 6 layers, the default route - the coarse-projected levels
    are off there (GD4D_COARSE_MAX_ROWS), so the loop gathers all four levels from the slice-planar copy."""
    n = 24
    tr, regs = bench.build_decoder(G, n, 6, 'fp32', 1003)
    case = _Case(tr, regs, synthetic.feature_pyramid(n, synthetic.VOV_LEVELS, seed=80),
                 torch.randn(900, 512, generator=torch.Generator().manual_seed(9)), synthetic.make_img_metas(synthetic.camera_rig(4)))
    calls = _Calls(monkeypatch)
    with torch.no_grad(), MaskSpy() as spy:
        states, init_ref, refs = case.tr(case.feats_d, case.qe_d, reg_branches=case.regs, img_metas=case.metas)
        torch.cuda.synchronize()
    assert len(calls.single) == 1 and spy.kinds == ['cross_attn_plan_fwd'] * 6
    case.check(states, init_ref, refs, spy.masks, 'vovnet 900x24')


# ----------------------------------------------------------------------------------------------- 300 queries x 12 cameras
MID = {
    # name: (Deform3DCrossAttn options, transformer type, oracle options)
    'points1': (dict(num_points=1), 'Detr3DTransformer', dict(num_points=1)),
    'points2': (dict(num_points=2), 'Detr3DTransformer', dict(num_points=2)),
    'points8': (dict(num_points=8), 'Detr3DTransformer', dict(num_points=8)),
    'hdetr-mask': (dict(num_points=4), 'HDetr3DTransformer', dict()),
    'depth-encode': (dict(num_points=4, depth_encode=True), 'Detr3DTransformer', dict(depth_encode=True)),
    # bf16 value storage (configs[1]): the channels-last copy the gathers read is bf16, everything else fp32 - the oracle's
    # 'bf16_features' mode is that arithmetic (as in tests/test_timed_size_parity_gpu.py)
    'bf16-values': (dict(num_points=4, value_dtype='bf16'), 'Detr3DTransformer', dict(value_dtype='bf16_features')),
}


@pytest.mark.parametrize('case', list(MID))
def test_six_layer_call_300q_12cams_steps_the_oracle(case, monkeypatch):
    """Mid size (300 queries, 12 cameras = 2 frames, 256 x 448 images): num_points 1 / 2 / 8 (run_single), an H-DETR
    one-to-one / one-to-many self-attention mask (h_detr3d_head_pe.py:299-314), depth_encode (the multi-stream run()), bf16
    value storage."""
    ca_kw, kind, okw = MID[case]
    n, q, nl = 12, 300, 6
    img_hw, levels = (256, 448), [(32, 56), (16, 28), (8, 14), (4, 7)]
    torch.manual_seed(2000)
    tr = G.build_transformer(dict(type=kind, num_feature_levels=4, num_cams=n,
                                  decoder=decoder_cfg(dict(type='Deform3DCrossAttn', num_cams=n, pc_range=PC, embed_dims=256,
                                                           **ca_kw), nl)))
    tr.init_weights()
    for i, layer in enumerate(tr.decoder.layers):
        synthetic.randomise_cross_attn_(layer.attentions[1], seed=2000 + i)
    regs = reg_branches(nl, 2001)
    metas = synthetic.make_img_metas(synthetic.camera_rig(2, img_hw), img_shape=(*img_hw, 3), pad_shape=(*img_hw, 3))
    feats = synthetic.feature_pyramid(n, levels, seed=81)
    qe = torch.randn(q, 512, generator=torch.Generator().manual_seed(10))
    extra = {}
    if case == 'hdetr-mask':
        one2one = 100                                  # queries [0, 100) one-to-one, [100, 300) one-to-many: no attention across
        mask = torch.zeros(q, q, dtype=torch.bool)
        mask[:one2one, one2one:] = True
        mask[one2one:, :one2one] = True
        okw = dict(okw, attn_mask=mask)
        extra = dict(decoder_self_attn_mask=[mask.to(DEV), None])
    c = _Case(tr, regs, feats, qe, metas, okw)
    calls = _Calls(monkeypatch)
    with torch.no_grad(), MaskSpy() as spy:
        states, init_ref, refs = c.tr(c.feats_d, c.qe_d, reg_branches=c.regs, img_metas=metas, **extra)
        torch.cuda.synchronize()
    assert len(calls.run) == 1 and len(calls.single) == (0 if case == 'depth-encode' else 1), (calls.run, calls.single)
    assert spy.kinds == ['cross_attn_plan_fwd'] * nl, spy.kinds
    c.check(states, init_ref, refs, spy.masks, f'300x12 {case}')


# ----------------------------------------------------------------------------------------------- free-running yardstick
def test_free_running_six_layers_against_fp64_oracle():
    """tools/freerun_parity.py at 900 x 24 (docs/measurements_r09.md): all six layers free-running, rows off by > 1e-3 from the
    fp64 oracle after layer 6 for (A) the default x3 route and (B) every chain GEMM exact, against (C) the fp32 oracle.  The
    rule, fixed before measuring: off(A) <= 2 off(C) + 9 and off(B) <= 2 off(C) + 9 (9 = 1 % of the rows)."""
    spec = importlib.util.spec_from_file_location('freerun_parity', os.path.join(ROOT, 'tools', 'freerun_parity.py'))
    fr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fr)
    res = fr.measure()
    print(fr.table(res))
    off = {k: res['layers'][-1][k]['off'] for k in 'ABC'}
    assert off['A'] <= 2 * off['C'] + 9, off
    assert off['B'] <= 2 * off['C'] + 9, off
