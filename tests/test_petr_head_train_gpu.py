"""The PETR head's training kernels on the GPU, alone, against the fp64 reference of petr_head_train_cases.py: ops.petr_keys_train_fwd
(bit-equal to ops.petr_keys_fwd; the stored embedding and logits within the forward test's 2e-4), ops.petr_keys_bwd_rows (permutations
bit-equal; dpe / dlogit within KERNEL_TOL of the tensor's largest |entry|), ops.mlp2_wgrad (both sources of X, every case x
partitions, each gradient within KERNEL_TOL of its largest |entry|, the errors of ops.gemm_tn_bf16x3 on materialised operands printed
beside them), the memory contract of the three launches and the no-allocation call.  Tolerances are the project's per-kernel rule
(KERNEL_TOL of tests/test_fpn_train_gpu.py).

Then the module: PETRHead / PETRv2Head with hip_train=True on the fixture of tests/test_petr_head_gpu.py, eval mode with autograd - the
gradients of every parameter and of the features against torch_ops=True on the GPU and against the fp64 restatement (BWD_TOL, relative
Frobenius per tensor), no gradient at padded pixels, bit-equal repeats in train mode under a seed, needs_input_grad, the refusals of
the node, and the inference route left as it was.  Every measured error is printed before it is asserted."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import graph_detr4d_amd as G
from graph_detr4d_amd import _lib, ops
from graph_detr4d_amd.petr_transformer import PETRTransformer

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import petr_head_train_cases as C  # noqa: E402
from contract import as_input, contract  # noqa: E402
from golden_io import Golden  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
KERNEL_TOL = 1e-4
FWD_TOL = 2e-4                       # test_petr_head_gpu.test_petr_keys_fwd_alone's bound on this MLP
P = C.P


def _rel(got, ref):
    """max |got - ref| over the reference's largest |entry|."""
    ref = ref.to(torch.float64)
    return float((got.double().cpu() - ref).abs().max() / ref.abs().max())


def _images(c, gate):
    d = {k: {n: t.to(DEV) for n, t in c[k].items() if torch.is_tensor(t)} for k in ('pe', 'gate')}
    pe_image = ops.mlp2_frustum_image(d['pe']['w1'], d['pe']['b1'], d['pe']['w2'])
    se_image = ops.mlp2_image(d['gate']['w1'], d['gate']['b1'], d['gate']['w2']) if gate else None
    return d, pe_image, se_image


def _fwd_args(c, gate, wrap=lambda t: t):
    d, pe_image, se_image = _images(c, gate)
    return dict(x=wrap(c['x'].to(DEV)), img2lidar=wrap(c['i2l'].to(DEV)), pad_hw=c['pad_hw'], depth_num=64, depth_start=1,
                position_range=P.POSITION_RANGE, pe_image=pe_image, pe_b2=wrap(d['pe']['b2']), sine=wrap(c['sine'].to(DEV)),
                se_image=se_image, se_b2=wrap(d['gate']['b2']) if gate else None)


# ---- 1. petr_keys_train_fwd ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('gate', [True, False])
@pytest.mark.parametrize('bs,n,h,w', C.CASES)
def test_train_fwd_equals_the_inference_launch_and_stores_pe_and_logits(bs, n, h, w, gate):
    c = C.case(bs, n, h, w)
    a = _fwd_args(c, gate)
    nan = lambda *shape: torch.full(shape, float('nan'), device=DEV)      # noqa: E731
    memory, key_pos = nan(n * h * w, bs, 256), nan(n * h * w, bs, 256)
    pe, logits = (nan(c['m'], 256), nan(c['m'], 256)) if gate else (None, None)
    got = ops.petr_keys_train_fwd(**a, memory=memory, key_pos=key_pos, pe=pe, logits=logits)
    want = ops.petr_keys_fwd(**a)
    assert got[0] is memory and got[1] is key_pos
    assert torch.equal(memory, want[0]) and torch.equal(key_pos, want[1])
    assert torch.equal(memory, PETRTransformer._camera_pixels_first(a['x']))
    pe64, lg64, kp64 = C.keys_reference(c, gate)
    err = float((key_pos.double().cpu() - kp64).abs().max())
    print(f'{(bs, n, h, w)} gate {gate}: max |key_pos - fp64| = {err:.2e}')
    assert not torch.isnan(key_pos).any() and err < FWD_TOL
    if not gate:
        assert got[2] is None and got[3] is None
        return
    e_pe, e_lg = float((pe.double().cpu() - pe64).abs().max()), float((logits.double().cpu() - lg64).abs().max())
    print(f'   max |pe - fp64| = {e_pe:.2e} (values up to {float(pe64.abs().max()):.1f}), max |logits - fp64| = {e_lg:.2e}')
    assert not torch.isnan(pe).any() and not torch.isnan(logits).any() and e_pe < FWD_TOL and e_lg < FWD_TOL


# ---- 2. petr_keys_bwd_rows -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('gate', [True, False])
@pytest.mark.parametrize('with_dmemory', [True, False])
@pytest.mark.parametrize('bs,n,h,w', C.CASES)
def test_bwd_rows(bs, n, h, w, with_dmemory, gate):
    c = C.case(bs, n, h, w)
    pe32 = logit32 = None
    if gate:
        pe64, lg64, _ = C.keys_reference(c, True)
        pe32, logit32 = pe64.float(), lg64.float()
    dkey, dmem = c['dkey_pos'].to(DEV), c['dmemory'].to(DEV) if with_dmemory else None
    dpe, dlogit, dsine, dx0 = ops.petr_keys_bwd_rows(dkey, dmem, (bs, n, h, w), None if pe32 is None else pe32.to(DEV),
                                                     None if logit32 is None else logit32.to(DEV))
    r_dpe, r_dlogit, r_dsine, r_dx0 = C.rows_reference(c, pe32, logit32)
    assert torch.equal(dsine.cpu(), r_dsine.float())                      # permutations: bit-equal
    if bs == 1:
        assert dsine.data_ptr() == dkey.data_ptr()                        # key rows ARE camera-major rows: no copy
    if with_dmemory:
        assert torch.equal(dx0.cpu(), r_dx0.float())
    else:
        assert int(dx0.count_nonzero()) == 0
    if not gate:
        assert dlogit is None and dpe.data_ptr() == dsine.data_ptr()
        return
    e = _rel(dpe, r_dpe), _rel(dlogit, r_dlogit)
    print(f'{(bs, n, h, w)}: dpe {e[0]:.2e}, dlogit {e[1]:.2e} of the largest |entry|')
    assert max(e) <= KERNEL_TOL


# ---- 3. mlp2_wgrad ---------------------------------------------------------------------------------------------------------
def _wgrad_call(c, kind, partitions, wrap=lambda t: t, outs=None, workspace=None):
    d = c[kind]
    w1, b1, w2, dy = (wrap(t.to(DEV)) for t in (d['w1'], d['b1'], d['w2'], c['dy']))
    if kind == 'pe':
        return ops.mlp2_wgrad(dy, w1, b1, w2, frustum=(wrap(c['i2l'].to(DEV)), (c['h'], c['w']), c['pad_hw'], 64, 1, P.POSITION_RANGE),
                              partitions=partitions, outs=outs, workspace=workspace)
    return ops.mlp2_wgrad(dy, w1, b1, w2, x=wrap(d['x'].to(DEV)), partitions=partitions, outs=outs, workspace=workspace)


_REF = {}


def _reference(case, kind):
    key = (case, kind)
    if key not in _REF:
        c = C.case(*case)
        d = c[kind]
        _REF[key] = C.mlp_grads(d['x'], d['w1'], d['b1'], d['w2'], c['dy'])
    return _REF[key]


def _composed(c, kind):
    """The parent's kernels on materialised operands: gemm_bf16x3_fwd, the masked one, gemm_tn_bf16x3 twice."""
    d = c[kind]
    if kind == 'pe':
        fr, _ = ops.frustum_pe_input_fwd(c['i2l'].to(DEV), (c['h'], c['w']), c['pad_hw'], 64, 1, P.POSITION_RANGE)
        x = fr.flatten(2).transpose(1, 2).reshape(c['m'], 192).contiguous()
    else:
        x = d['x'].to(DEV)
    w1, b1, w2, dy = (t.to(DEV) for t in (d['w1'], d['b1'], d['w2'], c['dy']))
    hid = ops.gemm_bf16x3_fwd(x, *ops.split_bf16_fwd(w1), b1, relu=True)
    dw2, db2 = ops.gemm_tn_bf16x3(dy, hid)
    ops.gemm_bf16x3_fwd(dy, *ops.split_bf16_fwd(w2.t().contiguous()), out=hid, mask_out=True)
    dw1, db1 = ops.gemm_tn_bf16x3(hid, x)
    return dict(dw2=dw2, db2=db2, dw1=dw1, db1=db1)


@pytest.mark.parametrize('kind', ['pe', 'adapt'])
@pytest.mark.parametrize('case,partitions', C.CASE_PARTS)
def test_mlp2_wgrad(case, partitions, kind):
    c = C.case(*case)
    got = dict(zip(('dw2', 'db2', 'dw1', 'db1'), _wgrad_call(c, kind, partitions)))
    ref = _reference(case, kind)
    comp = _composed(c, kind)
    errs = {k: _rel(got[k], ref[k]) for k in ref}
    cerr = {k: _rel(comp[k], ref[k]) for k in ref}
    print(f'{case} partitions {partitions} {kind}: ' + ', '.join(f'{k} {errs[k]:.2e} (composed {cerr[k]:.2e})' for k in ref))
    assert all(bool(torch.isfinite(t).all()) for t in got.values())
    assert max(errs.values()) <= KERNEL_TOL, errs


def test_mlp2_wgrad_default_partitions_and_no_db2():
    case = C.CASES[-1]
    c = C.case(*case)
    d = c['adapt']
    w1, b1, w2, dy, x = (t.to(DEV) for t in (d['w1'], d['b1'], d['w2'], c['dy'], d['x']))
    dw2, db2, dw1, db1 = ops.mlp2_wgrad(dy, w1, b1, w2, x=x, want_db2=False)
    ref = _reference(case, 'adapt')
    assert db2 is None
    assert max(_rel(dw2, ref['dw2']), _rel(dw1, ref['dw1']), _rel(db1, ref['db1'])) <= KERNEL_TOL


# ---- 4. the memory contract ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('gate', [True, False])
def test_contract_train_fwd(gate):
    bs, n, h, w = 2, 3, 5, 7
    c = C.case(bs, n, h, w)
    pe64, lg64, kp64 = C.keys_reference(c, gate)

    def launch(run):
        a = _fwd_args(c, gate, wrap=as_input)
        out = ops.petr_keys_train_fwd(**a, memory=run.out((n * h * w, bs, 256)), key_pos=run.out((n * h * w, bs, 256)),
                                      pe=run.out((c['m'], 256)) if gate else None, logits=run.out((c['m'], 256)) if gate else None)
        return dict(memory=out[0], key_pos=out[1], pe=out[2], logits=out[3])

    def check(res):
        assert float((res['key_pos'].double().cpu() - kp64).abs().max()) < FWD_TOL
    contract(f'petr_keys_train_fwd gate {gate}', launch, check)


@pytest.mark.parametrize('gate', [True, False])
@pytest.mark.parametrize('bs,n,h,w', [(2, 3, 5, 7), (1, 1, 16, 8)])
def test_contract_bwd_rows(bs, n, h, w, gate):
    c = C.case(bs, n, h, w)
    pe32 = logit32 = None
    if gate:
        pe64, lg64, _ = C.keys_reference(c, True)
        pe32, logit32 = pe64.float(), lg64.float()
    ref = C.rows_reference(c, pe32, logit32)

    def launch(run):
        m = c['m']
        outs = (run.out((m, 256)) if gate else None, run.out((m, 256)) if gate else None, run.out((m, 256)) if bs > 1 else None,
                run.out((bs * n, 256, h, w)))
        dpe, dlogit, dsine, dx0 = ops.petr_keys_bwd_rows(as_input(c['dkey_pos']), as_input(c['dmemory']), (bs, n, h, w), as_input(pe32),
                                                         as_input(logit32), outs=outs)
        return dict(dpe=dpe if gate else None, dlogit=dlogit, dsine=dsine if bs > 1 else None, dx0=dx0)

    def check(res):
        assert torch.equal(res['dx0'].cpu(), ref[3].float())
        if gate:
            assert max(_rel(res['dpe'], ref[0]), _rel(res['dlogit'], ref[1])) <= KERNEL_TOL
    contract(f'petr_keys_bwd_rows {(bs, n, h, w)} gate {gate}', launch, check)


@pytest.mark.parametrize('kind', ['pe', 'adapt'])
@pytest.mark.parametrize('case,partitions', [((2, 3, 5, 7), 3), ((1, 3, 1, 43), 8)])
def test_contract_mlp2_wgrad(case, partitions, kind):
    c = C.case(*case)
    ref = _reference(case, kind)
    k1 = c[kind]['w1'].shape[1]
    nbytes = int(ops._lib.load().gd4d_mlp2_wgrad_workspace_bytes(k1, 1024, 256, partitions))

    def launch(run):
        outs = (run.out((256, 1024)), run.out((256,)), run.out((1024, k1)), run.out((1024,)))
        ws = run.out((nbytes // 4,))
        res = _wgrad_call(c, kind, partitions, wrap=as_input, outs=outs, workspace=ws)
        return dict(zip(('dw2', 'db2', 'dw1', 'db1'), res), workspace=ws)

    def check(res):
        assert max(_rel(res[k], ref[k]) for k in ref) <= KERNEL_TOL
    contract(f'mlp2_wgrad {case} x {partitions} {kind}', launch, check)


# ---- 5. no allocation ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['pe', 'adapt'])
def test_mlp2_wgrad_allocates_nothing_with_outs_and_workspace(kind):
    c = C.case(2, 3, 8, 10)
    d = c[kind]
    k1 = d['w1'].shape[1]
    parts = 3
    nbytes = int(ops._lib.load().gd4d_mlp2_wgrad_workspace_bytes(k1, 1024, 256, parts))
    new = lambda *s: torch.empty(s, device=DEV)      # noqa: E731
    outs, ws = (new(256, 1024), new(256), new(1024, k1), new(1024)), new(nbytes // 4)
    w1, b1, w2, dy = (t.to(DEV) for t in (d['w1'], d['b1'], d['w2'], c['dy']))
    x = None if kind == 'pe' else d['x'].to(DEV)
    fr = (c['i2l'].to(DEV), (c['h'], c['w']), c['pad_hw'], 64, 1, P.POSITION_RANGE) if kind == 'pe' else None
    ops.mlp2_wgrad(dy, w1, b1, w2, x=x, frustum=fr, partitions=parts, outs=outs, workspace=ws)           # (the LDS attribute: first call)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    res = ops.mlp2_wgrad(dy, w1, b1, w2, x=x, frustum=fr, partitions=parts, outs=outs, workspace=ws)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() == before
    assert all(r is o for r, o in zip(res, outs))


# ---- the module: PETRHead / PETRv2Head with hip_train=True ---------------------------------------------------------------------
BWD_TOL = 1e-3                       # the project's per-module rule: relative Frobenius per tensor
OUT_TOL = dict(rtol=1e-3, atol=1e-3)  # test_petr_head_gpu.OUT_TOL
KEY_SIDE = ('input_proj.', 'position_encoder.', 'adapt_pos3d.', 'fpe.')


@pytest.fixture(scope='module')
def golden():
    return Golden('petr_head')


def _state(g, kind):
    keys = json.loads(bytes(g.arrays[kind + '.keys']).decode())
    shapes = json.loads(bytes(g.arrays[kind + '.shapes']).decode())
    return P.state_dict(keys, shapes, shared=kind == 'v1')


def _metas(g, kind):
    ts = g.arrays[kind + '.timestamps'] if g.has(kind + '.timestamps') else None
    return P.img_metas(g.arrays[kind + '.lidar2img'].astype(np.float64), ts)


def _head(g, kind, **kw):
    head = G.build_head(P.head_config(kind, **kw))
    head.load_state_dict(_state(g, kind), strict=True)                      # the fixture's keys still load
    return head.to(DEV).eval()                                              # eval mode with autograd: no dropout, with_cp inactive


def _weights(outs):
    """The fixed G of the loss sum(outputs G)."""
    return {k: C.grid(tuple(outs[k].shape), 41 + i, 8, 8) for i, k in enumerate(('all_cls_scores', 'all_bbox_preds'))}


def _step(head, g, kind, hooks=None):
    """One forward + backward of sum(outputs G): (outputs, {parameter name or 'feat': gradient})."""
    feat = g.t(kind + '.feat').float().to(DEV).requires_grad_(True)
    if hooks is not None:
        real = head.transformer.forward_keys

        def spy(keys, key_pos, mask, query_embed, reg_branch=None):
            keys.register_hook(lambda t: hooks.__setitem__('dmemory', t.clone()))
            key_pos.register_hook(lambda t: hooks.__setitem__('dkey_pos', t.clone()))
            hooks['mask'] = mask
            return real(keys, key_pos, mask, query_embed, reg_branch)
        head.transformer.forward_keys = spy
    try:
        outs = head([feat], _metas(g, kind))
    finally:
        if hooks is not None:
            del head.transformer.forward_keys
    wts = _weights(outs)
    sum((outs[k] * wts[k].to(DEV)).sum() for k in wts).backward()
    grads = {k: p.grad for k, p in head.named_parameters() if p.grad is not None}
    grads['feat'] = feat.grad
    return {k: outs[k].detach() for k in wts}, grads


@pytest.fixture(scope='module')
def steps(golden):
    """hip_train=True and torch_ops=True, one step each per kind, and the fp64 restatement's gradients; computed once."""
    out = {}
    for kind in ('v1', 'v2'):
        hooks = {}
        hip = _step(_head(golden, kind, hip_train=True), golden, kind, hooks)
        ref = _step(_head(golden, kind, torch_ops=True), golden, kind)
        sd = {k: v.double().requires_grad_(k != 'code_weights') for k, v in _state(golden, kind).items()}
        feat = golden.t(kind + '.feat').double().requires_grad_(True)
        o64 = P.head_forward(sd, P.head_config(kind), feat, _metas(golden, kind))
        wts = _weights(o64)
        sum((o64[k] * wts[k].double()).sum() for k in wts).backward()
        g64 = {k: v.grad for k, v in sd.items() if v.grad is not None}
        g64['feat'] = feat.grad
        out[kind] = dict(hip=hip, ref=ref, g64=g64, hooks=hooks)
    return out


def _fro(got, ref):
    ref = ref.double().cpu()
    den = float(ref.norm())
    num = float((got.double().cpu() - ref).norm())
    return num / den if den > 0 else num


def _norm(t):
    return float(t.double().norm())


@pytest.mark.parametrize('kind', ['v1', 'v2'])
def test_head_gradients_match_torch_ops_and_fp64(steps, kind):
    """Per tensor, relative Frobenius <= BWD_TOL against torch_ops=True on the GPU - every parameter and feat - and against the fp64
    restatement - the key-side parameters and feat.

    A relative error needs a reference that is not zero, and three gradients of this model are zero identically: a shift of every
    key's position encoding by one vector is cancelled by the softmax over the keys (adapt_pos3d.2.bias; position_encoder.2.bias
    where no gate multiplies it), and layer 0's self-attention reads a zero query, so its values are one constant row and neither its
    scores nor its value weights matter (its in_proj_weight).  Both routes return rounding noise for them (observed: 0.65 - 1.95 of
    each other).  Which tensors these are is read from the fp64 restatement alone: its gradient's norm is below 1e-9 of the largest
    gradient norm (fp64 rounding leaves ~1e-13; nothing a 1e-3 test could resolve lies in between).  For those the bound is absolute:
    the noise stays below BWD_TOL of the largest gradient norm among the same module's other parameters - a bias gradient is the
    weight gradient for a constant input of one, so that is the scale its rounding lives on.  The set is asserted by name, per kind:
    another tensor that lands in it is a failure."""
    s = steps[kind]
    (o_hip, g_hip), (o_ref, g_ref), g64 = s['hip'], s['ref'], s['g64']
    for k in o_hip:
        print(f'{kind} {k}: max |hip_train - torch_ops| = {float((o_hip[k] - o_ref[k]).abs().max()):.2e}')
        torch.testing.assert_close(o_hip[k], o_ref[k], **OUT_TOL)
    assert sorted(g_hip) == sorted(g_ref)                                   # every parameter that trains on one route trains on the other
    top64 = max(_norm(v) for v in g64.values())
    zero = sorted(k for k in g_ref if k in g64 and _norm(g64[k]) <= 1e-9 * top64)
    print(f'{kind}: gradients that are zero in fp64 (norm <= 1e-9 of the largest, {top64:.2e}): '
          + ', '.join(f'{k} ({_norm(g64[k]):.1e})' for k in zero))
    errs = {k: _fro(g_hip[k], g_ref[k]) for k in g_ref if k not in zero}
    e64 = {k: _fro(g_hip[k], g64[k]) for k in errs if k in g64 and (k.startswith(KEY_SIDE) or k == 'feat')}
    t64 = {k: _fro(g_ref[k], g64[k]) for k in e64}
    print(f'{"tensor":52s} {"vs torch_ops":>12s} {"vs fp64":>10s} {"torch/fp64":>10s}')
    for k in sorted(errs):
        print(f'{k:52s} {errs[k]:12.2e} ' + (f'{e64[k]:10.2e} {t64[k]:10.2e}' if k in e64 else ''))
    assert all(bool(torch.isfinite(v).all()) for v in g_hip.values())
    assert any(k.startswith('position_encoder.') for k in e64) and any(k.startswith('adapt_pos3d.') for k in e64)
    assert (kind == 'v1') != any(k.startswith('fpe.') for k in e64)
    late = {k: v for k, v in errs.items() if v > BWD_TOL}
    assert not late, late
    late = {k: v for k, v in e64.items() if v > BWD_TOL}
    assert not late, late
    layer0 = 'transformer.decoder.layers.0.attentions.0.attn.in_proj_weight'
    assert zero == sorted(['adapt_pos3d.2.bias', layer0] + (['position_encoder.2.bias'] if kind == 'v1' else [])), zero      # these, no others
    for k in zero:
        module = k.rsplit('.', 1)[0] + '.'
        scale = max(_norm(g_ref[j]) for j in g_ref if j.startswith(module) and j.count('.') == k.count('.') and j not in zero)
        print(f'{k}: |hip_train| {_norm(g_hip[k]):.2e}, |torch_ops| {_norm(g_ref[k]):.2e}, the module\'s other gradients {scale:.2e}')
        assert _norm(g_hip[k]) <= BWD_TOL * scale, k


@pytest.mark.parametrize('kind', ['v1', 'v2'])
def test_no_gradient_reaches_a_padded_pixel(steps, golden, kind):
    """The core writes exact zeros for masked keys, so dkey_pos and dmemory are zero there - and with them dpe, dlogit and dx: the
    gradient of feat at a padded pixel is exactly zero."""
    s = steps[kind]
    hooks, feat_grad = s['hooks'], s['hip'][1]['feat']
    mask = hooks['mask']                                                    # (bs, n h w)
    assert bool(mask.any())
    key_mask = mask.t()                                                     # (n h w, bs): the key rows
    assert bool((hooks['dkey_pos'][key_mask] == 0).all()) and bool((hooks['dmemory'][key_mask] == 0).all())
    bs, n, c, h, w = feat_grad.shape
    pad = mask.view(bs, n, 1, h, w).expand_as(feat_grad)
    assert bool((feat_grad[pad] == 0).all()) and float(feat_grad[~pad].abs().max()) > 0


@pytest.mark.parametrize('kind', ['v1', 'v2'])
def test_train_mode_is_deterministic_under_a_seed(golden, kind):
    head = _head(golden, kind, hip_train=True).train()                     # default dropout
    runs = []
    for _ in range(2):
        head.zero_grad(set_to_none=True)
        torch.manual_seed(7)
        runs.append(_step(head, golden, kind))
    (o1, g1), (o2, g2) = runs
    assert all(torch.equal(o1[k], o2[k]) and bool(torch.isfinite(o1[k]).all()) for k in o1)
    assert sorted(g1) == sorted(g2)
    assert all(torch.equal(g1[k], g2[k]) and bool(torch.isfinite(g1[k]).all()) for k in g1)


@pytest.mark.parametrize('kind', ['v1', 'v2'])
def test_a_second_forward_with_other_cameras_leaves_the_first_backward_alone(golden, kind):
    """The node generates the frustum again in its backward, from the camera matrices of ITS forward: a second forward with other
    lidar2img before the first backward (losses summed over samples) refreshes the head's persistent matrix buffer in place and must
    not reach it.  Same bits as the step alone."""
    head = _head(golden, kind, hip_train=True)
    metas = _metas(golden, kind)
    other = [dict(m, lidar2img=list(m['lidar2img'])[::-1]) for m in metas]                 # each sample's two cameras swapped
    feat = golden.t(kind + '.feat').float().to(DEV)
    wts = None

    def grads_of(between, first=metas):
        nonlocal wts
        head.zero_grad(set_to_none=True)
        outs = head([feat], first)
        if wts is None:
            wts = {k: v.to(DEV) for k, v in _weights(outs).items()}
        if between is not None:
            head([feat], between)
        sum((outs[k] * wts[k]).sum() for k in wts).backward()
        return {k: p.grad.clone() for k, p in head.named_parameters() if p.grad is not None}
    alone = grads_of(None)
    with_second = grads_of(other)
    elsewhere = grads_of(None, first=other)
    assert sorted(alone) == sorted(with_second)
    differ = [k for k in alone if not torch.equal(alone[k], with_second[k])]
    assert not differ, differ
    # (the second forward's cameras do give other gradients: the comparison above could have failed)
    assert _fro(elsewhere['position_encoder.0.weight'], alone['position_encoder.0.weight']) > 1e-2


class _Calls:
    """Every launch ops._call makes while it is open, from whichever thread.  _lib.recording is per thread and the backward runs on
    autograd's, so a recording stand-in never sees it; what is observed here is what goes through ops._call - which ops.mlp2_wgrad,
    the launch in question, does."""

    def __enter__(self):
        self.real, self.calls = ops._call, []
        ops._call = self
        return self

    def __exit__(self, *exc):
        ops._call = self.real

    def __call__(self, entry, *args):
        self.calls.append((entry, args))
        return self.real(entry, *args)


def test_a_frozen_position_encoder_skips_its_launch(golden):
    head = _head(golden, 'v2', hip_train=True)
    for p in head.position_encoder.parameters():
        p.requires_grad_(False)
    with _Calls() as seen:
        _, grads = _step(head, golden, 'v2')
    assert all(p.grad is None for p in head.position_encoder.parameters())
    k1 = [args[1] for entry, args in seen.calls if entry == 'gd4d_mlp2_wgrad']
    assert k1 == [384], k1                                                  # adapt_pos3d's only; none for the 192 frustum inputs
    assert 'adapt_pos3d.0.weight' in grads and 'fpe.conv_reduce.weight' in grads and 'input_proj.weight' in grads
    full = _head(golden, 'v2', hip_train=True)
    with _Calls() as seen:
        _step(full, golden, 'v2')
    assert sorted(args[1] for entry, args in seen.calls if entry == 'gd4d_mlp2_wgrad') == [192, 384]


def _short_circuit(head):
    """forward_keys replaced by a cheap differentiable stand-in: the graph behind the key-side node holds only nodes that allow a
    second backward."""
    def stand_in(keys, key_pos, mask, query_embed, reg_branch=None):
        row = (keys.mean(0) + key_pos.mean(0))[None, :, None, :] + query_embed[None, None]
        return row.expand(2, -1, -1, -1)
    head.transformer.forward_keys = stand_in


def test_second_backward_and_in_place_updates_are_refused(golden):
    head = _head(golden, 'v2', hip_train=True)
    _short_circuit(head)
    feat = golden.t('v2.feat').float().to(DEV).requires_grad_(True)
    outs = head([feat], _metas(golden, 'v2'))
    loss = outs['all_cls_scores'].sum() + outs['all_bbox_preds'].sum()
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match='consumed by the first backward'):
        loss.backward()
    outs = head([feat], _metas(golden, 'v2'))
    with torch.no_grad():
        head.position_encoder[0].weight.add_(0.0)                           # in place: the version counter moves
    with pytest.raises(RuntimeError, match='modified in place'):
        (outs['all_cls_scores'].sum() + outs['all_bbox_preds'].sum()).backward()


class _Log:
    """A _lib.recording stand-in that launches: the library, with the name of every entry point called through it kept."""

    def __init__(self):
        self.real, self.names = _lib.load(), []

    def __getattr__(self, name):
        if not name.startswith('gd4d_'):
            raise AttributeError(name)
        fn = getattr(self.real, name)

        def call(*args):
            self.names.append(name)
            return fn(*args)
        return call

    def record_event(self, stream):
        ev = torch.cuda.Event()
        ev.record(stream)
        return ev

    def wait_event(self, stream, event):
        stream.wait_event(event)

    def copy(self, dst, src):
        dst.copy_(src)


@pytest.mark.parametrize('kind', ['v1', 'v2'])
def test_eval_without_autograd_takes_the_inference_route_unchanged(golden, kind):
    feat, metas = [golden.t(kind + '.feat').float().to(DEV)], _metas(golden, kind)
    res = []
    for flag in (False, True):
        head = _head(golden, kind, hip_train=flag)
        log = _Log()
        with torch.no_grad(), _lib.recording(log):
            outs = head(feat, metas)
        res.append((outs, log.names))
    (a, names_a), (b, names_b) = res
    assert torch.equal(a['all_cls_scores'], b['all_cls_scores']) and torch.equal(a['all_bbox_preds'], b['all_bbox_preds'])
    assert names_a == names_b and 'gd4d_petr_keys_fwd' in names_a and 'gd4d_petr_keys_train_fwd' not in names_a


def test_uncovered_calls_name_torch_ops(golden):
    head = _head(golden, 'v1')                                              # hip_train=False: autograd is refused as before
    feat = golden.t('v1.feat').float().to(DEV).requires_grad_(True)
    with pytest.raises(_lib.Gd4dError, match='torch_ops'):
        head([feat], _metas(golden, 'v1'))
    head = _head(golden, 'v1', hip_train=True)
    with pytest.raises(_lib.Gd4dError, match='torch_ops'):
        head([feat.double()], _metas(golden, 'v1'))
