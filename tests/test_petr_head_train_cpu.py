"""Training PETRHead / PETRv2Head on HIP, the part that needs no GPU: the conditions the cases of petr_head_train_cases.py are held to
(the ReLU margin, the active share, nothing excluded), the fp64 reference against a second, explicit form of the five gradients, the
host side of gd4d_mlp2_wgrad (plan, workspace, argument checks before any launch) and the public interface of hip_train."""
import ctypes
import inspect
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import petr_head_train_cases as C  # noqa: E402

P = C.P


# ---- the cases ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['pe', 'adapt', 'gate'])
@pytest.mark.parametrize('case', C.CASES)
def test_cases_meet_the_relu_margin_condition(case, kind):
    c = C.case(*case)
    d = c[kind]
    pre = C.pre_activation(d['x'], d['w1'], d['b1'])
    assert tuple(pre.shape) == (c['m'], d['w1'].shape[0]) and c['m'] == case[0] * case[1] * case[2] * case[3]
    near = int((pre.abs() < C.TAU).sum())
    active = float((pre > 0).double().mean())
    print(f'{case} {kind}: {d["rounds"]} rounds of + 1 / 64, {near} (row, unit) pairs within {C.TAU}, active share {active:.3f}, '
          f'largest |pre-activation| {float(pre.abs().max()):.2f}')
    assert near == 0                                        # no (row, unit) within tau: nothing has to be excluded
    assert 0.3 <= active <= 0.7
    assert C.SEED[case] == 0                                # (a case that needed another seed would say so here)


def test_partitions_of_the_cases():
    assert [c[0] * c[1] * c[2] * c[3] for c in C.CASES] == [105, 128, 129, 210, 480]
    assert all(C.PARTITIONS[c] == (1, 3, 8) for c in C.CASES[2:])


@pytest.mark.parametrize('kind', ['pe', 'adapt'])
@pytest.mark.parametrize('case', C.CASES)
def test_reference_gradients_against_the_explicit_form(case, kind):
    c = C.case(*case)
    d = c[kind]
    a = C.mlp_grads(d['x'], d['w1'], d['b1'], d['w2'], c['dy'])
    b = C.mlp_grads_explicit(d['x'], d['w1'], d['b1'], d['w2'], c['dy'])
    k1 = d['w1'].shape[1]
    assert {k: tuple(v.shape) for k, v in a.items()} == dict(dw2=(256, 1024), db2=(256,), dw1=(1024, k1), db1=(1024,))   # all of each
    for k in a:
        err = float((a[k] - b[k]).abs().max() / b[k].abs().max())
        print(f'{case} {kind} {k}: {err:.1e}')
        assert err <= 1e-12


def test_rows_reference_is_the_adjoint_of_the_forward():
    c = C.case(2, 3, 5, 7)
    pe64, lg64, _ = C.keys_reference(c, True)
    pe, lg = pe64.clone().requires_grad_(True), lg64.clone().requires_grad_(True)
    sine = c['sine'].double().view(-1, 256).requires_grad_(True)
    key_pos = C.key_rows(pe * torch.sigmoid(lg) + sine, 2, 3)
    (key_pos * c['dkey_pos'].double()).sum().backward()
    dpe, dlogit, dsine, _ = C.rows_reference(c, pe64, lg64)
    for got, want in ((dpe, pe.grad), (dlogit, lg.grad), (dsine, sine.grad)):
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


# ---- the host side of gd4d_mlp2_wgrad ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('m', [1, 105, 128, 129, 480, 48000])
@pytest.mark.parametrize('partitions', [1, 3, 8, 400])
def test_plan_covers_every_tile_once(m, partitions):
    from graph_detr4d_amd import ops
    grid, ranges = ops.mlp2_wgrad_plan(m, partitions)
    tiles = (m + 127) // 128
    assert grid == (1024 // 32, partitions) and len(ranges) == partitions
    assert ranges[0][0] == 0 and ranges[-1][1] == tiles
    assert all(lo <= hi for lo, hi in ranges)                               # (lo == hi: an empty partition)
    assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))            # contiguous, every tile once
    if partitions > tiles:
        assert any(lo == hi for lo, hi in ranges)
    if (m, partitions) == (480, 3):
        assert sorted(hi - lo for lo, hi in ranges) == [1, 1, 2]


def test_workspace_does_not_depend_on_the_rows():
    """M = 105 and M = 48 000 take the same workspace because the entry point has no row count to take: what carries the weight here
    is its signature - (K1, H, N2, partitions), in the header as in _lib - and the closed form of its value, one partial per (hidden
    chunk, partition) and one row of db2 per partition."""
    import re
    from graph_detr4d_amd import _lib
    lib = _lib.load()
    assert len(_lib.SIGNATURES['gd4d_mlp2_wgrad_workspace_bytes'][1]) == 4
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'gd4d.h')).read()
    assert re.search(r'size_t gd4d_mlp2_wgrad_workspace_bytes\(int K1, int H, int N2, int partitions\);', header)
    for k1 in (192, 384):
        for parts in (1, 8, 400):
            assert int(lib.gd4d_mlp2_wgrad_workspace_bytes(k1, 1024, 256, parts)) == 4 * (parts * 32 * (256 * 32 + 32 * k1 + 32) + parts * 256)
    assert lib.gd4d_mlp2_wgrad_workspace_bytes(100, 1024, 256, 1) == 0
    assert lib.gd4d_mlp2_wgrad_workspace_bytes(192, 1000, 256, 1) == 0
    assert lib.gd4d_mlp2_wgrad_workspace_bytes(192, 1024, 128, 1) == 0
    assert lib.gd4d_mlp2_wgrad_workspace_bytes(192, 1024, 256, 0) == 0


def _buf(floats=64, offset=0):
    raw = (ctypes.c_char * (4 * floats + 64))()
    base = ctypes.addressof(raw)
    return raw, ctypes.c_void_p(base + (-base) % 16 + offset)


def test_argument_checks_return_before_any_gpu_work():
    from graph_detr4d_amd import _lib
    lib = _lib.load()
    keep, p = _buf()
    keep2, odd = _buf(offset=4)
    rng = (ctypes.c_double * 6)(*P.POSITION_RANGE)
    EINVAL, EUNSUPPORTED, EALIGN, EWORKSPACE = -1, -2, -3, -5
    # gd4d_mlp2_wgrad
    big = 1 << 40

    def wgrad(x=p, k1=384, i2l=None, r=0, d=64, w1=p, dy=p, m=128, h=1024, n2=256, parts=1, ws=p, ws_bytes=big, dw2=p):
        return lib.gd4d_mlp2_wgrad(x, k1, i2l, r, 1, 1, 16., 16., d, 1.0, rng, w1, p, p, dy, m, h, n2, parts, ws, ws_bytes, dw2, p, p, p, None)
    assert wgrad(w1=None) == EINVAL and wgrad(dw2=None) == EINVAL and wgrad(m=0) == EINVAL and wgrad(ws=None) == EINVAL
    assert wgrad(x=None, k1=192) == EINVAL                                   # generated X without its cameras
    assert wgrad(x=None, k1=192, i2l=p, r=3, m=128) == EINVAL                # 3 cameras of 1 x 1 pixels are not 128 rows
    assert wgrad(k1=256) == EUNSUPPORTED and wgrad(h=1000) == EUNSUPPORTED and wgrad(n2=128) == EUNSUPPORTED
    assert wgrad(parts=5000) == EUNSUPPORTED and wgrad(k1=192) == EUNSUPPORTED      # 192 inputs are generated, 384 read
    assert wgrad(x=None, k1=192, i2l=p, r=128, d=32) == EUNSUPPORTED
    assert wgrad(ws_bytes=16) == EWORKSPACE
    assert wgrad(x=odd) == EALIGN and wgrad(dy=odd) == EALIGN and wgrad(w1=odd) == EALIGN and wgrad(ws=odd) == EALIGN
    assert lib.gd4d_mlp2_wgrad_plan(0, 1024, 1, None, None) == EINVAL and lib.gd4d_mlp2_wgrad_plan(128, 1024, 0, None, None) == EINVAL
    assert lib.gd4d_mlp2_wgrad_plan(128, 1000, 1, None, None) == EUNSUPPORTED
    # gd4d_petr_keys_bwd_rows
    rows = lambda **kw: lib.gd4d_petr_keys_bwd_rows(kw.get('dkey', p), p, kw.get('pe', None), kw.get('logit', None), kw.get('bs', 1), 1, 2,      # noqa: E731
                                                    kw.get('w', 2), kw.get('dpe', None), kw.get('dlogit', None), p, kw.get('dx0', p), None)
    assert rows(dkey=None) == EINVAL and rows(dx0=None) == EINVAL and rows(bs=0) == EINVAL
    assert rows(logit=p) == EINVAL and rows(pe=p) == EINVAL                   # the gate's tensors come together
    assert rows(bs=4096, w=1 << 20) == EUNSUPPORTED
    assert rows(dkey=odd) == EALIGN and rows(dx0=odd) == EALIGN and rows(logit=p, pe=p, dpe=odd, dlogit=p) == EALIGN
    # gd4d_petr_keys_train_fwd
    fwd = lambda **kw: lib.gd4d_petr_keys_train_fwd(p, p, kw.get('bs', 1), 1, kw.get('c', 256), 2, 2, 32., 32., kw.get('d', 64), 1.0, rng,      # noqa: E731
                                                    kw.get('img', p), None, kw.get('pe_h', 1024), kw.get('se', None), None, 256, p, p, p,
                                                    kw.get('pe_out', None), None, None)
    assert fwd(bs=0) == EINVAL and fwd(img=None) == EINVAL
    assert fwd(se=p) == EINVAL and fwd(se=p, pe_out=p) == EINVAL             # a gate stores pe AND logits
    assert fwd(c=128) == EUNSUPPORTED and fwd(d=32) == EUNSUPPORTED and fwd(pe_h=512) == EUNSUPPORTED
    assert fwd(img=odd) == EALIGN
    del keep, keep2


# ---- the public interface --------------------------------------------------------------------------------------------------
def test_hip_train_is_a_named_parameter():
    from graph_detr4d_amd.petr_head import _PETRHeadBase
    sig = inspect.signature(_PETRHeadBase.__init__)
    assert 'hip_train' in sig.parameters and sig.parameters['hip_train'].default is False
    assert sig.parameters['hip_train'].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD


@pytest.mark.parametrize('kind', ['v1', 'v2'])
def test_one_keyword_trains_the_stage(kind):
    import graph_detr4d_amd as G
    from graph_detr4d_amd.petr_head import RegLayer
    from graph_detr4d_amd.petr_transformer import PETRMultiheadAttention
    for flag in (False, True):
        head = G.build_head(P.head_config(kind, hip_train=flag))
        assert head.hip_train is flag
        below = [m for m in head.modules() if isinstance(m, (PETRMultiheadAttention, RegLayer))]
        assert below and all(m.hip_train is flag for m in below)
    sd_keys = set(G.build_head(P.head_config(kind)).state_dict())
    assert set(head.state_dict()) == sd_keys                                 # no new state-dict key


def test_uncovered_configurations_raise_at_construction():
    import graph_detr4d_amd as G
    from graph_detr4d_amd._lib import Gd4dError
    with pytest.raises(Gd4dError, match='torch_ops=True'):
        G.build_head(P.head_config('v1', hip_train=True, LID=False))
    with pytest.raises(Gd4dError, match='torch_ops=True'):
        G.build_head(P.head_config('v2', hip_train=True, depth_num=32))
    head = G.build_head(P.head_config('v1', hip_train=True, LID=False, torch_ops=True))          # torch_ops wins
    assert head.torch_ops and head.hip_train


def test_reg_layer_alone_still_refuses_training():
    from graph_detr4d_amd._lib import Gd4dError
    from graph_detr4d_amd.petr_head import RegLayer
    layer = RegLayer()
    assert layer.hip_train is False and 'hip_train' not in inspect.signature(RegLayer.__init__).parameters
    layer.train()
    with pytest.raises(Gd4dError, match='torch_ops'):
        layer(torch.zeros(2, 256))
