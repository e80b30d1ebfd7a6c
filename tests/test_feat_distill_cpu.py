"""MixDistill's feature-distillation loss without a GPU: the fp64 restatement (tests/feat_distill_ref.py) against vectors captured from
the reference's own `MixDistill.get_feat_distill_loss` (tools/gen_golden.py::case_feat_distill), the C ABI's argument checks, and the
module's surface."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from feat_distill_ref import attention_maps, feat_distill_ref
from golden_io import Golden

FIXTURES = ['feat_distill_vanilla', 'feat_distill_attention']
NEW_EXPORTS = ('gd4d_feat_distill_stats_workspace_bytes', 'gd4d_feat_distill_stats_fwd', 'gd4d_feat_distill_workspace_bytes',
               'gd4d_feat_distill_fwd')


def fixture_levels(g):
    nl = len(g.meta['levels'])
    return ([g.arrays[f'teacher{l}'] for l in range(nl)], [g.arrays[f'student{l}'] for l in range(nl)],
            [g.arrays[f'lateral_convs.{l}.weight'] for l in range(nl)], [g.arrays[f'lateral_convs.{l}.bias'] for l in range(nl)])


@pytest.mark.parametrize('name', FIXTURES)
def test_restatement_reproduces_the_reference(name):
    g = Golden(name)
    m = g.meta
    teacher, student, weights, biases = fixture_levels(g)
    loss, gx, gw, gb = feat_distill_ref(teacher, student, weights, biases, m['type'], m['loss_weight'])
    # tests/test_distill_oracle.py's tolerance for sums taken in another order than the fixture's: the fixture is the reference's fp32
    # run, the restatement is fp64 (it equals the same op sequence run by torch in fp64 to 4e-16), so the two differ by the
    # reference's own fp32 rounding - up to 1.1e-6 of an element of the attention fixture's coarsest level
    tol = dict(rtol=1e-5, atol=1e-7)
    f32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))     # noqa: E731
    torch.testing.assert_close(f32(loss), g.t('feat_loss').reshape(()), **tol)
    assert float(g.t('feat_loss')) > 0.1
    for l in range(len(teacher)):
        for got, key in ((gx[l], f'grad_student{l}'), (gw[l], f'grad_weight{l}'), (gb[l], f'grad_bias{l}')):
            ref = g.t(key)
            torch.testing.assert_close(f32(got).reshape(ref.shape), ref, **tol)
            # the gradients are small numbers (coef = loss_weight / (levels R 256 HW)), so also relative to their own size: the
            # reference is fp32 and chains two 256-term sums (convolution, its transpose) with the loss in between; allowed:
            # 4 * sqrt(256) * 2^-24 = 3.8e-6 of the tensor's norm
            rel = np.linalg.norm(np.asarray(got).ravel() - ref.double().numpy().ravel()) / np.linalg.norm(ref.double().numpy().ravel())
            assert rel < 4 * 16 * 2.0 ** -24, (key, rel)
            assert float(ref.abs().max()) > 0


def test_fixture_attention_maps_are_far_from_uniform():
    g = Golden('feat_distill_attention')
    for l, (h, w) in enumerate(g.meta['levels']):
        a_c, a_s = attention_maps(g.arrays[f'teacher{l}'].reshape(-1, 256, h * w))
        assert abs(float(a_s.mean()) - h * w / 256.0) < 1e-9 and abs(float(a_c.mean()) - 256.0 / (h * w)) < 1e-9
        assert float(a_s.max() / a_s.min()) > 3.0                           # uniform maps would give 1
        assert float(a_c.max() / a_c.min()) > 1.5


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
    EINVAL, EUNSUPPORTED, EALIGN, EWORKSPACE = -1, -2, -3, -5
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 96)()
    ptr = ctypes.c_void_p((ctypes.addressof(buf) + 63) & ~63)               # 64-byte aligned: alignment checks pass
    odd = ctypes.c_void_p(ptr.value + 4)
    lv = (ctypes.c_int32 * 6)(15, 25, 5, 13, 1, 1)
    zero = (ctypes.c_int32 * 6)(15, 25, 0, 13, 1, 1)
    huge = (ctypes.c_int32 * 6)(15, 25, 32768, 32768, 1, 1)                 # R * H * W = 2 * 2^30 = 2^31
    ptrs = (ctypes.c_void_p * 3)(*[ptr.value] * 3)
    holes = (ctypes.c_void_p * 3)(ptr.value, None, ptr.value)
    big = 1 << 40
    # workspace sizes: what the layouts in gd4d_feat_distill.hip need, 0 for arguments the functions refuse
    up = lambda b: (b + 255) & ~255                                         # noqa: E731
    tiles = sum(-(-hw // 64) for hw in (375, 65, 1))
    want = up(2 * tiles * 4) + up(3 * 4 * 256 * 256 * 2) + up(128 * 256 * 256 * 4) + up(128 * 256 * 4) + up(2 * 256 * 375 * 4)
    assert lib.gd4d_feat_distill_workspace_bytes(lv, 3, 2) == want
    assert lib.gd4d_feat_distill_stats_workspace_bytes(lv, 3, 2) == up(2 * 2 * 256 * 4)      # 375 pixels: two 256-pixel chunks
    for fn in (lib.gd4d_feat_distill_workspace_bytes, lib.gd4d_feat_distill_stats_workspace_bytes):
        assert fn(null, 3, 2) == 0 and fn(lv, 0, 2) == 0 and fn(lv, 9, 2) == 0 and fn(lv, 3, 0) == 0
        assert fn(zero, 3, 2) == 0 and fn(huge, 3, 2) == 0

    def stats(teacher=ptrs, hw=lv, levels=3, r=2, c=256, temp=0.5, a_c=ptrs, a_s=ptrs, ws=ptr, nbytes=big):
        return lib.gd4d_feat_distill_stats_fwd(teacher, hw, levels, r, c, temp, a_c, a_s, ws, nbytes, null)
    assert stats(teacher=null) == EINVAL and stats(a_c=null) == EINVAL and stats(a_s=null) == EINVAL and stats(ws=null) == EINVAL
    assert stats(hw=null) == EINVAL and stats(hw=zero) == EINVAL and stats(levels=0) == EINVAL and stats(r=0) == EINVAL
    assert stats(teacher=holes) == EINVAL and stats(a_c=holes) == EINVAL and stats(a_s=holes) == EINVAL      # a level without a map
    assert stats(temp=0.0) == EINVAL
    assert stats(c=128) == EUNSUPPORTED
    assert stats(levels=9) == EUNSUPPORTED
    assert stats(hw=huge) == EUNSUPPORTED                                   # R * HW >= 2^31
    assert stats(ws=odd) == EALIGN
    assert stats(nbytes=lib.gd4d_feat_distill_stats_workspace_bytes(lv, 3, 2) - 1) == EWORKSPACE

    def fwd(student=ptrs, teacher=ptrs, hw=lv, levels=3, r=2, c=256, weight=ptr, bias=ptr, a_c=ptrs, a_s=ptrs, loss=ptr, gx=ptrs,
            gw=ptr, gb=ptr, ws=ptr, nbytes=big):
        return lib.gd4d_feat_distill_fwd(student, teacher, hw, levels, r, c, weight, bias, a_c, a_s, 1.0, loss, gx, gw, gb, ws, nbytes, null)
    for key in ('student', 'teacher', 'weight', 'bias', 'loss', 'gx', 'gw', 'gb', 'ws', 'hw'):
        assert fwd(**{key: null}) == EINVAL, key
    assert fwd(a_c=null) == EINVAL and fwd(a_s=null) == EINVAL              # both attention maps, or neither
    for key in ('student', 'teacher', 'gx', 'a_c', 'a_s'):
        assert fwd(**{key: holes}) == EINVAL, key
    assert fwd(hw=zero) == EINVAL and fwd(levels=0) == EINVAL and fwd(r=0) == EINVAL
    assert fwd(c=128) == EUNSUPPORTED and fwd(c=512) == EUNSUPPORTED
    assert fwd(levels=9) == EUNSUPPORTED
    assert fwd(hw=huge) == EUNSUPPORTED
    assert fwd(ws=odd) == EALIGN
    assert fwd(nbytes=want - 1) == EWORKSPACE and fwd(a_c=null, a_s=null, nbytes=want - 1) == EWORKSPACE


def test_module_keys_strict_load_and_types():
    from graph_detr4d_amd import FeatureDistillLoss
    m = FeatureDistillLoss(dict(type='attention', loss_weight=5e-3))
    keys = [f'lateral_convs.{i}.{p}' for i in range(4) for p in ('weight', 'bias')]
    assert list(m.state_dict()) == keys
    assert all(tuple(c.weight.shape) == (256, 256, 1, 1) and tuple(c.bias.shape) == (256,) for c in m.lateral_convs)
    g = Golden('feat_distill_vanilla')
    sd = {k: g.t(k) for k in g.arrays if k.startswith('lateral_convs.')}  # the reference's key names
    m2 = FeatureDistillLoss(dict(type='vanilla', loss_weight=2.0), num_levels=len(g.meta['levels']))
    m2.load_state_dict(sd, strict=True)
    assert torch.equal(m2.lateral_convs[1].weight.detach(), sd['lateral_convs.1.weight'])
    with pytest.raises(RuntimeError):
        m.load_state_dict(sd, strict=True)                                  # four levels expected, two given
    for bad in ('Vanilla', 'mse', None):
        with pytest.raises(ValueError, match='vanilla.*attention'):
            FeatureDistillLoss(dict(type=bad, loss_weight=1.0))
    assert FeatureDistillLoss(dict(loss_weight=1.0)).loss_feat_distill.get('type', 'vanilla') == 'vanilla'     # the reference's default


def test_function_refuses_unknown_types_teacher_grads_and_cpu_tensors():
    from graph_detr4d_amd import FeatureDistillLoss, get_feat_distill_loss
    from graph_detr4d_amd._lib import Gd4dError
    torch.manual_seed(0)
    m = FeatureDistillLoss(dict(type='vanilla', loss_weight=1.0), num_levels=2)
    t = [torch.randn(1, 2, 256, 3, 5), torch.randn(1, 2, 256, 1, 2)]
    s = [torch.randn(1, 2, 256, 3, 5, requires_grad=True), torch.randn(1, 2, 256, 1, 2, requires_grad=True)]
    with pytest.raises(ValueError, match='vanilla.*attention'):
        get_feat_distill_loss(t, s, m.lateral_convs, dict(type='l1', loss_weight=1.0))
    with pytest.raises(ValueError, match='detached'):
        m([t[0], t[1].clone().requires_grad_()], s)
    with pytest.raises(ValueError):
        m(t, [s[0], s[1][..., :1]])                                         # a level whose shapes disagree
    with pytest.raises(Gd4dError):
        m(t, s)                                                             # no CPU fallback
    out = get_feat_distill_loss(t, s, m.lateral_convs, m.loss_feat_distill, torch_ops=True)       # the torch-op route is device-agnostic
    assert list(out) == ['feat_loss'] and out['feat_loss'].dim() == 0
    ref, _, _, _ = feat_distill_ref([x.numpy() for x in t], [x.detach().numpy() for x in s], [c.weight.detach().numpy() for c in m.lateral_convs],
                                    [c.bias.detach().numpy() for c in m.lateral_convs], 'vanilla', 1.0)
    assert abs(float(out['feat_loss'].detach()) - ref) < 1e-5 * ref
