"""Training of the FPN neck on the library's kernels (fpn.py hip_train=True, gd4d_fpn_train.hip) without a GPU: the constructor keyword,
what still raises, the fp64 backward (fpn_train_ref.py) against fp64 autograd, the top-down adjoint's children, and the C ABI's argument
checks."""
import ctypes
import os
import re

import pytest
import torch

import fpn_ref as R
import fpn_train_ref as T

SMALL = dict(in_channels=[32, 64, 96, 128], out_channels=256)
HW = [(26, 42), (13, 21), (7, 11), (4, 6)]
NEW_SYMBOLS = ('gd4d_fpn_lateral_image_mode_bytes', 'gd4d_fpn_lateral_image_mode', 'gd4d_fpn_lateral_dgrad',
               'gd4d_fpn_lateral_wgrad_workspace_bytes', 'gd4d_fpn_lateral_wgrad_tiles', 'gd4d_fpn_lateral_wgrad', 'gd4d_fpn_topdown_bwd',
               'gd4d_fpn_extra_conv_dgrad', 'gd4d_fpn_extra_conv_wgrad', 'gd4d_fpn_bias_grad')


def _inputs(channels, hw=HW, n=2, seed=3):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, c, *s, generator=g) for c, s in zip(channels, hw)]


def test_constructor_accepts_hip_train():
    import graph_detr4d_amd as G
    fpn = G.FPN(**SMALL, num_outs=4, hip_train=True)
    cp = G.CPFPN(**SMALL, num_outs=4, hip_train=True)
    assert fpn.hip_train is True and cp.hip_train is True and not fpn.torch_ops
    assert G.FPN(**SMALL, num_outs=4).hip_train is False
    built = G.build_neck(dict(type='FPN', **SMALL, num_outs=5, start_level=1, add_extra_convs='on_output', hip_train=True))
    assert type(built) is G.FPN and built.hip_train is True


def test_torch_ops_wins_over_hip_train():
    import graph_detr4d_amd as G
    xs = _inputs(SMALL['in_channels'])
    for cls in (G.FPN, G.CPFPN):
        mod = cls(**SMALL, num_outs=4, torch_ops=True, hip_train=True).train()
        sum(o.sum() for o in mod(xs)).backward()                               # CPU tensors: only the torch route can have run
        assert mod.lateral_convs[0].conv.weight.grad is not None


def test_without_hip_train_the_kernel_route_still_raises_and_names_the_keyword(monkeypatch):
    import graph_detr4d_amd as G
    from graph_detr4d_amd import functional as Fn
    from graph_detr4d_amd._lib import Gd4dError
    monkeypatch.delenv('GD4D_TORCH_OPS', raising=False)
    monkeypatch.setattr(Fn, 'require_gpu', lambda t, name: None)
    xs = _inputs(SMALL['in_channels'])
    for cls in (G.FPN, G.CPFPN):
        mod = cls(**SMALL, num_outs=4)
        with torch.no_grad(), pytest.raises(Gd4dError, match='train.*torch_ops=True.*hip_train=True'):
            mod.train()(xs)
        with pytest.raises(Gd4dError, match='autograd.*torch_ops=True.*hip_train=True'):
            mod.eval()(xs)
    # outside the kernels' limits hip_train=True still needs torch_ops=True
    with pytest.raises(Gd4dError, match='torch_ops'):
        G.FPN(**dict(SMALL, out_channels=128), num_outs=4, hip_train=True)


@pytest.mark.parametrize('cp', [False, True], ids=['FPN', 'CPFPN'])
def test_reference_backward_agrees_with_fp64_autograd(cp):
    import graph_detr4d_amd as G
    torch.manual_seed(2)
    kw = dict(start_level=0, num_outs=4) if cp else dict(start_level=1, num_outs=5)
    mod = (G.CPFPN if cp else G.FPN)(**SMALL, add_extra_convs='on_output', relu_before_extra_convs=True, torch_ops=True, **kw)
    with torch.no_grad():
        for p in mod.parameters():
            if p.dim() == 1:
                p.normal_(0, 0.1)
    sd, xs = mod.state_dict(), _inputs(SMALL['in_channels'])
    cfg = dict(start_level=kw['start_level'], num_outs=kw['num_outs'], relu_before_extra_convs=True, cp=cp)
    outs = T.forward({k: v.double() for k, v in sd.items()}, [x.double() for x in xs], **cfg)
    rs = [torch.randn(o.shape, generator=torch.Generator().manual_seed(40 + i)) for i, o in enumerate(outs)]
    o_ref, p_ref, x_ref = T.backward(sd, xs, rs, forward_fn=R.fpn_forward, **cfg)              # autograd over fpn_ref itself
    o_own, p_own, x_own = T.backward(sd, xs, rs, **cfg)
    masks = None if cp else {3: o_own[3] > 0}                                                  # the ReLU'd level's own mask, imposed
    o_msk, p_msk, x_msk = T.backward(sd, xs, rs, relu_masks=masks, **cfg)
    for a, b, c in zip(o_ref, o_own, o_msk):
        assert torch.equal(a, b) and torch.equal(a, c)
    for k in p_ref:
        assert T.rel_fro(p_own[k], p_ref[k]) < 1e-12 and T.rel_fro(p_msk[k], p_ref[k]) < 1e-12, k
    for i, (a, b, c) in enumerate(zip(x_ref, x_own, x_msk)):
        if i < kw['start_level']:
            assert a is None and b is None and c is None
        else:
            assert T.rel_fro(b, a) < 1e-12 and T.rel_fro(c, a) < 1e-12
    # ... and the module's fp32 autograd on the torch route is the same backward
    xg = [x.clone().requires_grad_(i >= kw['start_level']) for i, x in enumerate(xs)]
    sum((o * r).sum() for o, r in zip(mod(xg), rs)).backward()
    for k, p in mod.named_parameters():
        assert T.rel_fro(p.grad, p_ref[k]) < 1e-5, k
    for a, b in zip(xg[kw['start_level']:], x_ref[kw['start_level']:]):
        assert T.rel_fro(a.grad, b) < 1e-5


def test_an_imposed_mask_changes_the_backward():
    """The hook is live: with every entry masked the ReLU'd level passes no gradient on."""
    sd = {'lateral_convs.0.conv.weight': torch.randn(256, 32, 1, 1), 'lateral_convs.0.conv.bias': torch.randn(256)}
    for k in range(3):
        sd[f'fpn_convs.{k}.conv.weight'], sd[f'fpn_convs.{k}.conv.bias'] = torch.randn(256, 256, 3, 3) * 0.02, torch.randn(256) * 0.1
    xs = [torch.randn(1, 32, 4, 6)]
    cfg = dict(start_level=0, num_outs=3, relu_before_extra_convs=True)
    rs = [torch.zeros(1, 256, 4, 6), torch.zeros(1, 256, 2, 3), torch.randn(1, 256, 1, 2)]
    _, p, _ = T.backward(sd, xs, rs, relu_masks={1: torch.zeros(1, 256, 2, 3, dtype=torch.bool)}, **cfg)
    assert float(p['fpn_convs.1.conv.weight'].abs().max()) == 0 and float(p['fpn_convs.2.conv.bias'].abs().max()) > 0


def test_topdown_children_partition_the_fine_grid():
    """For all 1 <= coarse <= fine <= 64: the candidates the kernel tests hold every child, each fine index is the child of exactly
    one coarse index, and the children are the nearest_index preimages."""
    pairs = 0
    for n_fine in range(1, 65):
        for n_coarse in range(1, n_fine + 1):
            kids = T.topdown_children(n_coarse, n_fine)
            flat = [d for c in kids for d in c]
            assert flat == list(range(n_fine)), (n_coarse, n_fine)                 # a partition, in order
            src = R.nearest_index(torch.arange(n_fine), n_coarse, n_fine).tolist()
            assert all(src[d] == c for c, ks in enumerate(kids) for d in ks)
            pairs += 1
    assert pairs == 64 * 65 // 2
    assert [len(k) for k in T.topdown_children(7, 13)] == [2, 2, 2, 2, 2, 2, 1] and len(T.topdown_children(4, 13)) == 4
    g = torch.randn(2, 3, 13, 21, dtype=torch.float64)
    adj = T.upsample_adjoint(g, (7, 11))
    ky, kx = T.topdown_children(7, 13), T.topdown_children(11, 21)
    want = torch.stack([torch.stack([g[..., ys, :][..., xs].sum((-2, -1)) for xs in kx], -1) for ys in ky], -2)
    assert torch.allclose(adj, want, rtol=0, atol=1e-12)


def test_abi_stays_56_and_declares_the_training_entry_points(repo_root):
    from graph_detr4d_amd import _lib
    hdr = open(os.path.join(repo_root, 'include', 'gd4d.h')).read()
    assert re.search(r'#define GD4D_ABI_VERSION 56\b', hdr) and _lib.ABI_VERSION == 56 and _lib.load().gd4d_abi_version() == 56
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and re.search(rf'\b{name}\s*\(', hdr)


def test_training_entry_points_validate_before_any_gpu_work():
    from graph_detr4d_amd import _lib
    lib = _lib.load()
    EINVAL, EUNSUPPORTED, EALIGN = -1, -2, -3
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 96)()
    ptr = ctypes.c_void_p((ctypes.addressof(buf) + 63) & ~63)
    odd = ctypes.c_void_p(ptr.value + 4)
    # transposed image
    assert lib.gd4d_fpn_lateral_image_mode_bytes(512, 0) == lib.gd4d_fpn_lateral_image_bytes(512)
    assert lib.gd4d_fpn_lateral_image_mode_bytes(32, 1) == lib.gd4d_fpn_lateral_image_mode_bytes(256, 1) == 8 * 32768
    assert lib.gd4d_fpn_lateral_image_mode_bytes(288, 1) == 2 * 8 * 32768 and lib.gd4d_fpn_lateral_image_mode_bytes(2048, 1) == 8 * 8 * 32768
    for cin in (0, 16, 48, 2080, -32):
        assert lib.gd4d_fpn_lateral_image_mode_bytes(cin, 1) == 0
        assert lib.gd4d_fpn_lateral_image_mode(ptr, cin, 256, 1, ptr, null) == EUNSUPPORTED
    assert lib.gd4d_fpn_lateral_image_mode_bytes(64, 2) == 0 and lib.gd4d_fpn_lateral_image_mode(ptr, 64, 256, 2, ptr, null) == EUNSUPPORTED
    assert lib.gd4d_fpn_lateral_image_mode(null, 64, 256, 1, ptr, null) == EINVAL
    assert lib.gd4d_fpn_lateral_image_mode(ptr, 64, 256, 1, null, null) == EINVAL
    assert lib.gd4d_fpn_lateral_image_mode(ptr, 64, 128, 1, ptr, null) == EUNSUPPORTED
    assert lib.gd4d_fpn_lateral_image_mode(ptr, 64, 256, 1, odd, null) == EALIGN
    assert lib.gd4d_fpn_lateral_image_mode(null, 64, 256, 0, ptr, null) == EINVAL                # (mode 0 is gd4d_fpn_lateral_image)

    def dgrad(g=ptr, n=2, cin=64, h=13, w=21, image=ptr, dx=ptr):
        return lib.gd4d_fpn_lateral_dgrad(g, n, cin, h, w, image, dx, null)
    assert dgrad(g=null) == EINVAL and dgrad(image=null) == EINVAL and dgrad(dx=null) == EINVAL and dgrad(h=0) == EINVAL and dgrad(w=-1) == EINVAL
    assert dgrad(n=0) == EUNSUPPORTED and dgrad(cin=48) == EUNSUPPORTED and dgrad(cin=4096) == EUNSUPPORTED and dgrad(image=odd) == EALIGN

    assert lib.gd4d_fpn_lateral_wgrad_workspace_bytes(64, 3) == 3 * 256 * 65 * 4
    assert lib.gd4d_fpn_lateral_wgrad_workspace_bytes(48, 3) == 0 and lib.gd4d_fpn_lateral_wgrad_workspace_bytes(64, 0) == 0
    assert lib.gd4d_fpn_lateral_wgrad_workspace_bytes(64, 4097) == 0
    assert lib.gd4d_fpn_lateral_wgrad_tiles(2, 13, 21) == 10 and lib.gd4d_fpn_lateral_wgrad_tiles(3, 1, 2) == 3
    assert lib.gd4d_fpn_lateral_wgrad_tiles(0, 13, 21) == 0 and lib.gd4d_fpn_lateral_wgrad_tiles(2, 0, 21) == 0

    def wgrad(g=ptr, x=ptr, n=2, cin=64, h=13, w=21, parts=4, ws=ptr, dw=ptr, db=ptr):
        return lib.gd4d_fpn_lateral_wgrad(g, x, n, cin, h, w, parts, ws, dw, db, null)
    assert wgrad(g=null) == EINVAL and wgrad(x=null) == EINVAL and wgrad(ws=null) == EINVAL and wgrad(dw=null) == EINVAL
    assert wgrad(db=null) == EINVAL and wgrad(h=0) == EINVAL
    assert wgrad(n=0) == EUNSUPPORTED and wgrad(cin=48) == EUNSUPPORTED and wgrad(parts=0) == EUNSUPPORTED and wgrad(parts=4097) == EUNSUPPORTED
    assert wgrad(ws=odd) == EALIGN

    def topdown(fine=ptr, n=2, c=256, h=13, w=21, coarse=ptr, hc=7, wc=11):
        return lib.gd4d_fpn_topdown_bwd(fine, n, c, h, w, coarse, hc, wc, null)
    assert topdown(fine=null) == EINVAL and topdown(coarse=null) == EINVAL and topdown(h=0) == EINVAL and topdown(wc=0) == EINVAL
    assert topdown(c=128) == EUNSUPPORTED and topdown(n=0) == EUNSUPPORTED and topdown(hc=14) == EUNSUPPORTED and topdown(wc=22) == EUNSUPPORTED

    def xdgrad(dy=ptr, n=2, c=256, h=4, w=6, image=ptr, mask=null, add=null, dx=ptr):
        return lib.gd4d_fpn_extra_conv_dgrad(dy, n, c, h, w, image, mask, add, dx, null)
    assert xdgrad(dy=null) == EINVAL and xdgrad(image=null) == EINVAL and xdgrad(dx=null) == EINVAL and xdgrad(h=0) == EINVAL
    assert xdgrad(c=128) == EUNSUPPORTED and xdgrad(n=0) == EUNSUPPORTED and xdgrad(image=odd) == EALIGN

    def xwgrad(dy=ptr, x=ptr, n=2, c=256, h=4, w=6, relu=0, dw=ptr, db=ptr):
        return lib.gd4d_fpn_extra_conv_wgrad(dy, x, n, c, h, w, relu, dw, db, null)
    assert xwgrad(dy=null) == EINVAL and xwgrad(x=null) == EINVAL and xwgrad(dw=null) == EINVAL and xwgrad(w=0) == EINVAL
    assert xwgrad(c=128) == EUNSUPPORTED and xwgrad(n=0) == EUNSUPPORTED and xwgrad(relu=2) == EUNSUPPORTED

    def bias(g=ptr, n=2, c=256, h=4, w=6, ws=ptr, db=ptr):
        return lib.gd4d_fpn_bias_grad(g, n, c, h, w, ws, db, null)
    assert bias(g=null) == EINVAL and bias(ws=null) == EINVAL and bias(db=null) == EINVAL and bias(h=-1) == EINVAL
    assert bias(c=128) == EUNSUPPORTED and bias(n=0) == EUNSUPPORTED


def test_training_ops_refuse_cpu_tensors():
    from graph_detr4d_amd import _lib, ops
    z = torch.zeros
    img = z(16, dtype=torch.uint8)
    with pytest.raises(_lib.Gd4dError):
        ops.fpn_lateral_image_t(z(256, 64, 1, 1))
    with pytest.raises(_lib.Gd4dError):
        ops.fpn_lateral_image_t(z(256, 48, 1, 1))
    with pytest.raises(_lib.Gd4dError):
        ops.fpn_lateral_dgrad(z(2, 256, 4, 6), img, 64)
    with pytest.raises(_lib.Gd4dError):
        ops.fpn_lateral_wgrad(z(2, 256, 4, 6), z(2, 64, 4, 6), partitions=1)
    with pytest.raises(_lib.Gd4dError):
        ops.fpn_topdown_bwd(z(2, 256, 4, 6), z(2, 256, 2, 3))
    with pytest.raises(_lib.Gd4dError):
        ops.fpn_extra_conv_dgrad(z(2, 256, 2, 3), img, (4, 6))
    with pytest.raises(_lib.Gd4dError):
        ops.fpn_extra_conv_wgrad(z(2, 256, 2, 3), z(2, 256, 4, 6))
    with pytest.raises(_lib.Gd4dError):
        ops.fpn_bias_grad(z(2, 256, 4, 6))
