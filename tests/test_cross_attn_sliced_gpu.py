"""Channel-sliced aggregate-then-project gather (gd4d_pyramid_slice_planar_fwd, gd4d_cross_attn_plan_fwd,
gd4d_cross_attn_agg_sliced_fwd) through the C ABI: against golden vectors captured from the reference (incl. the B = 2
row-pairing quirk), against the CPU oracle, against the one-workgroup-per-query aggregate kernel, and on every pyramid
source it can read (its own slice-planar copy, the pixel-major copy, caller-owned channels-last levels in place).
GPU only."""
import pytest
import torch

from golden_io import Golden

pytestmark = pytest.mark.gpu

ATOL = RTOL = 1e-4        # fp32 path: only summation order differs from the reference (north_star: 1e-3)


ITEMS = True              # module default of _sliced: the plan form of the inference step (32-byte items; the gather works out the
                          # corners and wsum); every test below also checks it against the pairs form, bit for bit


def _sliced_form(items, pyr, ref, offsets, attn, cam, l2i, pc_range, img_h, img_w, heads=8, order=None, want=False, slices=None):
    from graph_detr4d_amd import ops
    b, q = ref.shape[0], ref.shape[1]
    res = ops.cross_attn_plan_fwd(pyr, ref, offsets, attn, cam, l2i, pc_range, img_h, img_w, heads,
                                  want_mask=want, want_uv=want, query_order=order, items=items)
    plan = res[0] if want else res
    if items:
        plan.wsum.fill_(float('nan'))                # the gather (slice 0) must write every row
    if slices is None:
        agg = ops.cross_attn_agg_sliced_fwd(plan)
    else:                                            # the slices in several launches, any order
        agg = torch.full((b, q, heads, 256), float('nan'), device=ref.device)
        for lo, n in slices:
            ops.cross_attn_agg_sliced_fwd(plan, slices=(lo, n), agg=agg)
    return (agg, plan.wsum) + (tuple(res[1:]) if want else ())


def _sliced(*args, **kwargs):
    """Both forms of the plan - pairs, items - must agree bit for bit (same products, same order); returns the items form's result."""
    from graph_detr4d_amd import ops
    got = _sliced_form(ITEMS, *args, **kwargs)
    other = _sliced_form(not ITEMS, *args, **kwargs)
    for a, b in zip(got, other):
        assert torch.equal(a, b), 'items form and pairs form of the plan disagree'
    pyr, ref, offsets = args[0], args[1], args[2]
    if not kwargs.get('want') and kwargs.get('slices') is None:
        # both forms from ONE launch (a training step): the pairs region is the pairs-only plan byte for byte, the forward gather
        # on its items region gives the same aggregate
        attn, cam, l2i, pc_range, img_h, img_w = args[3:9]
        heads, order = kwargs.get('heads', 8), kwargs.get('order')
        both = ops.cross_attn_plan_fwd(pyr, ref, offsets, attn, cam, l2i, pc_range, img_h, img_w, heads, query_order=order, both=True)
        pairs = ops.cross_attn_plan_fwd(pyr, ref, offsets, attn, cam, l2i, pc_range, img_h, img_w, heads, query_order=order)
        assert both.buf.numel() == 2 * pairs.buf.numel() and not both.items
        hdr = ops._lib.load().gd4d_cross_attn_plan_bytes(ref.shape[0], pyr.rows // ref.shape[0], ref.shape[1], heads, offsets.shape[3])
        assert hdr == pairs.buf.numel()
        assert torch.equal(both.wsum, pairs.wsum)
        agg_b = ops.cross_attn_agg_sliced_fwd(both)
        assert torch.equal(agg_b, got[0]) and torch.equal(both.wsum, got[1])
        both.items_buf = None                            # ... and the pairs of the same buffer through the pairs gather
        assert torch.equal(ops.cross_attn_agg_sliced_fwd(both), got[0])
    return got


def test_items_plan_is_refused_by_the_training_kernels():
    from graph_detr4d_amd import _lib, ops, synthetic
    torch.manual_seed(1)
    fd = [torch.randn(1, 6, 256, h, w).cuda() for h, w in [(16, 28), (8, 14)]]
    sp, shp = ops.pyramid_slice_planar_fwd(fd)
    l2i = torch.from_numpy(synthetic.camera_rig(1)).unsqueeze(0).cuda()
    plan = ops.cross_attn_plan_fwd(ops.PyramidView.slice_planar(sp, shp), torch.rand(1, 9, 3).cuda(), torch.randn(1, 9, 8, 4, 3).cuda(),
                                   torch.randn(1, 9, 8, 2, 4).cuda(), torch.randn(1, 9, 6).cuda(), l2i, synthetic.PC_RANGE, 900, 1600, 8,
                                   items=True)
    with pytest.raises(_lib.Gd4dError):
        ops.cross_attn_dot_sliced(plan, torch.zeros(1, 9, 8, 256).cuda())


def test_slice_planar_is_the_reference_flatten_transpose_cat():
    """deform3d_cross_attn.py:264-276 with the channel axis cut into 8 planes: sp[s, r, pixel, k] = flat[r, pixel, 32 s + k]."""
    from graph_detr4d_amd import ops
    from oracle import torch_oracle as O
    torch.manual_seed(3)
    feats = [torch.randn(1, 5, 256, h, w) for h, w in [(29, 50), (15, 25), (8, 13), (3, 5)]]   # odd sizes: partial tiles
    flat, shapes = O.flatten_pyramid(feats)
    want = flat.reshape(5, -1, 8, 32).permute(2, 0, 1, 3).contiguous()
    fd = [f.cuda() for f in feats]
    sp, got_shapes = ops.pyramid_slice_planar_fwd(fd)
    assert list(map(tuple, got_shapes)) == list(map(tuple, shapes))
    assert torch.equal(sp.cpu(), want)
    for cus in (1, 8, 224, 4096):                                # the persistent form: one workgroup on each of `cus` CUs
        assert torch.equal(ops.pyramid_slice_planar_fwd(fd, max_cus=cus)[0], sp), cus
    sp16, _ = ops.pyramid_slice_planar_fwd(fd, out_dtype=torch.bfloat16)
    assert sp16.dtype == torch.bfloat16 and torch.equal(sp16.cpu(), want.bfloat16())
    assert torch.equal(ops.pyramid_slice_planar_fwd(fd, out_dtype=torch.bfloat16, max_cus=8)[0], sp16)


@pytest.mark.parametrize('name', ['deform_n6', 'deform_n12_depth', 'deform_edge', 'deform_n24_b2'])
def test_sliced_matches_reference_golden(name):
    """mask / uv bit-exact, value_proj of the aggregates = the reference's MSDA output summed over cameras; deform_n24_b2
    pins the B > 1 pairing of value row i with the logits of batch (i % B) (deform3d_cross_attn.py:277)."""
    from graph_detr4d_amd import ops
    g = Golden(name)
    m = g.meta
    b, n, q = m['batch'], m['num_cams'], m['num_query']
    sd = g.state()
    dev = 'cuda'
    l2i = torch.from_numpy(g.arrays['lidar2img']).unsqueeze(0).expand(b, -1, -1, -1).contiguous().to(dev)
    feats = [f.to(dev) for f in g.feats()]
    sp, shapes = ops.pyramid_slice_planar_fwd(feats)
    pyr = ops.PyramidView.slice_planar(sp, shapes)
    agg, wsum, mask, uv = _sliced(pyr, g.t('reference_points').to(dev), g.t('offsets').view(b, q, 8, 4, 3).contiguous().to(dev),
                                  g.t('attn_logits').view(b, q, 8, 4, 4).contiguous().to(dev), g.t('cam_logits').to(dev), l2i,
                                  m['pc_range'], m['img_shape'][0], m['img_shape'][1], want=True)
    out = ops.value_proj_heads_fwd(agg, wsum, sd['value_proj.weight'].to(dev), sd['value_proj.bias'].to(dev))
    gmask = g.t('mask').view(b, n, q, 8, 4, 4)[..., 0, :]
    guv = g.t('uv').view(b, n, q, 8, 4, 4, 2)[..., 0, :, :]
    assert torch.equal(mask.cpu(), gmask), 'visibility mask must be bit-exact'
    assert torch.equal(uv.cpu(), guv), 'projected coordinates must be bit-exact'
    torch.testing.assert_close(out.cpu(), g.t('agg'), rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize('heads,levels,n,q,b', [
    (8, [(29, 50), (15, 25), (8, 13), (4, 7)], 12, 300, 1),
    (8, [(16, 28)], 6, 64, 1),
    (8, [(16, 28), (8, 14)], 7, 50, 1),
    (8, [(16, 28), (8, 14), (4, 7)], 1, 33, 1),
    (4, [(16, 28), (8, 14), (4, 7), (2, 4)], 6, 40, 1),
    (16, [(16, 28), (8, 14), (4, 7), (2, 4)], 6, 40, 1),
    (8, [(12, 20), (6, 10), (3, 5), (2, 3)], 64, 20, 1),
    (8, [(16, 28), (8, 14), (4, 7), (2, 4)], 6, 37, 3),
])
def test_sliced_vs_oracle_and_other_kernels(heads, levels, n, q, b):
    """Every compiled (heads, levels) form against the plain-torch oracle (value_proj then sample_aggregate, incl. B > 1),
    against gd4d_cross_attn_agg_fwd (B = 1) and on all three pyramid sources; locality order and split launches are
    scheduling only (bit-identical)."""
    from graph_detr4d_amd import ops, synthetic
    from oracle import torch_oracle as O
    torch.manual_seed(heads * 100 + len(levels) * 10 + n + b)
    dh, nl = 256 // heads, len(levels)
    rig = synthetic.camera_rig((n + 5) // 6)[:n]
    l2i = torch.from_numpy(rig).unsqueeze(0).expand(b, -1, -1, -1).contiguous()
    feats = [torch.randn(b, n, 256, h, w) for h, w in levels]
    w, bias = torch.randn(256, 256) * 0.06, torch.randn(256)
    ref = torch.rand(b, q, 3)
    offsets = torch.randn(b, q, heads, 4, 3) * 2.0
    attn = torch.randn(b, q, heads, nl, 4)
    cam = torch.randn(b, q, n)
    flat, shapes = O.flatten_pyramid(feats)
    val = torch.nn.functional.linear(flat, w, bias).view(b * n, -1, heads, dh)
    o_ref, uv_ref, m_ref = O.sample_aggregate(val, shapes, ref, offsets, attn.flatten(-2), cam, l2i, synthetic.PC_RANGE, 900, 1600)
    dev = 'cuda'
    d = [t.to(dev) for t in (ref, offsets, attn, cam, l2i)]
    fd = [f.to(dev) for f in feats]
    sp, shp = ops.pyramid_slice_planar_fwd(fd)
    pyr = ops.PyramidView.slice_planar(sp, shp)
    agg, wsum, mask, uv = _sliced(pyr, *d, synthetic.PC_RANGE, 900, 1600, heads=heads, want=True)
    out = ops.value_proj_heads_fwd(agg, wsum, w.to(dev), bias.to(dev))
    mism = mask.cpu() != m_ref.to(torch.uint8)
    flipped = mism.any(dim=4).any(dim=3).any(dim=1)                  # (B, Q): torch's matmul decides m_ref on this host
    assert flipped.sum().item() <= 2
    keep = ~flipped
    torch.testing.assert_close(out.cpu()[keep], o_ref[keep], rtol=RTOL, atol=ATOL)
    if b == 1:
        cl, _ = ops.pyramid_channels_last_fwd(fd)
        a0, s0, m0, u0 = ops.cross_attn_agg_fwd(cl, shp, *d, synthetic.PC_RANGE, 900, 1600, heads, want_mask=True, want_uv=True)
        assert torch.equal(mask, m0) and torch.equal(uv, u0)         # one projection routine in all kernels
        torch.testing.assert_close(agg, a0, rtol=2e-5, atol=2e-5)
        torch.testing.assert_close(wsum, s0, rtol=1e-5, atol=1e-6)
        # the pixel-major copy read through strides
        a1, s1 = _sliced(ops.PyramidView.pixel_major(cl, shp), *d, synthetic.PC_RANGE, 900, 1600, heads=heads)
        assert torch.equal(a1, agg) and torch.equal(s1, wsum)
    # caller-owned channels-last levels, read in place (no copy)
    nhwc = [f.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3) for f in fd]
    assert all(ops.PyramidView.is_channels_last_level(t) for t in nhwc) and not ops.PyramidView.is_channels_last_level(fd[0])
    a2, s2 = _sliced(ops.PyramidView.channels_last_levels(nhwc), *d, synthetic.PC_RANGE, 900, 1600, heads=heads)
    assert torch.equal(a2, agg) and torch.equal(s2, wsum)
    # scheduling only: locality order, slices in separate launches
    order = ops.query_order_fwd(d[0], synthetic.PC_RANGE)
    a3, s3 = _sliced(pyr, *d, synthetic.PC_RANGE, 900, 1600, heads=heads, order=order)
    assert torch.equal(a3, agg) and torch.equal(s3, wsum)
    a4, s4 = _sliced(pyr, *d, synthetic.PC_RANGE, 900, 1600, heads=heads, order=order, slices=[(4, 4), (0, 3), (3, 1)])
    assert torch.equal(a4, agg) and torch.equal(s4, wsum)
    # wsum is the sum of the in-bounds weights: with a zero weight matrix the output is bias * wsum
    out0 = ops.value_proj_heads_fwd(agg, wsum, torch.zeros_like(w).to(dev), bias.to(dev))
    torch.testing.assert_close(out0, (bias.to(dev).view(heads, dh) * wsum.unsqueeze(-1)).reshape(b, q, 256), rtol=1e-6, atol=1e-6)


def test_bf16_storage_sliced():
    """value_dtype='bf16': bf16-rounded features (copy or caller-owned), fp32 accumulation - equals the fp32 kernel on the
    same rounded features within summation order."""
    from graph_detr4d_amd import ops, synthetic
    torch.manual_seed(13)
    levels = [(29, 50), (15, 25), (8, 13), (3, 5)]
    n, q = 6, 200
    fd = [torch.randn(1, n, 256, h, w).cuda() for h, w in levels]
    l2i = torch.from_numpy(synthetic.camera_rig(1)).unsqueeze(0).cuda()
    ref, off = torch.rand(1, q, 3).cuda(), (torch.randn(1, q, 8, 4, 3) * 2).cuda()
    attn, cam = torch.randn(1, q, 8, 4, 4).cuda(), torch.randn(1, q, n).cuda()
    args = (ref, off, attn, cam, l2i, synthetic.PC_RANGE, 900, 1600)
    sp16, shp = ops.pyramid_slice_planar_fwd(fd, out_dtype=torch.bfloat16)
    a16, s16 = _sliced(ops.PyramidView.slice_planar(sp16, shp), *args)
    a32, s32 = _sliced(ops.PyramidView.slice_planar(sp16.float(), shp), *args)
    assert torch.equal(s16, s32)
    torch.testing.assert_close(a16, a32, rtol=1e-6, atol=1e-6)
    nhwc16 = [f.bfloat16().permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3) for f in fd]
    a16b, s16b = _sliced(ops.PyramidView.channels_last_levels(nhwc16), *args)
    assert torch.equal(a16b, a16) and torch.equal(s16b, s16)


def test_full_size_sliced_equals_rows_and_early():
    """BASELINE configs[2] size (900 queries, 24 cameras, R50 pyramid): the sliced gather against the one-workgroup-per-
    query aggregate kernel (summation order only) and against the projected-value path within 1e-3 (north_star)."""
    from graph_detr4d_amd import ops, synthetic
    dev = 'cuda'
    g = torch.Generator(device='cpu').manual_seed(21)
    b, q, n = 1, 900, 24
    feats = [torch.randn(b, n, 256, h, w, generator=g).to(dev) for h, w in synthetic.R50_LEVELS]
    w = (torch.randn(256, 256, generator=g) * 0.06).to(dev)
    bias = torch.randn(256, generator=g).to(dev)
    l2i = torch.from_numpy(synthetic.camera_rig(4)).unsqueeze(0).to(dev)
    ref = torch.rand(b, q, 3, generator=g).to(dev)
    offsets = (torch.randn(b, q, 8, 4, 3, generator=g) * 2).to(dev)
    attn = torch.randn(b, q, 8, 4, 4, generator=g).to(dev)
    cam = torch.randn(b, q, n, generator=g).to(dev)
    args = (ref, offsets, attn, cam, l2i, synthetic.PC_RANGE, 900, 1600)
    order = ops.query_order_fwd(ref, synthetic.PC_RANGE)
    sp, shapes = ops.pyramid_slice_planar_fwd(feats, max_cus=224)
    agg, wsum, mask, uv = _sliced(ops.PyramidView.slice_planar(sp, shapes), *args, order=order, want=True)
    cl, _ = ops.pyramid_channels_last_fwd(feats)
    a0, s0, m0 = ops.cross_attn_agg_fwd(cl, shapes, *args, 8, want_mask=True, query_order=order)
    assert torch.equal(mask, m0)
    torch.testing.assert_close(agg, a0, rtol=2e-5, atol=2e-5)
    torch.testing.assert_close(wsum, s0, rtol=1e-5, atol=1e-6)
    out = ops.value_proj_heads_fwd(agg, wsum, w, bias)
    val = ops.value_proj_fwd(feats, w, bias).view(b * n, -1, 8, 32)
    early = ops.cross_attn_fwd(val, shapes, *args)
    assert (out - early).abs().max().item() < 1e-3
    assert out.abs().max().item() > 0.1
    # run-to-run identical (fixed summation order)
    agg2, wsum2 = _sliced(ops.PyramidView.slice_planar(sp, shapes), *args, order=order)
    assert torch.equal(agg, agg2) and torch.equal(wsum, wsum2)


def test_transformer_on_channels_last_levels_equals_the_copied_path():
    """Detr3DTransformer fed (B, N, C, H, W) levels stored channels-last: no copy kernel is launched (the gather reads the
    caller's tensors through per-level pointers and strides) and the result is the copied path's, bit for bit - fp32 and,
    with value_dtype='bf16' modules, bf16 levels (equal to the bf16 slice-planar copy of the fp32 levels)."""
    import graph_detr4d_amd as G
    from graph_detr4d_amd import functional as Fn, ops
    g = Golden('decoder_deform')
    m = g.meta
    n = m['num_cams']

    def build(value_dtype):
        tr = G.build_transformer(dict(
            type='Detr3DTransformer', num_feature_levels=4, num_cams=n,
            decoder=dict(type='Detr3DTransformerDecoder', num_layers=m['num_layers'], return_intermediate=True,
                         transformerlayers=dict(
                             type='DetrTransformerDecoderLayer',
                             attn_cfgs=[dict(type='MultiheadAttention', embed_dims=256, num_heads=8, dropout=0.1),
                                        dict(type='Deform3DCrossAttn', num_cams=n, pc_range=m['pc_range'], num_points=4,
                                             embed_dims=256, value_dtype=value_dtype)],
                             feedforward_channels=512, ffn_dropout=0.1,
                             operation_order=('self_attn', 'norm', 'cross_attn', 'norm', 'ffn', 'norm')))))
        tr.load_state_dict(g.state(), strict=True)
        return tr.cuda().eval()
    nn = torch.nn
    regs = nn.ModuleList([nn.Sequential(nn.Linear(256, 256), nn.ReLU(), nn.Linear(256, 256), nn.ReLU(),
                                        nn.Linear(256, 10)) for _ in range(m['num_layers'])])
    regs.load_state_dict(g.state(prefix='reg.'), strict=True)
    regs = regs.cuda().eval()
    feats = [f.cuda() for f in g.feats()]
    qe, metas = g.t('query_embed').cuda(), g.img_metas()
    copies = []
    orig = ops.pyramid_slice_planar_fwd

    def counting(*a, **k):
        copies.append(1)
        return orig(*a, **k)
    ops.pyramid_slice_planar_fwd = counting
    try:
        for value_dtype, store in (('fp32', torch.float32), ('bf16', torch.bfloat16)):
            tr = build(value_dtype)
            nhwc = [f.to(store).permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3) for f in feats]
            assert Fn.LateValues.applicable([tr.decoder.layers[0].attentions[1]], nhwc)
            with torch.no_grad():
                del copies[:]
                want = tr(feats, qe, reg_branches=regs, img_metas=metas)
                assert len(copies) == 1
                got = tr(nhwc, qe, reg_branches=regs, img_metas=metas)
                assert len(copies) == 1, 'channels-last levels must be gathered in place'
            for a, b in zip(got, want):
                assert torch.equal(a, b), value_dtype
            if value_dtype == 'fp32':
                torch.testing.assert_close(got[0].cpu(), g.t('inter_states'), rtol=1e-3, atol=1e-3)
    finally:
        ops.pyramid_slice_planar_fwd = orig


@pytest.mark.parametrize('seed', range(8))
def test_sliced_random_configurations_vs_plain_c_oracle(seed):
    """Seeded random shapes (cameras 1 .. 64, queries 1 .. 200, 1 - 4 levels of odd sizes, 4 / 8 / 16 heads), reference points
    that straddle the image borders and the eps plane, random rigs: agg / wsum through value_proj against the plain-C oracle
    (oracle/gd4d_oracle.c) fed the projected values; mask and uv bit-exact."""
    import numpy as np
    from graph_detr4d_amd import ops, synthetic
    from oracle import c_oracle
    from oracle import torch_oracle as O
    rng = np.random.default_rng(1000 + seed)
    heads = int(rng.choice([4, 8, 16]))
    nl = int(rng.integers(1, 5))
    n = int(rng.choice([1, 2, 5, 6, 12, 24, 37, 64]))
    q = int(rng.integers(1, 201))
    levels = [(int(rng.integers(2, 34)), int(rng.integers(2, 50))) for _ in range(nl)]
    torch.manual_seed(seed)
    rig = synthetic.camera_rig((n + 5) // 6)[:n].copy()
    rig[:, :3, 3] += rng.normal(0, 0.5, (n, 3)).astype(np.float32)          # jitter the translations
    l2i = torch.from_numpy(rig).unsqueeze(0).contiguous()
    feats = [torch.randn(1, n, 256, h, w) for h, w in levels]
    w, bias = torch.randn(256, 256) * 0.06, torch.randn(256)
    ref = torch.rand(1, q, 3)
    ref[0, : q // 4] = torch.round(ref[0, : q // 4] * 8) / 8                # some points on coarse grid values
    offsets = torch.randn(1, q, heads, 4, 3) * float(rng.choice([0.1, 2.0, 8.0]))
    attn = torch.randn(1, q, heads, nl, 4) * 2
    cam = torch.randn(1, q, n) * 2
    flat, shapes = O.flatten_pyramid(feats)
    val = torch.nn.functional.linear(flat, w, bias).view(n, -1, heads, 256 // heads).contiguous()
    o_c, m_c, uv_c = c_oracle.cross_attn_fwd(val.numpy(), shapes, ref.numpy(), offsets.numpy(), attn.flatten(-2).numpy(), cam.numpy(),
                                             l2i.numpy(), synthetic.PC_RANGE, 900, 1600)
    dev = 'cuda'
    sp, shp = ops.pyramid_slice_planar_fwd([f.to(dev) for f in feats])
    order = ops.query_order_fwd(ref.to(dev), synthetic.PC_RANGE) if seed % 2 else None
    agg, wsum, mask, uv = _sliced(ops.PyramidView.slice_planar(sp, shp), ref.to(dev), offsets.to(dev), attn.to(dev), cam.to(dev),
                                  l2i.to(dev), synthetic.PC_RANGE, 900, 1600, heads=heads, order=order, want=True)
    assert np.array_equal(mask.cpu().numpy(), m_c) and np.array_equal(uv.cpu().numpy(), uv_c)
    out = ops.value_proj_heads_fwd(agg, wsum, w.to(dev), bias.to(dev))
    np.testing.assert_allclose(out.cpu().numpy(), o_c, rtol=RTOL, atol=ATOL)


def _coarse_groups(pyr, coarse, args):
    """{slices per fine workgroup: (agg, wsum, pagg)} of gd4d_cross_attn_agg_items_coarse_fwd on `pyr`, 1, 2, 4 and 8 slices per
    workgroup; the gather has to write every element of all three."""
    from graph_detr4d_amd import ops
    b, q = args[0].shape[0], args[0].shape[1]
    plan = ops.cross_attn_plan_fwd(pyr, *args, 8, items=True)
    out, was = {}, ops.gather_slice_group()
    try:
        for ns in (1, 2, 4, 8):
            ops.gather_slice_group(ns)
            plan.wsum.fill_(float('nan'))
            agg = torch.full((b, q, 8, 256), float('nan'), device=args[0].device)
            pagg = torch.full((b, q, 256), float('nan'), device=args[0].device)
            ops.cross_attn_agg_coarse_fwd(plan, coarse, agg=agg, pagg=pagg)
            out[ns] = (agg, plan.wsum.clone(), pagg)
    finally:
        ops.gather_slice_group(was)
    return out


def test_levels_of_more_than_4_gib_are_gathered_in_place():
    """VERDICT r3, missing #5: VoVNet-99 levels stored channels-last with two samples - level 0 alone is 2 x 24 x 232 x 400 x 1 KB
    = 4.56 GB, past the 32-bit byte offsets of the pairs form.  The items form's gather switches to 16-byte units (64 GiB per
    level): results equal, bit for bit, the gather of the slice-planar copy of the same levels (757 MB per slice plane: narrow
    offsets), which tests/test_timed_size_parity_gpu.py and the cases above tie to the oracle.  The pairs form refuses.

    The same for the gather of the inference step, gd4d_cross_attn_agg_items_coarse_fwd (levels 0, 1 raw, levels 2, 3 from projected
    rows): agg, wsum and pagg on the wide levels equal those on the narrow copy for every slice-group size, fp32 and bf16 - a bf16
    level 0 is 2.28 GB, so the bf16 pixels are stored at the fp32 pixels' pitch of 1 KB, which makes the level as wide."""
    from graph_detr4d_amd import _lib, ops, synthetic
    gen = torch.Generator(device='cuda').manual_seed(17)
    b, n, q = 2, 24, 300
    fd = [torch.randn(b, n, 256, h, w, device='cuda', generator=gen) for h, w in synthetic.VOV_LEVELS]
    cg = torch.Generator().manual_seed(18)
    l2i = torch.from_numpy(synthetic.camera_rig(4)).unsqueeze(0).expand(b, -1, -1, -1).contiguous().cuda()
    ref, off = torch.rand(b, q, 3, generator=cg).cuda(), (torch.randn(b, q, 8, 4, 3, generator=cg) * 2).cuda()
    attn, cam = torch.randn(b, q, 8, 4, 4, generator=cg).cuda(), torch.randn(b, q, n, generator=cg).cuda()
    args = (ref, off, attn, cam, l2i, synthetic.PC_RANGE, 900, 1600)
    sp, shp = ops.pyramid_slice_planar_fwd(fd)
    want_a, want_s, mask, _ = _sliced_form(True, ops.PyramidView.slice_planar(sp, shp), *args, want=True)
    assert 0.05 < mask.float().mean().item() < 0.4 and want_a.abs().max().item() > 0.1
    coarse = ops.CoarseValues(torch.randn(b * n, sum(h * w for h, w in shp[2:]), 256, device='cuda', generator=gen), shp[2:])
    want_c = _coarse_groups(ops.PyramidView.slice_planar(sp, shp), coarse, args)
    assert all(bool(torch.isfinite(t).all()) for t in want_c[1]) and want_c[1][2].abs().max().item() > 0.1
    del sp
    sp16, _ = ops.pyramid_slice_planar_fwd(fd, out_dtype=torch.bfloat16)
    want_c16 = _coarse_groups(ops.PyramidView.slice_planar(sp16, shp), coarse, args)
    assert not torch.equal(want_c16[1][0], want_c[1][0])
    del sp16
    nhwc = [f.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3) for f in fd]
    del fd
    view = ops.PyramidView.channels_last_levels(nhwc)
    assert (b * n - 1) * view.cam_stride[0] + shp[0][0] * shp[0][1] * view.pix_stride >= 2 ** 32       # level 0 really is wide
    got_a, got_s = _sliced_form(True, view, *args)
    assert torch.equal(got_a, want_a) and torch.equal(got_s, want_s)
    with pytest.raises(_lib.Gd4dError):
        _sliced_form(False, view, *args)
    for ns, got in _coarse_groups(view, coarse, args).items():
        for name, a, w in zip(('agg', 'wsum', 'pagg'), got, want_c[ns]):
            assert torch.equal(a, w), (name, ns)
    # bf16 pixels (512 bytes) at a pitch of 1 KB: the two fine levels only - the gather reads no other level raw
    padded = []
    for f in nhwc[:2]:
        buf = torch.zeros(b, n, f.shape[3], f.shape[4], 512, device='cuda', dtype=torch.bfloat16)
        buf[..., :256] = f.permute(0, 1, 3, 4, 2)
        padded.append(buf)
    del nhwc
    view16 = ops.PyramidView(padded, [padded[0].data_ptr()] + [padded[1].data_ptr()] * 3, shp, [h * w * 1024 for h, w in shp], 1024, 64,
                             torch.bfloat16, b * n)
    assert (b * n - 1) * view16.cam_stride[0] + shp[0][0] * shp[0][1] * view16.pix_stride >= 2 ** 32
    for ns, got in _coarse_groups(view16, coarse, args).items():
        for name, a, w in zip(('agg', 'wsum', 'pagg'), got, want_c16[ns]):
            assert torch.equal(a, w), (name, ns, 'bf16')


@pytest.mark.parametrize('points,levels,n,q,b', [(1, [(16, 28), (8, 14), (4, 7), (2, 4)], 6, 50, 1), (2, [(16, 28), (8, 14)], 12, 40, 1),
                                                 (8, [(16, 28), (8, 14), (4, 7), (2, 4)], 6, 33, 1), (8, [(12, 20)], 7, 20, 2),
                                                 (1, [(12, 20), (6, 10), (3, 5)], 24, 30, 2)])
def test_num_points_other_than_four_vs_plain_c_oracle(points, levels, n, q, b):
    """The reference's constructor takes any num_points (deform3d_cross_attn.py:52-69; every shipped config: 4).  1, 2 and 8
    points per head (8 heads) through plan + gather + value_proj of the aggregates against the plain-C oracle on the projected
    values: mask / uv bit-exact, both plan forms identical."""
    import numpy as np
    from graph_detr4d_amd import ops, synthetic
    from oracle import c_oracle
    rng = np.random.default_rng(points * 100 + n)
    nl = len(levels)
    feats = [rng.standard_normal((b, n, 256, h, w)).astype(np.float32) for h, w in levels]
    w_v, b_v = (rng.standard_normal((256, 256)) * 0.06).astype(np.float32), rng.standard_normal(256).astype(np.float32)
    ref = rng.random((b, q, 3)).astype(np.float32)
    offsets = (rng.standard_normal((b, q, 8, points, 3)) * 1.5).astype(np.float32)
    attn = rng.standard_normal((b, q, 8, nl, points)).astype(np.float32)
    cam = rng.standard_normal((b, q, n)).astype(np.float32)
    l2i = np.broadcast_to(synthetic.camera_rig((n + 5) // 6)[:n][None], (b, n, 4, 4)).astype(np.float32).copy()
    flat = np.concatenate([f.reshape(b * n, 256, -1).transpose(0, 2, 1) for f in feats], 1)               # (R, S, 256)
    val = (flat.astype(np.float64) @ w_v.astype(np.float64).T + b_v).astype(np.float32).reshape(b * n, -1, 8, 32)
    if b == 1:
        o_ref, m_ref, uv_ref = c_oracle.cross_attn_fwd(val, levels, ref, offsets, attn, cam, l2i, synthetic.PC_RANGE, 900, 1600)
    t = lambda a: torch.from_numpy(a).cuda()                # noqa: E731
    sp, shp = ops.pyramid_slice_planar_fwd([t(f) for f in feats])
    agg, wsum, mask, uv = _sliced(ops.PyramidView.slice_planar(sp, shp), t(ref), t(offsets), t(attn), t(cam), t(l2i), synthetic.PC_RANGE,
                                  900, 1600, want=True)
    out = ops.value_proj_heads_fwd(agg, wsum, t(w_v), t(b_v))
    assert mask.shape == (b, n, q, 8, points) and mask.sum().item() > 0
    if b == 1:
        assert np.array_equal(mask.cpu().numpy(), m_ref) and np.array_equal(uv.cpu().numpy(), uv_ref)
        np.testing.assert_allclose(out.cpu().numpy(), o_ref, rtol=1e-4, atol=1e-4)
    else:                                                    # B > 1 (the row % B pairing): against the torch oracle
        from oracle import torch_oracle as O
        o_t, _, m_t = O.sample_aggregate(torch.from_numpy(val), levels, torch.from_numpy(ref), torch.from_numpy(offsets),
                                         torch.from_numpy(attn).flatten(-2), torch.from_numpy(cam), torch.from_numpy(l2i),
                                         synthetic.PC_RANGE, 900, 1600)
        flipped = (mask.cpu() != m_t.to(torch.uint8)).any(dim=4).any(dim=3).any(dim=1)
        assert flipped.sum().item() <= 2
        torch.testing.assert_close(out.cpu()[~flipped], o_t[~flipped], rtol=1e-4, atol=1e-4)


def test_training_kernels_refuse_num_points_other_than_four():
    from graph_detr4d_amd import _lib, ops, synthetic
    torch.manual_seed(2)
    fd = [torch.randn(1, 6, 256, 16, 28).cuda()]
    sp, shp = ops.pyramid_slice_planar_fwd(fd)
    l2i = torch.from_numpy(synthetic.camera_rig(1)).unsqueeze(0).cuda()
    plan = ops.cross_attn_plan_fwd(ops.PyramidView.slice_planar(sp, shp), torch.rand(1, 9, 3).cuda(), torch.randn(1, 9, 8, 2, 3).cuda(),
                                   torch.randn(1, 9, 8, 1, 2).cuda(), torch.randn(1, 9, 6).cuda(), l2i, synthetic.PC_RANGE, 900, 1600, 8)
    assert plan.points == 2
    with pytest.raises(_lib.Gd4dError):
        ops.cross_attn_dot_sliced(plan, torch.zeros(1, 9, 8, 256).cuda())


def _coarse_layer(pyr, feats, w_v, b_v, args, heads=8, order=None):
    """One layer's sampled value through gd4d_cross_attn_agg_items_coarse_fwd: levels 0, 1 raw, levels 2, 3 projected first."""
    from graph_detr4d_amd import ops
    proj = ops.value_proj_fwd([f.contiguous() for f in feats[2:]], w_v, b_v)
    coarse = ops.CoarseValues(proj, [tuple(f.shape[-2:]) for f in feats[2:]])
    res = ops.cross_attn_plan_fwd(pyr, *args, heads, want_mask=True, want_uv=True, query_order=order, items=True)
    plan = res[0]
    plan.wsum.fill_(float('nan'))
    b, q = args[0].shape[0], args[0].shape[1]
    agg = torch.full((b, q, heads, 256), float('nan'), device=args[0].device)
    pagg = torch.full((b, q, 256), float('nan'), device=args[0].device)
    ops.cross_attn_agg_coarse_fwd(plan, coarse, agg=agg, pagg=pagg)
    return ops.value_proj_heads_fwd(agg, plan.wsum, w_v, b_v) + pagg, res[1], res[2]


@pytest.mark.parametrize('name', ['deform_n6', 'deform_n12_depth', 'deform_edge', 'deform_n24_b2'])
def test_coarse_projected_gather_matches_reference_golden(name):
    """gd4d_cross_attn_agg_items_coarse_fwd (levels 2, 3 gathered from value_proj's rows, levels 0, 1 raw) against the reference's
    MSDA output summed over cameras; mask / uv stay bit-exact (the plan is the same plan)."""
    from graph_detr4d_amd import ops
    g = Golden(name)
    m = g.meta
    b, n, q = m['batch'], m['num_cams'], m['num_query']
    sd = g.state()
    dev = 'cuda'
    l2i = torch.from_numpy(g.arrays['lidar2img']).unsqueeze(0).expand(b, -1, -1, -1).contiguous().to(dev)
    feats = [f.to(dev) for f in g.feats()]
    sp, shapes = ops.pyramid_slice_planar_fwd(feats)
    args = (g.t('reference_points').to(dev), g.t('offsets').view(b, q, 8, 4, 3).contiguous().to(dev),
            g.t('attn_logits').view(b, q, 8, 4, 4).contiguous().to(dev), g.t('cam_logits').to(dev), l2i,
            m['pc_range'], m['img_shape'][0], m['img_shape'][1])
    w_v, b_v = sd['value_proj.weight'].to(dev), sd['value_proj.bias'].to(dev)
    out, mask, uv = _coarse_layer(ops.PyramidView.slice_planar(sp, shapes), feats, w_v, b_v, args)
    assert torch.equal(mask.cpu(), g.t('mask').view(b, n, q, 8, 4, 4)[..., 0, :]), 'visibility mask must be bit-exact'
    assert torch.equal(uv.cpu(), g.t('uv').view(b, n, q, 8, 4, 4, 2)[..., 0, :, :]), 'projected coordinates must be bit-exact'
    torch.testing.assert_close(out.cpu(), g.t('agg'), rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize('levels,n,q,b,source', [
    ([(29, 50), (15, 25), (8, 13), (4, 7)], 12, 300, 1, 'planar'),
    ([(16, 28), (8, 14), (4, 7), (2, 4)], 6, 37, 3, 'planar'),
    ([(12, 20), (6, 10), (3, 5), (2, 3)], 64, 20, 1, 'nhwc'),
    ([(29, 50), (15, 25), (8, 13), (4, 7)], 7, 129, 2, 'pixel_major'),
])
def test_coarse_projected_gather_vs_the_raw_gather_and_the_oracle(levels, n, q, b, source):
    """The same layer through the all-raw items gather and through the coarse-projected one: equal to summation order (value_proj
    commutes with the bilinear sum), both equal to the torch oracle; on every pyramid source, with a locality order."""
    from graph_detr4d_amd import ops, synthetic
    from oracle import torch_oracle as O
    torch.manual_seed(len(levels) * 10 + n + b)
    rig = synthetic.camera_rig((n + 5) // 6)[:n]
    l2i = torch.from_numpy(rig).unsqueeze(0).expand(b, -1, -1, -1).contiguous()
    feats = [torch.randn(b, n, 256, h, w) for h, w in levels]
    ref = torch.rand(b, q, 3)
    offsets, attn, cam = torch.randn(b, q, 8, 4, 3) * 2.0, torch.randn(b, q, 8, 4, 4), torch.randn(b, q, n)
    w_v, b_v = torch.randn(256, 256) * 0.06, torch.randn(256)
    dev = 'cuda'
    fd = [f.to(dev) for f in feats]
    if source == 'planar':
        sp, shp = ops.pyramid_slice_planar_fwd(fd)
        pyr = ops.PyramidView.slice_planar(sp, shp)
    elif source == 'pixel_major':
        cl, shp = ops.pyramid_channels_last_fwd(fd)
        pyr = ops.PyramidView.pixel_major(cl, shp)
    else:
        nhwc = [f.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3) for f in fd]
        pyr = ops.PyramidView.channels_last_levels(nhwc)
    args = (ref.to(dev), offsets.to(dev), attn.to(dev), cam.to(dev), l2i.to(dev), synthetic.PC_RANGE, 900, 1600)
    order = ops.query_order_fwd(args[0], synthetic.PC_RANGE)
    out, mask, uv = _coarse_layer(pyr, fd, w_v.to(dev), b_v.to(dev), args, order=order)
    agg, wsum, mask_r, uv_r = _sliced_form(True, pyr, *args, order=order, want=True)
    raw = ops.value_proj_heads_fwd(agg, wsum, w_v.to(dev), b_v.to(dev))
    assert torch.equal(mask, mask_r) and torch.equal(uv, uv_r)
    torch.testing.assert_close(out, raw, rtol=RTOL, atol=ATOL)
    flat, shapes = O.flatten_pyramid(feats)
    val = torch.nn.functional.linear(flat, w_v, b_v).view(b * n, -1, 8, 32)
    want, _, m_ref = O.sample_aggregate(val, shapes, ref, offsets, attn.flatten(-2), cam, l2i, synthetic.PC_RANGE, 900, 1600)
    flipped = (mask.cpu() != m_ref.to(torch.uint8)).any(dim=4).any(dim=3).any(dim=1)   # (B, Q): torch's matmul decides m_ref on this host
    assert flipped.sum().item() <= 2
    torch.testing.assert_close(out.cpu()[~flipped], want[~flipped], rtol=RTOL, atol=ATOL)


def test_coarse_projected_gather_refuses_what_it_is_not_built_for():
    from graph_detr4d_amd import _lib, ops, synthetic
    torch.manual_seed(2)
    fd = [torch.randn(1, 6, 256, h, w).cuda() for h, w in [(16, 28), (8, 14), (4, 7)]]
    sp, shp = ops.pyramid_slice_planar_fwd(fd)
    l2i = torch.from_numpy(synthetic.camera_rig(1)).unsqueeze(0).cuda()
    plan = ops.cross_attn_plan_fwd(ops.PyramidView.slice_planar(sp, shp), torch.rand(1, 9, 3).cuda(), torch.randn(1, 9, 8, 4, 3).cuda(),
                                   torch.randn(1, 9, 8, 3, 4).cuda(), torch.randn(1, 9, 6).cuda(), l2i, synthetic.PC_RANGE, 900, 1600, 8,
                                   items=True)
    coarse = ops.CoarseValues(torch.zeros(6, 8 * 14 + 4 * 7, 256).cuda(), [(8, 14), (4, 7)])
    with pytest.raises(_lib.Gd4dError):
        ops.cross_attn_agg_coarse_fwd(plan, coarse)


def test_late_values_prepared_for_the_coarse_gather_still_serve_an_all_raw_consumer(monkeypatch):
    """LateValues(coarse_for=...) copies the two fine levels only and projects the first layer's coarse levels beside the copy - for the
    fused decoder loop.  A consumer that gathers every level raw after all (a module called on its own with this object) must get the
    full copy (made again, once) and the same result as from an object built for it."""
    import graph_detr4d_amd as G
    from graph_detr4d_amd import functional as Fn
    from graph_detr4d_amd import ops, synthetic
    monkeypatch.delenv('GD4D_COARSE', raising=False)              # (the default route, whatever the caller's environment says)
    torch.manual_seed(4)
    n, q = 6, 70
    levels = [(29, 50), (15, 25), (8, 13), (4, 7)]
    mod = G.build_attention(dict(type='Deform3DCrossAttn', num_cams=n, pc_range=synthetic.PC_RANGE, num_points=4, embed_dims=256)).cuda().eval()
    synthetic.randomise_cross_attn_(mod, seed=3)
    feats = [torch.randn(1, n, 256, h, w).cuda() for h, w in levels]
    l2i = torch.from_numpy(synthetic.camera_rig(1)).unsqueeze(0).cuda()
    ref, off = torch.rand(1, q, 3).cuda(), (torch.randn(1, q, 8, 4, 3) * 2).cuda()
    attn, cam = torch.randn(1, q, 8, 4, 4).cuda(), torch.randn(1, q, n).cuda()
    with torch.no_grad():
        plain = Fn.LateValues(feats)
        want_agg, want_wsum = plain.aggregate(mod, ref, off, attn, cam, l2i, 900, 1600)
        plain.finish()
        late = Fn.LateValues(feats, coarse_for=[mod])
        assert late.partial and late.coarse is not None and late.take_first(mod) and not late.take_first(mod)
        agg_c, wsum_c, pagg = late.aggregate(mod, ref, off, attn, cam, l2i, 900, 1600, coarse=True)        # what the fused loop asks for
        w_v, b_v = mod.value_proj.weight, mod.value_proj.bias
        torch.testing.assert_close(ops.value_proj_heads_fwd(agg_c, wsum_c, w_v, b_v) + pagg,
                                   ops.value_proj_heads_fwd(want_agg, want_wsum, w_v, b_v), rtol=RTOL, atol=ATOL)
        got_agg, got_wsum = late.aggregate(mod, ref, off, attn, cam, l2i, 900, 1600)                     # ... and an all-raw consumer
        assert not late.partial
        late.finish()
    torch.cuda.synchronize()
    assert torch.equal(got_agg, want_agg) and torch.equal(got_wsum, want_wsum)
