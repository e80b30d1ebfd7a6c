"""tests/detr3d_ref.py and tests/detr3d_cases.py without a GPU: the restatement reproduces what was recorded from the reference project
(the four detr3d fixtures), its corner-wise sample is F.grid_sample, every case meets the conditions its tests rely on, and the fp32
host errors that the GPU tests derive their bounds from are reproduced and printed."""
import pytest
import torch
import torch.nn.functional as F

import detr3d_cases as D
import detr3d_ref as R
from golden_io import Golden

F64 = torch.float64
# The fixtures hold the reference's fp32 results.  fp32 carries 6e-8; the projection's division and the scaling to pixels (up to 28)
# make that about 2e-6 of a pixel in dx, dy, and a sample sums four products of entries up to the map's largest: 2e-5 of the largest
# entry is ten times that.
FIXTURE_BOUND = 2e-5


def _fixture(name):
    g = Golden(name)
    m = g.meta
    feats = [f.to(F64) for f in g.feats()]
    b, n = feats[0].shape[:2]
    ref = g.t('reference_points').to(F64)
    l2i = torch.from_numpy(g.arrays['lidar2img']).to(F64).unsqueeze(0).expand(b, -1, -1, -1)
    return g, m, feats, ref, l2i, b, n, ref.shape[1]


@pytest.mark.parametrize('name', ['detr3d_n6', 'detr3d_n12_b2'])
def test_detr3d_reproduces_the_fixture(name):
    g, m, feats, ref, l2i, b, n, q = _fixture(name)
    out, mask, sampled = R.detr3d(feats, ref, g.t('attn_logits').to(F64).view(b, q, n, 1, len(feats)), l2i, m['pc_range'], *m['img_shape'][:2])
    assert torch.equal(mask.permute(0, 2, 1), g.t('fs_mask').view(b, q, n).bool())
    e_s, e_o = R.rel_err(sampled, g.t('fs_sampled').to(F64)), R.rel_err(out, g.t('agg').permute(1, 0, 2).to(F64))
    print(f'{name}: fs_sampled {e_s:.2e}, agg {e_o:.2e}')
    assert sampled.shape == g.t('fs_sampled').shape and e_s <= FIXTURE_BOUND and e_o <= FIXTURE_BOUND


@pytest.mark.parametrize('name', ['detr3d_v2_n6', 'detr3d_v2_n12'])
def test_detr3d_v2_reproduces_the_fixture(name):
    g, m, feats, ref, l2i, b, n, q = _fixture(name)
    nl = len(feats)
    out, mask = R.detr3d_v2(feats, ref, g.t('attn_logits').to(F64).view(b, q, n, 8, nl * nl), g.t('offsets').to(F64).view(b, q, n, 8, nl, nl, 2),
                            l2i, m['pc_range'], *m['img_shape'][:2], 8)
    assert torch.equal(mask.permute(0, 2, 1), g.t('mask').view(b, q, n).bool())
    e_o = R.rel_err(out, g.t('agg').permute(1, 0, 2).to(F64))
    print(f'{name}: agg {e_o:.2e}')
    assert e_o <= FIXTURE_BOUND


@pytest.mark.parametrize('name', list(D.SHAPES))
def test_cornerwise_sample_is_grid_sample(name):
    """fp64, the random points of the case on every camera and level that puts them within a few maps of the image (the zero padding
    included); beyond that F.grid_sample converts to integers, which is what the corner-wise form exists to avoid."""
    cs = D.case(name)
    rand = [i for i, kind in enumerate(cs.kinds) if kind == 'random']
    grid, _, _ = R.project(cs.ref[:, rand].to(F64), cs.lidar2img.to(F64), D.PC_RANGE, D.IMG_H, D.IMG_W)
    grid = grid.reshape(cs.B * cs.N, len(rand), 2)
    near = grid.abs().amax(-1) < 4
    assert int(near.sum()) >= len(rand) and bool((near & (grid.abs().amax(-1) > 1)).any())
    for f in cs.feats:
        maps = f.to(F64).reshape(cs.B * cs.N, cs.C, *f.shape[-2:])
        ours = R.sample(maps, grid[..., 0], grid[..., 1])
        aten = F.grid_sample(maps, grid.clamp(-4, 4)[:, :, None, :], mode='bilinear', padding_mode='zeros', align_corners=False)[..., 0]
        sel = near[:, None, :].expand_as(ours)
        assert float((ours - aten)[sel].abs().max()) <= 1e-12 * float(maps.abs().max())


@pytest.mark.parametrize('name', list(D.SHAPES))
def test_case_meets_its_conditions(name):
    cs = D.case(name)
    counts = D.check_case(cs)
    print(name, counts)
    assert cs.Q == D.Q_RANDOM + 14 + D.Q_BLOCK and cs.ref.dtype == torch.float32
    assert max(f.numel() for f in cs.feats) <= 6 * 256 * 16 * 28              # the fixtures' finest map: nothing here is larger


@pytest.mark.parametrize('name,variant', D.VARIANTS)
def test_fp32_host_errors(name, variant):
    """The figures the GPU tests multiply by 4.  An honest fp32 evaluation stays within a few hundred ulps of fp64; anything near 1e-4
    would mean that a visibility bit or a bilinear cell differs between the precisions, i.e. that the margins do not do their work."""
    _, host = D.reference(name, variant)
    _, block = D.reference(name, variant, block_only=True)
    for key, err in {**host, **block}.items():
        print(f'{name:>7} {variant} {key:<16} fp32 host {err:.2e}   bound {D.FACTOR * err:.2e}')
        assert 0 <= err < 1e-4, key
