"""gd4d_pyramid_slice_planar_fwd against a torch permute / reshape of the same input, bit for bit: fp32 and bf16 output, 2 and 3
camera rows, levels whose H W is a multiple of the 64-pixel tile and levels with an odd H W, a level smaller than one tile and one
of two pixels, a base offset by 4 bytes (no 16-byte alignment of the input is assumed), and every grid the host code can choose (one
workgroup per tile; persistent with fewer workgroups than tiles and with one per tile).  GPU only."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
LEVEL_LISTS = (((16, 16), (8, 8)), ((13, 21), (5, 7)), ((1, 2),), ((4, 6), (2, 2)), ((40, 30), (16, 16)))
GRIDS = (0, 8, 1 << 20)                       # max_cus: plain; persistent, 8 workgroups stride over the tiles; persistent, one per tile

_CASES = {}


def _case(levels, rows):
    """The input levels and the expected (8, R, S, 32) fp32 planes: made once, left unchanged."""
    key = (levels, rows)
    if key not in _CASES:
        g = torch.Generator().manual_seed(17 * rows + len(levels) + levels[0][0])
        feats = [torch.randn(1, rows, 256, h, w, generator=g).to(DEV) for h, w in levels]
        flat = torch.cat([f.reshape(rows, 256, -1).permute(0, 2, 1) for f in feats], dim=1)          # (R, S, 256)
        want = flat.reshape(rows, flat.shape[1], 8, 32).permute(2, 0, 1, 3).contiguous()
        _CASES[key] = (feats, want)
    return _CASES[key]


def _copy(feats, dtype, max_cus):
    from graph_detr4d_amd import ops
    rows, s = feats[0].reshape(-1, *feats[0].shape[-3:]).shape[0], sum(f.shape[-2] * f.shape[-1] for f in feats)
    out = torch.full((8, rows, s, 32), float('nan'), device=DEV, dtype=dtype)                        # the copy writes every element
    got, hw = ops.pyramid_slice_planar_fwd(feats, out=out, max_cus=max_cus)
    torch.cuda.synchronize()
    assert got is out and hw == [tuple(f.shape[-2:]) for f in feats]
    return out


@pytest.mark.parametrize('rows', (2, 3))
@pytest.mark.parametrize('levels', LEVEL_LISTS)
def test_copy_equals_permute(levels, rows):
    feats, want = _case(levels, rows)
    for dtype in (torch.float32, torch.bfloat16):
        for max_cus in GRIDS:
            got = _copy(feats, dtype, max_cus)
            assert torch.equal(got, want.to(dtype)), (levels, rows, dtype, max_cus)


@pytest.mark.parametrize('max_cus', GRIDS)
def test_base_offset_by_four_bytes(max_cus):
    """Level 0's base is 4 bytes past a 16-byte boundary, level 1's is aligned."""
    levels, rows = ((16, 16), (8, 8)), 3
    feats, want = _case(levels, rows)
    store = torch.empty(feats[0].numel() + 1, device=DEV)
    assert store.data_ptr() % 16 == 0
    shifted = store[1:].view(feats[0].shape)
    shifted.copy_(feats[0])
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous() and feats[1].data_ptr() % 16 == 0
    for dtype in (torch.float32, torch.bfloat16):
        assert torch.equal(_copy([shifted, feats[1]], dtype, max_cus), want.to(dtype))
