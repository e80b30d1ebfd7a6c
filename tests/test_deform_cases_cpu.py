"""tests/deform_cases.py without a GPU: every case meets the conditions its tests rely on, the fp64 arbiter (the oracle's grid_sample
form) equals the oracle's explicit-gather form and the raw association restated for the raw-pyramid route, and the fp32 host errors
that the GPU tests derive their bounds from are finite, non-zero and printed."""
import math

import pytest
import torch

import deform_cases as D
import detr3d_ref as R

F64 = torch.float64
NAMES = list(D.SHAPES)


@pytest.mark.parametrize('name', NAMES)
def test_case_meets_its_conditions(name):
    cs = D.case(name)
    counts = D.check_case(cs)
    print(name, counts)
    assert cs.Q == D.Q_RANDOM + 16 + D.Q_BLOCK and cs.ref.dtype == torch.float32
    assert bool(((cs.ref >= 0) & (cs.ref <= 1)).all())
    assert sum(t.numel() for t in (cs.ref, cs.offsets, cs.attn, cs.cam, cs.grad_out)) * 4 < 400 * 1024


@pytest.mark.parametrize('name', NAMES)
def test_fp64_arbiter_equals_its_explicit_gather_form_and_the_raw_association(name):
    """Three statements of one operation in fp64: grid_sample on the projected value (the arbiter), bilinear_zero_pad's rule on given
    corners (corners=), and the raw pixels gathered first and projected per head afterwards.  1e-12 of the largest entry: a corner
    test of `x0 + 1 <= W` in place of `x0 + 1 <= W - 1` in either restatement moves `out` by far more on the band and corner queries."""
    cs = D.case(name)
    want, _ = D.reference(name)
    with torch.no_grad():
        lv = {k: ([f.detach() for f in v] if isinstance(v, list) else v.detach()) for k, v in D.leaves(cs, F64).items()}
        gathered, mask, _ = D.projected(cs, lv, F64, corners=D.cell_corners(cs))
        raw, _, wsum, fine = D.raw_association(cs, lv, F64)
    assert torch.equal(mask, want['mask'])
    scale = float(want['out'].abs().max())
    assert float((gathered - want['out']).abs().max()) <= 1e-12 * scale
    assert float((raw - want['out']).abs().max()) <= 1e-12 * scale
    assert torch.equal(wsum, want['wsum']) and bool((fine <= wsum + 1e-15).all())
    band = D.of_kind(cs, 'side') + D.of_kind(cs, 'corner')
    assert float(want['out'][:, band].abs().min(-1).values.max()) >= 0 and float(want['out'][:, band].abs().max()) > 1e-3 * scale
    nobody = D.of_kind(cs, 'nobody')
    assert bool((want['out'][:, nobody] == 0).all()) and bool((want['grad_ref'][:, nobody] == 0).all())
    assert bool((want['grad_offsets'][:, nobody] == 0).all()) and bool((want['wsum'][:, nobody] == 0).all())


@pytest.mark.parametrize('name', NAMES)
def test_raw_association_gradients_are_the_arbiters(name):
    """fp64 autograd through the raw association gives the arbiter's gradients: the fp32 budget of the raw route is a budget for the
    same function."""
    cs = D.case(name)
    want, _ = D.reference(name)
    got = D.evaluate(cs, F64, raw=True)
    for key, err in D.figures(cs, got, want).items():
        assert err <= 1e-11, (key, err)


@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('raw', [False, True], ids=['projected', 'raw'])
def test_fp32_host_errors(name, raw):
    """The figures the GPU tests multiply by 4.  An honest fp32 evaluation stays within a few hundred ulps of fp64; anything near 1e-4
    would mean that a visibility bit or a bilinear cell differs between the precisions, i.e. that the margins do not do their work."""
    _, host = D.reference(name, raw=raw)
    _, block = D.reference(name, raw=raw, block_only=True)
    for key, err in {**host, **block}.items():
        print(f'{name:>7} {"raw" if raw else "projected":<9} {key:<18} fp32 host {err:.2e}   bound {D.FACTOR * err:.2e}')
        assert math.isfinite(err) and 0 < err < 1e-4, key
    assert ('grad_value' in host) != raw and len([k for k in host if k.startswith('grad_feats[')]) == len(D.SHAPES[name][3])


@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('what', ['value', 'feats'])
def test_bf16_references(name, what):
    """The bf16-storage references differ from the fp32 ones by bf16's rounding, and their own fp32 budget stays an fp32 budget."""
    out, host = D.reference_bf16(name, what)
    want, _ = D.reference(name)
    assert 1e-4 < R.rel_err(out, want['out']) < 2e-2 and 0 < host['out'] < 1e-4


def test_block_meets_on_the_same_pixels():
    """The block's queries put 32 x heads x 4 records on the block cell's pixels: their gradient is far above the map's median."""
    for name in NAMES:
        cs = D.case(name)
        want, _ = D.reference(name)
        g = want['grad_feats'][-1]
        assert float(D.block_grad(cs, want['grad_feats']).abs().max()) > 4 * float(g.abs().median()) and len(D.block_pixels(cs)) >= 1
        assert R.rel_err(want['grad_feats2'][-1], g) > 0.1                          # the second layer's gradient is another one
