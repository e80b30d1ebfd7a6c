"""Conditions on the rows of the memory-contract tests (memory_contract_cases.py), checked on the fp64 references alone: a ReLU row
whose reference is almost all zeros, or all positive, proves little (the rule of test_resnet_cpu.py), and a family without an exact
tile and a tile plus one pixel misses the two sizes an off-by-one in a tile count or a guard shows at."""
import pytest
import torch

import memory_contract_cases as C


def test_every_relu_row_exercises_its_relu():
    """At least a fifth of the reference's outputs at exactly 0 and at least a fifth positive - the (1, 1) maps included, which have
    only 2 x Cout outputs."""
    seen = 0
    for name, ref in C.relu_references():
        zeros, positive = float((ref == 0).double().mean()), float((ref > 0).double().mean())
        assert bool(torch.isfinite(ref).all()) and zeros + positive == 1.0, name
        assert zeros >= 0.2 and positive >= 0.2, f'{name}: {zeros:.2f} of the outputs are 0, {positive:.2f} positive ({ref.numel()} outputs)'
        seen += 1
    assert seen >= 50                                                              # (the generator did not run dry)


def test_the_rows_without_a_relu_let_negative_outputs_through():
    for r in C.RESNET_ROWS:
        if not r[5]:
            ref = C.resnet_case(*r)[5]
            assert float((ref < 0).double().mean()) >= 0.2, C.resnet_id(r)


@pytest.mark.parametrize('family', sorted(C.TILINGS))
def test_every_family_has_an_exact_tile_and_a_tile_plus_one(family):
    tile, sizes = C.TILINGS[family]
    exact, plus_one = C.has_exact_and_plus_one(tile, sizes)
    assert exact and plus_one, (family, tile, sorted(set(sizes)))
    assert (1, 1) in sizes or family in ('dense', 'dcn_wgrad')                     # the one-pixel map (dense: M = 1)
    if family == 'dense':
        assert 1 in C.DENSE_M


def test_the_flag_combinations_of_the_resnet_rows():
    """Both kernels at both strides with and without the identity and the ReLU."""
    for taps in (1, 9):
        for stride in (1, 2):
            flags = {(r[4], r[5]) for r in C.RESNET_ROWS if r[0] == taps and r[3] == stride}
            assert flags == {(False, False), (False, True), (True, False), (True, True)}, (taps, stride)


def test_the_crafted_planes_reach_the_border_and_beyond():
    used = {p for r in C.DCN_ROWS for p in r[5]}
    assert {'at_minus_1', 'at_h_minus_1', 'at_h_and_w', 'corner_tl', 'corner_br'} <= used
    for stride in (1, 2):
        assert {p for r in C.DCN_ROWS if r[2] == stride for p in r[5]} >= {'at_minus_1', 'at_h_minus_1', 'at_h_and_w'}


def test_the_gate_rows_hold_all_three_branches():
    for r in C.VOV_ESE_ROWS:
        gate = C.vov_ese_case(*r)['gate']
        assert (gate == 0).any() and (gate == 1).any() and ((gate > 0) & (gate < 1)).any(), r
