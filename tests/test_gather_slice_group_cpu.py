"""The walk of gd4d_cross_attn_agg_items_coarse_fwd with NS slices per fine workgroup, on the host (gd4d_gather_walk runs the
kernel's own walk function): every (position, slice group) exactly once, the projected rows' phase once per position, nothing else,
and workgroup i on the sector of XCD i % 8.  No GPU."""
import ctypes

import pytest

from graph_detr4d_amd import _lib, ops

BQS = (1, 7, 8, 9, 37, 900)
NSS = (1, 2, 4, 8)


def _blks(bq):
    per_xcd = (bq + 7) // 8
    return sorted({1, 8, per_xcd})


@pytest.mark.parametrize('ns', NSS)
@pytest.mark.parametrize('bq', BQS)
def test_walk_covers_every_group_once(bq, ns):
    lib = _lib.load()
    per_xcd = (bq + 7) // 8
    phases = 8 // ns + 1
    pos, grp = ctypes.c_int(), ctypes.c_int()
    for blk in _blks(bq):
        grid = lib.gd4d_gather_walk(bq, blk, ns, -1, None, None)
        assert grid == 8 * ((per_xcd + blk - 1) // blk) * blk * phases, (bq, blk, ns, grid)
        seen = {}
        for i in range(grid):
            assert lib.gd4d_gather_walk(bq, blk, ns, i, ctypes.byref(pos), ctypes.byref(grp)) == grid
            if pos.value < 0:
                assert pos.value == -1 and grp.value == -1                      # a workgroup past the sector's end: nothing to do
                continue
            xcd = i % 8
            assert xcd * per_xcd <= pos.value < min((xcd + 1) * per_xcd, bq), (bq, blk, ns, i, pos.value)
            assert 0 <= grp.value < phases
            key = (pos.value, grp.value)
            assert key not in seen, (bq, blk, ns, i, seen[key], key)
            seen[key] = i
        # every slice group of every position, and the projected rows' phase (group 8 / ns) once per position - nothing else
        assert set(seen) == {(p, g) for p in range(bq) for g in range(phases)}, (bq, blk, ns)


def test_walk_outside_the_grid_and_bad_arguments():
    lib = _lib.load()
    pos, grp = ctypes.c_int(5), ctypes.c_int(5)
    grid = lib.gd4d_gather_walk(37, 5, 4, 0, ctypes.byref(pos), ctypes.byref(grp))
    assert grid == 8 * 5 * 3 and (pos.value, grp.value) == (0, 0)
    for block in (-1, grid, grid + 7):
        assert lib.gd4d_gather_walk(37, 5, 4, block, ctypes.byref(pos), ctypes.byref(grp)) == grid
        assert (pos.value, grp.value) == (-1, -1)
    for bad in ((0, 1, 1), (8, 0, 1), (8, 1, 3), (8, 1, 0), (8, 1, 16)):
        assert lib.gd4d_gather_walk(*bad, 0, None, None) == -1                  # GD4D_EINVAL
    assert ops.gather_walk(9, 2, 8, 0) == (8 * 2 * 2, 0, 0)
    with pytest.raises(_lib.Gd4dError):
        ops.gather_walk(9, 2, 3)


def test_ns1_is_the_walk_of_nine_phases():
    """NS = 1: slice-major within a block of queries, the ninth phase the projected rows - what the launch walked before the setting
    existed."""
    bq, blk = 37, 5                                                              # per_xcd = 5
    for i in (0, 8, 8 * 4, 8 * 5, 8 * 5 * 8, 8 * 5 * 8 + 8 * 4 + 3):
        xcd, j = i % 8, i // 8
        sl, qi = j // blk, j % blk
        grid, pos, grp = ops.gather_walk(bq, blk, 1, i)
        want = (xcd * 5 + qi, sl) if xcd * 5 + qi < bq else (-1, -1)
        assert grid == 8 * 5 * 9 and (pos, grp) == want


def test_setter_and_getter():
    lib = _lib.load()
    was = ops.gather_slice_group()
    assert was in NSS and lib.gd4d_gather_slice_group_get() == was
    try:
        for ns in NSS:
            before = ops.gather_slice_group()
            assert ops.gather_slice_group(ns) == before and ops.gather_slice_group() == ns
        for bad in (0, 3, 5, 16, -1):
            assert lib.gd4d_gather_slice_group(bad) == 8 and lib.gd4d_gather_slice_group_get() == 8    # changes nothing
            with pytest.raises(ValueError):
                ops.gather_slice_group(bad)
    finally:
        ops.gather_slice_group(was)
    assert ops.gather_slice_group() == was
    assert lib.gd4d_abi_version() == 56                                          # additive exports
