"""The walk of gd4d_cross_attn_agg_items_coarse_fwd in both directions, on the host (gd4d_gather_walk_dir runs the kernel's own walk
function): every (position, phase) exactly once, the projected rows' phase last, workgroup i on the sector of XCD i % 8, the forward
direction the walk gd4d_gather_walk gives; reversed, an XCD meets its slice groups from last to first.  No GPU."""
import ctypes
import os
import re

import pytest

from graph_detr4d_amd import _lib, ops

BQS = (1, 7, 8, 9, 37, 900)
NSS = (1, 2, 4, 8)


def _walk(bq, blk, ns, reverse):
    """[(position, phase)] by workgroup, through the library."""
    lib = _lib.load()
    pos, grp = ctypes.c_int(), ctypes.c_int()
    grid = lib.gd4d_gather_walk_dir(bq, blk, ns, int(reverse), -1, None, None)
    out = []
    for i in range(grid):
        assert lib.gd4d_gather_walk_dir(bq, blk, ns, int(reverse), i, ctypes.byref(pos), ctypes.byref(grp)) == grid
        out.append((pos.value, grp.value))
    return out


@pytest.mark.parametrize('reverse', (False, True))
@pytest.mark.parametrize('ns', NSS)
@pytest.mark.parametrize('bq', BQS)
def test_walk_in_both_directions(bq, ns, reverse):
    per_xcd = (bq + 7) // 8
    phases = 8 // ns + 1
    for blk in sorted({1, 8, per_xcd}):
        walk = _walk(bq, blk, ns, reverse)
        assert len(walk) == 8 * ((per_xcd + blk - 1) // blk) * blk * phases
        seen = {}
        order = {}                                                              # (xcd, position) -> its phases in workgroup order
        for i, (pos, grp) in enumerate(walk):
            if pos < 0:
                assert (pos, grp) == (-1, -1)
                continue
            xcd = i % 8
            assert xcd * per_xcd <= pos < min((xcd + 1) * per_xcd, bq), (bq, blk, ns, i, pos)      # XCD i % 8's sector
            assert 0 <= grp < phases
            assert (pos, grp) not in seen, (bq, blk, ns, i, seen[(pos, grp)])
            seen[(pos, grp)] = i
            order.setdefault((xcd, pos), []).append(grp)
        assert set(seen) == {(p, g) for p in range(bq) for g in range(phases)}                      # every pair exactly once
        groups = list(range(phases - 1))
        want = (groups[::-1] if reverse else groups) + [phases - 1]                                 # the projected rows' phase last
        assert all(o == want for o in order.values()), (bq, blk, ns, reverse)
        if not reverse:
            lib = _lib.load()
            pos, grp = ctypes.c_int(), ctypes.c_int()
            for i in range(0, len(walk), max(1, len(walk) // 97)):                                  # forward = today's sequence
                assert lib.gd4d_gather_walk(bq, blk, ns, i, ctypes.byref(pos), ctypes.byref(grp)) == len(walk)
                assert (pos.value, grp.value) == walk[i]


def test_forward_is_the_walk_without_a_direction_everywhere():
    lib = _lib.load()
    pos, grp = ctypes.c_int(), ctypes.c_int()
    for bq, blk, ns in ((37, 5, 2), (9, 2, 1), (900, 113, 2)):
        walk = _walk(bq, blk, ns, False)
        for i, w in enumerate(walk):
            lib.gd4d_gather_walk(bq, blk, ns, i, ctypes.byref(pos), ctypes.byref(grp))
            assert (pos.value, grp.value) == w
        assert ops.gather_walk(bq, blk, ns, 8) == (len(walk), *walk[8])
        rev = _walk(bq, blk, ns, True)
        assert ops.gather_walk(bq, blk, ns, 8, reverse=True) == (len(walk), *rev[8])
        assert [p for p, _ in rev] == [p for p, _ in walk]                      # a workgroup keeps its position: only the phase turns


def test_bad_arguments_and_outside_the_grid():
    lib = _lib.load()
    pos, grp = ctypes.c_int(5), ctypes.c_int(5)
    for bad in ((0, 1, 1), (8, 0, 1), (8, 1, 3)):
        assert lib.gd4d_gather_walk_dir(*bad, 1, 0, None, None) == -1           # GD4D_EINVAL
    grid = lib.gd4d_gather_walk_dir(37, 5, 4, 1, 0, ctypes.byref(pos), ctypes.byref(grp))
    assert grid == 8 * 5 * 3 and (pos.value, grp.value) == (0, 1)               # reversed: the last slice group first
    for block in (-1, grid):
        lib.gd4d_gather_walk_dir(37, 5, 4, 1, block, ctypes.byref(pos), ctypes.byref(grp))
        assert (pos.value, grp.value) == (-1, -1)


def test_switch_and_the_flag():
    lib = _lib.load()
    get = ops.gather_walk_alternate
    was = get()
    assert was is True                                                          # on by default
    try:
        assert get(False) is True and get() is False
        assert get(True) is False and get() is True
    finally:
        get(was)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'gd4d.h')).read()
    assert re.search(r'#define GD4D_GATHER_REVERSED 0x100\b', hdr) and _lib.GATHER_REVERSED == 0x100
    assert _lib.GATHER_REVERSED & (_lib.F32 | _lib.BF16 | _lib.F16) == 0        # the bit rides beside every value type
    assert lib.gd4d_abi_version() == 56                                         # additive exports
