"""The marshalling helpers of ops.py (its module docstring states their contract), as far as they can be held to it without a GPU."""
import ctypes
import struct

import pytest
import torch

from graph_detr4d_amd import _lib, ops


def test_dtype_constants():
    assert (ops.F32, ops.I32, ops.U8) == (torch.float32, torch.int32, torch.uint8)


@pytest.mark.parametrize('seq', [[(2, 3), (1, 2)], [torch.empty(1, 2, 3), torch.empty(1, 1, 2)], [torch.empty(4, 7, 2, 3), (1, 2)]])
def test_levels_from_pairs_and_from_tensors(seq):
    table = ops._levels(seq)
    assert isinstance(table, ctypes.Array) and table._type_ is ctypes.c_int32 and len(table) == 4
    assert bytes(table) == struct.pack('<4i', 2, 3, 1, 2)


def test_range6_is_six_doubles():
    rng = [-51.2, -51.2, -5, 51.2, 51.2, 3]
    table = ops._range6(rng)
    assert isinstance(table, ctypes.Array) and table._type_ is ctypes.c_double and len(table) == 6
    assert bytes(table) == struct.pack('<6d', *rng)
    with pytest.raises((IndexError, ValueError, TypeError)):
        ops._range6(rng + [0.0])


def test_out_makes_a_tensor_or_refuses_the_shape_before_the_device():
    made = ops._out(None, (2, 3), 'cpu', 'w: out')
    assert tuple(made.shape) == (2, 3) and made.dtype == torch.float32
    assert ops._out(None, (2,), 'cpu', 'w: out', ops.I32).dtype == torch.int32
    mine = torch.empty(2, 3)
    assert ops._out(mine, (2, 3), 'cpu', 'w: out') is mine
    with pytest.raises(ValueError, match=r'w: out must be \(2, 3\)'):               # a CPU tensor: the shape is what is refused
        ops._out(torch.empty(3, 2), (2, 3), 'cpu', 'w: out')


def test_opt_and_order_hand_none_through():
    assert ops._opt(None, 'bias') is None and ops._opt(None, 'mask', None) is None
    assert ops._order_ptr(None, 7) is None
    assert bytes(ops._ptrs([None, None], 'biases', optional=True)) == bytes(16)


def test_a_cpu_tensor_is_refused_in_the_arguments_name():
    t = torch.zeros(4)
    with pytest.raises(_lib.Gd4dError, match='x must live on the GPU'):
        ops._dev(t, 'x', torch.float32)
    with pytest.raises(_lib.Gd4dError, match='bias must live on the GPU'):
        ops._opt(t, 'bias')
    with pytest.raises(_lib.Gd4dError, match=r'feats\[1\] must live on the GPU'):
        ops._ptrs([None, t], 'feats', optional=True)
    with pytest.raises(_lib.Gd4dError, match=r'feats\[0\] must live on the GPU'):
        ops._ptrs([t], 'feats')
    with pytest.raises(AttributeError):                                             # a None entry is a null only where the site says so
        ops._ptrs([None], 'feats')


def test_call_looks_the_entry_up_at_call_time_and_checks_in_its_name(monkeypatch):
    """_call(entry, *args): the entry of whatever _lib.load() hands out now (a recording's stand-in), args then the stream; a
    non-zero code raises in the entry's name."""
    handle = ctypes.c_void_p(1234)
    monkeypatch.setattr(ops, '_stream', lambda: handle)
    seen, real = [], _lib.load()

    class StandIn:
        def __getattr__(self, name):                     # (gd4d_error_string and the like: the library's own)
            return getattr(real, name)

        def gd4d_layernorm_fwd(self, *args):
            seen.append(args)
            return 0

        def gd4d_linear_fwd(self, *args):
            return -1

    with _lib.recording(StandIn()):
        assert ops._call('gd4d_layernorm_fwd', 1, 2.5, None) is None
        assert seen == [(1, 2.5, None, handle)]
        with pytest.raises(_lib.Gd4dError, match='gd4d_linear_fwd failed'):
            ops._call('gd4d_linear_fwd')
        with pytest.raises(AttributeError):
            ops._call('gd4d_no_such_entry')


def test_asked_results():
    assert ops._asked(('out',), None, None) == 'out'
    assert ops._asked(('out',), 'mask', None) == ('out', 'mask')
    assert ops._asked(('out',), None, 'uv') == ('out', 'uv')
    assert ops._asked(('out',), None, None, bare=False) == ('out',)
    assert ops._asked(('agg', 'wsum'), 'mask', 'uv', bare=False) == ('agg', 'wsum', 'mask', 'uv')
