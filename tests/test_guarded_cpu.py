"""guarded.py on the CPU, torch ops standing in for a kernel: a write one element before or after the view flips intact(), a write
inside does not, an element left unwritten stays NaN and is counted, the views keep the 16-byte alignment the entry points demand
for every shape of the memory-contract tables, and the channels-last view has the strides ops._is_cl expects."""
import math

import pytest
import torch

import memory_contract_cases as C
from guarded import PAD, SENTINEL, default_fill, embedded, guarded


def _storage(view):
    """The whole buffer a guarded / embedded view lies in, as a flat tensor."""
    return torch.empty(0, dtype=view.dtype).set_(view.untyped_storage())


def _table_shapes():
    """Every map shape the case tables produce (inputs and outputs), and the small vectors that go with them."""
    shapes = {(256,), (27,), (C.N, 256), (3 + C.N, 256)}
    for t, cin, cout, s, _, _, h, w in C.RESNET_ROWS:
        shapes |= {(C.N, cin, h, w), (C.N, cout, *C.out_hw(h, w, s))}
    for cin, cout, s, h, w in C.VOV_CONV_ROWS:
        shapes |= {(C.N, cin, h, w), (C.N, cout, *C.out_hw(h, w, s)), (cout, cin, 3, 3)}
    for chans, cout, h, w in C.VOV_OSA_ROWS:
        shapes |= {(C.N, c, h, w) for c in chans + (cout,)} | {(C.N, (h * w + 127) // 128, cout), (cout, sum(chans), 1, 1)}
    for cin, h, w, _, _ in C.FPN_LATERAL_ROWS:
        shapes |= {(C.N, cin, h, w), (C.N, 256, h, w), (C.N, 256, (h + 1) // 2, (w + 1) // 2), (256, cin, 1, 1)}
    for levels in [r[0] for r in C.FPN_CONV_ROWS] + [r[0] for r in C.DEPTH_ROWS]:
        shapes |= {(C.N, 256, h, w) for h, w in levels}
    for cin, cout, s, h, w, _ in C.DCN_ROWS + C.DCN_WGRAD_ROWS:
        ho, wo = C.out_hw(h, w, s)
        shapes |= {(C.N, cin, h, w), (C.N, cout, ho, wo), (C.N, 27, ho, wo), (cout, cin, 3, 3), (27, cin, 3, 3)}
    for m in C.DENSE_M:
        shapes |= {(m, k) for k, _ in C.LINEAR_KN} | {(m, n) for _, n in C.LINEAR_KN} | {(m, 8, 256), (m, 8)}
    return sorted(shapes)


def test_a_write_just_outside_the_view_flips_intact():
    for where in ('before', 'after'):
        view, intact = guarded((2, 3, 5))
        assert intact()
        big = _storage(view)
        assert big.numel() == 30 + 2 * PAD
        big[PAD - 1 if where == 'before' else PAD + 30] = 1.0
        assert not intact(), where
    # ... and so does one at either far end of the pads, and a NaN of another payload (the comparison is on the bits)
    for index in (0, -1):
        view, intact = guarded((7,))
        _storage(view)[index] = 0.0
        assert not intact()
    view, intact = guarded((7,))
    _storage(view).view(torch.int32)[PAD - 1] ^= 1
    assert math.isnan(float(_storage(view)[PAD - 1])) and not intact()


def test_writes_inside_the_view_leave_the_guards_alone():
    view, intact = guarded((2, 3, 5))
    assert bool(torch.isnan(view).all()) and intact.unwritten() == 30           # pre-filled
    view.copy_(torch.arange(30.).view(2, 3, 5))
    assert intact() and intact.unwritten() == 0
    assert torch.equal(_storage(view)[PAD:PAD + 30], torch.arange(30.))         # first and last element sit against the pads


def test_an_unwritten_element_stays_nan_and_is_counted():
    view, intact = guarded((4, 6))
    view[:, :5] = 1.0                                                            # a "kernel" that forgets the last column
    assert intact() and intact.unwritten() == 4
    assert torch.equal(torch.isnan(view), torch.tensor([[False] * 5 + [True]] * 4))
    assert not bool(torch.isfinite(view).all())


def test_integer_and_byte_buffers_use_the_sentinel_pattern():
    for dtype in (torch.uint8, torch.int32, torch.int64):
        view, intact = guarded((5, 3), dtype=dtype)
        assert intact() and intact.unwritten() == 15
        assert bool((view.contiguous().view(torch.uint8) == SENTINEL).all())
        view.zero_()
        assert intact() and intact.unwritten() == 0
        _storage(view)[PAD + 15] = 0
        assert not intact()
    assert default_fill(torch.uint8) == SENTINEL and math.isnan(default_fill(torch.float32))
    view, intact = guarded((3,), fill=777.0)                                     # test_optim_tails_gpu's sentinel
    assert bool((view == 777.0).all()) and intact()


def test_pad_must_keep_the_alignment():
    for pad in (0, 2, 63):
        with pytest.raises(ValueError):
            guarded((3,), pad=pad)
    view, intact = guarded((3,), pad=4)
    assert view.data_ptr() % 16 == 0 and intact()


@pytest.mark.parametrize('channels_last', [False, True])
def test_alignment_holds_for_every_shape_of_the_tables(channels_last):
    shapes = [s for s in _table_shapes() if len(s) == 4 or not channels_last]
    assert len(shapes) > 50
    for shape in shapes:
        view, intact = guarded(shape, channels_last=channels_last)
        assert view.data_ptr() % 16 == 0 and tuple(view.shape) == shape and intact(), shape
        src = torch.randn(shape)
        if channels_last:
            src = src.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        inside = embedded(src)
        assert inside.data_ptr() % 16 == 0 and torch.equal(inside, src) and inside.stride() == src.stride(), shape
        big = _storage(inside)
        assert bool(torch.isnan(big[:PAD]).all()) and bool(torch.isnan(big[PAD + src.numel():]).all())


def test_channels_last_view_has_the_strides_the_neck_expects():
    from graph_detr4d_amd import ops
    for shape in ((2, 256, 1, 1), (2, 256, 7, 9), (2, 256, 17, 16)):
        view, intact = guarded(shape, channels_last=True)
        made = ops.fpn_empty(shape[0], shape[2], shape[3], 'cpu', channels_last=True)
        assert tuple(view.shape) == tuple(made.shape) == shape and view.stride() == made.stride()
        assert ops._is_cl(view) and view.permute(0, 2, 3, 1).is_contiguous()
        view.copy_(torch.randn(shape))                                           # a strided write stays inside
        assert intact() and intact.unwritten() == 0
        plain, _ = guarded(shape)
        assert plain.is_contiguous() and (shape[2] * shape[3] == 1 or not ops._is_cl(plain))


def test_embedded_keeps_integer_tensors_and_refuses_other_layouts():
    t = torch.arange(12, dtype=torch.int32).view(3, 4)
    e = embedded(t)
    assert torch.equal(e, t) and bool((_storage(e)[:PAD].view(torch.uint8) == SENTINEL).all())
    with pytest.raises(ValueError):
        embedded(torch.randn(4, 6).t())
