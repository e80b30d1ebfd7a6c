"""The bytes of the convolution kernels' weight images against a packer written here from the format's description
(csrc/gd4d_conv_common.h), not from the kernel.  GPU only; exact equality.

The format.  The weight w (Cout, Cin, taps) is viewed as A[m][k][tap] - m = Cout, k = Cin, or transposed (m = Cin, k = Cout) with an
optional tap flip taps - 1 - tap - and M is padded with zeros to m_pad, a multiple of the row block MB.  The image is
[..][plane hi, lo][k-group of 8 (KC / 8)][MB rows][8 x bf16], the outer index [row block][chunk of KC][tap] or [tap][row block][chunk].
hi = bf16(w) to nearest even, lo = bf16(w - hi).

Weights: seeded normal values with planted 0.0 and -0.0, values already exact in bf16, round-to-even ties (low 16 bits 0x8000 under an
even and an odd upper half), 1e30 and 1e-30.  No NaN or inf and no nonzero |v| below 1e-30: every lo is then a normal fp32 (or zero),
where a software round-to-nearest-even, the hardware convert and torch's agree.
Shapes: the smallest that reach every branch - one and several chunks, a ragged last row block (zeros beyond the real rows), two and
three row blocks, every (Mpad, KC) geometry of the DCN image padded and unpadded."""
import functools

import pytest
import torch

from graph_detr4d_amd import ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _planted():
    ties = torch.tensor([0x3F808000, 0x3F818000, 0x3F808000 - (1 << 31), 0x3F818000 - (1 << 31)], dtype=torch.int32).view(torch.float32)
    exact = torch.tensor([1.0, -2.5, 0.15625, 3.0e-5]).to(torch.bfloat16).float()
    return torch.cat([torch.tensor([0.0, -0.0]), exact, ties, torch.tensor([1e30, -1e30, 1e-30, -1e-30])])


@functools.lru_cache(maxsize=None)
def _weight(*shape):
    w = torch.randn(*shape, generator=torch.Generator().manual_seed(sum(shape))) * 0.05
    flat, p = w.view(-1), _planted()
    flat[:p.numel()] = p                                                      # one k-group of row 0 and the next ...
    flat[(torch.arange(p.numel()) * 4099 + 17) % flat.numel()] = p            # ... and scattered over rows, chunks and taps
    assert torch.isfinite(w).all() and not ((w != 0) & (w.abs() < 1e-30)).any()
    return w


def _reference(w, mb, kc, m_pad, tap_outer=False, transposed=False, flip=False):
    """uint8 image of w (Cout, Cin, taps), from the description above."""
    a = w.permute(1, 0, 2) if transposed else w
    if flip:
        a = a.flip(2)
    m, k, taps = a.shape
    assert m_pad % mb == 0 and m_pad >= m and k % kc == 0 and kc % 8 == 0
    a = torch.cat([a, torch.zeros(m_pad - m, k, taps)]).contiguous()
    hi = a.to(torch.bfloat16)
    lo = (a - hi.float()).to(torch.bfloat16)
    x = torch.stack([hi, lo]).view(2, m_pad // mb, mb, k // kc, kc // 8, 8, taps)     # plane, block, row, chunk, k-group, j, tap
    x = x.permute(6, 1, 3, 0, 4, 2, 5) if tap_outer else x.permute(1, 3, 6, 0, 4, 2, 5)
    return x.contiguous().view(torch.uint8).flatten()


def _check(image, want):
    got = image.cpu()
    assert got.dtype == torch.uint8 and got.numel() == want.numel(), (got.numel(), want.numel())
    bad = (got != want).nonzero().flatten()
    assert bad.numel() == 0, f'{bad.numel()} bytes differ, the first at {int(bad[0])} (16-byte item {int(bad[0]) // 16})'


@pytest.mark.parametrize('transposed', [False, True])
def test_depth_net_image(transposed):
    w = _weight(256, 256, 3, 3)
    image = (ops.depth_net_image_t if transposed else ops.depth_net_image)(w.to(DEV))
    _check(image, _reference(w.view(256, 256, 9), 256, 32, 256, transposed=transposed, flip=transposed))


@pytest.mark.parametrize('cin', [32, 96])
def test_fpn_lateral_image(cin):
    w = _weight(256, cin, 1, 1)
    _check(ops.fpn_lateral_image(w.to(DEV)), _reference(w.view(256, cin, 1), 256, 32, 256))


@pytest.mark.parametrize('cin', [96, 288])
def test_fpn_lateral_image_t(cin):
    w = _weight(256, cin, 1, 1)
    _check(ops.fpn_lateral_image_t(w.to(DEV)), _reference(w.view(256, cin, 1), 256, 32, (cin + 255) // 256 * 256, transposed=True))


@pytest.mark.parametrize('cout,cin', [(32, 32), (96, 64)])
def test_conv3x3_image(cout, cin):
    w = _weight(cout, cin, 3, 3)
    _check(ops.conv3x3_image(w.to(DEV)), _reference(w.view(cout, cin, 9), 32, 32, cout))


def test_osa_concat_image():
    w = _weight(64, 96)
    _check(ops.osa_concat_image(w.to(DEV)), _reference(w.view(64, 96, 1), 32, 32, 64))


@pytest.mark.parametrize('cout,cin,mpad,kc', [(27, 64, 32, 16), (64, 64, 256, 32), (256, 64, 256, 32), (320, 64, 512, 16)])
def test_dcn_weight_image(cout, cin, mpad, kc):
    w = _weight(cout, cin, 3, 3)
    _check(ops.dcn_weight_image(w.to(DEV)), _reference(w.view(cout, cin, 9), mpad, kc, mpad, tap_outer=True))


@pytest.mark.parametrize('cout,cin', [(64, 64), (128, 192)])
def test_dcn_weight_image_t(cout, cin):
    w = _weight(cout, cin, 3, 3)
    _check(ops.dcn_weight_image_t(w.to(DEV)), _reference(w.view(cout, cin, 9), 32, cout, cin, tap_outer=True, transposed=True))
