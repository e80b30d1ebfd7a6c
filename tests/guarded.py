"""Guarded buffers for the memory-contract tests: an output inside a larger buffer whose surroundings hold a known fill, and an input
copied into a buffer whose surroundings are NaN.  A kernel that stores past an output flips the guard; one that reads past an input
and multiplies by zero brings a NaN into its result; an output element it never writes keeps the fill.  One implementation in place
of the private ones of test_vovnet_train_gpu.py (_guarded), test_optim_tails_gpu.py (_Buffers) and the cross-MHA tests.

Floating-point buffers are filled with NaN; integer and byte buffers (images, plans, workspaces) with the byte SENTINEL, since they
have no NaN.  The comparison is on the raw bytes, so a NaN of another payload, or a -0.0 over a 0.0 fill, counts as a write."""
import torch

PAD = 64
SENTINEL = 0xA5                  # the byte every element of an integer / byte guard is made of


def _numel(shape):
    n = 1
    for s in shape:
        n *= int(s)
    return n


def default_fill(dtype):
    """NaN for floating-point types; the element whose every byte is SENTINEL for the others."""
    if dtype.is_floating_point:
        return float('nan')
    return int(torch.full((torch.empty((), dtype=dtype).element_size(),), SENTINEL, dtype=torch.uint8).view(dtype).item())


def _bytes(t):
    return t.contiguous().view(torch.uint8)


def _buffer(shape, pad, dtype, device, fill, channels_last):
    """(big, view): a flat buffer of numel + 2 pad elements of `fill`; the view of `shape` over its middle."""
    shape = tuple(int(s) for s in shape)
    if pad <= 0 or pad % 4:
        raise ValueError(f'pad = {pad}: a positive multiple of 4 keeps the view 16-byte aligned')
    numel = _numel(shape)
    if fill is None:
        fill = default_fill(dtype)
    big = torch.full((numel + 2 * pad,), fill, dtype=dtype, device=device)
    mid = big[pad:pad + numel]
    if channels_last:
        if len(shape) != 4:
            raise ValueError(f'channels_last wants an (N, C, H, W) shape, got {shape}')
        n, c, h, w = shape
        view = mid.view(n, h, w, c).permute(0, 3, 1, 2)                      # ops.fpn_empty's layout: stored (N, H, W, C)
    else:
        view = mid.view(shape)
    if big.element_size() >= 4:                                              # (a byte buffer's 16-byte alignment needs pad % 16 == 0)
        assert big.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 0, 'the view lost the 16-byte alignment the entry points demand'
    assert view.data_ptr() == big.data_ptr() + pad * big.element_size()
    return big, view, numel, fill


def guarded(shape, pad=PAD, dtype=torch.float32, device='cpu', fill=None, channels_last=False):
    """(view, intact): a view of `shape` - contiguous, or the (N, H, W, C)-stored permutation ops.fpn_empty makes - inside one larger
    buffer with `pad` elements of `fill` on each side, itself pre-filled with `fill` (default: NaN, or the SENTINEL bytes for integer
    types).  intact() is True iff both pads still hold the fill bit for bit.  intact.unwritten() counts the view's elements that still
    hold the fill's bits."""
    big, view, numel, fill = _buffer(shape, pad, dtype, device, fill, channels_last)
    want = _bytes(torch.full((pad,), fill, dtype=dtype, device=device))
    one = _bytes(torch.full((1,), fill, dtype=dtype, device=device))

    def intact():
        return bool(torch.equal(_bytes(big[:pad]), want) and torch.equal(_bytes(big[pad + numel:]), want))

    def unwritten():
        mid = _bytes(big[pad:pad + numel]).view(numel, -1)
        return int((mid == one).all(dim=1).sum())
    intact.unwritten = unwritten
    intact.buffer = big
    return view, intact


def embedded(tensor, pad=PAD):
    """A copy of `tensor` (contiguous or channels-last) with the same layout, device and dtype inside a buffer whose other elements are
    NaN (the SENTINEL bytes for integer types): what a kernel picks up when it reads past the tensor's ends."""
    cl = tensor.dim() == 4 and not tensor.is_contiguous() and tensor.permute(0, 2, 3, 1).is_contiguous()
    if not cl and not tensor.is_contiguous():
        raise ValueError('embedded: a contiguous or channels-last tensor expected')
    _, view, _, _ = _buffer(tensor.shape, pad, tensor.dtype, tensor.device, None, cl)
    view.copy_(tensor)
    return view
