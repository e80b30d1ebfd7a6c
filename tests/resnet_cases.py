"""The kernel cases of the ResNet tests and their fp64 references, computed once per process: test_resnet_gpu.py runs the kernels on
them, test_resnet_cpu.py checks on the references alone that every case with the ReLU on has at least a fifth of its outputs at 0."""
import functools

import torch

import resnet_ref as R

N = 2
# (cin, cout, stride, identity, relu, h, w).  13 x 21: two ragged tiles each way (1x1 stride 1: three 128-pixel tiles of the flat image,
# the last ragged); 5 x 7: one ragged tile; 26 x 37 -> 13 x 19 and 5 x 7 -> 3 x 4: the even and odd stride-2 sizes.
CONV1X1_CASES = [(64, 64, 1, False, True, 13, 21), (256, 64, 1, False, True, 13, 21), (64, 256, 1, False, False, 13, 21),
                 (256, 512, 2, False, False, 26, 37), (256, 512, 2, False, False, 5, 7), (1024, 2048, 2, False, False, 5, 7),
                 (512, 2048, 1, True, True, 5, 7), (64, 256, 1, True, True, 13, 21), (2048, 512, 1, False, True, 5, 7)]
CONV3X3_CASES = [(512, 512, 1, False, True, 5, 7), (512, 512, 2, False, True, 5, 7), (256, 512, 2, False, True, 26, 37),
                 (64, 64, 1, True, True, 13, 21), (128, 128, 1, True, True, 5, 7)]


def case_id(c):
    return f'{c[0]}-{c[1]}-s{c[2]}' + ('-id' if c[3] else '') + ('-relu' if c[4] else '') + f'-{c[5]}x{c[6]}'


def rand(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def scale_shift(c, seed):
    """test_vovnet_gpu._scale_shift's choice: a scale around 1.5, a shift of std 0.5 around 0 - half of the pre-activations are negative."""
    return 1.5 + 0.1 * rand(c, seed=seed), rand(c, seed=seed + 1, scale=0.5)


@functools.lru_cache(maxsize=None)
def conv_case(taps, cin, cout, stride, identity, relu, h, w):
    """(x, weight, scale, shift, identity or None, the fp64 reference); the identity has zero mean."""
    k = 3 if taps == 9 else 1
    x = rand(N, cin, h, w, seed=1)
    weight = rand(cout, cin, k, k, seed=2, scale=(taps * cin) ** -0.5)
    scale, shift = scale_shift(cout, 3)
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    ident = rand(N, cout, ho, wo, seed=5) if identity else None
    return x, weight, scale, shift, ident, R.folded_conv_act(x, weight, scale, shift, stride, ident, relu)
