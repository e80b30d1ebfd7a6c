"""The kernel cases of the ResNet training tests and their fp64 references (resnet_train_ref.py), computed once per process and left
unchanged: test_resnet_train_gpu.py runs every new entry point of gd4d_resnet_train.hip on them, test_resnet_train_contract_gpu.py runs
the same launches under the memory contract.  N = 2 and the smallest shapes at which a tile count, a parity or a channel block can go
wrong; the data gradients' tile is 8 x 16 output pixels (1x1: 128 pixels of the flat map), the weight gradients' 16 x 16 input pixels
(1x1: 64 output pixels)."""
import functools

import torch

import resnet_train_ref as T

N = 2
KERNEL_TOL = 1e-4               # of a gradient's largest |entry|, per kernel (test_fpn_train_gpu.py)

# 1x1 adjoint: (cin = M, cout = K, h, w, even-pixel add).  1 x 1; exactly 128 pixels; 129 pixels; the even-pixel add at odd and even
# sizes; stage 4's conv3 adjoint K = 2048 -> M = 512 at 4 x 5
PW_DGRAD_CASES = [(64, 32, 1, 1, False), (32, 64, 8, 16, False), (32, 64, 3, 43, False), (64, 32, 9, 11, True), (64, 32, 8, 12, True),
                  (512, 2048, 4, 5, False)]
# 3x3 adjoint: (cin = M, cout = K, stride, H, W of dx, even-pixel add).  Stride 2 at both parities and a tile edge -1, 0, +1, Cout 32 and
# 512, with the even-pixel add (BasicBlock's conv1); stride 1 at ResNet's Cout = 512
C3_DGRAD_CASES = [(64, 32, 2, 1, 1, True), (64, 32, 2, 2, 2, True), (64, 32, 2, 15, 31, True), (64, 32, 2, 16, 32, True),
                  (64, 32, 2, 17, 33, True), (32, 512, 2, 17, 33, True), (32, 512, 2, 2, 2, False), (32, 512, 1, 5, 7, False)]
# weight gradients: (taps, cin, cout, stride, H, W of x).  1x1 stride 2 at (9, 11); 3x3 stride 2 at (15, 31) and (17, 33); 3x3 with
# Cout 512 x Cin 32 (both 256-blocks); 1x1 with Cout 288 (the guarded block); 1x1 at stage 4's K = 2048
WGRAD_CASES = [(1, 64, 32, 2, 9, 11), (9, 32, 32, 2, 15, 31), (9, 32, 32, 2, 17, 33), (9, 32, 512, 1, 5, 7), (1, 64, 288, 1, 5, 7),
               (1, 2048, 64, 1, 4, 5), (9, 32, 512, 2, 5, 7)]


def case_id(c):
    return '-'.join(str(int(v)) for v in c)


def rand(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def bn_params(c, seed):
    """gamma, beta, running mean, running var (resnet_ref.randomize_'s ranges)."""
    g = torch.Generator().manual_seed(seed)
    return (1.0 + 0.25 * (torch.rand(c, generator=g) - 0.5), 0.5 * torch.randn(c, generator=g), 0.2 * torch.randn(c, generator=g),
            0.75 + 0.5 * torch.rand(c, generator=g))


def bn_stats(bn):
    """(3, C): scale, rstd, mean - what the weight gradients' finishing kernel reads."""
    gamma, _, mean, var = bn
    rstd = torch.rsqrt(var + T.EPS)
    return torch.stack((gamma * rstd, rstd, mean)).contiguous()


def half(h, w):
    return (h - 1) // 2 + 1, (w - 1) // 2 + 1


@functools.lru_cache(maxsize=None)
def dgrad_case(taps, cin, cout, stride, h, w, even):
    """(weight, bn, dz, {name: operand}, {variant: (keywords' names, fp64 reference)}): mask, add and add2 present and absent, and
    the even-pixel add where the case has one."""
    k = 3 if taps == 9 else 1
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    weight = rand(cout, cin, k, k, seed=2, scale=(2.0 / (taps * cin)) ** 0.5)
    bn = bn_params(cout, 3)
    dz = rand(N, cout, ho, wo, seed=4) * (rand(N, cout, ho, wo, seed=5) > 0)        # a masked gradient, as behind a ReLU
    ops = dict(add=rand(N, cin, h, w, seed=6), mask=rand(N, cin, h, w, seed=7), add2=rand(N, cin, h, w, seed=8),
               add_even=rand(N, cin, *half(h, w), seed=9))
    share = float((ops['mask'] > 0).double().mean())
    assert 0.2 <= share <= 0.8                                                        # the ReLU rule, on the mask map
    plain = T.unit_data_grad(dz.double(), weight, bn, (h, w), stride)
    a, m, a2, ae = (ops[n].double() for n in ('add', 'mask', 'add2', 'add_even'))
    variants = {'plain': ((), plain),
                'add+mask': (('add', 'mask'), (plain + a) * (m > 0)),
                'add2': (('add2',), plain + a2),
                'add+mask+add2': (('add', 'mask', 'add2'), (plain + a) * (m > 0) + a2)}
    if even:
        variants['add_even'] = (('add_even',), T.even_pixels_add(plain, ae))
        variants['mask+add2+add_even'] = (('mask', 'add2', 'add_even'), T.even_pixels_add(plain * (m > 0) + a2, ae))
    return weight, bn, dz, ops, variants


@functools.lru_cache(maxsize=None)
def wgrad_case(taps, cin, cout, stride, h, w):
    """(x, weight, bn, dz, (dW, dgamma, dbeta) in fp64)."""
    k = 3 if taps == 9 else 1
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    x = torch.relu(rand(N, cin, h, w, seed=1))
    weight = rand(cout, cin, k, k, seed=2, scale=(2.0 / (taps * cin)) ** 0.5)
    bn = bn_params(cout, 3)
    dz = rand(N, cout, ho, wo, seed=4) * (rand(N, cout, ho, wo, seed=5) > 0)
    return x, weight, bn, dz, T.unit_param_grads(dz.double(), x.double(), weight, bn, stride)
