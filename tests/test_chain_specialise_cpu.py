"""Which instantiation of the chain kernel a program gets (gd4d_row_chain_choice; no GPU): the programs of the inference step -
written out here operation by operation as fused_decoder.run_single, initial_reference and functional.head_outputs build them - take
their table entries, anything outside every mask takes a generic kernel, the process-wide switch sends everything to it, and a
program a launch refuses is refused by the same code."""
import ctypes

import pytest

EINVAL, EUNSUPPORTED, EALIGN = -1, -2, -3
_BUF = (ctypes.c_float * 96)()
P = (ctypes.addressof(_BUF) + 63) & ~63             # a 16-byte aligned address nobody dereferences without a GPU


def _ops():
    from graph_detr4d_amd import ops
    return ops


def load(dst, n=256, second=False, inv=False, out=False):
    o = _ops()
    return o.ChainOp(kind=o.CHAIN_LOAD, src=-1, dst=dst, res=-1, N=n, ld0=n, ld1=n if second else 0, flags=o.CHAIN_INV_SIGMOID if inv else 0,
                     p0=P, p1=P if second else None, gout=P if out else None, ldg=n if out else 0)


def gemm(src, n=256, k=256, dst=-1, res=-1, flags=0, out=False, add=False, **kw):
    o = _ops()
    return o.ChainOp(kind=o.CHAIN_GEMM, src=src, dst=dst, res=res, K=k, N=n, flags=flags, p0=P, p1=P, gout=P if out else None,
                     ldg=n if out else 0, p2=P if add else None, ld2=n if add else 0, **kw)


def in_proj(src, src2):
    o = _ops()
    return o.ChainOp(kind=o.CHAIN_GEMM, src=src, dst=-1, res=src2, K=256, N=768, flags=o.CHAIN_SRC2 | o.CHAIN_SPLIT_KV, ld0=512, ldg=768,
                     p0=P, p1=P, gout=P, p2=P, ld2=8 * 4 * 512, p3=P, ld1=8 * 2 * 1024)


def three_outputs(src, exact):
    o = _ops()
    return o.ChainOp(kind=o.CHAIN_GEMM, src=src, dst=-1, res=-1, K=256, N=248, flags=o.CHAIN_SPLIT_OUT | (o.CHAIN_EXACT if exact else 0),
                     ldg=24, ld2=96, ld1=128, p0=P, p1=P, gout=P, p2=P, p3=P)


def layernorm(src, dst=-1, relu=False, out=False, dst2=-1, n=256):
    o = _ops()
    return o.ChainOp(kind=o.CHAIN_LAYERNORM, src=src, dst=dst, res=dst2, N=n, eps=1e-5, flags=o.CHAIN_RELU if relu else 0, p0=P, p1=P,
                     gout=P if out else None, ldg=n if out else 0, p2=P if dst2 >= 0 else None, ld2=n if dst2 >= 0 else 0)


def headgemm(addend=True):
    o = _ops()
    return o.ChainOp(kind=o.CHAIN_HEADGEMM, src=-1, dst=0, res=-1, K=256, N=256, ld0=8, ldg=256 if addend else 0, p0=P, p1=P, p2=P, p3=P,
                     flags=o.CHAIN_ADD_GOUT if addend else 0, gout=P if addend else None)


def reg_branch(src, tmp=(1, 2)):
    o = _ops()
    prog = []
    for i, n in enumerate((256, 256, 10)):
        prog.append(gemm(src, n=n, dst=tmp[i % 2], flags=o.CHAIN_EXACT | (o.CHAIN_RELU if i < 2 else 0)))
        src = tmp[i % 2]
    return prog + [o.ChainOp(kind=o.CHAIN_REFINE, src=src, dst=-1, res=-1, p0=P, gout=P)]


def position_encoder():
    o = _ops()
    return [load(0, n=3, inv=True), o.ChainOp(kind=o.CHAIN_SMALL_LINEAR, src=0, dst=1, res=-1, K=3, N=256, p0=P, p1=P),
            layernorm(1, dst=2, relu=True), gemm(2, dst=1), layernorm(1, relu=True, out=True),
            o.ChainOp(kind=o.CHAIN_SIGNAL, src=-1, dst=-1, res=-1, gout=P)]


def chain_b(last):
    o = _ops()
    prog = [headgemm(), o.ChainOp(kind=o.CHAIN_WAIT, src=-1, dst=-1, res=-1, p0=P, gout=P), load(3, second=True),
            gemm(0, dst=1, res=3), layernorm(1, dst=2), gemm(2, n=512, dst=0, flags=o.CHAIN_RELU), gemm(0, k=512, dst=1, res=2)]
    if last:
        return prog + [layernorm(1, dst=3, out=True)] + reg_branch(3)
    return prog + [layernorm(1, dst=3, out=True, dst2=0), in_proj(0, 3)]


def head_branch(exact):
    o = _ops()
    e = o.CHAIN_EXACT if exact else 0
    return [load(0), gemm(0, dst=1, flags=e), layernorm(1, dst=2, relu=True), gemm(2, dst=0, flags=e), layernorm(0, dst=1, relu=True),
            gemm(1, n=10, out=True, flags=e)]


def step_launches():
    """name -> (program a, program b or None, guests) of the inference step's launches."""
    o = _ops()
    chain_a = [load(0), gemm(0, dst=1, add=True), layernorm(1, dst=2, out=True, dst2=0)]
    return {
        'in_proj': ([load(0, second=True), load(1), in_proj(0, 1)], None, False),
        'initial_reference': ([load(0), gemm(0, n=3, out=True, flags=o.CHAIN_EXACT | o.CHAIN_SIGMOID)], None, False),
        'chain_a': (chain_a + [three_outputs(0, False)], [load(3)] + reg_branch(3), False),
        'chain_a layer 0, exact offsets': (chain_a + [three_outputs(0, True)], None, False),
        'chain_b': (position_encoder(), chain_b(False), True),
        'chain_b without guests': (position_encoder(), chain_b(False), False),
        'chain_b: the first in-projection with guests': ([load(0, second=True), load(1), in_proj(0, 1)], None, True),
        'chain_b_last': (position_encoder(), chain_b(True), False),
        'head': (head_branch(False), head_branch(True), False),
    }


def choice(a, b=None, guest=False):
    return _ops().row_chain_choice(a, b, guest)


def test_the_steps_programs_take_their_table_entries():
    for name, (a, b, guest) in step_launches().items():
        assert choice(a, b, guest) == name.split(':')[0].split(' ')[0], name


def test_programs_outside_every_mask_take_a_generic_kernel():
    o = _ops()
    add = o.ChainOp(kind=o.CHAIN_ADD, src=0, dst=1, res=-1, N=256)
    assert choice([load(0), add, gemm(1, out=True)]) == 'generic'                          # an operation no entry holds
    assert choice([load(0), gemm(0, out=True, flags=o.CHAIN_SIGMOID)]) == 'generic'         # a flag outside: sigmoid on three products
    assert choice([load(0), gemm(0, dst=1, add=True), layernorm(1, dst=2, out=True, dst2=0), three_outputs(0, False)], None, True) == 'generic'   # chain A with guests: only chain B' exists with them
    assert choice([load(0, out=True), gemm(0, out=True)]) == 'generic_train'               # a store from LOAD: a training program
    mask = gemm(0, out=True, add=True, flags=o.CHAIN_MASK_P2)
    assert choice([load(0), mask]) == 'generic_train'
    ln_bwd = o.ChainOp(kind=o.CHAIN_LN_BWD, src=0, dst=0, res=1, N=256, eps=1e-5, p0=P, p1=P)
    assert choice([load(0), load(1), ln_bwd]) == 'generic_train'


def test_the_switch_sends_inference_programs_to_the_generic_kernel():
    o = _ops()
    assert o.row_chain_specialise() is True                                                # the default, and asking changes nothing
    assert o.row_chain_specialise(False) is True
    try:
        assert o.row_chain_specialise() is False
        for name, (a, b, guest) in step_launches().items():
            assert choice(a, b, guest) == 'generic', name
        assert choice([load(0, out=True), gemm(0, out=True)]) == 'generic_train'
    finally:
        o.row_chain_specialise(True)
    assert o.row_chain_specialise() is True and choice(*step_launches()['chain_a']) == 'chain_a'


@pytest.mark.parametrize('code,what', [(EINVAL, 'no source'), (EINVAL, 'dst == src'), (EUNSUPPORTED, 'K not a multiple of 64'),
                                       (EALIGN, 'image not aligned'), (EINVAL, 'SIGNAL in a single program'), (EUNSUPPORTED, 'LayerNorm width'),
                                       (EINVAL, 'no operations'), (EUNSUPPORTED, 'too many operations')])
def test_validation_errors_are_the_launchs(code, what):
    """The choice refuses what the launch refuses, with the same code (both validate before anything touches a device)."""
    from graph_detr4d_amd import _lib
    o = _ops()
    bad = {'no source': [gemm(-1, out=True)], 'dst == src': [load(0), gemm(0, dst=0)], 'K not a multiple of 64': [load(0), gemm(0, k=96, out=True)],
           'image not aligned': [load(0), o.ChainOp(kind=o.CHAIN_GEMM, src=0, dst=1, res=-1, K=256, N=256, p0=P + 4)],
           'SIGNAL in a single program': [load(0), o.ChainOp(kind=o.CHAIN_SIGNAL, src=-1, dst=-1, res=-1, gout=P)],
           'LayerNorm width': [load(0), layernorm(0, dst=1, n=100)], 'no operations': [], 'too many operations': [load(0)] * 33}[what]
    lib = _lib.load()
    arr = (o.ChainOp * max(len(bad), 1))(*bad)
    assert lib.gd4d_row_chain_choice(arr, len(bad), None, 0, 0) == code
    assert lib.gd4d_row_chain_fwd(arr, len(bad), 37, None) == code
    if bad:
        with pytest.raises(_lib.Gd4dError):
            choice(bad)


def test_choice_names():
    from graph_detr4d_amd import _lib
    lib = _lib.load()
    assert [lib.gd4d_row_chain_choice_name(i) for i in range(-1, 9)] == [b'', b'generic', b'in_proj', b'initial_reference', b'chain_a', b'chain_b',
                                                                         b'chain_b_last', b'head', b'generic_train', b'']
