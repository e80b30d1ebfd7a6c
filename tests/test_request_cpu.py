"""The request program's C ABI (gd4d_decoder_request_*): exported, validated before any GPU work, and usable - create, describe,
destroy - on a box without a GPU."""
import ctypes
import os
import re

import pytest

from graph_detr4d_amd import _lib, ops

NEW = ('gd4d_request_step_bytes', 'gd4d_decoder_request_create', 'gd4d_decoder_request_run', 'gd4d_decoder_request_destroy',
       'gd4d_decoder_request_describe')
EINVAL = -1


def test_request_symbols_are_exported_and_declared(repo_root):
    lib = _lib.load()
    hdr = open(os.path.join(repo_root, 'include', 'gd4d.h')).read()
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert re.search(r'\b%s\s*\(' % name, hdr)
    assert lib.gd4d_request_step_bytes() == ctypes.sizeof(ops.RequestStep)
    assert lib.gd4d_chain_op_bytes() == ctypes.sizeof(ops.ChainOp)
    assert ctypes.sizeof(ops.RequestRef) == 16 and ctypes.sizeof(ops.RequestPatch) == 24 and ctypes.sizeof(ops.RequestBinding) == 8


def _chain_step(nops=1, m=16):
    prog = (ops.ChainOp * max(nops, 1))()
    s = ops.RequestStep(kind=ops.REQ_ROW_CHAIN, nops_a=nops, prog_a=ctypes.addressof(prog))
    s.i[0] = m
    s.fbind[0] = s.fbind[1] = -1
    for r in s.p:
        r.binding = -1
    return s, prog


def _copy_step(binding=-1):
    s = ops.RequestStep(kind=ops.REQ_COPY)
    s.l[0] = 64
    s.fbind[0] = s.fbind[1] = -1
    for r in s.p:
        r.binding = -1
    s.p[0].binding = binding
    return s


def _create(steps, nbindings=2, n=None):
    lib = _lib.load()
    arr = (ops.RequestStep * len(steps))(*steps)
    handle = ctypes.c_void_p()
    code = lib.gd4d_decoder_request_create(ctypes.addressof(arr), len(steps) if n is None else n, nbindings, ctypes.addressof(handle))
    return code, handle


def _accepted(steps, nbindings=2):
    """create succeeds; the program is destroyed again."""
    code, handle = _create(steps, nbindings)
    return code == 0 and bool(handle.value) and _lib.load().gd4d_decoder_request_destroy(handle) == 0


def test_request_create_validates_before_any_gpu_work():
    lib = _lib.load()
    handle = ctypes.c_void_p()
    good, keep = _chain_step()
    # a null table, no steps
    assert lib.gd4d_decoder_request_create(None, 1, 0, ctypes.addressof(handle)) == EINVAL and not handle.value
    assert _create([good], n=0)[0] == EINVAL and _create([good], n=-3)[0] == EINVAL
    assert lib.gd4d_decoder_request_create(ctypes.addressof((ops.RequestStep * 1)(good)), 1, 0, None) == EINVAL
    # an unknown kind
    for kind in (0, 16, -1, 1000):
        bad, k2 = _chain_step()
        bad.kind = kind
        assert _create([bad])[0] == EINVAL
    # a binding index >= nbindings: a pointer argument, a scalar, a patch
    assert _create([_copy_step(binding=2)], nbindings=2)[0] == EINVAL
    assert _accepted([_copy_step(binding=1)], nbindings=2)
    patched, k3 = _chain_step()
    patch = (ops.RequestPatch * 1)(ops.RequestPatch(0, 5, ops.ChainOp.p0.offset, 0))
    patched.patches, patched.npatches = ctypes.addressof(patch), 1
    assert _create([patched], nbindings=5)[0] == EINVAL and _accepted([patched], nbindings=6)
    patch[0] = ops.RequestPatch(0, 0, ctypes.sizeof(ops.ChainOp), 0)                  # past the program's last operation
    assert _create([patched], nbindings=6)[0] == EINVAL
    patch[0] = ops.RequestPatch(1, 0, ops.ChainOp.p0.offset, 0)                       # a table the step does not have
    assert _create([patched], nbindings=6)[0] == EINVAL
    second, k6 = _chain_step()                                                       # a one-program step keeps no second table,
    other = (ops.ChainOp * 1)()                                                      # whatever its record points to
    second.prog_b, second.nops_b = ctypes.addressof(other), 1
    second.patches, second.npatches = ctypes.addressof(patch), 1
    assert _create([second], nbindings=6)[0] == EINVAL
    second.kind = ops.REQ_ROW_CHAIN2
    assert _accepted([second], nbindings=6)
    # a chain program with a null operation table / without operations / with too many
    null_prog, k4 = _chain_step()
    null_prog.prog_a = None
    assert _create([null_prog])[0] == EINVAL
    assert _create([_chain_step(nops=0)[0]])[0] == EINVAL and _create([_chain_step(nops=33)[0]])[0] == EINVAL
    two, k5 = _chain_step()
    two.kind, two.nops_b = ops.REQ_ROW_CHAIN2, 1                                     # the second program is missing
    assert _create([two])[0] == EINVAL
    # a wait for an event no earlier step records
    wait = ops.RequestStep(kind=ops.REQ_STREAM_WAIT, event=0)
    assert _create([good, wait])[0] == EINVAL
    record_later = ops.RequestStep(kind=ops.REQ_EVENT_RECORD, event=0, side=1)
    assert _create([wait, record_later])[0] == EINVAL
    assert _create([ops.RequestStep(kind=ops.REQ_EVENT_RECORD, event=64)])[0] == EINVAL
    # a plan without its host tables
    plan = ops.RequestStep(kind=ops.REQ_PLAN)
    assert _create([plan])[0] == EINVAL


def test_request_null_handles():
    lib = _lib.load()
    bind = (ops.RequestBinding * 2)()
    assert lib.gd4d_decoder_request_run(None, bind, 2, None, None) == EINVAL
    assert lib.gd4d_decoder_request_destroy(None) == EINVAL
    assert lib.gd4d_decoder_request_describe(None, 0) is None


def test_request_create_describe_destroy_without_a_gpu():
    """A hand-made two-step table: the program is a deep copy (the caller's records may go), describe names the entry points."""
    lib = _lib.load()
    chain, prog = _chain_step(nops=2, m=900)
    code, handle = _create([chain, _copy_step(binding=0)], nbindings=1)
    assert code == 0 and handle.value
    ctypes.memset(ctypes.addressof(prog), 0xff, ctypes.sizeof(prog))
    del chain, prog
    assert lib.gd4d_decoder_request_describe(handle, 0) == b'gd4d_row_chain_fwd'
    assert lib.gd4d_decoder_request_describe(handle, 1) == b'hipMemcpyAsync'
    assert lib.gd4d_decoder_request_describe(handle, 2) is None and lib.gd4d_decoder_request_describe(handle, -1) is None
    # the number of bindings is the program's
    bind = (ops.RequestBinding * 2)()
    assert lib.gd4d_decoder_request_run(handle, bind, 2, None, None) == EINVAL
    assert lib.gd4d_decoder_request_run(handle, None, 1, None, None) == EINVAL
    assert lib.gd4d_decoder_request_destroy(handle) == 0


def test_recorder_turns_wrapper_calls_into_steps():
    """ops.StepRecorder in place of the library: a wrapper's call becomes a step; pointers inside a binding's extent are bound, the
    others stay fixed; an entry point without a step kind raises."""

    class Fake:                                                    # (a tensor as far as the recorder looks: address, extent)
        def __init__(self, addr, nbytes):
            self.addr, self.nbytes = addr, nbytes

        def data_ptr(self):
            return self.addr

        def numel(self):
            return self.nbytes

        def element_size(self):
            return 1

        shape = property(lambda self: (self.nbytes,))

        def stride(self):
            return (1,)

    lib = _lib.load()
    rec = ops.StepRecorder(lib, main_stream=0x10)
    prog = (ops.ChainOp * 2)(ops.ChainOp(kind=ops.CHAIN_LOAD, p0=0x1000, gout=0x9000), ops.ChainOp(kind=ops.CHAIN_GEMM, p0=0x5000, gout=0x2040))
    with _lib.recording(rec):
        assert _lib.load() is rec
        assert _lib.load().gd4d_row_chain_fwd(prog, 2, 900, ctypes.c_void_p(0x10)) == 0
        assert _lib.load().gd4d_chain_op_bytes() == ctypes.sizeof(ops.ChainOp)             # size queries pass through
        with pytest.raises(_lib.Gd4dError):
            _lib.load().gd4d_linear_fwd
    assert _lib.load() is lib
    steps, keep = rec.steps({0: Fake(0x1000, 0x100), 1: Fake(0x2000, 0x100)}, {})
    assert len(steps) == 1 and steps[0].kind == ops.REQ_ROW_CHAIN and steps[0].side == 0 and steps[0].i[0] == 900
    patches = ctypes.cast(steps[0].patches, ctypes.POINTER(ops.RequestPatch))
    got = sorted((patches[k].binding, patches[k].offset, patches[k].add) for k in range(steps[0].npatches))
    assert got == [(0, ops.ChainOp.p0.offset, 0), (1, ctypes.sizeof(ops.ChainOp) + ops.ChainOp.gout.offset, 0x40)]
    handle = ctypes.c_void_p()
    assert lib.gd4d_decoder_request_create(ctypes.addressof(steps), 1, 2, ctypes.addressof(handle)) == 0
    assert lib.gd4d_decoder_request_describe(handle, 0) == b'gd4d_row_chain_fwd'
    assert lib.gd4d_decoder_request_destroy(handle) == 0


def test_recording_is_per_thread():
    """While one thread records a program, another thread's _lib.load() is the library: its requests keep launching."""
    import threading
    lib = _lib.load()
    rec = ops.StepRecorder(lib, main_stream=0)
    seen = []
    with _lib.recording(rec):
        t = threading.Thread(target=lambda: seen.append((_lib.load(), _lib.recorder())))
        t.start()
        t.join()
        assert _lib.load() is rec and _lib.recorder() is rec
    assert seen == [(lib, None)] and _lib.recorder() is None
