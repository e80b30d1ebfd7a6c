"""The harness of the memory-contract tests (test_memory_contract_gpu.py, test_deform_kernels_gpu.py): guarded outputs of one launch, the
pointers the wrappers hand to the library, and the two-launch discipline.  Not a test module; needs a GPU only when it is used."""
import ctypes

import torch

import dcn_train_ref
from guarded import embedded, guarded

DEV = 'cuda:0'
ATOMICS_TOL = 1e-6              # test_dcn_train_gpu.test_two_runs_only_dx_comes_from_atomics: dX between two runs, relative Frobenius


class Run:
    """The guarded outputs of one launch."""

    def __init__(self):
        self.guards = []

    def out(self, shape, holds=None, **kw):
        """A guarded output of `shape`, pre-filled with NaN - or with `holds`, for a kernel that works in place."""
        view, intact = guarded(tuple(shape), device=DEV, **kw)
        if holds is not None:
            view.copy_(holds)
        self.guards.append((tuple(shape), intact, view))
        return view

    def check(self, what):
        for i, (shape, intact, _) in enumerate(self.guards):
            assert intact(), f'{what}: memory beyond guarded buffer {i} {shape} was written'

    def holds(self, t):
        """t lies inside one of the guarded views."""
        for _, _, view in self.guards:
            begin = view.data_ptr()
            if t.untyped_storage().data_ptr() == view.untyped_storage().data_ptr() and \
                    begin <= t.data_ptr() and t.data_ptr() + t.numel() * t.element_size() <= begin + view.numel() * view.element_size():
                return True
        return False


class Handed:
    """Every device pointer the wrappers hand to the library while it is open (ops._call's arguments: pointers and pointer tables)."""

    def __enter__(self):
        from graph_detr4d_amd import ops
        self.ops, self.real, self.ptrs = ops, ops._call, set()
        ops._call = self
        return self

    def __exit__(self, *exc):
        self.ops._call = self.real

    def __call__(self, entry, *args):
        for a in args:
            if isinstance(a, ctypes.c_void_p):
                self.ptrs.add(a.value)
            elif isinstance(a, ctypes.Array) and a._type_ is ctypes.c_void_p:
                self.ptrs.update(a)
        return self.real(entry, *args)


def as_input(t):
    """A floating-point input on the device with NaNs around it."""
    return None if t is None else embedded(t.to(DEV).contiguous())


def err(what, got, ref, bound, metric):
    assert tuple(got.shape) == tuple(ref.shape), (what, tuple(got.shape), tuple(ref.shape))
    e = metric(got, ref)
    print(f'{what}: {e:.3e} (bound {bound:.1e})')
    assert e <= bound, f'{what}: {e:.3e} > {bound:.1e}'


def contract(what, launch, check, atomics=(), native=True):
    """launch(run) -> {name: result tensor}, its outputs taken from run.out(...); check(results) asserts the family's bounds.  Two
    launches into fresh guarded buffers: every guarded buffer reached the library (native: the launch goes through ops) and every
    result lies in one, guards intact, every result finite, the bound met, and the same bits both times (atomics: the results that
    follow an atomic hand-out, compared to ATOMICS_TOL in the relative Frobenius norm)."""
    first = None
    for attempt in range(2):
        run = Run()
        with Handed() as seen:
            res = {k: v for k, v in launch(run).items() if v is not None}
        torch.cuda.synchronize()
        assert run.guards, f'{what}: nothing was guarded'
        for i, (shape, _, view) in enumerate(run.guards):
            assert not native or view.data_ptr() in seen.ptrs, f'{what}: guarded buffer {i} {shape} was never handed to the library'
        for k, t in res.items():
            assert run.holds(t), f'{what} {k}: the result does not lie in a guarded buffer'
        run.check(what)
        for k, t in res.items():
            bad = int((~torch.isfinite(t)).sum())
            assert bad == 0, f'{what} {k}: {bad} of {t.numel()} entries are not finite - never written, or read from beyond an input'
        if first is None:
            check(res)
            first = {k: t.clone() for k, t in res.items()}
        else:
            for k, t in res.items():
                if k in atomics:
                    assert dcn_train_ref.rel_fro(t, first[k].cpu()) <= ATOMICS_TOL, f'{what} {k}: two runs differ'
                else:
                    assert torch.equal(t, first[k]), f'{what} {k}: two runs give different bits'
    return first
