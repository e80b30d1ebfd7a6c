"""The one validity rule of every value derived from parameters and kept (ops._Stamp, ops.invalidate_chain_images), driven with CPU
tensors and a counting build function - no GPU."""
import copy
import gc
import pickle

import torch

from graph_detr4d_amd import ops


class Counter:
    """A cache in the form of ops._kept: table[key] = (stamp, value); `builds` counts the misses."""

    def __init__(self):
        self.table, self.builds = {}, 0

    def __call__(self, *sources, key='k'):
        def build():
            self.builds += 1
            return self.builds
        return ops._kept(self.table, key, sources, build)


def test_unchanged_source_hits_and_an_in_place_edit_misses():
    w = torch.randn(4, 8)
    c = Counter()
    assert c(w) == 1 and c(w) == 1
    w.add_(1)
    assert c(w) == 2 and c(w) == 2


def test_a_write_through_data_needs_the_epoch():
    w = torch.nn.Parameter(torch.randn(4, 8))
    c = Counter()
    c(w)
    w.data.copy_(torch.randn(4, 8))            # no version bump: the rule cannot see it ...
    assert c(w) == 1
    ops.invalidate_chain_images()              # ... until the caller says so
    assert c(w) == 2 and c(w) == 2


def test_another_tensor_at_the_same_address_and_version_misses():
    w = torch.randn(4, 8)
    twin = torch.empty(0).set_(w.untyped_storage()).view(4, 8)       # (set_ counts as one write of the new tensor)
    w.add_(0)
    c = Counter()
    c(w)
    assert twin.data_ptr() == w.data_ptr() and twin.shape == w.shape and twin._version == w._version
    assert c(twin) == 2


def test_shape_and_dtype_are_part_of_the_stamp():
    w = torch.randn(4, 8)
    s = ops._Stamp([w])
    assert s.valid([w]) and not s.valid([w.view(8, 4)]) and not s.valid([w.view(torch.int32)]) and not s.valid([w[:2]])


def test_a_view_of_the_same_base_behaves_like_the_base():
    w = torch.nn.Parameter(torch.randn(4, 8))
    c = Counter()
    assert c(w.view(4, 8)) == 1
    assert c(w.view(4, 8)) == 1 and c(w) == 1             # a new view object each call: still the same source
    with torch.no_grad():
        w.mul_(2)
    assert c(w.view(4, 8)) == 2


def test_absent_sources():
    w, b = torch.randn(4, 8), torch.randn(4)
    c = Counter()
    assert c(w, None) == 1 and c(w, None) == 1
    assert c(w, b) == 2 and c(w, b) == 2
    assert c(w, None) == 3
    assert not ops._Stamp([w, None]).valid([None, w]) and not ops._Stamp([w]).valid([w, None])


def test_the_entry_dies_with_its_source():
    w, b = torch.randn(4, 8), torch.randn(4)
    c = Counter()
    c(w, b, key='wb')
    c(w, key='w')
    del b
    gc.collect()
    assert set(c.table) == {'w'}
    del w
    gc.collect()
    assert not c.table


class Holder(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.lin = torch.nn.Linear(8, 4)
        self.keep = (ops._Stamp([self.lin.weight, self.lin.bias]), torch.ones(3))


def test_a_copied_module_never_validates():
    m = Holder()
    for twin in (copy.deepcopy(m), pickle.loads(pickle.dumps(m))):
        stamp, value = twin.keep
        assert torch.equal(value, m.keep[1])
        assert not stamp.valid([twin.lin.weight, twin.lin.bias]) and not stamp.valid([m.lin.weight, m.lin.bias])
    assert m.keep[0].valid([m.lin.weight, m.lin.bias])
