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


class InPlace:
    """A cache in the form of ops.kept_in_place: the value is a tensor built from the sources, kept at a fixed address."""

    def __init__(self):
        self.table, self.builds = {}, 0

    def __call__(self, *sources, key='k'):
        def build():
            self.builds += 1
            assert not torch.is_grad_enabled()
            return sum(t.sum() for t in sources if t is not None) + torch.zeros(sources[0].shape[0])
        return ops.kept_in_place(self.table, key, sources, build, self)


def test_kept_in_place_hit_serves_the_same_object():
    w = torch.nn.Parameter(torch.randn(4, 8))
    c = InPlace()
    v = c(w)
    assert c(w) is v and c.builds == 1 and not v.requires_grad


def test_kept_in_place_rebuilds_into_the_same_buffer_after_an_in_place_edit():
    w = torch.randn(4, 8)
    c = InPlace()
    v = c(w)
    ptr, old = v.data_ptr(), v.clone()
    w.add_(1)
    v2 = c(w)
    assert v2 is v and v2.data_ptr() == ptr and c.builds == 2
    assert torch.equal(v2, w.sum() + torch.zeros(4)) and not torch.equal(v2, old)
    assert c(w) is v and c.builds == 2


def test_kept_in_place_a_shape_change_replaces_the_buffer():
    c = InPlace()
    v = c(torch.randn(4, 8))
    w2 = torch.randn(6, 8)
    v2 = c(w2)
    assert v2 is not v and v2.shape == (6,) and v.shape == (4,) and c.builds == 2
    assert c(w2) is v2


def test_kept_in_place_invalidate_forces_a_rebuild():
    w = torch.nn.Parameter(torch.randn(4, 8))
    c = InPlace()
    v = c(w)
    w.data.copy_(torch.randn(4, 8))
    assert c(w) is v and c.builds == 1
    ops.invalidate_chain_images()
    v2 = c(w)
    assert v2 is v and c.builds == 2 and torch.equal(v2, w.detach().sum() + torch.zeros(4))


def test_kept_in_place_accepts_an_absent_source():
    w, b = torch.randn(4, 8), torch.randn(4)
    c = InPlace()
    v = c(w, None)
    assert c(w, None) is v and c.builds == 1
    assert c(w, b) is v and c.builds == 2 and torch.equal(v, w.sum() + b.sum() + torch.zeros(4))
    first_absent = ops.kept_in_place({}, 'k', (None, w), lambda: w.sum(0), c)           # the device comes from the first tensor present
    assert torch.equal(first_absent, w.sum(0))
