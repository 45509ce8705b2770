"""CPU: the two rules of real3dportrait_amd/_state.py -- Derived (is a value computed from tensors stale?) and StreamBuffers (which
buffers may a launch on this stream use?) -- and the helper the modules' own tests replace a parameter with."""
import gc
import weakref

import numpy as np
import pytest
import torch
import torch.nn as nn

from real3dportrait_amd import _state
from real3dportrait_amd._state import Derived, StreamBuffers


def same_address_pair():
    """(a, b, array): two tensors over ONE array, so equal data_ptr() and equal _version -- what the caching allocator makes of a freed
    tensor and the next one of its size."""
    arr = np.arange(6, dtype=np.float32).reshape(2, 3)
    a, b = torch.from_numpy(arr), torch.from_numpy(arr)
    assert a is not b and a.data_ptr() == b.data_ptr() and a._version == b._version
    return a, b, arr


def replaced_at_same_address(module, name, prepare):
    """Replace module.<name> twice by a new nn.Parameter over one array, scaled by 3 in between, so that the second has the first's
    data_ptr() and _version and other contents; returns (prepare() with the first, prepare() with the second)."""
    arr = getattr(module, name).detach().numpy().copy()
    first = nn.Parameter(torch.from_numpy(arr))
    setattr(module, name, first)
    before = prepare()
    arr *= 3.0
    second = nn.Parameter(torch.from_numpy(arr))
    setattr(module, name, second)
    assert second is not first and second.data_ptr() == first.data_ptr() and second._version == first._version
    return before, prepare()


def test_derived_serves_the_same_object_until_a_source_changes():
    d, calls = Derived(), []
    t, u = torch.ones(3), torch.zeros(2)

    def fn():
        calls.append(1)
        return [float(t.sum()), float(u.sum())]

    v = d.get([t, u], fn, extra=("cpu", 1))
    assert d.get([t, u], fn, extra=("cpu", 1)) is v and len(calls) == 1 and d.generation == 1
    t.add_(1.0)                                                    # an in-place edit
    v2 = d.get([t, u], fn, extra=("cpu", 1))
    assert v2 is not v and v2[0] == 6.0 and len(calls) == 2 and d.generation == 2
    assert d.get([t, u], fn, extra=("cpu", 2)) is not v2 and len(calls) == 3 and d.generation == 3          # another extra
    assert d.get([t], fn, extra=("cpu", 2)) is not None and len(calls) == 4 and d.generation == 4          # fewer sources
    assert d.get([t], fn, extra=("cpu", 2)) is not None and len(calls) == 4 and d.generation == 4


def test_derived_recomputes_for_another_tensor_at_the_same_address_and_version():
    a, b, arr = same_address_pair()
    d = Derived()
    va = d.get([a], lambda: a.clone())
    arr *= 2.0
    vb = d.get([b], lambda: b.clone())
    assert vb is not va and torch.equal(vb, torch.from_numpy(arr)) and not torch.equal(vb, va) and d.generation == 2
    # the other construction: two tensors set_ on one storage, both at version 1
    s = torch.arange(6.0).untyped_storage()
    x, y = torch.empty(0).set_(s, 0, (2, 3), (3, 1)), torch.empty(0).set_(s, 0, (2, 3), (3, 1))
    assert x is not y and x.data_ptr() == y.data_ptr() and x._version == y._version == 1
    vx = d.get([x], lambda: 1)
    assert d.get([y], lambda: 2) == 2 and vx == 1 and d.generation == 4


def test_derived_keeps_its_sources_alive():
    d = Derived()
    t = torch.ones(4)
    ref = weakref.ref(t)
    d.get([t], lambda: 0)
    del t
    gc.collect()
    assert ref() is not None          # held: its address cannot be handed to another tensor while the entry lives
    d.get([torch.zeros(4)], lambda: 1)
    gc.collect()
    assert ref() is None              # and released with the entry


def test_valid_and_put_are_the_two_halves_of_get():
    d, t = Derived(), torch.ones(2)
    assert not d.valid([], None) and not d.valid([t], 5)
    d.put([t], None, 5)
    assert d.valid([t], 5) and not d.valid([t], 6) and d.generation == 1
    t.mul_(2.0)
    assert not d.valid([t], 5)


def test_stream_buffers_make_one_entry_per_device_stream_and_shape(monkeypatch):
    class Stream:
        cuda_stream = 11
    monkeypatch.setattr(_state.torch.cuda, "current_stream", lambda: Stream)          # the CPU has no current stream
    made = []

    def factory(dev, *shape):
        made.append((dev, shape))
        return object()

    sb = StreamBuffers(factory)
    a = sb.get("cuda:0", 2, 3)
    assert sb.get("cuda:0", 2, 3) is a and len(sb) == 1 and made == [("cuda:0", (2, 3))]
    b = sb.get("cuda:0", 2, 4)
    Stream.cuda_stream = 12
    c = sb.get("cuda:0", 2, 3)                                      # another stream never shares the first one's buffers
    d = sb.get("cuda:1", 2, 3)
    assert len({id(o) for o in (a, b, c, d)}) == 4 and len(sb) == 4 and len(made) == 4
    Stream.cuda_stream = 11
    assert sb.get("cuda:0", 2, 3) is a and sb.get("cuda:0", 2, 4) is b and len(made) == 4
    for n in range(20):                                             # no cap: nothing is ever dropped
        sb.get("cuda:0", n)
    assert len(sb) == 24 and sb.get("cuda:0", 2, 3) is a


def test_stream_buffers_cap_empties_the_store_when_it_is_reached(monkeypatch):
    class Stream:
        cuda_stream = 0
    monkeypatch.setattr(_state.torch.cuda, "current_stream", lambda: Stream)
    made = []

    def factory(dev, n):
        if n < 0:
            raise ValueError("refused")
        made.append(n)
        return [n]

    sb = StreamBuffers(factory, cap=8)
    first = [sb.get("d", n) for n in range(8)]
    assert len(sb) == 8 and all(sb.get("d", n) is first[n] for n in range(8)) and made == list(range(8))
    with pytest.raises(ValueError):
        sb.get("d", -1)
    assert len(sb) == 8                                             # a refused shape drops nothing
    ninth = sb.get("d", 8)
    assert len(sb) == 1 and sb.get("d", 8) is ninth                 # the cap was reached: cleared, then the new entry
    assert sb.get("d", 0) is not first[0] and len(sb) == 2 and made == list(range(9)) + [0]
