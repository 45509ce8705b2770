"""The two decisions every operator's host state rests on, stated once.

    Derived         is a value computed from tensors stale?  It is valid while every source is the same object at the same _version and
                    a hashable `extra` (device, precision, N ...) is equal.  Never an address: the allocator hands a freed block, and a
                    fresh tensor's version 0, to the next tensor of that size.
    StreamBuffers   which buffers may a launch on this stream use?  What a factory made for (device, current stream, *shape): two streams
                    in flight never share one.
    _DeviceBuffers  one grow-only uint8 buffer per attribute, for an object that runs on one stream (frames.clone_generator_shell).
"""
import torch
import torch.nn as nn


class Derived:
    """get(sources, fn, extra) -> fn(), computed again only when valid(sources, extra) fails.  The entry holds its sources, so their
    addresses cannot be recycled while it lives; `generation` counts the recomputations."""

    def __init__(self):
        self._srcs, self._versions, self._extra, self._val, self.generation = (), (), None, None, 0

    def valid(self, sources, extra=None):
        if len(sources) != len(self._srcs) or extra != self._extra or self.generation == 0:
            return False
        return all(t is s and t._version == v for t, s, v in zip(sources, self._srcs, self._versions))

    def put(self, sources, value, extra=None):
        self._srcs, self._versions, self._extra, self._val = tuple(sources), tuple(t._version for t in sources), extra, value
        self.generation += 1
        return value

    def get(self, sources, fn, extra=None):
        return self._val if self.valid(sources, extra) else self.put(sources, fn(), extra)


class StreamBuffers:
    """get(dev, *shape) -> factory(dev, *shape), made once per (dev, current stream, *shape).  cap: the store is emptied when it holds
    that many entries and another is needed (a long-lived process does not collect every shape it ever saw); None: no limit."""

    def __init__(self, factory, cap=None):
        self._factory, self._cap, self._entries = factory, cap, {}

    def __len__(self):
        return len(self._entries)

    def get(self, dev, *shape):
        key = (dev, torch.cuda.current_stream().cuda_stream) + shape
        b = self._entries.get(key)
        if b is None:
            b = self._factory(dev, *shape)
            if self._cap is not None and len(self._entries) >= self._cap:
                self._entries.clear()
            self._entries[key] = b
        return b


class _DeviceBuffers:
    """`_buf(name, nbytes, dev)`: the uint8 device buffer kept in attribute `name`, grown (or moved) when it does not hold nbytes on dev."""

    def _buf(self, name, nbytes, dev):
        t = getattr(self, name)
        if t is None or t.numel() < nbytes or t.device != dev:
            t = torch.empty(nbytes, device=dev, dtype=torch.uint8)
            setattr(self, name, t)
        return t


class _FoldedModule(nn.Module):
    """An nn.Module whose kernels read weights derived from its parameters.  A subclass supplies _fold() -> the derived weights and
    _new_buffers(dev, *shape) -> the work buffers of one launch."""

    def __init__(self):
        super().__init__()
        self._derived, self._work = Derived(), StreamBuffers(self._new_buffers)

    def _prepare(self):
        """_fold(), again only after a parameter or buffer was replaced, modified in place, moved or converted (Module.to keeps both the
        object and its version)."""
        srcs = list(self.parameters()) + list(self.buffers())
        with torch.no_grad():
            return self._derived.get(srcs, self._fold, tuple((t.device, t.dtype) for t in srcs))

    def _buffers_for(self, dev, *shape):
        return self._work.get(dev, *shape)

    def _check_device(self, t, what, own=None):
        """The device rule, first part: t (named `what` in the message) is on a GPU, and on the device of the module's parameters (of `own`,
        one of them; the first by default).  Raised before the library is entered."""
        if not t.is_cuda:
            raise ValueError("%s: the %s is not on a GPU: the library operates on device tensors only" % (type(self).__name__, what))
        own = (next(self.parameters()) if own is None else own).device
        if own != t.device:
            raise ValueError("%s: the %s is on %s, the module's parameters on %s" % (type(self).__name__, what, t.device, own))

    @staticmethod
    def _device_of(t):
        """The device rule, second part: `with self._device_of(t):` makes t's device the current one for the launches, so that
        torch.cuda.current_stream() is that device's stream whatever the process's current device is."""
        return torch.cuda.device(t.device)
