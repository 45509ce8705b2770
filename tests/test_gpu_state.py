"""GPU: the rules of real3dportrait_amd/_state.py where the device decides -- an SR conv and an SR block re-lay their weights for a
parameter that was replaced by another tensor at the same address and version (what the caching allocator makes of a freed one) and for
nothing else, and StreamBuffers hands a side stream buffers of its own."""
import collections

import pytest
import torch
import torch.nn as nn

from real3dportrait_amd import _lib
from real3dportrait_amd._state import StreamBuffers
from real3dportrait_amd.superresolution import Conv2d, SynthesisBlock

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def counted(fn):
    with _lib.counting() as calls:
        out = fn()
    torch.cuda.synchronize()
    return out, collections.Counter(name for name, _ in calls)


def replace_at_same_address(module, name):
    """module.<name> becomes a parameter set_ on a device storage of its own, then -- after that storage was scaled by 3 through another
    tensor, which bumps no version of the parameter's -- a second parameter set_ on the same storage: equal data_ptr(), equal _version,
    other contents.  Returns a function that makes the second replacement."""
    base = getattr(module, name).detach().clone()
    view = lambda: nn.Parameter(torch.empty(0, device=base.device).set_(base.untyped_storage(), 0, base.shape, base.stride()))
    first = view()
    setattr(module, name, first)

    def second():
        base.mul_(3.0)
        p = view()
        assert p is not first and p.data_ptr() == first.data_ptr() and p._version == first._version
        setattr(module, name, p)
    return second


def test_conv2d_prepacks_once_per_weight_tensor():
    torch.manual_seed(3)
    c = Conv2d(16, 16, 3, 1, 1).to(DEV)
    x = torch.randn(1, 16, 8, 8, device=DEV)
    replace = replace_at_same_address(c, "weight")
    y0 = c(x)
    y1, calls = counted(lambda: c(x))
    assert calls["r3d_conv_prepack"] == 0 and calls["r3d_conv_forward"] == 1 and torch.equal(y0, y1)
    replace()
    y2, calls = counted(lambda: c(x))
    assert calls["r3d_conv_prepack"] == 1 and calls["r3d_conv_forward"] == 1
    fresh = Conv2d(16, 16, 3, 1, 1).to(DEV)
    fresh.load_state_dict(c.state_dict())
    fresh.precision = c.precision
    assert torch.equal(y2, fresh(x)) and not torch.equal(y2, y1) and bool(torch.isfinite(y2).all())
    assert counted(lambda: c(x))[1]["r3d_conv_prepack"] == 0


def test_synthesis_block_prepacks_once_per_weight_tensor():
    torch.manual_seed(4)
    make = lambda: SynthesisBlock(16, 128, w_dim=512, resolution=16, img_channels=3, is_last=False, conv_clamp=None).to(DEV)
    blk = make()
    x, img, ws = torch.randn(1, 16, 8, 8, device=DEV), torch.randn(1, 3, 8, 8, device=DEV), torch.randn(1, 3, 512, device=DEV)
    run = lambda b: b(x, img, ws, noise_mode="none")
    replace = replace_at_same_address(blk.conv0, "weight")
    x0, img0 = run(blk)
    (x1, img1), calls = counted(lambda: run(blk))
    assert calls["r3d_sr_block_prepack"] == 0 and calls["r3d_sr_block_styles"] == 0 and calls["r3d_sr_block_forward"] == 1
    assert torch.equal(x0, x1) and torch.equal(img0, img1)
    replace()
    (x2, img2), calls = counted(lambda: run(blk))
    # the demodulation coefficients among the style vectors are sums over the weight: they follow it too
    assert calls["r3d_sr_block_prepack"] == 1 and calls["r3d_sr_block_styles"] == 1 and calls["r3d_sr_block_forward"] == 1
    fresh = make()
    fresh.load_state_dict(blk.state_dict())
    fresh.precision = blk.precision
    xf, imgf = run(fresh)
    assert torch.equal(x2, xf) and torch.equal(img2, imgf) and not torch.equal(img2, img1) and bool(torch.isfinite(img2).all())
    calls = counted(lambda: run(blk))[1]
    assert calls["r3d_sr_block_prepack"] == 0 and calls["r3d_sr_block_styles"] == 0


def test_stream_buffers_on_a_side_stream():
    dev = torch.device(DEV)
    sb = StreamBuffers(lambda d, n: torch.empty(n, device=d))
    a = sb.get(dev, 64)
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        b = sb.get(dev, 64)
        assert sb.get(dev, 64) is b
    assert b is not a and b.data_ptr() != a.data_ptr() and sb.get(dev, 64) is a and len(sb) == 2
    torch.cuda.synchronize()
