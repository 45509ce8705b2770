"""GPU: the prepack entry points stay inside the sizes the library reports (SrPackLayout / ConvPackLayout, csrc/r3d_sr_common.h).
The buffer is ONE allocation of *_prepacked_bytes + a 4096-byte guard filled with a pattern: a region that ran past `total` lands in the guard
(a failed assertion, never a fault)."""
import pytest

pytestmark = pytest.mark.gpu

GUARD, PATTERN = 4096, 0xA5


def _guarded(torch, nbytes):
    buf = torch.empty(nbytes + GUARD, dtype=torch.uint8, device="cuda")
    buf[nbytes:] = PATTERN
    return buf


def _guard_intact(torch, buf, nbytes):
    torch.cuda.synchronize()
    return bool((buf[nbytes:] == PATTERN).all())


def test_prepack_stays_inside_prepacked_bytes():
    import torch
    from real3dportrait_amd import _lib
    assert torch.cuda.is_available()
    lib = _lib.load()
    g = torch.Generator(device="cpu").manual_seed(7)
    Cin, Cout = 16, 128                                         # every region of the block pack; R3D_SR_F16MX writes all eight
    w0, w1 = torch.randn(Cout, Cin, 3, 3, generator=g).cuda(), torch.randn(Cout, Cout, 3, 3, generator=g).cuda()
    nbytes = int(lib.r3d_sr_block_prepacked_bytes(Cin, Cout))
    for prec in (0, 1, 2):                                      # R3D_SR_F32, R3D_SR_F16X3, R3D_SR_F16MX
        buf = _guarded(torch, nbytes)
        _lib.check(lib.r3d_sr_block_prepack(Cin, Cout, _lib.ptr(w0), _lib.ptr(w1), _lib.ptr(buf), prec, _lib.stream_ptr()), "sr_block_prepack")
        assert _guard_intact(torch, buf, nbytes), "r3d_sr_block_prepack(precision %d) wrote past r3d_sr_block_prepacked_bytes" % prec
    for Cin, Cout, k in ((3, 4, 3), (16, 128, 1), (20, 132, 3)):        # both channel counts padded; 1x1 (two regions); padded to 32 x 256
        w = torch.randn(Cout, Cin, k, k, generator=g).cuda()
        nbytes = int(lib.r3d_conv_prepacked_bytes(Cin, Cout, k))
        buf = _guarded(torch, nbytes)
        _lib.check(lib.r3d_conv_prepack(_lib.ptr(w), Cin, Cout, k, _lib.ptr(buf), _lib.stream_ptr()), "conv_prepack")
        assert _guard_intact(torch, buf, nbytes), "r3d_conv_prepack(%d, %d, k = %d) wrote past r3d_conv_prepacked_bytes" % (Cin, Cout, k)
