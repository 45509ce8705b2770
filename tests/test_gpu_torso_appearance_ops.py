"""GPU: r3d_torso_conv_pool, r3d_torso_conv_split and r3d_torso_conv3d_res (include/r3d_hip.h, csrc/r3d_torso_appearance.hip)
called directly, as torso_appearance.py calls them, and compared with a float64 torch statement of the same operation on the CPU at the
shapes and values where the additions can go wrong: the smallest even images under the pool, ragged tiles, channel counts off the vector
width, both input layouts, a window the ReLU zeroes entirely, split runs of one channel and of thirty-two, a prologue with a positive shift
(so that a tap padded BEFORE it instead of after would be wrong on every border voxel, in depth too), the residual in place, both output
layouts from one launch.

One error rule for every case and both tiers, that of tests/test_gpu_torso_ops.py: e = max|y - y64| / max|y64| must stay within
max(2^-22 sqrt(K_eff), 4 e32), where e32 is the same statement evaluated in fp32 torch on the CPU and K_eff = kd ksize^2 Cin."""
import math

import pytest
import torch
import torch.nn.functional as F

import torso_motion_ref64 as R64
from test_gpu_torso_ops import DEV, FLOOR, call, dev, randn

pytestmark = pytest.mark.gpu
TIERS = [0, 1]                     # R3D_TORSO_F32, R3D_TORSO_BF16X3
WORST = {}                         # entry point -> (share of the bound, e, what): printed by test_report_the_worst_cases


def check(fn, what, y, ref, keff):
    """test_gpu_torso_ops.check, which also records the case that used the largest share of its bound."""
    torch.cuda.synchronize()
    y = y.cpu().double()
    y64, y32 = ref(torch.float64), ref(torch.float32).double()
    assert y.shape == y64.shape and bool(torch.isfinite(y).all()), what
    m = float(y64.abs().max())
    assert m > 0.0, what
    e, e32 = float((y - y64).abs().max()) / m, float((y32 - y64).abs().max()) / m
    bound = max(FLOOR * math.sqrt(keff), 4.0 * e32)
    print("%s: e %.2e e32 %.2e bound %.2e" % (what, e, e32, bound))
    if e / bound > WORST.get(fn, (0.0,))[0]:
        WORST[fn] = (e / bound, e, what)
    assert e <= bound, (what, e, e32, bound)


def _act(y, act, slope):
    return F.leaky_relu(y, slope) if act == 1 else torch.sigmoid(y) if act == 2 else y


# ---- r3d_torso_conv_pool ----------------------------------------------------------------------------------------------------------------
def _pool(seed, B, H, W, Cin, Cout, k, nchw, prec, act=1, slope=0.0, pool=1, negative_channel=False):
    g = torch.Generator().manual_seed(seed)
    x = randn(g, B, Cin, H, W)
    w = randn(g, Cout, Cin, k, k, scale=(Cin * k * k) ** -0.5)
    b = randn(g, Cout, scale=0.1)
    if negative_channel:
        b[0] = -100.0              # every window of channel 0 is negative before the ReLU

    def ref(dt):
        y = _act(F.conv2d(x.to(dt), w.to(dt), b.to(dt), padding=k // 2), act, slope)
        return F.avg_pool2d(y, (2, 2)) if pool else y

    y = torch.empty(B, H >> pool, W >> pool, Cout, device=DEV)
    call("conv_pool", dev(x if nchw else x.permute(0, 2, 3, 1)), B, H, W, Cin, int(nchw), dev(w.permute(0, 2, 3, 1)), dev(b), Cout, k, act, float(slope),
         pool, y, prec)
    return y.permute(0, 3, 1, 2), ref, k * k * Cin


POOL_SIZES = [(2, 2), (2, 6), (6, 2), (62, 66)]
POOL_PAIRS = [(cin, cout, (1, 3, 7)[(i + j) % 3], POOL_SIZES[(i + 2 * j) % 4], (i + j) % 2)
              for i, cin in enumerate((1, 3, 5, 8, 64)) for j, cout in enumerate((1, 4, 64, 128))]


@pytest.mark.parametrize("prec", TIERS)
@pytest.mark.parametrize("Cin,Cout,k,size,nchw", POOL_PAIRS)
def test_pool_channel_pairs(Cin, Cout, k, size, nchw, prec):
    """Every Cin x Cout with ksize, image size and input layout rotating (Cin 8 and 64 channel-last take the 16-byte loader).  LeakyReLU 0.2:
    a single output channel behind a single weight can be negative everywhere."""
    y, ref, keff = _pool(3000 + Cin + Cout + k, 2, size[0], size[1], Cin, Cout, k, nchw, prec, slope=0.2)
    check("conv_pool", "pool tier%d %dx%d Cin%d Cout%d k%d nchw%d" % (prec, size[0], size[1], Cin, Cout, k, nchw), y, ref, keff)


@pytest.mark.parametrize("prec", TIERS)
@pytest.mark.parametrize("nchw", [0, 1])
@pytest.mark.parametrize("H,W", POOL_SIZES)
@pytest.mark.parametrize("Cin,Cout,act", [(8, 64, 0), (5, 4, 1), (64, 128, 1)])
def test_pool_sizes_layouts_and_activations(H, W, Cin, Cout, act, nchw, prec):
    """Both layouts at every size; act none and ReLU, with one channel whose every window the ReLU zeroes (the average is exactly 0)."""
    y, ref, keff = _pool(3100 + H + W + Cin, 2, H, W, Cin, Cout, 3, nchw, prec, act=act, negative_channel=act == 1)
    check("conv_pool", "pool tier%d %dx%d Cin%d Cout%d act%d nchw%d" % (prec, H, W, Cin, Cout, act, nchw), y, ref, keff)
    if act == 1:
        assert float(y[:, 0].abs().max()) == 0.0 and float(y[:, 1:].abs().max()) > 0.0


# ---- r3d_torso_conv_split ---------------------------------------------------------------------------------------------------------------
def _split(seed, B, H, W, Cin, C, D, k, prec, nchw=0):
    """Returns (the volume as [B, C, D, H, W], ref, K_eff, (the whole buffer, its fill, floats written))."""
    g = torch.Generator().manual_seed(seed)
    x = randn(g, B, Cin, H, W)
    w = randn(g, C * D, Cin, k, k, scale=(Cin * k * k) ** -0.5)          # the reference's order: channel c D + d
    b = randn(g, C * D, scale=0.1)
    ref = lambda dt: F.conv2d(x.to(dt), w.to(dt), b.to(dt), padding=k // 2).view(B, C, D, H, W)
    wk = w.view(C, D, Cin, k, k).transpose(0, 1).reshape(C * D, Cin, k, k).permute(0, 2, 3, 1)
    bk = b.view(C, D).t().reshape(-1)
    n = B * D * H * W * C
    fill = randn(g, n + 64)
    buf = dev(fill)
    call("conv_split", dev(x if nchw else x.permute(0, 2, 3, 1)), B, H, W, Cin, int(nchw), dev(wk), dev(bk), C * D, k, 0, 0.0, D, buf, prec)
    return buf[:n].view(B, D, H, W, C).permute(0, 4, 1, 2, 3), ref, k * k * Cin, (buf, fill, n)


@pytest.mark.parametrize("prec", TIERS)
@pytest.mark.parametrize("H,W", [(1, 1), (5, 7)])
@pytest.mark.parametrize("C,D,Cin,k", [(1, 1, 5, 1), (1, 16, 8, 3), (3, 2, 5, 1), (32, 16, 256, 1)])
def test_split_store(C, D, Cin, k, H, W, prec):
    y, ref, keff, (buf, fill, n) = _split(3200 + C + D + H, 2, H, W, Cin, C, D, k, prec, nchw=int(Cin == 5 and H == 5))
    check("conv_split", "split tier%d C%d D%d %dx%d Cin%d k%d" % (prec, C, D, H, W, Cin, k), y, ref, keff)
    assert torch.equal(buf[n:].cpu(), fill[n:])                           # the floats behind the volume are bit-unchanged
    assert bool((buf[:n].cpu() != fill[:n]).all())                        # and every float of it was written


# ---- r3d_torso_conv3d_res ---------------------------------------------------------------------------------------------------------------
def _res(seed, B, D, H, W, Cin, Cout, k, prec, prologue=True, pslope=0.0, act=0, res=None, out="both"):
    """res: None, 'sep' (its own buffer) or 'alias' (y itself).  Returns (outputs as [B, Cout, D, H, W], ref, K_eff)."""
    g = torch.Generator().manual_seed(seed)
    x = randn(g, B, Cin, D, H, W)
    w = randn(g, Cout, Cin, k, k, k, scale=(Cin * k ** 3) ** -0.5)
    b = randn(g, Cout, scale=0.1)
    ps = 1.0 + 0.2 * randn(g, Cin)
    pt = 0.5 + 0.5 * torch.rand(Cin, generator=g)                         # positive: act(ps 0 + pt) != 0, a tap padded before the prologue shows
    r = randn(g, B, Cout, D, H, W)

    def ref(dt):
        a = x.to(dt)
        if prologue:
            a = F.leaky_relu(a * ps.to(dt)[None, :, None, None, None] + pt.to(dt)[None, :, None, None, None], pslope)
        y = _act(R64.conv3d(a, w.to(dt), b.to(dt), k // 2, dt), act, 0.0)
        return y + r.to(dt) if res else y

    r_cl = dev(r.permute(0, 2, 3, 4, 1))
    y = None
    if out in ("cl", "both") or res == "alias":
        y = r_cl.clone() if res == "alias" else torch.empty(B, D, H, W, Cout, device=DEV)
    yn = torch.empty(B, Cout, D, H, W, device=DEV) if out in ("ncdhw", "both") else None
    call("conv3d_res", dev(x.permute(0, 2, 3, 4, 1)), B, D, H, W, Cin, dev(ps) if prologue else None, dev(pt) if prologue else None, float(pslope),
         dev(w.permute(0, 2, 3, 4, 1)), dev(b), Cout, k, act, 0.0, y if res == "alias" else r_cl if res else None, y, yn, prec)
    outs = ([y.permute(0, 4, 1, 2, 3)] if y is not None else []) + ([yn] if yn is not None else [])
    return outs, ref, k ** 3 * Cin


def _check_res(what, outs, ref, keff):
    for o in outs:
        check("conv3d_res", what, o, ref, keff)
    if len(outs) == 2:
        assert torch.equal(outs[0], outs[1]), what


@pytest.mark.parametrize("prec", TIERS)
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("D", [1, 2, 16])
@pytest.mark.parametrize("H,W,Cin,Cout", [(1, 1, 32, 32), (2, 3, 5, 3), (6, 5, 28, 64), (9, 7, 32, 32)])
def test_res_prologue_depth_ksize_size(H, W, Cin, Cout, D, k, prec):
    """The prologue with a positive shift and the residual in place, y and y_ncdhw from one launch, from the 1 x 1 x 1 volume up."""
    outs, ref, keff = _res(3300 + H + Cin + D + k, 2, D, H, W, Cin, Cout, k, prec, act=(D + k) % 2, res="alias")
    _check_res("res tier%d D%d %dx%d Cin%d Cout%d k%d" % (prec, D, H, W, Cin, Cout, k), outs, ref, keff)


@pytest.mark.parametrize("prec", TIERS)
@pytest.mark.parametrize("prologue,pslope,res,out", [(True, 0.2, None, "cl"), (True, 0.0, "sep", "ncdhw"), (False, 0.0, "alias", "ncdhw"),
                                                     (False, 0.0, "sep", "both"), (True, 0.0, None, "both")])
def test_res_each_addition_alone(prologue, pslope, res, out, prec):
    outs, ref, keff = _res(3400, 1, 3, 6, 10, 32, 32, 3, prec, prologue=prologue, pslope=pslope, act=1, res=res, out=out)
    _check_res("res tier%d prologue%d slope%g res %s out %s" % (prec, prologue, pslope, res, out), outs, ref, keff)


def test_res_padding_follows_the_prologue():
    """A constant volume: with the zero AFTER the prologue an interior voxel and a corner voxel differ by the taps outside; padding before
    it would make every voxel equal."""
    B, D, H, W, Cn = 1, 4, 5, 5, 4
    x = torch.zeros(B, D, H, W, Cn, device=DEV)
    ps, pt = torch.ones(Cn, device=DEV), torch.full((Cn,), 2.0, device=DEV)
    w = torch.ones(1, 3, 3, 3, Cn, device=DEV)
    y = torch.empty(B, D, H, W, 1, device=DEV)
    call("conv3d_res", x, B, D, H, W, Cn, ps, pt, 0.0, w, None, 1, 3, 0, 0.0, None, y, None, 0)
    torch.cuda.synchronize()
    v = y.view(D, H, W).cpu()
    assert float(v[1, 2, 2]) == 27 * Cn * 2.0 and float(v[0, 0, 0]) == 8 * Cn * 2.0 and float(v[0, 2, 2]) == 18 * Cn * 2.0
    assert float(v[3, 4, 2]) == 12 * Cn * 2.0


# ---- the extractor's layers at the product shape -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", TIERS)
def test_product_down_convs(prec):
    for i, (H, Cin, Cout) in enumerate(((256, 64, 128), (128, 128, 256))):
        y, ref, keff = _pool(3500 + i, 1, H, H, Cin, Cout, 3, 0, prec)
        check("conv_pool", "product down.%d tier%d" % (i, prec), y, ref, keff)


@pytest.mark.parametrize("prec", TIERS)
def test_product_in_conv_and_mid_conv(prec):
    g = torch.Generator().manual_seed(3510)
    x, w, b = randn(g, 1, 5, 256, 256), randn(g, 64, 5, 7, 7, scale=245 ** -0.5), randn(g, 64, scale=0.1)
    y = torch.empty(1, 256, 256, 64, device=DEV)
    call("conv_prec", dev(x), 1, 256, 256, 5, 1, 0, None, None, 0.0, dev(w.permute(0, 2, 3, 1)), dev(b), 64, 7, 1, 0.0, None, y, None, prec)
    check("conv", "product in_conv tier%d" % prec, y.permute(0, 3, 1, 2), lambda dt: F.relu(F.conv2d(x.to(dt), w.to(dt), b.to(dt), padding=3)), 245)
    y, ref, keff, _ = _split(3511, 1, 64, 64, 256, 32, 16, 1, prec)
    check("conv_split", "product mid_conv tier%d" % prec, y, ref, keff)


@pytest.mark.parametrize("prec", TIERS)
def test_product_res_convs(prec):
    """Cin = Cout = 32 on 16 x 64 x 64: conv A (prologue, ReLU) and conv B (residual in place, both layouts)."""
    outs, ref, keff = _res(3520, 1, 16, 64, 64, 32, 32, 3, prec, act=1, out="cl")
    _check_res("product res conv A tier%d" % prec, outs, ref, keff)
    outs, ref, keff = _res(3521, 1, 16, 64, 64, 32, 32, 3, prec, prologue=False, res="alias", out="both")
    _check_res("product res conv B tier%d" % prec, outs, ref, keff)


# ---- with the additions off: the old entry points, bit for bit ----------------------------------------------------------------------------
@pytest.mark.parametrize("prec", TIERS)
@pytest.mark.parametrize("B,H,W,Cin,Cout,k,nchw", [(2, 9, 13, 32, 64, 3, 0), (1, 62, 66, 5, 4, 7, 1), (2, 6, 6, 3, 128, 1, 0), (1, 30, 34, 64, 20, 3, 0),
                                                   (1, 1, 1, 8, 1, 3, 0)])
def test_2d_entry_points_with_the_additions_off_equal_torso_conv(B, H, W, Cin, Cout, k, nchw, prec):
    g = torch.Generator().manual_seed(3600 + Cin)
    x = dev(randn(g, B, Cin, H, W) if nchw else randn(g, B, H, W, Cin))
    w, b = dev(randn(g, Cout, k, k, Cin, scale=0.1)), dev(randn(g, Cout))
    old, a, c = (torch.empty(B, H, W, Cout, device=DEV) for _ in range(3))
    call("conv_prec", x, B, H, W, Cin, nchw, 0, None, None, 0.0, w, b, Cout, k, 1, 0.2, None, old, None, prec)
    call("conv_pool", x, B, H, W, Cin, nchw, w, b, Cout, k, 1, 0.2, 0, a, prec)
    call("conv_split", x, B, H, W, Cin, nchw, w, b, Cout, k, 1, 0.2, 1, c, prec)
    torch.cuda.synchronize()
    assert torch.equal(a, old) and torch.equal(c, old)


@pytest.mark.parametrize("prec", TIERS)
@pytest.mark.parametrize("B,D,H,W,Cin,Cout,k", [(2, 16, 9, 13, 32, 32, 3), (1, 2, 6, 5, 5, 3, 3), (1, 1, 30, 34, 28, 64, 1), (1, 3, 4, 4, 4, 600, 3)])
def test_3d_entry_point_with_the_additions_off_equals_torso_conv3d(B, D, H, W, Cin, Cout, k, prec):
    g = torch.Generator().manual_seed(3700 + Cin)
    x, w, b = dev(randn(g, B, D, H, W, Cin)), dev(randn(g, Cout, k, k, k, Cin, scale=0.1)), dev(randn(g, Cout))
    old, new = (torch.empty(B, D, H, W, Cout, device=DEV) for _ in range(2))
    oldn, newn = (torch.empty(B, Cout, D, H, W, device=DEV) for _ in range(2))
    call("conv3d_prec", x, B, D, H, W, Cin, 0, w, b, Cout, k, 0, 1, 0.2, 0, old, Cout, 0, oldn, prec)
    call("conv3d_res", x, B, D, H, W, Cin, None, None, 0.0, w, b, Cout, k, 1, 0.2, None, new, newn, prec)
    torch.cuda.synchronize()
    assert torch.equal(new, old) and torch.equal(newn, oldn)


def test_report_the_worst_cases():
    """Last in the file: the largest share of its bound any case above used, per entry point (DESIGN 4.12 quotes these)."""
    for fn, (share, e, what) in sorted(WORST.items()):
        print("worst %s: e %.2e = %.0f %% of its bound (%s)" % (fn, e, 100 * share, what))
    assert all(share <= 1.0 for share, _, _ in WORST.values())
