"""GPU: every r3d_torso_* entry point (include/r3d_hip.h, csrc/r3d_torso.hip) called directly, as torso_generator.py calls
it, and compared with a float64 torch statement of the same operation at the shapes and values where tiling, padding and addressing go
wrong: ragged tiles, 1-pixel images, channel counts off every vector width, coordinates outside the volume and exactly on its faces.

One error rule for every case (check), that of tests/test_gpu_secc_ops.py: e = max|y - y64| / max|y64| must stay within
max(2^-22 sqrt(K_eff), 4 e32), where e32 is the same statement evaluated in fp32 torch on the CPU and K_eff the reduction length:
ksize^2 Cin for the conv, 8 taps for the warp.  Inputs come from seeded CPU generators."""
import math

import pytest
import torch
import torch.nn.functional as F

from real3dportrait_amd import _lib
import torso_ref64 as R64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR = 2.0 ** -22


def call(name, *args):
    """Tensor arguments go in as device pointers; holding them here keeps temporaries alive until the launch is queued."""
    args = [_lib.ptr(a) if torch.is_tensor(a) else a for a in args]
    _lib.check(getattr(_lib.load(), "r3d_torso_" + name)(*args, _lib.stream_ptr()), "torso_" + name)


def randn(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


def dev(t):
    return t.float().contiguous().to(DEV)


def check(what, y, ref, keff):
    """y: the kernel's output (on the device, in the reference's layout); ref(dtype): the operation on the CPU in that dtype."""
    torch.cuda.synchronize()
    y = y.cpu().double()
    y64, y32 = ref(torch.float64), ref(torch.float32).double()
    assert y.shape == y64.shape and bool(torch.isfinite(y).all()), what
    m = float(y64.abs().max())
    assert m > 0.0, what
    e, e32 = float((y - y64).abs().max()) / m, float((y32 - y64).abs().max()) / m
    bound = max(FLOOR * math.sqrt(keff), 4.0 * e32)
    print("%s: e %.2e e32 %.2e bound %.2e%s" % (what, e, e32, bound, "  [within the floor only]" if e > 4.0 * e32 else ""))
    assert e <= bound, (what, e, e32, bound)
    return e


# ---- warp -------------------------------------------------------------------------------------------------------------------------------
def _identity(D, H, W):
    lin = lambda n: torch.linspace(-1.0, 1.0, n) if n > 1 else torch.zeros(1)
    z, y, x = torch.meshgrid(lin(D), lin(H), lin(W), indexing="ij")
    return torch.stack([x, y, z], dim=-1)


def _grid(g, kind, N, Do, Ho, Wo):
    if kind == "jitter":                    # the identity + noise: about a quarter of the points leave the volume
        return _identity(Do, Ho, Wo)[None] + randn(g, N, Do, Ho, Wo, 3, scale=0.2)
    if kind == "far":                       # every coordinate far outside, on either side
        return (torch.rand(N, Do, Ho, Wo, 3, generator=g) * 8.0 + 1.5) * torch.where(torch.rand(N, Do, Ho, Wo, 3, generator=g) < 0.5, -1.0, 1.0)
    if kind == "faces":                     # every coordinate exactly -1 or 1
        return torch.where(torch.rand(N, Do, Ho, Wo, 3, generator=g) < 0.5, -1.0, 1.0)
    if kind == "nodes":                     # exactly on source nodes (when the grid has the source's size)
        return _identity(Do, Ho, Wo)[None].expand(N, -1, -1, -1, -1).contiguous()
    return torch.rand(N, Do, Ho, Wo, 3, generator=g) * 2.0 - 1.0          # "inside"


WARP = [  # N, C, D, H, W, (Do, Ho, Wo) or None (the source's), grid kind
    (2, 32, 16, 24, 20, None, "jitter"), (1, 32, 16, 64, 64, None, "jitter"), (1, 32, 16, 8, 8, None, "far"), (2, 32, 4, 5, 7, None, "faces"),
    (1, 32, 16, 12, 9, None, "nodes"), (2, 32, 1, 9, 6, None, "jitter"), (1, 32, 1, 1, 1, None, "jitter"), (1, 5, 3, 4, 6, (2, 9, 5), "inside"),
    (3, 1, 2, 7, 3, (5, 1, 1), "jitter"), (1, 33, 16, 1, 10, None, "far"),
]


@pytest.mark.parametrize("channel_last", [0, 1])
@pytest.mark.parametrize("N,C,D,H,W,odims,kind", WARP)
def test_warp(N, C, D, H, W, odims, kind, channel_last):
    g = torch.Generator().manual_seed(500 + N + C + D + H + W)
    Do, Ho, Wo = odims or (D, H, W)
    fs, grid = randn(g, N, C, D, H, W), _grid(g, kind, N, Do, Ho, Wo).float()
    fsd, gd = dev(fs), dev(grid)
    cl = torch.empty(N, D, H, W, C, device=DEV)
    call("volume_to_cl", fsd, N, C, D, H, W, cl)
    assert torch.equal(cl, fsd.permute(0, 2, 3, 4, 1))
    out = torch.empty(N * C * Do * Ho * Wo, device=DEV)
    call("warp", cl, N, C, D, H, W, gd, Do, Ho, Wo, out, channel_last)
    y = out.view(N, Ho, Wo, C, Do).permute(0, 3, 4, 1, 2) if channel_last else out.view(N, C, Do, Ho, Wo)
    ref = lambda dt: F.grid_sample(fs.to(dt), grid.to(dt), align_corners=True, padding_mode="border")
    check("warp %s N%d C%d %dx%dx%d -> %dx%dx%d cl%d" % (kind, N, C, D, H, W, Do, Ho, Wo, channel_last), y, ref, 8)
    if kind == "nodes":                     # a point on a node is that node's value: weights 1 and 0 exactly (up to the coordinate's own rounding)
        torch.testing.assert_close(y.cpu(), fs, rtol=0, atol=2e-6 * float(fs.abs().max()))


def test_warp_restatement_is_the_one_the_module_tests_use():
    """tests/torso_ref64.py's spelt-out warp against grid_sample in fp64 on this device's inputs (it is the reference beyond the goldens)."""
    g = torch.Generator().manual_seed(77)
    fs, grid = randn(g, 2, 32, 16, 10, 12).double(), _grid(g, "jitter", 2, 16, 10, 12).double()
    ref = F.grid_sample(fs, grid, align_corners=True, padding_mode="border")
    assert float((R64.warp(fs, grid) - ref).abs().max()) <= 1e-14 * float(ref.abs().max())


# ---- conv -------------------------------------------------------------------------------------------------------------------------------
def _conv(seed, B, Hs, Ws, Cin, Cout, k, in_nchw=False, up=0, pro=None, pslope=0.0, act=0, slope=0.0, bias=True, res=None, out="cl",
          xscale=1.0, bias_scale=0.1):
    """pro: None or the size of the prologue's shift against the data ('large': t ~ 30 x the data).  res: None, 'separate', 'in_place'.
    out: 'cl', 'nchw' or 'both'.  Returns (outputs in NCHW, ref)."""
    g = torch.Generator().manual_seed(seed)
    H, W = Hs << up, Ws << up
    x = randn(g, B, Cin, Hs, Ws, scale=xscale)
    w = randn(g, Cout, Cin, k, k, scale=(Cin * k * k) ** -0.5)
    b = randn(g, Cout, scale=bias_scale) if bias else None
    ps = pt = None
    if pro:
        ps = torch.rand(Cin, generator=g) + 0.5
        pt = randn(g, Cin, scale=30.0 if pro == "large" else 0.5)
        pt = torch.where(pt.abs() < 0.05, torch.full_like(pt, 0.3), pt)
    r = randn(g, B, Cout, H, W) if res else None

    def ref(dt):
        a = x.to(dt)
        if pro:
            a = F.leaky_relu(a * ps.to(dt)[None, :, None, None] + pt.to(dt)[None, :, None, None], pslope)
        if up:
            a = F.interpolate(a, scale_factor=2, mode="nearest")
        y = F.conv2d(a, w.to(dt), b.to(dt) if bias else None, padding=k // 2)
        if act == 1:
            y = F.leaky_relu(y, slope)
        elif act == 2:
            y = torch.sigmoid(y)
        return y + r.to(dt) if res else y

    xd = dev(x) if in_nchw else dev(x.permute(0, 2, 3, 1))
    wd = dev(w.permute(0, 2, 3, 1))
    y = (dev(r.permute(0, 2, 3, 1)) if res == "in_place" else torch.empty(B, H, W, Cout, device=DEV)) if out in ("cl", "both") else None
    yn = torch.empty(B, Cout, H, W, device=DEV) if out in ("nchw", "both") else None
    rd = None
    if res:
        rd = y if res == "in_place" else dev(r.permute(0, 2, 3, 1))
    call("conv", xd, B, Hs, Ws, Cin, int(in_nchw), up, dev(ps) if pro else None, dev(pt) if pro else None, float(pslope), wd,
         dev(b) if bias else None, Cout, k, act, float(slope), rd, y, yn)
    outs = ([y.permute(0, 3, 1, 2)] if y is not None else []) + ([yn] if yn is not None else [])
    return outs, ref


def _check_conv(what, outs, ref, keff):
    for o in outs:
        check(what, o, ref, keff)
    if len(outs) == 2:
        assert torch.equal(outs[0], outs[1]), what


KS, CINS, COUTS = (1, 3, 7), (1, 3, 32, 65, 512), (1, 3, 64, 256)
SIZES = [(1, 1), (1, 5), (5, 1), (63, 65), (65, 63), (5, 63), (63, 5), (1, 65)]
CONV_SHAPES = []
for i, k in enumerate(KS):
    for j, cin in enumerate(CINS):
        for c, cout in enumerate(COUTS):
            Hs, Ws = SIZES[(3 * i + 2 * j + c) % 8]
            if cin == 512 and k == 7 and Hs * Ws > 400:       # (keeps the fp64 reference on the CPU short)
                Hs, Ws = 5, 63
            CONV_SHAPES.append((1 + (i + j + c) % 2, Hs, Ws, cin, cout, k))


@pytest.mark.parametrize("B,Hs,Ws,Cin,Cout,k", CONV_SHAPES)
def test_conv_shapes(B, Hs, Ws, Cin, Cout, k):
    """Every ksize x Cin x Cout, channel-last in and out (Cin 32 and 512 take the 16-byte loader, the others the element loader)."""
    outs, ref = _conv(1000 + Hs + Ws + Cin + Cout + k, B, Hs, Ws, Cin, Cout, k, bias=(Cin + Cout) % 2 == 0)
    _check_conv("conv B%d %dx%d Cin%d Cout%d k%d" % (B, Hs, Ws, Cin, Cout, k), outs, ref, k * k * Cin)


@pytest.mark.parametrize("out", ["nchw", "both"])
@pytest.mark.parametrize("in_nchw", [False, True])
@pytest.mark.parametrize("B,Hs,Ws,Cin,Cout,k", [(2, 63, 65, 65, 32, 3), (1, 65, 63, 32, 3, 7), (3, 5, 5, 512, 256, 3), (1, 1, 1, 3, 1, 7),
                                                (2, 5, 63, 64, 64, 1), (1, 65, 5, 1, 64, 3)])
def test_conv_layouts(B, Hs, Ws, Cin, Cout, k, in_nchw, out):
    outs, ref = _conv(1100 + Hs + Cin + Cout, B, Hs, Ws, Cin, Cout, k, in_nchw=in_nchw, out=out, act=1, slope=0.2)
    _check_conv("conv layouts B%d %dx%d Cin%d Cout%d k%d in_nchw%d out %s" % (B, Hs, Ws, Cin, Cout, k, in_nchw, out), outs, ref, k * k * Cin)


@pytest.mark.parametrize("pslope", [0.0, 0.2])
@pytest.mark.parametrize("pro", ["small", "large"])
@pytest.mark.parametrize("B,Hs,Ws,Cin,Cout,k,in_nchw", [(1, 63, 65, 32, 64, 3, False), (2, 5, 5, 256, 256, 3, False), (1, 1, 1, 512, 3, 7, False),
                                                        (1, 65, 63, 65, 32, 3, True), (2, 5, 63, 3, 64, 7, False), (1, 1, 5, 32, 1, 3, False)])
def test_conv_prologue(B, Hs, Ws, Cin, Cout, k, in_nchw, pro, pslope):
    """act(s x + t) in the tap loads, zero outside the image after it.  'large': t is 30 x the data, so a kernel that padded with act(t)
    instead of 0 would be wrong by the size of the output along every border (and everywhere on a 1 x 1 image)."""
    outs, ref = _conv(1200 + Hs + Cin + Cout, B, Hs, Ws, Cin, Cout, k, in_nchw=in_nchw, pro=pro, pslope=pslope)
    _check_conv("conv prologue %s slope %g B%d %dx%d Cin%d Cout%d k%d" % (pro, pslope, B, Hs, Ws, Cin, Cout, k), outs, ref, k * k * Cin)


def test_conv_prologue_padding_rule_is_visible_to_the_check():
    """The bound of test_conv_prologue('large') is far below what padding with act(t) would cost."""
    g = torch.Generator().manual_seed(5)
    x, w, t = randn(g, 1, 32, 5, 5).double(), randn(g, 8, 32, 3, 3, scale=288 ** -0.5).double(), randn(g, 32, scale=30.0).double()
    a = F.relu(x + t[None, :, None, None])
    right = F.conv2d(a, w, padding=1)
    wrong = F.conv2d(F.pad(a, (1, 1, 1, 1)) + F.pad(torch.zeros_like(a), (1, 1, 1, 1), value=1.0) * F.relu(t)[None, :, None, None], w)
    assert float((right - wrong).abs().max() / right.abs().max()) > 0.05


@pytest.mark.parametrize("pro", [None, "large"])
@pytest.mark.parametrize("B,Hs,Ws,Cin,Cout,k", [(1, 1, 1, 32, 64, 3), (2, 5, 3, 256, 128, 3), (1, 31, 33, 128, 64, 3), (1, 7, 1, 3, 3, 7),
                                                (1, 1, 9, 65, 1, 1)])
def test_conv_upsample_from_odd_sizes(B, Hs, Ws, Cin, Cout, k, pro):
    # (LeakyReLU 0.2, not ReLU: behind a one-signed prologue a single output channel can be negative everywhere)
    outs, ref = _conv(1300 + Hs + Cin + Cout, B, Hs, Ws, Cin, Cout, k, up=1, pro=pro, act=1, slope=0.2, out="both")
    _check_conv("conv up B%d %dx%d Cin%d Cout%d k%d pro %s" % (B, Hs, Ws, Cin, Cout, k, pro), outs, ref, k * k * Cin)


@pytest.mark.parametrize("res", ["separate", "in_place"])
@pytest.mark.parametrize("B,Hs,Ws,Cin,Cout,k,act", [(1, 63, 65, 256, 256, 3, 0), (2, 5, 5, 32, 3, 3, 1), (1, 65, 1, 3, 64, 1, 0), (3, 1, 1, 512, 65, 3, 1)])
def test_conv_residual(B, Hs, Ws, Cin, Cout, k, act, res):
    outs, ref = _conv(1400 + Hs + Cin + Cout, B, Hs, Ws, Cin, Cout, k, act=act, slope=0.2, res=res)
    _check_conv("conv residual %s B%d %dx%d Cin%d Cout%d k%d" % (res, B, Hs, Ws, Cin, Cout, k), outs, ref, k * k * Cin)


@pytest.mark.parametrize("B,Hs,Ws,Cin,Cout,k", [(1, 63, 65, 32, 1, 3), (2, 5, 5, 65, 3, 3), (1, 1, 1, 3, 64, 1)])
def test_conv_sigmoid_to_plus_minus_30(B, Hs, Ws, Cin, Cout, k):
    """Pre-activations spread over about [-35, 35] (bias ~ 12 n): the sigmoid saturates on both sides without a NaN or an Inf."""
    outs, ref = _conv(1500 + Hs + Cin + Cout, B, Hs, Ws, Cin, Cout, k, act=2, bias_scale=12.0, out="both")
    _check_conv("conv sigmoid B%d %dx%d Cin%d Cout%d k%d" % (B, Hs, Ws, Cin, Cout, k), outs, ref, k * k * Cin)
    assert float(outs[0].min()) >= 0.0 and float(outs[0].max()) <= 1.0


def test_conv_sigmoid_extremes():
    """Pre-activations of exactly +-30 and +-100 (zero weights, the bias alone)."""
    x = torch.zeros(1, 2, 2, 4, device=DEV)
    w = torch.zeros(4, 1, 1, 4, device=DEV)
    b = torch.tensor([-100.0, -30.0, 30.0, 100.0], device=DEV)
    y = torch.empty(1, 2, 2, 4, device=DEV)
    call("conv", x, 1, 2, 2, 4, 0, 0, None, None, 0.0, w, b, 4, 1, 2, 0.0, None, y, None)
    torch.cuda.synchronize()
    ref = torch.sigmoid(b.double().cpu())
    got = y[0, 0, 0].double().cpu()
    assert bool(torch.isfinite(got).all()) and float((got - ref).abs().max()) <= 2e-7, (got, ref)
    assert float(got[0]) == 0.0 or float(got[0]) < 1e-40
