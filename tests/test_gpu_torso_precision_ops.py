"""GPU: r3d_torso_conv_prec, r3d_torso_conv3d_prec and r3d_torso_split_bf16x3 (include/r3d_hip.h, csrc/r3d_torso_conv.h)
called directly with precision = R3D_TORSO_BF16X3, at the smallest shapes that reach every code path of the shared tile: each tile
selection with both loaders, the m-fast order, reductions of 1, 36, ragged and 13 824 entries, the 2-D and 3-D prologues and epilogues.

The error rule is check() of tests/test_gpu_torso_ops.py, unchanged -- e = max|y - y64| / max|y64| within max(2^-22 sqrt(K_eff), 4 e32)
against fp64 torch on the CPU -- and the case builders are those of the exact tier's tests (test_gpu_torso_ops._conv,
test_gpu_torso_motion_ops._conv3d) with their `call` routed to the _prec entry points.  The operand-range cases are the tier's own claim:
the same bound with the activations scaled by 2^e and the weights by 2^-e."""
import pytest
import torch
import torch.nn.functional as F

import test_gpu_torso_motion_ops as MOPS
import test_gpu_torso_ops as OPS
from real3dportrait_amd import _lib
from test_gpu_torso_ops import DEV, check, dev, randn
from test_torso_precision_host import split_values
from real3dportrait_amd.torso_precision import split_bf16x3

pytestmark = pytest.mark.gpu
BF16X3 = 1
_call = OPS.call


def call_prec(precision):
    def call(name, *args):
        if name in ("conv", "conv3d"):
            _call(name + "_prec", *args, precision)
        else:
            _call(name, *args)
    return call


@pytest.fixture(autouse=True)
def tier(monkeypatch):
    """The builders' conv / conv3d calls go through the _prec entry points with precision 1."""
    monkeypatch.setattr(OPS, "call", call_prec(BF16X3))
    monkeypatch.setattr(MOPS, "call", call_prec(BF16X3))


# ---- 1. the split ------------------------------------------------------------------------------------------------------------------------
def test_split_equals_the_host_mirror_bit_for_bit():
    x = split_values()
    n = x.numel()
    out = [torch.zeros(n, dtype=torch.int16, device=DEV) for _ in range(3)]
    _call("split_bf16x3", x.to(DEV), n, *out)
    torch.cuda.synchronize()
    for name, got, want in zip("hml", out, split_bf16x3(x)):
        bad = (got.cpu() != want.view(torch.int16)).nonzero().flatten()
        assert bad.numel() == 0, (name, bad[:8], x[bad[:8]])


# ---- 2. per-kernel parity ---------------------------------------------------------------------------------------------------------------
# tile branches of r3d_torso_conv3d: (Cout, few / many tiles); B, D, Hs, Ws.  Many: M = 2 x 2 x 91 x 91 = 33 124 positions, 259 row tiles of
# 128 (Cout <= 16: the 128 x 16 tile instead of 64 x 16) and 518 x 2 tiles of 64 x 64 (Cout > 32: 64 x 64 instead of 32 x 64)
TILES3 = [(1, "few"), (5, "few"), (1, "many"), (5, "many"), (24, "few"), (40, "few"), (72, "few"), (40, "many"), (72, "many")]


@pytest.mark.parametrize("Cin", [4, 5])
@pytest.mark.parametrize("Cout,tiles", TILES3)
def test_conv3d_tile_branches(Cout, tiles, Cin):
    B, D, Hs, Ws = (2, 2, 91, 91) if tiles == "many" else (2, 2, 6, 5)
    outs, ref, keff, _ = MOPS._conv3d(3000 + Cout + Cin + Hs, B, D, Hs, Ws, Cin, Cout, 3, act=1, slope=0.2, out="both")
    MOPS._check("bf16x3 conv3d tiles Cout%d %s Cin%d" % (Cout, tiles, Cin), outs, ref, keff)


# r3d_torso_conv: 128 x 16 up to 16 channels, 128 x 32 up to 32, 32 x 64 / 64 x 64 above (many: 2 x 91 x 91 = 16 562 pixels, 259 x 2 tiles of 64 x 64)
@pytest.mark.parametrize("Cin", [4, 5])
@pytest.mark.parametrize("Cout,tiles", [(1, "few"), (5, "many"), (24, "few"), (40, "few"), (72, "few"), (40, "many"), (72, "many")])
def test_conv_tile_branches(Cout, tiles, Cin):
    B, Hs, Ws = (2, 91, 91) if tiles == "many" else (2, 6, 5)
    outs, ref = OPS._conv(3100 + Cout + Cin + Hs, B, Hs, Ws, Cin, Cout, 3, act=1, slope=0.2, out="both")
    OPS._check_conv("bf16x3 conv tiles Cout%d %s Cin%d" % (Cout, tiles, Cin), outs, ref, 9 * Cin)


@pytest.mark.parametrize("Cin", [28, 25])
def test_conv3d_m_fast_order(Cin):
    """M = 2 x 2 x 2 x 2 = 16 positions under 40 channels."""
    outs, ref, keff, _ = MOPS._conv3d(3200 + Cin, 2, 2, 2, 2, Cin, 40, 3, act=1, slope=0.2, out="both")
    MOPS._check("bf16x3 conv3d m-fast Cin%d" % Cin, outs, ref, keff)


@pytest.mark.parametrize("Hs,Ws", [(1, 1), (2, 2), (6, 5), (17, 9)])
@pytest.mark.parametrize("Cin,k,D", [(1, 1, 1), (4, 3, 1), (25, 3, 2), (28, 3, 2), (89, 3, 1), (92, 3, 1)])
def test_reduction_lengths_and_image_sizes(Cin, k, D, Hs, Ws):
    """K = 1, K = 36 (the 2-D entry point), and K = 27 Cin / 9 Cin off the step of 32 through both loaders."""
    what = "bf16x3 K Cin%d k%d D%d %dx%d" % (Cin, k, D, Hs, Ws)
    if Cin <= 4:
        outs, ref = OPS._conv(3300 + Cin + Hs + Ws, 2, Hs, Ws, Cin, 40, k, out="both")
        OPS._check_conv(what, outs, ref, k * k * Cin)
    else:
        outs, ref, keff, _ = MOPS._conv3d(3300 + Cin + Hs + Ws, 2, D, Hs, Ws, Cin, 24, k, out="both")
        MOPS._check(what, outs, ref, keff)


def test_long_reduction():
    outs, ref, keff, _ = MOPS._conv3d(3400, 2, 2, 6, 5, 512, 40, 3, act=1, slope=0.2, out="both")
    assert keff == 13824
    MOPS._check("bf16x3 conv3d Cin512 k3 D2", outs, ref, keff)


# ---- the 2-D paths
@pytest.mark.parametrize("Cin,Cout", [(32, 40), (65, 24)])
@pytest.mark.parametrize("out", ["nchw", "both"])
def test_conv_in_nchw(Cin, Cout, out):
    outs, ref = OPS._conv(3500 + Cin, 2, 17, 9, Cin, Cout, 3, in_nchw=True, out=out, act=1, slope=0.2)
    OPS._check_conv("bf16x3 conv in_nchw Cin%d out %s" % (Cin, out), outs, ref, 9 * Cin)


@pytest.mark.parametrize("pslope", [0.0, 0.2])
@pytest.mark.parametrize("Hs,Ws,Cin,Cout,k,in_nchw", [(17, 9, 32, 40, 3, False), (6, 5, 25, 24, 3, False), (1, 1, 92, 5, 7, False), (6, 5, 65, 40, 3, True)])
def test_conv_prologue_before_the_padding(Hs, Ws, Cin, Cout, k, in_nchw, pslope):
    """The shift is 30 x the data: a kernel that split (or padded) before the prologue, or padded with act(t), would be wrong by the size of
    the output along every border (test_gpu_torso_ops.test_conv_prologue_padding_rule_is_visible_to_the_check)."""
    outs, ref = OPS._conv(3600 + Hs + Cin, 2, Hs, Ws, Cin, Cout, k, in_nchw=in_nchw, pro="large", pslope=pslope)
    OPS._check_conv("bf16x3 conv prologue slope %g %dx%d Cin%d" % (pslope, Hs, Ws, Cin), outs, ref, k * k * Cin)


@pytest.mark.parametrize("Cin,Cout", [(32, 40), (25, 5)])
def test_conv_residual_aliasing_y(Cin, Cout):
    outs, ref = OPS._conv(3700 + Cin, 2, 17, 9, Cin, Cout, 3, act=1, slope=0.2, res="in_place")
    OPS._check_conv("bf16x3 conv residual in place Cin%d" % Cin, outs, ref, 9 * Cin)


@pytest.mark.parametrize("Hs,Ws,Cin,Cout", [(1, 1, 32, 72), (6, 5, 25, 24)])
def test_conv_upsample(Hs, Ws, Cin, Cout):
    outs, ref = OPS._conv(3800 + Hs + Cin, 2, Hs, Ws, Cin, Cout, 3, up=1, pro="large", act=1, slope=0.2, out="both")
    OPS._check_conv("bf16x3 conv up %dx%d Cin%d" % (Hs, Ws, Cin), outs, ref, 9 * Cin)


def test_conv_sigmoid():
    outs, ref = OPS._conv(3900, 2, 17, 9, 65, 3, 3, act=2, bias_scale=12.0, out="both")            # pre-activations over about [-35, 35]
    OPS._check_conv("bf16x3 conv sigmoid", outs, ref, 9 * 65)
    assert float(outs[0].min()) >= 0.0 and float(outs[0].max()) <= 1.0
    OPS.test_conv_sigmoid_extremes()            # +-30 and +-100 exactly, through r3d_torso_conv_prec (the fixture)
    MOPS.test_conv3d_sigmoid_extremes()


# ---- the 3-D paths
@pytest.mark.parametrize("k", [1, 3, 7])
@pytest.mark.parametrize("D", [1, 2, 5])
@pytest.mark.parametrize("Cin,Cout", [(28, 40), (25, 5)])
def test_conv3d_depth_and_ksize(Cin, Cout, D, k):
    outs, ref, keff, _ = MOPS._conv3d(4000 + k + D + Cin, 2, D, 6, 5, Cin, Cout, k, act=1, slope=0.2, out="both")
    MOPS._check("bf16x3 conv3d k%d D%d Cin%d Cout%d" % (k, D, Cin, Cout), outs, ref, keff)


@pytest.mark.parametrize("Cin,Cout", [(28, 72), (25, 24)])
def test_conv3d_pool_and_upsample_from_the_smallest_sizes(Cin, Cout):
    outs, ref, keff, _ = MOPS._conv3d(4100 + Cin, 2, 2, 2, 2, Cin, Cout, 3, pool=1, act=1, slope=0.2)
    MOPS._check("bf16x3 conv3d pool from 2x2 Cin%d" % Cin, outs, ref, keff)
    outs, ref, keff, _ = MOPS._conv3d(4101 + Cin, 2, 2, 1, 1, Cin, Cout, 3, up=1, act=1, slope=0.2, out="both")
    MOPS._check("bf16x3 conv3d up from 1x1 Cin%d" % Cin, outs, ref, keff)
    outs, ref, keff, _ = MOPS._conv3d(4102 + Cin, 2, 2, 1, 1, Cin, Cout, 3, up=1, pool=1, act=1)
    MOPS._check("bf16x3 conv3d 1x1 up pool Cin%d" % Cin, outs, ref, keff)


@pytest.mark.parametrize("Cin,Cout", [(32, 2), (25, 40)])
def test_conv3d_full_depth_is_conv2d_on_the_viewed_tensor(Cin, Cout):
    outs, ref, keff, _ = MOPS._conv3d(4200 + Cin, 2, 3, 6, 5, Cin, Cout, 7, full=1, act=2, out="both")
    MOPS._check("bf16x3 conv3d full-depth D3 Cin%d Cout%d" % (Cin, Cout), outs, ref, keff)


@pytest.mark.parametrize("pool", [0, 1])
@pytest.mark.parametrize("Cin,Cout,ycs,yco", [(64, 32, 92, 28), (25, 5, 7, 2)])
def test_conv3d_channel_slice_leaves_the_rest_bit_unchanged(Cin, Cout, ycs, yco, pool):
    outs, ref, keff, (y, fill) = MOPS._conv3d(4300 + Cin + pool, 2, 2, 6, 6, Cin, Cout, 3, pool=pool, act=1, slope=0.2, ycs=ycs, yco=yco)
    MOPS._check("bf16x3 conv3d slice [%d, %d) of %d pool%d" % (yco, yco + Cout, ycs, pool), outs, ref, keff)
    got = y.cpu()
    keep = torch.ones(ycs, dtype=torch.bool)
    keep[yco:yco + Cout] = False
    assert torch.equal(got[:, keep], fill[:, keep]) and not torch.equal(got[:, ~keep], fill[:, ~keep])


# ---- 3. operand range --------------------------------------------------------------------------------------------------------------------
RANGE_CASES = [("conv", 32, 40), ("conv", 25, 24), ("conv3d", 28, 72)]          # 16-byte loader, element loader, the 3-D tile


def _range_case(kind, Cin, Cout, e, spike=False):
    """B = 2, 17 x 9 (D = 2 for conv3d), ksize 3, no bias: x 2^e against w 2^-e, so the result is the unscaled one and only the operands move."""
    g = torch.Generator().manual_seed(4400 + Cin + Cout)
    B, D, H, W = 2, (2 if kind == "conv3d" else 1), 17, 9
    x = randn(g, B, Cin, D, H, W)
    w = randn(g, Cout, Cin, 3 if kind == "conv3d" else 1, 3, 3, scale=(Cin * 9 * (3 if kind == "conv3d" else 1)) ** -0.5)
    if spike:
        x[1, Cin // 2, D - 1, 8, 4] = 2.0 ** 14
    x, w = x * 2.0 ** e, w * 2.0 ** -e
    assert bool(torch.isfinite(x).all()) and float(w.abs()[w != 0].min()) > 2.0 ** -100
    y = torch.empty(B, D, H, W, Cout, device=DEV)
    if kind == "conv3d":
        _call("conv3d_prec", dev(x.permute(0, 2, 3, 4, 1)), B, D, H, W, Cin, 0, dev(w.permute(0, 2, 3, 4, 1)), None, Cout, 3, 0, 0, 0.0, 0, y, Cout, 0,
              None, BF16X3)
        ref = lambda dt: F.conv3d(x.to(dt), w.to(dt), padding=1)
    else:
        _call("conv_prec", dev(x[:, :, 0].permute(0, 2, 3, 1)), B, H, W, Cin, 0, 0, None, None, 0.0, dev(w[:, :, 0].permute(0, 2, 3, 1)), None, Cout, 3, 0,
              0.0, None, y, None, BF16X3)
        ref = lambda dt: F.conv2d(x[:, :, 0].to(dt), w[:, :, 0].to(dt), padding=1)[:, :, None]
    return y.permute(0, 4, 1, 2, 3), ref, w.shape[2] * 9 * Cin, float(x.abs().max())


@pytest.mark.parametrize("e", [-60, -20, 17, 60])
@pytest.mark.parametrize("kind,Cin,Cout", RANGE_CASES)
def test_operand_range(kind, Cin, Cout, e):
    y, ref, keff, xmax = _range_case(kind, Cin, Cout, e)
    assert e != 17 or xmax > 65504.0          # beyond fp16's range
    check("bf16x3 %s Cin%d Cout%d x 2^%d" % (kind, Cin, Cout, e), y, ref, keff)


@pytest.mark.parametrize("kind,Cin,Cout", RANGE_CASES)
def test_one_activation_of_2_to_the_14_sigma(kind, Cin, Cout):
    y, ref, keff, xmax = _range_case(kind, Cin, Cout, 0, spike=True)
    assert xmax == 2.0 ** 14
    check("bf16x3 %s Cin%d Cout%d spike" % (kind, Cin, Cout), y, ref, keff)


# ---- 4. identities -----------------------------------------------------------------------------------------------------------------------
def _pair(precision, fn):
    """fn's outputs with the builders' calls at `precision` through the _prec entry points."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(OPS, "call", call_prec(precision))
        mp.setattr(MOPS, "call", call_prec(precision))
        return fn()


@pytest.mark.parametrize("Cin", [32, 25])
def test_precision_0_is_the_existing_entry_point_bit_for_bit(Cin):
    conv = lambda: OPS._conv(4500, 2, 17, 9, Cin, 40, 3, pro="small", act=1, slope=0.2, res="separate", out="both")[0]
    conv3 = lambda: MOPS._conv3d(4501, 2, 2, 6, 6, Cin, 24, 3, pool=1, act=1, slope=0.2)[0]
    for fn in (conv, conv3):
        via_prec = _pair(0, fn)
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(OPS, "call", _call)
            mp.setattr(MOPS, "call", _call)
            plain = fn()
        tier = fn()                                   # the fixture: precision 1
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(via_prec, plain))
        assert not any(torch.equal(a, b) for a, b in zip(tier, plain))          # ... and the tier is another kernel


def test_conv3d_depth_one_is_the_2d_conv_bit_for_bit():
    MOPS.test_conv3d_depth_one_is_the_2d_conv()          # both calls through the _prec entry points at precision 1 (the fixture)


def test_a_bad_precision_is_an_invalid_argument():
    lib = _lib.load()
    x, w, y = torch.zeros(1, 4, 4, 4, device=DEV), torch.zeros(4, 1, 1, 4, device=DEV), torch.full((1, 4, 4, 4), 7.0, device=DEV)
    P = _lib.ptr
    for bad in (2, -1):
        rc = lib.r3d_torso_conv_prec(P(x), 1, 4, 4, 4, 0, 0, None, None, 0.0, P(w), None, 4, 1, 0, 0.0, None, P(y), None, bad, _lib.stream_ptr())
        assert rc == -1 and b"precision %d" % bad in lib.r3d_last_error()
        rc = lib.r3d_torso_conv3d_prec(P(x), 1, 1, 4, 4, 4, 0, P(w), None, 4, 1, 0, 0, 0.0, 0, P(y), 4, 0, None, bad, _lib.stream_ptr())
        assert rc == -1 and b"precision %d" % bad in lib.r3d_last_error()
    torch.cuda.synchronize()
    assert float(y.min()) == 7.0 == float(y.max())          # nothing was launched
