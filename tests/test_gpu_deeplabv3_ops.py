"""GPU: each kernel of include/r3d_hip_deeplab.h at its edges, against the fp64 op on the CPU.  r3d_dl_conv and
r3d_dl_global_mean follow the rule of DESIGN 4.22: at most four times as far from fp64 as the same op in fp32 torch on the CPU (the kernel
sums in k-chunks of 4 and need not match torch's order; more than that is a bug, not rounding), and never more than 2e-4 of max|ref|.
r3d_dl_maxpool and r3d_dl_assemble_input match their torch operators bit for bit."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from real3dportrait_amd import _lib, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2e-4
SENTINEL = -12345.678


def unit(seed, shape, stream=0):
    return torch.from_numpy(synth.hash_unitvar(seed, shape, stream))


def cl(t):
    return t.permute(0, 2, 3, 1).contiguous()


def conv_inputs(B, H, W, Cin, Cout, k, seed):
    x = unit(seed, (B, Cin, H, W), 1)
    w = unit(seed, (Cout, Cin, k, k), 2) * float((2.0 / (Cin * k * k)) ** 0.5)
    return x, w


def out_size(n, k, s, d, p):
    return (n + 2 * p - d * (k - 1) - 1) // s + 1


def torch_conv(x, w, bias, s, d, p, res, act):
    """The op in x's dtype on the CPU: conv + bias[b] + residual, THEN ReLU.  bias [Cout] or [B, Cout]; res NCHW."""
    y = F.conv2d(x, w.to(x.dtype), None, s, p, d)
    if bias is not None:
        y = y + (bias.to(x.dtype).view(1, -1, 1, 1) if bias.dim() == 1 else bias.to(x.dtype)[:, :, None, None])
    if res is not None:
        y = y + res.to(x.dtype)
    return F.relu(y) if act else y


def hip_conv(x, w, bias, s, d, p, res=None, act=0, y=None, ycs=None, yco=0, in_place_res=False):
    """x, w, res NCHW on the CPU -> the [M, ycs] tensor the kernel wrote into (y when given; NaN-filled otherwise)."""
    B, Cin, H, W = x.shape
    Cout, k = w.shape[0], w.shape[2]
    M = B * out_size(H, k, s, d, p) * out_size(W, k, s, d, p)
    ycs = Cout if ycs is None else ycs
    if y is None:
        y = torch.full((M, ycs), float("nan"), device=DEV)
    r = None
    if res is not None:
        r = cl(res).to(DEV)
        if in_place_res:
            y = r.view(M, Cout)
            r = y
    b = None if bias is None else bias.contiguous().to(DEV)
    bs = 0 if bias is None or bias.dim() == 1 else bias.shape[1]
    _lib.call("r3d_dl_conv", cl(x).to(DEV), B, H, W, Cin, cl(w).to(DEV), b, bs, Cout, k, s, d, p, r, act, y, ycs, yco)
    return y


def check(out_cl, x, w, bias, s, d, p, res, act, tag):
    """out_cl [M, Cout] (CPU) by the rule; returns the fp64 reference channel-last."""
    ref = cl(torch_conv(x.double(), w, bias, s, d, p, res, act)).reshape(-1, w.shape[0])
    cpu32 = cl(torch_conv(x, w, bias, s, d, p, res, act)).reshape(-1, w.shape[0])
    assert out_cl.shape == ref.shape and bool(torch.isfinite(out_cl).all()), tag
    top = float(ref.abs().max())
    e_hip, e_cpu = float((out_cl.double() - ref).abs().max()) / top, float((cpu32.double() - ref).abs().max()) / top
    print("dl_conv %s: hip %.3g, fp32 torch on the CPU %.3g of max|ref|" % (tag, e_hip, e_cpu))
    assert e_hip <= TOL and e_hip <= 4.0 * e_cpu, (tag, e_hip, e_cpu)
    return ref


def test_conv_7x7_stride2_element_loader_bias_relu():
    """2 x 19 x 23 x 5 -> 64, 7 / 2 / 1 / 3: the stem's geometry at odd sizes; Cin = 5 takes the element loader."""
    x, w = conv_inputs(2, 19, 23, 5, 64, 7, 11)
    bias = unit(11, (64,), 3) * 0.3
    out = hip_conv(x, w, bias, 2, 1, 3, act=1).cpu()
    ref = check(out, x, w, bias, 2, 1, 3, None, 1, "7x7/2")
    assert 0.2 < float((ref > 0).double().mean()) < 0.8          # the ReLU acts


@pytest.mark.parametrize("B,H,W,Cin,Cout,k,s,d,p", [(1, 9, 11, 8, 72, 3, 2, 1, 1),          # strided 3 x 3, Cout over one 64-wide tile
                                                     (2, 9, 9, 12, 20, 1, 2, 1, 0),           # the strided 1 x 1 downsample (layer2)
                                                     (2, 9, 9, 12, 20, 1, 1, 2, 0),           # the dilated, padding-0 1 x 1 downsample (layer3)
                                                     (2, 1, 1, 512, 256, 1, 1, 1, 0),         # the pooled branch: a 1 x 1 image
                                                     (1, 6, 50, 4, 8, 3, 2, 4, 4)])           # stride and dilation together, W >> H
def test_conv_geometries(B, H, W, Cin, Cout, k, s, d, p):
    x, w = conv_inputs(B, H, W, Cin, Cout, k, 20 + Cin + k + s + d)
    out = hip_conv(x, w, None, s, d, p).cpu()
    check(out, x, w, None, s, d, p, None, 0, "%dx%dx%dx%d->%d %d/%d/%d/%d" % (B, H, W, Cin, Cout, k, s, d, p))


def test_conv_residual_is_y_and_goes_in_before_the_relu():
    """2 x 13 x 10 x 16 -> 40, 3 / 1 / 2 / 2 with residual == y and ReLU: BasicBlock's relu(sum + residual), not relu(sum) + residual."""
    x, w = conv_inputs(2, 13, 10, 16, 40, 3, 31)
    bias = unit(31, (40,), 3) * 0.2
    res = unit(31, (2, 40, 13, 10), 4) * 1.5
    out = hip_conv(x, w, bias, 1, 2, 2, res=res, act=1, in_place_res=True).cpu()
    ref = check(out, x, w, bias, 1, 2, 2, res, 1, "residual == y")
    other = cl(F.relu(torch_conv(x.double(), w, bias, 1, 2, 2, None, 0)) + res.double()).reshape(-1, 40)
    top = float(ref.abs().max())
    assert float((other - ref).abs().max()) > 0.1 * top          # the two orders differ on this input by far more than rounding
    assert float((out.double() - other).abs().max()) > 0.1 * top and float(out.min()) == 0.0
    # a residual of its own buffer gives the same bits
    sep = hip_conv(x, w, bias, 1, 2, 2, res=res, act=1).cpu()
    assert torch.equal(sep, out)


def test_conv_aspp_rates_write_their_slices():
    """1 x 40 x 37 x 8 -> 24, 3 / 1 / {12, 24, 36} / same into yco 0, 24, 48 of rows of 100 floats: columns 72 .. 99 keep the sentinel."""
    x, _ = conv_inputs(1, 40, 37, 8, 24, 3, 41)
    M = 40 * 37
    y = torch.full((M, 100), SENTINEL, device=DEV)
    ws = []
    for i, r in enumerate((12, 24, 36)):
        w = unit(41, (24, 8, 3, 3), 10 + i) * float((2.0 / 72) ** 0.5)
        ws.append(w)
        assert hip_conv(x, w, None, 1, r, r, act=1, y=y, ycs=100, yco=24 * i) is y
    out = y.cpu()
    assert torch.equal(out[:, 72:], torch.full((M, 28), SENTINEL))
    for i, r in enumerate((12, 24, 36)):
        ref = check(out[:, 24 * i:24 * i + 24].contiguous(), x, ws[i], None, 1, r, r, None, 1, "rate %d" % r)
        # at 40 x 37 every rate reaches real pixels: the result is not the centre tap's alone
        centre = cl(F.relu(F.conv2d(x.double(), ws[i][:, :, 1:2, 1:2].double()))).reshape(-1, 24)
        assert float((centre - ref).abs().max()) > 0.1 * float(ref.abs().max()), r


def test_conv_rate_36_on_8x8_is_the_centre_tap():
    """1 x 8 x 8 x 8 -> 16, 3 / 1 / 36 / 36: every tap but the centre falls in padding."""
    x, w = conv_inputs(1, 8, 8, 8, 16, 3, 51)
    out = hip_conv(x, w, None, 1, 36, 36).cpu()
    centre = w[:, :, 1:2, 1:2].contiguous()
    full, one = torch_conv(x.double(), w, None, 1, 36, 36, None, 0), F.conv2d(x.double(), centre.double())
    assert float((full - one).abs().max()) <= 1e-14 * float(one.abs().max())          # the other eight taps add exact zeros
    check(out, x, centre, None, 1, 1, 0, None, 0, "rate 36 on 8 x 8")


def test_conv_per_sample_bias_and_ragged_k():
    """3 x 5 x 5 x 36 -> 28, 1 / 1 / 1 / 0 with bias[b]: K = 36 is no multiple of the 32-wide k step."""
    x, w = conv_inputs(3, 5, 5, 36, 28, 1, 61)
    bias = unit(61, (3, 28), 3)
    out = hip_conv(x, w, bias, 1, 1, 0, act=1).cpu()
    check(out, x, w, bias, 1, 1, 0, None, 1, "per-sample bias")
    one = hip_conv(x, w, bias[1], 1, 1, 0, act=1).cpu()          # the same bias for all: sample 1 agrees, sample 0 does not
    assert torch.equal(one[25:50], out[25:50]) and not torch.equal(one[:25], out[:25])


@pytest.mark.parametrize("H,W", [(7, 9), (5, 13), (3, 43)])
@pytest.mark.parametrize("Cin,Cout", [(8, 33), (5, 65), (8, 16), (8, 17)])
def test_conv_tile_edges(H, W, Cin, Cout):
    """M = 63, 65, 129 rows and Cout = 33, 65 (and 16, 17: the 128 x 16 and 128 x 32 tiles) around the tile sizes, both loaders."""
    x, w = conv_inputs(1, H, W, Cin, Cout, 3, 70 + H + Cout)
    bias = unit(70, (Cout,), 3) * 0.1
    out = hip_conv(x, w, bias, 1, 1, 1, act=1).cpu()
    check(out, x, w, bias, 1, 1, 1, None, 1, "M %d Cout %d Cin %d" % (H * W, Cout, Cin))


@pytest.mark.parametrize("H", [31, 32])
def test_conv_tile_threshold(H):
    """2 x H x 32 x 4 -> 1024, 1 x 1: 496 tiles of 64 x 64 at H = 31 (the 32-row tile runs), 512 at H = 32 (the 64-row tile does)."""
    x, w = conv_inputs(2, H, 32, 4, 1024, 1, 80 + H)
    out = hip_conv(x, w, None, 1, 1, 0).cpu()
    check(out, x, w, None, 1, 1, 0, None, 0, "tile threshold, M %d" % (2 * H * 32))


def test_conv_sample_does_not_depend_on_batch_and_runs_agree():
    x, w = conv_inputs(2, 13, 10, 16, 40, 3, 91)
    bias = unit(91, (2, 40), 3)
    res = unit(91, (2, 40, 13, 10), 4)
    both = hip_conv(x, w, bias, 1, 2, 2, res=res, act=1).cpu()
    again = hip_conv(x, w, bias, 1, 2, 2, res=res, act=1).cpu()
    assert torch.equal(both, again)
    for b in range(2):
        alone = hip_conv(x[b:b + 1], w, bias[b:b + 1], 1, 2, 2, res=res[b:b + 1], act=1).cpu()
        assert torch.equal(alone, both[130 * b:130 * (b + 1)]), b
    # the element loader too
    x, w = conv_inputs(2, 9, 11, 5, 64, 7, 92)
    both = hip_conv(x, w, None, 2, 1, 3).cpu()
    assert torch.equal(both, hip_conv(x, w, None, 2, 1, 3).cpu())
    n = out_size(9, 7, 2, 1, 3) * out_size(11, 7, 2, 1, 3)
    for b in range(2):
        assert torch.equal(hip_conv(x[b:b + 1], w, None, 2, 1, 3).cpu(), both[n * b:n * (b + 1)]), b


def same_bits(a, b):
    """Equal, with NaN equal to NaN."""
    return a.shape == b.shape and bool(torch.equal(torch.isnan(a), torch.isnan(b))) and bool(torch.equal(torch.nan_to_num(a, 7.0), torch.nan_to_num(b, 7.0)))


@pytest.mark.parametrize("H,W", [(1, 1), (2, 2), (3, 3), (7, 5), (8, 6), (1, 9), (16, 1)])
def test_maxpool_is_torchs(H, W):
    B, C = 2, 5
    x = unit(100 + H + W, (B, C, H, W), 1)
    for name, t in (("random", x), ("all negative", -x.abs() - 1.0)):          # zero padding would win every border window of the second
        y = torch.full((B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C), float("nan"), device=DEV)
        _lib.call("r3d_dl_maxpool", cl(t).to(DEV), B, H, W, C, y)
        want = cl(F.max_pool2d(t, 3, 2, 1))
        assert torch.equal(y.cpu(), want), name
    if H * W > 1:
        t = x.clone()
        t[1, 2, H // 2, W // 2] = float("nan")
        y = torch.zeros(B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C, device=DEV)
        _lib.call("r3d_dl_maxpool", cl(t).to(DEV), B, H, W, C, y)
        want = cl(F.max_pool2d(t, 3, 2, 1))
        assert bool(torch.isnan(want).any()) and same_bits(y.cpu(), want)


@pytest.mark.parametrize("B,HW,C", [(2, 35, 24), (1, 1, 70), (3, 1600, 65), (1, 4099, 512)])
def test_global_mean(B, HW, C):
    x = unit(110 + HW, (B, HW, C), 1) + 0.5
    y = torch.full((B, C), float("nan"), device=DEV)
    _lib.call("r3d_dl_global_mean", x.to(DEV), B, HW, C, y)
    ref, cpu32 = x.double().mean(1), x.mean(1)
    top = float(ref.abs().max())
    e_hip, e_cpu = float((y.cpu().double() - ref).abs().max()) / top, float((cpu32.double() - ref).abs().max()) / top
    print("dl_global_mean %dx%dx%d: hip %.3g, fp32 torch on the CPU %.3g of max|ref|" % (B, HW, C, e_hip, e_cpu))
    assert e_hip <= TOL and e_hip <= 4.0 * e_cpu
    y2 = torch.empty(B, C, device=DEV)
    _lib.call("r3d_dl_global_mean", x.to(DEV), B, HW, C, y2)
    assert torch.equal(y, y2)
    one = torch.empty(1, C, device=DEV)
    _lib.call("r3d_dl_global_mean", x[B - 1:].contiguous().to(DEV), 1, HW, C, one)
    assert torch.equal(one[0], y[B - 1])


@pytest.mark.parametrize("mode", ["rgb", "rgb_alpha", "rgb_camera", "rgb_alpha_camera"])
@pytest.mark.parametrize("H,W", [(7, 7), (16, 16), (6, 10)])
def test_assemble_input_is_the_references_cat(mode, H, W):
    """Against the cats of img2plane_model.py:52-64 as torch evaluates them on the CPU, bit for bit; both grids divide by H."""
    B = 2
    img = unit(120 + H, (B, 3, H, W), 1)
    alpha = (unit(120 + H, (B, 1, H, W), 2) > 0).float() if "alpha" in mode else None
    cam = unit(120 + H, (B, 3), 3) if "camera" in mode else None
    parts = [img] + ([alpha] if alpha is not None else []) + ([cam.reshape(B, 3, 1, 1).repeat([1, 1, H, W])] if cam is not None else [])
    grid_x, grid_y = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    grid_x, grid_y = grid_x / H, grid_y / H
    parts += [grid_x[None, None].repeat(B, 1, 1, 1), grid_y[None, None].repeat(B, 1, 1, 1)]
    want = cl(torch.cat(parts, dim=1))
    y = torch.full(tuple(want.shape), float("nan"), device=DEV)
    dev = lambda t: None if t is None else t.contiguous().to(DEV)
    _lib.call("r3d_dl_assemble_input", dev(img), dev(alpha), dev(cam), B, H, W, y)
    assert torch.equal(y.cpu(), want)
