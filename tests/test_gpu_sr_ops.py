"""GPU: the small kernels around the SR convolutions -- format conversion, resampling, blending, the fp16 range fold and the plane layout
pass (include/r3d_hip.h; csrc/r3d_sr.hip, r3d_sr_f16x3.hip, r3d_api.hip, r3d_render.hip) -- called directly, as the Python operators call
them, and compared with a float64 torch statement of the same operation at the sizes where addressing goes wrong: 1-pixel images, extents of 1,
ragged blocks, channel groups that straddle a concatenation, every code path of the reductions.

Floating-point results follow the one error rule of tests/test_gpu_torso_ops.py (check); layout-only results are torch.equal.  What a producer
of the SPLIT / SPLIT_MX activation format writes is decoded and held to the format's contract by tests/sr_formats.py (check_split), for all
five producers: the blend/concatenation, the bilinear up-sampling, the conv epilogues, the SR block's epilogue and (through them) the input
conversion.  The range fold is tested as properties: a bound bounds, a multiplier puts the bound in the top binade, nothing stored reaches 2^15.

Every output is a 16-byte-aligned window inside a larger allocation filled with a sentinel; the bytes on both sides must survive each call."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from real3dportrait_amd import _lib
from real3dportrait_amd.superresolution import Conv2d, SynthesisBlock, SynthesisBlockNoUp, chain_fold
import sr_formats as SF
from test_gpu_torso_ops import check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NCHW, CB8, SPLIT, SPLIT_MX = 0, 1, 2, 3
FMT = {"nchw": NCHW, "cb8": CB8, "split": SPLIT, "split_mx": SPLIT_MX}
INVALID_ARG = -1
GUARD, SENT = 256, 0x5A


class Out:
    """An output window of `shape` x dtype, GUARD sentinel bytes on either side (and inside, until somebody writes)."""

    def __init__(self, shape, dtype=torch.float32, fill=None):
        self.nbytes = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
        self.raw = torch.full((GUARD + self.nbytes + GUARD,), SENT, dtype=torch.uint8, device=DEV)
        self.t = self.raw[GUARD:GUARD + self.nbytes].view(dtype).view(*shape)
        assert self.t.data_ptr() % 16 == 0 and self.t.is_contiguous()
        if fill is not None:
            self.t.fill_(fill)

    def intact(self):
        torch.cuda.synchronize()
        return bool((self.raw[:GUARD] == SENT).all()) and bool((self.raw[GUARD + self.nbytes:] == SENT).all())

    def cpu(self):
        assert self.intact(), "a kernel wrote outside its output"
        return self.t.cpu()


def call(name, *args):
    args = [_lib.ptr(a) if torch.is_tensor(a) else a for a in args]
    _lib.check(getattr(_lib.load(), "r3d_" + name)(*args, _lib.stream_ptr()), name)


def rc_of(name, *args):
    args = [_lib.ptr(a) if torch.is_tensor(a) else a for a in args]
    return getattr(_lib.load(), "r3d_" + name)(*args, _lib.stream_ptr())


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


def dev(t):
    return t.float().contiguous().to(DEV)


def to_cb8(x):
    N, C, H, W = x.shape
    return x.reshape(N, C // 8, 8, H, W).permute(0, 1, 3, 4, 2).contiguous()


def from_cb8(y):
    N, C8, H, W, _ = y.shape
    return y.permute(0, 1, 4, 2, 3).reshape(N, C8 * 8, H, W)


def pow2_scales(g, N, C, stride, lo=-6, hi=7):
    """[N, stride] per-channel powers of two that differ per sample (the tail of each row is never read: NaN)."""
    s = torch.full((N, stride), float("nan"))
    s[:, :C] = torch.exp2(torch.randint(lo, hi, (N, C), generator=g).float())
    return s


def mask_with_ends(g, N, H, W):
    """[N, 1, H, W] in [0, 1] with exact 0 and exact 1 among the interior values (where there is room for them)."""
    m = torch.rand(N, 1, H, W, generator=g)
    f = m.view(-1)
    if f.numel() >= 3:
        f[0::4] = 0.0
        f[1::4] = 1.0
    return m


def absmax(x, N):
    """r3d_absmax into a fresh zeroed slot: device float[N] view."""
    out = Out((N,), fill=0.0)
    call("absmax", x, x.numel() // N, N, out.t, None)
    assert out.intact()
    return out.t


# ---- 2a. r3d_upsample2x_bilinear ------------------------------------------------------------------------------------------------------------
def _upsample(xd, N, C, H, W, fmt, ns=None, stride=0):
    y = Out((N, C // 8, 2 * H, 2 * W, 8)) if fmt == CB8 else Out((N, 2, C // 8, 2 * H, 2 * W, 8), torch.float16)
    call("upsample2x_bilinear", xd, N, C, H, W, y.t, fmt, ns, stride)
    return y


@pytest.mark.parametrize("N,C,H,W", SF.UPSAMPLE_SHAPES)
def test_upsample2x_bilinear(N, C, H, W):
    g = gen(100 + C + H + W)
    x = randn(g, N, C, H, W)
    xd = dev(to_cb8(x))
    what = "upsample2x N%d C%d %dx%d" % (N, C, H, W)
    y = _upsample(xd, N, C, H, W, CB8)
    ycb = from_cb8(y.cpu())
    check(what + " cb8", ycb, SF.upsample_ref(x), 4)
    assert torch.equal(ycb[:, :, 0, 0], x[:, :, 0, 0]) and torch.equal(ycb[:, :, -1, -1], x[:, :, -1, -1]), what + ": corners"
    stride = C + 5
    variants = [("none", None, False), ("pow2", pow2_scales(g, N, C, stride, -10, 12), True)]
    if (H, W) in ((5, 9), (33, 17)):
        s = torch.full((N, stride), float("nan"))
        s[:, :C] = torch.rand(N, C, generator=g) * 1.5 + 0.5                  # not powers of two: contract bounds only
        variants.append(("any", s, False))
    for name, ns, exact in variants:
        nsd = dev(ns) if ns is not None else None
        t64 = ycb.double() * (ns[:, :C, None, None].double() if ns is not None else 1.0)
        for fmt in (SPLIT, SPLIT_MX):
            if fmt == SPLIT_MX and C % 16:
                continue
            ys = _upsample(xd, N, C, H, W, fmt, nsd, stride if ns is not None else 0)
            SF.check_split(ys.cpu(), t64, mx=fmt == SPLIT_MX, exact_lo=exact or ns is None, what="%s %s scale %s" % (what, "split_mx" if fmt == SPLIT_MX else "split", name))


def test_upsample2x_bilinear_refuses_half_a_record_group():
    xd = torch.zeros(1, 3, 5, 9, 8, device=DEV)
    y = Out((1, 2, 3, 10, 18, 8), torch.float16)
    assert rc_of("upsample2x_bilinear", xd, 1, 24, 5, 9, y.t, SPLIT_MX, None, 0) == INVALID_ARG
    assert b"SPLIT_MX" in _lib.load().r3d_last_error()
    assert y.intact() and bool((y.t.view(torch.uint8) == SENT).all())


# ---- 2b. r3d_blend_cat_to_split -------------------------------------------------------------------------------------------------------------
def _blend_cat_inputs(g, N, Ca, Cb, H, W):
    a = randn(g, N, Ca, H, W) * torch.exp2(torch.randint(-3, 6, (N, Ca, 1, 1), generator=g).float())
    b = randn(g, N, Cb, H, W) * torch.exp2(torch.randint(-3, 6, (N, Cb, 1, 1), generator=g).float())
    return a, b, mask_with_ends(g, N, H, W)


@pytest.mark.parametrize("mx", [False, True])
@pytest.mark.parametrize("N,Ca,Cb,H,W,fa,fb", SF.BLEND_CAT_CASES)
def test_blend_cat_to_split(N, Ca, Cb, H, W, fa, fb, mx):
    g = gen(200 + Ca + Cb + H + W)
    a, b, m = _blend_cat_inputs(g, N, Ca, Cb, H, W)
    C = Ca + Cb
    stride = C + 3
    ns = pow2_scales(g, N, C, stride)
    t = torch.cat([a * m, b * (1.0 - m)], dim=1) * ns[:, :C, None, None]              # (v sc) ns in fp32, as the kernel: exact t
    assert t.dtype == torch.float32
    y = Out((N, 2, C // 8, H, W, 8), torch.float16)
    call("blend_cat_to_split", dev(to_cb8(a) if fa == "cb8" else a), FMT[fa], Ca, dev(to_cb8(b) if fb == "cb8" else b), FMT[fb], Cb, dev(m),
         N, H, W, y.t, SPLIT_MX if mx else SPLIT, dev(ns), stride)
    SF.check_split(y.cpu(), t.double(), mx=mx, exact_lo=True, what="blend_cat N%d %d+%d %dx%d %s/%s mx%d" % (N, Ca, Cb, H, W, fa, fb, mx))


@pytest.mark.parametrize("mx", [False, True])
def test_blend_cat_to_split_without_b_leaves_its_part_alone(mx):
    N, Ca, Cb, H, W = 2, 16, 16, 5, 3
    g = gen(230)
    a, _, m = _blend_cat_inputs(g, N, Ca, Cb, H, W)
    ns = pow2_scales(g, N, Ca + Cb, Ca + Cb)
    y = Out((N, 2, (Ca + Cb) // 8, H, W, 8), torch.float16)
    call("blend_cat_to_split", dev(to_cb8(a)), CB8, Ca, None, NCHW, Cb, dev(m), N, H, W, y.t, SPLIT_MX if mx else SPLIT, dev(ns), Ca + Cb)
    yc = y.cpu()
    SF.check_split(yc[:, :, :Ca // 8].contiguous(), ((a * m) * ns[:, :Ca, None, None]).double(), mx=mx, exact_lo=True, what="blend_cat b=NULL, a part, mx%d" % mx)
    assert bool((yc[:, :, Ca // 8:].contiguous().view(torch.uint8) == SENT).all()), "the b part (hi chunks and lo chunks / records) was written"


# ---- 2c. r3d_resize_bilinear ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("antialias", [0, 1])
@pytest.mark.parametrize("planes,H,W,OH,OW", SF.RESIZE_SHAPES)
def test_resize_bilinear(planes, H, W, OH, OW, antialias):
    x = randn(gen(300 + H + W + OH), 1, planes, H, W)
    y = Out((1, planes, OH, OW))
    call("resize_bilinear", dev(x), planes, H, W, y.t, OH, OW, antialias)
    what = "resize %d planes %dx%d -> %dx%d aa%d" % (planes, H, W, OH, OW, antialias)
    got = y.cpu()
    check(what, got, SF.resize_ref(x, OH, OW, antialias), SF.resize_keff(H, W, OH, OW))
    if (H, W) == (OH, OW):
        assert torch.equal(got, x), what + ": the identity"


# ---- 2d. r3d_blend, r3d_person_occlusion ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,C,H,W", [(1, 1, 1, 1), (2, 3, 7, 9), (3, 5, 17, 16)])
def test_blend(N, C, H, W):
    g = gen(400 + C + H)
    a, b, m = randn(g, N, C, H, W), randn(g, N, C, H, W), mask_with_ends(g, N, H, W)
    y = Out((N, C, H, W))
    call("blend", dev(a), dev(b), dev(m), N, C, H, W, y.t)
    check("blend N%d C%d %dx%d" % (N, C, H, W), y.cpu(), lambda dt: a.to(dt) * m.to(dt) + b.to(dt) * (1.0 - m.to(dt)), 2)


@pytest.mark.parametrize("count", [1, 255, 257, 1000])
def test_person_occlusion(count):
    g = gen(450 + count)
    thr = torch.tensor(0.6, dtype=torch.float32)
    inf = torch.tensor(float("inf"))
    special = torch.stack([thr, torch.nextafter(thr, inf), torch.nextafter(thr, -inf), torch.tensor(0.0), torch.tensor(1.0)])
    alpha = torch.rand(count, generator=g)
    alpha[:min(count, 5)] = special[:min(count, 5)]
    if count > 10:
        alpha[-5:] = special
    occ = randn(g, count) * 0.8                                        # sums below 0 and above 1 on both branches
    if count > 10:
        occ[:5] = torch.tensor([0.0, 0.0, 0.0, -0.5, 0.5])
    y = Out((count,))
    call("person_occlusion", dev(alpha), dev(occ), float(thr), count, y.t)
    ref = (occ + torch.where(alpha > thr, torch.ones_like(alpha), alpha)).clamp(0.0, 1.0)
    assert ref.dtype == torch.float32 and torch.equal(y.cpu(), ref)
    if count > 10:
        assert float(ref.min()) == 0.0 and float(ref.max()) == 1.0 and bool(((ref > 0) & (ref < 1)).any())


# ---- 2e. r3d_absmax -------------------------------------------------------------------------------------------------------------------------
ABSMAX_BIG = 4 * (4 * 512 * 256) + 4            # one 16-byte vector past the 4x-unrolled loop of a grid capped at 512 blocks


@pytest.mark.parametrize("count,N", [(1, 1), (3, 2), (4, 3), (255, 2), (1024, 1), (1030, 3), (ABSMAX_BIG, 2)])
def test_absmax(count, N):
    """1, 3, 255, 1030: the scalar path (1030 with samples 1 and 2 off 16-byte alignment); 4, 1024: the vector remainder loop; the last: the
    unrolled loop and one vector of remainder."""
    g = gen(500 + count % 1000)
    base = randn(g, N, count)
    for where in ("first", "last", "negative"):
        x = base.clone()
        for n in range(N):
            i = 0 if where == "first" else count - 1 if where == "last" else (count // 2 + n) % count
            x[n, i] = (-1.0 if where == "negative" else 1.0) * (100.0 + n)
        out, nxt = Out((N,), fill=0.0), Out((N,), fill=7.0)
        call("absmax", dev(x), count, N, out.t, nxt.t)
        assert torch.equal(out.cpu(), x.abs().amax(dim=1)), (count, N, where)
        assert torch.equal(nxt.cpu(), torch.zeros(N)), (count, N, where)
    out = Out((N,), fill=0.0)
    call("absmax", dev(base), count, N, out.t, None)                 # (no planted value: the maximum sits anywhere)
    assert torch.equal(out.cpu(), base.abs().amax(dim=1))


@pytest.mark.parametrize("count", [3, 1024, 1030, 4096 + 4])
def test_absmax_all_zero_sample(count):
    x = randn(gen(560 + count), 3, count)
    x[1] = 0.0
    x[2, ::2] = -0.0
    out, nxt = Out((3,), fill=0.0), Out((3,), fill=-3.0)
    call("absmax", dev(x), count, 3, out.t, nxt.t)
    got = out.cpu()
    assert torch.equal(got, x.abs().amax(dim=1)) and float(got[1]) == 0.0
    assert torch.equal(nxt.cpu(), torch.zeros(3))


# ---- layers for 2f / 2g: the wrappers hold parameters, packs and folded scales; the forward entry points are called here ----------------------
def make_conv(g, Cin, Cout, k, bias_scale=0.1):
    c = Conv2d(Cin, Cout, k, 1, padding=k // 2)
    with torch.no_grad():
        c.weight.copy_(randn(g, Cout, Cin, k, k, scale=(Cin * k * k) ** -0.5))
        c.bias.copy_(randn(g, Cout, scale=bias_scale))
    c = c.to(DEV)
    c.precision = "f16x3"
    return c


def conv_ref(c, x, slope, dt=torch.float64):
    y = F.conv2d(x.to(dt), c.weight.detach().cpu().to(dt), c.bias.detach().cpu().to(dt), padding=c.kernel_size[0] // 2)
    return y if slope is None else F.leaky_relu(y, slope)


def conv_run(c, x, x_fmt, N, H, W, slope, y_fmt, nxt=None, y_absmax=None):
    """r3d_conv_forward of the (prepared, folded) layer c into a guarded window; nxt: the folded consumer of a SPLIT / SPLIT_MX output; y_absmax: a zeroed
    device float[N] the epilogue maxes |y| into."""
    lib = _lib.load()
    Cin, Cout, k = c.in_channels, c.out_channels, c.kernel_size[0]
    need = int(lib.r3d_conv_workspace_bytes(N, Cin, H, W))
    work = c._buf("_workspace", need, x.device) if x_fmt < SPLIT else None
    ns, stride = nxt.in_scale() if nxt is not None else (None, 0)
    if y_fmt >= SPLIT:
        y = Out((N, 2, Cout // 8, H, W, 8), torch.float16)
    else:
        y = Out((N, Cout // 8, H, W, 8) if y_fmt == CB8 else (N, Cout, H, W))
    call("conv_forward", c._prepacked, c._scales, c._bias32, N, Cin, Cout, H, W, k, x, x_fmt, 0 if slope is None else 1, float(slope or 0.0), 1.0, -1.0,
         y.t, y_fmt, ns, stride, y_absmax, work, need if work is not None else 0)
    return y


def make_block(g, Cin, Cout, up, clamp=None, precision="f16x3"):
    """(module on the device, its parameters as numpy for the float64 restatement)."""
    def layer(ci, co, k):
        return (randn(g, co, ci, k, k).numpy(), randn(g, co, scale=0.1).numpy(), randn(g, ci, 512).numpy(), (1.0 + randn(g, ci, scale=0.05)).numpy())
    p = {"conv0": layer(Cin, Cout, 3), "conv1": layer(Cout, Cout, 3), "torgb": layer(Cout, 3, 1)}
    blk = (SynthesisBlock if up else SynthesisBlockNoUp)(Cin, Cout, w_dim=512, resolution=64, img_channels=3, is_last=False, conv_clamp=clamp)
    with torch.no_grad():
        for name in ("conv0", "conv1", "torgb"):
            layer_, (w, b, aw, ab) = getattr(blk, name), p[name]
            layer_.weight.copy_(torch.from_numpy(w)); layer_.bias.copy_(torch.from_numpy(b))
            layer_.affine.weight.copy_(torch.from_numpy(aw)); layer_.affine.bias.copy_(torch.from_numpy(ab))
    blk = blk.to(DEV)
    blk.precision = precision
    return blk, p


def block_run(blk, prep, x, x_fmt, img, N, Hin, Win, out_fmt, nxt=None, x_absmax=None):
    """r3d_sr_block_forward of the (prepared, folded) block into guarded windows: (x_out, img_out); x_absmax: a zeroed device float[N] conv1's epilogue
    maxes |x_out| into."""
    lib = _lib.load()
    Cin, Cout = blk.in_channels, blk.out_channels
    need = int(lib.r3d_sr_block_workspace_bytes(N, Cin, Cout, Hin, Win))
    work = blk._buf("_workspace", need, x.device)
    OH, OW = (2 * Hin, 2 * Win) if blk._UP else (Hin, Win)
    ns, stride = nxt.in_scale() if nxt is not None else (None, 0)
    x_out = Out((N, 2, Cout // 8, OH, OW, 8), torch.float16) if out_fmt >= SPLIT else Out((N, Cout, OH, OW))
    img_out = Out((N, 3, OH, OW))
    call("sr_block_forward", prep[0], prep[1], N, Cin, Cout, Hin, Win, blk._UP, x, x_fmt, img, blk._clamp(), x_out.t, out_fmt, ns, stride,
         img_out.t, None, x_absmax, blk._prec(), work, need)
    return x_out, img_out


def in_multiplier(c, N):
    """The folded in-multiplier vector of a conv layer, [N, padded Cin] on the CPU."""
    v, stride = c.in_scale()
    torch.cuda.synchronize()
    cin_padded = (c.in_channels + 15) // 16 * 16
    return v[:N * stride].view(N, stride)[:, :cin_padded].cpu()


def check_in_multiplier(what, c, B):
    """(ii): one power of two 2^e per sample with 2^14 <= B 2^e < 2^15, e = 15 for B = 0.  B: float[N] on the CPU."""
    m = in_multiplier(c, len(B))
    for n in range(len(B)):
        v = float(m[n, 0])
        assert bool((m[n] == v).all()) and math.isfinite(v) and v > 0.0 and math.frexp(v)[0] == 0.5, (what, n, m[n])
        stored = float(B[n]) * v
        print("fold %s n%d: bound in %.4e multiplier 2^%d stored bound %.1f" % (what, n, float(B[n]), math.frexp(v)[1] - 1, stored))
        if float(B[n]) == 0.0:
            assert v == 2.0 ** 15, (what, n, v)
        else:
            assert 2.0 ** 14 <= stored < 2.0 ** 15, (what, n, float(B[n]), v)


def check_bound(what, bound, y_dev, y64):
    """(i): bound[n] >= max|y[n]| for the device's y and for its float64 evaluation; prints the slack."""
    torch.cuda.synchronize()
    bound = bound.cpu().double()
    for n in range(bound.numel()):
        md, m64 = float(y_dev[n].abs().max()), float(y64[n].abs().max())
        print("fold slack %s n%d: bound %.4e max|y| %.4e (float64 %.4e) slack x%.1f" % (what, n, float(bound[n]), md, m64, float(bound[n]) / max(md, 1e-300)))
        assert math.isfinite(float(bound[n])) and float(bound[n]) >= md and float(bound[n]) >= m64, (what, n, float(bound[n]), md, m64)


def check_stored(what, ys):
    """(iii): every stored hi of a SPLIT / SPLIT_MX tensor is below 2^15 (and something was stored)."""
    hi = ys.cpu()[:, 0].float().abs()
    assert bool(torch.isfinite(hi).all()) and 0.0 < float(hi.max()) < 2.0 ** 15, (what, float(hi.max()))
    print("fold stored %s: max|hi| %.1f" % (what, float(hi.max())))


# ---- 2f. r3d_chain_fold ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [-20, 0, 14])
def test_chain_fold_three_convs(k):
    N, H, W = 2, 13, 11
    g = gen(600 + k)
    convs = [make_conv(g, 48, 128, 3), make_conv(g, 128, 64, 1), make_conv(g, 64, 32, 3)]
    slopes = [0.2, None, None]
    x = randn(g, N, 48, H, W) * 2.0 ** k
    x[1] *= 2.0 ** -7
    xd = dev(x)
    for c in convs:
        c.prepare(N, xd.device)
    bx = absmax(xd, N)
    assert torch.equal(bx.cpu(), x.abs().amax(dim=(1, 2, 3)))
    chain_fold([convs[0].chain_op(-1, negative_slope=0.2), convs[1].chain_op(0), convs[2].chain_op(1)], N, [bx])
    B, cur, cur64, split = bx.cpu(), xd, x.double(), None
    for j, (c, slope) in enumerate(zip(convs, slopes)):
        what = "3 convs 2^%d op%d" % (k, j)
        check_in_multiplier(what, c, B)
        y = conv_run(c, cur, NCHW, N, H, W, slope, NCHW)
        cur64 = conv_ref(c, cur64, slope)
        bound = c.bound_out(N)
        check_bound(what, bound, y.cpu(), cur64)
        if j + 1 < len(convs):           # the same layer's SPLIT output for its folded consumer, fed by the previous SPLIT tensor
            split = conv_run(c, cur if split is None else split.t, NCHW if split is None else SPLIT, N, H, W, slope, SPLIT, nxt=convs[j + 1])
            check_stored(what, split)
        else:
            ys = conv_run(c, split.t, SPLIT, N, H, W, slope, NCHW)
            e = float((ys.cpu().double() - cur64).abs().max() / cur64.abs().max())
            print("fold 3 convs 2^%d: SPLIT hand-offs end to end %.2e of max|ref|" % (k, e))
            assert e <= 2e-5, e          # (the fp32-class tier of tests/test_gpu_range_and_sizes.py test_conv_stack_range_sweep)
        B, cur = bound.cpu(), y.t


@pytest.mark.parametrize("up,clamp,tail", [(1, None, False), (0, None, False), (1, 0.75, False), (1, None, True)])
def test_chain_fold_two_blocks(up, clamp, tail):
    from test_gpu_range_and_sizes import _block_fp64
    N, H, W = 2, 9, 7
    g = gen(650 + up)
    b0, p0 = make_block(g, 32, 128, up, clamp)
    b1, p1 = make_block(g, 128, 128, up, clamp)
    x = randn(g, N, 32, H, W, scale=3.0)
    x[1] *= 2.0 ** -5
    img = randn(g, N, 3, H, W, scale=0.5)
    ws = 1.0 + randn(g, N, 3, 512, scale=0.2)
    xd, imgd, wsd = dev(x), dev(img), dev(ws)
    prep0, prep1 = b0.prepare(wsd, xd.device), b1.prepare(wsd, xd.device)
    bx = absmax(xd, N)
    chain_fold([b0.chain_op(-1), b1.chain_op(0)], N, [bx])
    what = "2 blocks up%d clamp %s%s" % (up, clamp, " tail" if tail else "")
    x0, img0 = block_run(b0, prep0, xd, NCHW, imgd, N, H, W, NCHW)
    r0, ri0 = _block_fp64(torch, p0, x, img, ws, up, clamp)
    bound0 = b0.bound_out(N)
    check_bound(what + " op0", bound0, x0.cpu(), r0)
    xs, _ = block_run(b0, prep0, xd, NCHW, imgd, N, H, W, SPLIT, nxt=b1)
    check_stored(what + " op0", xs)
    H1, W1 = (2 * H, 2 * W) if up else (H, W)
    bound1 = b1.bound_out(N)
    if tail:
        mx = absmax(x0.t, N)
        chain_fold([b1.chain_op(-1, tail=True)], N, [mx])
        tailb = b1.bound_out(N)
        torch.cuda.synchronize()
        print("fold %s: bound of op1 %s -> %s from the measured input maximum" % (what, bound1.cpu().tolist(), tailb.cpu().tolist()))
        assert bool((tailb <= bound1).all()) and bool((tailb > 0).all())
        bound1 = tailb
    x1, img1 = block_run(b1, prep1, x0.t, NCHW, img0.t, N, H1, W1, NCHW)
    r1, _ = _block_fp64(torch, p1, r0, ri0, ws, up, clamp)
    check_bound(what + " op1", bound1, x1.cpu(), r1)
    e = float((x1.cpu().double() - r1).abs().max() / r1.abs().max())
    print("fold %s: two blocks end to end %.2e of max|ref|" % (what, e))
    assert e <= 1e-5, e                  # (two blocks of test_sr_block_range_sweep's 4e-6 tier; a fold that broke the operands would be far outside)
    assert img0.intact() and img1.intact()
    if clamp is not None:
        torch.cuda.synchronize()
        assert float(bound0.max()) <= clamp and float(bound1.max()) <= clamp
        assert float(x0.t.abs().max()) <= clamp and float(x1.t.abs().max()) <= clamp


def test_chain_fold_two_sources_follow_the_larger():
    N, Ca, Cb, H, W = 2, 32, 32, 7, 5
    g = gen(700)
    a, b, m = randn(g, N, Ca, H, W), randn(g, N, Cb, H, W), mask_with_ends(g, N, H, W)
    a[0] *= 3.0; a[1] *= 0.01; b[0] *= 0.5; b[1] *= 8.0               # sample 0: a is the larger; sample 1: b
    c = make_conv(g, Ca + Cb, 32, 1)
    ad, bd = dev(a), dev(b)
    c.prepare(N, ad.device)
    ba, bb = absmax(ad, N), absmax(bd, N)
    chain_fold([c.chain_op(-1, -2)], N, [ba, bb])
    B = torch.maximum(a.abs().amax(dim=(1, 2, 3)), b.abs().amax(dim=(1, 2, 3)))
    check_in_multiplier("two sources", c, B)
    ns, stride = c.in_scale()
    ys = Out((N, 2, (Ca + Cb) // 8, H, W, 8), torch.float16)
    call("blend_cat_to_split", ad, NCHW, Ca, bd, NCHW, Cb, dev(m), N, H, W, ys.t, SPLIT, ns, stride)
    check_stored("two sources", ys)
    y = conv_run(c, ys.t, SPLIT, N, H, W, None, NCHW)
    check_bound("two sources", c.bound_out(N), y.cpu(), conv_ref(c, torch.cat([a.double() * m.double(), b.double() * (1.0 - m.double())], dim=1), None))


def test_chain_fold_reads_an_external_bound_before_it_clears_the_same_slot():
    N = 2
    g = gen(710)
    c = make_conv(g, 32, 32, 3)
    c.prepare(N, torch.device(DEV))
    slot = Out((N,))
    held = torch.tensor([5.0, 0.25])
    slot.t.copy_(held)
    other = Out((N,), fill=9.0)
    chain_fold([c.chain_op(-1)], N, [slot.t], zero=[slot.t, other.t])
    check_in_multiplier("ext bound that is also a zero slot", c, held)
    assert torch.equal(slot.cpu(), torch.zeros(N)) and torch.equal(other.cpu(), torch.zeros(N))


def test_chain_fold_zero_bound():
    N, H, W = 2, 5, 3
    g = gen(720)
    c, nxt = make_conv(g, 32, 32, 3, bias_scale=1.0), make_conv(g, 32, 16, 1)
    xd = torch.zeros(N, 32, H, W, device=DEV)
    c.prepare(N, xd.device); nxt.prepare(N, xd.device)
    zero = Out((N,), fill=0.0)
    chain_fold([c.chain_op(-1, negative_slope=0.2), nxt.chain_op(0)], N, [zero.t])
    check_in_multiplier("zero bound", c, torch.zeros(N))
    torch.cuda.synchronize()
    for layer in (c, nxt):
        v, stride = layer.in_scale()
        cin_p, cout_p = (layer.in_channels + 15) // 16 * 16, (layer.out_channels + 127) // 128 * 128
        assert bool(torch.isfinite(v[:N * stride].view(N, stride)[:, :cin_p + cout_p]).all())
    y = conv_run(c, xd, NCHW, N, H, W, 0.2, NCHW)
    act_bias = F.leaky_relu(c.bias.detach().cpu(), 0.2)
    assert torch.equal(y.cpu(), act_bias[None, :, None, None].expand(N, -1, H, W))
    check_bound("zero bound", c.bound_out(N), y.cpu(), conv_ref(c, torch.zeros(N, 32, H, W), 0.2))


# ---- 2g. SPLIT / SPLIT_MX from the conv and block epilogues -----------------------------------------------------------------------------------
def _consumer_scale(nxt, N, C):
    v, stride = nxt.in_scale()
    torch.cuda.synchronize()
    return v[:N * stride].view(N, stride)[:, :C].cpu().double()


@pytest.mark.parametrize("Cin,Cout,k", [(64, 48, 1), (32, 64, 3)])
def test_conv_epilogue_writes_the_split_formats(Cin, Cout, k):
    N, H, W = 2, 13, 11                  # partial 16 x 16 tiles in both directions
    g = gen(800 + Cout)
    c, nxt = make_conv(g, Cin, Cout, k), make_conv(g, Cout, 32, 3)
    x = randn(g, N, Cin, H, W, scale=2.0)
    x[1] *= 2.0 ** -4
    xd = dev(x)
    c.prepare(N, xd.device); nxt.prepare(N, xd.device)
    chain_fold([c.chain_op(-1, negative_slope=0.2), nxt.chain_op(0)], N, [absmax(xd, N)])
    y32 = conv_run(c, xd, NCHW, N, H, W, 0.2, NCHW).cpu()
    r = conv_ref(c, x, 0.2)
    e = float((y32.double() - r).abs().max() / r.abs().max())
    print("conv %d->%d k%d fp32 out: %.2e of max|ref|" % (Cin, Cout, k, e))
    assert e <= 2e-6, e                  # (the conv's own tier, test_conv2d_range_sweep: what the formats are checked against is the layer's output)
    t64 = y32.double() * _consumer_scale(nxt, N, Cout)[:, :, None, None]
    for fmt in (SPLIT, SPLIT_MX):
        ys = conv_run(c, xd, NCHW, N, H, W, 0.2, fmt, nxt=nxt)
        SF.check_split(ys.cpu(), t64, mx=fmt == SPLIT_MX, what="conv %d->%d k%d epilogue, format %d" % (Cin, Cout, k, fmt))
        check_stored("conv %d->%d k%d format %d" % (Cin, Cout, k, fmt), ys)


@pytest.mark.parametrize("fmt,precision", [(SPLIT, "f16x3"), (SPLIT_MX, "f16mx")])
def test_block_epilogue_writes_the_split_formats(fmt, precision):
    N, H, W = 2, 9, 7                    # 18 x 14 out: partial tiles
    g = gen(850)
    b0, _ = make_block(g, 32, 128, 1, precision=precision)
    b1, _ = make_block(g, 128, 128, 1, precision=precision)
    x, img, ws = randn(g, N, 32, H, W, scale=2.0), randn(g, N, 3, H, W, scale=0.5), 1.0 + randn(g, N, 3, 512, scale=0.2)
    xd, imgd, wsd = dev(x), dev(img), dev(ws)
    prep0 = b0.prepare(wsd, xd.device)
    b1.prepare(wsd, xd.device)
    chain_fold([b0.chain_op(-1), b1.chain_op(0)], N, [absmax(xd, N)])
    x32, img32 = block_run(b0, prep0, xd, NCHW, imgd, N, H, W, NCHW)
    xs, imgs = block_run(b0, prep0, xd, NCHW, imgd, N, H, W, fmt, nxt=b1)
    assert img32.intact() and imgs.intact()
    t64 = x32.cpu().double() * _consumer_scale(b1, N, 128)[:, :, None, None]
    SF.check_split(xs.cpu(), t64, mx=fmt == SPLIT_MX, what="SynthesisBlock(32->128) x_out format %d (%s)" % (fmt, precision))
    check_stored("SynthesisBlock(32->128) format %d" % fmt, xs)


# ---- 2h. r3d_planes_to_nhwc -----------------------------------------------------------------------------------------------------------------
PLANE_CASES = [(1, 32, 16, 16, 1, False, 0)]                                                     # the fast kernel, no add
PLANE_CASES += [(1, 32, 16, 16, 1, True, f) for f in (0, 1, 2, 3, 3 << 2, 3 << 4, 53)]           # 0: the fast kernel with the add; the rest: the general one
PLANE_CASES += [(1, 5, 7, 9, 1, False, 0), (1, 5, 7, 9, 1, True, 53), (1, 32, 8, 8, 3, True, 53), (1, 32, 8, 8, 3, False, 0),
                (2, 32, 16, 16, 1, True, 0), (2, 5, 7, 9, 1, True, 53), (2, 32, 8, 8, 3, True, 6)]


@pytest.mark.parametrize("N,C,H,W,D,add,flip", PLANE_CASES)
def test_planes_to_nhwc(N, C, H, W, D, add, flip):
    """The number of partials: the general kernel writes one per block of its (HW/32, C/32, 3 N D) grid, which is what r3d_planes_absmax_partials
    reports; the fast kernel (C = 32, HW % 64 == 0, no flips, no depth, 16-byte aligned) works on 64 pixels per block and writes HW/64 x 3 N of
    them, half of the reported size -- r3d_planes_absmax_partials is documented as the size of the buffer, *n_partials as what was written."""
    lib = _lib.load()
    g = gen(900 + C + H + D + flip)
    src = randn(g, N, 3, C * D, H, W)
    a = randn(g, N, 3, C * D, H, W) if add else None
    ref = src.clone()
    if add:
        for p in range(3):
            dims = [d for d, bit in ((2, 1), (3, 2)) if (flip >> (2 * p)) & bit]          # bit 2p: along H, bit 2p + 1: along W
            ref[:, p] += torch.flip(a[:, p], dims) if dims else a[:, p]
    ref = ref.view(N, 3, C, D, H, W).permute(0, 1, 3, 4, 5, 2).contiguous()
    size = int(lib.r3d_planes_absmax_partials(N, C, H, W, D))
    assert size == ((H * W + 31) // 32) * ((C + 31) // 32) * 3 * N * D
    out, part = Out((N, 3, D, H, W, C)), Out((size,))
    n = ctypes.c_int(-1)
    srcd, ad = dev(src), dev(a) if add else None          # (held: a temporary's memory would be handed to the next allocation)
    _lib.check(lib.r3d_planes_to_nhwc(_lib.ptr(srcd), _lib.ptr(ad), _lib.ptr(out.t), N, C, H, W, D, flip if add else 0,
                                      _lib.ptr(part.t), ctypes.byref(n), _lib.stream_ptr()), "planes_to_nhwc")
    got = out.cpu()
    assert torch.equal(got, ref)
    fast = C == 32 and D == 1 and (H * W) % 64 == 0 and (flip == 0 or not add)
    assert n.value == ((H * W // 64) * 3 * N if fast else size), (n.value, size, fast)
    pc = part.cpu()
    assert float(pc[:n.value].max()) == float(ref.abs().max())
    assert bool((pc[n.value:].view(torch.uint8) == SENT).all())
    out2 = Out((N, 3, D, H, W, C))           # without partials: the same bytes
    _lib.check(lib.r3d_planes_to_nhwc(_lib.ptr(srcd), _lib.ptr(ad), _lib.ptr(out2.t), N, C, H, W, D, flip if add else 0,
                                      None, None, _lib.stream_ptr()), "planes_to_nhwc")
    assert torch.equal(out2.cpu(), ref)
