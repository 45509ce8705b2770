"""GPU: every kernel variant behind the SR conv entry points (csrc/r3d_sr_f16x3.hip; the table of DESIGN 4.2g) at ragged edges, by name.

Which kernel a call runs is decided by its shape, batch and input format.  Every case here is a row of tests/sr_variant_cases.py and first asserts,
through r3d_debug_conv_variant / r3d_debug_sr_block_variants (what the launchers dispatch on), that it reaches the variant, block order and grid it is
named after; tests/test_sr_conv_variant_host.py holds the same table to the rules without a GPU.  Every output is a sentinel-guarded window
(tests/test_gpu_sr_ops.py Out): a tile that is never written keeps the sentinel, 1.5e16, and fails the comparison.

 (a) against float64, per variant: seeded CPU inputs, a batch whose samples differ in magnitude (so the per-sample folds differ), weight rows of
     different magnitude, LeakyReLU on and off, bias present and NULL, every input format a variant accepts (SPLIT / SPLIT_MX operands are written from
     Python by tests/sr_formats.py).  The error is taken three times -- whole tensor, the image's border rows and columns, the pixels of partial tiles
     -- each against max|ref| of the sample, and held to the tier the suite already has: 2e-6 (f16x3) / MX_TOL (f16mx) for a conv layer, 4e-6 / 1e-4
     for a block.  A case that missed its tier would be allowed max(tier, 4 e32), e32 the same statement in fp32 torch on the CPU (the one error rule of
     tests/test_gpu_torso_ops.py check) and say so in its printed line; none needs it.
 (b) exact relations (torch.equal): the 16-row kernel == the 8-row kernel on the same sample; a ragged image == the same image at the origin of a
     larger zero canvas, for every direct 3x3 variant and for the up-sampling conv; CB8 == NCHW and the decoded SPLIT / SPLIT_MX outputs == the same
     values times the consumer's multiplier (sr_formats.check_split)."""
import functools
import os
import subprocess
import sys
import zlib

import pytest
import torch

from real3dportrait_amd import _lib
from real3dportrait_amd.superresolution import chain_fold
import sr_formats as SF
import sr_variant_cases as V
from test_gpu_mx import MX_TOL
from test_gpu_range_and_sizes import _block_fp64
from test_gpu_sr_ops import (CB8, DEV, NCHW, SPLIT, SPLIT_MX, Out, _consumer_scale, absmax, block_run, call, check_stored, conv_ref, conv_run, dev, from_cb8,
                             gen, in_multiplier, make_block, make_conv, mask_with_ends, randn, to_cb8)
from test_sr_conv_variant_host import block_variants, conv_variant

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONV_TIER = {False: 2e-6, True: MX_TOL}          # test_conv2d_range_sweep | tests/test_gpu_mx.py
BLOCK_TIER = {False: 4e-6, True: 1e-4}           # test_sr_block_range_sweep | test_sr_block_range_sweep_f16mx
TILE = {V.D16: (16, 16), V.D16_MX: (16, 16), V.R8: (8, 16), V.R8_MX: (8, 16), V.WINO: (16, 16), V.WINO_MX: (16, 16), V.C1X1: (16, 16), V.BLEND: (16, 16),
        V.UPCONV: (28, 28)}                      # output pixels of one block's tile (the up-sampling conv: 14 x 14 inputs)


def seed_of(name):
    return zlib.crc32(name.encode()) & 0x7FFFFFFF


def named(case):
    return case.name.replace(" ", "_")


def describe(rec):
    return "%s order %d grid %s" % (V.name_of(rec), rec[2], "x".join(str(v) for v in rec[3]))


# ---- error of a result against float64 ------------------------------------------------------------------------------------------------------
def regions(H, W, tiles):
    """(border, partial): the image's first / last rows and columns; the pixels of tiles that are not whole, for each (rows, cols) tile shape."""
    border = torch.zeros(H, W, dtype=torch.bool)
    border[0] = border[-1] = True
    border[:, 0] = border[:, -1] = True
    partial = torch.zeros(H, W, dtype=torch.bool)
    for th, tw in tiles:
        partial[(H // th) * th:] = True
        partial[:, (W // tw) * tw:] = True
    return border, partial


def hold(what, y, ref, tier, tiles, ref32=None):
    """Per sample: max|y - ref| over the whole tensor, the border and the partial tiles, each over max|ref| of the sample, printed and held to the tier
    (max(tier, 4 e32) if it were missed and ref32 is given).  Returns the worst."""
    N, _, H, W = ref.shape
    border, partial = regions(H, W, tiles)
    worst = 0.0
    for n in range(N):
        m = float(ref[n].abs().max())
        assert m > 0.0, what
        d = (y[n].double() - ref[n]).abs()
        e = (float(d.max()) / m, float(d[:, border].max()) / m, float(d[:, partial].max()) / m if bool(partial.any()) else 0.0)
        bound, note = tier, ""
        if max(e) > tier and ref32 is not None:
            e32 = float((ref32()[n].double() - ref[n]).abs().max()) / m
            bound, note = max(tier, 4.0 * e32), " | tier missed: e32 %.2e, allowed max(tier, 4 e32) = %.2e" % (e32, max(tier, 4.0 * e32))
        print("variants %s n%d: whole %.2e border %.2e partial tiles (%d px) %.2e of max|ref| %.3e, tier %.0e%s" % (what, n, e[0], e[1], int(partial.sum()), e[2], m, tier, note))
        assert max(e) <= bound, (what, n, e, bound)
        worst = max(worst, max(e))
    return worst


# ---- a conv layer and its operand -------------------------------------------------------------------------------------------------------------
def layer(g, Cin, Cout, k, bias):
    """A HIP Conv2d whose weight rows differ in magnitude by up to 2^10.  bias False: the module keeps a zero bias (for conv_ref) and fold() takes it away
    from the entry points, which then get NULL."""
    c = make_conv(g, Cin, Cout, k, bias_scale=0.1 if bias else 0.0)
    with torch.no_grad():
        c.weight.mul_(torch.exp2(torch.randint(-6, 5, (Cout, 1, 1, 1), generator=g).float()).to(DEV))
    return c


def samples(g, N, C, H, W, distinct=None, scale=2.0):
    """[N, C, H, W]: sample 1 is 2^-5 of sample 0's magnitude; distinct = 2: sample n repeats base sample n % 2 (a large batch, two references)."""
    base = randn(g, distinct or N, C, H, W, scale=scale)
    if base.shape[0] > 1:
        base[1] *= 2.0 ** -5
    return base if distinct is None else base[torch.arange(N) % distinct].contiguous()


def fold(c, xd, N, slope, bias=True, nxt=None):
    """prepare + one r3d_chain_fold from the measured max|x| per sample (xd: fp32 on the device, any layout); nxt: a consumer folded in the same chain."""
    c.prepare(N, xd.device)
    if not bias:
        c._bias32 = None
    ops = [c.chain_op(-1, negative_slope=slope)]
    if nxt is not None:
        nxt.prepare(N, xd.device)
        ops.append(nxt.chain_op(0))
    chain_fold(ops, N, [absmax(xd, N)])


def operand(x, x_fmt, scale):
    """x [N, C, H, W] fp32 on the CPU as the entry point takes it in x_fmt; the SPLIT formats: times the consumer's folded in-multiplier `scale` [N, C]
    in fp32, as a producer would, and written from Python (sr_formats)."""
    if x_fmt == NCHW:
        return dev(x)
    if x_fmt == CB8:
        return dev(to_cb8(x))
    t = x.float() * scale.float()[:, :, None, None]
    return (SF.encode_split_mx_ref(t) if x_fmt == SPLIT_MX else SF.encode_split_ref(t)).contiguous().to(DEV)


def conv_operand(c, x, x_fmt, N):
    return operand(x, x_fmt, in_multiplier(c, N)[:, :c.in_channels] if x_fmt >= SPLIT else None)


def same_values(what, got, want):
    """torch.equal with the count of differing elements in the printed line and in the failure."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    n = int((got != want).sum())
    print("variants %s: %d of %d elements differ" % (what, n, got.numel()))
    assert n == 0 and torch.equal(got, want), "%s: %d of %d elements differ" % (what, n, got.numel())


# ---- (a) the 8-row kernels and the 1x1 kernel against float64 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", V.CONV_CASES, ids=named)
def test_conv_variant_vs_fp64(case):
    k = case
    assert conv_variant(k.N, k.Cin, k.Cout, k.H, k.W, k.k, k.x_fmt) == k.expect, k.name
    g = gen(seed_of(k.name))
    c = layer(g, k.Cin, k.Cout, k.k, k.bias)
    x = samples(g, k.N, k.Cin, k.H, k.W)
    fold(c, dev(x), k.N, k.slope, k.bias)
    xin = conv_operand(c, x, k.x_fmt, k.N)
    slot = Out((k.N,), fill=0.0)
    y = conv_run(c, xin, k.x_fmt, k.N, k.H, k.W, k.slope, NCHW, y_absmax=slot.t).cpu()
    what = "%s [%s]" % (k.name, describe(k.expect))
    hold(what, y, conv_ref(c, x, k.slope), CONV_TIER[k.x_fmt == SPLIT_MX], [TILE[k.expect[0]]], lambda: conv_ref(c, x, k.slope, torch.float32))
    same_values(what + " y_absmax == max|y| of the image", slot.cpu(), y.abs().amax(dim=(1, 2, 3)))
    if k.Cout % 8 == 0:
        same_values(what + " CB8 == NCHW", from_cb8(conv_run(c, xin, k.x_fmt, k.N, k.H, k.W, k.slope, CB8).cpu()), y)


# ---- (a) + (b) the 16-row kernels: a batch that crosses 256 blocks == the 8-row kernel on the same samples, and float64 for the two base samples ----
@pytest.mark.parametrize("case", V.BATCH_CASES, ids=named)
def test_rows16_equals_rows8_and_fp64(case):
    k = case
    assert conv_variant(k.N, k.Cin, k.Cout, k.H, k.W, 3, k.x_fmt) == k.expect and conv_variant(2, k.Cin, k.Cout, k.H, k.W, 3, k.x_fmt) == k.small, k.name
    g = gen(seed_of(k.name))
    c = layer(g, k.Cin, k.Cout, 3, k.bias)
    x = samples(g, k.N, k.Cin, k.H, k.W, distinct=2)
    fold(c, dev(x), k.N, k.slope, k.bias)
    xin = conv_operand(c, x, k.x_fmt, k.N)
    slot = Out((k.N,), fill=0.0)
    big = conv_run(c, xin, k.x_fmt, k.N, k.H, k.W, k.slope, NCHW, y_absmax=slot.t).cpu()
    small = conv_run(c, xin[:2], k.x_fmt, 2, k.H, k.W, k.slope, NCHW).cpu()          # (the first two samples' scales lead the folded buffer)
    what = "%s [%s]" % (k.name, describe(k.expect))
    same_values(what + " == [%s] per sample" % describe(k.small), big, small[torch.arange(k.N) % 2])
    mx = k.x_fmt == SPLIT_MX
    ref = conv_ref(c, x[:2], k.slope)
    ref32 = lambda: conv_ref(c, x[:2], k.slope, torch.float32)
    hold(what, big[:2], ref, CONV_TIER[mx], [TILE[k.expect[0]]], ref32)
    hold("%s (N = 2) [%s]" % (k.name, describe(k.small)), small, ref, CONV_TIER[mx], [TILE[k.small[0]]], ref32)
    same_values(what + " y_absmax == max|y| of the image", slot.cpu(), big.abs().amax(dim=(1, 2, 3)))


# ---- (b) ragged == zero-embedded ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", V.EMBED_CASES, ids=named)
def test_ragged_equals_zero_embedded_conv(case):
    """The H x W image and the same image at the origin of a zero canvas have the same per-sample bound, folds and K order per output: every output on
    [0, H) x [0, W) is the same bits.  What differs is what the kernel had to zero-fill itself: the out-of-image slots, the masked DMA lanes, the
    segments that lie wholly outside."""
    k = case
    CH, CW = k.canvas
    assert conv_variant(k.N, k.Cin, k.Cout, k.H, k.W, 3, k.x_fmt) == k.expect and conv_variant(k.N, k.Cin, k.Cout, CH, CW, 3, k.x_fmt) == k.expect_canvas, k.name
    assert k.expect[0] == k.expect_canvas[0]
    g = gen(seed_of(k.name))
    c = layer(g, k.Cin, k.Cout, 3, True)
    x = samples(g, k.N, k.Cin, k.H, k.W, distinct=2 if k.N > 2 else None)
    canvas = torch.zeros(k.N, k.Cin, CH, CW)
    canvas[:, :, :k.H, :k.W] = x
    xd, cd = dev(x), dev(canvas)
    assert torch.equal(absmax(xd, k.N).cpu(), absmax(cd, k.N).cpu())
    fold(c, xd, k.N, 0.2)
    xin, cin = conv_operand(c, x, k.x_fmt, k.N), conv_operand(c, canvas, k.x_fmt, k.N)
    y = conv_run(c, xin, k.x_fmt, k.N, k.H, k.W, 0.2, NCHW).cpu()
    yc = conv_run(c, cin, k.x_fmt, k.N, CH, CW, 0.2, NCHW).cpu()
    assert float(y.abs().max()) > 0.0 and bool(torch.isfinite(yc).all())
    same_values("%s [%s] == canvas %dx%d [%s] on the image" % (k.name, describe(k.expect), CH, CW, describe(k.expect_canvas)), y, yc[:, :, :k.H, :k.W])


# ---- (b) formats agree ------------------------------------------------------------------------------------------------------------------------------
def _formats_agree(what, run, y32, nxt, N, Cout):
    """run(y_fmt, nxt) -> Out: CB8 == NCHW bit for bit; SPLIT / SPLIT_MX decode to fp16(fp32 value x consumer multiplier) (check_split) and fit fp16."""
    same_values(what + " CB8 == NCHW", from_cb8(run(CB8, None).cpu()), y32)
    t64 = y32.double() * _consumer_scale(nxt, N, Cout)[:, :, None, None]
    for fmt in (SPLIT, SPLIT_MX):
        ys = run(fmt, nxt)
        SF.check_split(ys.cpu(), t64, mx=fmt == SPLIT_MX, what="%s format %d" % (what, fmt))
        check_stored("%s format %d" % (what, fmt), ys)
        print("variants %s: %s holds the format contract against the NCHW values" % (what, "SPLIT_MX" if fmt == SPLIT_MX else "SPLIT"))


@pytest.mark.parametrize("case", V.FORMAT_CASES, ids=named)
def test_output_formats_agree(case):
    """The wide 16-byte SPLIT stores of the 16-row kernels at partial tiles (the `inside` test at the store) as well as the narrow ones of the 8-row kernels."""
    k = case
    assert conv_variant(k.N, k.Cin, k.Cout, k.H, k.W, k.k, k.x_fmt) == k.expect, k.name
    g = gen(seed_of(k.name))
    c, nxt = layer(g, k.Cin, k.Cout, k.k, True), make_conv(g, k.Cout, 32, 3)
    x = samples(g, k.N, k.Cin, k.H, k.W, distinct=2 if k.N > 2 else None)
    fold(c, dev(x), k.N, k.slope, nxt=nxt)
    xin = conv_operand(c, x, k.x_fmt, k.N)
    what = "%s [%s]" % (k.name, describe(k.expect))
    y32 = conv_run(c, xin, k.x_fmt, k.N, k.H, k.W, k.slope, NCHW).cpu()
    if k.expect[0] not in (V.WINO, V.WINO_MX):         # (the Winograd kernel's own accuracy: tests/test_gpu_wino.py)
        mx = k.x_fmt == SPLIT_MX
        hold(what, y32[:2], conv_ref(c, x[:2], k.slope), CONV_TIER[mx], [TILE[k.expect[0]]], lambda: conv_ref(c, x[:2], k.slope, torch.float32))
    _formats_agree(what, lambda fmt, n: conv_run(c, xin, k.x_fmt, k.N, k.H, k.W, k.slope, fmt, nxt=n), y32, nxt, k.N, k.Cout)


def test_blend_conv_vs_fp64_and_formats():
    """conv1x1_blend_f16x3_kernel (r3d_conv_forward_blend) at a ragged size: float64, y_absmax, and its four output formats."""
    k = V.BLEND_CASE
    Ca, Cb = 24, 40
    assert Ca + Cb == k.Cin and conv_variant(k.N, k.Cin, k.Cout, k.H, k.W, 1, CB8, blend=1) == k.expect
    g = gen(seed_of(k.name))
    c, nxt = layer(g, k.Cin, k.Cout, 1, True), make_conv(g, k.Cout, 32, 3)
    a, b, m = samples(g, k.N, Ca, k.H, k.W), samples(g, k.N, Cb, k.H, k.W) * 3.0, mask_with_ends(g, k.N, k.H, k.W)
    ad, bd, md = dev(to_cb8(a)), dev(to_cb8(b)), dev(m)
    c.prepare(k.N, ad.device); nxt.prepare(k.N, ad.device)
    chain_fold([c.chain_op(-1, -2, negative_slope=k.slope), nxt.chain_op(0)], k.N, [absmax(ad, k.N), absmax(bd, k.N)])

    def run(fmt, n, slot=None):
        ns, stride = n.in_scale() if n is not None else (None, 0)
        y = Out((k.N, 2, k.Cout // 8, k.H, k.W, 8), torch.float16) if fmt >= SPLIT else Out((k.N, k.Cout // 8, k.H, k.W, 8) if fmt == CB8 else (k.N, k.Cout, k.H, k.W))
        call("conv_forward_blend", c._prepacked, c._scales, c._bias32, k.N, Ca, Cb, k.Cout, k.H, k.W, ad, bd, md, 1, float(k.slope), 1.0, -1.0,
             y.t, fmt, ns, stride, slot)
        return y

    slot = Out((k.N,), fill=0.0)
    y32 = run(NCHW, None, slot.t).cpu()
    cat = lambda dt: torch.cat([a.to(dt) * m.to(dt), b.to(dt) * (1.0 - m.to(dt))], dim=1)
    what = "%s [%s]" % (k.name, describe(k.expect))
    hold(what, y32, conv_ref(c, cat(torch.float64), k.slope), CONV_TIER[False], [TILE[V.BLEND]], lambda: conv_ref(c, cat(torch.float32), k.slope, torch.float32))
    same_values(what + " y_absmax == max|y| of the image", slot.cpu(), y32.abs().amax(dim=(1, 2, 3)))
    _formats_agree(what, run, y32, nxt, k.N, k.Cout)


# ---- (a) SR blocks: the eight up-sampling instantiations ---------------------------------------------------------------------------------------------
# A block's input has standard deviation 3/8.  Both convs are demodulated (unit gain), so their results have about that deviation: clamp 0.75 is two
# deviations and holds a few percent of sample 0 (and nothing of sample 1, 2^-5 of it): it bites, as in test_sr_block_ragged_vs_oracle, and the tensor
# is still the conv's result.  The tiers are relative to max|ref|, which a clamp caps while a layer's rounding error follows the magnitude BEFORE the
# clamp: with a deviation of 2 (clamp at 0.37 deviations, most of the tensor saturated, max|ref| an eleventh of the unclamped one) the f16mx block on a
# SPLIT_MX input measured 1.42e-4 of max|ref| = 1.06e-4 absolute, where the same block without the clamp has 2.98e-5 of max|ref| = 2.5e-4 absolute.
BLOCK_INPUT_STD = 0.375


def _block_seed(k):
    return seed_of("block %d %d %d %d %d %s" % (k.Cin, k.Cout, k.Hin, k.Win, getattr(k, "up", 1), k.clamp))


@functools.lru_cache(maxsize=None)
def _block_reference(Cin, Cout, Hin, Win, up, clamp, seed):
    """(x, img, ws, float64 x_out, float64 img_out) of the block make_block(gen(seed), ..) builds: one reference for every precision and input format."""
    _, p = make_block(gen(seed), Cin, Cout, up, clamp)
    g = gen(seed + 1)
    x, img, ws = samples(g, 2, Cin, Hin, Win, scale=BLOCK_INPUT_STD), randn(g, 2, 3, Hin, Win, scale=0.5), 1.0 + randn(g, 2, 3, 512, scale=0.2)
    rx, ri = _block_fp64(torch, p, x, img, ws, up, clamp)
    return x, img, ws, rx, ri


def _block_setup(k, x, wsd):
    """The block of case k on the device, prepared and folded for x."""
    blk, _ = make_block(gen(_block_seed(k)), k.Cin, k.Cout, getattr(k, "up", 1), k.clamp, precision="f16mx" if k.precision == V.F16MX else "f16x3")
    prep = blk.prepare(wsd, wsd.device)
    chain_fold([blk.chain_op(-1)], k.N, [absmax(dev(x), k.N)])
    return blk, prep


def _block_operand(blk, x, x_fmt, N):
    return operand(x, x_fmt, _consumer_scale(blk, N, blk.in_channels) if x_fmt >= SPLIT else None)


def run_block_case(k):
    got = block_variants(k.N, k.Cin, k.Cout, k.Hin, k.Win, k.up, k.x_fmt, k.precision, k.clamp)
    assert got == (k.expect0, k.expect1), (k.name, got)
    x, img, ws, rx, ri = _block_reference(k.Cin, k.Cout, k.Hin, k.Win, k.up, k.clamp, _block_seed(k))
    imgd, wsd = dev(img), dev(ws)
    blk, prep = _block_setup(k, x, wsd)
    xin = _block_operand(blk, x, k.x_fmt, k.N)
    slot = Out((k.N,), fill=0.0)
    xo, io = block_run(blk, prep, xin, k.x_fmt, imgd, k.N, k.Hin, k.Win, NCHW, x_absmax=slot.t)
    xo, io = xo.cpu(), io.cpu()
    mx = k.precision == V.F16MX
    what = "%s [%s | %s]" % (k.name, describe(k.expect0), describe(k.expect1))
    tiles = [TILE[k.expect1[0]]] + ([TILE[V.UPCONV]] if k.up else [TILE[k.expect0[0]]])
    hold(what + " x", xo, rx, BLOCK_TIER[mx], tiles)
    hold(what + " img", io, ri, BLOCK_TIER[mx], tiles)
    same_values(what + " x_absmax == max|x| of the image", slot.cpu(), xo.abs().amax(dim=(1, 2, 3)))
    if k.clamp is not None:
        bite = float((xo[0].abs() >= k.clamp - 1e-6).float().mean())
        print("variants %s: clamp %.2f holds %.1f%% of sample 0's x" % (what, k.clamp, 100.0 * bite))
        assert float(xo.abs().max()) <= k.clamp and (bite > 0.01 or k.Hin * k.Win == 1), (k.name, float(xo.abs().max()), bite)
        assert float(rx.abs().max()) == k.clamp, "the clamp does not bite in the reference"


@pytest.mark.parametrize("case", V.BLOCK_CASES, ids=named)
def test_block_vs_fp64(case):
    run_block_case(case)


def child_main():
    """The cases that need another R3D_CONV_WINO than the default (the mode is read once per process)."""
    mode = int(os.environ["R3D_CONV_WINO"])
    for k in V.BLOCK_CASES_WINO1:
        if k.mode == mode:
            run_block_case(k)
    print("variants child: R3D_CONV_WINO=%d done" % mode)


def test_upconv_records_in_plain_split_out_under_winograd_mode_1():
    """upconv_fir_f16x3_kernel<*, false, true>: a SPLIT_MX input whose conv1 runs the Winograd kernel (conv_wino_f16x3_kernel<true>), which only
    R3D_CONV_WINO = 1 | 2 sends an f16mx block to -- in a child process, at the block's f16mx tier."""
    env = dict(os.environ, R3D_CONV_WINO="1")
    r = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_sr_conv_variants as t; t.child_main()"
                        % (ROOT, os.path.join(ROOT, "tests"))], env=env, capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and "R3D_CONV_WINO=1 done" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


# ---- (b) the up-sampling conv: ragged == zero-embedded ---------------------------------------------------------------------------------------------------
def _conv0_output(blk, N, Cin, Cout, Hin, Win):
    """conv0's SPLIT / SPLIT_MX output [N, 2, Cout/8, 2 Hin, 2 Win, 8] as 16-bit words, read from the block's workspace after a forward: xin, T, y0, xo, rgbp,
    each rounded up to 256 bytes (the sizes tests/test_abi.py pins)."""
    a256 = lambda b: (b + 255) // 256 * 256
    xin, T = a256(N * Cin * Hin * Win * 4), a256(N * Cout * 4 * (Hin + 1) * (Win + 1) * 4)
    y, rgbp = a256(N * Cout * 4 * Hin * Win * 4), a256(N * (Cout // 64) * 3 * 4 * Hin * Win * 4)
    assert xin + T + 2 * y + rgbp == int(_lib.load().r3d_sr_block_workspace_bytes(N, Cin, Cout, Hin, Win))
    torch.cuda.synchronize()
    return blk._workspace[xin + T:xin + T + N * Cout * 4 * Hin * Win * 4].view(torch.int16).view(N, 2, Cout // 8, 2 * Hin, 2 * Win, 8).cpu()


@pytest.mark.parametrize("case", V.BLOCK_EMBED_CASES, ids=named)
def test_block_ragged_equals_zero_embedded(case):
    """A block on Hin x Win and on the same input (and image) at the origin of a zero canvas: conv0's output is the same bits on [0, 2 Hin) x [0, 2 Win)
    (the FIR's zero rows, the tile mostly outside the image, the idle blocks of the grid); the block's x and img are on [0, 2 Hin - 1) x [0, 2 Win - 1),
    where conv1 reads nothing else (beyond the image the canvas holds conv0's activated bias, not zero)."""
    k = case
    CH, CW = k.canvas
    assert block_variants(k.N, k.Cin, k.Cout, k.Hin, k.Win, 1, k.x_fmt, k.precision, k.clamp) == (k.expect0, k.expect1), k.name
    assert block_variants(k.N, k.Cin, k.Cout, CH, CW, 1, k.x_fmt, k.precision, k.clamp) == (k.canvas0, k.canvas1), k.name
    assert k.expect0[:2] == k.canvas0[:2] and k.expect1[0] == k.canvas1[0]
    g = gen(seed_of(k.name))
    x, img, ws = samples(g, k.N, k.Cin, k.Hin, k.Win, scale=BLOCK_INPUT_STD), randn(g, k.N, 3, k.Hin, k.Win, scale=0.5), 1.0 + randn(g, k.N, 3, 512, scale=0.2)
    xc, imgc = torch.zeros(k.N, k.Cin, CH, CW), torch.zeros(k.N, 3, CH, CW)
    xc[:, :, :k.Hin, :k.Win], imgc[:, :, :k.Hin, :k.Win] = x, img
    wsd = dev(ws)
    assert torch.equal(absmax(dev(x), k.N).cpu(), absmax(dev(xc), k.N).cpu())
    blk, prep = _block_setup(k, x, wsd)
    xin, cin = _block_operand(blk, x, k.x_fmt, k.N), _block_operand(blk, xc, k.x_fmt, k.N)
    xo, io = block_run(blk, prep, xin, k.x_fmt, dev(img), k.N, k.Hin, k.Win, NCHW)
    y0 = _conv0_output(blk, k.N, k.Cin, k.Cout, k.Hin, k.Win)
    xoc, ioc = block_run(blk, prep, cin, k.x_fmt, dev(imgc), k.N, CH, CW, NCHW)
    y0c = _conv0_output(blk, k.N, k.Cin, k.Cout, CH, CW)
    xo, io, xoc, ioc = xo.cpu(), io.cpu(), xoc.cpu(), ioc.cpu()
    OH, OW = 2 * k.Hin, 2 * k.Win
    what = "%s canvas %dx%d [%s | %s]" % (k.name, CH, CW, describe(k.expect0), describe(k.expect1))
    assert bool((y0 != 0).any()) and float(xo.abs().max()) > 0.0
    same_values(what + " conv0 on the image", y0, y0c[:, :, :, :OH, :OW, :])
    same_values(what + " x inside the image", xo[:, :, :OH - 1, :OW - 1], xoc[:, :, :OH - 1, :OW - 1])
    same_values(what + " img inside the image", io[:, :, :OH - 1, :OW - 1], ioc[:, :, :OH - 1, :OW - 1])


def test_the_variant_table_is_printed():
    """One line per case of the table (pytest -s): what each case reaches, as recorded and as tests/test_sr_conv_variant_host.py checks it."""
    for name, rec in V.all_records():
        print("variants table: %-58s %s" % (name, describe(rec)))
    assert {r[0] for _, r in V.all_records()} == set(range(9))
