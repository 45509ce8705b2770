"""CPU: which kernel variant, grid and block order the host picks for an SR conv layer call (r3d_debug_conv_variant / r3d_debug_sr_block_variants,
include/r3d_hip.h: the launchers of csrc/r3d_sr_f16x3.hip dispatch on the same structs) against the rules written out in tests/sr_variant_cases.py, at
every boundary of the choice, and the variant column of the table tests/test_gpu_sr_conv_variants.py runs.  Nothing is launched."""
import ctypes
import os
import subprocess
import sys

import pytest

import sr_variant_cases as V
from sr_variant_cases import (BLEND, C1X1, CB8, D16, D16_MX, F16MX, F16X3, NCHW, R8, R8_MX, SPLIT, SPLIT_MX, UP_CLAMP, UP_MX, UP_MXIN, UPCONV, WINO,
                              WINO_MX)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = -1


def conv_variant(N, Cin, Cout, H, W, k, x_fmt, blend=0):
    from real3dportrait_amd import _lib
    out = (ctypes.c_int * 6)()
    _lib.check(_lib.load().r3d_debug_conv_variant(N, Cin, Cout, H, W, k, x_fmt, blend, out), "debug_conv_variant")
    return (out[0], out[1], out[2], (out[3], out[4], out[5]))


def block_variants(N, Cin, Cout, Hin, Win, up, x_fmt, precision, clamp):
    from real3dportrait_amd import _lib
    out = (ctypes.c_int * 12)()
    _lib.check(_lib.load().r3d_debug_sr_block_variants(N, Cin, Cout, Hin, Win, up, x_fmt, precision, -1.0 if clamp is None else float(clamp), out),
               "debug_sr_block_variants")
    return (out[0], out[1], out[2], (out[3], out[4], out[5])), (out[6], out[7], out[8], (out[9], out[10], out[11]))


def test_the_process_has_the_default_winograd_mode():
    assert "R3D_CONV_WINO" not in os.environ or os.environ["R3D_CONV_WINO"] == "3", "these tests state the default mode; the other modes run in child processes"


@pytest.mark.parametrize("x_fmt,direct,rows8", [(SPLIT, D16, R8), (NCHW, D16, R8), (SPLIT_MX, D16_MX, R8_MX)])
def test_the_256_block_boundary(x_fmt, direct, rows8):
    """N x tiles x cout tiles = 256 is the last launch on 8-row tiles, 257 the first on 16-row ones -- through each of the three factors."""
    for N, Cout, H, W in [(256, 128, 9, 9), (128, 256, 9, 9), (64, 128, 17, 17), (32, 256, 17, 31), (1, 128, 16 * 16 - 1, 16 * 16 - 3), (4, 128, 127, 113)]:
        tiles = -(-H // 16) * -(-W // 16)
        assert N * tiles * (Cout // 128) == 256
        t8 = -(-H // 8) * -(-W // 16)
        got = conv_variant(N, 32, Cout, H, W, 3, x_fmt)
        assert got == (rows8, 0, 2 if t8 % 8 == 0 else 0, (t8, Cout // 128, N)) == V.rules_conv(N, 32, Cout, H, W, 3, x_fmt), (N, Cout, H, W, got)
    for N, Cout, H, W in [(257, 128, 9, 9), (43, 128, 17, 33), (129, 256, 9, 9), (1, 128, 16 * 16 + 1, 16 * 16 - 3), (1, 128, 16 * 16 - 1, 16 * 17 - 3), (13, 256, 3, 150)]:
        tiles = -(-H // 16) * -(-W // 16)
        assert N * tiles * (Cout // 128) > 256
        got = conv_variant(N, 32, Cout, H, W, 3, x_fmt)
        assert got == (direct, 0, 2 if tiles % 8 == 0 else 0, (tiles, Cout // 128, N)) == V.rules_conv(N, 32, Cout, H, W, 3, x_fmt), (N, Cout, H, W, got)
    # the padded cout tile counts as a whole one: Cout 132 is two
    assert conv_variant(43, 32, 132, 17, 17, 3, x_fmt)[0] == direct and conv_variant(43, 32, 128, 17, 17, 3, x_fmt)[0] == rows8


def test_winograd_eligibility_in_the_default_mode():
    """A plain 3x3 conv over fp32 / plain SPLIT takes the Winograd kernel on whole 16 x 16 tiles only; an operand with fp8 records never does."""
    for x_fmt in (NCHW, CB8, SPLIT):
        assert conv_variant(2, 32, 128, 32, 48, 3, x_fmt) == (WINO, 0, 0, (6, 1, 2))
        assert conv_variant(40, 32, 256, 64, 32, 3, x_fmt) == (WINO, 0, 2, (8, 2, 40))             # (no 256-block rule for it)
    assert conv_variant(2, 7, 72, 32, 48, 3, NCHW) == (WINO, 0, 0, (6, 1, 2))                        # Cin padded to 16, Cout to 128: whole stages and blocks
    for H, W in [(31, 48), (33, 48), (32, 47), (32, 49), (16, 15), (1, 16)]:
        for x_fmt in (NCHW, SPLIT):
            got = conv_variant(2, 32, 128, H, W, 3, x_fmt)
            assert got[0] == R8 and got == V.rules_conv(2, 32, 128, H, W, 3, x_fmt), (H, W, got)
        assert conv_variant(90, 32, 128, H, W, 3, SPLIT)[0] in (D16, R8)
    assert conv_variant(2, 32, 128, 32, 48, 3, SPLIT_MX) == (R8_MX, 0, 0, (12, 1, 2))
    assert conv_variant(50, 32, 128, 32, 48, 3, SPLIT_MX) == (D16_MX, 0, 0, (6, 1, 50))
    # an SR block: conv1 of an f16x3 block on whole tiles, never of an f16mx one; conv0 of a block without up-sampling never (it has no Winograd pack)
    assert block_variants(2, 32, 128, 8, 24, 1, NCHW, F16X3, None)[1] == (WINO, 0, 0, (3, 1, 2))
    assert block_variants(2, 32, 128, 8, 24, 1, NCHW, F16MX, None)[1] == (R8_MX, 0, 0, (6, 1, 2))
    c0, c1 = block_variants(2, 32, 128, 16, 48, 0, SPLIT, F16X3, None)
    assert c0 == (R8, 0, 0, (6, 1, 2)) and c1 == (WINO, 0, 0, (3, 1, 2))


_CHILD = """
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import test_sr_conv_variant_host as T
import sr_variant_cases as V
mode = %d
for x_fmt in (V.NCHW, V.SPLIT, V.SPLIT_MX):
    for H, W in ((32, 48), (32, 47), (17, 33)):
        for N in (2, 50):
            assert T.conv_variant(N, 32, 128, H, W, 3, x_fmt) == V.rules_conv(N, 32, 128, H, W, 3, x_fmt, mode=mode), (x_fmt, H, W, N)
for prec in (V.F16X3, V.F16MX):
    for x_fmt in ((V.NCHW, V.SPLIT) if prec == V.F16X3 else (V.NCHW, V.SPLIT_MX)):
        for up, Hin, Win in ((1, 8, 24), (1, 13, 15), (0, 16, 48), (0, 15, 29)):
            for clamp in (None, 0.75):
                assert T.block_variants(2, 32, 128, Hin, Win, up, x_fmt, prec, clamp) == V.rules_block(2, 32, 128, Hin, Win, up, x_fmt, prec, clamp, mode=mode), (prec, x_fmt, up, Hin)
for c in V.BLOCK_CASES_WINO1:
    if c.mode == mode:
        assert T.block_variants(c.N, c.Cin, c.Cout, c.Hin, c.Win, c.up, c.x_fmt, c.precision, c.clamp) == (c.expect0, c.expect1), c.name
print("conv layer on whole tiles:", T.conv_variant(2, 32, 128, 32, 48, 3, V.SPLIT)[0], "f16x3 conv1:", T.block_variants(2, 32, 128, 8, 24, 1, V.NCHW, V.F16X3, None)[1][0],
      "f16mx conv0 bits / conv1:", T.block_variants(2, 32, 128, 8, 24, 1, V.SPLIT_MX, V.F16MX, None)[0][1], T.block_variants(2, 32, 128, 8, 24, 1, V.SPLIT_MX, V.F16MX, None)[1][0])
"""


@pytest.mark.parametrize("mode,conv,conv1_x3,bits_mx,conv1_mx", [(0, R8, R8, UP_MX | UP_MXIN, R8_MX), (1, WINO, WINO, UP_MXIN, WINO_MX), (2, R8, R8, UP_MXIN, WINO_MX),
                                                                 (3, WINO, WINO, UP_MX | UP_MXIN, R8_MX)])
def test_winograd_modes_in_a_child_process(mode, conv, conv1_x3, bits_mx, conv1_mx):
    """R3D_CONV_WINO is read once per process: 0 never | 1 both precisions | 2 f16mx only | 3 f16x3 only.  A conv layer is an f16x3 layer to the switch; an
    f16mx block whose conv1 takes the Winograd kernel gets a plain SPLIT operand from conv0 (no UP_MX)."""
    env = dict(os.environ, R3D_CONV_WINO=str(mode))
    r = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, os.path.join(ROOT, "tests"), mode)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    want = "conv layer on whole tiles: %d f16x3 conv1: %d f16mx conv0 bits / conv1: %d %d" % (conv, conv1_x3, bits_mx, conv1_mx)
    assert r.stdout.strip().splitlines()[-1] == want, (r.stdout, want)


@pytest.mark.parametrize("H,W,tiles16,tiles8", [(17, 97, 14, 21), (16, 97, 7, 14), (20, 50, 8, 12), (31, 17, 4, 8), (33, 33, 9, 15), (31, 50, 8, 16), (57, 31, 8, 16), (33, 50, 12, 20),
                                                (64, 49, 16, 32), (8, 97, 7, 7), (24, 33, 6, 9)])
def test_block_order_follows_the_tile_count_of_the_kernel_that_runs(H, W, tiles16, tiles8):
    """order = 2 exactly when the tile count of the launched kernel is a multiple of 8: 7, 8, 9, 16 (and more) tiles on 16-row and on 8-row tiles."""
    for x_fmt, d16, r8 in ((SPLIT, D16, R8), (SPLIT_MX, D16_MX, R8_MX)):
        assert conv_variant(1, 16, 8, H, W, 3, x_fmt) == (r8, 0, 2 if tiles8 % 8 == 0 else 0, (tiles8, 1, 1))
        N = 256 // tiles16 + 1
        assert conv_variant(N, 16, 8, H, W, 3, x_fmt) == (d16, 0, 2 if tiles16 % 8 == 0 else 0, (tiles16, 1, N))
    assert conv_variant(1, 16, 8, H, W, 1, SPLIT) == (C1X1, 0, 2 if tiles16 % 8 == 0 else 0, (tiles16, 1, 1))
    assert conv_variant(1, 16, 8, H, W, 1, SPLIT, blend=1) == (BLEND, 0, 0, (tiles16, 1, 1))           # the blend kernel takes its blocks in grid order


def test_a_1x1_conv_never_takes_a_3x3_kernel():
    for N in (1, 2, 300):
        for Cin, Cout in ((3, 4), (16, 128), (64, 136), (512, 256)):
            for H, W in ((1, 1), (16, 16), (32, 48), (17, 33), (128, 128)):
                for x_fmt in ((NCHW,) if Cin % 16 else (NCHW, CB8, SPLIT)):
                    got = conv_variant(N, Cin, Cout, H, W, 1, x_fmt)
                    tiles = -(-H // 16) * -(-W // 16)
                    assert got == (C1X1, 0, 2 if tiles % 8 == 0 else 0, (tiles, -(-Cout // 128), N)) == V.rules_conv(N, Cin, Cout, H, W, 1, x_fmt), (N, Cin, Cout, H, W, got)
                if Cin % 64 == 0:
                    assert conv_variant(N, Cin, Cout, H, W, 1, CB8, blend=1) == (BLEND, 0, 0, (tiles, -(-Cout // 128), N)) == V.rules_conv(N, Cin, Cout, H, W, 1, CB8, blend=1)


@pytest.mark.parametrize("clamp", [None, 0.0, 0.75])
@pytest.mark.parametrize("precision,x_fmt", [(F16X3, NCHW), (F16X3, CB8), (F16X3, SPLIT), (F16MX, NCHW), (F16MX, SPLIT), (F16MX, SPLIT_MX)])
def test_upsampling_instantiations_of_the_default_mode(precision, x_fmt, clamp):
    """<CLAMP, MX, MXIN>: clamp >= 0 | an f16mx block whose conv1 stays on the direct kernels | a SPLIT_MX input.  In the default mode an f16mx block's
    conv1 never takes the Winograd kernel, so the remaining two, <*, false, true>, need R3D_CONV_WINO = 1 | 2 (test_winograd_modes_in_a_child_process)."""
    for Hin, Win in ((13, 15), (8, 24), (16, 16)):                        # (8x24, 16x16: conv1's output is whole 16 x 16 tiles)
        c0, c1 = block_variants(2, 32, 128, Hin, Win, 1, x_fmt, precision, clamp)
        bits = (UP_CLAMP if clamp is not None else 0) | (UP_MX if precision == F16MX else 0) | (UP_MXIN if x_fmt == SPLIT_MX else 0)
        assert c0[:3] == (UPCONV, bits, 0), (Hin, Win, c0)
        whole = (2 * Hin) % 16 == 0 and (2 * Win) % 16 == 0
        assert c1[0] == (R8_MX if precision == F16MX else WINO if whole else R8), (Hin, Win, c1)
        assert (c0, c1) == V.rules_block(2, 32, 128, Hin, Win, 1, x_fmt, precision, clamp)


@pytest.mark.parametrize("Hin,Win,tiles", [(1, 1, 1), (14, 14, 1), (13, 15, 2), (14, 28, 2), (15, 29, 6), (20, 50, 8), (28, 56, 8), (29, 56, 12), (42, 42, 9), (15, 113, 18)])
def test_upsampling_grid_and_its_idle_slots(Hin, Win, tiles):
    """8 XCDs x ceil(tiles / 8) tile slots x Cout / 32 cout groups: 1, 2 and 9 tiles leave 7, 6 and 7 slots per cout group idle, 8 none."""
    for Cout, N in ((128, 1), (256, 3)):
        c0, _ = block_variants(N, 16, Cout, Hin, Win, 1, NCHW, F16X3, None)
        slots = 8 * -(-tiles // 8)
        assert c0 == (UPCONV, 0, 0, (slots * (Cout // 32), N, 1)), (Hin, Win, c0)
        assert V.upconv_idle_slots(c0, Cout, tiles) == (slots - tiles) * (Cout // 32)
    if tiles in (1, 2, 8, 9):
        assert slots - tiles == {1: 7, 2: 6, 8: 0, 9: 7}[tiles]


def test_block_conv1_and_plain_conv0_follow_the_conv_rules():
    """conv1 (and conv0 of a block without up-sampling) take the 3x3 rules at the block's output size, the 256-block boundary included."""
    for N, Hin, Win in ((2, 13, 15), (64, 16, 15), (65, 16, 15), (10, 40, 41)):          # conv1 out 26x30 .. 80x82: 8, 256, 260, 300 blocks of 16 rows
        for precision, x_fmt in ((F16X3, NCHW), (F16MX, NCHW), (F16MX, SPLIT_MX)):
            mx = precision == F16MX
            c0, c1 = block_variants(N, 32, 128, Hin, Win, 1, x_fmt, precision, None)
            assert c1 == V.rules_conv(N, 128, 128, 2 * Hin, 2 * Win, 3, SPLIT_MX if mx else SPLIT), (N, Hin, Win, c1)
            n0, n1 = block_variants(N, 32, 128, 2 * Hin, 2 * Win, 0, x_fmt, precision, None)
            assert n1 == c1 and n0 == V.rules_conv(N, 32, 128, 2 * Hin, 2 * Win, 3, x_fmt, mode=0), (N, Hin, Win, n0)
    assert block_variants(65, 32, 128, 16, 15, 1, NCHW, F16MX, None)[1] == (D16_MX, 0, 0, (4, 1, 65))
    assert block_variants(64, 32, 128, 16, 15, 1, NCHW, F16MX, None)[1] == (R8_MX, 0, 2, (8, 1, 64))


def test_the_hooks_refuse_what_the_entry_points_refuse():
    from real3dportrait_amd import _lib
    lib = _lib.load()
    out = (ctypes.c_int * 12)()
    for args in ((0, 16, 8, 4, 4, 3, NCHW, 0), (1, 16, 8, 4, 4, 5, NCHW, 0), (1, 24, 8, 4, 4, 3, SPLIT, 0), (1, 16, 8, 4, 4, 1, SPLIT_MX, 0), (1, 16, 8, 4, 4, 3, 4, 0),
                 (1, 64, 8, 4, 4, 3, CB8, 1)):
        assert lib.r3d_debug_conv_variant(*args, out) == INVALID_ARG and b"debug_conv_variant" in lib.r3d_last_error(), args
    assert lib.r3d_debug_conv_variant(1, 16, 8, 4, 4, 3, NCHW, 0, None) == INVALID_ARG
    for args in ((1, 24, 128, 4, 4, 1, NCHW, F16X3), (1, 16, 64, 4, 4, 1, NCHW, F16X3), (1, 16, 128, 4, 4, 2, NCHW, F16X3), (1, 16, 128, 4, 4, 1, NCHW, 0),
                 (1, 16, 128, 4, 4, 1, SPLIT_MX, F16X3), (1, 16, 128, 0, 4, 1, NCHW, F16MX)):
        assert lib.r3d_debug_sr_block_variants(*args, -1.0, out) == INVALID_ARG and b"debug_sr_block_variants" in lib.r3d_last_error(), args


def test_the_gpu_table_reaches_the_variants_it_is_named_after():
    """Every case of tests/test_gpu_sr_conv_variants.py: the recorded variant, order and grid are what the library picks and what the rules say; the table
    as a whole has every row of the variant table at a ragged shape, both precisions, order 0 and 2 on 16-row and 8-row tiles, and all eight
    up-sampling instantiations."""
    for c in V.CONV_CASES + V.FORMAT_CASES:
        assert conv_variant(c.N, c.Cin, c.Cout, c.H, c.W, c.k, c.x_fmt) == c.expect == V.rules_conv(c.N, c.Cin, c.Cout, c.H, c.W, c.k, c.x_fmt), c.name
    b = V.BLEND_CASE
    assert conv_variant(b.N, b.Cin, b.Cout, b.H, b.W, 1, CB8, blend=1) == b.expect == V.rules_conv(b.N, b.Cin, b.Cout, b.H, b.W, 1, CB8, blend=1)
    for c in V.BATCH_CASES:
        assert conv_variant(c.N, c.Cin, c.Cout, c.H, c.W, 3, c.x_fmt) == c.expect == V.rules_conv(c.N, c.Cin, c.Cout, c.H, c.W, 3, c.x_fmt), c.name
        assert conv_variant(2, c.Cin, c.Cout, c.H, c.W, 3, c.x_fmt) == c.small == V.rules_conv(2, c.Cin, c.Cout, c.H, c.W, 3, c.x_fmt), c.name
        assert c.expect[0] in (D16, D16_MX) and c.small[0] == c.expect[0] + 2
    for c in V.EMBED_CASES:
        assert conv_variant(c.N, c.Cin, c.Cout, c.H, c.W, 3, c.x_fmt) == c.expect == V.rules_conv(c.N, c.Cin, c.Cout, c.H, c.W, 3, c.x_fmt), c.name
        assert conv_variant(c.N, c.Cin, c.Cout, c.canvas[0], c.canvas[1], 3, c.x_fmt) == c.expect_canvas == V.rules_conv(c.N, c.Cin, c.Cout, c.canvas[0], c.canvas[1], 3, c.x_fmt)
        assert c.expect[0] == c.expect_canvas[0] and c.canvas[0] >= c.H and c.canvas[1] >= c.W
    for c in V.BLOCK_CASES:
        got = block_variants(c.N, c.Cin, c.Cout, c.Hin, c.Win, c.up, c.x_fmt, c.precision, c.clamp)
        assert c.mode == 3 and got == (c.expect0, c.expect1) == V.rules_block(c.N, c.Cin, c.Cout, c.Hin, c.Win, c.up, c.x_fmt, c.precision, c.clamp), c.name
    for c in V.BLOCK_CASES_WINO1:          # (the library's own answer under that mode: test_winograd_modes_in_a_child_process)
        assert c.mode == 1 and (c.expect0, c.expect1) == V.rules_block(c.N, c.Cin, c.Cout, c.Hin, c.Win, c.up, c.x_fmt, c.precision, c.clamp, mode=1), c.name
    for c in V.BLOCK_EMBED_CASES:
        assert block_variants(c.N, c.Cin, c.Cout, c.Hin, c.Win, 1, c.x_fmt, c.precision, c.clamp) == (c.expect0, c.expect1), c.name
        assert block_variants(c.N, c.Cin, c.Cout, c.canvas[0], c.canvas[1], 1, c.x_fmt, c.precision, c.clamp) == (c.canvas0, c.canvas1), c.name
        assert c.expect0[:2] == c.canvas0[:2] and c.expect1[0] == c.canvas1[0]
    recs = [r for _, r in V.all_records()]
    assert {r[0] for r in recs} == set(range(9))
    assert {r[1] for r in recs if r[0] == UPCONV} == set(range(8))
    for v in (D16, D16_MX, R8, R8_MX):
        assert {r[2] for r in recs if r[0] == v} == {0, 2}, V.NAMES[v]
    # ... at a partial tile (the Winograd kernels take whole tiles only)
    ragged = {c.expect[0] for c in V.CONV_CASES + V.BATCH_CASES + V.EMBED_CASES + V.FORMAT_CASES + [b] if c.H % 16 or c.W % 16}
    assert ragged == {D16, D16_MX, R8, R8_MX, C1X1, BLEND}
    assert all(c.Hin % 14 or c.Win % 14 or (c.Hin, c.Win) == (14, 14) for c in V.BLOCK_CASES if c.up)
    # odd stage counts (16, 48 channels) into a padded cout tile, on every direct 3x3 variant
    assert {c.expect[0] for c in V.CONV_CASES + V.BATCH_CASES if getattr(c, "k", 3) == 3 and c.Cin in (16, 48) and c.Cout % 128} == {D16, D16_MX, R8, R8_MX}
