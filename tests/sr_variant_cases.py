"""Which kernel an SR conv layer call runs on, restated in plain Python from the dispatch rules, and the table of shapes
tests/test_gpu_sr_conv_variants.py runs, each with the variant, block order and grid it is meant to reach.  tests/test_sr_conv_variant_host.py
holds the library's answer (r3d_debug_conv_variant / r3d_debug_sr_block_variants, which the launchers dispatch on) to both on a machine
without a GPU; the GPU tests assert the same record before they run a case, so a shape that drifts to another kernel fails instead of
testing something else.  Never imports the library (like tests/sr_formats.py).

A record is (variant, bits, order, (grid x, y, z)) as include/r3d_hip.h documents it."""
from collections import namedtuple

D16, D16_MX, R8, R8_MX, WINO, WINO_MX, C1X1, BLEND, UPCONV = range(9)
NAMES = {D16: "conv_mfma_f16x3_kernel<4,2,4>", D16_MX: "conv_mfma_f16x3_kernel<4,2,4,MX>", R8: "conv_mfma_f16x3_rows8_kernel", R8_MX: "conv_mfma_f16x3_rows8_kernel<MX>",
         WINO: "conv_wino_f16x3_kernel", WINO_MX: "conv_wino_f16x3_kernel<MX>", C1X1: "conv1x1_mfma_f16x3_kernel<4,2,4>", BLEND: "conv1x1_blend_f16x3_kernel",
         UPCONV: "upconv_fir_f16x3_kernel"}
UP_CLAMP, UP_MX, UP_MXIN = 4, 2, 1
NCHW, CB8, SPLIT, SPLIT_MX = 0, 1, 2, 3
F16X3, F16MX = 1, 2
WINO_DEFAULT = 3                     # R3D_CONV_WINO unset: the Winograd kernel for the f16x3 precision only


def name_of(rec):
    v, bits = rec[0], rec[1]
    if v != UPCONV:
        return NAMES[v]
    return "%s<%s,%s,%s>" % (NAMES[v], "CLAMP" if bits & UP_CLAMP else "-", "MX" if bits & UP_MX else "-", "MXIN" if bits & UP_MXIN else "-")


def _cdiv(a, b):
    return -(-a // b)


def _wino_ok(mode, Ci, Co, H, W, layer_mx):
    """Winograd F(2,3): the mode allows the layer's precision; whole 16 x 16 tiles, whole 16-channel stages and 128-cout blocks."""
    allowed = {0: False, 1: True, 2: layer_mx, 3: not layer_mx}.get(mode, False)
    small = Ci * H * W * 4 < 2 ** 31 and 48 * Ci * Co < 2 ** 31         # 32-bit buffer offsets
    return allowed and H % 16 == 0 and W % 16 == 0 and Ci % 16 == 0 and Co % 128 == 0 and small


def _conv3x3_or_1x1(k, Ci, Co, H, W, N, operand_mx, layer_mx, mode):
    cout_tiles, t16 = Co // 128, _cdiv(W, 16) * _cdiv(H, 16)
    if k == 1:
        variant, tiles = C1X1, t16
    elif not operand_mx and _wino_ok(mode, Ci, Co, H, W, layer_mx):
        variant, tiles = (WINO_MX if layer_mx else WINO), t16
    elif t16 * cout_tiles * N <= 256:                                    # at most half of the 512 block slots: 8-row tiles
        variant, tiles = (R8_MX if operand_mx else R8), _cdiv(W, 16) * _cdiv(H, 8)
    else:
        variant, tiles = (D16_MX if operand_mx else D16), t16
    return (variant, 0, 2 if tiles % 8 == 0 else 0, (tiles, cout_tiles, N))


def rules_conv(N, Cin, Cout, H, W, k, x_fmt, blend=0, mode=WINO_DEFAULT):
    """r3d_conv_forward / _cat (blend 0) or r3d_conv_forward_blend (blend 1)."""
    Ci, Co = _cdiv(Cin, 16) * 16, _cdiv(Cout, 128) * 128
    if blend:
        return (BLEND, 0, 0, (_cdiv(W, 16) * _cdiv(H, 16), Co // 128, N))
    return _conv3x3_or_1x1(k, Ci, Co, H, W, N, x_fmt == SPLIT_MX, False, mode)


def rules_block(N, Cin, Cout, Hin, Win, up, x_fmt, precision, clamp, mode=WINO_DEFAULT):
    """r3d_sr_block_forward at F16X3 | F16MX: (conv0's record, conv1's record)."""
    mx = precision == F16MX
    OH, OW = (2 * Hin, 2 * Win) if up else (Hin, Win)
    wino1 = _wino_ok(mode, Cout, Cout, OH, OW, mx)
    conv1 = _conv3x3_or_1x1(3, Cout, Cout, OH, OW, N, mx and not wino1, mx, mode)     # f16mx on the direct kernels: conv0 left fp8 records
    if not up:                                                                         # conv0 of SynthesisBlockNoUp has no Winograd pack
        return _conv3x3_or_1x1(3, Cin, Cout, OH, OW, N, x_fmt == SPLIT_MX, mx, 0), conv1
    bits = (UP_CLAMP if clamp is not None and clamp >= 0 else 0) | (UP_MX if mx and not wino1 else 0) | (UP_MXIN if x_fmt == SPLIT_MX else 0)
    tiles = _cdiv(Win, 14) * _cdiv(Hin, 14)
    return (UPCONV, bits, 0, (8 * _cdiv(tiles, 8) * (Cout // 32), N, 1)), conv1        # 8 XCDs x tiles-per-XCD slots (the rest idle) x 32-cout groups


def upconv_idle_slots(rec, Cout, tiles):
    """Blocks of an up-sampling grid that find no tile."""
    return rec[3][0] - tiles * (Cout // 32)


# ---- the GPU table ----------------------------------------------------------------------------------------------------------------------------
# slope: the fused LeakyReLU (None: off); bias: present | NULL; x_fmt: the input format of the call; expect: the record the case is named after
ConvCase = namedtuple("ConvCase", "name N Cin Cout H W k x_fmt slope bias expect")
# canvas: the zero canvas the H x W image is placed at the origin of; expect_canvas: its record (the same variant)
EmbedCase = namedtuple("EmbedCase", "name N Cin Cout H W x_fmt canvas expect expect_canvas")
# small: the record of the same shape at N = 2, the 8-row kernel the 16-row one must equal bit for bit
BatchCase = namedtuple("BatchCase", "name N Cin Cout H W x_fmt slope bias expect small")
BlockCase = namedtuple("BlockCase", "name N Cin Cout Hin Win up clamp precision x_fmt mode expect0 expect1")
BlockEmbedCase = namedtuple("BlockEmbedCase", "name N Cin Cout Hin Win clamp precision x_fmt canvas expect0 expect1 canvas0 canvas1")

# (a) small launches vs float64: the 8-row kernels at 1 x 1, one valid row / column in the last tile, 5 / 8 / 9 tiles, one and three 16-channel stages
# with a padded cout tile, two cout tiles, every input format; the 1x1 kernel
CONV_CASES = [
    ConvCase("r8 48->72 17x33 k3 nchw", 2, 48, 72, 17, 33, 3, NCHW, 0.2, True, (R8, 0, 0, (9, 1, 2))),
    ConvCase("r8 16->8 1x1 k3 split", 2, 16, 8, 1, 1, 3, SPLIT, None, False, (R8, 0, 0, (1, 1, 2))),
    ConvCase("r8 3->128 15x31 k3 nchw", 2, 3, 128, 15, 31, 3, NCHW, 0.2, True, (R8, 0, 0, (4, 1, 2))),
    ConvCase("r8 7->256 16x17 k3 nchw", 2, 7, 256, 16, 17, 3, NCHW, None, True, (R8, 0, 0, (4, 2, 2))),
    ConvCase("r8 32->128 31x17 k3 cb8", 2, 32, 128, 31, 17, 3, CB8, 0.2, True, (R8, 0, 2, (8, 1, 2))),
    ConvCase("r8 32->72 33x15 k3 split", 2, 32, 72, 33, 15, 3, SPLIT, 0.2, False, (R8, 0, 0, (5, 1, 2))),
    ConvCase("r8 32->128 20x50 k3 cb8", 2, 32, 128, 20, 50, 3, CB8, None, True, (R8, 0, 0, (12, 1, 2))),
    ConvCase("r8_mx 48->72 17x33 k3 split_mx", 2, 48, 72, 17, 33, 3, SPLIT_MX, 0.2, True, (R8_MX, 0, 0, (9, 1, 2))),
    ConvCase("r8_mx 16->128 31x17 k3 split_mx", 2, 16, 128, 31, 17, 3, SPLIT_MX, None, False, (R8_MX, 0, 2, (8, 1, 2))),
    ConvCase("r8_mx 32->256 1x15 k3 split_mx", 2, 32, 256, 1, 15, 3, SPLIT_MX, 0.2, True, (R8_MX, 0, 0, (1, 2, 2))),
    ConvCase("r8_mx 32->8 33x16 k3 split_mx", 2, 32, 8, 33, 16, 3, SPLIT_MX, None, True, (R8_MX, 0, 0, (5, 1, 2))),
    ConvCase("c1x1 48->72 17x33 k1 nchw", 2, 48, 72, 17, 33, 1, NCHW, 0.2, True, (C1X1, 0, 0, (6, 1, 2))),
    ConvCase("c1x1 7->256 20x50 k1 nchw", 2, 7, 256, 20, 50, 1, NCHW, None, True, (C1X1, 0, 2, (8, 2, 2))),
    ConvCase("c1x1 16->8 1x1 k1 cb8", 2, 16, 8, 1, 1, 1, CB8, 0.2, False, (C1X1, 0, 0, (1, 1, 2))),
]

# (a) + (b) the 16-row kernels: the same ragged shapes at a batch that crosses 256 blocks; sample n of the batch is base sample n % 2
BATCH_CASES = [
    BatchCase("d16 N43 32->128 17x33 nchw", 43, 32, 128, 17, 33, NCHW, 0.2, True, (D16, 0, 0, (6, 1, 43)), (R8, 0, 0, (9, 1, 2))),
    BatchCase("d16 N17 16->256 20x50 split", 17, 16, 256, 20, 50, SPLIT, None, False, (D16, 0, 2, (8, 2, 17)), (R8, 0, 0, (12, 2, 2))),
    BatchCase("d16 N29 48->72 33x33 cb8", 29, 48, 72, 33, 33, CB8, 0.2, True, (D16, 0, 0, (9, 1, 29)), (R8, 0, 0, (15, 1, 2))),
    BatchCase("d16_mx N43 32->128 17x33 split_mx", 43, 32, 128, 17, 33, SPLIT_MX, 0.2, True, (D16_MX, 0, 0, (6, 1, 43)), (R8_MX, 0, 0, (9, 1, 2))),
    BatchCase("d16_mx N17 16->256 20x50 split_mx", 17, 16, 256, 20, 50, SPLIT_MX, None, False, (D16_MX, 0, 2, (8, 2, 17)), (R8_MX, 0, 0, (12, 2, 2))),
    BatchCase("d16_mx N29 48->72 33x33 split_mx", 29, 48, 72, 33, 33, SPLIT_MX, 0.2, True, (D16_MX, 0, 0, (9, 1, 29)), (R8_MX, 0, 0, (15, 1, 2))),
]

# (b) ragged == zero-embedded, every 3x3 variant; the second 16-row pair also sets order 2 against order 0
EMBED_CASES = [
    EmbedCase("r8 N2 48->72 17x33 nchw", 2, 48, 72, 17, 33, NCHW, (35, 50), (R8, 0, 0, (9, 1, 2)), (R8, 0, 0, (20, 1, 2))),
    EmbedCase("r8 N2 16->128 1x15 split", 2, 16, 128, 1, 15, SPLIT, (9, 18), (R8, 0, 0, (1, 1, 2)), (R8, 0, 0, (4, 1, 2))),
    EmbedCase("r8_mx N2 48->72 17x33 split_mx", 2, 48, 72, 17, 33, SPLIT_MX, (35, 50), (R8_MX, 0, 0, (9, 1, 2)), (R8_MX, 0, 0, (20, 1, 2))),
    EmbedCase("r8_mx N2 16->128 1x15 split_mx", 2, 16, 128, 1, 15, SPLIT_MX, (9, 18), (R8_MX, 0, 0, (1, 1, 2)), (R8_MX, 0, 0, (4, 1, 2))),
    EmbedCase("d16 N43 32->128 17x33 nchw", 43, 32, 128, 17, 33, NCHW, (35, 50), (D16, 0, 0, (6, 1, 43)), (D16, 0, 0, (12, 1, 43))),
    EmbedCase("d16 N17 16->256 20x50 cb8", 17, 16, 256, 20, 50, CB8, (37, 63), (D16, 0, 2, (8, 2, 17)), (D16, 0, 0, (12, 2, 17))),
    EmbedCase("d16_mx N43 32->128 17x33 split_mx", 43, 32, 128, 17, 33, SPLIT_MX, (35, 50), (D16_MX, 0, 0, (6, 1, 43)), (D16_MX, 0, 0, (12, 1, 43))),
    EmbedCase("d16_mx N17 16->256 20x50 split_mx", 17, 16, 256, 20, 50, SPLIT_MX, (37, 63), (D16_MX, 0, 2, (8, 2, 17)), (D16_MX, 0, 0, (12, 2, 17))),
]

# (b) formats agree: one call shape, NCHW / CB8 / SPLIT / SPLIT_MX out of every variant (Cout % 16 == 0 for the records)
FORMAT_CASES = [
    ConvCase("r8 N2 48->80 17x33 k3 nchw", 2, 48, 80, 17, 33, 3, NCHW, 0.2, True, (R8, 0, 0, (9, 1, 2))),
    ConvCase("r8_mx N2 48->80 17x33 k3 split_mx", 2, 48, 80, 17, 33, 3, SPLIT_MX, 0.2, True, (R8_MX, 0, 0, (9, 1, 2))),
    ConvCase("d16 N43 32->128 17x33 k3 nchw", 43, 32, 128, 17, 33, 3, NCHW, 0.2, True, (D16, 0, 0, (6, 1, 43))),
    ConvCase("d16 N17 16->256 20x50 k3 split", 17, 16, 256, 20, 50, 3, SPLIT, 0.2, True, (D16, 0, 2, (8, 2, 17))),
    ConvCase("d16_mx N43 32->128 17x33 k3 split_mx", 43, 32, 128, 17, 33, 3, SPLIT_MX, 0.2, True, (D16_MX, 0, 0, (6, 1, 43))),
    ConvCase("d16 N29 48->80 33x33 k3 cb8", 29, 48, 80, 33, 33, 3, CB8, 0.2, True, (D16, 0, 0, (9, 1, 29))),
    ConvCase("c1x1 N2 48->80 17x33 k1 nchw", 2, 48, 80, 17, 33, 1, NCHW, 0.2, True, (C1X1, 0, 0, (6, 1, 2))),
    ConvCase("wino N2 32->128 32x48 k3 nchw", 2, 32, 128, 32, 48, 3, NCHW, 0.2, True, (WINO, 0, 0, (6, 1, 2))),
]
BLEND_CASE = ConvCase("blend 24+40->80 17x33", 2, 64, 80, 17, 33, 1, CB8, 0.2, True, (BLEND, 0, 0, (6, 1, 2)))

# (a) SR blocks: 1, 2, 1, 6 and 8 up-sampling tiles (never whole: 14-input tiles), clamp off and biting, the three (precision, input) pairs the default
# mode has; then Cout 256, an output of whole 16 x 16 tiles (conv1 on Winograd), a block without up-sampling on a SPLIT_MX input, a plain SPLIT input
BLOCK_CASES = [
    BlockCase("up 32->128 1x1 f16x3 nchw clamp None", 2, 32, 128, 1, 1, 1, None, F16X3, NCHW, 3, (UPCONV, 0, 0, (32, 2, 1)), (R8, 0, 0, (1, 1, 2))),
    BlockCase("up 32->128 1x1 f16mx nchw clamp None", 2, 32, 128, 1, 1, 1, None, F16MX, NCHW, 3, (UPCONV, UP_MX, 0, (32, 2, 1)), (R8_MX, 0, 0, (1, 1, 2))),
    BlockCase("up 32->128 1x1 f16mx split_mx clamp None", 2, 32, 128, 1, 1, 1, None, F16MX, SPLIT_MX, 3, (UPCONV, UP_MX | UP_MXIN, 0, (32, 2, 1)), (R8_MX, 0, 0, (1, 1, 2))),
    BlockCase("up 32->128 1x1 f16x3 nchw clamp 0.75", 2, 32, 128, 1, 1, 1, 0.75, F16X3, NCHW, 3, (UPCONV, UP_CLAMP, 0, (32, 2, 1)), (R8, 0, 0, (1, 1, 2))),
    BlockCase("up 32->128 1x1 f16mx nchw clamp 0.75", 2, 32, 128, 1, 1, 1, 0.75, F16MX, NCHW, 3, (UPCONV, UP_CLAMP | UP_MX, 0, (32, 2, 1)), (R8_MX, 0, 0, (1, 1, 2))),
    BlockCase("up 32->128 1x1 f16mx split_mx clamp 0.75", 2, 32, 128, 1, 1, 1, 0.75, F16MX, SPLIT_MX, 3, (UPCONV, UP_CLAMP | UP_MX | UP_MXIN, 0, (32, 2, 1)), (R8_MX, 0, 0, (1, 1, 2))),
    BlockCase("up 32->128 13x15 f16x3 nchw clamp None", 2, 32, 128, 13, 15, 1, None, F16X3, NCHW, 3, (UPCONV, 0, 0, (32, 2, 1)), (R8, 0, 2, (8, 1, 2))),
    BlockCase("up 32->128 13x15 f16mx nchw clamp None", 2, 32, 128, 13, 15, 1, None, F16MX, NCHW, 3, (UPCONV, UP_MX, 0, (32, 2, 1)), (R8_MX, 0, 2, (8, 1, 2))),
    BlockCase("up 32->128 13x15 f16mx split_mx clamp None", 2, 32, 128, 13, 15, 1, None, F16MX, SPLIT_MX, 3, (UPCONV, UP_MX | UP_MXIN, 0, (32, 2, 1)), (R8_MX, 0, 2, (8, 1, 2))),
    BlockCase("up 32->128 13x15 f16x3 nchw clamp 0.75", 2, 32, 128, 13, 15, 1, 0.75, F16X3, NCHW, 3, (UPCONV, UP_CLAMP, 0, (32, 2, 1)), (R8, 0, 2, (8, 1, 2))),
    BlockCase("up 32->128 13x15 f16mx nchw clamp 0.75", 2, 32, 128, 13, 15, 1, 0.75, F16MX, NCHW, 3, (UPCONV, UP_CLAMP | UP_MX, 0, (32, 2, 1)), (R8_MX, 0, 2, (8, 1, 2))),
    BlockCase("up 32->128 13x15 f16mx split_mx clamp 0.75", 2, 32, 128, 13, 15, 1, 0.75, F16MX, SPLIT_MX, 3, (UPCONV, UP_CLAMP | UP_MX | UP_MXIN, 0, (32, 2, 1)), (R8_MX, 0, 2, (8, 1, 2))),
    BlockCase("up 32->128 14x14 f16x3 nchw clamp None", 2, 32, 128, 14, 14, 1, None, F16X3, NCHW, 3, (UPCONV, 0, 0, (32, 2, 1)), (R8, 0, 2, (8, 1, 2))),
    BlockCase("up 32->128 14x14 f16mx nchw clamp None", 2, 32, 128, 14, 14, 1, None, F16MX, NCHW, 3, (UPCONV, UP_MX, 0, (32, 2, 1)), (R8_MX, 0, 2, (8, 1, 2))),
    BlockCase("up 32->128 14x14 f16mx split_mx clamp None", 2, 32, 128, 14, 14, 1, None, F16MX, SPLIT_MX, 3, (UPCONV, UP_MX | UP_MXIN, 0, (32, 2, 1)), (R8_MX, 0, 2, (8, 1, 2))),
    BlockCase("up 32->128 14x14 f16x3 nchw clamp 0.75", 2, 32, 128, 14, 14, 1, 0.75, F16X3, NCHW, 3, (UPCONV, UP_CLAMP, 0, (32, 2, 1)), (R8, 0, 2, (8, 1, 2))),
    BlockCase("up 32->128 14x14 f16mx nchw clamp 0.75", 2, 32, 128, 14, 14, 1, 0.75, F16MX, NCHW, 3, (UPCONV, UP_CLAMP | UP_MX, 0, (32, 2, 1)), (R8_MX, 0, 2, (8, 1, 2))),
    BlockCase("up 32->128 14x14 f16mx split_mx clamp 0.75", 2, 32, 128, 14, 14, 1, 0.75, F16MX, SPLIT_MX, 3, (UPCONV, UP_CLAMP | UP_MX | UP_MXIN, 0, (32, 2, 1)), (R8_MX, 0, 2, (8, 1, 2))),
    BlockCase("up 32->128 15x29 f16x3 nchw clamp None", 2, 32, 128, 15, 29, 1, None, F16X3, NCHW, 3, (UPCONV, 0, 0, (32, 2, 1)), (R8, 0, 2, (16, 1, 2))),
    BlockCase("up 32->128 15x29 f16mx nchw clamp None", 2, 32, 128, 15, 29, 1, None, F16MX, NCHW, 3, (UPCONV, UP_MX, 0, (32, 2, 1)), (R8_MX, 0, 2, (16, 1, 2))),
    BlockCase("up 32->128 15x29 f16mx split_mx clamp None", 2, 32, 128, 15, 29, 1, None, F16MX, SPLIT_MX, 3, (UPCONV, UP_MX | UP_MXIN, 0, (32, 2, 1)), (R8_MX, 0, 2, (16, 1, 2))),
    BlockCase("up 32->128 15x29 f16x3 nchw clamp 0.75", 2, 32, 128, 15, 29, 1, 0.75, F16X3, NCHW, 3, (UPCONV, UP_CLAMP, 0, (32, 2, 1)), (R8, 0, 2, (16, 1, 2))),
    BlockCase("up 32->128 15x29 f16mx nchw clamp 0.75", 2, 32, 128, 15, 29, 1, 0.75, F16MX, NCHW, 3, (UPCONV, UP_CLAMP | UP_MX, 0, (32, 2, 1)), (R8_MX, 0, 2, (16, 1, 2))),
    BlockCase("up 32->128 15x29 f16mx split_mx clamp 0.75", 2, 32, 128, 15, 29, 1, 0.75, F16MX, SPLIT_MX, 3, (UPCONV, UP_CLAMP | UP_MX | UP_MXIN, 0, (32, 2, 1)), (R8_MX, 0, 2, (16, 1, 2))),
    BlockCase("up 32->128 20x50 f16x3 nchw clamp None", 2, 32, 128, 20, 50, 1, None, F16X3, NCHW, 3, (UPCONV, 0, 0, (32, 2, 1)), (R8, 0, 0, (35, 1, 2))),
    BlockCase("up 32->128 20x50 f16mx nchw clamp None", 2, 32, 128, 20, 50, 1, None, F16MX, NCHW, 3, (UPCONV, UP_MX, 0, (32, 2, 1)), (R8_MX, 0, 0, (35, 1, 2))),
    BlockCase("up 32->128 20x50 f16mx split_mx clamp None", 2, 32, 128, 20, 50, 1, None, F16MX, SPLIT_MX, 3, (UPCONV, UP_MX | UP_MXIN, 0, (32, 2, 1)), (R8_MX, 0, 0, (35, 1, 2))),
    BlockCase("up 32->128 20x50 f16x3 nchw clamp 0.75", 2, 32, 128, 20, 50, 1, 0.75, F16X3, NCHW, 3, (UPCONV, UP_CLAMP, 0, (32, 2, 1)), (R8, 0, 0, (35, 1, 2))),
    BlockCase("up 32->128 20x50 f16mx nchw clamp 0.75", 2, 32, 128, 20, 50, 1, 0.75, F16MX, NCHW, 3, (UPCONV, UP_CLAMP | UP_MX, 0, (32, 2, 1)), (R8_MX, 0, 0, (35, 1, 2))),
    BlockCase("up 32->128 20x50 f16mx split_mx clamp 0.75", 2, 32, 128, 20, 50, 1, 0.75, F16MX, SPLIT_MX, 3, (UPCONV, UP_CLAMP | UP_MX | UP_MXIN, 0, (32, 2, 1)), (R8_MX, 0, 0, (35, 1, 2))),
    BlockCase("up 16->256 13x15 f16mx split_mx clamp None", 2, 16, 256, 13, 15, 1, None, F16MX, SPLIT_MX, 3, (UPCONV, UP_MX | UP_MXIN, 0, (64, 2, 1)), (R8_MX, 0, 2, (8, 2, 2))),
    BlockCase("up 16->256 13x15 f16x3 nchw clamp 0.75", 2, 16, 256, 13, 15, 1, 0.75, F16X3, NCHW, 3, (UPCONV, UP_CLAMP, 0, (64, 2, 1)), (R8, 0, 2, (8, 2, 2))),
    BlockCase("up 32->128 8x24 f16x3 nchw clamp None", 2, 32, 128, 8, 24, 1, None, F16X3, NCHW, 3, (UPCONV, 0, 0, (32, 2, 1)), (WINO, 0, 0, (3, 1, 2))),
    BlockCase("noup 32->128 15x29 f16mx split_mx clamp None", 2, 32, 128, 15, 29, 0, None, F16MX, SPLIT_MX, 3, (R8_MX, 0, 0, (4, 1, 2)), (R8_MX, 0, 0, (4, 1, 2))),
    BlockCase("noup 48->128 15x29 f16x3 split clamp 0.75", 2, 48, 128, 15, 29, 0, 0.75, F16X3, SPLIT, 3, (R8, 0, 0, (4, 1, 2)), (R8, 0, 0, (4, 1, 2))),
    BlockCase("up 32->128 13x15 f16x3 split clamp None", 2, 32, 128, 13, 15, 1, None, F16X3, SPLIT, 3, (UPCONV, 0, 0, (32, 2, 1)), (R8, 0, 2, (8, 1, 2))),
]
# upconv_fir_f16x3_kernel<*, false, true>: an f16mx block whose conv1 runs the Winograd kernel, i.e. R3D_CONV_WINO = 1 | 2 (a child process)
BLOCK_CASES_WINO1 = [
    BlockCase("up 32->128 8x24 f16mx split_mx clamp None", 2, 32, 128, 8, 24, 1, None, F16MX, SPLIT_MX, 1, (UPCONV, UP_MXIN, 0, (32, 2, 1)), (WINO_MX, 0, 0, (3, 1, 2))),
    BlockCase("up 32->128 8x24 f16mx split_mx clamp 0.75", 2, 32, 128, 8, 24, 1, 0.75, F16MX, SPLIT_MX, 1, (UPCONV, UP_CLAMP | UP_MXIN, 0, (32, 2, 1)), (WINO_MX, 0, 0, (3, 1, 2))),
]

BLOCK_EMBED_CASES = [
    BlockEmbedCase("up 32->128 13x15 f16x3 nchw clamp None", 2, 32, 128, 13, 15, None, F16X3, NCHW, (17, 20), (UPCONV, 0, 0, (32, 2, 1)), (R8, 0, 2, (8, 1, 2)), (UPCONV, 0, 0, (32, 2, 1)), (R8, 0, 0, (15, 1, 2))),
    BlockEmbedCase("up 32->128 13x15 f16mx nchw clamp 0.75", 2, 32, 128, 13, 15, 0.75, F16MX, NCHW, (17, 20), (UPCONV, UP_CLAMP | UP_MX, 0, (32, 2, 1)), (R8_MX, 0, 2, (8, 1, 2)), (UPCONV, UP_CLAMP | UP_MX, 0, (32, 2, 1)), (R8_MX, 0, 0, (15, 1, 2))),
    BlockEmbedCase("up 32->128 13x15 f16mx split_mx clamp None", 2, 32, 128, 13, 15, None, F16MX, SPLIT_MX, (17, 20), (UPCONV, UP_MX | UP_MXIN, 0, (32, 2, 1)), (R8_MX, 0, 2, (8, 1, 2)), (UPCONV, UP_MX | UP_MXIN, 0, (32, 2, 1)), (R8_MX, 0, 0, (15, 1, 2))),
    BlockEmbedCase("up 32->128 1x1 f16mx split_mx clamp 0.75", 2, 32, 128, 1, 1, 0.75, F16MX, SPLIT_MX, (3, 5), (UPCONV, UP_CLAMP | UP_MX | UP_MXIN, 0, (32, 2, 1)), (R8_MX, 0, 0, (1, 1, 2)), (UPCONV, UP_CLAMP | UP_MX | UP_MXIN, 0, (32, 2, 1)), (R8_MX, 0, 0, (1, 1, 2))),
    BlockEmbedCase("up 32->128 15x29 f16x3 split clamp None", 2, 32, 128, 15, 29, None, F16X3, SPLIT, (30, 31), (UPCONV, 0, 0, (32, 2, 1)), (R8, 0, 2, (16, 1, 2)), (UPCONV, 0, 0, (64, 2, 1)), (R8, 0, 2, (32, 1, 2))),
]


def all_records():
    """Every (case name, record) of the GPU table, for the printed variant table."""
    out = []
    for c in CONV_CASES + FORMAT_CASES + [BLEND_CASE]:
        out.append((c.name, c.expect))
    for c in BATCH_CASES:
        out += [(c.name, c.expect), (c.name + " (N = 2)", c.small)]
    for c in EMBED_CASES:
        out += [(c.name, c.expect), (c.name + " canvas %dx%d" % c.canvas, c.expect_canvas)]
    for c in BLOCK_CASES + BLOCK_CASES_WINO1:
        out += [(c.name + " conv0", c.expect0), (c.name + " conv1", c.expect1)]
    for c in BLOCK_EMBED_CASES:
        out += [(c.name + " conv0", c.expect0), (c.name + " conv1", c.expect1), (c.name + " canvas conv0", c.canvas0), (c.name + " canvas conv1", c.canvas1)]
    return out
