// Host side of the SR conv layers: the one call description, the one argument check and the one fill of the kernels' common arguments behind
// r3d_conv_forward / _cat / _blend (r3d_sr.hip) and the two convs of an SR block (sr_block_forward_f16x3, r3d_sr_f16x3.hip).  An entry point
// describes its call as an SrConvCall, check()s it and hands it to conv_forward_f16x3 / conv_forward_blend_f16x3.  No device code here.
#pragma once
#include "r3d_sr_common.h"

namespace r3d {

// one sample's activation is indexed with 32 bits
inline int check_index32(const char* what, size_t channels, size_t H, size_t W)
{
    if (channels * H * W < ((size_t)1 << 32)) return R3D_OK;
    set_error("%s: activation of %zu elements per sample exceeds the 32-bit index range", what, channels * H * W);
    return R3D_ERR_INVALID_ARG;
}

// One conv layer call as its entry point sees it.  What an entry point has no argument for keeps its default, and the rule about it holds trivially.
struct SrConvCall {
    const char* what = "";
    int N = 0, Cin = 0, Cout = 0, H = 0, W = 0, ksize = 0;
    const void* prepacked = nullptr; const void* scales = nullptr; const float* bias = nullptr;
    const void* x = nullptr; int x_format = R3D_FMT_SPLIT;                      // the input [N][Cin][H][W] in x_format, or ...
    bool blend = false;                                                         // ... cat([bl_a * bl_mask, bl_b * (1 - bl_mask)]): fp32 CB8, Ca + Cb = Cin,
    const float* bl_a = nullptr; const float* bl_b = nullptr; const float* bl_mask = nullptr; int Ca = 0, Cb = 0;      // read by the kernel (no conversion)
    void* y = nullptr; int y_format = R3D_FMT_NONE;                             // the output [N][Cout][H][W]; the SPLIT formats times next_scale
    const float* next_scale = nullptr; size_t next_scale_stride = 0;
    const ConvCat* cat = nullptr;                                               // y is one part of a concatenated SPLIT tensor
    float* y_absmax = nullptr;
    int act = 0; float act_slope = 0.f, act_gain = 1.f, clamp = -1.f;
    void* workspace = nullptr; size_t workspace_bytes = 0;                      // an NCHW | CB8 input as SPLIT
    hipStream_t stream = nullptr;

    bool x_is_split() const { return x_format == R3D_FMT_SPLIT || x_format == R3D_FMT_SPLIT_MX; }

    // What every conv kernel reads of the call; Ci / Co: the channel counts the weights are packed for (padded for a plain conv layer).  The operand
    // (x | bl_*), the weight pack, the toRGB partials and a ConvCat's place in the concatenation stay with the caller.
    template <class Args>
    void fill(Args& a, int Ci, int Co, const float* out_scale, size_t out_scale_stride, size_t bias_stride) const
    {
        a.out_scale = out_scale; a.out_scale_stride_n = out_scale_stride; a.bias = bias; a.bias_stride_n = bias_stride;
        a.OH = H; a.OW = W;
        if (y_format == R3D_FMT_CB8) { a.y_f32 = reinterpret_cast<float*>(y); a.y_f32_stride_n = (size_t)Cout * H * W; }
        else if (y_format == R3D_FMT_NCHW) { a.y_nchw = reinterpret_cast<float*>(y); a.y_nchw_stride_n = (size_t)Cout * H * W; }
        else if (y_format == R3D_FMT_SPLIT || y_format == R3D_FMT_SPLIT_MX) {
            a.y_split = reinterpret_cast<uint4*>(y); a.y_split_stride_n = (size_t)Cout / 8 * H * W * 2;
            a.next_scale = next_scale; a.next_scale_stride_n = next_scale_stride;
            a.y_split_mx = y_format == R3D_FMT_SPLIT_MX ? 1 : 0;
        }
        a.y_absmax = reinterpret_cast<unsigned*>(y_absmax);
        a.Cin = Ci; a.Cout = Co; a.CoutReal = Cout; a.H = H; a.W = W; a.nphase = 1;
        a.act = act; a.act_slope = act_slope; a.act_gain = act_gain; a.clamp = clamp;
        if (ksize == 3) sr_fill_conv3x3_phase(a.ph, H, W);
        else sr_fill_conv1x1_phase(a.ph, H, W);
    }
};

// the arguments every conv layer call has
inline SrConvCall sr_conv_call(const char* what, int N, int Cin, int Cout, int H, int W, int ksize, int act, float act_slope, float act_gain,
                               float clamp, void* y, int y_format, const float* next_scale, size_t next_scale_stride, float* y_absmax, hipStream_t st)
{
    SrConvCall c;
    c.what = what; c.N = N; c.Cin = Cin; c.Cout = Cout; c.H = H; c.W = W; c.ksize = ksize;
    c.act = act; c.act_slope = act_slope; c.act_gain = act_gain; c.clamp = clamp;
    c.y = y; c.y_format = y_format; c.next_scale = next_scale; c.next_scale_stride = next_scale_stride; c.y_absmax = y_absmax; c.stream = st;
    return c;
}

// every rule of r3d_conv_forward / _cat / _blend, once
inline int check(const SrConvCall& c)
{
    const bool no_input = c.blend ? (!c.bl_a || !c.bl_b || !c.bl_mask || c.Ca <= 0 || c.Cb <= 0) : !c.x;
    if (!c.prepacked || !c.scales || !c.y || no_input || (c.cat && !c.cat->mask) || c.N <= 0 || c.Cin <= 0 || c.Cout <= 0 || c.H <= 0 || c.W <= 0)
        { set_error("%s: bad argument", c.what); return R3D_ERR_INVALID_ARG; }
    if (c.cat && c.ksize != 1)
        { set_error("%s: ksize %d: only the 1x1 conv kernel carries the concatenation epilogue", c.what, c.ksize); return R3D_ERR_INVALID_ARG; }
    if (c.ksize != 1 && c.ksize != 3) { set_error("%s: bad argument (ksize %d is not 1 or 3)", c.what, c.ksize); return R3D_ERR_INVALID_ARG; }
    if (c.cat && c.y_format != R3D_FMT_SPLIT && c.y_format != R3D_FMT_SPLIT_MX)
        { set_error("%s: y_format %d must be SPLIT or SPLIT_MX", c.what, c.y_format); return R3D_ERR_INVALID_ARG; }
    if (c.cat && ((c.Cout & 15) || (c.cat->chan_off & 15) || (c.cat->C_total & 15) || c.cat->chan_off < 0 || c.cat->chan_off + c.Cout > c.cat->C_total)) {
        set_error("%s: Cout %d, chan_off %d, C_total %d must be multiples of 16 with chan_off + Cout <= C_total", c.what, c.Cout, c.cat->chan_off, c.cat->C_total);
        return R3D_ERR_INVALID_ARG;
    }
    if (c.blend && ((c.Ca & 7) || (c.Cb & 7) || ((c.Ca + c.Cb) & 63)))
        { set_error("%s: Ca %d and Cb %d must be multiples of 8 and their sum a multiple of 64", c.what, c.Ca, c.Cb); return R3D_ERR_INVALID_ARG; }
    // SPLIT_MX in: fp8 records for the f16mx main loop of the 3x3 kernels; SPLIT_MX out: records for an f16mx consumer, in 16-channel groups
    if (c.x_format < R3D_FMT_NCHW || c.x_format > R3D_FMT_SPLIT_MX || (c.x_format != R3D_FMT_NCHW && (c.Cin & 15)) || (c.x_format == R3D_FMT_SPLIT_MX && c.ksize != 3)) {
        set_error("%s: unsupported input (format %d, Cin %d, ksize %d): blocked formats need Cin %% 16 == 0, SPLIT_MX a 3x3 conv", c.what, c.x_format, c.Cin, c.ksize);
        return R3D_ERR_INVALID_ARG;
    }
    if (c.y_format < R3D_FMT_NCHW || c.y_format > R3D_FMT_SPLIT_MX || (c.Cout & 3) || (c.y_format != R3D_FMT_NCHW && (c.Cout & 7)) || (c.y_format == R3D_FMT_SPLIT_MX && (c.Cout & 15))) {
        set_error("%s: unsupported output (format %d, Cout %d): Cout must be a multiple of 4, blocked formats need Cout %% 8 == 0, SPLIT_MX Cout %% 16 == 0", c.what, c.y_format, c.Cout);
        return R3D_ERR_INVALID_ARG;
    }
    // (Cout padded to the 128-cout block; a concatenation part: the whole destination)
    const int cout = c.cat ? c.cat->C_total : c.Cout;
    if (int rc = check_index32(c.what, (size_t)((c.Cin > cout ? c.Cin : cout) + BLOCK_M), c.H, c.W)) return rc;
    if (!c.blend && !c.x_is_split() && (!c.workspace || c.workspace_bytes < conv_workspace_bytes_f16x3(c.N, c.Cin, c.H, c.W)))
        { set_error("%s: workspace too small", c.what); return R3D_ERR_WORKSPACE; }
    return R3D_OK;
}

// ---- which kernel a conv layer runs on ---------------------------------------------------------------------------------------------------
// The nine kernel variants behind r3d_conv_forward / _cat / _blend and the two convs of an SR block, and the one place that picks among them: the
// launchers of r3d_sr_f16x3.hip dispatch on what sr_conv_variant / sr_blend_variant / sr_block_variants return, and the test hooks
// r3d_debug_conv_variant / r3d_debug_sr_block_variants (include/r3d_hip.h) return the same structs, so what a test is told is what was launched.
enum SrVariant {
    SR_VAR_DIRECT16 = 0,        // conv_mfma_f16x3_kernel<4,2,4>: 3x3, 16 x 16-pixel tiles
    SR_VAR_DIRECT16_MX = 1,     // ... <4,2,4,true>: the f16mx main loop over a SPLIT_MX operand
    SR_VAR_ROWS8 = 2,           // conv_mfma_f16x3_rows8_kernel<false>: 3x3, 8-row tiles, an under-filled launch
    SR_VAR_ROWS8_MX = 3,        // ... <true>
    SR_VAR_WINO = 4,            // conv_wino_f16x3_kernel<false>: Winograd F(2,3) over a plain SPLIT operand
    SR_VAR_WINO_MX = 5,         // ... <true>: conv1 of an f16mx block under R3D_CONV_WINO = 1 | 2
    SR_VAR_CONV1X1 = 6,         // conv1x1_mfma_f16x3_kernel<4,2,4> (with the concatenation epilogue)
    SR_VAR_BLEND1X1 = 7,        // conv1x1_blend_f16x3_kernel (r3d_conv_forward_blend)
    SR_VAR_UPCONV = 8,          // upconv_fir_f16x3_kernel<CLAMP, MX, MXIN>: conv0 of an up-sampling block; `bits` names the instantiation
};
enum { SR_UP_CLAMP = 4, SR_UP_MX = 2, SR_UP_MXIN = 1 };     // SrVariantChoice::bits of SR_VAR_UPCONV

// the tile sizes the grids follow (static_asserted against the kernels' own constants in r3d_sr_f16x3.hip)
static constexpr int SR_TILE = 16, SR_TILE_ROWS8 = 8, SR_UP_TILE = 14, SR_UP_COUTS = 32;
static constexpr size_t SR_ROWS8_MAX_BLOCKS = 256;          // a 3x3 launch of at most this many 16-row blocks (half of the 512 block slots) takes 8-row tiles

struct SrVariantChoice {
    int variant = -1, bits = 0;
    int order = 0;                                          // Conv2Args::order: 2 = the XCD-aware block order, whenever the tile count divides over the 8 XCDs
    unsigned gx = 0, gy = 0, gz = 1;                        // the grid
    int tiles = 0;                                          // pixel tiles of one sample and one cout tile (SR_VAR_UPCONV: gx counts 8 tiles_per_xcd slots, the rest idle)
    bool wino() const { return variant == SR_VAR_WINO || variant == SR_VAR_WINO_MX; }
};

// R3D_CONV_WINO, the A/B switch of the Winograd F(2,3) conv (r3d_sr_wino.h), read once per process: 0 keeps every plain 3x3 conv on the direct
// kernels, 1 both precisions, 2 f16mx only, 3 (default) f16x3 only
inline int sr_wino_mode() { static const int v = getenv("R3D_CONV_WINO") ? atoi(getenv("R3D_CONV_WINO")) : 3; return v; }

// ... and when a plain 3x3 conv over a plain SPLIT operand takes it (mx: the layer's precision is f16mx): the mode allows the precision, and the
// shape is whole 16 x 16-pixel tiles, 16-channel stages, 128-cout blocks
inline bool sr_use_wino(int wino_mode, int Ci, int Co, int H, int W, bool mx)
{
    const int m = wino_mode;
    // (the kernel addresses one sample's SPLIT activation and the weight pack through 32-bit buffer offsets)
    return (m == 1 || (m == 2 && mx) || (m == 3 && !mx)) && (H & 15) == 0 && (W & 15) == 0 && (Ci & 15) == 0 && (Co % BLOCK_M) == 0 &&
           (size_t)Ci * H * W * 4 < ((size_t)1 << 31) && (size_t)48 * Ci * Co < ((size_t)1 << 31);
}

inline int sr_tiles_of(int H, int W, int rows = SR_TILE) { return ((W + SR_TILE - 1) / SR_TILE) * ((H + rows - 1) / rows); }

// One conv layer of ksize 1 | 3 over a SPLIT operand.  Ci / Co: the padded channel counts; operand_mx: the operand carries fp8 records (SPLIT_MX);
// layer_mx: the layer's precision is f16mx (it matters to the Winograd kernel alone, whose operand is always plain SPLIT); wino_mode:
// sr_wino_mode(), or 0 for a layer that has no Winograd weight pack.
inline SrVariantChoice sr_conv_variant(int ksize, int Ci, int Co, int H, int W, int N, bool operand_mx, bool layer_mx, int wino_mode)
{
    SrVariantChoice c;
    c.tiles = sr_tiles_of(H, W);
    c.gy = (unsigned)(Co / BLOCK_M); c.gz = (unsigned)N;
    if (ksize == 3 && !operand_mx && sr_use_wino(wino_mode, Ci, Co, H, W, layer_mx)) c.variant = layer_mx ? SR_VAR_WINO_MX : SR_VAR_WINO;
    else if (ksize == 3 && (size_t)c.tiles * c.gy * c.gz <= SR_ROWS8_MAX_BLOCKS) {
        // under-filled launch: 8 x 16-pixel tiles, twice the blocks (bit-identical results)
        c.variant = operand_mx ? SR_VAR_ROWS8_MX : SR_VAR_ROWS8;
        c.tiles = sr_tiles_of(H, W, SR_TILE_ROWS8);
    }
    // 8 waves x (64 couts x 64 px): 4 waves/SIMD at 2 blocks/CU
    else c.variant = ksize == 1 ? SR_VAR_CONV1X1 : operand_mx ? SR_VAR_DIRECT16_MX : SR_VAR_DIRECT16;
    c.gx = (unsigned)c.tiles;
    c.order = (c.tiles & 7) == 0 ? 2 : 0;
    return c;
}

// cat([a * mask, b * (1 - mask)]) -> 1x1 conv (r3d_conv_forward_blend): one kernel, blocks in grid order
inline SrVariantChoice sr_blend_variant(int Co, int H, int W, int N)
{
    SrVariantChoice c;
    c.variant = SR_VAR_BLEND1X1; c.tiles = sr_tiles_of(H, W);
    c.gx = (unsigned)c.tiles; c.gy = (unsigned)(Co / BLOCK_M); c.gz = (unsigned)N;
    return c;
}

// The two convs of an SR block at precision f16x3 | f16mx (mx), input [N][Cin][Hin][Win] in x_format: v[0] conv0 (the fused up-sampling conv, or the
// plain 3x3 conv of SynthesisBlockNoUp, which has no Winograd pack), v[1] conv1.  conv1 on the Winograd kernel transforms its operand in fp32, so
// conv0 then hands over plain SPLIT: its epilogue writes conv1's fp8 records only when conv1 stays on the direct f16mx kernels.
inline void sr_block_variants(int N, int Cin, int Cout, int Hin, int Win, int up, int x_format, bool mx, float clamp, int wino_mode, SrVariantChoice v[2])
{
    const int OH = up ? 2 * Hin : Hin, OW = up ? 2 * Win : Win;
    const bool mx_in = x_format == R3D_FMT_SPLIT_MX;
    v[1] = sr_conv_variant(3, Cout, Cout, OH, OW, N, mx && !sr_use_wino(wino_mode, Cout, Cout, OH, OW, mx), mx, wino_mode);
    const bool mx0 = mx && !v[1].wino();
    if (!up) { v[0] = sr_conv_variant(3, Cin, Cout, OH, OW, N, mx_in, mx, 0); return; }
    SrVariantChoice c;
    c.variant = SR_VAR_UPCONV;
    c.bits = (clamp >= 0.f ? SR_UP_CLAMP : 0) | (mx0 ? SR_UP_MX : 0) | (mx_in ? SR_UP_MXIN : 0);
    c.tiles = ((Win + SR_UP_TILE - 1) / SR_UP_TILE) * ((Hin + SR_UP_TILE - 1) / SR_UP_TILE);
    c.gx = (unsigned)(8 * ((c.tiles + 7) / 8) * (Cout / SR_UP_COUTS)); c.gy = (unsigned)N;      // 8 XCDs x tiles_per_xcd slots x 32-cout groups
    v[0] = c;
}

// f16x3 implementation (r3d_sr_f16x3.hip)
int conv_forward_f16x3(const SrConvCall& c);
int conv_forward_blend_f16x3(const SrConvCall& c);

}  // namespace r3d
