// Host side of the torso convolutions: the one argument check, the one ConvArgs fill, the one tile table and the one launcher behind the
// seven entry points r3d_torso_conv / _prec (r3d_torso.hip), r3d_torso_conv3d / _prec (r3d_torso_motion.hip) and r3d_torso_conv_pool,
// r3d_torso_conv_split, r3d_torso_conv3d_res (r3d_torso_appearance.hip), and behind r3d_dl_conv (r3d_deeplab.hip: ConvCall::dl, the strided,
// dilated form, which calls check_conv, fill and dispatch itself since it has one tier; r3d_p2g_conv3d of r3d_plane2grid.hip, ConvCall::rp, does the same).  An entry point describes its call as a ConvCall and hands it,
// with its unit's kernel family, to run<Family>().  A family is a tag struct with
//   static constexpr bool tile64x16                                  it has the 64 x 16 tile (the two 3-D families)
//   template <int PREC, bool VEC, int WM, int WN, int TM, int TN>
//   static void (*kernel())(ConvArgs)                                its instantiation of conv_tile (r3d_torso_conv.h) for that tier, loader and tile
// No device code here.
#pragma once
#include "r3d_common.h"
#include "r3d_torso_conv.h"

namespace r3d {
namespace tlaunch {

using tconv::ConvArgs;

// One conv call as its entry point sees it.  What an entry point has no argument for keeps its default, and the rule about it holds trivially.
struct ConvCall {
    const float* x = nullptr; int B = 0, D = 1, Hs = 0, Ws = 0, Cin = 0;       // [B, D, Hs, Ws, Cin] (in_nchw: [B, Cin, Hs, Ws]); D = 1: a 2-D input
    bool volume = false;                         // a Conv3d with ksize depth taps; false: a 2-D layer, one depth and ONE depth tap (no zero taps)
    int in_nchw = 0, ksize = 0, upsample = 0;
    const float* ps = nullptr; const float* pt = nullptr; float pslope = 0.0f;  // the prologue pair
    const float* w = nullptr; const float* bias = nullptr; int Cout = 0;
    int act = 0; float slope = 0.0f;
    int pool = 0, full_depth = 0, split = 1;     // split: the depth of the depth-split store (1: none)
    const float* res = nullptr;
    float* y = nullptr; int ycs = 0, yco = 0;    // channel-last output, its row length and this conv's first channel in it
    float* yn = nullptr;                         // NCHW / NCDHW output
    int precision = R3D_TORSO_F32;
    // the strided, dilated form (r3d_dl_conv; conv_tile's DL): H x W is then the output grid, act 1 is ReLU and res goes in before it
    bool dl = false; int stride = 1, dilation = 1, pad = 0, bias_bstride = 0;
    // replicate padding behind a per-sample prologue (r3d_p2g_conv3d; conv_tile's RP): ps, pt are then [B, Cin]
    bool rp = false;

    int out_size(int n) const { const long long v = (long long)n + 2LL * pad - (long long)dilation * (ksize - 1) - 1; return v < 0 ? 0 : (int)(v / stride) + 1; }
    int H() const { return dl ? out_size(Hs) : Hs << upsample; }
    int W() const { return dl ? out_size(Ws) : Ws << upsample; }
    int Do() const { return full_depth ? 1 : D; }
    int kd() const { return full_depth ? D : volume ? ksize : 1; }

    void fill(ConvArgs& g) const
    {
        g.x = x; g.B = B; g.Hs = Hs; g.Ws = Ws; g.Cin = Cin; g.H = H(); g.W = W(); g.up = upsample; g.in_nchw = in_nchw ? 1 : 0; g.ks = ksize;
        g.split = split; g.ps = ps; g.pt = pt; g.pslope = pslope; g.w = w; g.Cout = Cout; g.bias = bias; g.act = act; g.slope = slope;
        g.res = res; g.y = y; g.y_nchw = yn;
        g.D = D; g.Do = Do(); g.kd = kd(); g.padz = volume && !full_depth ? ksize / 2 : 0; g.pool = pool; g.ycs = ycs; g.yco = yco;
        g.M = B * g.Do * g.H * g.W; g.K = g.kd * ksize * ksize * Cin;
        // a volume with fewer positions than output channels (down.4, up.0: 256 voxels under 57 MB of weights): the tiles that share a slab
        // of weights run next to each other on one XCD, so the slab comes from HBM once
        g.mfast = volume && g.M < Cout;
        if (dl) g.set_dl(stride, dilation, pad, bias_bstride);          // after M and K: in the depth words
    }
};

// the arguments every entry point has
inline ConvCall conv_call(const float* x, int B, int Hs, int Ws, int Cin, const float* w, const float* bias, int Cout, int ksize, int act,
                          float act_slope, float* y, int precision)
{
    ConvCall c;
    c.x = x; c.B = B; c.Hs = Hs; c.Ws = Ws; c.Cin = Cin; c.w = w; c.bias = bias; c.Cout = Cout; c.ksize = ksize; c.act = act; c.slope = act_slope;
    c.y = y; c.ycs = Cout; c.precision = precision;
    return c;
}

// every rule of the seven entry points, once
inline int check_conv(const char* what, const ConvCall& c)
{
    if (c.precision != R3D_TORSO_F32 && c.precision != R3D_TORSO_BF16X3)
        { set_error("%s: precision %d is not 0 (R3D_TORSO_F32) or 1 (R3D_TORSO_BF16X3)", what, c.precision); return R3D_ERR_INVALID_ARG; }
    if (!c.x || !c.w || (!c.y && !c.yn) || (!c.ps) != (!c.pt)) { set_error("%s: NULL pointer", what); return R3D_ERR_INVALID_ARG; }
    if (c.B <= 0 || c.D <= 0 || c.Hs <= 0 || c.Ws <= 0 || c.Cin <= 0 || c.Cout <= 0 || c.Cin > 4096 || c.Cout > 4096 || c.D > 1024)
        { set_error("%s: bad argument (B, Hs, Ws > 0, 1 <= Cin, Cout <= 4096, a depth of 1 .. 1024)", what); return R3D_ERR_INVALID_ARG; }
    if (c.ksize != 1 && c.ksize != 3 && c.ksize != 7) { set_error("%s: ksize %d is not 1, 3 or 7", what, c.ksize); return R3D_ERR_INVALID_ARG; }
    if (c.upsample != 0 && c.upsample != 1) { set_error("%s: upsample %d is not 0 or 1", what, c.upsample); return R3D_ERR_INVALID_ARG; }
    if (c.act < 0 || c.act > 2) { set_error("%s: act %d is not 0 (none), 1 (leaky) or 2 (sigmoid)", what, c.act); return R3D_ERR_INVALID_ARG; }
    if ((c.pool != 0 && c.pool != 1) || (c.full_depth != 0 && c.full_depth != 1))
        { set_error("%s: pool %d / full_depth %d is not 0 or 1", what, c.pool, c.full_depth); return R3D_ERR_INVALID_ARG; }
    if (c.dl) {
        if (c.stride != 1 && c.stride != 2) { set_error("%s: stride %d is not 1 or 2", what, c.stride); return R3D_ERR_INVALID_ARG; }
        if (c.dilation < 1 || c.dilation > 64) { set_error("%s: dilation %d is not in 1 .. 64", what, c.dilation); return R3D_ERR_INVALID_ARG; }
        if (c.pad < 0 || c.pad > 65536 || c.Hs > (1 << 24) || c.Ws > (1 << 24))
            { set_error("%s: pad %d is not in 0 .. 65536, or a side of %d x %d is above 2^24", what, c.pad, c.Hs, c.Ws); return R3D_ERR_INVALID_ARG; }
        if (c.act > 1) { set_error("%s: act %d is not 0 (none) or 1 (ReLU)", what, c.act); return R3D_ERR_INVALID_ARG; }
        if (c.H() <= 0 || c.W() <= 0)
            { set_error("%s: no output: %d x %d with ksize %d, dilation %d, pad %d is smaller than one window", what, c.Hs, c.Ws, c.ksize, c.dilation, c.pad);
              return R3D_ERR_INVALID_ARG; }
        if (c.bias_bstride != 0 && c.bias_bstride < c.Cout)
            { set_error("%s: bias_bstride %d is not 0 or at least Cout = %d", what, c.bias_bstride, c.Cout); return R3D_ERR_INVALID_ARG; }
        if (c.res && c.res == c.y && (c.ycs != c.Cout || c.yco != 0))
            { set_error("%s: the residual [M, %d] cannot be y with rows of %d floats at channel %d", what, c.Cout, c.ycs, c.yco); return R3D_ERR_INVALID_ARG; }
        if ((double)c.B * c.Hs * c.Ws * c.Cin > 9.0e18) { set_error("%s: more than 2^63 input elements", what); return R3D_ERR_INVALID_ARG; }
    }
    const int H = c.H(), W = c.W(), Do = c.Do();
    if (c.pool && (H % 2 || W % 2)) { set_error("%s: pooling an odd size (%d x %d)", what, H, W); return R3D_ERR_INVALID_ARG; }
    if (c.pool && (c.yn || !c.y)) { set_error("%s: the pooled output is channel-last only (y, not y_ncdhw)", what); return R3D_ERR_INVALID_ARG; }
    if (c.y && (c.yco < 0 || c.ycs < c.yco + c.Cout))
        { set_error("%s: channel slice [%d, %d + %d) does not fit rows of %d", what, c.yco, c.yco, c.Cout, c.ycs); return R3D_ERR_INVALID_ARG; }
    if (c.split < 1 || c.Cout % c.split) { set_error("%s: Cout %d is not a multiple of depth %d (>= 1)", what, c.Cout, c.split); return R3D_ERR_INVALID_ARG; }
    if ((double)c.B * Do * H * W > 2147483647.0 || (double)c.B * c.D * H * W * (c.Cin > c.Cout ? c.Cin : c.Cout) > 9.0e18 ||
        (double)c.B * Do * H * W * (c.y ? c.ycs : 1) > 9.0e18)
        { set_error("%s: more than 2^31 - 1 output positions", what); return R3D_ERR_INVALID_ARG; }
    const size_t nin = (size_t)c.B * c.D * c.Hs * c.Ws * c.Cin, nw = (size_t)c.Cout * c.kd() * c.ksize * c.ksize * c.Cin;
    const size_t rows = (size_t)c.B * Do * (H >> c.pool) * (W >> c.pool), ny = rows * (size_t)(c.y ? c.ycs : 0), nyn = rows * c.Cout;
    for (int o = 0; o < 2; ++o) {          // (an output, a bias or a prologue that is absent takes no part)
        const float* p = o ? c.yn : c.y;
        const size_t np = o ? nyn : ny;
        const size_t nbias = (size_t)(c.B - 1) * c.bias_bstride + c.Cout;          // bias_bstride is 0 outside dl
        const size_t npro = (size_t)(c.rp ? c.B : 1) * c.Cin;
        const Span spans[] = {writes(p, np), reads(c.x, nin), reads(c.w, nw), reads(c.bias, nbias), reads(c.ps, npro), reads(c.pt, npro)};
        if (clash(spans)) { set_error("%s: an output overlaps x, w, bias or the prologue", what); return R3D_ERR_INVALID_ARG; }
        if (c.res != c.y && overlap(p, np, c.res, nyn))
            { set_error("%s: an output overlaps the residual without y being the residual", what); return R3D_ERR_INVALID_ARG; }
    }
    if (overlap(c.y, ny, c.yn, nyn))
        { set_error("%s: y and %s overlap", what, c.volume ? "y_ncdhw" : "y_nchw"); return R3D_ERR_INVALID_ARG; }
    return R3D_OK;
}

template <class F, int PREC, bool VEC, int WM, int WN, int TM, int TN>
void launch(ConvArgs g, hipStream_t st)
{
    constexpr int BM = WM * TM * 16, BN = WN * TN * 16;
    g.ntn = (g.Cout + BN - 1) / BN;
    g.ntm = (g.M + BM - 1) / BM;          // read by the 3-D bodies only
    const long long nblk = (long long)g.ntm * g.ntn;
    hipLaunchKernelGGL((F::template kernel<PREC, VEC, WM, WN, TM, TN>()), dim3((unsigned)nblk), dim3(256), 0, st, g);
}

// The tile follows Cout: 64 x 64 (positions x channels) or 32 x 64, 128 x 32 up to 32 channels, 128 x 16 up to 16 (out_conv's 3, the predictor's 1).
// 32 x 64 where 64 x 64 tiles would give the 256 CUs fewer than two blocks each (the 64^2 layers; one wave per SIMD otherwise); in the 3-D
// families 64 x 16 where 128 x 16 tiles would leave most CUs without a block.  Every BM is a multiple of 4: a pooling window never
// straddles two tiles.
template <class F, int PREC, bool VEC>
void dispatch(const ConvArgs& g, hipStream_t st)
{
    const long long big = (long long)((g.M + 63) / 64) * ((g.Cout + 63) / 64);
    if (g.Cout > 32 && big < 512) return launch<F, PREC, VEC, 2, 2, 1, 2>(g, st);
    if (g.Cout > 32) return launch<F, PREC, VEC, 2, 2, 2, 2>(g, st);
    if (g.Cout > 16) return launch<F, PREC, VEC, 4, 1, 2, 2>(g, st);
    if constexpr (F::tile64x16)
        if ((g.M + 127) / 128 < 256) return launch<F, PREC, VEC, 4, 1, 1, 1>(g, st);
    launch<F, PREC, VEC, 4, 1, 2, 1>(g, st);
}

// check, fill, pick the loader and the tier, launch.  VEC: channel-last input, Cin % 4 == 0 and 16-byte aligned x, w and prologue
// vectors: 16-byte loads; otherwise one element per load (NCHW input, Cin = 65, 3, 1).
template <class F>
int run(const char* what, const ConvCall& c, r3d_stream_t stream)
{
    if (int rc = check_conv(what, c)) return rc;
    ConvArgs g = {};
    c.fill(g);
    hipStream_t st = (hipStream_t)stream;
    const bool vec = !c.in_nchw && c.Cin % 4 == 0 && aligned16(c.x) && aligned16(c.w) && aligned16(c.ps) && aligned16(c.pt);
    if (c.precision == R3D_TORSO_BF16X3) { if (vec) dispatch<F, tconv::BF16X3, true>(g, st); else dispatch<F, tconv::BF16X3, false>(g, st); }
    else { if (vec) dispatch<F, tconv::F32, true>(g, st); else dispatch<F, tconv::F32, false>(g, st); }
    return check_launch(what);
}

}  // namespace tlaunch
}  // namespace r3d
