// The appearance feature extractor of the face-vid2vid torso network (modules/real3d/facev2v_warp/network2.py:16-45), inference only
// (DESIGN 4.12).  Activations are channel-last fp32.  Its first layer is r3d_torso_conv; the other fifteen run on
//   tappear::conv<VEC, WM, WN, TM, TN>      the D3 = true, EXT = true instantiation of conv_tile (r3d_torso_conv.h): the 3-D body with a
//                                           residual and the depth-split store in its epilogue.  A 2-D layer is that body with D = 1 and ONE
//                                           depth tap (kd = 1, K = ks ks Cin: no zero taps), which gives it the quad-major 2 x 2 average pool.
//   tappear_bf3::conv<...>                  the same tiles with the products on the BF16X3 tier.
// behind three entry points: r3d_torso_conv_pool (DownBlock2D), r3d_torso_conv_split (mid_conv + view) and r3d_torso_conv3d_res (the convs
// of ResBlock3D).  The order of every sum is conv_tile's, so with the additions off each equals r3d_torso_conv / r3d_torso_conv3d bit for bit.
#include "r3d_common.h"
#include "r3d_torso_conv.h"

namespace r3d {
namespace tappear {

using tconv::ConvArgs;

template <bool VEC, int WM, int WN, int TM, int TN>
__global__ void __launch_bounds__(256) conv(ConvArgs g) { tconv::conv_tile<tconv::F32, VEC, true, WM, WN, TM, TN, true>(g); }

}  // namespace tappear

namespace tappear_bf3 {

template <bool VEC, int WM, int WN, int TM, int TN>
__global__ void __launch_bounds__(256) conv(tconv::ConvArgs g) { tconv::conv_tile<tconv::BF16X3, VEC, true, WM, WN, TM, TN, true>(g); }

}  // namespace tappear_bf3

namespace tappear {

template <int PREC, bool VEC, int WM, int WN, int TM, int TN>
static void launch(ConvArgs g, hipStream_t st)
{
    constexpr int BM = WM * TM * 16, BN = WN * TN * 16;
    g.ntn = (g.Cout + BN - 1) / BN;
    g.ntm = (g.M + BM - 1) / BM;
    const long long nblk = (long long)g.ntm * g.ntn;
    if constexpr (PREC == tconv::BF16X3) hipLaunchKernelGGL((tappear_bf3::conv<VEC, WM, WN, TM, TN>), dim3((unsigned)nblk), dim3(256), 0, st, g);
    else hipLaunchKernelGGL((conv<VEC, WM, WN, TM, TN>), dim3((unsigned)nblk), dim3(256), 0, st, g);
}

// the tile follows Cout as in r3d_torso_conv3d (every BM is a multiple of 4: a pooling window never straddles two tiles)
template <int PREC>
static void dispatch(const ConvArgs& g, bool vec, hipStream_t st)
{
    const long long big = (long long)((g.M + 63) / 64) * ((g.Cout + 63) / 64);
    if (g.Cout > 32 && big < 512) { if (vec) launch<PREC, true, 2, 2, 1, 2>(g, st); else launch<PREC, false, 2, 2, 1, 2>(g, st); }
    else if (g.Cout > 32) { if (vec) launch<PREC, true, 2, 2, 2, 2>(g, st); else launch<PREC, false, 2, 2, 2, 2>(g, st); }
    else if (g.Cout > 16) { if (vec) launch<PREC, true, 4, 1, 2, 2>(g, st); else launch<PREC, false, 4, 1, 2, 2>(g, st); }
    else if ((g.M + 127) / 128 < 256) { if (vec) launch<PREC, true, 4, 1, 1, 1>(g, st); else launch<PREC, false, 4, 1, 1, 1>(g, st); }
    else { if (vec) launch<PREC, true, 4, 1, 2, 1>(g, st); else launch<PREC, false, 4, 1, 2, 1>(g, st); }
}

}  // namespace tappear
}  // namespace r3d

using namespace r3d;
using namespace r3d::tappear;

// [a, a + na) and [b, b + nb) (counts of floats) share an element
static bool overlap(const float* a, size_t na, const float* b, size_t nb) { return a < b + nb && b < a + na; }
static bool aligned16(const void* p) { return p == nullptr || ((uintptr_t)p & 15) == 0; }

// what the three entry points check alike; H x W is the conv's grid, D its depth (1 for the 2-D layers)
static int common_checks(const char* what, const float* x, const float* w, int B, int D, int H, int W, int Cin, int Cout, int ksize, int act,
                         int precision)
{
    if (precision != R3D_TORSO_F32 && precision != R3D_TORSO_BF16X3)
        { set_error("%s: precision %d is not 0 (R3D_TORSO_F32) or 1 (R3D_TORSO_BF16X3)", what, precision); return R3D_ERR_INVALID_ARG; }
    if (!x || !w) { set_error("%s: NULL pointer", what); return R3D_ERR_INVALID_ARG; }
    if (B <= 0 || D <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || Cin > 4096 || Cout > 4096 || D > 1024)
        { set_error("%s: bad argument (B, Hs, Ws > 0, 1 <= D <= 1024, 1 <= Cin, Cout <= 4096)", what); return R3D_ERR_INVALID_ARG; }
    if (ksize != 1 && ksize != 3 && ksize != 7) { set_error("%s: ksize %d is not 1, 3 or 7", what, ksize); return R3D_ERR_INVALID_ARG; }
    if (act < 0 || act > 2) { set_error("%s: act %d is not 0 (none), 1 (leaky) or 2 (sigmoid)", what, act); return R3D_ERR_INVALID_ARG; }
    if ((double)B * D * H * W > 2147483647.0 || (double)B * D * H * W * (Cin > Cout ? Cin : Cout) > 9.0e18)
        { set_error("%s: more than 2^31 - 1 output positions", what); return R3D_ERR_INVALID_ARG; }
    return R3D_OK;
}

static void run(const ConvArgs& g, bool vec, int precision, hipStream_t st)
{
    if (precision == R3D_TORSO_BF16X3) dispatch<tconv::BF16X3>(g, vec, st);
    else dispatch<tconv::F32>(g, vec, st);
}

// a 2-D layer on the 3-D body: one depth, one depth tap
static ConvArgs args2d(const float* x, int B, int Hs, int Ws, int Cin, int in_nchw, const float* w, const float* bias, int Cout, int ksize,
                       int act, float act_slope, float* y)
{
    ConvArgs g = {};
    g.x = x; g.B = B; g.Hs = Hs; g.Ws = Ws; g.Cin = Cin; g.H = Hs; g.W = Ws; g.in_nchw = in_nchw ? 1 : 0; g.ks = ksize;
    g.w = w; g.Cout = Cout; g.bias = bias; g.act = act; g.slope = act_slope; g.y = y;
    g.D = 1; g.Do = 1; g.kd = 1; g.padz = 0; g.ycs = Cout; g.yco = 0;
    g.M = B * Hs * Ws; g.K = ksize * ksize * Cin;
    return g;
}

extern "C" int r3d_torso_conv_pool(const float* x, int B, int Hs, int Ws, int Cin, int in_nchw, const float* w, const float* bias, int Cout,
                                   int ksize, int act, float act_slope, int pool, float* y, int precision, r3d_stream_t stream)
{
    if (int rc = common_checks("torso_conv_pool", x, w, B, 1, Hs, Ws, Cin, Cout, ksize, act, precision)) return rc;
    if (!y) { set_error("torso_conv_pool: NULL pointer"); return R3D_ERR_INVALID_ARG; }
    if (pool != 0 && pool != 1) { set_error("torso_conv_pool: pool %d is not 0 or 1", pool); return R3D_ERR_INVALID_ARG; }
    if (pool && (Hs % 2 || Ws % 2)) { set_error("torso_conv_pool: pooling an odd size (%d x %d)", Hs, Ws); return R3D_ERR_INVALID_ARG; }
    const size_t nin = (size_t)B * Hs * Ws * Cin, nw = (size_t)Cout * ksize * ksize * Cin, ny = (size_t)B * (Hs >> pool) * (Ws >> pool) * Cout;
    if (overlap(y, ny, x, nin) || overlap(y, ny, w, nw) || (bias && overlap(y, ny, bias, Cout)))
        { set_error("torso_conv_pool: y overlaps x, w or bias"); return R3D_ERR_INVALID_ARG; }
    ConvArgs g = args2d(x, B, Hs, Ws, Cin, in_nchw, w, bias, Cout, ksize, act, act_slope, y);
    g.pool = pool;
    run(g, !in_nchw && Cin % 4 == 0 && aligned16(x) && aligned16(w), precision, (hipStream_t)stream);
    return check_launch("torso_conv_pool");
}

extern "C" int r3d_torso_conv_split(const float* x, int B, int Hs, int Ws, int Cin, int in_nchw, const float* w, const float* bias, int Cout,
                                    int ksize, int act, float act_slope, int depth, float* y, int precision, r3d_stream_t stream)
{
    if (int rc = common_checks("torso_conv_split", x, w, B, 1, Hs, Ws, Cin, Cout, ksize, act, precision)) return rc;
    if (!y) { set_error("torso_conv_split: NULL pointer"); return R3D_ERR_INVALID_ARG; }
    if (depth < 1 || Cout % depth) { set_error("torso_conv_split: Cout %d is not a multiple of depth %d (>= 1)", Cout, depth); return R3D_ERR_INVALID_ARG; }
    const size_t nin = (size_t)B * Hs * Ws * Cin, nw = (size_t)Cout * ksize * ksize * Cin, ny = (size_t)B * Hs * Ws * Cout;
    if (overlap(y, ny, x, nin) || overlap(y, ny, w, nw) || (bias && overlap(y, ny, bias, Cout)))
        { set_error("torso_conv_split: y overlaps x, w or bias"); return R3D_ERR_INVALID_ARG; }
    ConvArgs g = args2d(x, B, Hs, Ws, Cin, in_nchw, w, bias, Cout, ksize, act, act_slope, y);
    g.split = depth;
    run(g, !in_nchw && Cin % 4 == 0 && aligned16(x) && aligned16(w), precision, (hipStream_t)stream);
    return check_launch("torso_conv_split");
}

extern "C" int r3d_torso_conv3d_res(const float* x, int B, int D, int Hs, int Ws, int Cin, const float* pro_scale, const float* pro_shift,
                                    float pro_slope, const float* w, const float* bias, int Cout, int ksize, int act, float act_slope,
                                    const float* residual, float* y, float* y_ncdhw, int precision, r3d_stream_t stream)
{
    if (int rc = common_checks("torso_conv3d_res", x, w, B, D, Hs, Ws, Cin, Cout, ksize, act, precision)) return rc;
    if ((!y && !y_ncdhw) || (!pro_scale) != (!pro_shift)) { set_error("torso_conv3d_res: NULL pointer"); return R3D_ERR_INVALID_ARG; }
    const size_t nin = (size_t)B * D * Hs * Ws * Cin, nw = (size_t)Cout * ksize * ksize * ksize * Cin, nout = (size_t)B * D * Hs * Ws * Cout;
    for (float* o : {y, y_ncdhw}) {
        if (!o) continue;
        if (overlap(o, nout, x, nin) || overlap(o, nout, w, nw) || (bias && overlap(o, nout, bias, Cout)) ||
            (pro_scale && (overlap(o, nout, pro_scale, Cin) || overlap(o, nout, pro_shift, Cin))))
            { set_error("torso_conv3d_res: an output overlaps x, w, bias or the prologue"); return R3D_ERR_INVALID_ARG; }
        if (residual && residual != y && overlap(o, nout, residual, nout))
            { set_error("torso_conv3d_res: an output overlaps the residual without y being the residual"); return R3D_ERR_INVALID_ARG; }
    }
    if (y && y_ncdhw && overlap(y, nout, y_ncdhw, nout)) { set_error("torso_conv3d_res: y and y_ncdhw overlap"); return R3D_ERR_INVALID_ARG; }
    ConvArgs g = {};
    g.x = x; g.B = B; g.Hs = Hs; g.Ws = Ws; g.Cin = Cin; g.H = Hs; g.W = Ws; g.ks = ksize;
    g.ps = pro_scale; g.pt = pro_shift; g.pslope = pro_slope;
    g.w = w; g.Cout = Cout; g.bias = bias; g.act = act; g.slope = act_slope; g.res = residual; g.y = y; g.y_nchw = y_ncdhw;
    g.D = D; g.Do = D; g.kd = ksize; g.padz = ksize / 2; g.ycs = Cout; g.yco = 0;
    g.M = B * D * Hs * Ws; g.K = ksize * ksize * ksize * Cin;
    g.mfast = g.M < Cout;
    const bool vec = Cin % 4 == 0 && aligned16(x) && aligned16(w) && aligned16(pro_scale) && aligned16(pro_shift);
    run(g, vec, precision, (hipStream_t)stream);
    return check_launch("torso_conv3d_res");
}
