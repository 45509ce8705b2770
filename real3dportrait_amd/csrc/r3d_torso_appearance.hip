// The appearance feature extractor of the face-vid2vid torso network (modules/real3d/facev2v_warp/network2.py:16-45), inference only
// (DESIGN 4.12).  Activations are channel-last fp32.  Its first layer is r3d_torso_conv; the other fifteen run on
//   tappear::conv<VEC, WM, WN, TM, TN>      the D3 = true, EXT = true instantiation of conv_tile (r3d_torso_conv.h): the 3-D body with a
//                                           residual and the depth-split store in its epilogue.  A 2-D layer is that body with D = 1 and ONE
//                                           depth tap (kd = 1, K = ks ks Cin: no zero taps), which gives it the quad-major 2 x 2 average pool.
//   tappear_bf3::conv<...>                  the same tiles with the products on the BF16X3 tier.
// behind three entry points: r3d_torso_conv_pool (DownBlock2D), r3d_torso_conv_split (mid_conv + view) and r3d_torso_conv3d_res (the convs
// of ResBlock3D).  The order of every sum is conv_tile's, so with the additions off each equals r3d_torso_conv / r3d_torso_conv3d bit for bit.
// Each describes its call and hands it, with this unit's kernel family, to the shared check, tile table and launcher (r3d_torso_launch.h).
#include "r3d_common.h"
#include "r3d_torso_launch.h"

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

// this unit's kernel family for tlaunch::run (r3d_torso_launch.h): the 3-D body with the extended epilogue
struct Family {
    static constexpr bool tile64x16 = true;
    template <int PREC, bool VEC, int WM, int WN, int TM, int TN>
    static void (*kernel())(ConvArgs)
    {
        if constexpr (PREC == tconv::BF16X3) return tappear_bf3::conv<VEC, WM, WN, TM, TN>;
        else return conv<VEC, WM, WN, TM, TN>;
    }
};

}  // namespace tappear
}  // namespace r3d

using namespace r3d;
using namespace r3d::tappear;

// A 2-D layer (conv_pool, conv_split) is the 3-D body with one depth and one depth tap: ConvCall's defaults.

extern "C" int r3d_torso_conv_pool(const float* x, int B, int Hs, int Ws, int Cin, int in_nchw, const float* w, const float* bias, int Cout,
                                   int ksize, int act, float act_slope, int pool, float* y, int precision, r3d_stream_t stream)
{
    tlaunch::ConvCall c = tlaunch::conv_call(x, B, Hs, Ws, Cin, w, bias, Cout, ksize, act, act_slope, y, precision);
    c.in_nchw = in_nchw; c.pool = pool;
    return tlaunch::run<Family>("torso_conv_pool", c, stream);
}

extern "C" int r3d_torso_conv_split(const float* x, int B, int Hs, int Ws, int Cin, int in_nchw, const float* w, const float* bias, int Cout,
                                    int ksize, int act, float act_slope, int depth, float* y, int precision, r3d_stream_t stream)
{
    tlaunch::ConvCall c = tlaunch::conv_call(x, B, Hs, Ws, Cin, w, bias, Cout, ksize, act, act_slope, y, precision);
    c.in_nchw = in_nchw; c.split = depth;
    return tlaunch::run<Family>("torso_conv_split", c, stream);
}

extern "C" int r3d_torso_conv3d_res(const float* x, int B, int D, int Hs, int Ws, int Cin, const float* pro_scale, const float* pro_shift,
                                    float pro_slope, const float* w, const float* bias, int Cout, int ksize, int act, float act_slope,
                                    const float* residual, float* y, float* y_ncdhw, int precision, r3d_stream_t stream)
{
    tlaunch::ConvCall c = tlaunch::conv_call(x, B, Hs, Ws, Cin, w, bias, Cout, ksize, act, act_slope, y, precision);
    c.D = D; c.volume = true; c.ps = pro_scale; c.pt = pro_shift; c.pslope = pro_slope; c.res = residual; c.yn = y_ncdhw;
    return tlaunch::run<Family>("torso_conv3d_res", c, stream);
}
