// The second half of the face-vid2vid torso network, inference only, exact fp32: Generator (modules/real3d/facev2v_warp/
// network2.py:248-301) = a trilinear warp of the appearance volume + a 2D decoder, and occlusion_2_predictor (model2.py:212-219).
//
// Activations are channel-last fp32.  Every product of the convolutions runs on v_mfma_f32_16x16x4_f32 (exact f32 products, an fmaf chain
// per k step); the warp, the prologue and the epilogues run on the fp32 VALU.  Kernels:
//   torso_volume_to_cl   [N, C, D, H, W] -> [N, D, H, W, C]: the clip-constant source of the warp, so that one tap is one contiguous read
//                        of the C channels.
//   torso_warp           F.grid_sample(fs, grid, align_corners=True, padding_mode='border') on the 5-D volume, 8 taps per output value.
//   torso_conv<VEC, WM, WN, TM, TN>
//                        (the D3 = false instantiation of conv_tile, r3d_torso_conv.h) implicit-GEMM stride-1 convolution, zero padding ksize / 2: a (WM TM 16) x (WN TN 16) tile of pixels x output
//                        channels per 256-thread block, K = (ky, kx, ci) staged 32 at a time through two LDS buffers while the next two
//                        steps are in flight in registers.  Tap loads apply the prologue act(s[c] x + t[c]) (zero outside the image AFTER it:
//                        the reference pads the activated tensor) and nearest x2 up-sampling in the addressing; the epilogue adds the bias,
//                        applies LeakyReLU / sigmoid, adds a residual and writes channel-last and / or NCHW.  VEC: Cin % 4 == 0,
//                        channel-last input, 16-byte loads; otherwise one element per load (NCHW input, Cin = 65, 3, 1).
//   torso_bf3::torso_conv<...>  the same tiles with the products on the BF16X3 tier (r3d_torso_conv_prec), and
//   torso_bf3::torso_split      that tier's split of a plain array (r3d_torso_split_bf16x3, for the tests).
// r3d_torso_conv / _prec describe their call and hand it, with this unit's kernel family, to the argument check, the tile table and the
// launcher all seven torso conv entry points share (r3d_torso_launch.h).
#include "r3d_common.h"
#include "r3d_torso_launch.h"
#include <math.h>

namespace r3d {
namespace torso {

__global__ void __launch_bounds__(256) torso_volume_to_cl(const float* fs, int C, size_t DHW, size_t total, float* out)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C);
    const size_t p = i / C, n = p / DHW, s = p - n * DHW;
    out[i] = fs[(n * C + c) * DHW + s];
}

struct WarpArgs {
    const float* src; int N, C, D, H, W;        // [N, D, H, W, C]
    const float* grid; int Do, Ho, Wo;          // [N, Do, Ho, Wo, 3]: component 0 indexes W, 1 H, 2 D
    float* out; int channel_last;               // [N, C, Do, Ho, Wo], or [N, Ho, Wo, C Do] with channel c Do + d
};

// the source coordinate of a normalised one (align_corners=True), clipped to the volume (padding_mode='border'): the lower corner and
// the weight of the upper one; an upper corner equal to `size` has weight 0 and is not read
__device__ __forceinline__ void warp_axis(float g, int size, int& i0, float& f)
{
    float x = ((g + 1.0f) * 0.5f) * (float)(size - 1);
    x = fminf(fmaxf(x, 0.0f), (float)(size - 1));
    const float fl = floorf(x);
    i0 = (int)fl;
    f = x - fl;
}

__global__ void __launch_bounds__(256) torso_warp(WarpArgs a)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, total = (size_t)a.N * a.Do * a.Ho * a.Wo * a.C;
    if (i >= total) return;
    const int c = (int)(i % a.C);
    size_t p = i / a.C;                          // point index ((n Do + d) Ho + h) Wo + w
    const float* g = a.grid + p * 3;
    int x0, y0, z0;
    float fx, fy, fz;
    warp_axis(g[0], a.W, x0, fx);
    warp_axis(g[1], a.H, y0, fy);
    warp_axis(g[2], a.D, z0, fz);
    const int w = (int)(p % a.Wo); p /= a.Wo;
    const int h = (int)(p % a.Ho); p /= a.Ho;
    const int d = (int)(p % a.Do);
    const size_t n = p / a.Do;
    const float* s = a.src + n * a.D * a.H * a.W * a.C + c;
    float acc = 0.0f;
#pragma unroll
    for (int dz = 0; dz < 2; ++dz) {
        const float wz = dz ? fz : 1.0f - fz;
        if (z0 + dz >= a.D) continue;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            const float wy = dy ? fy : 1.0f - fy;
            if (y0 + dy >= a.H) continue;
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const float wx = dx ? fx : 1.0f - fx;
                if (x0 + dx >= a.W) continue;
                acc = fmaf(s[(((size_t)(z0 + dz) * a.H + (y0 + dy)) * a.W + (x0 + dx)) * a.C], wx * wy * wz, acc);
            }
        }
    }
    const size_t hw = (size_t)a.Ho * a.Wo, px = (size_t)h * a.Wo + w;
    if (a.channel_last) a.out[(n * hw + px) * ((size_t)a.C * a.Do) + (size_t)c * a.Do + d] = acc;
    else a.out[((n * a.C + c) * a.Do + d) * hw + px] = acc;
}

using tconv::ConvArgs;

// the 2-D instantiation of the shared tile (r3d_torso_conv.h)
template <bool VEC, int WM, int WN, int TM, int TN>
__global__ void __launch_bounds__(256) torso_conv(ConvArgs g) { tconv::conv_tile<tconv::F32, VEC, false, WM, WN, TM, TN>(g); }

}  // namespace torso

// the kernels of the BF16X3 tier (R3D_TORSO_BF16X3)
namespace torso_bf3 {

template <bool VEC, int WM, int WN, int TM, int TN>
__global__ void __launch_bounds__(256) torso_conv(tconv::ConvArgs g) { tconv::conv_tile<tconv::BF16X3, VEC, false, WM, WN, TM, TN>(g); }

// r3d_torso_split_bf16x3: the staging split of the tier, one element per thread
__global__ void __launch_bounds__(256) torso_split(const float* x, size_t n, uint16_t* h, uint16_t* m, uint16_t* l)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) tconv::split_bf16x3(x[i], h[i], m[i], l[i]);
}

}  // namespace torso_bf3

namespace torso {

// this unit's kernel family for tlaunch::run (r3d_torso_launch.h): the 2-D body
struct Family {
    static constexpr bool tile64x16 = false;
    template <int PREC, bool VEC, int WM, int WN, int TM, int TN>
    static void (*kernel())(ConvArgs)
    {
        if constexpr (PREC == tconv::BF16X3) return torso_bf3::torso_conv<VEC, WM, WN, TM, TN>;
        else return torso_conv<VEC, WM, WN, TM, TN>;
    }
};

}  // namespace torso
}  // namespace r3d

using namespace r3d;
using namespace r3d::torso;

extern "C" int r3d_torso_volume_to_cl(const float* fs, int N, int C, int D, int H, int W, float* out, r3d_stream_t stream)
{
    if (!fs || !out) { set_error("torso_volume_to_cl: NULL pointer"); return R3D_ERR_INVALID_ARG; }
    if (N <= 0 || C <= 0 || D <= 0 || H <= 0 || W <= 0 || (double)N * C * D * H * W > 2147483647.0)
        { set_error("torso_volume_to_cl: bad argument (positive sizes, fewer than 2^31 elements)"); return R3D_ERR_INVALID_ARG; }
    const size_t dhw = (size_t)D * H * W, total = (size_t)N * C * dhw;
    if (overlap(fs, total, out, total)) { set_error("torso_volume_to_cl: fs and out overlap"); return R3D_ERR_INVALID_ARG; }
    hipLaunchKernelGGL(torso_volume_to_cl, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, fs, C, dhw, total, out);
    return check_launch("torso_volume_to_cl");
}

extern "C" int r3d_torso_warp(const float* fs_cl, int N, int C, int D, int H, int W, const float* grid, int Do, int Ho, int Wo,
                              float* out, int channel_last, r3d_stream_t stream)
{
    if (!fs_cl || !grid || !out) { set_error("torso_warp: NULL pointer"); return R3D_ERR_INVALID_ARG; }
    if (N <= 0 || C <= 0 || D <= 0 || H <= 0 || W <= 0 || Do <= 0 || Ho <= 0 || Wo <= 0 || (double)N * C * D * H * W > 2147483647.0 ||
        (double)N * C * Do * Ho * Wo > 2147483647.0)
        { set_error("torso_warp: bad argument (positive sizes, fewer than 2^31 elements)"); return R3D_ERR_INVALID_ARG; }
    const size_t nsrc = (size_t)N * C * D * H * W, npts = (size_t)N * Do * Ho * Wo, nout = npts * C;
    if (overlap(out, nout, fs_cl, nsrc) || overlap(out, nout, grid, npts * 3)) { set_error("torso_warp: out overlaps an input"); return R3D_ERR_INVALID_ARG; }
    WarpArgs a = {fs_cl, N, C, D, H, W, grid, Do, Ho, Wo, out, channel_last ? 1 : 0};
    hipLaunchKernelGGL(torso_warp, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    return check_launch("torso_warp");
}

extern "C" int r3d_torso_conv_prec(const float* x, int B, int Hs, int Ws, int Cin, int in_nchw, int upsample, const float* pro_scale,
                                   const float* pro_shift, float pro_slope, const float* w, const float* bias, int Cout, int ksize, int act,
                                   float act_slope, const float* residual, float* y, float* y_nchw, int precision, r3d_stream_t stream)
{
    tlaunch::ConvCall c = tlaunch::conv_call(x, B, Hs, Ws, Cin, w, bias, Cout, ksize, act, act_slope, y, precision);
    c.in_nchw = in_nchw; c.upsample = upsample; c.ps = pro_scale; c.pt = pro_shift; c.pslope = pro_slope; c.res = residual; c.yn = y_nchw;
    return tlaunch::run<Family>("torso_conv", c, stream);
}

extern "C" int r3d_torso_conv(const float* x, int B, int Hs, int Ws, int Cin, int in_nchw, int upsample, const float* pro_scale,
                              const float* pro_shift, float pro_slope, const float* w, const float* bias, int Cout, int ksize, int act,
                              float act_slope, const float* residual, float* y, float* y_nchw, r3d_stream_t stream)
{
    return r3d_torso_conv_prec(x, B, Hs, Ws, Cin, in_nchw, upsample, pro_scale, pro_shift, pro_slope, w, bias, Cout, ksize, act, act_slope,
                               residual, y, y_nchw, R3D_TORSO_F32, stream);
}

extern "C" int r3d_torso_split_bf16x3(const float* x, size_t n, uint16_t* h, uint16_t* m, uint16_t* l, r3d_stream_t stream)
{
    if (!x || !h || !m || !l) { set_error("torso_split_bf16x3: NULL pointer"); return R3D_ERR_INVALID_ARG; }
    if (n == 0 || n > 2147483647u) { set_error("torso_split_bf16x3: n is not in 1 .. 2^31 - 1"); return R3D_ERR_INVALID_ARG; }
    const Span spans[4] = {reads(x, n), writes(h, n), writes(m, n), writes(l, n)};
    for (int i = 1; i < 4; ++i) {          // every output against x, then against the outputs before it
        const Span with_x[2] = {spans[0], spans[i]};
        if (clash(with_x)) { set_error("torso_split_bf16x3: an output overlaps x"); return R3D_ERR_INVALID_ARG; }
        if (clash(spans + 1, i)) { set_error("torso_split_bf16x3: two outputs overlap"); return R3D_ERR_INVALID_ARG; }
    }
    hipLaunchKernelGGL(torso_bf3::torso_split, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, n, h, m, l);
    return check_launch("torso_split_bf16x3");
}
