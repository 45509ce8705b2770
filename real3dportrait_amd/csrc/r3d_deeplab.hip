// DeepLabV3, the low-resolution encoder of Img2PlaneModel (modules/img2plane/deeplabv3/decoders/my_model.py: a ResNet dilated to output
// stride 8, ASPP, one 3 x 3 conv), inference only, exact fp32 (include/r3d_hip_deeplab.h).  Kernels:
//   dl_conv<VEC, WM, WN, TM, TN>  nn.Conv2d with a stride, a dilation and an explicit padding on v_mfma_f32_16x16x4_f32: the shared tile of
//                                 r3d_torso_conv.h with its DL flag, through the launcher, tile table and argument check of
//                                 r3d_torso_launch.h.  Epilogue sum + bias[b] + residual, then ReLU, into a channel slice.
//   dl_maxpool                    nn.MaxPool2d(3, 2, 1), channel-last; padding is -inf, a NaN in a window gives NaN.
//   dl_global_mean                nn.AdaptiveAvgPool2d(1): per (sample, channel) an fp64 sum in a fixed order.
//   dl_assemble_input             rgb | alpha | camera | row / H | col / H, channel-last, from the NCHW image (img2plane_model.py:52-64).
#include "r3d_common.h"
#include "r3d_torso_launch.h"
#include "../../include/r3d_hip_deeplab.h"
#include <math.h>

namespace r3d {
namespace deeplab {

using tconv::ConvArgs;

template <bool VEC, int WM, int WN, int TM, int TN>
__global__ void __launch_bounds__(256) dl_conv(ConvArgs g) { tconv::conv_tile<tconv::F32, VEC, false, WM, WN, TM, TN, false, true>(g); }

// this unit's kernel family for tlaunch::dispatch: the strided, dilated 2-D body, fp32 only
struct Family {
    static constexpr bool tile64x16 = false;
    template <int PREC, bool VEC, int WM, int WN, int TM, int TN>
    static void (*kernel())(ConvArgs)
    {
        static_assert(PREC == tconv::F32, "r3d_dl_conv has no bf16x3 tier");
        return dl_conv<VEC, WM, WN, TM, TN>;
    }
};

__global__ void __launch_bounds__(256) dl_maxpool(const float* x, int H, int W, int C, int Ho, int Wo, size_t total, float* y)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;          // over [B, Ho, Wo, C]
    if (i >= total) return;
    const int c = (int)(i % C);
    const size_t p = i / C;
    const int ox = (int)(p % Wo), oy = (int)((p / Wo) % Ho);
    const size_t b = p / ((size_t)Wo * Ho);
    const float* s = x + b * H * W * C + c;
    float m = -INFINITY;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = 2 * oy - 1 + ky;
        if (iy < 0 || iy >= H) continue;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = 2 * ox - 1 + kx;
            if (ix < 0 || ix >= W) continue;
            const float v = s[((size_t)iy * W + ix) * C];
            if (v > m || v != v) m = v;          // a NaN stays: nothing compares greater than it
        }
    }
    y[i] = m;
}

// One block of 1024 lanes per (32 channels, sample): lane t sums rows t >> 5, (t >> 5) + 32, ... of channel t & 31 in fp64, and one lane per
// channel adds the 32 partial sums in their order.  The order depends on HW alone.  (At the product shape, 4 096 rows x 512 channels,
// that is 16 blocks of 128 rows per lane; 64 channels x 4 row phases in 256 lanes measured 0.24 ms, 7 % of the module.)
constexpr int GM_C = 32, GM_P = 32;
__global__ void __launch_bounds__(GM_C * GM_P) dl_global_mean(const float* x, int HW, int C, float* y)
{
    __shared__ double part[GM_P][GM_C + 1];
    const int t = threadIdx.x, lc = t % GM_C, c = blockIdx.x * GM_C + lc, ph = t / GM_C, b = blockIdx.y;
    double s = 0.0;
    if (c < C) {
        const float* p = x + (size_t)b * HW * C + c;
        for (int r = ph; r < HW; r += GM_P) s += (double)p[(size_t)r * C];
    }
    part[ph][lc] = s;
    __syncthreads();
    if (ph == 0 && c < C) {
        double sum = part[0][lc];
        for (int q = 1; q < GM_P; ++q) sum += part[q][lc];
        y[(size_t)b * C + c] = (float)(sum / (double)HW);
    }
}

__global__ void __launch_bounds__(256) dl_assemble_input(const float* img, const float* alpha, const float* cam, int H, int W, int Cin, size_t total,
                                                         float* y)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;          // over [B, H, W, Cin]
    if (i >= total) return;
    const int c = (int)(i % Cin);
    const size_t p = i / Cin, hw = (size_t)H * W, b = p / hw, px = p - b * hw;
    const int na = alpha ? 1 : 0, nc = cam ? 3 : 0;
    float v;
    if (c < 3) v = img[(b * 3 + c) * hw + px];
    else if (c < 3 + na) v = alpha[b * hw + px];
    else if (c < 3 + na + nc) v = cam[b * 3 + (c - 3 - na)];
    else if (c == 3 + na + nc) v = (float)(int)(px / W) / (float)H;          // IEEE division of two exact integers: torch's arange(H) / H
    else v = (float)(int)(px % W) / (float)H;                                 // the reference divides the columns by H as well
    y[i] = v;
}

static inline dim3 grid_for(size_t total) { return dim3((unsigned)((total + 255) / 256)); }

}  // namespace deeplab
}  // namespace r3d

using namespace r3d;
using namespace r3d::deeplab;

extern "C" int r3d_dl_conv(const float* x, int B, int Hin, int Win, int Cin, const float* w, const float* bias, int bias_bstride, int Cout, int ksize,
                           int stride, int dilation, int pad, const float* residual, int act, float* y, int ycs, int yco, r3d_stream_t stream)
{
    tlaunch::ConvCall c = tlaunch::conv_call(x, B, Hin, Win, Cin, w, bias, Cout, ksize, act, 0.0f, y, R3D_TORSO_F32);
    c.dl = true; c.stride = stride; c.dilation = dilation; c.pad = pad; c.bias_bstride = bias ? bias_bstride : 0; c.res = residual;
    c.ycs = ycs; c.yco = yco;
    if (int rc = tlaunch::check_conv("dl_conv", c)) return rc;
    ConvArgs g = {};
    c.fill(g);
    hipStream_t st = (hipStream_t)stream;
    if (Cin % 4 == 0 && aligned16(x) && aligned16(w)) tlaunch::dispatch<Family, tconv::F32, true>(g, st);
    else tlaunch::dispatch<Family, tconv::F32, false>(g, st);
    return check_launch("dl_conv");
}

extern "C" int r3d_dl_maxpool(const float* x, int B, int H, int W, int C, float* y, r3d_stream_t stream)
{
    if (!x || !y) { set_error("dl_maxpool: NULL pointer"); return R3D_ERR_INVALID_ARG; }
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0) { set_error("dl_maxpool: bad argument (B = %d, H = %d, W = %d, C = %d must be > 0)", B, H, W, C); return R3D_ERR_INVALID_ARG; }
    if (!below_2_31("dl_maxpool", "B H W C", (double)B * H * W * C, "elements")) return R3D_ERR_INVALID_ARG;
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const size_t nin = (size_t)B * H * W * C, total = (size_t)B * Ho * Wo * C;
    if (overlap(y, total, x, nin)) { set_error("dl_maxpool: x and y overlap"); return R3D_ERR_INVALID_ARG; }
    hipLaunchKernelGGL(dl_maxpool, grid_for(total), dim3(256), 0, (hipStream_t)stream, x, H, W, C, Ho, Wo, total, y);
    return check_launch("dl_maxpool");
}

extern "C" int r3d_dl_global_mean(const float* x, int B, int HW, int C, float* y, r3d_stream_t stream)
{
    if (!x || !y) { set_error("dl_global_mean: NULL pointer"); return R3D_ERR_INVALID_ARG; }
    if (B <= 0 || HW <= 0 || C <= 0 || B > 65535) { set_error("dl_global_mean: bad argument (B = %d in 1 .. 65535, HW = %d, C = %d > 0)", B, HW, C); return R3D_ERR_INVALID_ARG; }
    if (!below_2_31("dl_global_mean", "B HW C", (double)B * HW * C, "elements")) return R3D_ERR_INVALID_ARG;
    if (overlap(y, (size_t)B * C, x, (size_t)B * HW * C)) { set_error("dl_global_mean: x and y overlap"); return R3D_ERR_INVALID_ARG; }
    hipLaunchKernelGGL(dl_global_mean, dim3((C + GM_C - 1) / GM_C, B), dim3(GM_C * GM_P), 0, (hipStream_t)stream, x, HW, C, y);
    return check_launch("dl_global_mean");
}

extern "C" int r3d_dl_assemble_input(const float* img, const float* alpha, const float* camera_feat, int B, int H, int W, float* y, r3d_stream_t stream)
{
    if (!img || !y) { set_error("dl_assemble_input: NULL pointer"); return R3D_ERR_INVALID_ARG; }
    if (B <= 0 || H <= 0 || W <= 0) { set_error("dl_assemble_input: bad argument (B = %d, H = %d, W = %d must be > 0)", B, H, W); return R3D_ERR_INVALID_ARG; }
    if (H > (1 << 24) || W > (1 << 24)) { set_error("dl_assemble_input: %d x %d: a side above 2^24 is not an exact fp32 integer", H, W); return R3D_ERR_INVALID_ARG; }
    const int Cin = 3 + (alpha ? 1 : 0) + (camera_feat ? 3 : 0) + 2;
    if (!below_2_31("dl_assemble_input", "B H W Cin", (double)B * H * W * Cin, "elements")) return R3D_ERR_INVALID_ARG;
    const size_t hw = (size_t)H * W, total = (size_t)B * hw * Cin;
    const Span spans[] = {writes(y, total), reads(img, (size_t)B * 3 * hw), reads(alpha, (size_t)B * hw), reads(camera_feat, (size_t)B * 3)};
    if (clash(spans)) { set_error("dl_assemble_input: y overlaps an input"); return R3D_ERR_INVALID_ARG; }
    hipLaunchKernelGGL(dl_assemble_input, grid_for(total), dim3(256), 0, (hipStream_t)stream, img, alpha, camera_feat, H, W, Cin, total, y);
    return check_launch("dl_assemble_input");
}
