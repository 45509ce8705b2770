// The motion-field estimator of the face-vid2vid torso network (modules/real3d/facev2v_warp/network2.py:162-244), inference only, exact
// fp32.  Activations are channel-last fp32 [N, D, H, W, C].  Kernels:
//   conv3d<VEC, WM, WN, TM, TN>  the D3 = true instantiation of conv_tile (r3d_torso_conv.h): stride-1 Conv3d on v_mfma_f32_16x16x4_f32
//                                with nearest x2 up-sampling of H and W in the tap addresses, AvgPool3d((1, 2, 2)) in the epilogue, an output
//                                channel slice, and the full-depth form (a Conv2d over x.view(N, C D, H, W)).
//   tmotion_bf3::conv3d<...>     the same tiles with the products on the BF16X3 tier (r3d_torso_conv3d_prec).
//   motion_input                 compress (Conv3d 1x1x1) + the heatmaps + the sparse motions + grid_sample(align_corners=True, zeros
//                                padding) of the compressed volume, one thread per (voxel, k): the hourglass input.
//   motion_deform                softmax over the K + 1 mask logits and the mask-weighted sum of the sparse motions, one thread per voxel.
//   motion_broadcast             the 2-D head features repeated over depth into their slice of the fuser's input.
// The sparse motions (the identity grid for k = 0, J (grid - kp_d[k]) + kp_s[k] for k >= 1) are never stored: both small kernels recompute them.
// r3d_torso_conv3d / _prec describe their call and hand it, with this unit's kernel family, to the shared check, tile table and launcher
// (r3d_torso_launch.h).
#include "r3d_common.h"
#include "r3d_torso_launch.h"
#include <math.h>

namespace r3d {
namespace tmotion {

using tconv::ConvArgs;

template <bool VEC, int WM, int WN, int TM, int TN>
__global__ void __launch_bounds__(256) conv3d(ConvArgs g) { tconv::conv_tile<tconv::F32, VEC, true, WM, WN, TM, TN>(g); }

}  // namespace tmotion

// the kernels of the BF16X3 tier (R3D_TORSO_BF16X3)
namespace tmotion_bf3 {

template <bool VEC, int WM, int WN, int TM, int TN>
__global__ void __launch_bounds__(256) conv3d(tconv::ConvArgs g) { tconv::conv_tile<tconv::BF16X3, VEC, true, WM, WN, TM, TN>(g); }

}  // namespace tmotion_bf3

namespace tmotion {

// this unit's kernel family for tlaunch::run (r3d_torso_launch.h): the 3-D body
struct Family {
    static constexpr bool tile64x16 = true;
    template <int PREC, bool VEC, int WM, int WN, int TM, int TN>
    static void (*kernel())(ConvArgs)
    {
        if constexpr (PREC == tconv::BF16X3) return tmotion_bf3::conv3d<VEC, WM, WN, TM, TN>;
        else return conv3d<VEC, WM, WN, TM, TN>;
    }
};

struct MotionArgs {
    const float* fs; int N, C, D, H, W;          // [N, D, H, W, C]
    const float* cw; const float* cb;            // compress: [4, C], [4]
    const float* kp_s; const float* kp_d;        // [N, K, 3]: component 0 indexes W, 1 H, 2 D
    const float* J; int K;                       // [N, 3, 3]
    float* inp; int cpad;                        // [N, D, H, W, cpad]: channel 5 k + c, zeros from 5 (K + 1) on
    float* fuse; int fcs;                        // the same channels in rows of fcs floats (or nullptr)
    const float* mask; float* out;               // motion_deform: [N, D, H, W, K + 1] -> [N, D, H, W, 3]
};

// the identity grid of align_corners=True as the reference computes it (func_utils.py:91-103)
__device__ __forceinline__ float grid_coord(int i, int size) { return 2.0f * ((float)i / (float)(size - 1)) - 1.0f; }

// sparse motion k >= 1 at grid point (gx, gy, gz) of sample n (func_utils.py:152-165)
__device__ __forceinline__ void sparse_motion(const MotionArgs& a, size_t n, int k, float gx, float gy, float gz, float& sx, float& sy, float& sz)
{
    const float* kd = a.kp_d + (n * a.K + (k - 1)) * 3;
    const float* ks = a.kp_s + (n * a.K + (k - 1)) * 3;
    const float* J = a.J + n * 9;
    const float vx = gx - kd[0], vy = gy - kd[1], vz = gz - kd[2];
    sx = (J[0] * vx + J[1] * vy + J[2] * vz) + ks[0];
    sy = (J[3] * vx + J[4] * vy + J[5] * vz) + ks[1];
    sz = (J[6] * vx + J[7] * vy + J[8] * vz) + ks[2];
}

// a normalised coordinate's lower corner and the weight of the upper one (align_corners=True); corners outside [0, size) contribute 0.
// The source coordinate is clipped to [-2, size + 1] first (both corners stay outside) so that the conversion to int is defined.
__device__ __forceinline__ void sample_axis(float g, int size, int& i0, float& f)
{
    float x = ((g + 1.0f) * 0.5f) * (float)(size - 1);
    x = fminf(fmaxf(x, -2.0f), (float)(size + 1));
    const float fl = floorf(x);
    i0 = (int)fl;
    f = x - fl;
}

__global__ void __launch_bounds__(256) motion_input(MotionArgs a)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, total = (size_t)a.N * a.D * a.H * a.W * (a.K + 1);
    if (i >= total) return;
    const int k = (int)(i % (a.K + 1));
    const size_t p = i / (a.K + 1);                     // voxel ((n D + d) H + h) W + w
    size_t q = p;
    const int w = (int)(q % a.W); q /= a.W;
    const int h = (int)(q % a.H); q /= a.H;
    const int d = (int)(q % a.D);
    const size_t n = q / a.D;
    const float gx = grid_coord(w, a.W), gy = grid_coord(h, a.H), gz = grid_coord(d, a.D);
    float sx = gx, sy = gy, sz = gz, heat = 0.0f;
    if (k > 0) {
        sparse_motion(a, n, k, gx, gy, gz, sx, sy, sz);
        const float* kd = a.kp_d + (n * a.K + (k - 1)) * 3;
        const float* ks = a.kp_s + (n * a.K + (k - 1)) * 3;
        const float dx = gx - kd[0], dy = gy - kd[1], dz = gz - kd[2], ex = gx - ks[0], ey = gy - ks[1], ez = gz - ks[2];
        heat = expf(-0.5f * (dx * dx + dy * dy + dz * dz) / 0.01f) - expf(-0.5f * (ex * ex + ey * ey + ez * ez) / 0.01f);
    }
    int x0, y0, z0;
    float fx, fy, fz;
    sample_axis(sx, a.W, x0, fx);
    sample_axis(sy, a.H, y0, fy);
    sample_axis(sz, a.D, z0, fz);
    const float* src = a.fs + n * a.D * a.H * a.W * a.C;
    float o0 = 0.0f, o1 = 0.0f, o2 = 0.0f, o3 = 0.0f;
#pragma unroll
    for (int dz = 0; dz < 2; ++dz) {
        const int z = z0 + dz;
        const float wz = dz ? fz : 1.0f - fz;
        if (z < 0 || z >= a.D) continue;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            const int y = y0 + dy;
            const float wy = dy ? fy : 1.0f - fy;
            if (y < 0 || y >= a.H) continue;
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int x = x0 + dx;
                const float wx = dx ? fx : 1.0f - fx;
                if (x < 0 || x >= a.W) continue;
                // the compressed features of this corner: compress.weight . fs + compress.bias
                const float* v = src + (((size_t)z * a.H + y) * a.W + x) * a.C;
                float c0 = a.cb[0], c1 = a.cb[1], c2 = a.cb[2], c3 = a.cb[3];
                for (int c = 0; c < a.C; ++c) {
                    const float f = v[c];
                    c0 = fmaf(a.cw[c], f, c0); c1 = fmaf(a.cw[a.C + c], f, c1);
                    c2 = fmaf(a.cw[2 * a.C + c], f, c2); c3 = fmaf(a.cw[3 * a.C + c], f, c3);
                }
                const float wgt = wx * wy * wz;
                o0 = fmaf(c0, wgt, o0); o1 = fmaf(c1, wgt, o1); o2 = fmaf(c2, wgt, o2); o3 = fmaf(c3, wgt, o3);
            }
        }
    }
    const int nreal = 5 * (a.K + 1);
    auto put = [&](float* dst) {
        float* o = dst + 5 * k;
        o[0] = heat; o[1] = o0; o[2] = o1; o[3] = o2; o[4] = o3;
        if (k == 0)
            for (int c = nreal; c < a.cpad; ++c) dst[c] = 0.0f;
    };
    put(a.inp + p * a.cpad);
    if (a.fuse) put(a.fuse + p * a.fcs);
}

__global__ void __launch_bounds__(256) motion_deform(MotionArgs a)
{
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x, total = (size_t)a.N * a.D * a.H * a.W;
    if (p >= total) return;
    size_t q = p;
    const int w = (int)(q % a.W); q /= a.W;
    const int h = (int)(q % a.H); q /= a.H;
    const int d = (int)(q % a.D);
    const size_t n = q / a.D;
    const float gx = grid_coord(w, a.W), gy = grid_coord(h, a.H), gz = grid_coord(d, a.D);
    const float* l = a.mask + p * (a.K + 1);
    float mx = l[0];
    for (int k = 1; k <= a.K; ++k) mx = fmaxf(mx, l[k]);
    float sum = 0.0f;
    for (int k = 0; k <= a.K; ++k) sum += expf(l[k] - mx);
    float ox = 0.0f, oy = 0.0f, oz = 0.0f;
    for (int k = 0; k <= a.K; ++k) {
        const float m = expf(l[k] - mx) / sum;
        float sx = gx, sy = gy, sz = gz;
        if (k > 0) sparse_motion(a, n, k, gx, gy, gz, sx, sy, sz);
        ox = fmaf(sx, m, ox); oy = fmaf(sy, m, oy); oz = fmaf(sz, m, oz);
    }
    a.out[p * 3] = ox; a.out[p * 3 + 1] = oy; a.out[p * 3 + 2] = oz;
}

__global__ void __launch_bounds__(256) motion_broadcast(const float* feats, int C, int D, size_t HW, size_t total, float* fuse, int fcs, int fco)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C);
    const size_t p = i / C;                              // (n D + d) HW + px
    const size_t px = p % HW, n = p / HW / D;
    fuse[p * fcs + fco + c] = feats[(n * C + c) * HW + px];
}

}  // namespace tmotion
}  // namespace r3d

using namespace r3d;
using namespace r3d::tmotion;

extern "C" int r3d_torso_conv3d_prec(const float* x, int B, int D, int Hs, int Ws, int Cin, int upsample, const float* w, const float* bias,
                                     int Cout, int ksize, int full_depth, int act, float act_slope, int pool, float* y, int y_cstride,
                                     int y_coffset, float* y_ncdhw, int precision, r3d_stream_t stream)
{
    tlaunch::ConvCall c = tlaunch::conv_call(x, B, Hs, Ws, Cin, w, bias, Cout, ksize, act, act_slope, y, precision);
    c.D = D; c.volume = true; c.upsample = upsample; c.full_depth = full_depth; c.pool = pool; c.ycs = y_cstride; c.yco = y_coffset; c.yn = y_ncdhw;
    return tlaunch::run<Family>("torso_conv3d", c, stream);
}

extern "C" int r3d_torso_conv3d(const float* x, int B, int D, int Hs, int Ws, int Cin, int upsample, const float* w, const float* bias,
                                int Cout, int ksize, int full_depth, int act, float act_slope, int pool, float* y, int y_cstride,
                                int y_coffset, float* y_ncdhw, r3d_stream_t stream)
{
    return r3d_torso_conv3d_prec(x, B, D, Hs, Ws, Cin, upsample, w, bias, Cout, ksize, full_depth, act, act_slope, pool, y, y_cstride, y_coffset,
                                 y_ncdhw, R3D_TORSO_F32, stream);
}

static int motion_common(const char* what, const float* kp_s, const float* kp_d, const float* J, int N, int D, int H, int W, int K)
{
    if (!kp_s || !kp_d || !J) { set_error("%s: NULL pointer", what); return R3D_ERR_INVALID_ARG; }
    if (N <= 0 || D < 2 || H < 2 || W < 2 || K < 1 || K > 64 || (double)N * D * H * W * 5 * (K + 1) > 2147483647.0)
        { set_error("%s: bad argument (N > 0; D, H, W >= 2; 1 <= K <= 64; fewer than 2^31 elements)", what); return R3D_ERR_INVALID_ARG; }
    return R3D_OK;
}

extern "C" int r3d_torso_motion_input(const float* fs_cl, int N, int C, int D, int H, int W, const float* compress_w,
                                      const float* compress_b, const float* kp_s, const float* kp_d, const float* J, int K, float* inp,
                                      int inp_channels, float* fuse, int fuse_cstride, r3d_stream_t stream)
{
    if (!fs_cl || !compress_w || !compress_b || !inp) { set_error("torso_motion_input: NULL pointer"); return R3D_ERR_INVALID_ARG; }
    if (int rc = motion_common("torso_motion_input", kp_s, kp_d, J, N, D, H, W, K)) return rc;
    if (C <= 0 || C > 4096 || inp_channels < 5 * (K + 1) || (fuse && fuse_cstride < inp_channels) || (double)N * D * H * W * C > 2147483647.0 ||
        (double)N * D * H * W * inp_channels > 2147483647.0 || (double)N * D * H * W * (fuse ? fuse_cstride : 1) > 9.0e18)
        { set_error("torso_motion_input: bad argument (1 <= C <= 4096, 5 (K + 1) <= inp_channels <= fuse_cstride, fewer than 2^31 elements)");
          return R3D_ERR_INVALID_ARG; }
    const size_t vox = (size_t)N * D * H * W, nfs = vox * C, ninp = vox * inp_channels, nfuse = fuse ? vox * fuse_cstride : 0;
    Span spans[] = {writes(inp, ninp), reads(fs_cl, nfs), reads(compress_w, (size_t)4 * C), reads(compress_b, 4), reads(kp_s, (size_t)N * K * 3),
                    reads(kp_d, (size_t)N * K * 3), reads(J, (size_t)N * 9)};
    const bool inp_clashes = clash(spans);
    spans[0] = writes(fuse, nfuse);          // the other output against the same inputs (absent: no part)
    if (inp_clashes || clash(spans)) { set_error("torso_motion_input: an output overlaps an input"); return R3D_ERR_INVALID_ARG; }
    if (overlap(inp, ninp, fuse, nfuse)) { set_error("torso_motion_input: inp and fuse overlap"); return R3D_ERR_INVALID_ARG; }
    MotionArgs a = {};
    a.fs = fs_cl; a.N = N; a.C = C; a.D = D; a.H = H; a.W = W; a.cw = compress_w; a.cb = compress_b; a.kp_s = kp_s; a.kp_d = kp_d; a.J = J;
    a.K = K; a.inp = inp; a.cpad = inp_channels; a.fuse = fuse; a.fcs = fuse_cstride;
    const size_t total = vox * (K + 1);
    hipLaunchKernelGGL(motion_input, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    return check_launch("torso_motion_input");
}

extern "C" int r3d_torso_motion_deform(const float* mask, int N, int D, int H, int W, int K, const float* kp_s, const float* kp_d,
                                       const float* J, float* out, r3d_stream_t stream)
{
    if (!mask || !out) { set_error("torso_motion_deform: NULL pointer"); return R3D_ERR_INVALID_ARG; }
    if (int rc = motion_common("torso_motion_deform", kp_s, kp_d, J, N, D, H, W, K)) return rc;
    const size_t vox = (size_t)N * D * H * W;
    const Span spans[] = {writes(out, vox * 3), reads(mask, vox * (K + 1)), reads(kp_s, (size_t)N * K * 3), reads(kp_d, (size_t)N * K * 3),
                          reads(J, (size_t)N * 9)};
    if (clash(spans)) { set_error("torso_motion_deform: out overlaps an input"); return R3D_ERR_INVALID_ARG; }
    MotionArgs a = {};
    a.N = N; a.D = D; a.H = H; a.W = W; a.kp_s = kp_s; a.kp_d = kp_d; a.J = J; a.K = K; a.mask = mask; a.out = out;
    hipLaunchKernelGGL(motion_deform, dim3((unsigned)((vox + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    return check_launch("torso_motion_deform");
}

extern "C" int r3d_torso_motion_broadcast(const float* feats, int N, int C, int H, int W, int D, float* fuse, int fuse_cstride,
                                          int fuse_coffset, r3d_stream_t stream)
{
    if (!feats || !fuse) { set_error("torso_motion_broadcast: NULL pointer"); return R3D_ERR_INVALID_ARG; }
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || D <= 0 || fuse_coffset < 0 || fuse_cstride < fuse_coffset + C ||
        (double)N * D * H * W * C > 2147483647.0 || (double)N * D * H * W * fuse_cstride > 9.0e18)
        { set_error("torso_motion_broadcast: bad argument (positive sizes, the slice inside the row, fewer than 2^31 elements)"); return R3D_ERR_INVALID_ARG; }
    const size_t hw = (size_t)H * W, total = (size_t)N * D * hw * C;
    if (overlap(fuse, (size_t)N * D * hw * fuse_cstride, feats, (size_t)N * C * hw))
        { set_error("torso_motion_broadcast: fuse overlaps feats"); return R3D_ERR_INVALID_ARG; }
    hipLaunchKernelGGL(motion_broadcast, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, feats, C, D, hw, total,
                       fuse, fuse_cstride, fuse_coffset);
    return check_launch("torso_motion_broadcast");
}
