// The glue of WarpBasedTorsoModelMediaPipe.forward between its three modules (modules/real3d/facev2v_warp/model2.py:226-236), inference
// only, fp32.  Two bandwidth kernels on the fp32 VALU, no matrix work:
//   seg_input     cat(img, bilinear(segmap[:, [c0, c1]], (OH, OW))) as one NCHW tensor: in_conv's input in rgb_alpha mode (:226-228).
//   mask_volume<VEC>
//                       (:231-236) one block per (sample, TH x TW pixel tile, run of depth slices).  The block resizes the two segmap
//                       channels over its tile plus the dilation's halo once, into LDS (the halo positions are those `reflect` padding
//                       names), takes the ksize x ksize maximum of their sum per tile pixel, and then streams its depth slices of the
//                       channel-last volume: masked = feats * mask_d, and the same values followed by (seg0, seg1) as the (C + 2)-channel
//                       volume r3d_torso_motion_input reads.  VEC (C % 4 == 0, 16-byte aligned pointers): 16-byte loads and stores on
//                       the C-channel side, 8-byte stores on the (C + 2)-channel side, whose pixels are only 8-byte aligned; otherwise
//                       one float per access.
// F.interpolate(mode='bilinear', align_corners=False, antialias=False) is ATen's: src = max((dst + 0.5) in / out - 0.5, 0), the upper
// neighbour clamped at the edge, h0 (w0 x00 + w1 x01) + h1 (w0 x10 + w1 x11).
#include "r3d_common.h"
#include <type_traits>

namespace r3d {
namespace tglue {

constexpr int TH = 4, TW = 16, TP = TH * TW;          // the pixel tile of mask_volume: rows of 16 pixels (2 KiB of a 32-channel slice)

struct Axis { int i0, i1; float l0, l1; };

__device__ __forceinline__ Axis resize_axis(int dst, float scale, int in_size)
{
    const float src = fmaxf(((float)dst + 0.5f) * scale - 0.5f, 0.0f);
    Axis a;
    a.i0 = min((int)src, in_size - 1);
    a.i1 = a.i0 + (a.i0 < in_size - 1 ? 1 : 0);
    a.l1 = src - (float)a.i0;
    a.l0 = 1.0f - a.l1;
    return a;
}

__device__ __forceinline__ float bilinear(const float* p, int W, const Axis& y, const Axis& x)
{
    const float* r0 = p + (size_t)y.i0 * W;
    const float* r1 = p + (size_t)y.i1 * W;
    return y.l0 * (x.l0 * r0[x.i0] + x.l1 * r0[x.i1]) + y.l1 * (x.l0 * r1[x.i0] + x.l1 * r1[x.i1]);
}

struct SegInputArgs {
    const float* img; int Ci;                   // [N, Ci, OH, OW] or NULL with Ci = 0
    const float* seg; int Cs, Hs, Ws, c0, c1;   // [N, Cs, Hs, Ws]
    float* out; int OH, OW;                     // [N, Ci + 2, OH, OW]
    size_t total;
};

__global__ void __launch_bounds__(256) seg_input(SegInputArgs a)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.total) return;
    const size_t hw = (size_t)a.OH * a.OW;
    const size_t plane = i / hw, p = i - plane * hw;
    const int Co = a.Ci + 2;
    const size_t n = plane / Co;
    const int c = (int)(plane - n * Co);
    if (c < a.Ci) { a.out[i] = a.img[(n * a.Ci + c) * hw + p]; return; }
    const int oy = (int)(p / a.OW), ox = (int)(p - (size_t)oy * a.OW);
    const Axis y = resize_axis(oy, (float)a.Hs / (float)a.OH, a.Hs), x = resize_axis(ox, (float)a.Ws / (float)a.OW, a.Ws);
    const int cs = c == a.Ci ? a.c0 : a.c1;
    a.out[i] = bilinear(a.seg + (n * a.Cs + cs) * ((size_t)a.Hs * a.Ws), a.Ws, y, x);
}

struct MaskArgs {
    const float* feats; int N, D, H, W, C;      // [N, D, H, W, C]
    const float* seg; int Cs, Hs, Ws, c0, c1;   // [N, Cs, Hs, Ws]
    int pad, mul, dchunk, tiles_x;
    float* masked;                              // [N, D, H, W, C], may be `feats`
    float* motion;                              // [N, D, H, W, C + 2]
};

// i < 0 -> -i, i >= n -> 2 (n - 1) - i (F.pad(mode='reflect'), pad < n); positions no window of an image pixel reaches are clamped
__device__ __forceinline__ int reflect(int i, int n)
{
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * (n - 1) - i : i;
    return min(max(i, 0), n - 1);
}

template <bool VEC>
__global__ void __launch_bounds__(256) mask_volume(MaskArgs a)
{
    extern __shared__ float lds[];
    const int t = threadIdx.x, pad = a.pad, hh = TH + 2 * pad, hw = TW + 2 * pad;
    float* s0 = lds;                            // [TP] seg0, [TP] seg1, [TP] the dilated mask, [hh, hw] seg0 + seg1 over tile + halo
    float* s1 = lds + TP;
    float* md = lds + 2 * TP;
    float* halo = lds + 3 * TP;
    const int tile = blockIdx.x, ty0 = (tile / a.tiles_x) * TH, tx0 = (tile % a.tiles_x) * TW;
    const int n = blockIdx.z, d0 = blockIdx.y * a.dchunk, d1 = min(d0 + a.dchunk, a.D);
    const size_t shw = (size_t)a.Hs * a.Ws;
    const float* p0 = a.seg + ((size_t)n * a.Cs + a.c0) * shw;
    const float* p1 = a.seg + ((size_t)n * a.Cs + a.c1) * shw;
    const float sy = (float)a.Hs / (float)a.H, sx = (float)a.Ws / (float)a.W;
    for (int j = t; j < hh * hw; j += 256) {
        const int hy = j / hw, hx = j - hy * hw;
        const Axis y = resize_axis(reflect(ty0 + hy - pad, a.H), sy, a.Hs), x = resize_axis(reflect(tx0 + hx - pad, a.W), sx, a.Ws);
        const float v0 = bilinear(p0, a.Ws, y, x), v1 = bilinear(p1, a.Ws, y, x);
        halo[j] = v0 + v1;
        const int cy = hy - pad, cx = hx - pad;
        if (cy >= 0 && cy < TH && cx >= 0 && cx < TW) { s0[cy * TW + cx] = v0; s1[cy * TW + cx] = v1; }
    }
    __syncthreads();
    if (t < TP) {
        const int cy = t / TW, cx = t - cy * TW;
        float m = halo[cy * hw + cx];
        for (int dy = 0; dy <= 2 * pad; ++dy)
            for (int dx = 0; dx <= 2 * pad; ++dx) m = fmaxf(m, halo[(cy + dy) * hw + cx + dx]);
        md[t] = m;
    }
    __syncthreads();
    // the block's slices: `per` accesses a slice, each the CV channels of one tile pixel; four loads in flight per lane before the
    // first store (at the product shape a lane has exactly four)
    constexpr int CV = VEC ? 4 : 1, NB = 4;
    typedef typename std::conditional<VEC, f32x4, float>::type V;
    const int cpp = a.C / CV, per = TP * cpp, total = (d1 - d0) * per, Cm = a.C + 2;
    const bool mul = a.mul != 0;
    for (int base = t; base < total; base += 256 * NB) {
        V v[NB];
        size_t pix[NB];
        int c[NB];
        float m[NB];
        bool ok[NB];
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            const int i = base + k * 256, dd = i / per, r = i - dd * per, px = r / cpp;
            const int y = ty0 + px / TW, x = tx0 + px % TW;
            ok[k] = i < total && y < a.H && x < a.W;
            c[k] = (r - px * cpp) * CV;
            pix[k] = (((size_t)n * a.D + d0 + dd) * a.H + y) * a.W + x;
            // no branch around the load, so that the four stay in flight together: a lane without work reads element 0
            v[k] = *reinterpret_cast<const V*>(a.feats + (ok[k] ? pix[k] * a.C + c[k] : 0));
            m[k] = md[px];
        }
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            if (!ok[k]) continue;
            if (mul) v[k] *= m[k];
            *reinterpret_cast<V*>(a.masked + pix[k] * a.C + c[k]) = v[k];
            float* q = a.motion + pix[k] * Cm + c[k];
            if constexpr (VEC) {          // a pixel of C + 2 channels is 8-byte aligned, not 16
                reinterpret_cast<float2*>(q)[0] = make_float2(v[k].x, v[k].y);
                reinterpret_cast<float2*>(q)[1] = make_float2(v[k].z, v[k].w);
            } else {
                q[0] = v[k];
            }
        }
    }
    // the two segmap channels, repeated over depth
    for (int i = t; i < (d1 - d0) * TP; i += 256) {
        const int dd = i / TP, px = i - dd * TP;
        const int y = ty0 + px / TW, x = tx0 + px % TW;
        if (y >= a.H || x >= a.W) continue;
        float* q = a.motion + ((((size_t)n * a.D + d0 + dd) * a.H + y) * a.W + x) * Cm + a.C;
        if constexpr (VEC) *reinterpret_cast<float2*>(q) = make_float2(s0[px], s1[px]);
        else { q[0] = s0[px]; q[1] = s1[px]; }
    }
}

}  // namespace tglue
}  // namespace r3d

using namespace r3d;
using namespace r3d::tglue;

extern "C" int r3d_torso_seg_input(const float* img, int N, int Ci, const float* segmap, int Cs, int Hs, int Ws, int c0, int c1, float* out,
                                   int OH, int OW, r3d_stream_t stream)
{
    if (!segmap || !out || (Ci > 0 && !img)) { set_error("torso_seg_input: NULL pointer"); return R3D_ERR_INVALID_ARG; }
    if (N <= 0 || Ci < 0 || Cs <= 0 || Hs <= 0 || Ws <= 0 || OH <= 0 || OW <= 0 || (double)N * (Ci + 2.0) * OH * OW > 2147483647.0 ||
        (double)N * Cs * Hs * Ws > 2147483647.0)
        { set_error("torso_seg_input: bad argument (positive sizes, Ci >= 0, fewer than 2^31 elements)"); return R3D_ERR_INVALID_ARG; }
    if (c0 < 0 || c1 < 0 || c0 >= Cs || c1 >= Cs)
        { set_error("torso_seg_input: channels %d and %d are not both in a segmap of %d channels", c0, c1, Cs); return R3D_ERR_INVALID_ARG; }
    const size_t ohw = (size_t)OH * OW, nout = (size_t)N * (Ci + 2) * ohw, nseg = (size_t)N * Cs * Hs * Ws;
    if (overlap(out, nout, segmap, nseg) || (Ci > 0 && overlap(out, nout, img, (size_t)N * Ci * ohw)))
        { set_error("torso_seg_input: out overlaps an input"); return R3D_ERR_INVALID_ARG; }
    SegInputArgs a = {Ci > 0 ? img : nullptr, Ci, segmap, Cs, Hs, Ws, c0, c1, out, OH, OW, nout};
    hipLaunchKernelGGL(seg_input, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    return check_launch("torso_seg_input");
}

extern "C" int r3d_torso_mask_volume(const float* feats_cl, int N, int D, int H, int W, int C, const float* segmap, int Cs, int Hs, int Ws,
                                     int c0, int c1, int ksize, int mul_mask, float* masked_cl, float* motion_cl, r3d_stream_t stream)
{
    if (!feats_cl || !segmap || !masked_cl || !motion_cl) { set_error("torso_mask_volume: NULL pointer"); return R3D_ERR_INVALID_ARG; }
    if (N <= 0 || D <= 0 || H <= 0 || W <= 0 || C <= 0 || Cs <= 0 || Hs <= 0 || Ws <= 0 || N > 65535 ||
        (double)N * D * H * W * (C + 2.0) > 2147483647.0 || (double)N * Cs * Hs * Ws > 2147483647.0)
        { set_error("torso_mask_volume: bad argument (positive sizes, N < 65536, fewer than 2^31 elements)"); return R3D_ERR_INVALID_ARG; }
    if (c0 < 0 || c1 < 0 || c0 >= Cs || c1 >= Cs)
        { set_error("torso_mask_volume: channels %d and %d are not both in a segmap of %d channels", c0, c1, Cs); return R3D_ERR_INVALID_ARG; }
    if (ksize < 1 || ksize % 2 == 0) { set_error("torso_mask_volume: ksize %d is not odd and positive", ksize); return R3D_ERR_INVALID_ARG; }
    const int pad = (ksize - 1) / 2;
    if (pad >= (H < W ? H : W))
        { set_error("torso_mask_volume: ksize %d needs reflect padding %d, not smaller than the %d x %d image", ksize, pad, H, W); return R3D_ERR_INVALID_ARG; }
    const size_t lds = ((size_t)(TH + 2 * pad) * (TW + 2 * pad) + 3 * TP) * sizeof(float);
    if (lds > 65536) { set_error("torso_mask_volume: ksize %d needs more than 64 KiB of LDS for a tile's window", ksize); return R3D_ERR_INVALID_ARG; }
    const size_t vox = (size_t)N * D * H * W, nf = vox * C, nm = vox * (C + 2), nseg = (size_t)N * Cs * Hs * Ws;
    if (masked_cl != feats_cl && overlap(masked_cl, nf, feats_cl, nf))
        { set_error("torso_mask_volume: masked_cl overlaps feats_cl without being feats_cl"); return R3D_ERR_INVALID_ARG; }
    const Span spans[] = {reads(segmap, nseg), writes(masked_cl, nf), writes(motion_cl, nm)};          // (feats_cl: masked_cl may be it)
    if (clash(spans) || overlap(motion_cl, nm, feats_cl, nf)) { set_error("torso_mask_volume: an output overlaps the segmap, feats_cl or the other output"); return R3D_ERR_INVALID_ARG; }
    const int tiles_x = (W + TW - 1) / TW, tiles = tiles_x * ((H + TH - 1) / TH);
    // a block resizes and dilates its tile once per run of depth slices: runs of D / 8, so that the product shape (64 x 64 x 16) still
    // gives every compute unit two blocks
    const int dchunk = (D + 7) / 8, zc = (D + dchunk - 1) / dchunk;
    MaskArgs a = {feats_cl, N, D, H, W, C, segmap, Cs, Hs, Ws, c0, c1, pad, mul_mask ? 1 : 0, dchunk, tiles_x, masked_cl, motion_cl};
    const bool vec = C % 4 == 0 && aligned(feats_cl, 16) && aligned(masked_cl, 16) && aligned(motion_cl, 8);
    const dim3 grid((unsigned)tiles, (unsigned)zc, (unsigned)N);
    if (vec) hipLaunchKernelGGL(mask_volume<true>, grid, dim3(256), lds, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(mask_volume<false>, grid, dim3(256), lds, (hipStream_t)stream, a);
    return check_launch("torso_mask_volume");
}
