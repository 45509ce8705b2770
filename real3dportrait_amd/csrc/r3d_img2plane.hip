// Img2PlaneModel without its DeepLabV3 (modules/img2plane/img2plane_model.py:12-82): what HighResoEncoder, LowResolutionViT and
// TriplanePredictorViT (modules/img2plane/segformer/models.py, base.py) need beyond the r3d_secc_* and r3d_torso_conv entry points,
// inference only, exact fp32 (include/r3d_hip_img2plane.h).  Kernels:
//   i2p_attention<DMAX>  softmax(q k^T scale) v at head dimension D <= DMAX in {64, 128, 256}, any number of keys.  One block per
//                        (batch, head, 64 queries), 4 waves x 16 queries; keys and values stream through LDS 32 at a time (66.5 KiB at
//                        DMAX 256, so two blocks share a CU's 160 KiB); S = q k^T and O = P v on v_mfma_f32_16x16x4_f32, a running
//                        maximum and sum per query row.  A wave's state: its 16 x DMAX queries as the A operand (DMAX / 4 registers), the
//                        16 x DMAX output tile (DMAX / 4 accumulator registers), two 16 x 16 tiles of S.
//   i2p_upsample2x       bilinear x2, align_corners=True, channel-last.
//   i2p_pixel_shuffle    nn.PixelShuffle(2) of a token tensor into a channel slice.
//   i2p_copy_channels    one side of a channel concatenation.
//   i2p_nchw_to_cl       [B, C, H, W] -> [B, H, W, C].
//   i2p_planes_out       [B, H, W, 3 Cp] -> the flipped planes [B, 3, Cp, H, W].
#include "r3d_common.h"
#include "../../include/r3d_hip_img2plane.h"
#include <math.h>

namespace r3d {
namespace i2p {

constexpr int QB = 64, KC = 32, PLD = KC + 1;          // queries per block, keys per chunk, row stride of a wave's P tile

// The k index of the S product is a head channel, and any one-to-one map from (MFMA step, lane group) to channels serves as long as q and k
// use the same: step s of lane group g takes channel g DMAX / 4 + s, so four consecutive steps read one 16-byte piece of a key's row.
template <int DMAX>
__global__ void __launch_bounds__(256, 2) i2p_attention(const float* q, const float* kv, int N, int L, int C, int D, float scale, float* out)
{
    constexpr int DQ = DMAX / 4, DT = DMAX / 16, KLD = DMAX + 4, VLD = DMAX + 16;
    __shared__ __attribute__((aligned(16))) float Ks[KC * KLD];
    __shared__ __attribute__((aligned(16))) float Vs[KC * VLD];
    __shared__ float Ps[4][16 * PLD];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int h = blockIdx.y, b = blockIdx.z, q0 = blockIdx.x * QB + wave * 16;
    const int li = lane & 15, lg = lane >> 4;

    float qa[DQ];
    {
        const int qi = q0 + li;
        const float* qr = q + ((size_t)b * N + (qi < N ? qi : 0)) * C + (size_t)h * D;
#pragma unroll
        for (int s = 0; s < DQ; s += 4) {
            const int d = lg * DQ + s;
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (qi < N && d < D) v = *(const float4*)(qr + d);
            qa[s] = v.x; qa[s + 1] = v.y; qa[s + 2] = v.z; qa[s + 3] = v.w;
        }
    }
    f32x4 o[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) o[dt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    float mrow[4], lrow[4];                              // rows 4 lg + r of the wave's 16
#pragma unroll
    for (int r = 0; r < 4; ++r) { mrow[r] = -INFINITY; lrow[r] = 0.0f; }
    float* P = Ps[wave];
    const float* kvb = kv + (size_t)b * L * 2 * C + (size_t)h * D;

    for (int j0 = 0; j0 < L; j0 += KC) {
        __syncthreads();
        // the chunk's keys and values, 16 bytes at a time; rows past L and channels past D are zero
        for (int e = t; e < KC * DQ; e += 256) {
            const int kr = e / DQ, d = (e - kr * DQ) * 4, key = j0 + kr;
            float4 kk = make_float4(0.0f, 0.0f, 0.0f, 0.0f), vv = kk;
            if (key < L && d < D) {
                const float* src = kvb + (size_t)key * 2 * C + d;
                kk = *(const float4*)src;
                vv = *(const float4*)(src + C);
            }
            *(float4*)(Ks + kr * KLD + d) = kk;
            *(float4*)(Vs + kr * VLD + d) = vv;
        }
        __syncthreads();
        // S = q k^T for the 2 tiles of 16 keys: two independent accumulator chains
        f32x4 s[2] = {f32x4{0.0f, 0.0f, 0.0f, 0.0f}, f32x4{0.0f, 0.0f, 0.0f, 0.0f}};
#pragma unroll
        for (int st = 0; st < DQ; st += 4) {
            const float4 k0 = *(const float4*)(Ks + li * KLD + lg * DQ + st);
            const float4 k1 = *(const float4*)(Ks + (16 + li) * KLD + lg * DQ + st);
            s[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[st], k0.x, s[0], 0, 0, 0);
            s[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[st], k1.x, s[1], 0, 0, 0);
            s[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[st + 1], k0.y, s[0], 0, 0, 0);
            s[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[st + 1], k1.y, s[1], 0, 0, 0);
            s[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[st + 2], k0.z, s[0], 0, 0, 0);
            s[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[st + 2], k1.z, s[1], 0, 0, 0);
            s[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[st + 3], k0.w, s[0], 0, 0, 0);
            s[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[st + 3], k1.w, s[1], 0, 0, 0);
        }
        // D layout of 16x16x4: key column lane & 15, query rows 4 (lane >> 4) + r.  Row maxima over the chunk, then the rescale.
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float mx = -INFINITY;
#pragma unroll
            for (int kt = 0; kt < 2; ++kt) {
                const float v = j0 + kt * 16 + li < L ? s[kt][r] * scale : -INFINITY;
                s[kt][r] = v;
                mx = fmaxf(mx, v);
            }
#pragma unroll
            for (int off = 8; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
            const float mnew = fmaxf(mrow[r], mx);             // finite: every chunk holds at least one valid key
            const float corr = expf(mrow[r] - mnew);           // 0 on the first chunk (exp(-inf))
            float ps = 0.0f;
#pragma unroll
            for (int kt = 0; kt < 2; ++kt) {
                const float p = expf(s[kt][r] - mnew);         // 0 for masked keys
                ps += p;
                P[(lg * 4 + r) * PLD + kt * 16 + li] = p;
            }
#pragma unroll
            for (int off = 8; off >= 1; off >>= 1) ps += __shfl_xor(ps, off);
            lrow[r] = lrow[r] * corr + ps;
            mrow[r] = mnew;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) o[dt][r] *= corr;
        }
        __builtin_amdgcn_wave_barrier();      // P is written and read by this wave only (LDS accesses of a wave complete in order)
        // O += P v: A = P[query li][key 4 st + lg], B = v[key][channel 16 dt + li]
#pragma unroll
        for (int st = 0; st < KC / 4; ++st) {
            const float pa = P[li * PLD + 4 * st + lg];
            const float* vr = Vs + (4 * st + lg) * VLD + li;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt)
                o[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(pa, vr[dt * 16], o[dt], 0, 0, 0);          // channels past D: zero columns
        }
        __builtin_amdgcn_wave_barrier();
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int qi = q0 + lg * 4 + r;
        if (qi >= N) continue;
        const float inv = 1.0f / lrow[r];
        float* orow = out + ((size_t)b * N + qi) * C + (size_t)h * D + li;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
            if (dt * 16 < D) orow[dt * 16] = o[dt][r] * inv;
    }
}

// source row / column and weight of output index o of an x2 align_corners=True resize of n entries: position o (n - 1) / (2n - 1).
// o (n - 1) passes 2^31 from n = 32 769 on: the product and the remainder are 64-bit.
__device__ __forceinline__ void up2_tap(int o, int n, int& i0, int& i1, float& lam)
{
    const long long den = 2LL * n - 1, num = (long long)o * (n - 1);
    i0 = (int)(num / den);
    lam = (float)(num - i0 * den) / (float)den;
    i1 = min(i0 + 1, n - 1);
}

__global__ void __launch_bounds__(256) i2p_upsample2x(const float* x, int H, int W, int C, size_t total, float* y)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C);
    const size_t p = i / C;
    const int ox = (int)(p % (2 * W)), oy = (int)((p / (2 * W)) % (2 * H));
    const size_t b = p / ((size_t)4 * W * H);
    int y0, y1, x0, x1;
    float ly, lx;
    up2_tap(oy, H, y0, y1, ly);
    up2_tap(ox, W, x0, x1, lx);
    const float* s = x + b * H * W * C + c;
    const float v00 = s[((size_t)y0 * W + x0) * C], v01 = s[((size_t)y0 * W + x1) * C];
    const float v10 = s[((size_t)y1 * W + x0) * C], v11 = s[((size_t)y1 * W + x1) * C];
    const float top = fmaf(lx, v01, (1.0f - lx) * v00), bot = fmaf(lx, v11, (1.0f - lx) * v10);
    y[i] = fmaf(ly, bot, (1.0f - ly) * top);
}

__global__ void __launch_bounds__(256) i2p_pixel_shuffle(const float* x, int h, int w, int Co, size_t total, float* y, int cstride, int coffset)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;          // over [B, 2h, 2w, Co]
    if (i >= total) return;
    const int c = (int)(i % Co);
    const size_t p = i / Co;
    const int ox = (int)(p % (2 * w)), oy = (int)((p / (2 * w)) % (2 * h));
    const size_t b = p / ((size_t)4 * w * h);
    y[p * cstride + coffset + c] = x[((b * h + (oy >> 1)) * w + (ox >> 1)) * 4 * Co + 4 * c + 2 * (oy & 1) + (ox & 1)];
}

__global__ void __launch_bounds__(256) i2p_copy_channels(const float* x, int C, size_t total, float* y, int cstride, int coffset)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    y[(i / C) * cstride + coffset + (int)(i % C)] = x[i];
}

__global__ void __launch_bounds__(256) i2p_nchw_to_cl(const float* x, int C, size_t hw, size_t total, float* y)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;          // over [B, H W, C]
    if (i >= total) return;
    const int c = (int)(i % C);
    const size_t p = i / C, b = p / hw;
    y[i] = x[(b * C + c) * hw + (p - b * hw)];
}

__global__ void __launch_bounds__(256) i2p_planes_out(const float* x, int H, int W, int Cp, size_t total, float* planes)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;          // over [B, 3, Cp, H, W]
    if (i >= total) return;
    const int ox = (int)(i % W), oy = (int)((i / W) % H);
    const size_t pc = i / ((size_t)W * H);                             // (b 3 + plane) Cp + c
    const int c = (int)(pc % Cp), plane = (int)((pc / Cp) % 3);
    const size_t b = pc / ((size_t)3 * Cp);
    const int sy = H - 1 - oy, sx = plane == 2 ? W - 1 - ox : ox;
    planes[i] = x[((b * H + sy) * W + sx) * 3 * Cp + plane * Cp + c];
}

static inline dim3 grid_for(size_t total) { return dim3((unsigned)((total + 255) / 256)); }

}  // namespace i2p
}  // namespace r3d

using namespace r3d;
using namespace r3d::i2p;

extern "C" int r3d_i2p_attention(const float* q, const float* kv, int B, int N, int L, int C, int heads, float scale, float* out,
                                 r3d_stream_t stream)
{
    if (!q || !kv || !out) { set_error("i2p_attention: NULL pointer"); return R3D_ERR_INVALID_ARG; }
    if (B <= 0 || N <= 0 || L <= 0 || heads <= 0 || C <= 0 || B > 65535 || heads > 65535)
        { set_error("i2p_attention: bad argument (B, N, L, C, heads > 0; B, heads <= 65535)"); return R3D_ERR_INVALID_ARG; }
    const int D = C / heads;
    if (C % heads || D % 16 || D > 256)
        { set_error("i2p_attention: head dimension C / heads = %d / %d is not a multiple of 16 in 16 .. 256", C, heads); return R3D_ERR_INVALID_ARG; }
    if (!(fabsf(scale) <= 3.402823466e38f)) { set_error("i2p_attention: scale is not finite"); return R3D_ERR_INVALID_ARG; }
    if (!below_2_31("i2p_attention", "B N C", (double)B * N * C, "elements") || !below_2_31("i2p_attention", "2 B L C", 2.0 * B * L * C, "elements"))
        return R3D_ERR_INVALID_ARG;
    if (!aligned16(q) || !aligned16(kv) || !aligned16(out)) { set_error("i2p_attention: q, kv and out must be 16-byte aligned"); return R3D_ERR_INVALID_ARG; }
    const size_t nq = (size_t)B * N * C;
    const Span spans[] = {writes(out, nq), reads(q, nq), reads(kv, (size_t)B * L * 2 * C)};
    if (clash(spans)) { set_error("i2p_attention: out overlaps q or kv"); return R3D_ERR_INVALID_ARG; }
    const dim3 grid((N + QB - 1) / QB, heads, B);
    hipStream_t st = (hipStream_t)stream;
    if (D <= 64) hipLaunchKernelGGL(i2p_attention<64>, grid, dim3(256), 0, st, q, kv, N, L, C, D, scale, out);
    else if (D <= 128) hipLaunchKernelGGL(i2p_attention<128>, grid, dim3(256), 0, st, q, kv, N, L, C, D, scale, out);
    else hipLaunchKernelGGL(i2p_attention<256>, grid, dim3(256), 0, st, q, kv, N, L, C, D, scale, out);
    return check_launch("i2p_attention");
}

extern "C" int r3d_i2p_upsample2x(const float* x, int B, int H, int W, int C, float* y, r3d_stream_t stream)
{
    if (!x || !y) { set_error("i2p_upsample2x: NULL pointer"); return R3D_ERR_INVALID_ARG; }
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0) { set_error("i2p_upsample2x: bad argument (B, H, W, C > 0)"); return R3D_ERR_INVALID_ARG; }
    if (!below_2_31("i2p_upsample2x", "4 B H W C", 4.0 * B * H * W * C, "elements")) return R3D_ERR_INVALID_ARG;
    const size_t nin = (size_t)B * H * W * C, total = 4 * nin;
    if (overlap(y, total, x, nin)) { set_error("i2p_upsample2x: x and y overlap"); return R3D_ERR_INVALID_ARG; }
    hipLaunchKernelGGL(i2p_upsample2x, grid_for(total), dim3(256), 0, (hipStream_t)stream, x, H, W, C, total, y);
    return check_launch("i2p_upsample2x");
}

extern "C" int r3d_i2p_pixel_shuffle(const float* x, int B, int h, int w, int Co, float* y, int y_cstride, int y_coffset, r3d_stream_t stream)
{
    if (!x || !y) { set_error("i2p_pixel_shuffle: NULL pointer"); return R3D_ERR_INVALID_ARG; }
    if (B <= 0 || h <= 0 || w <= 0 || Co <= 0) { set_error("i2p_pixel_shuffle: bad argument (B, h, w, Co > 0)"); return R3D_ERR_INVALID_ARG; }
    if (y_coffset < 0 || y_cstride <= 0 || (long long)y_coffset + Co > y_cstride)
        { set_error("i2p_pixel_shuffle: channels [%d, %d + %d) outside a row of %d", y_coffset, y_coffset, Co, y_cstride); return R3D_ERR_INVALID_ARG; }
    if (!below_2_31("i2p_pixel_shuffle", "4 B h w y_cstride", 4.0 * B * h * w * y_cstride, "elements")) return R3D_ERR_INVALID_ARG;
    const size_t total = (size_t)B * h * w * 4 * Co;
    if (overlap(y, (size_t)B * h * w * 4 * y_cstride, x, total)) { set_error("i2p_pixel_shuffle: x and y overlap"); return R3D_ERR_INVALID_ARG; }
    hipLaunchKernelGGL(i2p_pixel_shuffle, grid_for(total), dim3(256), 0, (hipStream_t)stream, x, h, w, Co, total, y, y_cstride, y_coffset);
    return check_launch("i2p_pixel_shuffle");
}

extern "C" int r3d_i2p_copy_channels(const float* x, size_t M, int C, float* y, int y_cstride, int y_coffset, r3d_stream_t stream)
{
    if (!x || !y) { set_error("i2p_copy_channels: NULL pointer"); return R3D_ERR_INVALID_ARG; }
    if (M == 0 || C <= 0) { set_error("i2p_copy_channels: bad argument (M, C > 0)"); return R3D_ERR_INVALID_ARG; }
    if (y_coffset < 0 || y_cstride <= 0 || (long long)y_coffset + C > y_cstride)
        { set_error("i2p_copy_channels: channels [%d, %d + %d) outside a row of %d", y_coffset, y_coffset, C, y_cstride); return R3D_ERR_INVALID_ARG; }
    if (!below_2_31("i2p_copy_channels", "M y_cstride", (double)M * y_cstride, "elements")) return R3D_ERR_INVALID_ARG;
    const size_t total = M * C;
    if (overlap(y, M * y_cstride, x, total)) { set_error("i2p_copy_channels: x and y overlap"); return R3D_ERR_INVALID_ARG; }
    hipLaunchKernelGGL(i2p_copy_channels, grid_for(total), dim3(256), 0, (hipStream_t)stream, x, C, total, y, y_cstride, y_coffset);
    return check_launch("i2p_copy_channels");
}

extern "C" int r3d_i2p_nchw_to_cl(const float* x, int B, int C, int H, int W, float* y, r3d_stream_t stream)
{
    if (!x || !y) { set_error("i2p_nchw_to_cl: NULL pointer"); return R3D_ERR_INVALID_ARG; }
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) { set_error("i2p_nchw_to_cl: bad argument (B, C, H, W > 0)"); return R3D_ERR_INVALID_ARG; }
    if (!below_2_31("i2p_nchw_to_cl", "B C H W", (double)B * C * H * W, "elements")) return R3D_ERR_INVALID_ARG;
    const size_t total = (size_t)B * C * H * W;
    if (overlap(y, total, x, total)) { set_error("i2p_nchw_to_cl: x and y overlap"); return R3D_ERR_INVALID_ARG; }
    hipLaunchKernelGGL(i2p_nchw_to_cl, grid_for(total), dim3(256), 0, (hipStream_t)stream, x, C, (size_t)H * W, total, y);
    return check_launch("i2p_nchw_to_cl");
}

extern "C" int r3d_i2p_planes_out(const float* x, int B, int H, int W, int Cp, float* planes, r3d_stream_t stream)
{
    if (!x || !planes) { set_error("i2p_planes_out: NULL pointer"); return R3D_ERR_INVALID_ARG; }
    if (B <= 0 || H <= 0 || W <= 0 || Cp <= 0) { set_error("i2p_planes_out: bad argument (B, H, W, Cp > 0)"); return R3D_ERR_INVALID_ARG; }
    if (!below_2_31("i2p_planes_out", "3 B H W Cp", 3.0 * B * H * W * Cp, "elements")) return R3D_ERR_INVALID_ARG;
    const size_t total = (size_t)B * H * W * 3 * Cp;
    if (overlap(planes, total, x, total)) { set_error("i2p_planes_out: x and planes overlap"); return R3D_ERR_INVALID_ARG; }
    hipLaunchKernelGGL(i2p_planes_out, grid_for(total), dim3(256), 0, (hipStream_t)stream, x, H, W, Cp, total, planes);
    return check_launch("i2p_planes_out");
}
