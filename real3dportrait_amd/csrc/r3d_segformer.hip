// SegFormerSECC2PlaneBackbone front half, mode b0 (modules/real3d/segformer.py:672-731): the prenet 1x1 Conv2dLayer, the MiT-b0
// encoder (mix_vit, :244-413) and the SegFormerHead (fuse_head, :463-537), inference only, exact fp32.
//
// Activations are token-major (NHWC) fp32.  Every matrix product runs on v_mfma_f32_16x16x4_f32 (exact f32 products, an fmaf chain
// per k step); LayerNorm statistics, softmax, GELU and the depthwise conv run on the fp32 VALU.  Kernels:
//   seg_gemm<AMODE, HEAD>  Y = epilogue(A . W^T): 64 x 64 output tile per 256-thread block, K staged through LDS 16 at a time.
//                          A is read as  ROW  (token rows, optional LayerNorm prologue),  CONV  (implicit-GEMM strided conv over an NHWC
//                          input, k = (ky, kx, ci)),  PRENET  (stage 1: the 7x7/s4 conv whose taps are the prenet's 1x1 conv of the raw
//                          NCHW image, zero outside the image).  Epilogue: + bias, exact GELU, + residual;  HEAD: + bilinear samples of
//                          the three folded low-resolution maps + constant, BatchNorm scale/shift, ReLU, NCHW store.
//   seg_layernorm          one wave per token row, two-pass statistics of the row shifted by its first entry.
//   seg_attention          one block per (batch, head, 64 queries): keys / values staged in LDS 64 at a time, S = QK^T and O = PV on the
//                          MFMA, online max-subtracted softmax (d = 32 for every MiT-b0 stage).
//   seg_dwconv_gelu        depthwise 3x3 + bias + exact GELU on [B, H, W, C].
#include "r3d_common.h"
#include <math.h>

namespace r3d {
namespace seg {

enum { A_ROW = 0, A_CONV = 1, A_PRENET = 2 };
constexpr int BM = 64, BN = 64, BK = 16, LDA = BM + 4, LDW = BN + 4;

struct GemmArgs {
    const float* a; int M, K, lda;             // ROW: A[m * lda + k]
    const float* ln_g; const float* ln_b; float ln_eps;     // ROW: LayerNorm prologue over the K entries of a row (ln_g == nullptr: none)
    // CONV / PRENET: input [B, Hin, Win, Cin] NHWC (PRENET: [B, Craw, Hin, Win] NCHW, Cin = 3 prenet outputs), output grid Ho x Wo
    int Hin, Win, Cin, Ho, Wo, ks, stride, pad;
    const float* pw; const float* pb; float pgain; int Craw;    // PRENET: Conv2dLayer weight [Cin, Craw], bias, weight gain
    const float* w; int N;                      // W [N, K]
    const float* bias;                          // [N] or nullptr
    int gelu;
    const float* res;                           // [M, ldy] residual or nullptr (may alias y: each element is read, then written, by one lane)
    float* y; int ldy;
    // HEAD
    const float* f2; const float* f3; const float* f4;      // folded maps [B, H1/2 x W1/2 | H1/4 x W1/4 | H1/8 x W1/8, N]
    const float* hconst; const float* bn_s; const float* bn_t;
    int H1, W1;
};

// one element of A (zero outside [M, K] and outside the zero-padded input)
template <int AMODE>
__device__ __forceinline__ float load_a(const GemmArgs& g, int m, int k, float sh, float mu, float rs)
{
    if (m >= g.M || k >= g.K) return 0.0f;
    if (AMODE == A_ROW) {
        float v = g.a[(size_t)m * g.lda + k];
        if (g.ln_g) v = ((v - sh) - mu) * rs * g.ln_g[k] + g.ln_b[k];
        return v;
    } else {
        const int hw = g.Ho * g.Wo, b = m / hw, r = m - b * hw, oy = r / g.Wo, ox = r - oy * g.Wo;
        const int ci = k % g.Cin, tap = k / g.Cin, ky = tap / g.ks, kx = tap - ky * g.ks;
        const int iy = oy * g.stride - g.pad + ky, ix = ox * g.stride - g.pad + kx;
        if (iy < 0 || iy >= g.Hin || ix < 0 || ix >= g.Win) return 0.0f;
        if (AMODE == A_CONV) return g.a[(((size_t)b * g.Hin + iy) * g.Win + ix) * g.Cin + ci];
        // the prenet's output at (iy, ix): its 1x1 conv with w * gain (networks_stylegan2.py:177), then + bias (linear act, gain 1)
        const size_t plane = (size_t)g.Hin * g.Win;
        const float* src = g.a + (size_t)b * g.Craw * plane + (size_t)iy * g.Win + ix;
        float acc = 0.0f;
        for (int j = 0; j < g.Craw; ++j) acc = fmaf(g.pw[ci * g.Craw + j] * g.pgain, src[j * plane], acc);
        return acc + g.pb[ci];
    }
}

__device__ __forceinline__ float bilerp(const float* f, int b, int h, int w, int N, int n, int y, int x, int H1, int W1)
{
    // F.interpolate(mode='bilinear', align_corners=False) from h x w to H1 x W1
    const float sy = fmaxf(((float)y + 0.5f) * ((float)h / (float)H1) - 0.5f, 0.0f);
    const float sx = fmaxf(((float)x + 0.5f) * ((float)w / (float)W1) - 0.5f, 0.0f);
    const int y0 = min((int)sy, h - 1), x0 = min((int)sx, w - 1);
    const int y1 = min(y0 + 1, h - 1), x1 = min(x0 + 1, w - 1);
    const float ly = sy - (float)y0, lx = sx - (float)x0;
    const float* base = f + (size_t)b * h * w * N + n;
    const float v00 = base[((size_t)y0 * w + x0) * N], v01 = base[((size_t)y0 * w + x1) * N];
    const float v10 = base[((size_t)y1 * w + x0) * N], v11 = base[((size_t)y1 * w + x1) * N];
    return (1.0f - ly) * ((1.0f - lx) * v00 + lx * v01) + ly * ((1.0f - lx) * v10 + lx * v11);
}

template <int AMODE, bool HEAD>
__global__ void __launch_bounds__(256) seg_gemm(GemmArgs g)
{
    __shared__ float As[BK * LDA];
    __shared__ float Ws[BK * LDW];
    __shared__ float s_sh[BM], s_mu[BM], s_rs[BM];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    const int lr = t >> 2, lk = (t & 3) * 4;          // loader: row / column lr of the tile, k entries lk .. lk + 3

    float sh = 0.0f, mu = 0.0f, rs = 0.0f;
    if (AMODE == A_ROW && g.ln_g) {
        // statistics of row m0 + lr by the 4 lanes t & ~3, as seg_layernorm: shifted by the row's first entry x0, two passes (the mean of
        // x - x0, then the mean squared deviation)
        const int m = m0 + lr;
        const float* row = g.a + (size_t)m * g.lda;
        const float x0 = m < g.M ? row[0] : 0.0f;
        float s = 0.0f;
        if (m < g.M) for (int k = t & 3; k < g.K; k += 4) s += row[k] - x0;
        s += __shfl_xor(s, 1); s += __shfl_xor(s, 2);
        const float mean = s / (float)g.K;
        float q = 0.0f;
        if (m < g.M) for (int k = t & 3; k < g.K; k += 4) { const float d = (row[k] - x0) - mean; q = fmaf(d, d, q); }
        q += __shfl_xor(q, 1); q += __shfl_xor(q, 2);
        if ((t & 3) == 0) { s_sh[lr] = x0; s_mu[lr] = mean; s_rs[lr] = 1.0f / sqrtf(q / (float)g.K + g.ln_eps); }
        __syncthreads();
        sh = s_sh[lr]; mu = s_mu[lr]; rs = s_rs[lr];
    }

    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;     // the wave's 32 x 32 sub-tile: 2 x 2 MFMA tiles of 16 x 16
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    for (int k0 = 0; k0 < g.K; k0 += BK) {
        float av[4], wv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            av[j] = load_a<AMODE>(g, m0 + lr, k0 + lk + j, sh, mu, rs);
            const int n = n0 + lr, k = k0 + lk + j;
            wv[j] = (n < g.N && k < g.K) ? g.w[(size_t)n * g.K + k] : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) { As[(lk + j) * LDA + lr] = av[j]; Ws[(lk + j) * LDW + lr] = wv[j]; }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < BK; kk += 4) {
            const int k = kk + (lane >> 4);
            float a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                a[i] = As[k * LDA + wm + i * 16 + (lane & 15)];
                b[i] = Ws[k * LDW + wn + i * 16 + (lane & 15)];
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
    }

    // D layout of 16x16x4: column lane & 15, rows 4 (lane >> 4) + r
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + wm + i * 16 + (lane >> 4) * 4 + r, n = n0 + wn + j * 16 + (lane & 15);
                if (m >= g.M || n >= g.N) continue;
                float v = acc[i][j][r];
                if (HEAD) {
                    const int hw = g.H1 * g.W1, b = m / hw, p = m - b * hw, y = p / g.W1, x = p - y * g.W1;
                    v += bilerp(g.f4, b, g.H1 >> 3, g.W1 >> 3, g.N, n, y, x, g.H1, g.W1);
                    v += bilerp(g.f3, b, g.H1 >> 2, g.W1 >> 2, g.N, n, y, x, g.H1, g.W1);
                    v += bilerp(g.f2, b, g.H1 >> 1, g.W1 >> 1, g.N, n, y, x, g.H1, g.W1);
                    v = fmaxf(fmaf(v + g.hconst[n], g.bn_s[n], g.bn_t[n]), 0.0f);
                    g.y[((size_t)b * g.N + n) * hw + p] = v;
                } else {
                    if (g.bias) v += g.bias[n];
                    if (g.gelu) v = gelu_erf(v);
                    if (g.res) v += g.res[(size_t)m * g.ldy + n];
                    g.y[(size_t)m * g.ldy + n] = v;
                }
            }
}

// nn.LayerNorm over the C entries of each of M rows; one wave per row.  The statistics are those of the row shifted by its first entry x0
// (x - x0 is exact for entries within a factor 2 of x0): a constant row normalises to exactly 0, and a row whose mean is large next to its
// spread keeps the accuracy of its deviations (an unshifted fp32 mean of such a row is off by a rounding of the mean itself).
__global__ void __launch_bounds__(256) seg_layernorm(const float* x, int M, int C, const float* gam, const float* bet, float eps, float* y)
{
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const float* xr = x + (size_t)row * C;
    const float x0 = xr[0];
    float s = 0.0f;
    for (int c = lane; c < C; c += 64) s += xr[c] - x0;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
    const float mean = s / (float)C;          // of x - x0
    float q = 0.0f;
    for (int c = lane; c < C; c += 64) { const float d = (xr[c] - x0) - mean; q = fmaf(d, d, q); }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) q += __shfl_xor(q, o);
    const float rs = 1.0f / sqrtf(q / (float)C + eps);
    for (int c = lane; c < C; c += 64) y[(size_t)row * C + c] = ((xr[c] - x0) - mean) * rs * gam[c] + bet[c];
}

// depthwise 3x3 (padding 1, bias) + exact GELU on [B, H, W, C] (DWConv, segformer.py:394-404; Mlp.act, :92)
__global__ void __launch_bounds__(256) seg_dwconv_gelu(const float* x, int B, int H, int W, int C, const float* w, const float* bias, float* y)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, total = (size_t)B * H * W * C;
    if (i >= total) return;
    const int c = (int)(i % C);
    const size_t p = i / C;
    const int xx = (int)(p % W), yy = (int)((p / W) % H), b = (int)(p / ((size_t)W * H));
    float acc = 0.0f;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = yy + ky - 1;
        if (iy < 0 || iy >= H) continue;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = xx + kx - 1;
            if (ix < 0 || ix >= W) continue;
            acc = fmaf(w[c * 9 + ky * 3 + kx], x[(((size_t)b * H + iy) * W + ix) * C + c], acc);
        }
    }
    y[i] = gelu_erf(acc + bias[c]);
}

// Attention (segformer.py:135-158) with head_dim 32: q [B, N, C], kv [B, L, 2C] (k = channels [0, C), v = [C, 2C)), head h owns channels
// [32 h, 32 h + 32); out [B, N, C].  Block = 4 waves x 16 queries; keys in chunks of 64 through LDS; online softmax per query row.
constexpr int AQ = 64, AK = 64, KLD = 33;
__global__ void __launch_bounds__(256) seg_attention(const float* q, const float* kv, int N, int L, int C, float scale, float* out)
{
    __shared__ float Ks[AK * KLD], Vs[AK * KLD];
    __shared__ float Ps[4][16 * (AK + 1)];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int h = blockIdx.y, b = blockIdx.z, q0 = blockIdx.x * AQ + wave * 16;
    const int li = lane & 15, lg = lane >> 4;
    // Q as the A operand of 8 k-steps: lane holds Q[q0 + li][4 s + lg]
    float qa[8];
    {
        const int qi = q0 + li;
#pragma unroll
        for (int s = 0; s < 8; ++s) qa[s] = qi < N ? q[((size_t)b * N + qi) * C + h * 32 + 4 * s + lg] : 0.0f;
    }
    f32x4 o[2] = {f32x4{0.0f, 0.0f, 0.0f, 0.0f}, f32x4{0.0f, 0.0f, 0.0f, 0.0f}};
    float mrow[4], lrow[4];                              // rows 4 lg + r of the wave's 16
#pragma unroll
    for (int r = 0; r < 4; ++r) { mrow[r] = -INFINITY; lrow[r] = 0.0f; }
    float* P = Ps[wave];
    const float* kvb = kv + (size_t)b * L * 2 * C;

    for (int j0 = 0; j0 < L; j0 += AK) {
        __syncthreads();
        for (int e = t; e < AK * 32; e += 256) {
            const int kr = e >> 5, d = e & 31, key = j0 + kr;
            Ks[kr * KLD + d] = key < L ? kvb[(size_t)key * 2 * C + h * 32 + d] : 0.0f;
            Vs[kr * KLD + d] = key < L ? kvb[(size_t)key * 2 * C + C + h * 32 + d] : 0.0f;
        }
        __syncthreads();
        // S = Q K^T for 4 tiles of 16 keys
        f32x4 s[4];
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            s[kt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int st = 0; st < 8; ++st)
                s[kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[st], Ks[(kt * 16 + li) * KLD + 4 * st + lg], s[kt], 0, 0, 0);
        }
        // row maxima over the chunk (row 4 lg + r is spread over the 16 lanes of group lg and the 4 key tiles)
        float cmax[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float mx = -INFINITY;
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) {
                const float v = j0 + kt * 16 + li < L ? s[kt][r] * scale : -INFINITY;
                s[kt][r] = v;
                mx = fmaxf(mx, v);
            }
#pragma unroll
            for (int off = 8; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
            cmax[r] = mx;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float mnew = fmaxf(mrow[r], cmax[r]);        // finite: every chunk holds at least one valid key
            const float corr = expf(mrow[r] - mnew);           // 0 on the first chunk (exp(-inf))
            float ps = 0.0f;
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) {
                const float p = expf(s[kt][r] - mnew);         // 0 for masked keys
                ps += p;
                P[(lg * 4 + r) * (AK + 1) + kt * 16 + li] = p;
            }
#pragma unroll
            for (int off = 8; off >= 1; off >>= 1) ps += __shfl_xor(ps, off);
            lrow[r] = lrow[r] * corr + ps;
            mrow[r] = mnew;
            o[0][r] *= corr;
            o[1][r] *= corr;
        }
        __builtin_amdgcn_wave_barrier();      // P is written and read by this wave only (LDS accesses of a wave complete in order)
        // O += P V: A = P[i = li][key = 4 st + lg], B = V[key][d]
#pragma unroll
        for (int st = 0; st < AK / 4; ++st) {
            const float pa = P[li * (AK + 1) + 4 * st + lg];
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) o[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(pa, Vs[(4 * st + lg) * KLD + dt * 16 + li], o[dt], 0, 0, 0);
        }
        __builtin_amdgcn_wave_barrier();
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int qi = q0 + lg * 4 + r;
        if (qi >= N) continue;
        const float inv = 1.0f / lrow[r];
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) out[((size_t)b * N + qi) * C + h * 32 + dt * 16 + li] = o[dt][r] * inv;
    }
}

// The kernels index the rows of a call in int, up to the end of the last 64-row tile (m0 + lr of seg_gemm, q0 + li of seg_attention): M, or
// the product `expr` it stands for, rounded up to whole tiles, stays below 2^31.  Shown before the product is formed in int.
static bool rows_ok(const char* what, const char* expr, double rows)
{
    return below_2_31(what, expr, ceil(rows / BM) * BM, "rows with the last 64-row tile filled up");
}

static int launch_gemm(int amode, bool head, const GemmArgs& g, hipStream_t st, const char* what)
{
    dim3 grid((g.M - 1) / BM + 1, (g.N - 1) / BN + 1);
    if (head) hipLaunchKernelGGL((seg_gemm<A_ROW, true>), grid, dim3(256), 0, st, g);
    else if (amode == A_ROW) hipLaunchKernelGGL((seg_gemm<A_ROW, false>), grid, dim3(256), 0, st, g);
    else if (amode == A_CONV) hipLaunchKernelGGL((seg_gemm<A_CONV, false>), grid, dim3(256), 0, st, g);
    else hipLaunchKernelGGL((seg_gemm<A_PRENET, false>), grid, dim3(256), 0, st, g);
    return check_launch(what);
}

static int launch_layernorm(const float* x, int M, int C, const float* gam, const float* bet, float eps, float* y, hipStream_t st)
{
    hipLaunchKernelGGL(seg_layernorm, dim3((M - 1) / 4 + 1), dim3(256), 0, st, x, M, C, gam, bet, eps, y);
    return check_launch("secc_layernorm");
}

}  // namespace seg
}  // namespace r3d

using namespace r3d;
using namespace r3d::seg;

extern "C" int r3d_secc_embed1(const float* x, int B, int in_dim, int H, int W, const float* prenet_w, const float* prenet_b,
                               const float* w, const float* bias, const float* ln_g, const float* ln_b, float* y, r3d_stream_t stream)
{
    if (!x || !prenet_w || !prenet_b || !w || !bias || !ln_g || !ln_b || !y) { set_error("secc_embed1: NULL pointer"); return R3D_ERR_INVALID_ARG; }
    if (B <= 0 || (in_dim != 6 && in_dim != 9)) { set_error("secc_embed1: bad argument: B = %d, in_dim = %d (B > 0, in_dim 6 or 9)", B, in_dim); return R3D_ERR_INVALID_ARG; }
    if (H <= 0 || W <= 0 || H % 32 || W % 32) { set_error("secc_embed1: H and W must be positive multiples of 32"); return R3D_ERR_INVALID_ARG; }
    if ((size_t)(H / 32) * (W / 32) > 1024) { set_error("secc_embed1: L = (H/32)(W/32) > 1024 keys"); return R3D_ERR_INVALID_ARG; }
    if (!rows_ok("secc_embed1", "B (H/4)(W/4)", (double)B * (H / 4) * (W / 4))) return R3D_ERR_INVALID_ARG;
    const int M = B * (H / 4) * (W / 4);
    const Span spans[] = {writes(y, (size_t)M * 32), reads(x, (size_t)B * in_dim * H * W)};
    if (clash(spans)) { set_error("secc_embed1: x and y overlap"); return R3D_ERR_INVALID_ARG; }
    hipStream_t st = (hipStream_t)stream;
    GemmArgs g = {};
    g.a = x; g.Hin = H; g.Win = W; g.Cin = 3; g.Ho = H / 4; g.Wo = W / 4; g.ks = 7; g.stride = 4; g.pad = 3;
    g.pw = prenet_w; g.pb = prenet_b; g.pgain = (float)(1.0 / sqrt((double)in_dim)); g.Craw = in_dim;
    g.M = M; g.K = 7 * 7 * 3; g.w = w; g.N = 32; g.bias = bias; g.y = y; g.ldy = 32;
    int rc = launch_gemm(A_PRENET, false, g, st, "secc_embed1");
    if (rc) return rc;
    return launch_layernorm(y, g.M, 32, ln_g, ln_b, 1e-5f, y, st);
}

extern "C" int r3d_secc_conv(const float* x, int B, int Hin, int Win, int Cin, const float* w, const float* bias, int Cout, int ksize,
                             int stride, int pad, const float* ln_g, const float* ln_b, float ln_eps, float* y, r3d_stream_t stream)
{
    if (!x || !w || !bias || !y || (!ln_g) != (!ln_b)) { set_error("secc_conv: NULL pointer"); return R3D_ERR_INVALID_ARG; }
    if (B <= 0 || Hin <= 0 || Win <= 0 || stride <= 0)
        { set_error("secc_conv: bad argument: B = %d, Hin = %d, Win = %d, stride = %d must be positive", B, Hin, Win, stride); return R3D_ERR_INVALID_ARG; }
    if (Cin <= 0 || Cout <= 0 || Cin > 1024 || Cout > 1024)
        { set_error("secc_conv: bad argument: Cin = %d, Cout = %d outside 1 .. 1024", Cin, Cout); return R3D_ERR_INVALID_ARG; }
    if (ksize <= 0 || ksize > 8 || pad < 0 || pad >= ksize)
        { set_error("secc_conv: bad argument: ksize = %d outside 1 .. 8, or pad = %d outside 0 .. ksize - 1", ksize, pad); return R3D_ERR_INVALID_ARG; }
    // the padded input holds at least one window (C division truncates: without this, -stride < Hin + 2 pad - ksize < 0 gave Ho = 1)
    if (Hin < ksize - 2 * pad || Win < ksize - 2 * pad) { set_error("secc_conv: empty output (Hin or Win + 2 pad < ksize)"); return R3D_ERR_INVALID_ARG; }
    const long long Ho = ((long long)Hin + 2 * pad - ksize) / stride + 1, Wo = ((long long)Win + 2 * pad - ksize) / stride + 1;
    if (!rows_ok("secc_conv", "B Ho Wo", (double)B * (double)Ho * (double)Wo)) return R3D_ERR_INVALID_ARG;
    const int M = B * (int)Ho * (int)Wo, K = ksize * ksize * Cin;          // K <= 8 . 8 . 1024 by the bounds above
    const Span spans[] = {writes(y, (size_t)M * Cout), reads(x, (size_t)B * Hin * Win * Cin)};
    if (clash(spans)) { set_error("secc_conv: x and y overlap"); return R3D_ERR_INVALID_ARG; }
    hipStream_t st = (hipStream_t)stream;
    GemmArgs g = {};
    g.a = x; g.Hin = Hin; g.Win = Win; g.Cin = Cin; g.Ho = (int)Ho; g.Wo = (int)Wo; g.ks = ksize; g.stride = stride; g.pad = pad;
    g.M = M; g.K = K; g.w = w; g.N = Cout; g.bias = bias; g.y = y; g.ldy = Cout;
    int rc = launch_gemm(A_CONV, false, g, st, "secc_conv");
    if (rc || !ln_g) return rc;
    return launch_layernorm(y, g.M, Cout, ln_g, ln_b, ln_eps, y, st);
}

extern "C" int r3d_secc_linear(const float* x, int M, int K, const float* ln_g, const float* ln_b, float ln_eps, const float* w,
                               const float* bias, int N, int gelu, const float* residual, float* y, r3d_stream_t stream)
{
    if (!x || !w || !y || (!ln_g) != (!ln_b)) { set_error("secc_linear: NULL pointer"); return R3D_ERR_INVALID_ARG; }
    if (M <= 0 || K <= 0 || N <= 0 || K > 4096 || N > 4096)
        { set_error("secc_linear: bad argument: M = %d, K = %d, N = %d (M > 0; K, N in 1 .. 4096)", M, K, N); return R3D_ERR_INVALID_ARG; }
    if (!rows_ok("secc_linear", "M", (double)M)) return R3D_ERR_INVALID_ARG;
    // the residual may be y itself: each element is read, then written, by one lane
    const size_t ny = (size_t)M * N;
    const Span spans[] = {writes(y, ny), reads(x, (size_t)M * K), reads(residual == y ? nullptr : residual, ny)};
    if (clash(spans)) { set_error("secc_linear: y overlaps x, or residual without being residual"); return R3D_ERR_INVALID_ARG; }
    GemmArgs g = {};
    g.a = x; g.M = M; g.K = K; g.lda = K; g.ln_g = ln_g; g.ln_b = ln_b; g.ln_eps = ln_eps;
    g.w = w; g.N = N; g.bias = bias; g.gelu = gelu ? 1 : 0; g.res = residual; g.y = y; g.ldy = N;
    return launch_gemm(A_ROW, false, g, (hipStream_t)stream, "secc_linear");
}

extern "C" int r3d_secc_layernorm(const float* x, int M, int C, const float* ln_g, const float* ln_b, float eps, float* y, r3d_stream_t stream)
{
    if (!x || !ln_g || !ln_b || !y) { set_error("secc_layernorm: NULL pointer"); return R3D_ERR_INVALID_ARG; }
    if (M <= 0 || C <= 0 || !(eps > 0.0f))
        { set_error("secc_layernorm: bad argument: M = %d, C = %d, eps = %g must be positive", M, C, (double)eps); return R3D_ERR_INVALID_ARG; }
    const Span spans[] = {writes(y, (size_t)M * C), reads(x == y ? nullptr : x, (size_t)M * C)};
    if (clash(spans)) { set_error("secc_layernorm: x and y overlap (y may be x itself)"); return R3D_ERR_INVALID_ARG; }
    return launch_layernorm(x, M, C, ln_g, ln_b, eps, y, (hipStream_t)stream);
}

extern "C" int r3d_secc_attention(const float* q, const float* kv, int B, int N, int L, int C, int heads, float scale, float* out,
                                  r3d_stream_t stream)
{
    if (!q || !kv || !out) { set_error("secc_attention: NULL pointer"); return R3D_ERR_INVALID_ARG; }
    if (B <= 0 || N <= 0 || heads <= 0 || C != 32 * heads)
        { set_error("secc_attention: bad argument: B = %d, N = %d, C = %d, heads = %d (B, N, heads > 0; C = 32 heads)", B, N, C, heads); return R3D_ERR_INVALID_ARG; }
    if (L <= 0 || L > 1024) { set_error("secc_attention: L = %d keys outside 1 .. 1024", L); return R3D_ERR_INVALID_ARG; }
    if (!rows_ok("secc_attention", "N", (double)N)) return R3D_ERR_INVALID_ARG;
    const size_t nout = (size_t)B * N * C;
    const Span spans[] = {writes(out, nout), reads(kv, (size_t)B * L * 2 * C), reads(out == q ? nullptr : q, nout)};
    if (clash(spans)) { set_error("secc_attention: out overlaps kv, or q without being q"); return R3D_ERR_INVALID_ARG; }
    hipLaunchKernelGGL(seg_attention, dim3((N - 1) / AQ + 1, heads, B), dim3(256), 0, (hipStream_t)stream, q, kv, N, L, C, scale, out);
    return check_launch("secc_attention");
}

extern "C" int r3d_secc_dwconv_gelu(const float* x, int B, int H, int W, int C, const float* w, const float* bias, float* y, r3d_stream_t stream)
{
    if (!x || !w || !bias || !y) { set_error("secc_dwconv_gelu: NULL pointer"); return R3D_ERR_INVALID_ARG; }
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0)
        { set_error("secc_dwconv_gelu: bad argument: B = %d, H = %d, W = %d, C = %d must be positive", B, H, W, C); return R3D_ERR_INVALID_ARG; }
    // one thread an element, 256 a block: the block count is the grid's x, an unsigned below 2^31
    if (!below_2_31("secc_dwconv_gelu", "ceil(B H W C / 256)", ceil((double)B * H * W * C / 256.0), "blocks")) return R3D_ERR_INVALID_ARG;
    const size_t total = (size_t)B * H * W * C;
    const Span spans[] = {writes(y, total), reads(x, total)};
    if (clash(spans)) { set_error("secc_dwconv_gelu: bad argument (x and y overlap)"); return R3D_ERR_INVALID_ARG; }
    hipLaunchKernelGGL(seg_dwconv_gelu, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, B, H, W, C, w, bias, y);
    return check_launch("secc_dwconv_gelu");
}

extern "C" int r3d_secc_head(const float* c1, int B, int H1, int W1, const float* w1f, const float* f2, const float* f3, const float* f4,
                             const float* hconst, const float* bn_scale, const float* bn_shift, float* out, r3d_stream_t stream)
{
    if (!c1 || !w1f || !f2 || !f3 || !f4 || !hconst || !bn_scale || !bn_shift || !out) { set_error("secc_head: NULL pointer"); return R3D_ERR_INVALID_ARG; }
    if (B <= 0 || H1 <= 0 || W1 <= 0 || H1 % 8 || W1 % 8) { set_error("secc_head: H1, W1 (= H/4, W/4) must be positive multiples of 8"); return R3D_ERR_INVALID_ARG; }
    if (!rows_ok("secc_head", "B H1 W1", (double)B * H1 * W1)) return R3D_ERR_INVALID_ARG;
    const size_t hw = (size_t)H1 * W1, nout = (size_t)B * 256 * hw;
    const Span spans[] = {writes(out, nout), reads(c1, (size_t)B * hw * 32), reads(f2, (size_t)B * hw / 4 * 256), reads(f3, (size_t)B * hw / 16 * 256),
                          reads(f4, (size_t)B * hw / 64 * 256), reads(w1f, 256 * 32), reads(hconst, 256), reads(bn_scale, 256), reads(bn_shift, 256)};
    if (clash(spans)) { set_error("secc_head: out overlaps an input"); return R3D_ERR_INVALID_ARG; }
    GemmArgs g = {};
    g.a = c1; g.M = B * H1 * W1; g.K = 32; g.lda = 32; g.w = w1f; g.N = 256;
    g.f2 = f2; g.f3 = f3; g.f4 = f4; g.hconst = hconst; g.bn_s = bn_scale; g.bn_t = bn_shift; g.H1 = H1; g.W1 = W1; g.y = out;
    return launch_gemm(A_ROW, true, g, (hipStream_t)stream, "secc_head");
}
