// The second half of the face-vid2vid torso network, inference only, exact fp32: Generator (modules/real3d/facev2v_warp/
// network2.py:248-301) = a trilinear warp of the appearance volume + a 2D decoder, and occlusion_2_predictor (model2.py:212-219).
//
// Activations are channel-last fp32.  Every product of the convolutions runs on v_mfma_f32_16x16x4_f32 (exact f32 products, an fmaf chain
// per k step); the warp, the prologue and the epilogues run on the fp32 VALU.  Kernels:
//   torso_volume_to_cl   [N, C, D, H, W] -> [N, D, H, W, C]: the clip-constant source of the warp, so that one tap is one contiguous read
//                        of the C channels.
//   torso_warp           F.grid_sample(fs, grid, align_corners=True, padding_mode='border') on the 5-D volume, 8 taps per output value.
//   torso_conv<VEC, WM, WN, TM, TN>
//                        implicit-GEMM stride-1 convolution, zero padding ksize / 2: a (WM TM 16) x (WN TN 16) tile of pixels x output
//                        channels per 256-thread block, K = (ky, kx, ci) staged 32 at a time through two LDS buffers while the next two
//                        steps are in flight in registers.  Tap loads apply the prologue act(s[c] x + t[c]) (zero outside the image AFTER it:
//                        the reference pads the activated tensor) and nearest x2 up-sampling in the addressing; the epilogue adds the bias,
//                        applies LeakyReLU / sigmoid, adds a residual and writes channel-last and / or NCHW.  VEC: Cin % 4 == 0,
//                        channel-last input, 16-byte loads; otherwise one element per load (NCHW input, Cin = 65, 3, 1).
#include "r3d_common.h"
#include <math.h>
#include <initializer_list>

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

constexpr int BK = 32, LDK = BK + 4;     // LDS rows of 36 floats: 16-byte aligned, and 16 rows at one k offset touch 64 distinct banks

struct ConvArgs {
    const float* x; int B, Hs, Ws, Cin;          // stored input [B, Hs, Ws, Cin] (in_nchw: [B, Cin, Hs, Ws])
    int H, W;                                    // the conv's grid: Hs x Ws, or twice that (up: the input is x[h >> 1, w >> 1])
    int up, in_nchw, ks;
    const float* ps; const float* pt; float pslope;      // prologue a = ps[c] x + pt[c]; a < 0 ? pslope a : a  (ps == nullptr: none)
    const float* w; int Cout;                    // [Cout, ks, ks, Cin]
    const float* bias;                           // [Cout] or nullptr
    int act; float slope;                        // 0 none, 1 v < 0 ? slope v : v, 2 sigmoid
    const float* res;                            // [M, Cout] or nullptr (may alias y: each element is read, then written, by one lane)
    float* y; float* y_nchw;                     // [B, H, W, Cout] and / or [B, Cout, H, W]
    int M, K;
    int ntn;                                     // tiles along Cout (set by the launcher)
};

__device__ __forceinline__ float leaky(float v, float slope) { return v < 0.0f ? slope * v : v; }

// the position of a running k = (ky ks + kx) Cin + ci
struct KPos {
    int ci, kx, ky;
    __device__ __forceinline__ void init(int k, int Cin, int ks) { ci = k % Cin; const int tap = k / Cin; ky = tap / ks; kx = tap - ky * ks; }
    __device__ __forceinline__ void advance(int dk, int Cin, int ks)
    {
        ci += dk;
        while (ci >= Cin) { ci -= Cin; if (++kx == ks) { kx = 0; ++ky; } }
    }
};

template <bool VEC, int WM, int WN, int TM, int TN>
__global__ void __launch_bounds__(256) torso_conv(ConvArgs g)
{
    static_assert(WM * WN == 4, "four waves");
    constexpr int BM = WM * TM * 16, BN = WN * TN * 16;
    constexpr int AV = BM / 32, WV = (BN + 31) / 32;           // VEC: float4 loads per thread (A, W)
    constexpr int AS = BM / 8, WS = BN / 8, KSTEP = 256 / BM;  // scalar: elements per thread; A's k stride between them
    __shared__ __attribute__((aligned(16))) float As[2][BM * LDK];
    __shared__ __attribute__((aligned(16))) float Ws[2][BN * LDK];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    // Blocks are dealt to the 8 XCDs round-robin, and each XCD has an L2 of its own: block b takes tile (b % 8) (nblk / 8) + b / 8, so that
    // one XCD works on neighbouring pixel tiles (which share their taps' rows) and on all channel tiles of each (which share the taps).
    const int nblk = gridDim.x, bid = blockIdx.x;
    const int tile = nblk % 8 == 0 ? (bid % 8) * (nblk / 8) + bid / 8 : bid;
    const int m0 = (tile / g.ntn) * BM, n0 = (tile % g.ntn) * BN;
    const int pad = g.ks >> 1, hw = g.H * g.W;
    const int nsteps = (g.K + BK - 1) / BK;

    // ---- loader state ---------------------------------------------------------------------------------------------------------------
    // VEC: slot j is row (t >> 3) + 32 j of the tile, k entries 4 (t & 7) .. + 3 of the step (one tap, four channels);
    // scalar: row t % BM, k entries t / BM + KSTEP j (consecutive lanes read consecutive pixels: coalesced for an NCHW input)
    constexpr int NR = VEC ? AV : 1;
    int roy[NR], rox[NR]; size_t rbase[NR];                     // a row's pixel (oy < 0: no such row) and its sample's offset
#pragma unroll
    for (int j = 0; j < NR; ++j) {
        const int m = m0 + (VEC ? (t >> 3) + 32 * j : t % BM);
        if (m < g.M) {
            const int b = m / hw, r = m - b * hw;
            roy[j] = r / g.W; rox[j] = r - roy[j] * g.W;
            rbase[j] = (size_t)b * g.Hs * g.Ws * g.Cin;
        } else { roy[j] = -1000000; rox[j] = 0; rbase[j] = 0; }
    }
    KPos kp;
    kp.init(VEC ? 4 * (t & 7) : t / BM, g.Cin, g.ks);
    int kcur = VEC ? 4 * (t & 7) : t / BM;                      // the k of kp

    const int wm = (wave / WN) * TM * 16, wn = (wave % WN) * TN * 16;
    f32x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    // the registers of one k step in flight between its global loads and its LDS stores
    struct Stage {
        float4 av4[VEC ? AV : 1], wv4[VEC ? WV : 1], ps4, pt4;
        float avs[VEC ? 1 : AS], wvs[VEC ? 1 : WS], pss[VEC ? 1 : AS], pts[VEC ? 1 : AS];
        unsigned inside;                                        // bit j: slot / element j came from inside the image
    };
    int knext = 0;                                              // the step the next load() fetches (steps are loaded in order)

    auto load = [&](Stage& r) {
        r.inside = 0;
        if (knext >= nsteps) return;
        const int k0 = knext * BK;
        ++knext;
        if constexpr (VEC) {
            const bool kin = kcur < g.K;
#pragma unroll
            for (int j = 0; j < AV; ++j) {
                const int iy = roy[j] - pad + kp.ky, ix = rox[j] - pad + kp.kx;
                r.av4[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (kin && iy >= 0 && iy < g.H && ix >= 0 && ix < g.W) {
                    const size_t off = rbase[j] + ((size_t)(iy >> g.up) * g.Ws + (ix >> g.up)) * g.Cin + kp.ci;
                    r.av4[j] = *reinterpret_cast<const float4*>(g.x + off);
                    r.inside |= 1u << j;
                }
            }
            if (g.ps && kin) {
                r.ps4 = *reinterpret_cast<const float4*>(g.ps + kp.ci);
                r.pt4 = *reinterpret_cast<const float4*>(g.pt + kp.ci);
            }
#pragma unroll
            for (int j = 0; j < WV; ++j) {
                const int row = (t >> 3) + 32 * j, n = n0 + row;
                r.wv4[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (row < BN && n < g.Cout && kin) r.wv4[j] = *reinterpret_cast<const float4*>(g.w + (size_t)n * g.K + kcur);
            }
            kp.advance(BK, g.Cin, g.ks);
            kcur += BK;
        } else {
#pragma unroll
            for (int j = 0; j < AS; ++j) {
                const int iy = roy[0] - pad + kp.ky, ix = rox[0] - pad + kp.kx;
                r.avs[j] = 0.0f; r.pss[j] = 1.0f; r.pts[j] = 0.0f;
                if (kcur < g.K && iy >= 0 && iy < g.H && ix >= 0 && ix < g.W) {
                    const int sy = iy >> g.up, sx = ix >> g.up;
                    const size_t off = g.in_nchw ? rbase[0] + ((size_t)kp.ci * g.Hs + sy) * g.Ws + sx
                                                 : rbase[0] + ((size_t)sy * g.Ws + sx) * g.Cin + kp.ci;
                    r.avs[j] = g.x[off];
                    if (g.ps) { r.pss[j] = g.ps[kp.ci]; r.pts[j] = g.pt[kp.ci]; }
                    r.inside |= 1u << j;
                }
                kp.advance(KSTEP, g.Cin, g.ks);
                kcur += KSTEP;
            }
#pragma unroll
            for (int j = 0; j < WS; ++j) {
                const int e = t + 256 * j, n = n0 + (e >> 5), k = k0 + (e & 31);
                r.wvs[j] = (n < g.Cout && k < g.K) ? g.w[(size_t)n * g.K + k] : 0.0f;
            }
        }
    };
    auto store = [&](const Stage& r, int buf) {
        if constexpr (VEC) {
#pragma unroll
            for (int j = 0; j < AV; ++j) {
                float4 v = r.av4[j];
                if (g.ps && (r.inside >> j & 1)) {
                    v.x = leaky(fmaf(r.ps4.x, v.x, r.pt4.x), g.pslope); v.y = leaky(fmaf(r.ps4.y, v.y, r.pt4.y), g.pslope);
                    v.z = leaky(fmaf(r.ps4.z, v.z, r.pt4.z), g.pslope); v.w = leaky(fmaf(r.ps4.w, v.w, r.pt4.w), g.pslope);
                }
                *reinterpret_cast<float4*>(&As[buf][((t >> 3) + 32 * j) * LDK + 4 * (t & 7)]) = v;
            }
#pragma unroll
            for (int j = 0; j < WV; ++j) {
                const int row = (t >> 3) + 32 * j;
                if (row < BN) *reinterpret_cast<float4*>(&Ws[buf][row * LDK + 4 * (t & 7)]) = r.wv4[j];
            }
        } else {
#pragma unroll
            for (int j = 0; j < AS; ++j) {
                float v = r.avs[j];
                if (g.ps && (r.inside >> j & 1)) v = leaky(fmaf(r.pss[j], v, r.pts[j]), g.pslope);
                As[buf][(t % BM) * LDK + t / BM + KSTEP * j] = v;
            }
#pragma unroll
            for (int j = 0; j < WS; ++j) { const int e = t + 256 * j; Ws[buf][(e >> 5) * LDK + (e & 31)] = r.wvs[j]; }
        }
    };
    // one k step of the block's tile out of LDS buffer `cur`
    auto compute = [&](int cur) {
        // lane group lane >> 4 owns k entries 8 (lane >> 4) .. + 7 of the step, one per MFMA: the order of the sum is fixed, whichever
        float a[TM][8], b[TN][8];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const float* p = &As[cur][(wm + i * 16 + (lane & 15)) * LDK + 8 * (lane >> 4)];
            const float4 lo = *reinterpret_cast<const float4*>(p), hi = *reinterpret_cast<const float4*>(p + 4);
            a[i][0] = lo.x; a[i][1] = lo.y; a[i][2] = lo.z; a[i][3] = lo.w; a[i][4] = hi.x; a[i][5] = hi.y; a[i][6] = hi.z; a[i][7] = hi.w;
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const float* p = &Ws[cur][(wn + j * 16 + (lane & 15)) * LDK + 8 * (lane >> 4)];
            const float4 lo = *reinterpret_cast<const float4*>(p), hi = *reinterpret_cast<const float4*>(p + 4);
            b[j][0] = lo.x; b[j][1] = lo.y; b[j][2] = lo.z; b[j][3] = lo.w; b[j][4] = hi.x; b[j][5] = hi.y; b[j][6] = hi.z; b[j][7] = hi.w;
        }
#pragma unroll
        for (int kk = 0; kk < 8; ++kk)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][kk], b[j][kk], acc[i][j], 0, 0, 0);
    };

    // Two register stages and two LDS buffers: step s is computed out of buffer s & 1 while step s + 1 (loaded one iteration earlier)
    // goes from its stage into the other buffer and step s + 3 leaves for that stage, so a load has two compute phases to arrive.
    Stage r0, r1;
    load(r0);                       // step 0
    store(r0, 0);
    load(r0);                       // step 1
    load(r1);                       // step 2
    __syncthreads();
    for (int s = 0; s < nsteps; s += 2) {
        compute(0);
        if (s + 1 < nsteps) store(r0, 1);
        load(r0);                   // step s + 3
        __syncthreads();
        if (s + 1 >= nsteps) break;
        compute(1);
        if (s + 2 < nsteps) store(r1, 0);
        load(r1);                   // step s + 4
        __syncthreads();
    }

    // D layout of 16x16x4: column lane & 15, rows 4 (lane >> 4) + r.  The bias and the residuals are fetched before they are needed.
    float bias[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = n0 + wn + j * 16 + (lane & 15);
        bias[j] = (g.bias && n < g.Cout) ? g.bias[n] : 0.0f;
    }
    float res[TM][4][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int m = m0 + wm + i * 16 + (lane >> 4) * 4 + r, n = n0 + wn + j * 16 + (lane & 15);
                res[i][r][j] = (g.res && m < g.M && n < g.Cout) ? g.res[(size_t)m * g.Cout + n] : 0.0f;
            }
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + wm + i * 16 + (lane >> 4) * 4 + r;
            if (m >= g.M) continue;
            const int b = m / hw, px = m - b * hw;
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int n = n0 + wn + j * 16 + (lane & 15);
                if (n >= g.Cout) continue;
                float v = acc[i][j][r] + bias[j];
                if (g.act == 1) v = leaky(v, g.slope);
                else if (g.act == 2) v = 1.0f / (1.0f + expf(-v));
                v += res[i][r][j];
                if (g.y) g.y[(size_t)m * g.Cout + n] = v;
                if (g.y_nchw) g.y_nchw[((size_t)b * g.Cout + n) * hw + px] = v;
            }
        }
}

template <bool VEC, int WM, int WN, int TM, int TN>
static void launch_conv(ConvArgs g, hipStream_t st)
{
    constexpr int BM = WM * TM * 16, BN = WN * TN * 16;
    g.ntn = (g.Cout + BN - 1) / BN;
    const long long nblk = (long long)((g.M + BM - 1) / BM) * g.ntn;
    hipLaunchKernelGGL((torso_conv<VEC, WM, WN, TM, TN>), dim3((unsigned)nblk), dim3(256), 0, st, g);
}

}  // namespace torso
}  // namespace r3d

using namespace r3d;
using namespace r3d::torso;

// [a, a + na) and [b, b + nb) (counts of floats) share an element
static bool overlap(const float* a, size_t na, const float* b, size_t nb) { return a < b + nb && b < a + na; }

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

extern "C" int r3d_torso_conv(const float* x, int B, int Hs, int Ws, int Cin, int in_nchw, int upsample, const float* pro_scale,
                              const float* pro_shift, float pro_slope, const float* w, const float* bias, int Cout, int ksize, int act,
                              float act_slope, const float* residual, float* y, float* y_nchw, r3d_stream_t stream)
{
    if (!x || !w || (!y && !y_nchw) || (!pro_scale) != (!pro_shift)) { set_error("torso_conv: NULL pointer"); return R3D_ERR_INVALID_ARG; }
    if (B <= 0 || Hs <= 0 || Ws <= 0 || Cin <= 0 || Cout <= 0 || Cin > 4096 || Cout > 4096)
        { set_error("torso_conv: bad argument (B, Hs, Ws > 0, 1 <= Cin, Cout <= 4096)"); return R3D_ERR_INVALID_ARG; }
    if (ksize != 1 && ksize != 3 && ksize != 7) { set_error("torso_conv: ksize %d is not 1, 3 or 7", ksize); return R3D_ERR_INVALID_ARG; }
    if (upsample != 0 && upsample != 1) { set_error("torso_conv: upsample %d is not 0 or 1", upsample); return R3D_ERR_INVALID_ARG; }
    if (act < 0 || act > 2) { set_error("torso_conv: act %d is not 0 (none), 1 (leaky) or 2 (sigmoid)", act); return R3D_ERR_INVALID_ARG; }
    const int H = Hs << upsample, W = Ws << upsample;
    if ((double)B * H * W > 2147483647.0 || (double)B * H * W * (Cin > Cout ? Cin : Cout) > 9.0e18)
        { set_error("torso_conv: more than 2^31 - 1 output pixels"); return R3D_ERR_INVALID_ARG; }
    const size_t nin = (size_t)B * Hs * Ws * Cin, nout = (size_t)B * H * W * Cout, nw = (size_t)Cout * ksize * ksize * Cin;
    for (float* o : {y, y_nchw}) {
        if (!o) continue;
        if (overlap(o, nout, x, nin) || overlap(o, nout, w, nw) || (bias && overlap(o, nout, bias, Cout)) ||
            (pro_scale && (overlap(o, nout, pro_scale, Cin) || overlap(o, nout, pro_shift, Cin))))
            { set_error("torso_conv: an output overlaps x, w, bias or the prologue"); return R3D_ERR_INVALID_ARG; }
        if (residual && residual != y && overlap(o, nout, residual, nout))
            { set_error("torso_conv: an output overlaps the residual without y being the residual"); return R3D_ERR_INVALID_ARG; }
    }
    if (y && y_nchw && overlap(y, nout, y_nchw, nout)) { set_error("torso_conv: y and y_nchw overlap"); return R3D_ERR_INVALID_ARG; }
    hipStream_t st = (hipStream_t)stream;
    ConvArgs g = {};
    g.x = x; g.B = B; g.Hs = Hs; g.Ws = Ws; g.Cin = Cin; g.H = H; g.W = W; g.up = upsample; g.in_nchw = in_nchw ? 1 : 0; g.ks = ksize;
    g.ps = pro_scale; g.pt = pro_shift; g.pslope = pro_slope; g.w = w; g.Cout = Cout; g.bias = bias; g.act = act; g.slope = act_slope;
    g.res = residual; g.y = y; g.y_nchw = y_nchw; g.M = B * H * W; g.K = ksize * ksize * Cin;
    auto aligned = [](const void* p) { return p == nullptr || ((uintptr_t)p & 15) == 0; };
    const bool vec = !in_nchw && Cin % 4 == 0 && aligned(x) && aligned(w) && aligned(pro_scale) && aligned(pro_shift);
    // the tile follows Cout: 64 x 64 (pixels x channels) or 32 x 64, 128 x 32 up to 32 channels, 128 x 16 up to 16 (out_conv's 3, the predictor's 1)
    // (32 x 64 where 64 x 64 tiles would give the 256 CUs fewer than two blocks each: the 64^2 layers, one wave per SIMD otherwise)
    const long long big = (long long)((g.M + 63) / 64) * ((Cout + 63) / 64);
    if (Cout > 32 && big < 512) { if (vec) launch_conv<true, 2, 2, 1, 2>(g, st); else launch_conv<false, 2, 2, 1, 2>(g, st); }
    else if (Cout > 32) { if (vec) launch_conv<true, 2, 2, 2, 2>(g, st); else launch_conv<false, 2, 2, 2, 2>(g, st); }
    else if (Cout > 16) { if (vec) launch_conv<true, 4, 1, 2, 2>(g, st); else launch_conv<false, 4, 1, 2, 2>(g, st); }
    else { if (vec) launch_conv<true, 4, 1, 2, 1>(g, st); else launch_conv<false, 4, 1, 2, 1>(g, st); }
    return check_launch("torso_conv");
}
