// HuBERT's two convolutional ends (transformers HubertModel as data_gen/utils/process_audio/extract_hubert.py:13-80 runs it), inference only,
// exact fp32 (include/r3d_hip_hubert.h).  The transformer stack between them is r3d_secc_linear / r3d_i2p_attention /
// r3d_secc_layernorm, called as they are.  Kernels:
//   hub_wave_stats       mean and 1 / sqrt(var + 1e-7) of a clip in fp64: one block, two passes, a fixed tree.
//   hub_conv0            normalise on load, Conv1d(1, C0, k, stride), LayerNorm(C0), GELU.  VALU; one wave per output row, 64 rows a block.
//   hub_conv_ln_gelu     Conv1d(Cin, Cout, k, stride) as a GEMM whose A rows are contiguous spans of the channel-last input, LayerNorm(Cout)
//                        and GELU on the accumulators.  One block per 32 output rows and all Cout <= 512 columns; wave w owns the 16-column
//                        tiles w, w + 4, ... (up to 8), 2 x 8 tiles of v_mfma_f32_16x16x4_f32, accumulated on two levels: 2 x 64 accumulator registers.
//   hub_pos_conv<NCT>    x + gelu(grouped Conv1d(C, C, k, padding k / 2) + bias): one block per (64 rows, group, batch); the group's
//                        (64 + k - 1) x C/groups slab sits in LDS and is read shifted by the tap, the weights stream from global memory one tap ahead.
#include "r3d_common.h"
#include "../../include/r3d_hip_hubert.h"
#include <math.h>

namespace r3d {
namespace hub {

// ---- clip statistics ------------------------------------------------------------------------------------------------------------------
constexpr int ST_THREADS = 1024;

// the block's sum of v in a fixed order: thread t holds samples t, t + 1024, ... summed in that order; then a binary tree over threads
__device__ __forceinline__ double block_sum(double v, double* sh)
{
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int off = ST_THREADS / 2; off >= 1; off >>= 1) {
        if (t < off) sh[t] += sh[t + off];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

__global__ void __launch_bounds__(ST_THREADS) hub_wave_stats(const float* wave, size_t n, double* stats)
{
    __shared__ double sh[ST_THREADS];
    const int t = threadIdx.x;
    double s = 0.0;
    for (size_t i = t; i < n; i += ST_THREADS) s += (double)wave[i];
    const double mean = block_sum(s, sh) / (double)n;
    double q = 0.0;
    for (size_t i = t; i < n; i += ST_THREADS) { const double d = (double)wave[i] - mean; q += d * d; }
    const double var = block_sum(q, sh) / (double)n;
    if (t == 0) { stats[0] = mean; stats[1] = 1.0 / sqrt(var + 1e-7); }
}

// ---- layer 0 ----------------------------------------------------------------------------------------------------------------------------
constexpr int C0_ROWS = 64, C0_KMAX = 16, C0_CMAX = 512, C0_SMAX = 16;

__global__ void __launch_bounds__(256) hub_conv0(const float* wave, const double* stats, size_t offset, size_t sstride, int n_chunk, int T0,
                                                 const float* w, const float* bias, const float* ln_g, const float* ln_b, float eps, int C0, int k,
                                                 int stride, float* y)
{
    __shared__ float ws[C0_KMAX * C0_CMAX];                        // [tap][channel]
    __shared__ float xs[(C0_ROWS - 1) * C0_SMAX + C0_KMAX];
    const int t = threadIdx.x, lane = t & 63, wave_id = t >> 6;
    const int b = blockIdx.y, t0 = blockIdx.x * C0_ROWS;
    const double mean = stats[0], rstd = stats[1];
    const float* src = wave + offset + (size_t)b * sstride;
    const int first = t0 * stride, need = (C0_ROWS - 1) * stride + k;
    for (int e = t; e < need; e += 256) {
        const int i = first + e;
        xs[e] = i < n_chunk ? (float)(((double)src[i] - mean) * rstd) : 0.0f;
    }
    for (int e = t; e < C0 * k; e += 256) {
        const int c = e / k, j = e - c * k;
        ws[j * C0_CMAX + c] = w[e];
    }
    __syncthreads();
    const float inv = 1.0f / (float)C0;
    for (int i = 0; i < C0_ROWS / 4; ++i) {
        const int row = wave_id * (C0_ROWS / 4) + i, tt = t0 + row;
        if (tt >= T0) break;                                       // wave-uniform
        const float* xr = xs + row * stride;
        float v[C0_CMAX / 64];
        float s = 0.0f;
#pragma unroll
        for (int q = 0; q < C0_CMAX / 64; ++q) {
            const int c = lane + 64 * q;
            float a = 0.0f;
            if (c < C0) {
                a = bias[c];
                for (int j = 0; j < k; ++j) a = fmaf(ws[j * C0_CMAX + c], xr[j], a);
            }
            v[q] = a;
            s += a;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
        const float mu = s * inv;
        float qq = 0.0f;
#pragma unroll
        for (int q = 0; q < C0_CMAX / 64; ++q) {
            const float d = lane + 64 * q < C0 ? v[q] - mu : 0.0f;
            v[q] = d;
            qq += d * d;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) qq += __shfl_xor(qq, off);
        const float rs = 1.0f / sqrtf(qq * inv + eps);
        float* yr = y + ((size_t)b * T0 + tt) * C0;
#pragma unroll
        for (int q = 0; q < C0_CMAX / 64; ++q) {
            const int c = lane + 64 * q;
            if (c < C0) yr[c] = gelu_erf(v[q] * rs * ln_g[c] + ln_b[c]);
        }
    }
}

// ---- layers 1 .. 6 ----------------------------------------------------------------------------------------------------------------------
constexpr int CL_ROWS = 32, CL_KC = 16, CL_LD = CL_KC + 4, CL_NMAX = 512, CL_TILES = CL_NMAX / 64, CL_FLUSH = 8;

// Sum over the block's columns of one value per (row tile, r) and lane: the wave's own tiles are already added; here the 16 lanes that hold
// a row's columns, then the four waves through LDS in the order 0, 1, 2, 3.
__device__ __forceinline__ void cl_row_sums(float (&s)[2][4], float (*part)[CL_ROWS], int wave, int li, int lg)
{
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float v = s[rt][r];
#pragma unroll
            for (int off = 8; off >= 1; off >>= 1) v += __shfl_xor(v, off);
            if (li == 0) part[wave][rt * 16 + lg * 4 + r] = v;
        }
    __syncthreads();
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = rt * 16 + lg * 4 + r;
            s[rt][r] = ((part[0][row] + part[1][row]) + part[2][row]) + part[3][row];
        }
    __syncthreads();
}

// The k index of a 16-float chunk of K: step s of lane group g takes element 4 g + s, for x and for w alike, so an operand is one 16-byte
// LDS read per chunk (the map of i2p_attention).
__global__ void __launch_bounds__(256, 2) hub_conv_ln_gelu(const float* x, const float* w, const float* bias, const float* ln_g, const float* ln_b,
                                                           float eps, int M, int Tin, int Tout, int Cin, int Cout, int K, int stride, float* y)
{
    __shared__ __attribute__((aligned(16))) float As[CL_ROWS * CL_LD];
    __shared__ __attribute__((aligned(16))) float Ws[CL_NMAX * CL_LD];
    __shared__ float part[4][CL_ROWS];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 15, lg = lane >> 4;
    const int m0 = blockIdx.x * CL_ROWS, NT = Cout >> 4;

    // the A row this thread stages (threads 0 .. 127: row t / 4, 16-byte piece t % 4)
    const float* arow = nullptr;
    if (t < CL_ROWS * 4) {
        const int m = m0 + (t >> 2);
        if (m < M) {
            const int b = m / Tout, tt = m - b * Tout;
            arow = x + ((size_t)b * Tin + (size_t)stride * tt) * Cin + (t & 3) * 4;
        }
    }
    // Two levels of accumulation: `part_acc` takes CL_FLUSH chunks (128 of K, 32 MFMA steps) and is then added to `acc`, so no chain of
    // fp32 additions is longer than 32 + K / 128 whatever K is (one chain over K = 1536 was 4.4 times as far from fp64 as fp32 torch).
    f32x4 acc[2][CL_TILES], part_acc[2][CL_TILES];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int i = 0; i < CL_TILES; ++i) acc[rt][i] = part_acc[rt][i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    // The next chunk's operands wait in registers while this chunk's MFMAs run: thread t holds piece t % 4 of the weight rows t / 4 + 64 i
    // (up to 8 of them) and, below 128, of one A row.  Without this every chunk paid its global loads one after the other.
    // (A row past Cout reads row Cout - 1 and is not stored: every register is written on every path.)
    const f32x4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
    const int wr0 = t >> 2, piece = (t & 3) * 4;
    const float* wsrc = w + piece;
    f32x4 wreg[CL_NMAX / 64], areg = zero4;
#pragma unroll
    for (int i = 0; i < CL_NMAX / 64; ++i) wreg[i] = *(const f32x4*)(wsrc + (size_t)min(64 * i + wr0, Cout - 1) * K);
    if (arow) areg = *(const f32x4*)arow;
    for (int k0 = 0, chunk = 0; k0 < K; k0 += CL_KC, ++chunk) {
        __syncthreads();
        if (t < CL_ROWS * 4) *(f32x4*)(As + wr0 * CL_LD + piece) = areg;
#pragma unroll
        for (int i = 0; i < CL_NMAX / 64; ++i)
            if (64 * i + wr0 < Cout) *(f32x4*)(Ws + (64 * i + wr0) * CL_LD + piece) = wreg[i];
        __syncthreads();
        if (k0 + CL_KC < K) {
#pragma unroll
            for (int i = 0; i < CL_NMAX / 64; ++i) wreg[i] = *(const f32x4*)(wsrc + (size_t)min(64 * i + wr0, Cout - 1) * K + k0 + CL_KC);
            if (arow) areg = *(const f32x4*)(arow + k0 + CL_KC);
        }
        const float4 a0 = *(const float4*)(As + li * CL_LD + lg * 4);
        const float4 a1 = *(const float4*)(As + (16 + li) * CL_LD + lg * 4);
#pragma unroll
        for (int i = 0; i < CL_TILES; ++i) {
            const int ct = wave + 4 * i;
            if (ct < NT) {                                         // wave-uniform
                const float4 bw = *(const float4*)(Ws + (ct * 16 + li) * CL_LD + lg * 4);
                part_acc[0][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.x, bw.x, part_acc[0][i], 0, 0, 0);
                part_acc[1][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.x, bw.x, part_acc[1][i], 0, 0, 0);
                part_acc[0][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.y, bw.y, part_acc[0][i], 0, 0, 0);
                part_acc[1][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.y, bw.y, part_acc[1][i], 0, 0, 0);
                part_acc[0][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.z, bw.z, part_acc[0][i], 0, 0, 0);
                part_acc[1][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.z, bw.z, part_acc[1][i], 0, 0, 0);
                part_acc[0][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.w, bw.w, part_acc[0][i], 0, 0, 0);
                part_acc[1][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.w, bw.w, part_acc[1][i], 0, 0, 0);
            }
        }
        if ((chunk & (CL_FLUSH - 1)) == CL_FLUSH - 1 || k0 + CL_KC >= K) {
#pragma unroll
            for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                for (int i = 0; i < CL_TILES; ++i) { acc[rt][i] += part_acc[rt][i]; part_acc[rt][i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f}; }
        }
    }
    // D layout of 16x16x4: column lane & 15, rows 4 (lane >> 4) + r.  Bias, then the two-pass LayerNorm over the block's Cout columns.
    float s[2][4];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) s[rt][r] = 0.0f;
#pragma unroll
    for (int i = 0; i < CL_TILES; ++i) {
        const int ct = wave + 4 * i;
        if (ct < NT) {
            const float bv = bias[ct * 16 + li];
#pragma unroll
            for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                for (int r = 0; r < 4; ++r) { acc[rt][i][r] += bv; s[rt][r] += acc[rt][i][r]; }
        }
    }
    cl_row_sums(s, part, wave, li, lg);
    const float inv = 1.0f / (float)Cout;
    float mu[2][4];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) { mu[rt][r] = s[rt][r] * inv; s[rt][r] = 0.0f; }
#pragma unroll
    for (int i = 0; i < CL_TILES; ++i) {
        if (wave + 4 * i < NT) {
#pragma unroll
            for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                for (int r = 0; r < 4; ++r) { const float d = acc[rt][i][r] - mu[rt][r]; acc[rt][i][r] = d; s[rt][r] += d * d; }
        }
    }
    cl_row_sums(s, part, wave, li, lg);
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) s[rt][r] = 1.0f / sqrtf(s[rt][r] * inv + eps);
#pragma unroll
    for (int i = 0; i < CL_TILES; ++i) {
        const int ct = wave + 4 * i;
        if (ct < NT) {
            const int c = ct * 16 + li;
            const float g = ln_g[c], bt = ln_b[c];
#pragma unroll
            for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int m = m0 + rt * 16 + lg * 4 + r;
                    if (m < M) y[(size_t)m * Cout + c] = gelu_erf(acc[rt][i][r] * s[rt][r] * g + bt);
                }
        }
    }
}

// ---- positional conv ----------------------------------------------------------------------------------------------------------------------
constexpr int PC_ROWS = 64, PC_KMAX = 128, PC_NGMAX = 64, PC_FLUSH = 4;

template <int NCT>          // C / groups = 16 NCT
__global__ void __launch_bounds__(256, 2) hub_pos_conv(const float* x, const float* w, const float* bias, int T, int C, int k, float* y)
{
    constexpr int NG = 16 * NCT, LD = NG + 4;
    __shared__ __attribute__((aligned(16))) float slab[(PC_ROWS + PC_KMAX - 1) * LD];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 15, lg = lane >> 4;
    const int g = blockIdx.y, b = blockIdx.z, t0 = blockIdx.x * PC_ROWS, pad = k >> 1;
    const float* xb = x + (size_t)b * T * C + g * NG;
    const int rows = PC_ROWS + k - 1;
    for (int e = t; e < rows * (NG / 4); e += 256) {
        const int r = e / (NG / 4), piece = e - r * (NG / 4), tt = t0 - pad + r;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (tt >= 0 && tt < T) v = *(const float4*)(xb + (size_t)tt * C + piece * 4);
        *(float4*)(slab + r * LD + piece * 4) = v;
    }
    __syncthreads();
    if (t0 + wave * 16 >= T) return;                               // wave-uniform, after the last barrier
    // two levels of accumulation, as in hub_conv_ln_gelu: PC_FLUSH taps (at most 64 MFMA steps) into part_acc, then one addition
    f32x4 acc[NCT], part_acc[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) acc[ct] = part_acc[ct] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const float* ar = slab + (wave * 16 + li) * LD + lg * 4;
    const float* wr = w + ((size_t)(g * NG + li) * k) * NG + lg * 4;          // + ct 16 k NG + j NG + cc 16
    const size_t wtile = (size_t)16 * k * NG;
    // A tap's NCT x NCT weight pieces are loaded one tap ahead, into the register set the tap before last used
    auto fetch = [&](float4 (&wt)[NCT][NCT], int j) {
#pragma unroll
        for (int cc = 0; cc < NCT; ++cc)
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) wt[cc][ct] = *(const float4*)(wr + ct * wtile + (size_t)j * NG + cc * 16);
    };
    auto tap = [&](const float4 (&wt)[NCT][NCT], int j) {
#pragma unroll
        for (int cc = 0; cc < NCT; ++cc) {
            const float4 a = *(const float4*)(ar + j * LD + cc * 16);
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                const float4 bw = wt[cc][ct];
                part_acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, bw.x, part_acc[ct], 0, 0, 0);
                part_acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, bw.y, part_acc[ct], 0, 0, 0);
                part_acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, bw.z, part_acc[ct], 0, 0, 0);
                part_acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, bw.w, part_acc[ct], 0, 0, 0);
            }
        }
        if ((j & (PC_FLUSH - 1)) == PC_FLUSH - 1 || j == k - 1) {
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) { acc[ct] += part_acc[ct]; part_acc[ct] = f32x4{0.0f, 0.0f, 0.0f, 0.0f}; }
        }
    };
    float4 w0[NCT][NCT], w1[NCT][NCT];
    fetch(w0, 0);
    for (int j = 0; j < k; j += 2) {
        if (j + 1 < k) fetch(w1, j + 1);
        tap(w0, j);
        if (j + 1 < k) {
            if (j + 2 < k) fetch(w0, j + 2);
            tap(w1, j + 1);
        }
    }
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
        const int c = g * NG + ct * 16 + li;
        const float bv = bias[c];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int tt = t0 + wave * 16 + lg * 4 + r;
            if (tt < T) {
                const size_t o = ((size_t)b * T + tt) * C + c;
                y[o] = x[o] + gelu_erf(acc[ct][r] + bv);
            }
        }
    }
}

static inline bool finite_nonneg(float v) { return v >= 0.0f && v <= 3.402823466e38f; }

}  // namespace hub
}  // namespace r3d

using namespace r3d;
using namespace r3d::hub;

extern "C" int r3d_hubert_wave_stats(const float* wave, size_t n, double* stats, r3d_stream_t stream)
{
    if (!wave || !stats) { set_error("hubert_wave_stats: NULL pointer"); return R3D_ERR_INVALID_ARG; }
    if (n == 0) { set_error("hubert_wave_stats: bad argument (n > 0)"); return R3D_ERR_INVALID_ARG; }
    if (!below_2_31("hubert_wave_stats", "n", (double)n, "elements")) return R3D_ERR_INVALID_ARG;
    if (!aligned(stats, 8)) { set_error("hubert_wave_stats: stats must be 8-byte aligned"); return R3D_ERR_INVALID_ARG; }
    const Span spans[] = {writes(stats, 2), reads(wave, n)};
    if (clash(spans)) { set_error("hubert_wave_stats: stats overlaps wave"); return R3D_ERR_INVALID_ARG; }
    hipLaunchKernelGGL(hub_wave_stats, dim3(1), dim3(ST_THREADS), 0, (hipStream_t)stream, wave, n, stats);
    return check_launch("hubert_wave_stats");
}

extern "C" int r3d_hubert_conv0(const float* wave, const double* stats, int B, size_t sample_offset, size_t sample_stride, int n_chunk,
                                const float* w, const float* bias, const float* ln_g, const float* ln_b, float eps, int C0, int k, int stride,
                                float* y, r3d_stream_t stream)
{
    if (!wave || !stats || !w || !bias || !ln_g || !ln_b || !y) { set_error("hubert_conv0: NULL pointer"); return R3D_ERR_INVALID_ARG; }
    if (B <= 0 || B > 65535 || n_chunk <= 0 || stride <= 0 || k <= 0 || C0 <= 0)
        { set_error("hubert_conv0: bad argument (B, n_chunk, C0, k, stride > 0; B <= 65535)"); return R3D_ERR_INVALID_ARG; }
    if (k > C0_KMAX || stride > C0_SMAX || C0 % 16 || C0 > C0_CMAX)
        { set_error("hubert_conv0: outside the range k <= 16, stride <= 16, C0 a multiple of 16 up to 512 (k %d, stride %d, C0 %d)", k, stride, C0);
          return R3D_ERR_INVALID_ARG; }
    if (n_chunk < k) { set_error("hubert_conv0: n_chunk = %d is shorter than the kernel k = %d", n_chunk, k); return R3D_ERR_INVALID_ARG; }
    if (!finite_nonneg(eps)) { set_error("hubert_conv0: eps is negative or not finite"); return R3D_ERR_INVALID_ARG; }
    const int T0 = (n_chunk - k) / stride + 1;
    const double extent = (double)sample_offset + (double)(B - 1) * (double)sample_stride + n_chunk;
    if (!below_2_31("hubert_conv0", "sample_offset + (B - 1) sample_stride + n_chunk", extent, "samples") ||
        !below_2_31("hubert_conv0", "B T0 C0", (double)B * T0 * C0, "elements")) return R3D_ERR_INVALID_ARG;
    if (!aligned(stats, 8)) { set_error("hubert_conv0: stats must be 8-byte aligned"); return R3D_ERR_INVALID_ARG; }
    const Span spans[] = {writes(y, (size_t)B * T0 * C0), reads(wave + sample_offset, (size_t)(B - 1) * sample_stride + n_chunk), reads(stats, 2),
                          reads(w, (size_t)C0 * k), reads(bias, C0), reads(ln_g, C0), reads(ln_b, C0)};
    if (clash(spans)) { set_error("hubert_conv0: y overlaps an input"); return R3D_ERR_INVALID_ARG; }
    hipLaunchKernelGGL(hub_conv0, dim3((T0 + C0_ROWS - 1) / C0_ROWS, B), dim3(256), 0, (hipStream_t)stream, wave, stats, sample_offset, sample_stride,
                       n_chunk, T0, w, bias, ln_g, ln_b, eps, C0, k, stride, y);
    return check_launch("hubert_conv0");
}

extern "C" int r3d_hubert_conv_ln_gelu(const float* x, const float* w, const float* bias, const float* ln_g, const float* ln_b, float eps, int B,
                                       int Tin, int Cin, int Cout, int k, int stride, float* y, r3d_stream_t stream)
{
    if (!x || !w || !bias || !ln_g || !ln_b || !y) { set_error("hubert_conv_ln_gelu: NULL pointer"); return R3D_ERR_INVALID_ARG; }
    if (B <= 0 || Tin <= 0 || Cin <= 0 || Cout <= 0 || k <= 0 || stride <= 0)
        { set_error("hubert_conv_ln_gelu: bad argument (B, Tin, Cin, Cout, k, stride > 0)"); return R3D_ERR_INVALID_ARG; }
    if (k > 4 || Cin % 16 || Cout % 16 || Cin > CL_NMAX || Cout > CL_NMAX)
        { set_error("hubert_conv_ln_gelu: outside the range k <= 4, Cin and Cout multiples of 16 up to 512 (k %d, Cin %d, Cout %d)", k, Cin, Cout);
          return R3D_ERR_INVALID_ARG; }
    if (Tin < k) { set_error("hubert_conv_ln_gelu: Tin = %d is shorter than the kernel k = %d", Tin, k); return R3D_ERR_INVALID_ARG; }
    if (!finite_nonneg(eps)) { set_error("hubert_conv_ln_gelu: eps is negative or not finite"); return R3D_ERR_INVALID_ARG; }
    const int Tout = (Tin - k) / stride + 1;
    if (!below_2_31("hubert_conv_ln_gelu", "B Tin Cin", (double)B * Tin * Cin, "elements") ||
        !below_2_31("hubert_conv_ln_gelu", "B Tout Cout", (double)B * Tout * Cout, "elements")) return R3D_ERR_INVALID_ARG;
    if (!aligned16(x) || !aligned16(w)) { set_error("hubert_conv_ln_gelu: x and w must be 16-byte aligned"); return R3D_ERR_INVALID_ARG; }
    const Span spans[] = {writes(y, (size_t)B * Tout * Cout), reads(x, (size_t)B * Tin * Cin), reads(w, (size_t)Cout * k * Cin), reads(bias, Cout),
                          reads(ln_g, Cout), reads(ln_b, Cout)};
    if (clash(spans)) { set_error("hubert_conv_ln_gelu: y overlaps an input"); return R3D_ERR_INVALID_ARG; }
    const int M = B * Tout;
    hipLaunchKernelGGL(hub_conv_ln_gelu, dim3((M + CL_ROWS - 1) / CL_ROWS), dim3(256), 0, (hipStream_t)stream, x, w, bias, ln_g, ln_b, eps, M, Tin,
                       Tout, Cin, Cout, k * Cin, stride, y);
    return check_launch("hubert_conv_ln_gelu");
}

extern "C" int r3d_hubert_pos_conv(const float* x, const float* w, const float* bias, int B, int T, int C, int k, int groups, float* y,
                                   r3d_stream_t stream)
{
    if (!x || !w || !bias || !y) { set_error("hubert_pos_conv: NULL pointer"); return R3D_ERR_INVALID_ARG; }
    if (B <= 0 || B > 65535 || T <= 0 || C <= 0 || k <= 0 || groups <= 0 || groups > 65535)
        { set_error("hubert_pos_conv: bad argument (B, T, C, k, groups > 0; B, groups <= 65535)"); return R3D_ERR_INVALID_ARG; }
    const int Ng = C / groups;
    if (k > PC_KMAX || C % groups || Ng % 16 || Ng > PC_NGMAX)
        { set_error("hubert_pos_conv: outside the range k <= 128, C / groups a multiple of 16 up to 64 (k %d, C %d, groups %d)", k, C, groups);
          return R3D_ERR_INVALID_ARG; }
    if (!below_2_31("hubert_pos_conv", "B T C", (double)B * T * C, "elements") ||
        !below_2_31("hubert_pos_conv", "C k C / groups", (double)C * k * Ng, "elements")) return R3D_ERR_INVALID_ARG;
    if (!aligned16(x) || !aligned16(w)) { set_error("hubert_pos_conv: x and w must be 16-byte aligned"); return R3D_ERR_INVALID_ARG; }
    const size_t n = (size_t)B * T * C;
    const Span spans[] = {writes(y, n), reads(x, n), reads(w, (size_t)C * k * Ng), reads(bias, C)};
    if (clash(spans)) { set_error("hubert_pos_conv: y overlaps an input"); return R3D_ERR_INVALID_ARG; }
    const dim3 grid((T + PC_ROWS - 1) / PC_ROWS, groups, B);
    hipStream_t st = (hipStream_t)stream;
    switch (Ng / 16) {
    case 1: hipLaunchKernelGGL(hub_pos_conv<1>, grid, dim3(256), 0, st, x, w, bias, T, C, k, y); break;
    case 2: hipLaunchKernelGGL(hub_pos_conv<2>, grid, dim3(256), 0, st, x, w, bias, T, C, k, y); break;
    case 3: hipLaunchKernelGGL(hub_pos_conv<3>, grid, dim3(256), 0, st, x, w, bias, T, C, k, y); break;
    default: hipLaunchKernelGGL(hub_pos_conv<4>, grid, dim3(256), 0, st, x, w, bias, T, C, k, y); break;
    }
    return check_launch("hubert_pos_conv");
}
