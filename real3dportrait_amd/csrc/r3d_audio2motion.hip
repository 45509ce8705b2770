// The audio-to-motion VAE's inference path (include/r3d_hip_audio.h): Conv1d as a GEMM over taps with the model's glue in
// its loads and its epilogue, one WN layer per launch with the gated activations in LDS, and the pitch quantisation + embedding lookup.
// Every product runs on the f32 MFMA (16 x 16 x 4: A[m = lane & 15][k = lane >> 4], B[k = lane >> 4][n = lane & 15], D rows
// 4 (lane >> 4) + r, column lane & 15), so the sums are exact-fp32 products accumulated in fp32 in a fixed order.
#include <math.h>

#include "r3d_common.h"

namespace r3d {
namespace a2m {

// ---- conv1d: a block of 4 waves owns a 32-row x 32-column tile of one sample's output, a wave one 16 x 16 MFMA tile; K = k Cin is walked
// in chunks of 32 through LDS (k-major, rows padded to 33 floats).  The problems are a few hundred rows: the tile is small so that
// T = 250 still fills a few dozen CUs.
constexpr int CONV_THREADS = 256, BM = 32, BN = 32, BK = 32, LDT = BM + 1;

struct ConvArgs {
    const float* x; int Tin, Cin, x_stride, x_offset, row_mode;
    const float* w; const float* bias; int Cout, k, stride, pad, Tout;
    int gelu; const float* mask; const float* table; const int64_t* idx; int table_rows, idx_step;
    const float* amp0; const float* u0; const float* amp1; const float* u1;
    const float* other; float* y; int y_stride, y_offset, flip;
};

__global__ __launch_bounds__(CONV_THREADS) void conv1d_kernel(ConvArgs a)
{
    __shared__ float As[BK * LDT], Ws[BK * LDT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave & 1) * 16, wn = (wave >> 1) * 16;
    const int t0 = blockIdx.x * BM, n0 = blockIdx.y * BN, b = blockIdx.z;
    const int K = a.k * a.Cin, Tsrc = a.row_mode ? 2 * a.Tin : a.Tin;
    const float* xb = a.x + (size_t)b * Tsrc * a.x_stride + a.x_offset;
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int k0 = 0; k0 < K; k0 += BK) {
        for (int e = tid; e < BM * BK; e += CONV_THREADS) {
            const int kk = e & (BK - 1), m = e / BK, kg = k0 + kk;          // m: the tile's row for As, its column for Ws
            float av = 0.0f, wv = 0.0f;
            if (kg < K) {
                const int j = kg / a.Cin, ci = kg - j * a.Cin;
                const int t = t0 + m, tin = t * a.stride - a.pad + j;
                if (t < a.Tout && tin >= 0 && tin < a.Tin) {                 // zero padding, per sample
                    if (a.row_mode == 0) av = xb[(size_t)tin * a.x_stride + ci];
                    else if (a.row_mode == 1) av = xb[(size_t)(2 * tin) * a.x_stride + ci];
                    else av = 0.5f * (xb[(size_t)(2 * tin) * a.x_stride + ci] + xb[(size_t)(2 * tin + 1) * a.x_stride + ci]);
                }
                if (n0 + m < a.Cout) wv = a.w[(size_t)(n0 + m) * K + kg];
            }
            As[kk * LDT + m] = av;
            Ws[kk * LDT + m] = wv;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < BK; kk += 4) {
            const int k = kk + (lane >> 4);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(As[k * LDT + wm + (lane & 15)], Ws[k * LDT + wn + (lane & 15)], acc, 0, 0, 0);
        }
        __syncthreads();
    }
    const int n = n0 + wn + (lane & 15);
    if (n >= a.Cout) return;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int t = t0 + wm + (lane >> 4) * 4 + r;
        if (t >= a.Tout) continue;
        float v = acc[r];
        if (a.bias) v += a.bias[n];
        if (a.table) {
            long long id = a.idx[((size_t)b * a.Tout + t) * a.idx_step];
            id = id < 0 ? 0 : (id >= a.table_rows ? a.table_rows - 1 : id);
            v += a.table[(size_t)id * a.Cout + n];
        }
        if (a.amp0) v += a.amp0[b] * a.u0[n];
        if (a.amp1) v += a.amp1[b] * a.u1[n];
        if (a.gelu) v = 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f));
        if (a.mask) v *= a.mask[(size_t)b * a.Tout + t];
        int c = a.y_offset + n;
        if (a.flip) c = a.y_stride - 1 - c;
        const size_t i = ((size_t)b * a.Tout + t) * a.y_stride + c;
        if (a.other) v = a.other[i] - v;
        a.y[i] = v;
    }
}

// ---- one WN layer: a block of 4 waves owns WN_ROWS rows of one sample.  x with its halo and g are staged in LDS once; wave w owns the
// channels [w H / 4, (w + 1) H / 4) of BOTH halves of each GEMM's output, so tanh(a) sigmoid(b) and the res / skip split are
// register-local; the weights ([K, N], N contiguous) go from L2 to the MFMA's B operand directly: a block uses each element once.
// 16 rows: the layers are latency-bound at T = 63 .. 250 (4 .. 16 blocks a sample) and a larger tile would leave fewer blocks still.
constexpr int WN_ROWS = R3D_A2M_WN_ROWS, WN_THREADS = 256, WN_MAX_CG = 256;

struct WnArgs {
    const float* x; const float* g; int T, Cg, k;
    const float* w_in; const float* b_in; const float* w_rs; const float* b_rs; const float* mask;
    int first, last; float* x_next; float* out;
};

static size_t wn_lds_bytes(int H, int Cg, int k) { return sizeof(float) * ((size_t)(WN_ROWS + k - 1) * (H + 4) + (size_t)WN_ROWS * (Cg + 4) + (size_t)WN_ROWS * (H + 4)); }

template <int H>
__global__ __launch_bounds__(WN_THREADS) void wn_layer_kernel(WnArgs a)
{
    extern __shared__ float smem[];
    constexpr int NT = H / 64, LDX = H + 4, N2 = 2 * H;          // NT: 16-column tiles a wave owns in each half
    const int LDG = a.Cg + 4, pad = a.k / 2, rows = WN_ROWS + a.k - 1;
    float* xs = smem;                    // [rows][LDX]: x rows t0 - pad .. t0 + WN_ROWS - 1 + pad, zero outside the sample
    float* gs = xs + rows * LDX;         // [WN_ROWS][LDG]
    float* acts = gs + WN_ROWS * LDG;    // [WN_ROWS][LDX]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
    const int t0 = blockIdx.x * WN_ROWS, b = blockIdx.y, T = a.T;
    const float* xb = a.x + (size_t)b * T * H;
    const float* gb = a.g + (size_t)b * T * a.Cg;
    for (int e = tid; e < rows * H; e += WN_THREADS) {
        const int r = e / H, c = e - r * H, t = t0 - pad + r;
        xs[r * LDX + c] = t >= 0 && t < T ? xb[(size_t)t * H + c] : 0.0f;
    }
    for (int e = tid; e < WN_ROWS * a.Cg; e += WN_THREADS) {
        const int r = e / a.Cg, c = e - r * a.Cg, t = t0 + r;
        gs[r * LDG + c] = t < T ? gb[(size_t)t * a.Cg + c] : 0.0f;
    }
    __syncthreads();

    const int cw = wave * (H / 4) + li;          // this lane's column in the wave's first tile
    f32x4 at[NT], as[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) at[i] = as[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int j = 0; j < a.k; ++j) {
        const float* xr = xs + (li + j) * LDX + lg;
        const float* wr = a.w_in + (size_t)(j * H + lg) * N2 + cw;
#pragma unroll 4
        for (int c = 0; c < H; c += 4) {
            const float av = xr[c];
            const float* wc = wr + (size_t)c * N2;
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                at[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wc[i * 16], at[i], 0, 0, 0);
                as[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wc[H + i * 16], as[i], 0, 0, 0);
            }
        }
    }
    {
        const float* gr = gs + li * LDG + lg;
        const float* wr = a.w_in + (size_t)(a.k * H + lg) * N2 + cw;
        for (int c = 0; c < a.Cg; c += 4) {
            const float av = gr[c];
            const float* wc = wr + (size_t)c * N2;
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                at[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wc[i * 16], at[i], 0, 0, 0);
                as[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wc[H + i * 16], as[i], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int col = cw + i * 16;
        const float bt = a.b_in[col], bs = a.b_in[H + col];
#pragma unroll
        for (int r = 0; r < 4; ++r)
            acts[(lg * 4 + r) * LDX + col] = tanhf(at[i][r] + bt) * (1.0f / (1.0f + expf(-(as[i][r] + bs))));
    }
    __syncthreads();

    const int Crs = a.last ? H : N2;
    f32x4 r0[NT], r1[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) r0[i] = r1[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    {
        const float* ar = acts + li * LDX + lg;
        const float* wr = a.w_rs + (size_t)lg * Crs + cw;
#pragma unroll 4
        for (int c = 0; c < H; c += 4) {
            const float av = ar[c];
            const float* wc = wr + (size_t)c * Crs;
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                r0[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wc[i * 16], r0[i], 0, 0, 0);
                if (!a.last) r1[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wc[H + i * 16], r1[i], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int col = cw + i * 16;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = lg * 4 + r, t = t0 + row;
            if (t >= T) continue;
            const size_t o = ((size_t)b * T + t) * H + col;
            const float m = a.mask ? a.mask[(size_t)b * T + t] : 1.0f;
            if (!a.last) {
                a.x_next[o] = (xs[(row + pad) * LDX + col] + (r0[i][r] + a.b_rs[col])) * m;
                const float s = r1[i][r] + a.b_rs[H + col];
                a.out[o] = a.first ? s : a.out[o] + s;
            } else {
                const float s = r0[i][r] + a.b_rs[col];
                a.out[o] = (a.first ? s : a.out[o] + s) * m;
            }
        }
    }
}

// ---- f0_to_coarse + the embedding lookup: one wave per output row
constexpr int PITCH_THREADS = 64;

// mel_min = 1127 log(1 + 50 / 700) and span = 1127 log(1 + 1100 / 700) - mel_min: fp64 on the host, rounded to fp32 as torch rounds a scalar operand
__device__ __forceinline__ int f0_to_coarse(float f0, float mel_min, float span)
{
#pragma clang fp contract(off)          // the reference rounds after every operation
    float m = 1127.0f * logf(1.0f + f0 / 700.0f);
    if (m > 0.0f) m = (m - mel_min) * 254.0f / span + 1.0f;
    m = m <= 1.0f ? 1.0f : m;
    m = m > 255.0f ? 255.0f : m;
    return (int)(m + 0.5f);
}

__global__ __launch_bounds__(PITCH_THREADS) void pitch_embed_kernel(const float* f0, float mel_min, float span, const float* table, int rows, int C,
                                                                     int32_t* index, float* y)
{
    const size_t row = blockIdx.x;                          // b T + t; f0 [B, 2 T] is read at b 2 T + 2 t = 2 row
    int id = f0_to_coarse(f0[2 * row], mel_min, span);
    if (threadIdx.x == 0) index[row] = id;
    id = id < 0 ? 0 : (id >= rows ? rows - 1 : id);         // (a NaN pitch: the reference's assert fires; here row 0)
    for (int c = threadIdx.x; c < C; c += PITCH_THREADS) y[row * C + c] = table[(size_t)id * C + c];
}

}  // namespace a2m
}  // namespace r3d

using namespace r3d;

extern "C" int r3d_a2m_conv1d(const float* x, int B, int Tin, int Cin, int x_stride, int x_offset, int row_mode, const float* w,
                              const float* bias, int Cout, int k, int stride, int pad, int gelu, const float* mask, const float* table,
                              const int64_t* idx, int table_rows, int idx_step, const float* amp0, const float* u0, const float* amp1, const float* u1,
                              const float* subtract_from, float* y, int y_stride, int y_offset, int flip_out, r3d_stream_t stream)
{
    const char* what = "a2m_conv1d";
    if (!x || !w || !y) { set_error("%s: NULL pointer", what); return R3D_ERR_INVALID_ARG; }
    if (!table != !idx) { set_error("%s: NULL pointer (table and idx go together)", what); return R3D_ERR_INVALID_ARG; }
    if (!amp0 != !u0 || !amp1 != !u1) { set_error("%s: NULL pointer (amp and u go together)", what); return R3D_ERR_INVALID_ARG; }
    if (B < 1 || Tin < 1 || Cin < 1 || Cout < 1) { set_error("%s: B = %d, Tin = %d, Cin = %d, Cout = %d must be positive", what, B, Tin, Cin, Cout); return R3D_ERR_INVALID_ARG; }
    if (B > 65535) { set_error("%s: B = %d exceeds 65535", what, B); return R3D_ERR_INVALID_ARG; }
    if (k < 1 || k > 8) { set_error("%s: k = %d outside 1 .. 8", what, k); return R3D_ERR_INVALID_ARG; }
    if (stride < 1) { set_error("%s: stride = %d must be positive", what, stride); return R3D_ERR_INVALID_ARG; }
    if (pad < 0 || pad >= k) { set_error("%s: pad = %d outside 0 .. k - 1 = %d", what, pad, k - 1); return R3D_ERR_INVALID_ARG; }
    if (row_mode < 0 || row_mode > 2) { set_error("%s: row_mode = %d outside 0 .. 2", what, row_mode); return R3D_ERR_INVALID_ARG; }
    if ((long long)Tin + 2 * pad < k) { set_error("%s: Tin = %d with pad = %d is shorter than k = %d", what, Tin, pad, k); return R3D_ERR_INVALID_ARG; }
    if (x_offset < 0 || x_stride < 1 || (long long)x_offset + Cin > x_stride) { set_error("%s: columns x_offset = %d .. + Cin = %d lie outside a row of x_stride = %d", what, x_offset, Cin, x_stride); return R3D_ERR_INVALID_ARG; }
    if (y_offset < 0 || y_stride < 1 || (long long)y_offset + Cout > y_stride) { set_error("%s: columns y_offset = %d .. + Cout = %d lie outside a row of y_stride = %d", what, y_offset, Cout, y_stride); return R3D_ERR_INVALID_ARG; }
    if (table && table_rows < 1) { set_error("%s: table_rows = %d must be positive", what, table_rows); return R3D_ERR_INVALID_ARG; }
    if (table && idx_step != 1 && idx_step != 2) { set_error("%s: idx_step = %d is not 1 or 2", what, idx_step); return R3D_ERR_INVALID_ARG; }
    const int Tout = (int)(((long long)Tin + 2 * pad - k) / stride + 1), Tsrc_f = row_mode ? 2 : 1;
    if (!below_2_31(what, "B Tsrc x_stride", (double)B * Tin * Tsrc_f * x_stride, "elements")) return R3D_ERR_INVALID_ARG;
    if (!below_2_31(what, "B Tout y_stride", (double)B * Tout * y_stride, "elements")) return R3D_ERR_INVALID_ARG;
    if (!below_2_31(what, "Cout k Cin", (double)Cout * k * Cin, "elements")) return R3D_ERR_INVALID_ARG;
    if (table && !below_2_31(what, "table_rows Cout", (double)table_rows * Cout, "elements")) return R3D_ERR_INVALID_ARG;
    if (!below_2_31(what, "Tin stride", (double)Tin * stride + 8.0, "rows")) return R3D_ERR_INVALID_ARG;
    const size_t ny = (size_t)B * Tout * y_stride;
    const Span spans[] = {writes(y, ny), reads(x, (size_t)B * Tin * Tsrc_f * x_stride), reads(w, (size_t)Cout * k * Cin), reads(bias, (size_t)Cout),
                          reads(mask, (size_t)B * Tout), reads(table, (size_t)(table ? table_rows : 0) * Cout), reads(idx, (size_t)B * Tout * (table ? idx_step : 0)),
                          reads(amp0, (size_t)B), reads(u0, (size_t)Cout), reads(amp1, (size_t)B), reads(u1, (size_t)Cout),
                          reads(subtract_from == y ? nullptr : subtract_from, ny)};
    if (clash(spans)) { set_error("%s: the output overlaps an input (subtract_from may be y itself, nothing else may)", what); return R3D_ERR_INVALID_ARG; }
    a2m::ConvArgs a = {x, Tin, Cin, x_stride, x_offset, row_mode, w, bias, Cout, k, stride, pad, Tout, gelu, mask, table, idx, table_rows, idx_step,
                       amp0, u0, amp1, u1, subtract_from, y, y_stride, y_offset, flip_out};
    ProfScope ps(R3D_PROF_MISC, (hipStream_t)stream);
    const dim3 grid((unsigned)((Tout + a2m::BM - 1) / a2m::BM), (unsigned)((Cout + a2m::BN - 1) / a2m::BN), (unsigned)B);
    hipLaunchKernelGGL(a2m::conv1d_kernel, grid, dim3(a2m::CONV_THREADS), 0, (hipStream_t)stream, a);
    return check_launch(what);
}

extern "C" int r3d_a2m_wn_layer(const float* x, const float* g, int B, int T, int H, int Cg, int k, const float* w_in, const float* b_in,
                                const float* w_rs, const float* b_rs, const float* mask, int first, int last, float* x_next, float* out,
                                r3d_stream_t stream)
{
    const char* what = "a2m_wn_layer";
    if (!x || !g || !w_in || !b_in || !w_rs || !b_rs || !out) { set_error("%s: NULL pointer", what); return R3D_ERR_INVALID_ARG; }
    if (!last && !x_next) { set_error("%s: NULL pointer (x_next is written by every layer but the last)", what); return R3D_ERR_INVALID_ARG; }
    if (last && x_next) { set_error("%s: the last layer writes no x_next", what); return R3D_ERR_INVALID_ARG; }
    if (B < 1 || T < 1) { set_error("%s: B = %d, T = %d must be positive", what, B, T); return R3D_ERR_INVALID_ARG; }
    if (B > 65535) { set_error("%s: B = %d exceeds 65535", what, B); return R3D_ERR_INVALID_ARG; }
    if (H != 64 && H != 256) { set_error("%s: H = %d is not supported (64 or 256)", what, H); return R3D_ERR_INVALID_ARG; }
    if (k != 1 && k != 3 && k != 5) { set_error("%s: k = %d is not supported (1, 3 or 5)", what, k); return R3D_ERR_INVALID_ARG; }
    if (Cg < 4 || Cg > a2m::WN_MAX_CG || Cg % 4) { set_error("%s: Cg = %d must be a multiple of 4 in 4 .. %d", what, Cg, a2m::WN_MAX_CG); return R3D_ERR_INVALID_ARG; }
    if (!below_2_31(what, "B T max(H, Cg)", (double)B * T * (H > Cg ? H : Cg), "elements")) return R3D_ERR_INVALID_ARG;
    const size_t nx = (size_t)B * T * H, Crs = last ? H : 2 * H;
    const Span spans[] = {writes(out, nx), writes(x_next, nx), reads(x, nx), reads(g, (size_t)B * T * Cg), reads(w_in, (size_t)(k * H + Cg) * 2 * H),
                          reads(b_in, (size_t)2 * H), reads(w_rs, (size_t)H * Crs), reads(b_rs, Crs), reads(mask, (size_t)B * T)};
    if (clash(spans)) { set_error("%s: an output overlaps an input or the other output (x_next is another buffer than x: tiles read the halo)", what); return R3D_ERR_INVALID_ARG; }
    a2m::WnArgs a = {x, g, T, Cg, k, w_in, b_in, w_rs, b_rs, mask, first, last, x_next, out};
    ProfScope ps(R3D_PROF_MISC, (hipStream_t)stream);
    const dim3 grid((unsigned)((T + a2m::WN_ROWS - 1) / a2m::WN_ROWS), (unsigned)B);
    const size_t lds = a2m::wn_lds_bytes(H, Cg, k);
    if (H == 64) hipLaunchKernelGGL(a2m::wn_layer_kernel<64>, grid, dim3(a2m::WN_THREADS), lds, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(a2m::wn_layer_kernel<256>, grid, dim3(a2m::WN_THREADS), lds, (hipStream_t)stream, a);
    return check_launch(what);
}

extern "C" int r3d_a2m_pitch_embed(const float* f0, int B, int T, const float* table, int rows, int C, int32_t* index, float* y,
                                   r3d_stream_t stream)
{
    const char* what = "a2m_pitch_embed";
    if (!f0 || !table || !index || !y) { set_error("%s: NULL pointer", what); return R3D_ERR_INVALID_ARG; }
    if (B < 1 || T < 1 || rows < 1 || C < 1) { set_error("%s: B = %d, T = %d, rows = %d, C = %d must be positive", what, B, T, rows, C); return R3D_ERR_INVALID_ARG; }
    if (!below_2_31(what, "B T max(C, 2)", (double)B * T * (C > 2 ? C : 2), "elements")) return R3D_ERR_INVALID_ARG;
    if (!below_2_31(what, "rows C", (double)rows * C, "elements")) return R3D_ERR_INVALID_ARG;
    const size_t n = (size_t)B * T;
    const Span spans[] = {writes(y, n * C), writes(index, n), reads(f0, 2 * n), reads(table, (size_t)rows * C)};
    if (clash(spans)) { set_error("%s: an output overlaps an input or the other output", what); return R3D_ERR_INVALID_ARG; }
    ProfScope ps(R3D_PROF_MISC, (hipStream_t)stream);
    const double mel_min = 1127.0 * log(1.0 + 50.0 / 700.0), mel_max = 1127.0 * log(1.0 + 1100.0 / 700.0);
    hipLaunchKernelGGL(a2m::pitch_embed_kernel, dim3((unsigned)n), dim3(a2m::PITCH_THREADS), 0, (hipStream_t)stream, f0, (float)mel_min,
                       (float)(mel_max - mel_min), table, rows, C, index, y);
    return check_launch(what);
}
