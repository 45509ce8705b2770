// Landmark-driven 3DMM fit (include/r3d_hip_fit.h): the Adam loops of fit_3dmm_for_a_image / fit_3dmm_for_a_video
// (data_gen/utils/process_image/fit_3dmm_landmark.py:85-264, process_video/fit_3dmm_landmark.py:130-459), fp32 as the reference, two
// kernels per iteration and no others.
//   fit_grad   grid (slabs, frame runs).  A block owns V whole key points = 3 V rows of both key bases, copied once into LDS transposed
//              ([k][row], odd stride: a row walk and a column walk are both free of bank conflicts), and walks its frames.  Per frame:
//              A the frame's coefficients to LDS; B shape rows as partial fma chains over a split of k (row r, part j: a fixed order);
//              C one thread per point: shape, q = M shape + trans, projection, residual, d loss / d q, d loss / d shape = M^T dq, and the
//              point's share of the euler (dM / d angle), trans and loss sums; D thread k sums base[., k] x d shape over the slab's rows
//              (the slab's B^T d shape), seven more threads sum the point shares.  Everything a block writes goes to its own
//              workspace row [slab, t, Ki + Ke + 7]: no atomics.  The blocks of slab 0 also copy their frames' parameters to the
//              snapshot, which fit_step reads: fit_step's Laplacian terms need a frame's neighbours while other blocks overwrite them.
//   fit_step   one thread per parameter (a wave per column for a shared id row, whose gradient sums over T): the sum of the partials in
//              a fixed order, the mean-square and Laplacian gradients from the snapshot, Adam's update or (grad entry point) the
//              gradient itself.  Its last block reduces the loss record.
// Iterations are separated by launch boundaries alone; nothing waits for another block.
#include "r3d_common.h"

#include <algorithm>
#include <cmath>

namespace r3d {
namespace fit {

constexpr int THREADS = 256;
constexpr int TILE_FLOATS = 12800;             // the base tile; with the small buffers under 64 KiB
constexpr int MAX_V = 85;                      // 3 V <= THREADS - 1: a thread per row, and an odd stride within THREADS
constexpr int POSE = 39;                       // M, dM/dx, dM/dy, dM/dz (9 each) and trans (3) per frame
constexpr int PG = 16;                         // frames whose poses are computed together
constexpr int SHARES = 7;                      // euler 3, trans 3, loss 1
constexpr int LOSS = R3D_FIT_LOSS_WORDS;

struct GradArgs {
    const float* mean;                    // [3 L]
    const float* id_base;                 // [3 L, Ki]
    const float* exp_base;                // [3 L, Ke] or NULL with Ke = 0
    const float* lms;                     // [T, L, 2]
    const float* weights;                 // [L]
    const float* id;                      // [id_rows, Ki]
    const float* exp;                     // [T, Ke] or NULL with Ke = 0
    const float* euler;                   // [T, 3]
    const float* trans;                   // [T, 3]
    float* snap;                          // the parameters' copy, laid out as the state's first part, or NULL
    float* ws;                            // [slabs, T, Ki + Ke + 7]
    int L, Ki, Ke, T, id_rows, V, chunk;  // V points per block, chunk frames per blockIdx.y
    int need_idexp;                       // phase D's base columns are wanted
    float camera_distance, focal, center, scale;          // scale = 1 / (T L)
};

// rows x K floats from src (contiguous) to dst[k * stride + row]
__device__ __forceinline__ void stage(const float* __restrict__ src, float* dst, int rows, int K, int stride)
{
    const int n = rows * K;
    int r = (int)threadIdx.x / K, k = (int)threadIdx.x - r * K;
    const int dr = THREADS / K, dk = THREADS - dr * K;
    for (int i = threadIdx.x; i < n; i += THREADS) {
        dst[(size_t)k * stride + r] = src[i];
        r += dr; k += dk;
        if (k >= K) { k -= K; ++r; }
    }
}

__device__ __forceinline__ void mm3(const float* a, const float* b, float* o)
{
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) o[3 * i + j] = fmaf(a[3 * i + 2], b[6 + j], fmaf(a[3 * i + 1], b[3 + j], a[3 * i] * b[j]));
}

// M = Rz Ry Rx of compute_rotation (bfm.py:204-238) with its three derivatives, row-major, and the translation
__device__ void pose(const GradArgs& a, int t, float* o)
{
    const float ex = a.euler[(size_t)t * 3], ey = a.euler[(size_t)t * 3 + 1], ez = a.euler[(size_t)t * 3 + 2];
    const float sx = sinf(ex), cx = cosf(ex), sy = sinf(ey), cy = cosf(ey), sz = sinf(ez), cz = cosf(ez);
    const float rx[9] = {1.0f, 0.0f, 0.0f, 0.0f, cx, -sx, 0.0f, sx, cx}, dx[9] = {0.0f, 0.0f, 0.0f, 0.0f, -sx, -cx, 0.0f, cx, -sx};
    const float ry[9] = {cy, 0.0f, sy, 0.0f, 1.0f, 0.0f, -sy, 0.0f, cy}, dy[9] = {-sy, 0.0f, cy, 0.0f, 0.0f, 0.0f, -cy, 0.0f, -sy};
    const float rz[9] = {cz, -sz, 0.0f, sz, cz, 0.0f, 0.0f, 0.0f, 1.0f}, dz[9] = {-sz, -cz, 0.0f, cz, -sz, 0.0f, 0.0f, 0.0f, 0.0f};
    float yx[9], m[9];
    mm3(ry, rx, yx);
    mm3(rz, yx, m);
#pragma unroll
    for (int i = 0; i < 9; ++i) o[i] = m[i];
    mm3(dz, yx, m);
#pragma unroll
    for (int i = 0; i < 9; ++i) o[27 + i] = m[i];
    mm3(ry, dx, yx);
    mm3(rz, yx, m);
#pragma unroll
    for (int i = 0; i < 9; ++i) o[9 + i] = m[i];
    mm3(dy, rx, yx);
    mm3(rz, yx, m);
#pragma unroll
    for (int i = 0; i < 9; ++i) o[18 + i] = m[i];
    o[36] = a.trans[(size_t)t * 3]; o[37] = a.trans[(size_t)t * 3 + 1]; o[38] = a.trans[(size_t)t * 3 + 2];
}

__device__ __forceinline__ float row3(const float* m, int c, float px, float py, float pz)
{
    return fmaf(m[3 * c + 2], pz, fmaf(m[3 * c + 1], py, m[3 * c] * px));
}

__device__ __forceinline__ void copy_run(const float* __restrict__ src, float* __restrict__ dst, size_t n)
{
    for (size_t i = threadIdx.x; i < n; i += THREADS) dst[i] = src[i];
}

// phase B's split of k: row r of a block's rows3 = 3 V rows is summed by nsplit threads, Kc terms each (the last part the rest).
// Written once for the kernel and for the plan the host reports.
struct Split { int nsplit, Kc; };

__host__ __device__ __forceinline__ Split split_k(int K, int rows3)
{
    const int nsplit = THREADS / rows3;          // rows3 <= 255: at least one part
    return {nsplit, (K + nsplit - 1) / nsplit};
}

__global__ void __launch_bounds__(THREADS) fit_grad(GradArgs a)
{
    extern __shared__ float4 lds4[];
    float* tile = reinterpret_cast<float*>(lds4);
    const int tid = threadIdx.x, K = a.Ki + a.Ke, W = K + SHARES;
    const int l0 = (int)blockIdx.x * a.V;
    const int Vb = min(a.V, a.L - l0), rows = 3 * Vb, rows3 = 3 * a.V, stride = rows3 | 1;
    float* cbuf = tile + (size_t)K * stride;          // [K] the frame's coefficients
    float* pbuf = cbuf + K;                           // [nsplit][rows3] partial shape rows
    float* dbuf = pbuf + THREADS;                     // [rows3] d loss / d shape
    float* sbuf = dbuf + THREADS;                     // [SHARES][V]
    float* posebuf = sbuf + SHARES * a.V;             // [PG][POSE]
    float* meanbuf = posebuf + PG * POSE;             // [rows3]
    float* wbuf = meanbuf + rows3;                    // [V]
    stage(a.id_base + (size_t)3 * l0 * a.Ki, tile, rows, a.Ki, stride);
    if (a.Ke > 0) stage(a.exp_base + (size_t)3 * l0 * a.Ke, tile + (size_t)a.Ki * stride, rows, a.Ke, stride);
    if (tid < rows) meanbuf[tid] = a.mean[(size_t)3 * l0 + tid];
    if (tid < Vb) wbuf[tid] = a.weights[l0 + tid];
    const int t0 = (int)blockIdx.y * a.chunk, t1 = min(a.T, t0 + a.chunk);
    if (a.snap && blockIdx.x == 0) {          // state order: id, exp, euler, trans
        const size_t nid = (size_t)a.id_rows * a.Ki, n = (size_t)(t1 - t0);
        if (a.id_rows == 1) { if (blockIdx.y == 0) copy_run(a.id, a.snap, nid); }
        else copy_run(a.id + (size_t)t0 * a.Ki, a.snap + (size_t)t0 * a.Ki, n * a.Ki);
        float* s = a.snap + nid;
        if (a.Ke > 0) copy_run(a.exp + (size_t)t0 * a.Ke, s + (size_t)t0 * a.Ke, n * a.Ke);
        s += (size_t)a.T * a.Ke;
        copy_run(a.euler + (size_t)t0 * 3, s + (size_t)t0 * 3, n * 3);
        s += (size_t)a.T * 3;
        copy_run(a.trans + (size_t)t0 * 3, s + (size_t)t0 * 3, n * 3);
    }
    const Split sp = split_k(K, rows3);
    const int nsplit = sp.nsplit, Kc = sp.Kc;
    const int part = tid / rows3, r = tid - part * rows3;
    for (int t = t0; t < t1; ++t) {
        // (the last reader of posebuf and cbuf, phase C / B of the frame before, is two barriers back)
        const int f = (t - t0) % PG;
        if (f == 0 && tid < min(PG, t1 - t)) pose(a, t + tid, posebuf + tid * POSE);
        const float* idrow = a.id + (a.id_rows == 1 ? (size_t)0 : (size_t)t * a.Ki);
        for (int k = tid; k < K; k += THREADS) cbuf[k] = k < a.Ki ? idrow[k] : a.exp[(size_t)t * a.Ke + (k - a.Ki)];
        __syncthreads();
        if (part < nsplit && r < rows) {
            const int k1 = min(K, (part + 1) * Kc);
            float acc = 0.0f;
            for (int k = part * Kc; k < k1; ++k) acc = fmaf(tile[(size_t)k * stride + r], cbuf[k], acc);
            pbuf[part * rows3 + r] = acc;
        }
        __syncthreads();
        if (tid < Vb) {
            float p[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                float v = meanbuf[3 * tid + j];
                for (int s = 0; s < nsplit; ++s) v += pbuf[s * rows3 + 3 * tid + j];
                p[j] = v;
            }
            const float* m = posebuf + f * POSE;
            const float q0 = row3(m, 0, p[0], p[1], p[2]) + m[36], q1 = row3(m, 1, p[0], p[1], p[2]) + m[37];
            const float z = a.camera_distance - (row3(m, 2, p[0], p[1], p[2]) + m[38]);
            const float u = fmaf(a.focal, q0, a.center * z) / z, v = fmaf(a.focal, q1, a.center * z) / z;
            const float* lm = a.lms + ((size_t)t * a.L + l0 + tid) * 2;
            const float ru = u - lm[0], rv = v - lm[1], w = wbuf[tid];
            const float s = w * a.scale, fz = a.focal / z;
            const float g0 = s * ru * fz, g1 = s * rv * fz;
            const float g2 = fmaf(g0, q0, g1 * q1) / z;          // d / d q.z = -d / dz, and dz carries -(g0 q0 + g1 q1) / z
#pragma unroll
            for (int j = 0; j < 3; ++j) dbuf[3 * tid + j] = fmaf(m[6 + j], g2, fmaf(m[3 + j], g1, m[j] * g0));
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                const float* d = m + 9 * (e + 1);
                sbuf[e * a.V + tid] = fmaf(g2, row3(d, 2, p[0], p[1], p[2]), fmaf(g1, row3(d, 1, p[0], p[1], p[2]), g0 * row3(d, 0, p[0], p[1], p[2])));
            }
            sbuf[3 * a.V + tid] = g0; sbuf[4 * a.V + tid] = g1; sbuf[5 * a.V + tid] = g2;
            sbuf[6 * a.V + tid] = w * fmaf(ru, ru, rv * rv);
        }
        __syncthreads();
        float* out = a.ws + ((size_t)blockIdx.x * a.T + t) * W;
        for (int j = a.need_idexp ? tid : K + tid; j < W; j += THREADS) {
            float acc = 0.0f;
            if (j < K) {
                const float* col = tile + (size_t)j * stride;
                for (int i = 0; i < rows; ++i) acc = fmaf(col[i], dbuf[i], acc);
            } else {
                const float* col = sbuf + (j - K) * a.V;
                for (int i = 0; i < Vb; ++i) acc += col[i];
            }
            out[j] = acc;
        }
    }
}

struct StepArgs {
    const float* ws;                                       // [slabs, T, Ki + Ke + 7]
    const float *id, *exp, *euler, *trans;                 // the iterate the partials were taken at (the snapshot, or the caller's arrays)
    float *p_id, *p_exp, *p_euler, *p_trans;               // run: parameters, first and second moments of the state
    float *m_id, *m_exp, *m_euler, *m_trans;
    float *v_id, *v_exp, *v_euler, *v_trans;
    float *g_id, *g_exp, *g_euler, *g_trans;               // grad: the gradients' destination (then p, m, v are NULL)
    float* loss;                                           // [LOSS]
    int slabs, L, Ki, Ke, T, id_rows, groups;
    int elem_blocks, id_blocks;
    float lam[6];
    int step_idexp, step_frame;                            // Adam's step number of this launch, per group
    float size_idexp, size_frame;                          // lr / (1 - beta1^step)
    float rsq_idexp, rsq_frame;                            // sqrt(1 - beta2^step)
};

__device__ __forceinline__ float lap_out(const float* x, int C, int R, int t, int c)
{
    return x[(size_t)t * C + c] - 0.5f * x[(size_t)max(t - 1, 0) * C + c] - 0.5f * x[(size_t)min(t + 1, R - 1) * C + c];
}

// d / d x[s, c] of the sum over t of lap_out^2 / 2
__device__ __forceinline__ float lap_grad(const float* x, int C, int R, int s, int c)
{
    float g = 0.0f;
    for (int t = max(s - 1, 0); t <= min(s + 1, R - 1); ++t) {
        const float coef = (t == s ? 1.0f : 0.0f) - (max(t - 1, 0) == s ? 0.5f : 0.0f) - (min(t + 1, R - 1) == s ? 0.5f : 0.0f);
        g = fmaf(coef, lap_out(x, C, R, t, c), g);
    }
    return g;
}

// One parameter: grp 0 id, 1 exp, 2 euler, 3 trans; row t, column c; `sum` the landmark term's gradient.
__device__ void element(const StepArgs& a, int grp, int t, int c, float sum)
{
    const float* x = grp == 0 ? a.id : grp == 1 ? a.exp : grp == 2 ? a.euler : a.trans;
    const int C = grp == 0 ? a.Ki : grp == 1 ? a.Ke : 3, R = grp == 0 ? a.id_rows : a.T;
    const size_t e = (size_t)t * C + c;
    const float n2 = 2.0f / ((float)R * (float)C);
    float g = sum;
    if (grp < 2) g = fmaf(a.lam[grp] * n2, x[e], g);
    const float lap = a.lam[2 + grp];
    if (R > 1 && lap != 0.0f) g = fmaf(lap * n2, lap_grad(x, C, R, t, c), g);
    float* go = grp == 0 ? a.g_id : grp == 1 ? a.g_exp : grp == 2 ? a.g_euler : a.g_trans;
    if (go) { go[e] = g; return; }
    float* p = grp == 0 ? a.p_id : grp == 1 ? a.p_exp : grp == 2 ? a.p_euler : a.p_trans;
    float* m = grp == 0 ? a.m_id : grp == 1 ? a.m_exp : grp == 2 ? a.m_euler : a.m_trans;
    float* v = grp == 0 ? a.v_id : grp == 1 ? a.v_exp : grp == 2 ? a.v_euler : a.v_trans;
    const float size = grp < 2 ? a.size_idexp : a.size_frame, rsq = grp < 2 ? a.rsq_idexp : a.rsq_frame;
    // torch.optim.Adam, single-tensor path: lerp_, mul_ + addcmul_, sqrt / sqrt(bias_correction2) + eps, addcdiv_
    const float m1 = fmaf(g - m[e], (float)(1.0 - 0.9), m[e]);
    const float v1 = fmaf((float)(1.0 - 0.999) * g, g, v[e] * 0.999f);
    m[e] = m1; v[e] = v1;
    p[e] = x[e] - size * (m1 / (sqrtf(v1) / rsq + 1e-8f));
}

// the sum of one value per thread, in a fixed tree; every thread gets it
__device__ float block_sum(float v, float* red)
{
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}

__device__ float mean_square(const float* x, size_t n, float* red)
{
    float acc = 0.0f;
    for (size_t i = threadIdx.x; i < n; i += THREADS) acc = fmaf(x[i], x[i], acc);
    return n ? block_sum(acc, red) / (float)n : 0.0f;
}

__device__ float lap_mean(const float* x, int C, int R, float* red)
{
    float acc = 0.0f;
    const size_t n = (size_t)R * C;
    if (R > 1)
        for (size_t i = threadIdx.x; i < n; i += THREADS) {
            const float o = lap_out(x, C, R, (int)(i / C), (int)(i % C));
            acc = fmaf(o, o, acc);
        }
    return n ? block_sum(acc, red) / (float)n : 0.0f;
}

__global__ void __launch_bounds__(THREADS) fit_step(StepArgs a)
{
    __shared__ float red[THREADS];
    const int tid = threadIdx.x, K = a.Ki + a.Ke, W = K + SHARES, b = blockIdx.x;
    const bool grad = a.g_euler != nullptr, idexp = grad || (a.groups & 1), frame = grad || (a.groups & 2);
    if (b < a.elem_blocks) {
        // exp [T, Ke], euler [T, 3], trans [T, 3], then id [T, Ki] when every frame has a row of its own
        const long long ne = (long long)a.T * a.Ke, n3 = (long long)a.T * 3, ni = a.id_rows == 1 ? 0 : (long long)a.T * a.Ki;
        long long e = (long long)b * THREADS + tid;
        int grp, C, col;
        if (e < ne) { grp = 1; C = a.Ke; col = a.Ki; }
        else if ((e -= ne) < n3) { grp = 2; C = 3; col = K; }
        else if ((e -= n3) < n3) { grp = 3; C = 3; col = K + 3; }
        else if ((e -= n3) < ni) { grp = 0; C = a.Ki; col = 0; }
        else return;
        if (!(grp < 2 ? idexp : frame)) return;
        const int t = (int)(e / C), c = (int)(e - (long long)t * C);
        float sum = 0.0f;
        for (int s = 0; s < a.slabs; ++s) sum += a.ws[((size_t)s * a.T + t) * W + col + c];
        element(a, grp, t, c, sum);
    } else if (b < a.elem_blocks + a.id_blocks) {
        // the shared id row: a wave per column, lane l sums the terms l, l + 64, ..., lane 0 the 64 lane sums in order
        if (!idexp) return;
        const int wave = tid >> 6, lane = tid & 63, c = (b - a.elem_blocks) * (THREADS / 64) + wave;
        float acc = 0.0f;
        const long long n = (long long)a.slabs * a.T;
        if (c < a.Ki)
            for (long long i = lane; i < n; i += 64) acc += a.ws[(size_t)i * W + c];
        red[tid] = acc;
        __syncthreads();
        if (lane == 0 && c < a.Ki) {
            float sum = 0.0f;
            for (int i = 0; i < 64; ++i) sum += red[wave * 64 + i];
            element(a, 0, 0, c, sum);
        }
    } else {
        float acc = 0.0f;
        const long long n = (long long)a.slabs * a.T;
        for (long long i = tid; i < n; i += THREADS) acc += a.ws[(size_t)i * W + K + 6];
        const float lan = block_sum(acc, red) / (2.0f * (float)a.T * (float)a.L);
        const float rid = mean_square(a.id, (size_t)a.id_rows * a.Ki, red), rexp = mean_square(a.exp, (size_t)a.T * a.Ke, red);
        const float lid = lap_mean(a.id, a.Ki, a.id_rows, red), lexp = lap_mean(a.exp, a.Ke, a.T, red);
        const float leu = lap_mean(a.euler, 3, a.T, red), ltr = lap_mean(a.trans, 3, a.T, red);
        if (tid == 0) {
            a.loss[0] = lan; a.loss[1] = rid; a.loss[2] = rexp; a.loss[3] = lid; a.loss[4] = lexp; a.loss[5] = leu; a.loss[6] = ltr;
            a.loss[7] = lan + a.lam[0] * rid + a.lam[1] * rexp + a.lam[2] * lid + a.lam[3] * lexp + a.lam[4] * leu + a.lam[5] * ltr;
        }
    }
}

inline bool finite(float x) { return x == x && x - x == 0.0f; }

struct Plan { int V, slabs, chunk, ychunks, nsplit, Kc; size_t ws_floats, params, lds; };

static bool sizes_ok(int L, int Ki, int Ke, int T) { return L >= 1 && T >= 1 && Ki >= 1 && Ke >= 0 && (long long)Ki + Ke <= 512; }

static Plan plan(int L, int Ki, int Ke, int T)
{
    Plan p;
    const int K = Ki + Ke;
    p.V = std::max(1, std::min(std::min(TILE_FLOATS / (3 * K), MAX_V), L));          // K <= 512: at least 8 points
    p.slabs = (L + p.V - 1) / p.V;
    // frames are split over blockIdx.y until the grid fills the chip; every split reads the slab's tile again
    long long want = std::max(1LL, 512LL / p.slabs);
    want = std::min(std::min(want, (long long)T), 65535LL);
    p.chunk = (int)(((long long)T + want - 1) / want);
    p.ychunks = (int)(((long long)T + p.chunk - 1) / p.chunk);
    p.ws_floats = (size_t)p.slabs * T * (K + SHARES);
    p.ws_floats = (p.ws_floats + 3) & ~(size_t)3;
    p.params = ((size_t)T * (K + 6) + 3) & ~(size_t)3;          // the snapshot's room: a row of id per frame at the most
    const int rows3 = 3 * p.V;
    const Split sp = split_k(K, rows3);
    p.nsplit = sp.nsplit; p.Kc = sp.Kc;
    p.lds = ((size_t)K * (rows3 | 1) + K + 2 * THREADS + SHARES * p.V + PG * POSE + rows3 + p.V) * sizeof(float);
    return p;
}

struct Common {
    const float *mean, *id_base, *exp_base, *lms, *weights;
    int L, Ki, Ke, T, id_rows;
    float camera_distance, focal, center;
    const float* lambdas;
};

// The sizes both entry points (and the plan hook) refuse, in two steps because the entry points check their other arguments between
// them: the counts ...
static int check_counts(const char* what, int L, int Ki, int Ke, int T)
{
    if (L < 1 || T < 1) { set_error("%s: bad argument (L = %d, T = %d must be positive)", what, L, T); return R3D_ERR_INVALID_ARG; }
    if (Ki < 1 || Ke < 0 || (long long)Ki + Ke > 512) { set_error("%s: Ki = %d, Ke = %d: need Ki >= 1, Ke >= 0, Ki + Ke <= 512", what, Ki, Ke); return R3D_ERR_INVALID_ARG; }
    return R3D_OK;
}

// ... and the index products, of counts that passed
static int check_products(const char* what, int L, int Ki, int Ke, int T)
{
    const Plan p = plan(L, Ki, Ke, T);
    if (!below_2_31(what, "slabs T (Ki + Ke + 7)", (double)p.slabs * T * (Ki + Ke + SHARES), "elements")) return R3D_ERR_INVALID_ARG;
    if (!below_2_31(what, "2 L T", 2.0 * L * T, "elements")) return R3D_ERR_INVALID_ARG;
    return R3D_OK;
}

static int check_common(const char* what, const Common& c)
{
    if (!c.mean || !c.id_base || !c.lms || !c.weights || !c.lambdas) { set_error("%s: NULL pointer (key_mean, key_id_base, lms, weights and lambdas are required)", what); return R3D_ERR_INVALID_ARG; }
    if (const int rc = check_counts(what, c.L, c.Ki, c.Ke, c.T)) return rc;
    if (c.Ke > 0 && !c.exp_base) { set_error("%s: key_exp_base is NULL with Ke = %d", what, c.Ke); return R3D_ERR_INVALID_ARG; }
    if (c.id_rows != 1 && c.id_rows != c.T) { set_error("%s: id_rows = %d is neither 1 nor T = %d", what, c.id_rows, c.T); return R3D_ERR_INVALID_ARG; }
    if (!finite(c.camera_distance) || !finite(c.focal) || !finite(c.center)) { set_error("%s: camera_distance, focal or center is not finite", what); return R3D_ERR_INVALID_ARG; }
    if (!(c.focal > 0.0f)) { set_error("%s: focal = %g must be positive", what, (double)c.focal); return R3D_ERR_INVALID_ARG; }
    for (int i = 0; i < 6; ++i)
        if (!finite(c.lambdas[i])) { set_error("%s: lambdas[%d] is not finite", what, i); return R3D_ERR_INVALID_ARG; }
    return check_products(what, c.L, c.Ki, c.Ke, c.T);
}

// the two launches of one evaluation: `g` and `s` hold everything but the plan's numbers
static int enqueue(const char* what, const Common& c, const Plan& p, GradArgs g, StepArgs s, void* workspace, hipStream_t st)
{
    g.mean = c.mean; g.id_base = c.id_base; g.exp_base = c.Ke > 0 ? c.exp_base : nullptr; g.lms = c.lms; g.weights = c.weights;
    g.ws = (float*)workspace;
    g.L = c.L; g.Ki = c.Ki; g.Ke = c.Ke; g.T = c.T; g.id_rows = c.id_rows; g.V = p.V; g.chunk = p.chunk;
    g.camera_distance = c.camera_distance; g.focal = c.focal; g.center = c.center;
    g.scale = (float)(1.0 / ((double)c.T * (double)c.L));
    s.ws = g.ws; s.slabs = p.slabs; s.L = c.L; s.Ki = c.Ki; s.Ke = c.Ke; s.T = c.T; s.id_rows = c.id_rows;
    for (int i = 0; i < 6; ++i) s.lam[i] = c.lambdas[i];
    const long long elems = (long long)c.T * (c.Ke + 6) + (c.id_rows == 1 ? 0 : (long long)c.T * c.Ki);
    s.elem_blocks = (int)((elems + THREADS - 1) / THREADS);
    s.id_blocks = c.id_rows == 1 ? (c.Ki + THREADS / 64 - 1) / (THREADS / 64) : 0;
    hipLaunchKernelGGL(fit_grad, dim3((unsigned)p.slabs, (unsigned)p.ychunks), dim3(THREADS), p.lds, st, g);
    hipLaunchKernelGGL(fit_step, dim3((unsigned)(s.elem_blocks + s.id_blocks + 1)), dim3(THREADS), 0, st, s);
    return check_launch(what);
}

}  // namespace fit
}  // namespace r3d

using namespace r3d;

extern "C" size_t r3d_fit_workspace_bytes(int L, int Ki, int Ke, int T)
{
    if (!fit::sizes_ok(L, Ki, Ke, T)) return 0;
    const fit::Plan p = fit::plan(L, Ki, Ke, T);
    return (p.ws_floats + p.params) * sizeof(float);
}

extern "C" size_t r3d_fit_state_bytes(int Ki, int Ke, int T, int id_rows)
{
    if (!fit::sizes_ok(1, Ki, Ke, T) || (id_rows != 1 && id_rows != T)) return 0;
    return (3 * ((size_t)id_rows * Ki + (size_t)T * (Ke + 6)) + fit::LOSS) * sizeof(float);
}

extern "C" int r3d_fit_landmark_grad(const float* key_mean, const float* key_id_base, const float* key_exp_base, int L, int Ki, int Ke,
                                     const float* lms, const float* weights, int T, int id_rows, float camera_distance, float focal,
                                     float center, const float* lambdas, const float* id, const float* exp, const float* euler,
                                     const float* trans, float* grad_id, float* grad_exp, float* grad_euler, float* grad_trans, float* loss,
                                     void* workspace, size_t workspace_bytes, r3d_stream_t stream)
{
    const char* what = "fit_landmark_grad";
    const fit::Common c = {key_mean, key_id_base, key_exp_base, lms, weights, L, Ki, Ke, T, id_rows, camera_distance, focal, center, lambdas};
    if (!id || !euler || !trans || !grad_id || !grad_euler || !grad_trans || !loss) { set_error("%s: NULL pointer (the parameters, the gradients and the loss are required)", what); return R3D_ERR_INVALID_ARG; }
    if (const int rc = fit::check_common(what, c)) return rc;
    if (Ke > 0 && (!exp || !grad_exp)) { set_error("%s: NULL pointer (exp and grad_exp are required with Ke = %d)", what, Ke); return R3D_ERR_INVALID_ARG; }
    if (!workspace_ok(what, workspace, workspace_bytes, r3d_fit_workspace_bytes(L, Ki, Ke, T), 16, "r3d_fit_workspace_bytes")) return R3D_ERR_WORKSPACE;
    const size_t rows = (size_t)3 * L, nid = (size_t)id_rows * Ki, nexp = (size_t)T * Ke, n3 = (size_t)T * 3;
    const Span spans[] = {writes(grad_id, nid), writes(grad_exp, nexp), writes(grad_euler, n3), writes(grad_trans, n3), writes(loss, (size_t)fit::LOSS),
                          writes((const char*)workspace, r3d_fit_workspace_bytes(L, Ki, Ke, T)), reads(key_mean, rows), reads(key_id_base, rows * Ki),
                          reads(key_exp_base, rows * Ke), reads(lms, (size_t)T * L * 2), reads(weights, (size_t)L), reads(id, nid), reads(exp, nexp),
                          reads(euler, n3), reads(trans, n3)};
    if (clash(spans)) { set_error("%s: an output or the workspace overlaps an input or another output", what); return R3D_ERR_INVALID_ARG; }
    const fit::Plan p = fit::plan(L, Ki, Ke, T);
    fit::GradArgs g = {};
    g.id = id; g.exp = Ke > 0 ? exp : nullptr; g.euler = euler; g.trans = trans; g.snap = nullptr; g.need_idexp = 1;
    fit::StepArgs s = {};
    s.id = id; s.exp = g.exp; s.euler = euler; s.trans = trans;
    s.g_id = grad_id; s.g_exp = Ke > 0 ? grad_exp : nullptr; s.g_euler = grad_euler; s.g_trans = grad_trans; s.loss = loss; s.groups = 3;
    ProfScope ps(R3D_PROF_MISC, (hipStream_t)stream);
    return fit::enqueue(what, c, p, g, s, workspace, (hipStream_t)stream);
}

extern "C" int r3d_fit_landmark_run(const float* key_mean, const float* key_id_base, const float* key_exp_base, int L, int Ki, int Ke,
                                    const float* lms, const float* weights, int T, int id_rows, float camera_distance, float focal,
                                    float center, const float* lambdas, float lr_idexp, float lr_frame, int step0_idexp, int step0_frame,
                                    int n_iter, int groups, float* state, void* workspace, size_t workspace_bytes, r3d_stream_t stream)
{
    const char* what = "fit_landmark_run";
    const fit::Common c = {key_mean, key_id_base, key_exp_base, lms, weights, L, Ki, Ke, T, id_rows, camera_distance, focal, center, lambdas};
    if (!state) { set_error("%s: NULL pointer (state)", what); return R3D_ERR_INVALID_ARG; }
    if (const int rc = fit::check_common(what, c)) return rc;
    if (!fit::finite(lr_idexp) || !fit::finite(lr_frame) || !(lr_idexp > 0.0f) || !(lr_frame > 0.0f)) { set_error("%s: lr_idexp = %g and lr_frame = %g must be positive and finite", what, (double)lr_idexp, (double)lr_frame); return R3D_ERR_INVALID_ARG; }
    if (step0_idexp < 0 || step0_frame < 0) { set_error("%s: step0_idexp = %d and step0_frame = %d must not be negative", what, step0_idexp, step0_frame); return R3D_ERR_INVALID_ARG; }
    if (n_iter < 1 || (long long)n_iter + std::max(step0_idexp, step0_frame) > 2147483647LL) { set_error("%s: n_iter = %d must be positive (and step0 + n_iter below 2^31)", what, n_iter); return R3D_ERR_INVALID_ARG; }
    if (groups < 1 || groups > 3) { set_error("%s: groups = %d is outside 1 .. 3 (bit 0 id and exp, bit 1 euler and trans)", what, groups); return R3D_ERR_INVALID_ARG; }
    if (!workspace_ok(what, workspace, workspace_bytes, r3d_fit_workspace_bytes(L, Ki, Ke, T), 16, "r3d_fit_workspace_bytes")) return R3D_ERR_WORKSPACE;
    const size_t rows = (size_t)3 * L, nid = (size_t)id_rows * Ki, nexp = (size_t)T * Ke, n3 = (size_t)T * 3, np = nid + nexp + 2 * n3;
    const Span spans[] = {writes(state, 3 * np + fit::LOSS), writes((const char*)workspace, r3d_fit_workspace_bytes(L, Ki, Ke, T)), reads(key_mean, rows),
                          reads(key_id_base, rows * Ki), reads(key_exp_base, rows * Ke), reads(lms, (size_t)T * L * 2), reads(weights, (size_t)L)};
    if (clash(spans)) { set_error("%s: the state or the workspace overlaps an input or one another", what); return R3D_ERR_INVALID_ARG; }
    const fit::Plan p = fit::plan(L, Ki, Ke, T);
    fit::GradArgs g = {};
    float* par = state;
    g.id = par; g.exp = Ke > 0 ? par + nid : nullptr; g.euler = par + nid + nexp; g.trans = par + nid + nexp + n3;
    g.snap = (float*)workspace + p.ws_floats; g.need_idexp = groups & 1;
    fit::StepArgs s = {};
    s.id = g.snap; s.exp = g.snap + nid; s.euler = g.snap + nid + nexp; s.trans = g.snap + nid + nexp + n3;
    float* const base[3] = {state, state + np, state + 2 * np};
    s.p_id = base[0]; s.p_exp = base[0] + nid; s.p_euler = base[0] + nid + nexp; s.p_trans = base[0] + nid + nexp + n3;
    s.m_id = base[1]; s.m_exp = base[1] + nid; s.m_euler = base[1] + nid + nexp; s.m_trans = base[1] + nid + nexp + n3;
    s.v_id = base[2]; s.v_exp = base[2] + nid; s.v_euler = base[2] + nid + nexp; s.v_trans = base[2] + nid + nexp + n3;
    s.loss = state + 3 * np; s.groups = groups;
    ProfScope ps(R3D_PROF_MISC, (hipStream_t)stream);
    for (int i = 0; i < n_iter; ++i) {
        // the bias corrections as torch takes them: in double, from the step number
        s.step_idexp = step0_idexp + i + 1; s.step_frame = step0_frame + i + 1;
        s.size_idexp = (float)((double)lr_idexp / (1.0 - std::pow(0.9, (double)s.step_idexp)));
        s.size_frame = (float)((double)lr_frame / (1.0 - std::pow(0.9, (double)s.step_frame)));
        s.rsq_idexp = (float)std::sqrt(1.0 - std::pow(0.999, (double)s.step_idexp));
        s.rsq_frame = (float)std::sqrt(1.0 - std::pow(0.999, (double)s.step_frame));
        if (const int rc = fit::enqueue(what, c, p, g, s, workspace, (hipStream_t)stream)) return rc;
    }
    return R3D_OK;
}

// Test hook outside the C ABI of include/r3d_hip_fit.h (OPTIONAL_SIGNATURES of real3dportrait_amd/_lib.py): the plan both entry points
// launch fit_grad with at these sizes, out = V, slabs, chunk, ychunks, nsplit, Kc, lds_bytes, ws_floats (the partials' part of the
// workspace; the snapshot's room follows it); sizes they refuse are refused here with the same status.  No HIP call.
extern "C" int r3d_debug_fit_plan(int L, int Ki, int Ke, int T, int32_t out[8])
{
    const char* what = "debug_fit_plan";
    if (!out) { set_error("%s: NULL pointer (out)", what); return R3D_ERR_INVALID_ARG; }
    if (const int rc = fit::check_counts(what, L, Ki, Ke, T)) return rc;
    if (const int rc = fit::check_products(what, L, Ki, Ke, T)) return rc;
    const fit::Plan p = fit::plan(L, Ki, Ke, T);
    out[0] = p.V; out[1] = p.slabs; out[2] = p.chunk; out[3] = p.ychunks; out[4] = p.nsplit; out[5] = p.Kc;
    out[6] = (int32_t)p.lds; out[7] = (int32_t)p.ws_floats;
    return R3D_OK;
}
