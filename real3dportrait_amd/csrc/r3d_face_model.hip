// Morphable face model: ParametricFaceModel.compute_face_vertex (deep_3drecon/deep_3drecon_models/bfm.py:332-347) and
// Face3DHelper.reconstruct_lm2d (data_util/face3d_helper.py:132-169), inference only, fp32.  Per frame t and row r of the
// bases (row 3 n + c is component c of vertex n):
//   p[r]   = fma chain over k from 0.0f, in this order: id_base[r, 0 .. Ki) x id[t], then exp_base[r, 0 .. Ke) x exp[t]; then + mean[r].
//            (The mean is added last, as the reference does: a chain begun at the mean, of size 1, rounds every one of its K small
//            terms at the mean's ulp, and its error grows with K -- 2.9e-6 at K = 512 against 6e-7 this way.)
//   q[c]   = fma(M[c][2], p.z, fma(M[c][1], p.y, M[c][0] p.x)) + trans[t][c], M = Rz Ry Rx (the reference multiplies p by its transpose
//            from the right); q.z = camera_distance - q.z when to_camera
//   lm2d   = ((focal q.x + center q.z) / q.z, image_size - (focal q.y + center q.z) / q.z) / image_size          (landmarks only)
// One kernel template serves both entry points.  A block owns V vertices = 3 V rows, one row per thread.  It copies its rows of both bases,
// which are ONE contiguous run of each array, into LDS transposed ([k][row]: a wave then reads 64 consecutive floats per k, no bank
// conflict), then walks the frames in groups of 8, 4, 2, 1: one LDS read feeds 8 FMAs whose other operand, the frame's coefficient, is
// wave-uniform and comes through the scalar cache.  So the bases leave HBM once per call, not once per frame.  A frame's chain never
// depends on the group it falls in, on T or on the grid: frame t alone and frame t of 51 are bit-identical.  The three components of a
// vertex meet through LDS (two barriers per group), and each thread stores one float of vertex [T, N, 3]: consecutive threads,
// consecutive addresses.  Sines and cosines are computed by the group's first lanes, once per frame and block.
// A NULL exp, euler or trans reads as 0.0f in the very same arithmetic, so it is bit-identical to an array of zeros.
#include "r3d_common.h"

namespace r3d {
namespace face {

constexpr int THREADS = 128;
constexpr int LDS_FLOATS = 15000;              // the base tile; with the two small buffers under 64 KiB: two blocks per CU
constexpr int GROUP = 8;                       // frames per LDS read
constexpr int POSE = 12;                       // M (9) and trans (3) per frame

struct Args {
    const float* mean;                    // [3 N]
    const float* id_base;                 // [3 N, Ki]
    const float* exp_base;                // [3 N, Ke] or NULL with Ke = 0
    const float* euler;                   // [T, 3] or NULL
    const float* trans;                   // [T, 3] or NULL
    int N, Ki, Ke, T, V, chunk;           // V vertices per block, chunk frames per blockIdx.y
    int id_wide, exp_wide;                // 16-byte loads allowed for that base
    float camera_distance, focal, center, image_size;
    int to_camera;
};

// rows x K floats from src (contiguous) to dst[k * stride + row]
__device__ __forceinline__ void stage(const float* __restrict__ src, float* dst, int rows, int K, int stride, int wide)
{
    if (wide) {
        const int q = K >> 2, n = rows * q;
        int r = (int)threadIdx.x / q, kq = (int)threadIdx.x - r * q;
        const int dr = THREADS / q, dk = THREADS - dr * q;
        for (int i = threadIdx.x; i < n; i += THREADS) {
            const float4 v = *reinterpret_cast<const float4*>(src + (size_t)i * 4);
            float* d = dst + (size_t)(kq * 4) * stride + r;
            d[0] = v.x; d[stride] = v.y; d[2 * stride] = v.z; d[3 * stride] = v.w;
            r += dr; kq += dk;
            if (kq >= q) { kq -= q; ++r; }
        }
    } else {
        const int n = rows * K;
        int r = (int)threadIdx.x / K, k = (int)threadIdx.x - r * K;
        const int dr = THREADS / K, dk = THREADS - dr * K;
        for (int i = threadIdx.x; i < n; i += THREADS) {
            dst[(size_t)k * stride + r] = src[i];
            r += dr; k += dk;
            if (k >= K) { k -= K; ++r; }
        }
    }
}

// M = Rz Ry Rx of compute_rotation (bfm.py:204-238), row-major, and the translation
__device__ __forceinline__ void pose(const Args& a, int t, float* o)
{
    float ex = 0.0f, ey = 0.0f, ez = 0.0f, tx = 0.0f, ty = 0.0f, tz = 0.0f;
    if (a.euler) { ex = a.euler[(size_t)t * 3]; ey = a.euler[(size_t)t * 3 + 1]; ez = a.euler[(size_t)t * 3 + 2]; }
    if (a.trans) { tx = a.trans[(size_t)t * 3]; ty = a.trans[(size_t)t * 3 + 1]; tz = a.trans[(size_t)t * 3 + 2]; }
    const float sx = sinf(ex), cx = cosf(ex), sy = sinf(ey), cy = cosf(ey), sz = sinf(ez), cz = cosf(ez);
    const float a00 = cz * cy, a01 = -sz, a02 = cz * sy;          // Rz Ry
    const float a10 = sz * cy, a11 = cz, a12 = sz * sy;
    const float a20 = -sy, a22 = cy;
    o[0] = a00; o[1] = fmaf(a02, sx, a01 * cx); o[2] = fmaf(a02, cx, -(a01 * sx));
    o[3] = a10; o[4] = fmaf(a12, sx, a11 * cx); o[5] = fmaf(a12, cx, -(a11 * sx));
    o[6] = a20; o[7] = a22 * sx;                o[8] = a22 * cx;
    o[9] = tx; o[10] = ty; o[11] = tz;
}

__device__ __forceinline__ float transform(const float* m, int c, float px, float py, float pz)
{
    return fmaf(m[3 * c + 2], pz, fmaf(m[3 * c + 1], py, m[3 * c] * px)) + m[9 + c];
}

// frames t0 .. t0 + F of the block's rows: tile [K][stride] in LDS, pbuf [GROUP][THREADS], posebuf [GROUP][POSE]
template <int F, bool LM>
__device__ __forceinline__ void frames(const Args& a, const float* __restrict__ id, const float* __restrict__ exp, float* __restrict__ out,
                                       int t0, int rows, int r0, float mean, const float* tile, int stride, float* pbuf, float* posebuf)
{
    const int tid = threadIdx.x;
    if (tid < F) pose(a, t0 + tid, posebuf + tid * POSE);
    float acc[F];
#pragma unroll
    for (int f = 0; f < F; ++f) acc[f] = 0.0f;
    if (tid < rows) {
        const float* __restrict__ ci = id + (size_t)t0 * a.Ki;
        const float* col = tile + tid;
        for (int k = 0; k < a.Ki; ++k) {
            const float b = col[(size_t)k * stride];
#pragma unroll
            for (int f = 0; f < F; ++f) acc[f] = fmaf(b, ci[(size_t)f * a.Ki + k], acc[f]);
        }
        col += (size_t)a.Ki * stride;
        if (exp) {
            const float* __restrict__ ce = exp + (size_t)t0 * a.Ke;
            for (int k = 0; k < a.Ke; ++k) {
                const float b = col[(size_t)k * stride];
#pragma unroll
                for (int f = 0; f < F; ++f) acc[f] = fmaf(b, ce[(size_t)f * a.Ke + k], acc[f]);
            }
        } else {
            for (int k = 0; k < a.Ke; ++k) {
                const float b = col[(size_t)k * stride];
#pragma unroll
                for (int f = 0; f < F; ++f) acc[f] = fmaf(b, 0.0f, acc[f]);
            }
        }
    }
#pragma unroll
    for (int f = 0; f < F; ++f) pbuf[f * THREADS + tid] = acc[f] + mean;          // the mean last, as the reference: the chain rounds at its own size
    __syncthreads();
    if (tid < rows) {
        const int v = tid / 3, c = tid - 3 * v;
        const size_t n = (size_t)(r0 / 3) + v;
#pragma unroll
        for (int f = 0; f < F; ++f) {
            const float* p = pbuf + f * THREADS + 3 * v;
            const float* m = posebuf + f * POSE;
            const float px = p[0], py = p[1], pz = p[2];
            if (!LM) {
                float q = transform(m, c, px, py, pz);
                if (c == 2 && a.to_camera) q = a.camera_distance - q;
                out[((size_t)(t0 + f) * a.N + n) * 3 + c] = q;
            } else if (c < 2) {
                float z = transform(m, 2, px, py, pz);
                if (a.to_camera) z = a.camera_distance - z;
                float u = fmaf(a.focal, transform(m, c, px, py, pz), a.center * z) / z;
                if (c == 1) u = a.image_size - u;
                out[((size_t)(t0 + f) * a.N + n) * 2 + c] = u / a.image_size;
            }
        }
    }
    __syncthreads();
}

// id [T, Ki], exp [T, Ke] or NULL and out ([T, N, 3] or [T, N, 2]) are arguments of their own, declared not to alias: the coefficient of a
// (frame, k) is the same in every lane, and only then does the compiler fetch it with a scalar load into the FMA's scalar operand
template <bool LM>
__global__ void __launch_bounds__(THREADS) face_model(Args a, const float* __restrict__ id, const float* __restrict__ exp,
                                                      float* __restrict__ out)
{
    extern __shared__ float4 lds4[];
    float* tile = reinterpret_cast<float*>(lds4);
    const int K = a.Ki + a.Ke;
    const int r0 = (int)blockIdx.x * a.V * 3;
    const int rows = min(a.V * 3, a.N * 3 - r0), stride = a.V * 3;
    float* pbuf = tile + (size_t)K * stride;
    float* posebuf = pbuf + GROUP * THREADS;
    stage(a.id_base + (size_t)r0 * a.Ki, tile, rows, a.Ki, stride, a.id_wide);
    if (a.Ke > 0) stage(a.exp_base + (size_t)r0 * a.Ke, tile + (size_t)a.Ki * stride, rows, a.Ke, stride, a.exp_wide);
    const float mean = (int)threadIdx.x < rows ? a.mean[(size_t)r0 + threadIdx.x] : 0.0f;
    __syncthreads();
    int t = (int)blockIdx.y * a.chunk;
    const int t1 = min(a.T, t + a.chunk);
    for (; t + 8 <= t1; t += 8) frames<8, LM>(a, id, exp, out, t, rows, r0, mean, tile, stride, pbuf, posebuf);
    if (t + 4 <= t1) { frames<4, LM>(a, id, exp, out, t, rows, r0, mean, tile, stride, pbuf, posebuf); t += 4; }
    if (t + 2 <= t1) { frames<2, LM>(a, id, exp, out, t, rows, r0, mean, tile, stride, pbuf, posebuf); t += 2; }
    if (t < t1) frames<1, LM>(a, id, exp, out, t, rows, r0, mean, tile, stride, pbuf, posebuf);
}

inline bool finite(float x) { return x == x && x - x == 0.0f; }

// The sizes both entry points (and the plan hook) refuse, in two steps because the entry points check exp_base between them: the counts ...
static int check_counts(const char* what, bool lm, int N, int Ki, int Ke, int T)
{
    if (N < 1 || T < 1) { set_error("%s: bad argument (%s = %d, T = %d must be positive)", what, lm ? "L" : "N", N, T); return R3D_ERR_INVALID_ARG; }
    if (Ki < 1 || Ke < 0 || (long long)Ki + Ke > 512) { set_error("%s: Ki = %d, Ke = %d: need Ki >= 1, Ke >= 0, Ki + Ke <= 512", what, Ki, Ke); return R3D_ERR_INVALID_ARG; }
    return R3D_OK;
}

// ... and the index product
static int check_product(const char* what, bool lm, int N, int T)
{
    return below_2_31(what, lm ? "3 L T" : "3 N T", 3.0 * (double)N * (double)T, "elements") ? R3D_OK : R3D_ERR_INVALID_ARG;
}

// The launch plan of accepted sizes.  A block owns V vertices and walks `chunk` frames: grid (xblocks, yblocks), lds bytes of LDS.
struct Plan { int V, xblocks, chunk, yblocks; size_t lds; };

static Plan plan(int N, int Ki, int Ke, int T)
{
    Plan p;
    const int K = Ki + Ke;
    p.V = std::min(std::min(LDS_FLOATS / (3 * K), THREADS / 3), N);          // K <= 512: at least 9 vertices
    const long long xblocks = ((long long)N + p.V - 1) / p.V;
    // frames are split over blockIdx.y only while the vertex tiles alone leave the chip idle (landmarks: L = 68 is two tiles); every split
    // reads the tile again, and a frame's result does not depend on its split
    long long want = std::max(1LL, 512 / xblocks);
    want = std::min(std::min(want, ((long long)T + GROUP - 1) / GROUP), 65535LL);
    const long long per = ((long long)T + want - 1) / want;
    p.chunk = (int)std::min((long long)T, (per + GROUP - 1) / GROUP * GROUP);
    p.xblocks = (int)xblocks;
    p.yblocks = (int)(((long long)T + p.chunk - 1) / p.chunk);
    p.lds = ((size_t)K * p.V * 3 + GROUP * THREADS + GROUP * POSE) * sizeof(float);
    return p;
}

static int launch(const char* what, bool lm, const float* mean, const float* id_base, const float* exp_base, int N, int Ki, int Ke,
                  const float* id, const float* exp, const float* euler, const float* trans, int T, float camera_distance, int to_camera,
                  float focal, float center, float image_size, float* out, hipStream_t st)
{
    if (!mean || !id_base || !id || !out) { set_error("%s: NULL pointer (mean, id_base, id and the output are required)", what); return R3D_ERR_INVALID_ARG; }
    if (const int rc = check_counts(what, lm, N, Ki, Ke, T)) return rc;
    if (Ke > 0 && !exp_base) { set_error("%s: exp_base is NULL with Ke = %d", what, Ke); return R3D_ERR_INVALID_ARG; }
    if (const int rc = check_product(what, lm, N, T)) return rc;
    if (!finite(camera_distance)) { set_error("%s: camera_distance is not finite", what); return R3D_ERR_INVALID_ARG; }
    if (lm) {
        if (!finite(focal) || !finite(center) || !finite(image_size)) { set_error("%s: focal, center or image_size is not finite", what); return R3D_ERR_INVALID_ARG; }
        if (!(focal > 0.0f) || !(image_size > 0.0f)) { set_error("%s: focal = %g and image_size = %g must be positive", what, (double)focal, (double)image_size); return R3D_ERR_INVALID_ARG; }
    }
    const size_t rows = (size_t)3 * N, nout = (size_t)(lm ? 2 : 3) * N * T;
    const Span spans[] = {writes(out, nout), reads(mean, rows), reads(id_base, rows * Ki), reads(exp_base, rows * Ke), reads(id, (size_t)T * Ki),
                          reads(exp, (size_t)T * Ke), reads(euler, (size_t)T * 3), reads(trans, (size_t)T * 3)};          // (absent, or Ke = 0: no part)
    if (clash(spans)) { set_error("%s: the output overlaps an input", what); return R3D_ERR_INVALID_ARG; }

    Args a;
    a.mean = mean; a.id_base = id_base; a.exp_base = Ke > 0 ? exp_base : nullptr; a.euler = euler; a.trans = trans;
    if (Ke == 0) exp = nullptr;
    a.N = N; a.Ki = Ki; a.Ke = Ke; a.T = T;
    const Plan p = plan(N, Ki, Ke, T);
    a.V = p.V; a.chunk = p.chunk;
    a.id_wide = aligned16(id_base) && (Ki & 3) == 0;
    a.exp_wide = Ke > 0 && aligned16(exp_base) && (Ke & 3) == 0;
    a.camera_distance = camera_distance; a.focal = focal; a.center = center; a.image_size = image_size; a.to_camera = to_camera ? 1 : 0;

    ProfScope ps(R3D_PROF_MISC, st);
    if (lm) hipLaunchKernelGGL(face_model<true>, dim3((unsigned)p.xblocks, (unsigned)p.yblocks), dim3(THREADS), p.lds, st, a, id, exp, out);
    else hipLaunchKernelGGL(face_model<false>, dim3((unsigned)p.xblocks, (unsigned)p.yblocks), dim3(THREADS), p.lds, st, a, id, exp, out);
    return check_launch(what);
}

}  // namespace face
}  // namespace r3d

using namespace r3d;

extern "C" int r3d_face_vertex(const float* mean, const float* id_base, const float* exp_base, int N, int Ki, int Ke, const float* id,
                               const float* exp, const float* euler, const float* trans, int T, float camera_distance, int to_camera,
                               float* vertex, r3d_stream_t stream)
{
    return face::launch("face_vertex", false, mean, id_base, exp_base, N, Ki, Ke, id, exp, euler, trans, T, camera_distance, to_camera,
                        1.0f, 0.0f, 1.0f, vertex, (hipStream_t)stream);
}

extern "C" int r3d_face_landmarks(const float* key_mean, const float* key_id_base, const float* key_exp_base, int L, int Ki, int Ke,
                                  const float* id, const float* exp, const float* euler, const float* trans, int T, float camera_distance,
                                  int to_camera, float focal, float center, float image_size, float* lm2d, r3d_stream_t stream)
{
    return face::launch("face_landmarks", true, key_mean, key_id_base, key_exp_base, L, Ki, Ke, id, exp, euler, trans, T, camera_distance,
                        to_camera, focal, center, image_size, lm2d, (hipStream_t)stream);
}

// Test hook outside the C ABI of include/r3d_hip.h (OPTIONAL_SIGNATURES of real3dportrait_amd/_lib.py): the plan both entry points launch
// with at these sizes, out = V, xblocks, chunk, yblocks, lds_bytes; sizes they refuse are refused here with the same status.  No HIP call.
extern "C" int r3d_debug_face_plan(int N, int Ki, int Ke, int T, int32_t out[5])
{
    const char* what = "debug_face_plan";
    if (!out) { set_error("%s: NULL pointer (out)", what); return R3D_ERR_INVALID_ARG; }
    if (const int rc = face::check_counts(what, false, N, Ki, Ke, T)) return rc;
    if (const int rc = face::check_product(what, false, N, T)) return rc;
    const face::Plan p = face::plan(N, Ki, Ke, T);
    out[0] = p.V; out[1] = p.xblocks; out[2] = p.chunk; out[3] = p.yblocks; out[4] = (int32_t)p.lds;
    return R3D_OK;
}
