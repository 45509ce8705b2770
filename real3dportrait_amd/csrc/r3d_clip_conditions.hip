// Per-clip conditions of the frame loop, inference only: the camera trajectory of prepare_batch_from_inp
// (inference/real3d_infer.py:311-319), which is get_eg3d_convention_camera_pose_intrinsic (data_gen/eg3d/convert_to_eg3d_convention.py:
// 42-146) followed by smooth_camera_sequence (inference/infer_utils.py:40-69), and smooth_features_xd (infer_utils.py:71-101).
//
// Camera, one lane per frame, everything in fp64 between the fp32 loads and the fp32 stores:
//   F(t)   the frame's own camera: M = Rz Ry Rx of compute_rotation (bfm.py:204-238), R = M^T, rotation block R diag(1, -1, -1),
//          position -R (trans + (0, 0, -10)) 0.27 + (0, 0.006, 0.161), rescaled to length `radius` when radius > 0; the block goes to a
//          unit quaternion and back, and the twelve numbers are rounded to fp32.  The reference's frame camera is fp32-valued too (its R
//          and its position come out of fp32 arithmetic), and r3d_camera_smooth, which starts from an fp32 array, sees the same numbers.
//   out(i) over the window [max(0, i - K), min(T, i + K + 1)), K = kernel_size / 2: the mean of the positions and the chordal L2 mean of
//          the rotations -- each block to a unit quaternion q, A = sum q q^T, the eigenvector of A's largest eigenvalue, back to a matrix
//          (scipy's Rotation.mean) -- rounded to fp32 once.  A window of ONE frame returns that frame's F unchanged: the mean of one.
// Two traps of this product's data:
//   (1) at zero pose the block is exactly diag(1, -1, -1), a half turn about x with trace -1: w = sqrt(1 + trace) / 2 is 0 there, and
//       the one-formula conversion divides by it.  mat_to_quat branches on the largest of (w, x, y, z) (Shepperd);
//   (2) a static clip has windows of identical rotations: A has rank one and three eigenvalues are exactly 0.  The eigenproblem is solved
//       by cyclic Jacobi with a fixed number of sweeps, which needs no gap (an exactly zero off-diagonal element is skipped).
// Every frame is a pure function of its window: no atomics, no workspace, no reduction across lanes, so the result is bit-identical from
// run to run, from stream to stream and between a clip and a longer clip wherever the windows coincide.  Contraction into fused
// multiply-adds is off for the whole file, so the one-launch route and the two-step route (F stored, then smoothed) round alike.
//
// Features, one lane per output element: y[t, c] = (x[s(t - pad)] + ... + x[s(t + pad)]) * (1 / kernel_size) in fp32, summed from the
// earliest frame on, with the reference's padding s(u) = -1 - u in front and 2 T - 1 - u behind.
#include "r3d_common.h"

#pragma clang fp contract(off)

namespace r3d {
namespace clip {

constexpr int CAMERA_THREADS = 64;             // one wave per block: a clip's few hundred lanes spread over the CUs
constexpr int FEATURE_THREADS = 256;
constexpr int MAX_KERNEL = 255;                // kernel_size of either smoothing
constexpr int SWEEPS = 8;                      // cyclic Jacobi on a symmetric 4 x 4 in fp64 is converged after 5
constexpr int ROW = 25;                        // a camera row: c2w [4, 4] and intrinsics [3, 3]

// a 3 x 3 rotation (row-major) to the unit quaternion (x, y, z, w), by the largest component
__host__ __device__ inline void mat_to_quat(const double* m, double* q)
{
    const double tr = m[0] + m[4] + m[8];
    if (tr >= m[0] && tr >= m[4] && tr >= m[8]) {
        q[0] = m[7] - m[5]; q[1] = m[2] - m[6]; q[2] = m[3] - m[1]; q[3] = 1.0 + tr;
    } else if (m[0] >= m[4] && m[0] >= m[8]) {
        q[0] = 1.0 - tr + 2.0 * m[0]; q[1] = m[3] + m[1]; q[2] = m[6] + m[2]; q[3] = m[7] - m[5];
    } else if (m[4] >= m[8]) {
        q[0] = m[1] + m[3]; q[1] = 1.0 - tr + 2.0 * m[4]; q[2] = m[7] + m[5]; q[3] = m[2] - m[6];
    } else {
        q[0] = m[2] + m[6]; q[1] = m[5] + m[7]; q[2] = 1.0 - tr + 2.0 * m[8]; q[3] = m[3] - m[1];
    }
    const double s = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    q[0] *= s; q[1] *= s; q[2] *= s; q[3] *= s;
}

// a quaternion (x, y, z, w) of any length but 0 to its rotation
__host__ __device__ inline void quat_to_mat(const double* q, double* m)
{
    const double s = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double x = q[0] * s, y = q[1] * s, z = q[2] * s, w = q[3] * s;
    m[0] = 1.0 - 2.0 * (y * y + z * z); m[1] = 2.0 * (x * y - z * w);       m[2] = 2.0 * (x * z + y * w);
    m[3] = 2.0 * (x * y + z * w);       m[4] = 1.0 - 2.0 * (x * x + z * z); m[5] = 2.0 * (y * z - x * w);
    m[6] = 2.0 * (x * z - y * w);       m[7] = 2.0 * (y * z + x * w);       m[8] = 1.0 - 2.0 * (x * x + y * y);
}

// one Jacobi rotation in the (P, Q) plane of the symmetric a (kept in full), accumulated into the columns of v
template <int P, int Q>
__host__ __device__ inline void jacobi_rotate(double (&a)[4][4], double (&v)[4][4])
{
    const double apq = a[P][Q];
    if (apq == 0.0) return;
    const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
    const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));          // theta^2 = inf gives t = 0
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double p = a[k][P], q = a[k][Q];
        a[k][P] = c * p - s * q; a[k][Q] = s * p + c * q;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double p = a[P][k], q = a[Q][k];
        a[P][k] = c * p - s * q; a[Q][k] = s * p + c * q;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double p = v[k][P], q = v[k][Q];
        v[k][P] = c * p - s * q; v[k][Q] = s * p + c * q;
    }
}

// the eigenvector of the largest eigenvalue of the symmetric a (destroyed)
__host__ __device__ inline void top_eigenvector(double (&a)[4][4], double* q)
{
    double v[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) v[r][c] = r == c ? 1.0 : 0.0;
    for (int sweep = 0; sweep < SWEEPS; ++sweep) {
        jacobi_rotate<0, 1>(a, v); jacobi_rotate<0, 2>(a, v); jacobi_rotate<0, 3>(a, v);
        jacobi_rotate<1, 2>(a, v); jacobi_rotate<1, 3>(a, v); jacobi_rotate<2, 3>(a, v);
    }
    double lam = a[0][0];
    q[0] = v[0][0]; q[1] = v[1][0]; q[2] = v[2][0]; q[3] = v[3][0];
#pragma unroll
    for (int k = 1; k < 4; ++k)
        if (a[k][k] > lam) { lam = a[k][k]; q[0] = v[0][k]; q[1] = v[1][k]; q[2] = v[2][k]; q[3] = v[3][k]; }
}

// F(t): f[0 .. 9) the rotation block, f[9 .. 12) the position
__host__ __device__ inline void frame_camera(const float* euler, const float* trans, int t, double radius, float* f)
{
    const double ex = euler[(size_t)t * 3], ey = euler[(size_t)t * 3 + 1], ez = euler[(size_t)t * 3 + 2];
    const double tx = trans[(size_t)t * 3], ty = trans[(size_t)t * 3 + 1], tz = (double)trans[(size_t)t * 3 + 2] + -10.0;
    const double sx = sin(ex), cx = cos(ex), sy = sin(ey), cy = cos(ey), sz = sin(ez), cz = cos(ez);
    double m[9];                                  // M = Rz Ry Rx
    m[0] = cz * cy; m[1] = cz * sy * sx - sz * cx; m[2] = cz * sy * cx + sz * sx;
    m[3] = sz * cy; m[4] = sz * sy * sx + cz * cx; m[5] = sz * sy * cx - cz * sx;
    m[6] = -sy;     m[7] = cy * sx;                m[8] = cy * cx;
    double b[9], c[3];                            // R = M^T; block R diag(1, -1, -1); position -R t 0.27 + offset
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        b[3 * i] = m[i]; b[3 * i + 1] = -m[3 + i]; b[3 * i + 2] = -m[6 + i];
        c[i] = -(m[i] * tx + m[3 + i] * ty + m[6 + i] * tz) * 0.27;
    }
    c[1] += 0.006; c[2] += 0.161;
    if (radius > 0.0) {
        const double len = sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
        c[0] = c[0] / len * radius; c[1] = c[1] / len * radius; c[2] = c[2] / len * radius;
    }
    double q[4], r[9];
    mat_to_quat(b, q);
    quat_to_mat(q, r);
#pragma unroll
    for (int i = 0; i < 9; ++i) f[i] = (float)r[i];
    f[9] = (float)c[0]; f[10] = (float)c[1]; f[11] = (float)c[2];
}

// out(i) of the frames load(j, f) yields
template <class Load>
__host__ __device__ inline void smooth_frame(int i, int T, int K, Load load, float* out)
{
    const int j0 = i - K > 0 ? i - K : 0, j1 = i + K + 1 < T ? i + K + 1 : T;          // K <= MAX_KERNEL / 2: no overflow
    if (j1 - j0 == 1) { load(i, out); return; }
    double a[4][4], pos[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) a[r][c] = 0.0;
    for (int j = j0; j < j1; ++j) {
        float f[12];
        load(j, f);
        double m[9], q[4];
#pragma unroll
        for (int k = 0; k < 9; ++k) m[k] = (double)f[k];
        mat_to_quat(m, q);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = r; c < 4; ++c) a[r][c] += q[r] * q[c];
        pos[0] += (double)f[9]; pos[1] += (double)f[10]; pos[2] += (double)f[11];
    }
#pragma unroll
    for (int r = 1; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < r; ++c) a[r][c] = a[c][r];
    double q[4], m[9];
    top_eigenvector(a, q);
    quat_to_mat(q, m);
    const double n = (double)(j1 - j0);
#pragma unroll
    for (int k = 0; k < 9; ++k) out[k] = (float)m[k];
    out[9] = (float)(pos[0] / n); out[10] = (float)(pos[1] / n); out[11] = (float)(pos[2] / n);
}

__global__ void __launch_bounds__(CAMERA_THREADS) clip_camera_kernel(const float* __restrict__ euler, const float* __restrict__ trans, int T,
                                                                     int K, double radius, float* __restrict__ camera)
{
    const int i = (int)blockIdx.x * CAMERA_THREADS + (int)threadIdx.x;
    if (i >= T) return;
    float f[12];
    smooth_frame(i, T, K, [=](int j, float* o) { frame_camera(euler, trans, j, radius, o); }, f);
    float* o = camera + (size_t)i * ROW;
    const float fx = (float)(2985.29 / 700.0);
    o[0] = f[0]; o[1] = f[1]; o[2] = f[2]; o[3] = f[9];
    o[4] = f[3]; o[5] = f[4]; o[6] = f[5]; o[7] = f[10];
    o[8] = f[6]; o[9] = f[7]; o[10] = f[8]; o[11] = f[11];
    o[12] = 0.0f; o[13] = 0.0f; o[14] = 0.0f; o[15] = 1.0f;
    o[16] = fx; o[17] = 0.0f; o[18] = 0.5f;
    o[19] = 0.0f; o[20] = fx; o[21] = 0.5f;
    o[22] = 0.0f; o[23] = 0.0f; o[24] = 1.0f;
}

__global__ void __launch_bounds__(CAMERA_THREADS) camera_smooth_kernel(const float* __restrict__ in, int stride, int T, int K,
                                                                       float* __restrict__ out)
{
    const int i = (int)blockIdx.x * CAMERA_THREADS + (int)threadIdx.x;
    if (i >= T) return;
    float f[12];
    smooth_frame(i, T, K, [=](int j, float* o) {
        const float* p = in + (size_t)j * stride;
        o[0] = p[0]; o[1] = p[1]; o[2] = p[2]; o[3] = p[4]; o[4] = p[5]; o[5] = p[6]; o[6] = p[8]; o[7] = p[9]; o[8] = p[10];
        o[9] = p[3]; o[10] = p[7]; o[11] = p[11];
    }, f);
    const float* p = in + (size_t)i * stride;
    float* o = out + (size_t)i * stride;
    o[0] = f[0]; o[1] = f[1]; o[2] = f[2]; o[3] = f[9];
    o[4] = f[3]; o[5] = f[4]; o[6] = f[5]; o[7] = f[10];
    o[8] = f[6]; o[9] = f[7]; o[10] = f[8]; o[11] = f[11];
    for (int k = 12; k < stride; ++k) o[k] = p[k];          // the bottom row and the intrinsics are the input's
}

// Cout = C, or C + C / g with a +0.0f after every g values
__global__ void __launch_bounds__(FEATURE_THREADS) smooth_features_kernel(const float* __restrict__ x, int T, int C, int ks, int g, int Cout,
                                                                          float* __restrict__ y)
{
    const long long e = (long long)blockIdx.x * FEATURE_THREADS + (long long)threadIdx.x;
    if (e >= (long long)T * Cout) return;
    const int t = (int)(e / Cout), co = (int)(e - (long long)t * Cout);
    int c = co;
    if (g > 0) {
        const int grp = co / (g + 1), r = co - grp * (g + 1);
        if (r == g) { y[e] = 0.0f; return; }
        c = grp * g + r;
    }
    const int pad = (ks - 1) / 2;
    float s = 0.0f;
    for (int k = 0; k < ks; ++k) {
        int u = t - pad + k;                      // pad <= T: one reflection lands inside
        u = u < 0 ? -1 - u : (u >= T ? 2 * T - 1 - u : u);
        const float v = x[(size_t)u * C + c];
        s = k == 0 ? v : s + v;
    }
    y[e] = s * (1.0f / (float)ks);
}

static bool window_ok(const char* what, int T, int kernel_size)
{
    if (T < 1) { set_error("%s: T = %d must be positive", what, T); return false; }
    if (kernel_size < 1 || kernel_size > MAX_KERNEL) { set_error("%s: kernel_size = %d outside 1 .. %d", what, kernel_size, MAX_KERNEL); return false; }
    return true;
}

}  // namespace clip
}  // namespace r3d

using namespace r3d;

extern "C" int r3d_clip_camera(const float* euler, const float* trans, int T, int kernel_size, double radius, float* camera,
                               r3d_stream_t stream)
{
    const char* what = "clip_camera";
    if (!euler || !trans || !camera) { set_error("%s: NULL pointer", what); return R3D_ERR_INVALID_ARG; }
    if (!clip::window_ok(what, T, kernel_size)) return R3D_ERR_INVALID_ARG;
    if (!below_2_31(what, "25 T", (double)T * clip::ROW, "elements")) return R3D_ERR_INVALID_ARG;
    if (!(radius >= 0.0) || radius - radius != 0.0) { set_error("%s: radius = %g must be finite and not negative (0: no rescaling)", what, radius); return R3D_ERR_INVALID_ARG; }
    const size_t nout = (size_t)T * clip::ROW, nin = (size_t)T * 3;
    if (overlap(camera, nout, euler, nin) || overlap(camera, nout, trans, nin)) { set_error("%s: the output overlaps an input", what); return R3D_ERR_INVALID_ARG; }
    ProfScope ps(R3D_PROF_MISC, (hipStream_t)stream);
    const unsigned blocks = (unsigned)((T + clip::CAMERA_THREADS - 1) / clip::CAMERA_THREADS);
    hipLaunchKernelGGL(clip::clip_camera_kernel, dim3(blocks), dim3(clip::CAMERA_THREADS), 0, (hipStream_t)stream, euler, trans, T, kernel_size / 2,
                       radius, camera);
    return check_launch(what);
}

extern "C" int r3d_camera_smooth(const float* camera_in, int row_stride, int T, int kernel_size, float* camera_out, r3d_stream_t stream)
{
    const char* what = "camera_smooth";
    if (!camera_in || !camera_out) { set_error("%s: NULL pointer", what); return R3D_ERR_INVALID_ARG; }
    if (row_stride != 16 && row_stride != clip::ROW) { set_error("%s: row_stride = %d, a camera row has 16 or 25 values", what, row_stride); return R3D_ERR_INVALID_ARG; }
    if (!clip::window_ok(what, T, kernel_size)) return R3D_ERR_INVALID_ARG;
    if (!below_2_31(what, "T row_stride", (double)T * row_stride, "elements")) return R3D_ERR_INVALID_ARG;
    const size_t n = (size_t)T * row_stride;
    if (overlap(camera_out, n, camera_in, n)) { set_error("%s: the output overlaps the input (a frame reads its neighbours)", what); return R3D_ERR_INVALID_ARG; }
    ProfScope ps(R3D_PROF_MISC, (hipStream_t)stream);
    const unsigned blocks = (unsigned)((T + clip::CAMERA_THREADS - 1) / clip::CAMERA_THREADS);
    hipLaunchKernelGGL(clip::camera_smooth_kernel, dim3(blocks), dim3(clip::CAMERA_THREADS), 0, (hipStream_t)stream, camera_in, row_stride, T,
                       kernel_size / 2, camera_out);
    return check_launch(what);
}

extern "C" int r3d_smooth_features(const float* x, int T, int C, int kernel_size, int zero_columns_every, float* y, r3d_stream_t stream)
{
    const char* what = "smooth_features";
    if (!x || !y) { set_error("%s: NULL pointer", what); return R3D_ERR_INVALID_ARG; }
    if (!clip::window_ok(what, T, kernel_size)) return R3D_ERR_INVALID_ARG;
    if (C < 1) { set_error("%s: C = %d must be positive", what, C); return R3D_ERR_INVALID_ARG; }
    if (kernel_size % 2 == 0) { set_error("%s: kernel_size = %d is even (the reference's padding fits odd sizes only)", what, kernel_size); return R3D_ERR_INVALID_ARG; }
    if (T < (kernel_size - 1) / 2) { set_error("%s: T = %d is below the padding (kernel_size - 1) / 2 = %d", what, T, (kernel_size - 1) / 2); return R3D_ERR_INVALID_ARG; }
    const int g = zero_columns_every;
    if (g < 0 || (g > 0 && C % g != 0)) { set_error("%s: zero_columns_every = %d must be 0 or a divisor of C = %d", what, g, C); return R3D_ERR_INVALID_ARG; }
    const long long Cout = g > 0 ? (long long)C + C / g : (long long)C;
    if (!below_2_31(what, "T C", (double)T * (double)Cout, "elements with the zero columns")) return R3D_ERR_INVALID_ARG;
    const size_t nin = (size_t)T * C, nout = (size_t)T * (size_t)Cout;
    if (overlap(y, nout, x, nin)) { set_error("%s: the output overlaps the input (a frame reads its neighbours)", what); return R3D_ERR_INVALID_ARG; }
    ProfScope ps(R3D_PROF_MISC, (hipStream_t)stream);
    const unsigned blocks = (unsigned)((nout + clip::FEATURE_THREADS - 1) / clip::FEATURE_THREADS);
    hipLaunchKernelGGL(clip::smooth_features_kernel, dim3(blocks), dim3(clip::FEATURE_THREADS), 0, (hipStream_t)stream, x, T, C, kernel_size, g,
                       (int)Cout, y);
    return check_launch(what);
}
