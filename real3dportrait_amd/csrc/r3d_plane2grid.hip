// Plane2GridModule (modules/real3d/img2plane_baseline.py:32-77): the SameBlock3d residual blocks that make tri-grids of the canonical
// backbone's planes, inference only, exact fp32 (include/r3d_hip_plane2grid.h).  Kernels:
//   p2g_conv<WM, WN, TM, TN>   nn.Conv3d(3, padding=1, padding_mode='replicate') behind GroupNorm + ReLU as a per-sample prologue on
//                              v_mfma_f32_16x16x4_f32: the shared tile of r3d_torso_conv.h with its RP flag (3-D body, extended epilogue:
//                              + bias + residual, channel-last and / or NCDHW), through the tile table and argument check of
//                              r3d_torso_launch.h.  16-byte loads only.
//   p2g_stats_partial          per (1024 rows, sample): fp64 sum and sum of squares of every group, in a fixed order.
//   p2g_stats_finalize         per (sample, channel): the group's partial sums added in their order -> scale, shift.
#include "r3d_common.h"
#include "r3d_torso_launch.h"
#include "../../include/r3d_hip_plane2grid.h"
#include <math.h>

namespace r3d {
namespace plane2grid {

using tconv::ConvArgs;

template <int WM, int WN, int TM, int TN>
__global__ void __launch_bounds__(256) p2g_conv(ConvArgs g) { tconv::conv_tile<tconv::F32, true, true, WM, WN, TM, TN, true, false, true>(g); }

// this unit's kernel family for tlaunch::dispatch: the 3-D body with replicate padding and the per-sample prologue, fp32, 16-byte loads
struct Family {
    static constexpr bool tile64x16 = true;
    template <int PREC, bool VEC, int WM, int WN, int TM, int TN>
    static void (*kernel())(ConvArgs)
    {
        static_assert(PREC == tconv::F32 && VEC, "r3d_p2g_conv3d has one tier and one loader");
        return p2g_conv<WM, WN, TM, TN>;
    }
};

// ---- GroupNorm statistics ---------------------------------------------------------------------------------------------------------------
// A block owns GN_ROWS rows (positions) of one sample, all C channels of each: 256 lanes as (row phase p, channel quad cq), P = 256 / (C / 4)
// phases, lane (p, cq) reads rows p, p + P, ... of its four channels with 16-byte loads (a wave reads whole rows: coalesced) and keeps four
// fp64 sums and four fp64 sums of squares.  Then channel c adds its P phase sums in phase order, and group g its C / groups channel sums in
// channel order: ws[((b nchunk + chunk) groups + g) 2 + {0, 1}].  Nothing but (D H W, C, groups) decides the order.
constexpr int GN_ROWS = 1024, GN_T = 256, GN_CMAX = 1024;

__global__ void __launch_bounds__(GN_T) p2g_stats_partial(const float* x, int S, int C, int groups, double* ws)
{
    __shared__ double part[GN_T][8];
    __shared__ double chan[GN_CMAX][2];
    const int t = threadIdx.x, C4 = C >> 2, P = GN_T / C4, p = t / C4, cq = t - p * C4;
    const int chunk = blockIdx.x, b = blockIdx.y, row0 = chunk * GN_ROWS, row1 = min(row0 + GN_ROWS, S);
    double s[4] = {0.0, 0.0, 0.0, 0.0}, q[4] = {0.0, 0.0, 0.0, 0.0};
    auto add = [&](const float4& v) {
        const double a0 = v.x, a1 = v.y, a2 = v.z, a3 = v.w;
        s[0] += a0; s[1] += a1; s[2] += a2; s[3] += a3;
        q[0] += a0 * a0; q[1] += a1 * a1; q[2] += a2 * a2; q[3] += a3 * a3;
    };
    if (p < P) {
        const float* px = x + (size_t)b * S * C + 4 * cq;
        int r = row0 + p;
        for (; r + 3 * P < row1; r += 4 * P) {          // four loads in flight; added in row order
            const float4 v0 = *reinterpret_cast<const float4*>(px + (size_t)r * C), v1 = *reinterpret_cast<const float4*>(px + (size_t)(r + P) * C);
            const float4 v2 = *reinterpret_cast<const float4*>(px + (size_t)(r + 2 * P) * C), v3 = *reinterpret_cast<const float4*>(px + (size_t)(r + 3 * P) * C);
            add(v0); add(v1); add(v2); add(v3);
        }
        for (; r < row1; r += P) add(*reinterpret_cast<const float4*>(px + (size_t)r * C));
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) { part[t][k] = s[k]; part[t][4 + k] = q[k]; }
    __syncthreads();
    for (int c = t; c < C; c += GN_T) {
        double cs = 0.0, cqq = 0.0;
        for (int ph = 0; ph < P; ++ph) { cs += part[ph * C4 + (c >> 2)][c & 3]; cqq += part[ph * C4 + (c >> 2)][4 + (c & 3)]; }
        chan[c][0] = cs; chan[c][1] = cqq;
    }
    __syncthreads();
    const int Cg = C / groups;
    for (int g = t; g < groups; g += GN_T) {
        double gs = 0.0, gq = 0.0;
        for (int c = g * Cg; c < (g + 1) * Cg; ++c) { gs += chan[c][0]; gq += chan[c][1]; }
        double* o = ws + (((size_t)b * gridDim.x + chunk) * groups + g) * 2;
        o[0] = gs; o[1] = gq;
    }
}

__global__ void __launch_bounds__(256) p2g_stats_finalize(const double* ws, int B, int S, int C, int groups, int nchunk, const float* gamma,
                                                          const float* beta, float eps, float* scale, float* shift)
{
    const int i = blockIdx.x * 256 + threadIdx.x;          // over [B, C]
    if (i >= B * C) return;
    const int b = i / C, c = i - b * C, Cg = C / groups, g = c / Cg;
    double s = 0.0, q = 0.0;
    for (int k = 0; k < nchunk; ++k) {
        const double* o = ws + (((size_t)b * nchunk + k) * groups + g) * 2;
        s += o[0]; q += o[1];
    }
    const double n = (double)Cg * (double)S, mean = s / n;
    double var = q / n - mean * mean;
    if (!(var > 0.0)) var = var != var ? var : 0.0;          // clamped at 0 before + eps; a NaN stays
    const double rstd = 1.0 / sqrt(var + (double)eps);
    const float sc = (float)((double)gamma[c] * rstd);
    scale[i] = sc;
    shift[i] = (float)((double)beta[c] - mean * (double)sc);
}

static int stats_chunks(int D, int H, int W) { return (int)(((long long)D * H * W + GN_ROWS - 1) / GN_ROWS); }

static bool stats_shape_ok(int B, int D, int H, int W, int C, int groups)
{
    return B > 0 && D > 0 && H > 0 && W > 0 && C > 0 && groups > 0 && C <= GN_CMAX && C % 4 == 0 && C % groups == 0 && B <= 65535 &&
           (double)B * D * H * W * C < 2147483648.0;
}

}  // namespace plane2grid
}  // namespace r3d

using namespace r3d;
using namespace r3d::plane2grid;

extern "C" size_t r3d_p2g_groupnorm_stats_workspace_bytes(int B, int D, int H, int W, int C, int groups)
{
    if (!stats_shape_ok(B, D, H, W, C, groups)) return 0;
    return (size_t)B * stats_chunks(D, H, W) * groups * 2 * sizeof(double);
}

extern "C" int r3d_p2g_groupnorm_stats(const float* x_cl, int B, int D, int H, int W, int C, int groups, const float* gamma, const float* beta,
                                       float eps, float* scale, float* shift, void* workspace, size_t workspace_bytes, r3d_stream_t stream)
{
    const char* what = "p2g_groupnorm_stats";
    if (!x_cl || !gamma || !beta || !scale || !shift) { set_error("%s: NULL pointer", what); return R3D_ERR_INVALID_ARG; }
    if (B <= 0 || D <= 0 || H <= 0 || W <= 0 || C <= 0 || groups <= 0 || B > 65535)
        { set_error("%s: bad argument (B = %d in 1 .. 65535, D = %d, H = %d, W = %d, C = %d, groups = %d must be > 0)", what, B, D, H, W, C, groups);
          return R3D_ERR_INVALID_ARG; }
    if (C > GN_CMAX || C % 4 != 0 || C % groups != 0)
        { set_error("%s: C = %d is not a multiple of 4 and of groups = %d, at most %d", what, C, groups, GN_CMAX); return R3D_ERR_INVALID_ARG; }
    if (!(eps >= 0.0f) || isinf(eps)) { set_error("%s: eps %g is negative or not finite", what, (double)eps); return R3D_ERR_INVALID_ARG; }
    if (!below_2_31(what, "B D H W C", (double)B * D * H * W * C, "elements")) return R3D_ERR_INVALID_ARG;
    if (!aligned16(x_cl)) { set_error("%s: x_cl is not 16-byte aligned", what); return R3D_ERR_INVALID_ARG; }
    const size_t need = r3d_p2g_groupnorm_stats_workspace_bytes(B, D, H, W, C, groups);
    if (!workspace_ok(what, workspace, workspace_bytes, need, 16, "r3d_p2g_groupnorm_stats_workspace_bytes")) return R3D_ERR_INVALID_ARG;
    const int S = D * H * W, nchunk = stats_chunks(D, H, W);
    const Span spans[] = {writes(scale, (size_t)B * C), writes(shift, (size_t)B * C), writes((const char*)workspace, need),
                          reads(x_cl, (size_t)B * S * C), reads(gamma, (size_t)C), reads(beta, (size_t)C)};
    if (clash(spans)) { set_error("%s: scale, shift or the workspace overlaps another array of the call", what); return R3D_ERR_INVALID_ARG; }
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(p2g_stats_partial, dim3(nchunk, B), dim3(GN_T), 0, st, x_cl, S, C, groups, (double*)workspace);
    hipLaunchKernelGGL(p2g_stats_finalize, dim3((B * C + 255) / 256), dim3(256), 0, st, (const double*)workspace, B, S, C, groups, nchunk, gamma, beta,
                       eps, scale, shift);
    return check_launch(what);
}

extern "C" int r3d_p2g_conv3d(const float* x_cl, int B, int D, int H, int W, int Cin, const float* scale, const float* shift, const float* w,
                              const float* bias, int Cout, const float* residual, float* y_cl, float* y_ncdhw, r3d_stream_t stream)
{
    const char* what = "p2g_conv3d";
    tlaunch::ConvCall c = tlaunch::conv_call(x_cl, B, H, W, Cin, w, bias, Cout, 3, 0, 0.0f, y_cl, R3D_TORSO_F32);
    c.D = D; c.volume = true; c.rp = true; c.ps = scale; c.pt = shift; c.res = residual; c.yn = y_ncdhw;
    if (Cin > 0 && Cin % 4 != 0) { set_error("%s: Cin = %d is not a multiple of 4", what, Cin); return R3D_ERR_INVALID_ARG; }
    if (B > 0 && D > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 &&
        !below_2_31(what, "B D H W max(Cin, Cout)", (double)B * D * H * W * (Cin > Cout ? Cin : Cout), "elements")) return R3D_ERR_INVALID_ARG;
    if (int rc = tlaunch::check_conv(what, c)) return rc;
    if (!aligned16(x_cl) || !aligned16(w) || !aligned16(scale) || !aligned16(shift))
        { set_error("%s: x_cl, w, scale or shift is not 16-byte aligned", what); return R3D_ERR_INVALID_ARG; }
    ConvArgs g = {};
    c.fill(g);
    tlaunch::dispatch<Family, tconv::F32, true>(g, (hipStream_t)stream);
    return check_launch(what);
}
