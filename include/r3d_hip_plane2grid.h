/*
 * r3d_hip_plane2grid.h -- module header of r3d_hip.h (C ABI of libr3d_hip.so): Plane2GridModule, the Conv3d residual blocks that turn the
 * canonical backbone's planes into tri-grids (triplane_feature_type trigrid_v2).  It includes r3d_hip.h (r3d_stream_t, the status codes,
 * r3d_last_error); r3d_hip.h does not include it back.  The Python binding table of this header is real3dportrait_amd/_lib.py
 * MODULE_SIGNATURES["r3d_hip_plane2grid.h"].  Functions are added without a new r3d_version().
 */
#ifndef R3D_HIP_PLANE2GRID_H
#define R3D_HIP_PLANE2GRID_H

#include "r3d_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* --- Plane2GridModule (modules/real3d/img2plane_baseline.py:32-77): per SameBlock3d  GroupNorm(4, C), ReLU, Conv3d(C, C, 3, padding=1,
 * padding_mode='replicate'), GroupNorm, ReLU, Conv3d, x + alpha out ---------------------------------------------------------------------------
 * real3dportrait_amd/plane2grid.py drives these; tests/plane2grid_ref64.py is the fp64 restatement.  Same conventions as
 * r3d_hip.h: borrowed device pointers, contiguous fp32, volumes channel-last [B, D, H, W, C], weights [Cout, 3, 3, 3, Cin], `stream` a
 * hipStream_t, 0 or a negative r3d_status with the message from r3d_last_error().  No floating-point atomics, no grid barrier, no
 * allocation, no host synchronisation; run to run bit-identical, and a sample's result does not depend on B.  Inputs are never written.
 * Every refusal below is R3D_ERR_INVALID_ARG before any launch. */

/* Bytes of the workspace r3d_p2g_groupnorm_stats needs: B ceil(D H W / 1024) groups pairs of doubles.  0 for an argument it refuses. */
size_t r3d_p2g_groupnorm_stats_workspace_bytes(int B, int D, int H, int W, int C, int groups);

/* nn.GroupNorm(groups, C, eps) as a conv prologue: for x_cl [B, D, H, W, C]
 *   scale[b, c] = gamma[c] rstd(b, g)      shift[b, c] = beta[c] - mean(b, g) scale[b, c]      g = c / (C / groups)
 * so that GroupNorm(x) = scale x + shift.  mean and the biased variance E[x^2] - mean^2 cover the C / groups D H W values of (b, g); they
 * are formed in fp64 (every square exact), the variance is clamped at 0 before + eps, rstd = 1 / sqrt(var + eps) in fp64, scale is rounded
 * to fp32 and shift is formed in fp64 from the rounded scale.  Two passes: each block sums 1024 rows of one sample in a fixed order into
 * the workspace, then each (b, c) adds its group's partial sums in their order; the order depends on (D, H, W, C, groups) alone.
 * Refused: a NULL pointer; B, D, H, W, C or groups below 1; C above 1024 or not a multiple of 4 and of groups; B above 65535; eps negative
 * or not finite; B D H W C >= 2^31; x_cl or the workspace not 16-byte aligned; a workspace below ..._workspace_bytes; scale, shift or the
 * workspace overlapping each other or an input. */
int r3d_p2g_groupnorm_stats(const float* x_cl, int B, int D, int H, int W, int C, int groups, const float* gamma, const float* beta, float eps,
                            float* scale, float* shift, void* workspace, size_t workspace_bytes, r3d_stream_t stream);

/* nn.Conv3d(Cin, Cout, 3, 1, 1, padding_mode='replicate') on x_cl [B, D, H, W, Cin], exact fp32 on v_mfma_f32_16x16x4_f32.  Tap
 * (kz, ky, kx) of output (b, z, y, x) is
 *   a = x_cl[b, clamp(z - 1 + kz, 0, D - 1), clamp(y - 1 + ky, 0, H - 1), clamp(x - 1 + kx, 0, W - 1), :]
 *   a = max(scale[b, c] a + shift[b, c], 0)      scale, shift [B, Cin], both or neither (NULL: a as stored); a NaN stays a NaN
 * which is the replicate padding of the activated tensor.  The epilogue is sum + bias[n] (bias NULL: none) + residual[b, z, y, x, n]
 * (residual [B, D, H, W, Cout] or NULL; it may be y_cl itself), written to y_cl [B, D, H, W, Cout] and / or y_ncdhw [B, Cout, D, H, W]
 * (either may be NULL, not both).
 * Refused: NULL x_cl or w, or both outputs; one of scale, shift without the other; Cin not a multiple of 4;
 * B D H W max(Cin, Cout) >= 2^31; B, D, H, W, Cin or Cout below 1; Cin or Cout above 4096; D above 1024; x_cl, w, scale or shift not 16-byte
 * aligned; an output overlapping x_cl, w, bias, scale or shift; an output overlapping residual without y_cl being it; y_cl overlapping
 * y_ncdhw. */
int r3d_p2g_conv3d(const float* x_cl, int B, int D, int H, int W, int Cin, const float* scale, const float* shift, const float* w,
                   const float* bias, int Cout, const float* residual, float* y_cl, float* y_ncdhw, r3d_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* R3D_HIP_PLANE2GRID_H */
