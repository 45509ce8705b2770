/*
 * r3d_hip_clip.h -- companion header of r3d_hip.h (C ABI of libr3d_hip.so): the per-clip conditions.  r3d_hip.h includes it; it can also
 * be included on its own.  The Python binding table of this header is real3dportrait_amd/_lib.py SIGNATURES.
 */
#ifndef R3D_HIP_CLIP_H
#define R3D_HIP_CLIP_H

#include "r3d_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* --- per-clip conditions: the camera trajectory and the smoothed key points, inference (added under ABI 0.8.0) ----------------------------
 * What prepare_batch_from_inp and forward_secc2video compute once per clip between the fitted coefficients and the frame loop, on the
 * device (tests/clip_conditions_ref64.py is the fp64 restatement).  Same conventions as r3d_hip.h: borrowed
 * device pointers, contiguous fp32, `stream` a hipStream_t, 0 or a negative r3d_status, the message from r3d_last_error().
 *
 * r3d_clip_camera is inference/real3d_infer.py:312-319 in one launch: get_eg3d_convention_camera_pose_intrinsic
 * (data_gen/eg3d/convert_to_eg3d_convention.py:42-146) and smooth_camera_sequence (inference/infer_utils.py:40-69).  euler [T, 3] in
 * radians, trans [T, 3]; camera [T, 25]: c2w [4, 4] row-major, then the intrinsics [3, 3].
 *   The frame's own camera F(t), with R = (Rz Ry Rx)^T of compute_rotation (deep_3drecon/deep_3drecon_models/bfm.py:204-238): rotation
 *   block R diag(1, -1, -1); position -R (trans + (0, 0, -10)) 0.27 + (0, 0.006, 0.161), rescaled to length `radius` when radius > 0
 *   (_fix_pose_orig's 2.7 of convention_c2w; 0 gives the c2w inference uses; a position of length 0 then has no direction and comes
 *   back NaN); the block goes to a unit quaternion and back; the twelve numbers are rounded to fp32, as the reference's frame camera is
 *   fp32-valued.  Bottom row (0, 0, 0, 1); intrinsics (2985.29 / 700, 0, 0.5, 0, 2985.29 / 700, 0.5, 0, 0, 1).
 *   Frame i of the output, over the window [max(0, i - K), min(T, i + K + 1)), K = kernel_size / 2: the mean of the window's positions
 *   and the chordal L2 mean of its rotations (each to a unit quaternion q, A = sum q q^T, the eigenvector of A's largest eigenvalue,
 *   back to a matrix: scipy's Rotation.mean), rounded to fp32 once.  A window of one frame, kernel_size = 1 or T = 1, returns F itself.
 *   All arithmetic between the fp32 loads and the fp32 roundings is fp64.  The matrix-to-quaternion step branches on the largest
 *   component (at zero pose the block is diag(1, -1, -1), trace -1); the eigenproblem is solved by cyclic Jacobi with a fixed number of
 *   sweeps, so windows of identical rotations (three eigenvalues exactly 0) are ordinary input.
 * r3d_camera_smooth is smooth_camera_sequence alone on camera_in [T, row_stride], row_stride 16 or 25: the same window rule with F =
 * the input's rows; the bottom row and the columns from 16 on are copied.  camera_out must not overlap camera_in (a frame reads its
 * neighbours).  r3d_clip_camera(kernel_size) is bit-identical to r3d_clip_camera(1) followed by r3d_camera_smooth(kernel_size).
 *   Difference from the reference: the 3 x 3 blocks must be proper rotations.  Where scipy refuses a window (a block with a determinant
 *   <= 0) the reference copies the previous frame's rotation; this function does not, and the result of such a window is undefined
 *   (finite or NaN, nothing is accessed out of bounds).
 * r3d_smooth_features is smooth_features_xd (inference/infer_utils.py:71-101) on x [T, C], a tensor of any rank with everything but the
 * frames flattened: pad = (kernel_size - 1) / 2 frames in front, x[pad - 1], ..., x[0], and behind, x[T - 1], ..., x[T - pad], then
 * y[t] = (the sum of kernel_size consecutive frames, added in fp32 from the earliest on) * (1.0f / kernel_size).
 *   zero_columns_every = g > 0 (a divisor of C): y is [T, C + C / g], every g values followed by one +0.0f; g = 2 on key points
 *   [T, 68 x 2] gives the [T, 68, 3] of real3d_infer.py:481-482 for the whole clip.  g = 0: y [T, C].  kernel_size = 1 copies.
 * Each output is a pure function of its window: no atomics, no workspace, no allocation, no host synchronisation; run to run and stream
 * to stream bit-identical, and a frame whose window lies inside two clips alike is bit-identical in both.  Inputs are never written.
 * Refused before any launch with R3D_ERR_INVALID_ARG: a NULL pointer; T < 1; kernel_size < 1 or > 255; 25 T, T row_stride or
 * T (C + C / g) >= 2^31; an output that overlaps an input; radius negative or not finite; row_stride other than 16 or 25; C < 1; an
 * even kernel_size or T < pad for r3d_smooth_features (the reference fails with a reshape error there); g < 0 or not a divisor of C. */
int r3d_clip_camera(const float* euler, const float* trans, int T, int kernel_size, double radius, float* camera, r3d_stream_t stream);
int r3d_camera_smooth(const float* camera_in, int row_stride, int T, int kernel_size, float* camera_out, r3d_stream_t stream);
int r3d_smooth_features(const float* x, int T, int C, int kernel_size, int zero_columns_every, float* y, r3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* R3D_HIP_CLIP_H */
