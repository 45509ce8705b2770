/*
 * r3d_hip_fit.h -- companion header of r3d_hip.h (C ABI of libr3d_hip.so): the landmark-driven 3DMM fit.  r3d_hip.h includes it; it can
 * also be included on its own.  The Python binding table of this header is real3dportrait_amd/_lib.py SIGNATURES.
 */
#ifndef R3D_HIP_FIT_H
#define R3D_HIP_FIT_H

#include "r3d_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* --- fit the morphable model to 2-D landmarks: the Adam loops of fit_3dmm_for_a_image / fit_3dmm_for_a_video -----------------------------
 * (data_gen/utils/process_image/fit_3dmm_landmark.py:85-264, data_gen/utils/process_video/fit_3dmm_landmark.py:130-459; DESIGN 4.21;
 * tests/fit_3dmm_ref.py is the restatement with torch autograd and torch.optim.Adam.)  Same conventions as r3d_hip.h: borrowed device
 * pointers, contiguous fp32, `stream` a hipStream_t, 0 or a negative r3d_status, the message from r3d_last_error().  `lambdas` alone is a
 * HOST array, read before the call returns.
 *
 * The loss of T frames, L key points, id [id_rows, Ki] (id_rows 1: one row shared by all frames, its gradient summed over them; id_rows T:
 * a row per frame), exp [T, Ke], euler [T, 3] radians, trans [T, 3]:
 *   shape = key_mean + key_id_base id + key_exp_base exp (rows 3 l + c);  q = M shape + trans, M = Rz Ry Rx (compute_for_landmark_fit,
 *   bfm.py:349-366);  z = camera_distance - q.z;  proj = ((focal q.x + center z) / z, (focal q.y + center z) / z) -- no flip, no division
 *   by the image size;  lan = mean over all T L 2 elements of weights[l] (proj - lms)^2, lms [T, L, 2] in the same 224-pixel frame;
 *   total = lan + lambdas[0] mean(id^2) + lambdas[1] mean(exp^2) + lambdas[2] lap(id) + lambdas[3] lap(exp) + lambdas[4] lap(euler)
 *           + lambdas[5] lap(trans),   lap(x [R, C]) = mean over R C of (x[t] - (x[max(t - 1, 0)] + x[min(t + 1, R - 1)]) / 2)^2
 *   (cal_lap_loss: replicate padding, the kernel (-0.5, 1, -0.5)); lap of a single row is exactly 0.
 * The loss record is 8 floats: lan, mean(id^2), mean(exp^2), lap(id), lap(exp), lap(euler), lap(trans), total.
 *
 * Two kernels, and no others (R3D_FIT_LAUNCHES per evaluation or iteration).  fit_grad: a block owns a slab of whole key points, their
 * rows of the two bases in LDS, and walks a run of frames; per frame the forward, the residual and d loss / d shape are local to a point,
 * and the block writes the slab's partial sums of the gradients of id[t], exp[t], euler[t] (the analytic derivative of Rz Ry Rx), trans[t]
 * and of the loss to workspace [slabs, T, Ki + Ke + 7]; it also snapshots the parameters.  fit_step: sums the partials over the slabs (and
 * over T for a shared id row) in a fixed order, adds the gradients of the mean-square and Laplacian terms from the snapshot, applies
 * torch.optim.Adam's update (betas 0.9 / 0.999, eps 1e-8, both bias corrections from the group's step number, no weight decay) to the
 * active groups, and writes the loss record of the iterate it consumed.  No atomics: results are bit-identical from run to run and from
 * stream to stream.  No cooperative launch, no grid-wide barrier, no flag between blocks: iterations are separated by launch boundaries
 * only.  No allocation and no host synchronisation.
 *
 * r3d_fit_state_bytes: `state` of r3d_fit_landmark_run, floats in this order: id [id_rows, Ki], exp [T, Ke], euler [T, 3], trans [T, 3];
 *   Adam's first moments, laid out as the parameters; the second moments likewise; the loss record (R3D_FIT_LOSS_WORDS).  A fit starts
 *   from a state of zeros (or any parameters with zero moments).
 * r3d_fit_workspace_bytes: the partial sums and the snapshot; 16-byte aligned.  Both sizers return 0 for sizes the entry points refuse.
 * r3d_fit_landmark_grad: one evaluation at the given parameters -> the loss record and the four gradients of `total` (grad_id
 *   [id_rows, Ki], grad_exp [T, Ke], grad_euler, grad_trans [T, 3]).  exp and grad_exp may be NULL when Ke = 0.
 * r3d_fit_landmark_run: n_iter iterations from `state`, 2 n_iter launches.  groups: bit 0 steps id and exp with lr_idexp, bit 1 euler
 *   and trans with lr_frame; a group that is not active keeps its parameters, moments and step count.  Iteration i (from 0) of a group is
 *   Adam step number step0 + i + 1, step0 the number of steps the group's moments have seen (the reference's frame optimiser runs steps
 *   1 .. 200 alone, then 201 .. 400 beside steps 1 .. 200 of the id / exp optimiser).
 * Refused before any launch with R3D_ERR_INVALID_ARG: a NULL pointer (key_exp_base, exp, grad_exp only with Ke > 0); L or T < 1; Ki < 1,
 * Ke < 0, Ki + Ke > 512; id_rows other than 1 or T; a non-finite camera_distance, focal, center, lambda or learning rate; focal <= 0;
 * a learning rate <= 0; step0 < 0; n_iter < 1; groups outside 1 .. 3; an index product of 2^31 or more; the state, the workspace or a
 * gradient overlapping an input or one another.  R3D_ERR_WORKSPACE: a workspace that is NULL, not 16-byte aligned or smaller than
 * r3d_fit_workspace_bytes(L, Ki, Ke, T). */
#define R3D_FIT_LOSS_WORDS 8
#define R3D_FIT_LAUNCHES 2
size_t r3d_fit_workspace_bytes(int L, int Ki, int Ke, int T);
size_t r3d_fit_state_bytes(int Ki, int Ke, int T, int id_rows);
int r3d_fit_landmark_grad(const float* key_mean, const float* key_id_base, const float* key_exp_base, int L, int Ki, int Ke, const float* lms,
                          const float* weights, int T, int id_rows, float camera_distance, float focal, float center, const float* lambdas,
                          const float* id, const float* exp, const float* euler, const float* trans, float* grad_id, float* grad_exp,
                          float* grad_euler, float* grad_trans, float* loss, void* workspace, size_t workspace_bytes, r3d_stream_t stream);
int r3d_fit_landmark_run(const float* key_mean, const float* key_id_base, const float* key_exp_base, int L, int Ki, int Ke, const float* lms,
                         const float* weights, int T, int id_rows, float camera_distance, float focal, float center, const float* lambdas,
                         float lr_idexp, float lr_frame, int step0_idexp, int step0_frame, int n_iter, int groups, float* state,
                         void* workspace, size_t workspace_bytes, r3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* R3D_HIP_FIT_H */
