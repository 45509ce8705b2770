/*
 * r3d_hip_deeplab.h -- feature header of r3d_hip.h (C ABI of libr3d_hip.so): DeepLabV3, the low-resolution encoder of the canonical
 * image-to-plane backbone.  It includes r3d_hip.h (r3d_stream_t, the status codes, r3d_last_error); r3d_hip.h does not include it back.
 * The Python binding table of this header is real3dportrait_amd/_lib.py FEATURE_SIGNATURES["r3d_hip_deeplab.h"].  Functions are added
 * without a new r3d_version().
 */
#ifndef R3D_HIP_DEEPLAB_H
#define R3D_HIP_DEEPLAB_H

#include "r3d_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* --- DeepLabV3 (modules/img2plane/deeplabv3/decoders/my_model.py): a BasicBlock ResNet dilated to output stride 8 (encoders/resnet.py,
 * encoders/_utils.py:40-47), ASPP with rates 12 / 24 / 36 and one 3 x 3 conv (decoders/my_decoder.py) ----------------------------------------
 * real3dportrait_amd/deeplabv3.py drives these four; tests/deeplabv3_ref64.py is the fp64 restatement.  Same conventions as
 * r3d_hip.h: borrowed device pointers, contiguous fp32, activations channel-last [B, H, W, C], weights [Cout, k, k, Cin], `stream` a
 * hipStream_t, 0 or a negative r3d_status with the message from r3d_last_error().  Exact fp32: every product of r3d_dl_conv runs on
 * v_mfma_f32_16x16x4_f32.  No atomics, no workspace, no allocation, no host synchronisation; run to run bit-identical, and a sample's
 * result does not depend on B.  Inputs are never written.  Every refusal below is R3D_ERR_INVALID_ARG before any launch. */

/* nn.Conv2d(Cin, Cout, ksize, stride, padding = pad, dilation, bias=False) with its eval BatchNorm folded into w and bias by the caller:
 * output (oy, ox) sums taps (ky, kx) over x[oy stride - pad + ky dilation, ox stride - pad + kx dilation], zero outside Hin x Win;
 * Ho = (Hin + 2 pad - dilation (ksize - 1) - 1) / stride + 1, Wo likewise, M = B Ho Wo rows.
 *   v = sum + bias[b bias_bstride + n]     bias NULL: none; bias_bstride 0: one [Cout] bias, >= Cout: one per sample
 *   v += residual[m, n]                    residual [M, Cout] or NULL; it may be y itself (then ycs == Cout, yco == 0)
 *   v = max(v, 0) if act == 1              AFTER the residual: BasicBlock's order (a NaN stays a NaN)
 * written to y[m ycs + yco + n]: channels [yco, yco + Cout) of rows of ycs floats (a branch writes its slice of a concatenation).
 * Refused: NULL x, w or y; B, Hin, Win, Cin or Cout below 1; Cin or Cout above 4096; ksize not 1, 3 or 7; stride not 1 or 2; dilation
 * outside 1 .. 64; pad outside 0 .. 65536; Hin or Win above 2^24; act not 0 or 1; Ho or Wo below 1; bias_bstride in 1 .. Cout - 1 or
 * negative; a slice that does not fit ycs; more than 2^31 - 1 rows; y overlapping x, w or bias; y overlapping residual without being it;
 * residual == y with ycs != Cout or yco != 0. */
int r3d_dl_conv(const float* x, int B, int Hin, int Win, int Cin, const float* w, const float* bias, int bias_bstride, int Cout, int ksize,
                int stride, int dilation, int pad, const float* residual, int act, float* y, int ycs, int yco, r3d_stream_t stream);

/* nn.MaxPool2d(3, 2, 1): x [B, H, W, C] -> y [B, (H - 1) / 2 + 1, (W - 1) / 2 + 1, C].  Padding counts as -inf, a NaN in a window gives NaN
 * (as torch does); bit-exact.
 * Refused: a NULL pointer; B, H, W or C below 1; B H W C >= 2^31; y overlapping x. */
int r3d_dl_maxpool(const float* x, int B, int H, int W, int C, float* y, r3d_stream_t stream);

/* nn.AdaptiveAvgPool2d(1): x [B, HW, C] -> y [B, C], the mean over the HW rows.  Each (sample, channel) is 32 strided fp64 partial sums
 * added in a fixed order, rounded to fp32 once.
 * Refused: a NULL pointer; B, HW or C below 1; B > 65535; B HW C >= 2^31; y overlapping x. */
int r3d_dl_global_mean(const float* x, int B, int HW, int C, float* y, r3d_stream_t stream);

/* The input assembly of Img2PlaneModel.forward (img2plane_model.py:52-64) in one pass: img [B, 3, H, W] (NCHW), alpha [B, 1, H, W] or NULL,
 * camera_feat [B, 3] or NULL -> y [B, H, W, Cin], Cin = 3 + (alpha: 1) + (camera_feat: 3) + 2, channels rgb | alpha | camera | row / H |
 * col / H.  Both grids divide by H, as the reference does; each is one IEEE fp32 division of two exact integers, the value of torch's
 * arange(H) / H bit for bit.
 * Refused: NULL img or y; B, H or W below 1; H or W above 2^24; B H W Cin >= 2^31; y overlapping an input. */
int r3d_dl_assemble_input(const float* img, const float* alpha, const float* camera_feat, int B, int H, int W, float* y, r3d_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* R3D_HIP_DEEPLAB_H */
