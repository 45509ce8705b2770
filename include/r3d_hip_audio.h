/*
 * r3d_hip_audio.h -- companion header of r3d_hip.h (C ABI of libr3d_hip.so): the audio-to-motion VAE.  r3d_hip.h includes it; it can also
 * be included on its own.  The Python binding table of this header is real3dportrait_amd/_lib.py SIGNATURES.
 */
#ifndef R3D_HIP_AUDIO_H
#define R3D_HIP_AUDIO_H

#include "r3d_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* --- audio to motion: the inference path of PitchContourVAEModel / VAEModel (modules/audio2motion/vae.py:272-454) ----------------------
 * What forward_audio2secc (inference/real3d_infer.py:365-388) runs between the HuBERT / f0 features and the expression coefficients, as
 * three kernels (tests/audio2motion_ref64.py is the fp64 restatement).  Same conventions as r3d_hip.h: borrowed device
 * pointers, contiguous fp32, `stream` a hipStream_t, 0 or a negative r3d_status, the message from r3d_last_error().
 * Activations are time-major, [B, T, C]: channel c of row t of sample b is at ((b T + t) row_stride + offset + c).  Every product is an
 * exact fp32 product on the f32 MFMA; tanh, sigmoid, erf and log are the accurate device functions.  A sample never reads another
 * sample's rows (padding is per sample).  No atomics, no workspace, no allocation, no host synchronisation; run to run bit-identical,
 * and a sample's result does not depend on B.  Inputs are never written.
 *
 * r3d_a2m_conv1d is nn.Conv1d as a GEMM over taps: x [B, Tsrc, x_stride] read at columns x_offset .. x_offset + Cin, w [Cout, k, Cin]
 * (the host permutes torch's [Cout, Cin, k]), bias [Cout] or NULL, y [B, Tout, y_stride] written at columns y_offset .. y_offset + Cout,
 * Tout = (Tin + 2 pad - k) / stride + 1, zero padding.
 *   row_mode: which source row is input row t of Tin.  0: row t (Tsrc = Tin).  1: row 2 t (Tsrc = 2 Tin), the F.interpolate(scale_factor
 *   = 0.5, mode='nearest') of vae.py:385.  2: 0.5 (row 2 t + row 2 t + 1) (Tsrc = 2 Tin), mode='linear' at 0.5 (vae.py:295).
 *   The epilogue, in this order, each piece optional (NULL / 0):  v = sum + bias[co];  v += table[idx[b, idx_step t]][co], idx int64
 *   [B, idx_step Tout], idx_step 1 or 2 (2: the nearest 0.5 x down-sampling of the indices, as row mode 1 reads x), table
 *   [table_rows, Cout] (the folded blink_embed; an index outside the table is clamped into it, where the reference raises);
 *   v += amp0[b] u0[co] + amp1[b] u1[co], amp [B], u [Cout] (the folded mouth_amp_embed / eye_amp_embed);  gelu: v = 0.5 v (1 + erf(v / sqrt 2));  v *= mask[b, t], mask [B, Tout];  subtract_from: v = other - v, `other` laid
 *   out and addressed as y is and either y itself (in place) or disjoint from it (the mean-only reverse coupling x1 - m,
 *   flow_base.py:664);  flip_out: column y_offset + co is stored at y_stride - 1 - (y_offset + co) (Flip, flow_base.py:389-393).
 *   It covers mel_encoder and pitch_encoder (BatchNorm1d folded), cond_proj (k = 1 over [cond_feat | pitch_feat] plus the table and the
 *   amplitude terms), g_pre_net (k 8, stride 4, pad 2), the flows' pre and post, the decoder's ConvTranspose1d(16, 256, 4, 4) (k = 1 to
 *   [Tq, 4 x 256] viewed as [4 Tq, 256]) and out_proj with the final mask.
 * r3d_a2m_wn_layer is one layer of WN.forward (flow_base.py:77-96) in one launch: x [B, T, H], g [B, T, Cg] ->
 *   a = [taps of x | g] w_in + b_in, w_in [k H + Cg, 2 H]: row j H + ci is tap j of the weight-normed in_layer's input channel ci, row
 *   k H + cg the layer's slice of cond_layer, b_in the sum of the two biases ('same' zero padding, dilation 1; cond_layer(g) itself is
 *   never written);  acts = tanh(a[:H]) sigmoid(a[H:]), kept in LDS;  rs = acts w_rs + b_rs, w_rs [H, 2 H], or [H, H] when `last`.
 *   Not last: x_next = (x + rs[:H]) mask, out = rs[H:] (first) or out + rs[H:].  Last: out = (rs or out + rs) mask, x_next NULL.
 *   mask [B, T] or NULL (ones).  x_next is another buffer than x (neighbouring tiles read the halo); x itself is not written.  A block
 *   owns R3D_A2M_WN_ROWS rows of one sample plus the halo; T need not be a multiple.
 * r3d_a2m_pitch_embed is f0_to_coarse (utils/commons/pitch_utils.py:17-26) and the pitch_embed lookup: f0 [B, 2 T] read at 2 t
 *   (row mode 1), in fp32 in the reference's order of operations: m = 1127 log(1 + f0 / 700); where m > 0, m = (m - mel_min) 254 /
 *   (mel_max - mel_min) + 1; m <= 1 -> 1; m > 255 -> 255; index = (int)(m + 0.5).  index [B, T] int32 and y [B, T, C] = table[index],
 *   table [rows, C].  An fp32 log that differs from another library's by an ulp can move an index when m + 0.5 lies within about 1e-4
 *   of an integer.
 * Refused before any launch with R3D_ERR_INVALID_ARG: a NULL pointer that is not optional (or one half of a pair: table / idx, amp / u);
 * a size below 1; B > 65535; k outside 1 .. 8, stride < 1, pad outside 0 .. k - 1, Tin + 2 pad < k, row_mode outside 0 .. 2, a column
 * slice outside its row, idx_step other than 1 or 2 with a table (conv1d); H other than 64 or 256, k other than 1, 3 or 5, Cg outside
 * 4 .. 256 or no multiple of 4, x_next given with `last` or missing without it (wn_layer); an index product of 2^31 or more; an output that overlaps an input or another output. */
#define R3D_A2M_WN_ROWS 16
int r3d_a2m_conv1d(const float* x, int B, int Tin, int Cin, int x_stride, int x_offset, int row_mode, const float* w, const float* bias,
                   int Cout, int k, int stride, int pad, int gelu, const float* mask, const float* table, const int64_t* idx, int table_rows,
                   int idx_step, const float* amp0, const float* u0, const float* amp1, const float* u1, const float* subtract_from,
                   float* y, int y_stride, int y_offset, int flip_out, r3d_stream_t stream);
int r3d_a2m_wn_layer(const float* x, const float* g, int B, int T, int H, int Cg, int k, const float* w_in, const float* b_in,
                     const float* w_rs, const float* b_rs, const float* mask, int first, int last, float* x_next, float* out,
                     r3d_stream_t stream);
int r3d_a2m_pitch_embed(const float* f0, int B, int T, const float* table, int rows, int C, int32_t* index, float* y, r3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* R3D_HIP_AUDIO_H */
