/*
 * r3d_hip_hubert.h -- feature header of r3d_hip.h (C ABI of libr3d_hip.so): the HuBERT audio feature extractor.  It includes r3d_hip.h
 * (r3d_stream_t, the status codes, r3d_last_error); r3d_hip.h does not include it back.  The Python binding table of this header is
 * real3dportrait_amd/_lib.py FEATURE_SIGNATURES["r3d_hip_hubert.h"].  Functions are added without a new r3d_version().
 */
#ifndef R3D_HIP_HUBERT_H
#define R3D_HIP_HUBERT_H

#include "r3d_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* --- HuBERT features: GeneFace2Infer.get_hubert (inference/real3d_infer.py:323-334) -> get_hubert_from_16k_speech
 * (data_gen/utils/process_audio/extract_hubert.py:18-80) -> transformers.HubertModel of facebook/hubert-large-ls960-ft -------------------
 * The transformer layers are r3d_secc_linear (LayerNorm prologue, exact-erf GELU, residual), r3d_i2p_attention and r3d_secc_layernorm,
 * called as they are (real3dportrait_amd/hubert.py; tests/hubert_ref64.py is the fp64 restatement).  This header adds the
 * model's two convolutional ends and the clip statistics of its feature extractor.  Same conventions as r3d_hip.h: borrowed device
 * pointers, contiguous fp32, activations token-major [B, T, C], `stream` a hipStream_t, 0 or a negative r3d_status with the message from
 * r3d_last_error().  Exact fp32: every product of the two matrix kernels runs on v_mfma_f32_16x16x4_f32.  No atomics, no workspace, no
 * allocation, no host synchronisation; run to run bit-identical, and a frame's result does not depend on B, on T or on the block it lands
 * in.  Inputs are never written.  Every refusal below is R3D_ERR_INVALID_ARG before any launch. */

/* Wav2Vec2FeatureExtractor.zero_mean_unit_var_norm over the WHOLE waveform (the reference normalises before it cuts chunks, extract_hubert.py
 * :39, so the statistics are per clip, not per chunk): stats[0] = the mean of the n samples, stats[1] = 1 / sqrt(var + 1e-7) with the
 * population variance, both fp64, two passes (the mean, then the squared deviations), one block, a fixed summation order.
 * Refused: NULL wave or stats; n = 0; n >= 2^31; stats not 8-byte aligned; stats overlapping wave. */
int r3d_hubert_wave_stats(const float* wave, size_t n, double* stats, r3d_stream_t stream);

/* Front-end layer 0 (HubertLayerNormConvLayer, conv_layers.0): sequence b reads the n_chunk samples from
 * wave + sample_offset + b * sample_stride (chunks may overlap; nothing is copied), each normalised on load as
 * (float)(((double)x - stats[0]) * stats[1]); then Conv1d(1, C0, k, stride, no padding) + bias, LayerNorm over C0 (two-pass on the fp32
 * values, eps), exact-erf GELU.  w [C0, k], bias / ln_g / ln_b [C0]; y [B, T0, C0] with T0 = (n_chunk - k) / stride + 1.
 * Refused: a NULL pointer; B, n_chunk, C0, k or stride below 1; B > 65535; k > 16; stride > 16; C0 not a multiple of 16 or above 512;
 * n_chunk < k; eps negative or not finite; sample_offset + (B - 1) sample_stride + n_chunk >= 2^31 or B T0 C0 >= 2^31; stats not 8-byte
 * aligned; y overlapping the samples read, stats or a parameter. */
int r3d_hubert_conv0(const float* wave, const double* stats, int B, size_t sample_offset, size_t sample_stride, int n_chunk, const float* w,
                     const float* bias, const float* ln_g, const float* ln_b, float eps, int C0, int k, int stride, float* y, r3d_stream_t stream);

/* Front-end layers 1 .. 6 (HubertLayerNormConvLayer: k 3 or 2, stride 2): Conv1d(Cin, Cout, k, stride, no padding) + bias, LayerNorm over
 * Cout (eps), exact-erf GELU, one launch.  x [B, Tin, Cin], w [Cout, k, Cin] (the parameter [Cout, Cin, k] permuted), bias / ln_g / ln_b
 * [Cout]; y [B, Tout, Cout] with Tout = (Tin - k) / stride + 1.  On a channel-last tensor the im2col row of output t is the contiguous span
 * x[stride t .. stride t + k - 1, :], so this is a GEMM with K = k Cin and an A row stride of stride Cin, no gather.  A block owns 32 output
 * rows and all Cout columns; the LayerNorm statistics are two-pass on the accumulators in a fixed cross-wave order.
 * Refused: a NULL pointer; B, Tin, Cin, Cout, k or stride below 1; k > 4; Cin or Cout not a multiple of 16 or above 512; Tin < k; eps negative
 * or not finite; B Tin Cin >= 2^31 or B Tout Cout >= 2^31; x or w not 16-byte aligned; y overlapping x or a parameter. */
int r3d_hubert_conv_ln_gelu(const float* x, const float* w, const float* bias, const float* ln_g, const float* ln_b, float eps, int B, int Tin,
                            int Cin, int Cout, int k, int stride, float* y, r3d_stream_t stream);

/* HubertPositionalConvEmbedding + HubertSamePadLayer + the residual add of HubertEncoderStableLayerNorm.forward:
 * y = x + gelu(conv(x) + bias) with conv = Conv1d(C, C, k, padding = k / 2, groups), whose last output is dropped when k is even.
 * x, y [B, T, C]; w [C, k, C / groups] is the EFFECTIVE weight (the caller resolves the weight-norm parametrisation) permuted from
 * [C, C / groups, k]; bias [C].  Output t sums taps j = 0 .. k - 1 over x[t + j - k / 2], zero outside [0, T).
 * Refused: a NULL pointer; B, T, C, k or groups below 1; B or groups > 65535; k > 128; C not a multiple of groups; C / groups not a
 * multiple of 16 or above 64; B T C >= 2^31; x or w not 16-byte aligned; y overlapping x (y == x too) or a parameter. */
int r3d_hubert_pos_conv(const float* x, const float* w, const float* bias, int B, int T, int C, int k, int groups, float* y, r3d_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* R3D_HIP_HUBERT_H */
