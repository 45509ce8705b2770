/*
 * r3d_hip_img2plane.h -- extension header of r3d_hip.h (C ABI of libr3d_hip.so): the canonical image-to-plane backbone.  It includes
 * r3d_hip.h (r3d_stream_t, the status codes, r3d_last_error); r3d_hip.h does not include it back.  The Python binding table of this
 * header is real3dportrait_amd/_lib.py EXTENSION_SIGNATURES["r3d_hip_img2plane.h"].  Functions are added without a new r3d_version().
 */
#ifndef R3D_HIP_IMG2PLANE_H
#define R3D_HIP_IMG2PLANE_H

#include "r3d_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* --- canonical image to planes: Img2PlaneModel (modules/img2plane/img2plane_model.py:12-82) without its DeepLabV3 ------------------
 * HighResoEncoder (simple_encoders/high_resolution_encoder.py), LowResolutionViT and TriplanePredictorViT (segformer/models.py) with the
 * Block / Attention / Mlp / OverlapPatchEmbed of segformer/base.py, inference only, exact fp32 (tests/img2plane_ref64.py is
 * the fp64 restatement).  The linear layers, strided convs, LayerNorms and the MLP's depthwise conv are r3d_secc_linear / r3d_secc_conv /
 * r3d_secc_layernorm / r3d_secc_dwconv_gelu and the stride-1 convs are r3d_torso_conv of r3d_hip.h, called as they are; this header adds
 * the attention at head dimension up to 256 and the data movement no entry point covered.  Same conventions as r3d_hip.h: borrowed device
 * pointers, contiguous fp32, `stream` a hipStream_t, 0 or a negative r3d_status with the message from r3d_last_error().  Activations are
 * token-major / channel-last [B, H, W, C].  No atomics, no workspace, no allocation, no host synchronisation; run to run bit-identical,
 * and a sample's result does not depend on B.  Inputs are never written. */

/* softmax(q k^T * scale) v per head (Attention.forward, segformer/base.py:101-118): q [B, N, C], kv [B, L, 2C] with k in channels [0, C)
 * and v in [C, 2C) (the layout of r3d_secc_attention), head h owns channels [D h, D h + D) with D = C / heads, out [B, N, C].
 * D is a multiple of 16 in 16 .. 256; any N >= 1 and any L >= 1 (no key limit): keys stream through LDS 32 at a time under a running
 * maximum, S = q k^T and O = P v both on v_mfma_f32_16x16x4_f32.  One wave owns 16 queries from the first key to the last, so a query's
 * result does not depend on B, on N or on the block it lands in.  scale is finite (NaN and +-inf are refused).  q, kv and out are
 * 16-byte aligned.  out must not overlap q or kv (out == q is refused too, unlike r3d_secc_attention: the module has no use for the
 * in-place form, and the rule stays free). */
int r3d_i2p_attention(const float* q, const float* kv, int B, int N, int L, int C, int heads, float scale, float* out, r3d_stream_t stream);

/* nn.UpsamplingBilinear2d(scale_factor=2) (align_corners=True) on a channel-last tensor (LowResolutionViT.upsampling_bilinear1 / 2,
 * segformer/models.py:31,34,80,83): x [B, H, W, C] -> y [B, 2H, 2W, C].  Output row o reads source position o (H - 1) / (2H - 1): the
 * integer part and the remainder come from integer division, so the weight is the correctly rounded fraction (torch rounds the scale
 * first; the product is formed in 64 bits).  Any H, W, C >= 1 with 4 B H W C < 2^31.  y must not overlap x. */
int r3d_i2p_upsample2x(const float* x, int B, int H, int W, int C, float* y, r3d_stream_t stream);

/* nn.PixelShuffle(2) of a token tensor (segformer/models.py:76-79 and :169-171): x [B, h w, 4 Co] -> channels [y_coffset, y_coffset + Co)
 * of y [B, 2h, 2w, y_cstride], y[b, 2y + i, 2x + j, y_coffset + c] = x[b, y w + x, 4c + 2i + j]; the other channels of y are left
 * untouched (the 352-channel input of first_conv_after_cat, :173).  0 <= y_coffset, y_coffset + Co <= y_cstride.  y must not overlap x. */
int r3d_i2p_pixel_shuffle(const float* x, int B, int h, int w, int Co, float* y, int y_cstride, int y_coffset, r3d_stream_t stream);

/* A channel-slice copy, one side of torch.cat(dim=1) on channel-last tensors (segformer/models.py:157,173): x [M, C] -> channels
 * [y_coffset, y_coffset + C) of y [M, y_cstride]; the other channels of y are left untouched.  Bit-exact.  y must not overlap x. */
int r3d_i2p_copy_channels(const float* x, size_t M, int C, float* y, int y_cstride, int y_coffset, r3d_stream_t stream);

/* x [B, C, H, W] -> y [B, H, W, C]: the assembled input (img2plane_model.py:45-64) as HighResoEncoder.first reads it through
 * r3d_secc_conv (7x7, stride 2, padding 3), and DeepLabV3's feature map as LowResolutionViT.patch_embed reads it.  Bit-exact.  y must
 * not overlap x. */
int r3d_i2p_nchw_to_cl(const float* x, int B, int C, int H, int W, float* y, r3d_stream_t stream);

/* The output (img2plane_model.py:72-81): x [B, H, W, 3 Cp] channel-last, the last conv's result -> planes [B, 3, Cp, H, W] with plane p
 * taking channels [p Cp, p Cp + Cp), planes 0 and 1 flipped along H and plane 2 along H and W.  Bit-exact.  planes must not overlap x. */
int r3d_i2p_planes_out(const float* x, int B, int H, int W, int Cp, float* planes, r3d_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* R3D_HIP_IMG2PLANE_H */
