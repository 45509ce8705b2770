/*
 * r3d_hip.h -- C ABI of libr3d_hip.so: MI355X (gfx950) native tri-plane NeRF render + super-resolution.
 *
 * This is the drop-in boundary for the per-frame hot path of Real3D-Portrait.  The reference has no
 * native renderer (it is ~25 eager ATen ops per pass) and three pybind11/CUDA plugins for the SR
 * blocks; every entry point below names the reference interface it replaces (file:line relative to the
 * upstream repo).  All pointers are BORROWED raw device pointers (fp32 unless noted), all tensors are
 * contiguous, `stream` is a hipStream_t passed as void*.  No function synchronises, allocates or frees
 * device memory.  Every function returns 0 on success or a negative r3d_status; the message of the last
 * failure on the calling thread is available from r3d_last_error().
 *
 * Reference-side binding: see INTEGRATION.md (ctypes stub a maintainer would add).
 */
#ifndef R3D_HIP_H
#define R3D_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* r3d_stream_t; /* hipStream_t */

enum r3d_status {
    R3D_OK = 0,
    R3D_ERR_INVALID_ARG = -1,   /* shape / pointer / option outside what the kernels support */
    R3D_ERR_WORKSPACE = -2,     /* workspace pointer NULL or too small */
    R3D_ERR_LAUNCH = -3,        /* HIP launch / runtime error (message has hipGetErrorString) */
    R3D_ERR_UNSUPPORTED = -4    /* valid in the reference, not implemented here (e.g. trigrid) */
};

#define R3D_FEATURES 32         /* tri-plane channels C            (img2plane_model.py:72-82)        */
#define R3D_HIDDEN 64           /* OSGDecoder hidden width         (modules/eg3ds/models/triplane.py:169) */
#define R3D_DECODER_OUT 33      /* 1 density + 32 colour features  (triplane.py:175)                 */

int r3d_version(void);
const char* r3d_last_error(void);

/* --- plane layout -------------------------------------------------------------------------------
 * Re-lays tri-planes from the reference's NCHW [N,3,C,H,W] to channel-last [N,3,H,W,C] so that each
 * bilinear tap is one contiguous 128-byte read, optionally fusing the per-frame `cano + secc` add.
 * Replaces: the plane add in OSAvatarSECC_Img2plane.cal_plane_given_cano (modules/real3d/
 * secc_img2plane.py:73-81) + the reshape at modules/eg3ds/volumetric_rendering/renderer.py:68.
 * `add` may be NULL.  add_flip: bit 2k flips plane k of `add` along H, bit 2k+1 along W, while it is read -- the
 * torch.flip calls SegFormerSECC2PlaneBackbone.forward applies to its conv output (modules/real3d/segformer.py:722-728:
 * planes 0,1 along H, plane 2 along H and W = 0b110101 = 53) when `add` is the raw to_plane_cnn output; 0 = none.
 * depth > 1: tri-grids (triplane_feature_type 'trigrid' / 'trigrid_v2', renderer.py:78-89): planes_nchw is
 * [N,3,C*depth,H,W] with channel c*depth + d (the reference's .view(N*3, C, D, H, W)) -> [N,3,depth,H,W,C].
 * Limit: H * W <= 2^31 - 1 (the kernels index a plane with an int); larger planes are refused with R3D_ERR_INVALID_ARG. */
#define R3D_SECC_PLANE_FLIPS 53
int r3d_planes_to_nhwc(const float* planes_nchw, const float* add_nchw, float* planes_nhwc,
                       int N, int C, int H, int W, int depth, int add_flip, float* absmax_partials, int* n_partials,
                       r3d_stream_t stream);
/* absmax_partials (may be NULL): device float[r3d_planes_absmax_partials(...)] that receives one max|value| per thread block of the
 * layout pass (no extra pass over the 25 MB, no atomics); *n_partials (host int) = how many were written.  They feed the renderer's
 * fp16 range fold (r3d_render_forward / r3d_run_model `plane_absmax`). */
size_t r3d_planes_absmax_partials(int N, int C, int H, int W, int depth);

/* --- A1 ray generation --------------------------------------------------------------------------
 * Replaces RaySampler.forward(cam2world[N,4,4], intrinsics[N,3,3], resolution)
 * (modules/eg3ds/volumetric_rendering/ray_sampler.py:24-63).  origins/dirs: [N, R*R, 3].
 * Limit: R * R <= 2^31 - 1 (R <= 46340); a larger image is refused with R3D_ERR_INVALID_ARG. */
int r3d_raygen(const float* c2w, const float* intrinsics, int N, int R,
               float* origins, float* dirs, r3d_stream_t stream);

/* --- A2..A10 volume render ----------------------------------------------------------------------
 * Replaces ImportanceRenderer.forward(planes, decoder, ray_origins, ray_directions, rendering_options)
 * (modules/eg3ds/volumetric_rendering/renderer.py:118-167) with ray_start == ray_end == 'auto',
 * disparity_space_sampling False, clamp_mode 'softplus', feature type 'triplane': box limits + fix-up
 * (math_utils.py:46-98, renderer.py:121-126), stratified depths (:209-232), tri-plane sampling (:65-75),
 * OSGDecoder (modules/eg3ds/models/triplane.py:177-189), MipRayMarcher2 (ray_marcher.py:25-57),
 * importance resampling (:234-297), sort-merge (:197-207) and the final composite.
 *
 *   planes_nhwc  [N,3,H,W,32]      from r3d_planes_to_nhwc
 *   triplane_depth 1: tri-planes, bilinear (sample_from_planes, renderer.py:65-75);  D > 1: tri-grids [N,3,D,H,W,32],
 *                tri-linear with zero padding (sample_from_trigrids, renderer.py:78-89; hparams triplane_depth = 3)
 *   w1,b1,w2,b2  RAW decoder parameters decoder.net.0.{weight[64,32],bias[64]}, decoder.net.2.{weight[33,64],
 *                bias[33]}; the FullyConnectedLayer gains 1/sqrt(fan_in) are applied inside
 *   origins,dirs [N,M,3]
 *   Nc, Nf       depth_resolution / depth_resolution_importance (4 <= Nc <= 96, 0 <= Nf <= 96)
 *   noise_c      [N,M,Nc] U[0,1) stratification jitter (the reference's torch.rand_like, renderer.py:226)
 *   u_f          [N*M,Nf] U[0,1) importance draws       (the reference's torch.rand,      renderer.py:281)
 *                either may be NULL: the kernel then draws from a counter-based hash of
 *                (seed, ray, sample), which makes a frame's noise independent of how frames are sharded
 *   rgb [N,M,32] (rgb_channel_major = 0: what the reference's renderer returns) or [N,32,M] (rgb_channel_major = 1: the NCHW
 *                feature image TriPlaneGenerator.synthesis builds from it with permute(0,2,1).reshape(N,32,R,R), triplane.py:121-122,
 *                written directly so that no transposition pass runs per frame)
 *   depth [N,M] or NULL (no depth image: the global-range clamp launch is skipped), wsum [N,M], valid [N,M] (1 byte, is_ray_valid)
 *   plane_absmax device float[n_plane_absmax] whose maximum bounds |planes_nhwc| (the partials of r3d_planes_to_nhwc), or NULL / 0: the
 *                bound is then measured here (one extra pass over the planes).  fp16 range management of the decoder: the MLP runs on
 *                the f16 matrix pipe with fp32 operands split into fp16 hi + lo; one small launch per call (decoder_fold_kernel) derives
 *                exact power-of-two factors from this bound and from the weights (features * 2^b against W1 * 2^-b, and -- only when a
 *                bound would reach 2^15 -- 2^c on the hidden values / 2^d on the colour rows), so that the result equals the reference's
 *                unbounded fp32 evaluation for any magnitude of planes and weights whose pre-activations fit fp32.
 *                The bound must be RIGOROUS (max of the array >= max |planes_nhwc| as the kernel will read them): the per-sample fp16
 *                split has no saturation guard, so a stale or too small bound yields inf / NaN, not a clamp.  Pass NULL whenever the
 *                planes were modified after the partials were written (the Python operator does: it ties them to the tensor version).
 *   workspace    r3d_render_workspace_bytes() bytes of device scratch, 64-byte aligned.  Per-ray limits and the decoder's fold record; when Nc or Nf
 *                exceeds 48 AND Nf > 0 (the kernel shapes with more than three 16-sample tiles per pass and a fine pass) also 24 KB per wave of the
 *                launch's grid (min(512, rays / 4 rounded up to 8) blocks x 4 waves: 48 MB for a full grid), in which a wave parks the colours of the
 *                ray it is rendering between the decode and the composite (ABI 0.5.0: they do not fit the register file; 0.6.0: sized from the grid).
 * Limits, refused with R3D_ERR_INVALID_ARG: 3 * triplane_depth * H * W * 128 < 2^32 (the taps are 32-bit byte offsets into one image's planes) and
 * N * M <= 2^31 - 1 (the kernels carry the ray index in an int).
 */
size_t r3d_render_workspace_bytes(int N, int M, int Nc, int Nf);
int r3d_render_forward(const float* planes_nhwc, int N, int H, int W, int triplane_depth,
                       const float* w1, const float* b1, const float* w2, const float* b2,
                       const float* origins, const float* dirs, int M,
                       int Nc, int Nf, float box_warp, int white_back,
                       const float* noise_c, const float* u_f, uint64_t seed,
                       float* rgb, int rgb_channel_major, float* depth, float* wsum, uint8_t* valid,
                       const float* plane_absmax, int n_plane_absmax,
                       const float* cam2world, const float* intrinsics,
                       void* split_out, const float* split_scale, size_t split_scale_stride,
                       void* workspace, size_t workspace_bytes, r3d_stream_t stream);
/* Camera mode (origins = dirs = NULL, cam2world [N,4,4] + intrinsics [N,3,3] given, M = R * R): RaySampler.forward is evaluated inside
 * the limits pass and the render kernel with r3d_raygen's instruction sequence -- the same pixels as r3d_raygen + the ray arrays, without
 * the launch and the two [N,M,3] round trips.  cam2world / intrinsics are ignored when origins / dirs are given (pass NULL).
 * split_out (may be NULL): a second copy of the colours in R3D_FMT_SPLIT ([N][hi|lo][4][M][8] fp16), multiplied by split_scale[n][c]
 * (stride split_scale_stride floats; = the start of the consuming SR block's styles buffer AFTER r3d_chain_fold): the input of
 * r3d_sr_block_forward(x_format = R3D_FMT_SPLIT) without a conversion launch. */

/* Replaces ImportanceRenderer.run_model(planes, decoder, sample_coordinates, sample_directions, options)
 * (renderer.py:169-188; inference branches) -- the point-query used by .sample() (triplane.py:140-148).
 * coords [N,npts,3] -> rgb [N,npts,32], sigma [N,npts].
 * Limits, refused with R3D_ERR_INVALID_ARG: 3 * triplane_depth * H * W * 8 < 2^31 (the gather indexes one image's planes with an int in 16-byte
 * units) and H, W < 2^24 (24-bit row products). */
int r3d_run_model(const float* planes_nhwc, int N, int H, int W, int triplane_depth,
                  const float* w1, const float* b1, const float* w2, const float* b2,
                  const float* coords, int npts, float box_warp,
                  float* rgb, float* sigma, const float* plane_absmax, int n_plane_absmax,
                  void* workspace, size_t workspace_bytes, r3d_stream_t stream);
/* plane_absmax / n_plane_absmax: as for r3d_render_forward; workspace: r3d_run_model_workspace_bytes() bytes, 16-byte aligned */
size_t r3d_run_model_workspace_bytes(void);

/* --- A12..A14 super-resolution ------------------------------------------------------------------
 * One StyleGAN2 SynthesisBlock (architecture 'skip', up=2, fp32, eval, noise_mode 'none'):
 * replaces SynthesisBlock.forward (modules/eg3ds/models/networks_stylegan2.py:429-473) including
 * modulated_conv2d (:37-94), conv2d_resample up=2 path (torch_utils/ops/conv2d_resample.py:116-133),
 * and the three plugin calls it makes: bias_act_plugin.bias_act (ops/bias_act.cpp:36),
 * upfirdn2d_plugin.upfirdn2d (ops/upfirdn2d.cpp:20) for the post-T-conv FIR and the RGB-skip upsample2d.
 *
 * Modulated convolution is evaluated as  y = d[cout] * conv(s[ci] * x, W)  (== conv(x, W*s*d), :62-70), so:
 * r3d_sr_block_prepack: STATIC re-layout of conv0/conv1 weights ([tap][ci/8][cout][ci%8]); call once per
 *   parameter update.  prepacked: r3d_sr_block_prepacked_bytes(Cin,Cout) bytes.
 * r3d_sr_block_styles: per-forward small vectors for one batch of style inputs: styles s = affine(w) (:326),
 *   demodulation d = rsqrt(sum (W*s)^2 + 1e-8) (:65-70), modulated toRGB weights (:366-368), biases.
 *   ws3 [N,3,WD] (conv0, conv1, torgb);  *_w/_b/_aw/_ab = layer.weight / .bias / .affine.weight / .affine.bias;
 *   styles: r3d_sr_block_styles_bytes(N,Cin,Cout) bytes.
 * r3d_sr_block_forward:
 *   x [N,Cin,Hin,Win] in x_format, img [N,3,Hin,Win] NCHW fp32
 *   -> x_out in x_out_format (may be NULL / R3D_FMT_NONE), img_out [N,3,2Hin,2Win] NCHW fp32.
 *   up = 1: SynthesisBlock (conv0 up=2, RGB skip through upsample2d).  up = 0: SynthesisBlockNoUp
 *   (modules/eg3ds/models/superresolution.py:159-258: conv0 is a plain modulated 3x3 conv and img_out = img + toRGB(x)
 *   at the input resolution; img and img_out are [N,3,Hin,Win]); R3D_SR_F16X3 only.  Cin % 16 == 0, Cout % 128 == 0.
 *   Activation formats: R3D_FMT_NCHW fp32 (the reference layout); R3D_FMT_CB8 fp32 channel-blocked [N,C/8,H,W,8];
 *   R3D_FMT_SPLIT (f16x3 only): two fp16 planes [N][hi|lo][C/8][H][W][8] holding the activation ALREADY MULTIPLIED
 *   by the consumer conv's style vector -- as input it must have been scaled with this block's conv0 styles; as
 *   output it is scaled with `next_scale` ([N][Cout] floats, stride next_scale_stride: the next block's conv0 styles,
 *   i.e. the start of that block's styles buffer).
 *   R3D_FMT_SPLIT_MX (R3D_SR_F16MX): R3D_FMT_SPLIT whose lo plane holds, byte for byte in its place, the 8-bit correction
 *   records of the f16mx precision: lo chunk 2G: xh8 = e5m2(hi) of channels 16G..16G+15, lo chunk 2G+1: xl8 = e5m2(lo * 2^11) (OCP e5m2 since ABI
 *   0.5.0 -- a per-element exponent with the fp16 hi plane's range; 0.4.0: e4m3 of hi * 2^-7 / lo * 2^4, one exponent per tensor).
 *   As x_out_format the block's conv1 epilogue writes them; as x_format the block's up-sampling conv runs its cross products on the
 *   block-scaled 8-bit MFMA (2 instead of 3 matrix passes per MAC).  A producer / consumer pair must agree (same next_scale as SPLIT).
 *   clamp < 0 disables conv_clamp (the fp32 configuration Real3D uses, img2plane_baseline.py:102-104).
 *   img_u8 (may be NULL; R3D_SR_F16X3 only): [N,OH,OW,3] uint8 -- the block is the last one of the network and the frame leaves
 *   as clamp(-1,1) -> ((x + 1) / 2 * 255).int() (triplane.py:136 + inference/real3d_infer.py:472,518-522), fused into the
 *   toRGB finalize kernel; img_out may then be NULL.
 *   x_absmax (may be NULL; R3D_SR_F16X3 only): device float[N], atomically maxed with |x_out| (see r3d_chain_fold).
 *   R3D_SR_F16X3 reads the FOLDED vectors of the styles buffer: call r3d_chain_fold (below) after r3d_sr_block_styles and
 *   before r3d_sr_block_forward, every forward.
 *
 * precision: R3D_SR_F32   exact fp32 on v_mfma_f32_32x32x2_f32 (bitwise an fmaf chain);
 *            R3D_SR_F16X3 fp32-accurate on the f16 matrix pipe: every operand is split x = hi + lo (two fp16
 *                         terms, 2^-24 relative) and hi*hi + hi*lo + lo*hi is accumulated in fp32 by
 *                         v_mfma_f32_32x32x16_f16 (3 MFMAs at 16x the f32 rate; ~1e-7 relative per dot product).
 *            R3D_SR_F16MX (what the Python operators pass by default): as F16X3, but in the 3x3 convs whose input arrives as R3D_FMT_SPLIT_MX the two
 *                         2^-11-sized correction products hi*lo + lo*hi of two taps x 16 channels are ONE block-scaled 8-bit MFMA
 *                         (v_mfma_scale_f32_32x32x64_f8f6f4: activation records OCP e5m2, weight records OCP e4m3, 2x the f16 rate) instead of
 *                         four f16 MFMAs: 1.5x fewer matrix cycles.  The correction is then accurate to e5m2 rounding, i.e. ~2^-15 of each
 *                         product (between fp32's 2^-24 and TF32's 2^-11); parity: <= 5e-5 * max|ref| per block on the reference goldens,
 *                         <= 6.3e-5 near and far field on the heavy-tail sweeps (spikes of 2^6 .. 2^14 sigma) against the 2e-4 tolerance of
 *                         the path, <= 1e-4 over the 2^-20..2^14 operand sweeps vs fp64 (tests/test_gpu_mx.py, tests/test_gpu_pinned_config.py).
 *                         The records have the hi plane's exponent range: no measured bound is needed beyond what R3D_SR_F16X3 needs
 *                         (R3D_CHAIN_SR_BLOCK_TAIL stays available for chains deeper than three layers).
 *            The prepacked buffer is precision-specific (same size).
 *            Algorithm (ABI 0.6.0): the block's plain 3x3 conv (conv1) has a second implementation, Winograd F(2,3) along x with the input transform in
 *            the kernel (csrc/r3d_sr_wino.h: 12 instead of 18 matrix products per pair of output columns; the prepacked buffer carries the 12
 *            transformed tap matrices).  It is taken for R3D_SR_F16X3 when the output is whole 16 x 16 tiles (-13 % per launch, fp32-class:
 *            error x 1.4 of the direct form's 7e-8); for R3D_SR_F16MX the direct kernel is faster and stays.  Process-wide switch:
 *            R3D_CONV_WINO = 0 (never) | 1 (both precisions) | 2 (f16mx only) | 3 (f16x3 only, the default). */
enum r3d_sr_precision { R3D_SR_F32 = 0, R3D_SR_F16X3 = 1, R3D_SR_F16MX = 2 };
enum r3d_act_format { R3D_FMT_NONE = -1, R3D_FMT_NCHW = 0, R3D_FMT_CB8 = 1, R3D_FMT_SPLIT = 2, R3D_FMT_SPLIT_MX = 3 };
size_t r3d_sr_block_prepacked_bytes(int Cin, int Cout);
size_t r3d_sr_block_styles_bytes(int N, int Cin, int Cout);
size_t r3d_sr_block_workspace_bytes(int N, int Cin, int Cout, int Hin, int Win);
int r3d_sr_block_prepack(int Cin, int Cout, const float* c0_w, const float* c1_w, void* prepacked,
                         int precision, r3d_stream_t stream);
int r3d_sr_block_styles(const float* ws3, int N, int WD, int Cin, int Cout,
                        const float* c0_w, const float* c0_b, const float* c0_aw, const float* c0_ab,
                        const float* c1_w, const float* c1_b, const float* c1_aw, const float* c1_ab,
                        const float* rgb_w, const float* rgb_b, const float* rgb_aw, const float* rgb_ab,
                        void* styles, r3d_stream_t stream);
int r3d_sr_block_forward(const void* prepacked, const void* styles, int N, int Cin, int Cout, int Hin, int Win, int up,
                         const void* x, int x_format, const float* img, float clamp,
                         void* x_out, int x_out_format, const float* next_scale, size_t next_scale_stride,
                         float* img_out, uint8_t* img_u8, float* x_absmax, int precision,
                         void* workspace, size_t workspace_bytes, r3d_stream_t stream);

/* --- fp16 range management of the R3D_SR_F16X3 path ----------------------------------------------------------------
 * The reference runs these layers in fp32 with conv_clamp=None (no range limit).  The f16x3 kernels keep fp32 accuracy while a
 * stored fp16 operand tensor has rms >= 2^-3 and max < 65504, so every operand is stored times an exact power of two:
 * weight rows at prepack time (max|w[co]| -> [2^10, 2^11)), activations per sample from a guaranteed bound B >= max|x| that is
 * propagated layer to layer (B_out = gain * max_co(|b[co]| + d[co] * sum|w[co] * s| * B_in)); the factors are taken out again in
 * the fp32 epilogue.  r3d_chain_fold walks a chain of layers ON THE DEVICE (one launch, no host sync) and writes each layer's
 * folded multipliers: SR blocks into their styles buffer, plain convs into their `scales` buffer (r3d_conv_scales_bytes).
 *   src_a / src_b: where the layer's input bound comes from: k >= 0 = output bound of op k (k < this op's index);
 *   -1 - j = ext_bounds[j] (device float[N]: a measured r3d_absmax result, a previous chain's bound, or a constant);
 *   R3D_CHAIN_SRC_NONE = unused.  Two sources = a concatenation / blend of two tensors (r3d_blend_cat_to_split): the max.
 * The bound loosens ~5 binades per layer (10 binades of slack remain after one layer): re-measure (r3d_absmax on an fp32 tensor)
 * after at most 3 chained layers.  r3d_*_bound_offset: float offset, within one sample's buffer, of the op's output bound.
 * Measuring without an extra pass: r3d_sr_block_forward / r3d_conv_forward take `y_absmax` (device float[N] or NULL): the conv
 * epilogue then atomically maxes |y| into it; the slot must be zero beforehand -- pass it in `zero_slots` of the r3d_chain_fold
 * launch that precedes the producer (up to R3D_CHAIN_MAX_ZERO slots of N floats each are cleared by the fold kernel).  The kernel
 * reads its external bounds BEFORE it clears: a slot may be an ext bound and a zero slot of the same fold (consume the measured
 * maximum of this frame, re-arm the slot for the next frame). */
#define R3D_CHAIN_MAX_ZERO 4
#define R3D_CHAIN_MAX_OPS 12
#define R3D_CHAIN_MAX_EXT 4
#define R3D_CHAIN_SRC_NONE (-1000)
enum r3d_chain_kind {
    R3D_CHAIN_SR_BLOCK = 0,       /* both layers of an SR block from the bound of the block input */
    R3D_CHAIN_CONV = 1,           /* a plain conv layer */
    R3D_CHAIN_SR_BLOCK_TAIL = 2   /* re-fold only the block's second layer (conv1 operand) from a MEASURED max|block input|: the
                                     block's input was already written with the multipliers of an earlier R3D_CHAIN_SR_BLOCK fold */
};
typedef struct r3d_chain_op {
    int kind;                 /* r3d_chain_kind */
    int Cin, Cout, ksize;     /* ksize: R3D_CHAIN_CONV only */
    int act;                  /* R3D_CHAIN_CONV: activation after the bias (|act(t)| <= gain * |t|); SR blocks always activate */
    float gain, clamp;        /* act gain (sqrt(2) for SR blocks); clamp < 0: off */
    int src_a, src_b;
    void* scales;             /* SR block: styles buffer (r3d_sr_block_styles).  conv: r3d_conv_scales_bytes() buffer */
    const void* prepacked;    /* conv: r3d_conv_prepack buffer (its tail holds 2^-kw[co] and sum|w[co]|) */
    const float* bias;        /* conv: [Cout] or NULL */
} r3d_chain_op;
int r3d_chain_fold(const r3d_chain_op* ops, int nops, int N, const float* const* ext_bounds, int n_ext,
                   float* const* zero_slots, int n_zero, r3d_stream_t stream);
size_t r3d_sr_block_bound_offset(int Cin, int Cout);
size_t r3d_conv_scales_bound_offset(int Cin, int Cout);
/* out[n] = max |x[n, :]| over count_per_sample floats.  `out` (float[N]) must be zero on entry; zero_next (float[N], may be NULL)
 * is cleared by the same launch so that two alternating slots need no memset. */
int r3d_absmax(const float* x, size_t count_per_sample, int N, float* out, float* zero_next, r3d_stream_t stream);

/* --- plain convolution layers around the SR blocks --------------------------------------
 * replaces torch.nn.Conv2d(Cin, Cout, k, 1, padding=k//2) [+ torch.nn.LeakyReLU] as used by the torso / background
 * fusion stacks of SuperresolutionHybrid8XDC_Warp (modules/real3d/super_resolution/sr_with_ref.py:24-63:
 * torso_encoder, bg_encoder, fuse_head_torso_convs, fuse_fg_bg_convs) and by to_plane_cnn (modules/real3d/segformer.py:691-700),
 * on the f16x3 convolution kernel of the SR blocks (fp32-accurate, see r3d_sr_precision).
 *   y = act(conv_k(x, W) + bias[co]),  act(t) = (t < 0 ? act_slope * t : t) * act_gain when act != 0, then clamp to +-clamp
 *   when clamp >= 0.  ksize 1 | 3.  weight [Cout,Cin,k,k] fp32 (torch layout).  Cout % 4 == 0.  bias [Cout] or NULL.
 *   scales: this layer's r3d_conv_scales_bytes() buffer, filled by r3d_chain_fold for this forward.
 *   x / y formats as for the SR blocks; blocked formats (CB8, SPLIT) need Cin % 16 == 0 / Cout % 8 == 0, NCHW takes
 *   any Cin (zero padded to 16 inside).  A SPLIT x must have been written with this layer's in-multiplier (the start of
 *   `scales`); a SPLIT y is multiplied by next_scale = the CONSUMER's in-multiplier vector (start of its scales / styles
 *   buffer, already folded), NULL = 1.  y_format = R3D_FMT_SPLIT_MX (Cout % 16 == 0): a SPLIT y whose lo plane holds the fp8 records
 *   the consumer's f16mx main loop reads (an R3D_SR_F16MX SynthesisBlock[NoUp], or the next r3d_conv_forward called with
 *   x_format = R3D_FMT_SPLIT_MX).  x_format = R3D_FMT_SPLIT_MX (ksize 3, Cin % 16 == 0): this conv's cross products run on the
 *   block-scaled fp8 MFMA (precision tier of R3D_SR_F16MX); r3d_conv_prepack writes both weight layouts, the input format selects.
 *   workspace (r3d_conv_workspace_bytes) is only used for non-SPLIT inputs. */
size_t r3d_conv_prepacked_bytes(int Cin, int Cout, int ksize);
size_t r3d_conv_workspace_bytes(int N, int Cin, int H, int W);
size_t r3d_conv_scales_bytes(int N, int Cin, int Cout);
int r3d_conv_prepack(const float* weight, int Cin, int Cout, int ksize, void* prepacked, r3d_stream_t stream);
int r3d_conv_forward(const void* prepacked, const void* scales, const float* bias,
                     int N, int Cin, int Cout, int H, int W, int ksize,
                     const void* x, int x_format, int act, float act_slope, float act_gain, float clamp,
                     void* y, int y_format, const float* next_scale, size_t next_scale_stride, float* y_absmax,
                     void* workspace, size_t workspace_bytes, r3d_stream_t stream);

/* Alpha / occlusion blend + channel concatenation, emitted as the SPLIT input of the next conv:
 *   y = cat([a * mask, b * (1 - mask)], dim=1),  a [N,Ca,H,W], b [N,Cb,H,W] (NCHW or CB8 fp32), mask [N,1,H,W]
 * replaces `torch.cat([x * head_torso_alpha, x_torso * (1 - head_torso_alpha)], dim=1)` and the person_occlusion / x_bg
 * twin in SuperresolutionHybrid8XDC_Warp.forward (modules/real3d/super_resolution/sr_with_ref.py:104,114,126,136).
 * y_split: [N][hi|lo][(Ca+Cb)/8][H][W][8] halfs, multiplied by next_scale ([N][Ca+Cb], the consumer's in-multiplier; NULL = 1);
 * y_format R3D_FMT_SPLIT, or R3D_FMT_SPLIT_MX (fp8 records in the lo plane) when the consumer runs the f16mx main loop (since 0.4.0).
 * Ca % 8 == Cb % 8 == 0, (Ca + Cb) % 16 == 0.  b = NULL (since 0.6.1, Ca % 16 == 0): only the `a` part is written, the planes still hold
 * (Ca + Cb) / 8 chunks -- the `b` part is the output of r3d_conv_forward_cat. */
int r3d_blend_cat_to_split(const float* a, int a_format, int Ca, const float* b, int b_format, int Cb, const float* mask,
                           int N, int H, int W, void* y_split, int y_format, const float* next_scale, size_t next_scale_stride,
                           r3d_stream_t stream);

/* A conv layer that writes its output as ONE PART of such a concatenation (since 0.6.1): channels [chan_off, chan_off + Cout) of the C_total-channel
 * SPLIT / SPLIT_MX tensor y_cat [N][hi|lo][C_total/8][H][W][8], every value times mask (mask_invert = 0) or 1 - mask (1) of its pixel and the
 * consumer's in-multiplier next_scale[chan_off + co] -- `x_torso = self.torso_encoder(hid)` followed by its half of
 * `torch.cat([x * alpha, x_torso * (1 - alpha)], dim=1)` (sr_with_ref.py:88,104) without the fp32 x_torso in between; the other part comes from
 * r3d_blend_cat_to_split called with b = NULL (which then writes only channels [0, Ca) of the Ca + Cb).  Bit-identical to the two-step form.
 * ksize = 1 (the 3x3 kernels sit at their register limit and do not carry this epilogue); Cout, chan_off, C_total multiples of 16; other
 * arguments as r3d_conv_forward (next_scale: the consumer's whole vector, indexed by the concatenated channel). */
int r3d_conv_forward_cat(const void* prepacked, const void* scales, const float* bias,
                         int N, int Cin, int Cout, int H, int W, int ksize,
                         const void* x, int x_format, int act, float act_slope, float act_gain, float clamp,
                         void* y_cat, int y_format, int C_total, int chan_off, const float* mask, int mask_invert,
                         const float* next_scale, size_t next_scale_stride,
                         void* workspace, size_t workspace_bytes, r3d_stream_t stream);

/* The same blend + concatenation FUSED into the 1x1 conv that consumes it (since 0.6.1):
 *   y = act(conv_1x1(cat([a * mask, b * (1 - mask)], dim=1), W) + bias)
 * = `x = torch.cat([x * person_occlusion, x_bg * (1 - person_occlusion)], dim=1); x = self.fuse_fg_bg_convs(x)` up to the first layer of
 * fuse_fg_bg_convs (modules/real3d/super_resolution/sr_with_ref.py:113-114 / :125-126, the Sequential of :56-62) -- and the head / torso twin
 * when that Sequential starts with a 1x1 conv.  The 512-channel operand is never written: the kernel blends, scales by the layer's in-multiplier
 * and splits while it stages (bit-identical to r3d_blend_cat_to_split followed by r3d_conv_forward; 134 MB read instead of 67 + 134 MB
 * written + 270 MB read at 256^2).  a [N,Ca/8,H,W,8], b [N,Cb/8,H,W,8] R3D_FMT_CB8 fp32, mask [N,1,H,W]; Ca % 8 == Cb % 8 == 0,
 * (Ca + Cb) % 64 == 0.  prepacked / scales / bias / act... / y... as r3d_conv_forward with ksize 1 and Cin = Ca + Cb; the in-multiplier a
 * conv layer's r3d_chain_fold writes is one power of two for all channels (element 0 of `scales` is read). */
int r3d_conv_forward_blend(const void* prepacked, const void* scales, const float* bias,
                           int N, int Ca, int Cb, int Cout, int H, int W,
                           const float* a, const float* b, const float* mask,
                           int act, float act_slope, float act_gain, float clamp,
                           void* y, int y_format, const float* next_scale, size_t next_scale_stride, float* y_absmax, r3d_stream_t stream);

/* Test hooks (added under ABI 0.8.0): which kernel variant, grid and block order the host picks for a conv layer call, without launching anything
 * (no GPU needed).  The launchers dispatch on the same structs these report (csrc/r3d_sr_launch.h sr_conv_variant / sr_block_variants), the
 * R3D_CONV_WINO mode of the process included.  A record is 6 ints {variant, bits, order, grid x, grid y, grid z}:
 *   variant  0 / 1 conv_mfma_f16x3_kernel<4,2,4> plain / MX (3x3, 16 x 16 tiles)    2 / 3 conv_mfma_f16x3_rows8_kernel plain / MX (8-row tiles)
 *            4 / 5 conv_wino_f16x3_kernel plain / MX    6 conv1x1_mfma_f16x3_kernel    7 conv1x1_blend_f16x3_kernel    8 upconv_fir_f16x3_kernel
 *   bits     variant 8: 4 CLAMP | 2 MX (the epilogue writes conv1's fp8 records) | 1 MXIN (the input carries fp8 records); else 0
 *   order    2: the XCD-aware block order, 0: grid order
 * r3d_debug_conv_variant: r3d_conv_forward / _cat (blend = 0; Cin, Cout unpadded, as passed there) or r3d_conv_forward_blend (blend = 1, Cin = Ca + Cb,
 *   ksize 1); out[6].  r3d_debug_sr_block_variants: r3d_sr_block_forward at R3D_SR_F16X3 | R3D_SR_F16MX; out[12] = conv0's record, conv1's record.
 * Both return R3D_ERR_INVALID_ARG for a call the entry point would refuse for its shape, formats or precision. */
int r3d_debug_conv_variant(int N, int Cin, int Cout, int H, int W, int ksize, int x_format, int blend, int* out);
int r3d_debug_sr_block_variants(int N, int Cin, int Cout, int Hin, int Win, int up, int x_format, int precision, float clamp, int* out);

/* torch.nn.UpsamplingBilinear2d(scale_factor=2) (align_corners=True), the resampling step inside to_plane_cnn
 * (modules/real3d/segformer.py:691-700), between two r3d_conv_forward layers: x fp32 channel-blocked [N,C/8,H,W,8] ->
 * y at 2H x 2W in R3D_FMT_CB8, R3D_FMT_SPLIT or R3D_FMT_SPLIT_MX (scaled by next_scale, NULL = 1; SPLIT_MX -- the consumer runs the f16mx
 * main loop -- needs C % 16 == 0).  C % 8 == 0. */
int r3d_upsample2x_bilinear(const float* x_cb8, int N, int C, int H, int W, void* y, int y_format,
                            const float* next_scale, size_t next_scale_stride, r3d_stream_t stream);

/* --- small image ops of the torso / background fusion forward (modules/real3d/super_resolution/sr_with_ref.py:67-137) --------------
 * r3d_resize_bilinear: torch.nn.functional.interpolate(x, size=(OH, OW), mode='bilinear', align_corners=False, antialias=A) on
 *   `planes` = N*C contiguous H x W planes (the 128 -> 256 / 512 -> 256 / occlusion resizes of :76-81,110,120).
 * r3d_blend: out = a * mask + b * (1 - mask), a, b [N,C,H,W], mask [N,1,H,W]  (`rgb * alpha + rgb_torso * (1 - alpha)` :103,113).
 * r3d_person_occlusion: clamp(torso_occlusion + where(alpha > head_threshold, 1, alpha), 0, 1)  (:107-112,117-122). */
int r3d_resize_bilinear(const float* x, int planes, int H, int W, float* y, int OH, int OW, int antialias, r3d_stream_t stream);
int r3d_blend(const float* a, const float* b, const float* mask, int N, int C, int H, int W, float* out, r3d_stream_t stream);
int r3d_person_occlusion(const float* alpha, const float* torso_occlusion, float head_threshold, size_t count, float* out,
                         r3d_stream_t stream);

/* --- output side --------------------------------------------------------------------------------
 * clamp(-1,1) -> (x+1)*127.5 -> uint8 HWC, the conversion real3d_infer.py:495-521 does on the host
 * after the frame loop; used to build the per-rank frame ring that is gathered over RCCL.
 * img [N,3,H,W] fp32 -> out [N,H,W,3] uint8. */
int r3d_frames_to_u8(const float* img, int N, int H, int W, uint8_t* out, r3d_stream_t stream);

/* --- frame gather over RCCL / xGMI ---------------------------------------------------------------------------
 * One process per GPU renders a contiguous chunk of the clip into a device-resident uint8 ring; r3d_gather_frames re-assembles the
 * clip on `root`: every rank sends `bytes_per_rank` bytes of `local`, the root receives world x bytes_per_rank into root_buf in rank
 * order (grouped ncclSend / ncclRecv on `stream`; no reduction, each peer uses its own xGMI link to the root).  The reference has
 * no counterpart: its frame loop is serial (inference/real3d_infer.py:480-492).
 *   r3d_comm_unique_id: rank 0 fills a 128-byte id that the caller ships to the other ranks (any side channel);
 *   r3d_comm_init: collective, on the calling thread's current HIP device.  RCCL is resolved with dlopen at first use (a copy that
 *   is already mapped, e.g. torch's, is reused); R3D_ERR_UNSUPPORTED if no librccl.so can be found. */
#define R3D_COMM_ID_BYTES 128
int r3d_comm_unique_id(void* id128);
int r3d_comm_init(const void* id128, int rank, int world, void** comm);
int r3d_comm_destroy(void* comm);
int r3d_gather_frames(void* comm, const uint8_t* local, size_t bytes_per_rank, uint8_t* root_buf, int root, r3d_stream_t stream);

/* Time a region with HIP events ON THE GIVEN STREAM (bench.py's roofline leg): returns elapsed ms
 * between two events; handles are opaque. */
int r3d_event_create(void** ev);
int r3d_event_record(void* ev, r3d_stream_t stream);
int r3d_event_elapsed_ms(void* start, void* stop, float* ms); /* synchronises on `stop` */
int r3d_event_destroy(void* ev);

/* --- per-kernel-family timing (bench.py's roofline leg) -------------------------------------------
 * When a family's bit is set in `mask`, every launch site of that family is bracketed by a HIP event pair
 * recorded on the launch stream.  r3d_profile_read() synchronises on the recorded events and returns the
 * summed duration and the number of bracketed launches since the last r3d_profile_reset(). */
enum r3d_prof_id {
    R3D_PROF_RENDER = 0,     /* render_kernel<..> (fused ray kernel)                       */
    R3D_PROF_CONV = 1,       /* conv_mfma_kernel (3x3 / transposed-conv implicit GEMM)     */
    R3D_PROF_UPCONV = 2,     /* up-sampling conv: fused transposed conv + FIR (f16x3); FIR (f32)  */
    R3D_PROF_TORGB = 3,      /* torgb_upsample_kernel                                      */
    R3D_PROF_PACK = 4,       /* SR weight modulation / packing kernels                     */
    R3D_PROF_LAYOUT = 5,     /* layout kernels (planes_to_nhwc, nchw<->cb8, frames_to_u8)  */
    R3D_PROF_MISC = 6,       /* raygen, limits, clamp, init                                */
    R3D_PROF_COUNT = 7
};
int r3d_profile_configure(uint32_t mask);
int r3d_profile_reset(void);
int r3d_profile_read(int id, double* total_ms, int* launches);
/* The shader clock the family's sampled kernels ran at since the last reset, in GHz (0 if none was sampled): one wave per launch of
 * render_kernel (RENDER), the plain 3x3 f16x3/f16mx conv (CONV) and the fused up-sampling conv (UPCONV) reads s_memtime and
 * s_memrealtime at its start and end -- cycles / ticks x hipDeviceAttributeWallClockRate.  The peaks bench.py prices against assume the
 * 2.4 GHz peak engine clock; under an MFMA-dense kernel the power management holds less.  `cycles` (optional): the summed s_memtime
 * cycles of the sampled waves.  Synchronises the device.  Sample with ONE stream (the start stamps are per family, not per launch). */
int r3d_profile_clock(int id, double* ghz, unsigned long long* cycles);

/* --- SECC encoder: SegFormerSECC2PlaneBackbone in mode b0, inference (ABI 0.7.0) ----------------------------------------------
 * The front half of the per-frame SECC-to-plane step (OSAvatarSECC_Img2plane.cal_plane_given_cano, modules/real3d/secc_img2plane.py:
 * 73-81 -> SegFormerSECC2PlaneBackbone.forward, modules/real3d/segformer.py:710-718): prenet, the MiT-b0 encoder and the SegFormerHead.
 * Exact fp32 (every product on the f32 MFMA).  Activations are token-major: [B, H, W, C] with token index h W + w.  All weights are the
 * reference's parameters as stored, except that conv weights [Cout, Cin, k, k] are passed as [Cout, k, k, Cin] (permuted once per
 * parameter version by the Python module) and the head's parameters are folded (r3d_secc_head).
 * Checked on the host before any launch (R3D_ERR_INVALID_ARG, the message naming the values): the sizes below, the overlap rule of each
 * entry point, and the 2^31 limit of a call: the GEMM kernels index token rows in int up to the end of the last 64-row tile, so "rows
 * below 2^31" means the row count rounded up to a multiple of 64. */

/* prenet (Conv2dLayer(in_dim, 3, 1), networks_stylegan2.py:139-190: weight * 1/sqrt(in_dim), + bias, linear) folded into the taps of
 * patch_embed1 (OverlapPatchEmbed, segformer.py:201-241: Conv2d(3, 32, 7, stride 4, padding 3), then LayerNorm eps 1e-5).
 * x [B, in_dim, H, W] NCHW (in_dim 9: pncc_cond_mode cano_src_tgt, 6: cano_tgt), prenet_w [3, in_dim], prenet_b [3], w [32, 7, 7, 3],
 * bias / ln_g / ln_b [32]; y [B, H/4, W/4, 32].  H and W must be multiples of 32 with (H/32)(W/32) <= 1024 (the attention's key limit).
 * y must not overlap x.  B (H/4)(W/4) rows below 2^31. */
int r3d_secc_embed1(const float* x, int B, int in_dim, int H, int W, const float* prenet_w, const float* prenet_b,
                    const float* w, const float* bias, const float* ln_g, const float* ln_b, float* y, r3d_stream_t stream);
/* Strided conv over [B, Hin, Win, Cin] -> [B, Ho, Wo, Cout], zero padding, w [Cout, ksize, ksize, Cin], bias [Cout], then (ln_g, ln_b
 * not NULL) LayerNorm over Cout with ln_eps.  patch_embed2..4 (segformer.py:201-241: k3 s2 p1, LayerNorm eps 1e-5) and the attention's
 * spatial reduction Attention.sr (:119-121, k = s = sr_ratio, no padding; its LayerNorm goes to the kv r3d_secc_linear instead).
 * 1 <= ksize <= 8, 0 <= pad < ksize, Hin + 2 pad >= ksize and Win + 2 pad >= ksize (as nn.Conv2d), Cin and Cout <= 1024 (so
 * ksize^2 Cin <= 2^16), B Ho Wo rows below 2^31; y must not overlap x. */
int r3d_secc_conv(const float* x, int B, int Hin, int Win, int Cin, const float* w, const float* bias, int Cout, int ksize,
                  int stride, int pad, const float* ln_g, const float* ln_b, float ln_eps, float* y, r3d_stream_t stream);
/* y[M, N] = act(LN?(x[M, K]) w[N, K]^T + bias) (+ residual): nn.Linear with an optional LayerNorm prologue (ln_g / ln_b both given, eps
 * ln_eps), exact-erf GELU (gelu != 0) and a residual [M, N] that may be y itself.  Attention.q / kv / proj (segformer.py:110-115,
 * 135-148), Block's norm1 / norm2 and residual adds (:195-196), Mlp.fc1 / fc2 (:68-71) and the head's folded low-resolution GEMMs.
 * bias may be NULL; K and N <= 4096, M rows below 2^31; y must not overlap x, nor the residual unless it is the residual. */
int r3d_secc_linear(const float* x, int M, int K, const float* ln_g, const float* ln_b, float ln_eps, const float* w,
                    const float* bias, int N, int gelu, const float* residual, float* y, r3d_stream_t stream);
/* nn.LayerNorm over the C entries of M rows (MixVisionTransformer.norm1..4, segformer.py:344-375).  y may be x itself, but must not
 * overlap it otherwise. */
int r3d_secc_layernorm(const float* x, int M, int C, const float* ln_g, const float* ln_b, float eps, float* y, r3d_stream_t stream);
/* softmax(q k^T * scale) v per head (Attention.forward, segformer.py:150-154): q [B, N, C], kv [B, L, 2C] with k in channels [0, C) and v
 * in [C, 2C), head h owns channels [32 h, 32 h + 32) (C = 32 heads), out [B, N, C].  1 <= L <= 1024, N rows below 2^31.  out must not
 * overlap kv; it may be q itself (each block reads its queries before it writes them) but must not overlap q otherwise. */
int r3d_secc_attention(const float* q, const float* kv, int B, int N, int L, int C, int heads, float scale, float* out, r3d_stream_t stream);
/* DWConv (segformer.py:394-404: depthwise 3x3, padding 1, bias) + nn.GELU (exact erf) on [B, H, W, C]; w [C, 1, 3, 3].  y must not
 * overlap x.  One thread an element, 256 a block: ceil(B H W C / 256) blocks below 2^31. */
int r3d_secc_dwconv_gelu(const float* x, int B, int H, int W, int C, const float* w, const float* bias, float* y, r3d_stream_t stream);
/* SegFormerHead.forward (segformer.py:512-537) after the fold: with W_fuse = linear_fuse.conv.weight [256, 1024] and block(i) its input
 * columns of _c_i in the order [_c4, _c3, _c2, _c1],  w1f = W_fuse[:, block(1)] . linear_c1.proj.weight [256, 32],  f2 / f3 / f4 the
 * folded maps c_i . (W_fuse[:, block(i)] . linear_ci.proj.weight)^T at [B, H1/2, W1/2, 256] / [B, H1/4, W1/4, 256] / [B, H1/8, W1/8,
 * 256],  hconst = sum_i W_fuse[:, block(i)] . linear_ci.proj.bias [256],  bn_scale / bn_shift the eval BatchNorm (eps 1e-5) as
 * gamma / sqrt(var + eps) and beta - mean * bn_scale.  out = relu(bn_scale (c1 . w1f^T + sum_i bilinear(f_i) + hconst) + bn_shift)
 * [B, 256, H1, W1] NCHW, the bilinear resize with align_corners=False.  c1 [B, H1, W1, 32]; H1, W1 multiples of 8 (H, W of 32).
 * out must not overlap any input.  B H1 W1 rows below 2^31. */
int r3d_secc_head(const float* c1, int B, int H1, int W1, const float* w1f, const float* f2, const float* f3, const float* f4,
                  const float* hconst, const float* bn_scale, const float* bn_shift, float* out, r3d_stream_t stream);

/* --- torso generator: the second half of the face-vid2vid torso network, inference (ABI 0.8.0) --------------------------------
 * WarpBasedTorsoModelMediaPipe.infer_forward_stage2 (modules/real3d/facev2v_warp/model2.py:329-336) = deform_based_generator, the
 * Generator of network2.py:248-301 (a trilinear warp of the appearance volume, then in_conv, mid_conv, six ResBlock2D, two UpBlock2D
 * and out_conv), and occlusion_2_predictor (model2.py:212-219, called at :262).  Exact fp32 (every product of the convolutions on the
 * f32 MFMA).  Activations are channel-last [B, H, W, C]; conv weights [Cout, Cin, k, k] are passed as [Cout, k, k, Cin] with spectral
 * norm and the eval BatchNorms folded in once per parameter version by the Python module (real3dportrait_amd/torso_generator.py). */

/* fs [N, C, D, H, W] -> out [N, D, H, W, C]: the source layout of r3d_torso_warp (the appearance features are constant over a clip;
 * the Python module caches this copy).  out must not overlap fs. */
int r3d_torso_volume_to_cl(const float* fs, int N, int C, int D, int H, int W, float* out, r3d_stream_t stream);
/* Generator.get_deformed_feature (network2.py:297-301): F.grid_sample(fs, grid, align_corners=True, padding_mode='border') of a 5-D
 * volume.  fs_cl [N, D, H, W, C] (r3d_torso_volume_to_cl), grid [N, Do, Ho, Wo, 3] with component 0 indexing W, 1 H, 2 D:
 * i = (g + 1) / 2 * (size - 1) clipped to [0, size - 1], trilinear over floor(i) and floor(i) + 1 (a corner equal to `size` has weight 0
 * and is not read).  NaN grid entries are not defined.  out: channel_last == 0: [N, C, Do, Ho, Wo], the reference's tensor before its
 * .view(N, C D, H, W); channel_last != 0: [N, Ho, Wo, C Do] with channel c Do + d, the same tensor as the next conv reads it.
 * out must not overlap an input. */
int r3d_torso_warp(const float* fs_cl, int N, int C, int D, int H, int W, const float* grid, int Do, int Ho, int Wo, float* out,
                   int channel_last, r3d_stream_t stream);
/* Stride-1 convolution, ksize 1, 3 or 7, zero padding ksize / 2 (nn.Conv2d(Cin, Cout, k, 1, k // 2)) over an Hs x Ws image, or
 * (upsample = 1) over its nearest x2 up-sampling, which is read through the tap addresses x[h >> 1, w >> 1] and never written
 * (UpBlock2D, layers.py:77-93).  x [B, Hs, Ws, Cin], or [B, Cin, Hs, Ws] with in_nchw != 0 (the predictor's concatenated input).
 * Prologue (pro_scale, pro_shift [Cin], both or neither): each tap is a = pro_scale[c] x + pro_shift[c], then a < 0 ? pro_slope a : a,
 * and 0 outside the image after that -- the BatchNorm + ReLU in front of the padded conv of a "NAC" block (ResBlock2D, layers.py:96-105).
 * w [Cout, ksize, ksize, Cin]; bias [Cout] or NULL.  Epilogue: v = sum + bias; act 0: none, 1: v < 0 ? act_slope v : v (ReLU: slope 0),
 * 2: sigmoid; then + residual [B, H, W, Cout] (may be y itself).  Outputs with H = Hs << upsample, W = Ws << upsample: y [B, H, W, Cout]
 * and / or y_nchw [B, Cout, H, W] (at least one).  Any Cin, Cout in 1 .. 4096; x, w and the prologue vectors are read 16 bytes at a time
 * when Cin % 4 == 0, the input is channel-last and they are 16-byte aligned.  Outputs must not overlap an input or each other. */
int r3d_torso_conv(const float* x, int B, int Hs, int Ws, int Cin, int in_nchw, int upsample, const float* pro_scale,
                   const float* pro_shift, float pro_slope, const float* w, const float* bias, int Cout, int ksize, int act,
                   float act_slope, const float* residual, float* y, float* y_nchw, r3d_stream_t stream);

/* --- torso motion field: the per-frame first half of the face-vid2vid torso network, inference (added under ABI 0.8.0) --------
 * MotionFieldEstimator.forward (modules/real3d/facev2v_warp/network2.py:204-236) and create_occlusion (:239-244), as
 * WarpBasedTorsoModelMediaPipe.forward calls it (model2.py:250).  Exact fp32.  Activations are channel-last [N, D, H, W, C]; Conv3d
 * weights [Cout, Cin, kd, kh, kw] are passed as [Cout, kd, kh, kw, Cin] with the eval BatchNorms folded in and the channel groups
 * padded to multiples of 4 (zero columns) once per parameter version by the Python module (real3dportrait_amd/torso_motion.py).
 * Grid components: 0 indexes W, 1 H, 2 D (func_utils.py:91-103). */

/* Stride-1 Conv3d with a cubic kernel, ksize 1, 3 or 7, zero padding ksize / 2 in depth, height and width (nn.Conv3d(Cin, Cout, k, 1,
 * k // 2): compress / the convs of DownBlock3D and UpBlock3D / tgt_head_fuser / mask_conv, network2.py:187-197), the same kernel as
 * r3d_torso_conv with a depth tap.  x [B, D, Hs, Ws, Cin]; w [Cout, ksize, ksize, ksize, Cin]; bias [Cout] or NULL.
 * upsample = 1: the conv runs over the nearest x2 up-sampling of H and W (not D), read through the tap addresses x[d, h >> 1, w >> 1] and
 *   never written (UpBlock3D: nn.Upsample(scale_factor=(1, 2, 2)), layers.py:77-93).
 * Epilogue: v = sum + bias; act 0: none, 1: v < 0 ? act_slope v : v, 2: sigmoid.
 * pool = 1: then the average of each 2 x 2 window of H and W (DownBlock3D: conv, BatchNorm, ReLU, nn.AvgPool3d((1, 2, 2)), layers.py:
 *   58-75); the un-pooled tensor is never written; an odd H or W is R3D_ERR_INVALID_ARG, and y_ncdhw must be NULL.
 * full_depth = 1: one output depth, the depth kernel spans all of D without padding, w [Cout, D, ksize, ksize, Cin]: nn.Conv2d(Cin D,
 *   Cout, k, 1, k // 2) on x.view(N, Cin D, H, W) of the NCDHW tensor (occlusion_conv / occlusion_conv2, network2.py:199-200,233,239-244),
 *   whose weight [Cout, Cin D, k, k] the caller passes as .view(Cout, Cin, D, k, k).permute(0, 2, 3, 4, 1).
 * Outputs, with H = Hs << upsample, W = Ws << upsample, Do = full_depth ? 1 : D: y, rows of y_cstride floats, one per (b, d, h, w) (per
 *   pooled position with pool = 1), of which this conv writes channels [y_coffset, y_coffset + Cout) and leaves the others untouched (a
 *   slice of a concatenation); and / or y_ncdhw [B, Cout, Do, H, W].  Any Cin, Cout in 1 .. 4096, D <= 1024; x and w are read 16 bytes
 *   at a time when Cin % 4 == 0 and they are 16-byte aligned.  Outputs must not overlap an input or each other. */
int r3d_torso_conv3d(const float* x, int B, int D, int Hs, int Ws, int Cin, int upsample, const float* w, const float* bias,
                     int Cout, int ksize, int full_depth, int act, float act_slope, int pool, float* y, int y_cstride,
                     int y_coffset, float* y_ncdhw, r3d_stream_t stream);
/* The hourglass input (network2.py:205-214; func_utils.py:139-191): compress (nn.Conv3d(C, 4, 1)), create_heatmap_representations,
 * create_sparse_motions and create_deformed_source_image in one pass.  fs_cl [N, D, H, W, C] (r3d_torso_volume_to_cl), compress_w [4, C],
 * compress_b [4], kp_s / kp_d [N, K, 3], J [N, 3, 3] = Rs Rd^-1.  For voxel p with grid point g and k = 0 .. K: the sparse motion is
 * s = g (k = 0) or J (g - kp_d[k-1]) + kp_s[k-1]; channel 5 k of the output is exp(-|g - kp_d[k-1]|^2 / 0.02) - exp(-|g - kp_s[k-1]|^2
 * / 0.02) (0 for k = 0), channels 5 k + 1 .. 5 k + 4 are F.grid_sample(compressed, s, align_corners=True, padding_mode='zeros'): trilinear,
 * a corner outside the volume contributes 0.  inp [N, D, H, W, inp_channels], inp_channels >= 5 (K + 1), the channels from 5 (K + 1) on
 * written 0; fuse (or NULL): the same inp_channels channels at the start of rows of fuse_cstride floats.  D, H, W >= 2, K <= 64. */
int r3d_torso_motion_input(const float* fs_cl, int N, int C, int D, int H, int W, const float* compress_w, const float* compress_b,
                           const float* kp_s, const float* kp_d, const float* J, int K, float* inp, int inp_channels, float* fuse,
                           int fuse_cstride, r3d_stream_t stream);
/* deformation = sum_k softmax_k(mask) sparse_motion_k (network2.py:227-231): mask [N, D, H, W, K + 1] (mask_conv's logits), the sparse
 * motions recomputed as in r3d_torso_motion_input; out [N, D, H, W, 3], the grid r3d_torso_warp reads. */
int r3d_torso_motion_deform(const float* mask, int N, int D, int H, int W, int K, const float* kp_s, const float* kp_d, const float* J,
                            float* out, r3d_stream_t stream);
/* tgt_head_feats.unsqueeze(2).repeat(1, 1, D, 1, 1) into its slice of the fuser's input (network2.py:224): feats [N, C, H, W] ->
 * channels [fuse_coffset, fuse_coffset + C) of fuse [N, D, H, W, fuse_cstride]. */
int r3d_torso_motion_broadcast(const float* feats, int N, int C, int H, int W, int D, float* fuse, int fuse_cstride, int fuse_coffset,
                               r3d_stream_t stream);

/* --- a second precision tier for the torso convolutions (added under ABI 0.8.0; opt-in, the entry points above are unchanged) -------
 * r3d_torso_conv_prec / r3d_torso_conv3d_prec take the argument lists of r3d_torso_conv / r3d_torso_conv3d with `precision` in front of
 * `stream`; argument checks, overlap rules and everything outside the products (prologue, zero padding, bias, activation, residual, pool,
 * slices, output layouts, tile selection) are those functions'.  Any other precision is R3D_ERR_INVALID_ARG.
 *   R3D_TORSO_F32     the kernels of r3d_torso_conv / r3d_torso_conv3d, bit-identical to them.
 *   R3D_TORSO_BF16X3  every staged activation (after the prologue and the zero outside the image) and every staged weight is split into
 *     three bf16 pieces, x = h + m + l exactly: h = bf16(clamp(x, +-0x7f7f0000)), m = bf16(x - h), l = bf16(x - h - m), round to nearest
 *     even (the clamp keeps values that would round to infinity finite; both subtractions are exact in fp32).  Per 32 k entries six piece
 *     products are added on v_mfma_f32_16x16x32_bf16 to the fp32 accumulator in the fixed order
 *         xl wh, xh wl, xm wm, xm wh, xh wm, xh wh      (x: activation, w: weight)
 *     and the three below 2^-25 |x| |w| (xl wm, xm wl, xl wl) are left out.  The accumulator, the order of the k steps and of the k entries
 *     inside a step are the exact tier's, so the result is fp32-class (same test bound as the exact kernels) and, like theirs, depends on
 *     nothing but the operands: bit-identical across batch sizes, runs and streams.  bf16 has fp32's exponent range: there is no range
 *     fold, no scale and no per-tensor state, and operands up to fp32 max are split exactly.  Pieces below bf16's smallest normal are read
 *     as zero, so for |x| below about 2^-110 the value degrades to two, then one piece (relative accuracy 2^-16, 2^-8).  A non-finite
 *     operand gives a non-finite (possibly NaN where the exact tier gives an infinity) result.  Weights stay fp32 in memory. */
#define R3D_TORSO_F32 0
#define R3D_TORSO_BF16X3 1
int r3d_torso_conv_prec(const float* x, int B, int Hs, int Ws, int Cin, int in_nchw, int upsample, const float* pro_scale,
                        const float* pro_shift, float pro_slope, const float* w, const float* bias, int Cout, int ksize, int act,
                        float act_slope, const float* residual, float* y, float* y_nchw, int precision, r3d_stream_t stream);
int r3d_torso_conv3d_prec(const float* x, int B, int D, int Hs, int Ws, int Cin, int upsample, const float* w, const float* bias,
                          int Cout, int ksize, int full_depth, int act, float act_slope, int pool, float* y, int y_cstride,
                          int y_coffset, float* y_ncdhw, int precision, r3d_stream_t stream);
/* The split of R3D_TORSO_BF16X3, by the device function the convolutions' staging calls: h[i], m[i], l[i] = the 16 bits of the pieces of
 * x[i] (a piece as fp32 is its bits << 16), i < n, 1 <= n < 2^31.  For tests (real3dportrait_amd/torso_precision.py:split_bf16x3 is its
 * host mirror).  The outputs must not overlap x or each other. */
int r3d_torso_split_bf16x3(const float* x, size_t n, uint16_t* h, uint16_t* m, uint16_t* l, r3d_stream_t stream);

/* --- torso appearance extractor: the third module of the face-vid2vid torso network, inference (added under ABI 0.8.0) -------------
 * AppearanceFeatureExtractor.forward (modules/real3d/facev2v_warp/network2.py:38-45), as WarpBasedTorsoModelMediaPipe.forward calls it on
 * every frame (model2.py:230).  in_conv is r3d_torso_conv_prec; the three functions below are the rest.  They run the 3-D body of
 * r3d_torso_conv3d (a 2-D layer as one depth with ONE depth tap, K = ksize ksize Cin) and sum in its order: with pool = 0 / depth = 1 /
 * no prologue and no residual each equals r3d_torso_conv_prec / r3d_torso_conv3d_prec bit for bit, on both tiers.  `precision` is
 * R3D_TORSO_F32 or R3D_TORSO_BF16X3 as above; anything else is R3D_ERR_INVALID_ARG.  Weights [Cout, Cin, k, k] / [Cout, Cin, k, k, k]
 * are passed as [Cout, k, k, Cin] / [Cout, k, k, k, Cin] with the eval BatchNorms folded in once per parameter version by the Python
 * module (real3dportrait_amd/torso_appearance.py).  Any Cin, Cout in 1 .. 4096; x, w and the prologue vectors are read 16 bytes at a
 * time when Cin % 4 == 0, the input is channel-last and they are 16-byte aligned.  All arguments are checked before any launch. */

/* DownBlock2D (layers.py:58-69: conv 3 x 3, BatchNorm, ReLU, nn.AvgPool2d((2, 2))): the stride-1 convolution of r3d_torso_conv
 * (ksize 1, 3 or 7, zero padding ksize / 2; x [B, Hs, Ws, Cin], or [B, Cin, Hs, Ws] with in_nchw != 0; w [Cout, ksize, ksize, Cin];
 * bias [Cout] or NULL; v = sum + bias; act 0: none, 1: v < 0 ? act_slope v : v, 2: sigmoid), then with pool = 1 the average of each
 * 2 x 2 window, 0.25 ((v00 + v01) + (v10 + v11)) -- after the activation, so it cannot go into the weights.  The un-pooled tensor is
 * never written.  y [B, Hs >> pool, Ws >> pool, Cout].  pool = 1 with an odd Hs or Ws is R3D_ERR_INVALID_ARG.  y must not overlap x,
 * w or bias. */
int r3d_torso_conv_pool(const float* x, int B, int Hs, int Ws, int Cin, int in_nchw, const float* w, const float* bias, int Cout,
                        int ksize, int act, float act_slope, int pool, float* y, int precision, r3d_stream_t stream);
/* mid_conv followed by x.view(N, C, D, H, W) (network2.py:41-43): the same convolution with a depth-split store.  Cout = C depth.  The
 * caller passes the weight rows (and the bias) DEPTH-MAJOR: row d C + c is the reference's output channel c depth + d
 * (weight.view(C, depth, Cin, k, k).transpose(0, 1)), so that a lane group stores a contiguous run of C.  Row d C + c of position
 * (b, h, w) lands at y[b, d, h, w, c] of the channel-last volume y [B, depth, Hs, Ws, C], the layout r3d_torso_conv3d_res reads;
 * exactly B depth Hs Ws C floats are written, there is no [B, H, W, C depth] intermediate and no transpose launch.  depth = 1 is the
 * plain convolution.  depth < 1 or Cout % depth != 0 is R3D_ERR_INVALID_ARG.  y must not overlap x, w or bias. */
int r3d_torso_conv_split(const float* x, int B, int Hs, int Ws, int Cin, int in_nchw, const float* w, const float* bias, int Cout,
                         int ksize, int act, float act_slope, int depth, float* y, int precision, r3d_stream_t stream);
/* The convolutions of ResBlock3D (layers.py:96-115: x + NAC(NAC(x)), each NAC = BatchNorm, ReLU, nn.Conv3d(C, C, 3, 1, 1)): the
 * stride-1 Conv3d of r3d_torso_conv3d (cubic kernel, ksize 1, 3 or 7, zero padding ksize / 2 in depth, height and width; x [B, D, Hs,
 * Ws, Cin]; w [Cout, ksize, ksize, ksize, Cin]; bias [Cout] or NULL) with
 *   a prologue (pro_scale, pro_shift [Cin], both or neither): each tap is a = pro_scale[c] x + pro_shift[c], then a < 0 ? pro_slope a : a,
 *     and 0 outside the volume AFTER that, in depth as well as in height and width (the reference pads the activated tensor);
 *   the epilogue v = sum + bias; act as above; then + residual [B, D, Hs, Ws, Cout] (or NULL), which may be y itself.
 * Outputs: y [B, D, Hs, Ws, Cout] and / or y_ncdhw [B, Cout, D, Hs, Ws] (at least one), both writable from one launch.  Outputs must
 * not overlap an input (other than residual == y) or each other. */
int r3d_torso_conv3d_res(const float* x, int B, int D, int Hs, int Ws, int Cin, const float* pro_scale, const float* pro_shift,
                         float pro_slope, const float* w, const float* bias, int Cout, int ksize, int act, float act_slope,
                         const float* residual, float* y, float* y_ncdhw, int precision, r3d_stream_t stream);

/* --- torso forward glue: what WarpBasedTorsoModelMediaPipe.forward does between its three modules, inference (added under ABI 0.8.0) ----
 * modules/real3d/facev2v_warp/model2.py:226-236, fp32.  Both functions resize two channels c0, c1 (2 and 4 in the reference) of
 * segmap [N, Cs, Hs, Ws] with the semantics of F.interpolate(mode='bilinear', align_corners=False, antialias=False):
 * src = max((dst + 0.5) in / out - 0.5, 0), the upper neighbour clamped at the edge.  c0 or c1 outside 0 .. Cs - 1 is
 * R3D_ERR_INVALID_ARG.  A NaN in the segmap is not defined.  All arguments are checked before any launch. */

/* model2.py:226-228, in_conv's input in rgb_alpha mode: out [N, Ci + 2, OH, OW] = cat(img [N, Ci, OH, OW], resize(segmap[:, [c0, c1]],
 * (OH, OW))), NCHW.  The image channels are copied bit for bit; Ci = 0 (img may then be NULL) gives the resized pair alone.  out must not
 * overlap img or segmap. */
int r3d_torso_seg_input(const float* img, int N, int Ci, const float* segmap, int Cs, int Hs, int Ws, int c0, int c1, float* out, int OH,
                        int OW, r3d_stream_t stream);
/* model2.py:231-236 in one launch, on the channel-last volume feats_cl [N, D, H, W, C] (r3d_torso_conv3d_res's y):
 *   seg = resize(segmap[:, [c0, c1]], (H, W));  mask = seg0 + seg1;  mask_d = the maximum of mask over the ksize x ksize window with
 *   `reflect` indexing at the border (utils/commons/image_utils.py:10-15: F.pad(mode='reflect') + max_pool2d): ksize odd and
 *   (ksize - 1) / 2 < min(H, W), reflect padding's own condition, anything else is R3D_ERR_INVALID_ARG (as is a ksize above 117, whose
 *   window does not fit a tile's LDS);
 *   masked_cl [N, D, H, W, C] = feats_cl mask_d (mul_mask != 0) or a copy of feats_cl (mul_mask == 0): the source layout of r3d_torso_warp;
 *   motion_cl [N, D, H, W, C + 2] = the same values followed by seg0, seg1, repeated over depth: what r3d_torso_volume_to_cl of the
 *   reference's torch.cat would hold, the fs_cl of r3d_torso_motion_input.
 * masked_cl may be feats_cl itself (each element is read, then written, by one lane); any other overlap between an output and an input
 * or the other output is R3D_ERR_INVALID_ARG.  The resize and the dilation are computed once per pixel tile and run of depth slices,
 * not per voxel; the volume is read and written 16 bytes at a time when C % 4 == 0 and the pointers are 16-byte (motion_cl: 8-byte)
 * aligned. */
int r3d_torso_mask_volume(const float* feats_cl, int N, int D, int H, int W, int C, const float* segmap, int Cs, int Hs, int Ws, int c0,
                          int c1, int ksize, int mul_mask, float* masked_cl, float* motion_cl, r3d_stream_t stream);

/* --- mesh rasteriser: the SECC map's z-buffer rasterisation and attribute interpolation, inference (added under ABI 0.8.0) -------------
 * MeshRenderer.forward (deep_3drecon/util/mesh_renderer.py:53-130) as SECC_Renderer configures it: pytorch3d's rasteriser with
 * image_size = S, blur_radius = 0, faces_per_pixel = 1, cull_backfaces = False under FoVPerspectiveCameras(fov, znear, zfar), identity
 * pose, aspect 1.  The rule is restated from pytorch3d's naive rasteriser (tests/raster_ref64.py is the fp64 restatement);
 * equality with pytorch3d rests on that restatement and has not been measured.  fp32.
 *   vertex [B, N, 3] camera space, read only (negate_x != 0: x is negated on the fly, as mesh_renderer.py:69-71 does on its copy);
 *   tri [M, 3] (tri_batched = 0) or [B, M, 3] (tri_batched != 0), int32; feat [B, N, C], 1 <= C <= 4, or NULL together with image.
 *   Projection x_ndc = s x / z, y_ndc = s y / z, s = 1 / tan(fov / 2); pixel (row i from the top, column j from the left) has
 *   y_ndc = -1 + (2 (S - 1 - i) + 1) / S and x_ndc = -1 + (2 (S - 1 - j) + 1) / S.  A pixel is covered by a face iff its three
 *   barycentrics (areas over area + 1e-8, faces with |area| <= 1e-8 skipped) are STRICTLY positive, either winding; the depth is the
 *   perspective-corrected camera-space z, the smallest wins, the lower face index on an exact tie: deterministic, run to run and stream
 *   to stream.
 *   pix_to_face [B, S, S] int64 (may be NULL): the packed index b M + f, or -1.
 *   mask [B, 1, S, S] = pix_to_face > 0 with first_face_is_background != 0 -- the reference's own test (mesh_renderer.py:116), which
 *     turns face 0 of the batch's first mesh into background -- or pix_to_face >= 0 with 0.
 *   depth [B, 1, S, S] = mask pz; image [B, C, S, S] = (mask sum_k b_k feat[tri[f, k]]) out_scale + out_shift with the
 *   perspective-corrected barycentrics b_k (1, 0: the reference; 2, -1: SECC_Renderer's (x - 0.5) / 0.5 of secc_renderer.py:52 folded
 *   in).  Empty pixels are -1 / 0 / 0 / out_shift.  The barycentrics themselves are not stored.
 * Difference from pytorch3d, on input SECC_Renderer cannot produce (faces at z = 10 +- 1.5, znear = 5): a face with a vertex at
 * z < znear / 2 (or z <= 0) is DROPPED where pytorch3d clips it, as is a face with a non-finite vertex or projection or an index
 * outside [0, N); nothing is read out of bounds on such input.
 * Limits, refused with R3D_ERR_INVALID_ARG before any launch: NULL vertex / tri / mask / depth, feat without image or the reverse,
 * S outside 1 .. 16384, C outside 1 .. 4, B M >= 2^31, B S S >= 2^31, fov_deg not finite or not in (0, 180); R3D_ERR_WORKSPACE: a
 * workspace that is NULL, not 8-byte aligned or smaller than r3d_raster_workspace_bytes(B, S, M) (0 for sizes the call refuses).  The
 * workspace needs no initialisation and carries nothing between calls (one async memset per call clears the keys); two calls in
 * flight on different streams need a workspace each. */
size_t r3d_raster_workspace_bytes(int B, int S, int M);
int r3d_raster_forward(const float* vertex, const float* feat, const int32_t* tri, int tri_batched, int B, int N, int M, int C, int S,
                       float fov_deg, float znear, int negate_x, int first_face_is_background, float out_scale, float out_shift,
                       int64_t* pix_to_face, float* mask, float* depth, float* image, void* workspace, size_t workspace_bytes,
                       r3d_stream_t stream);

/* --- blink edit of SECC maps, inference (added under ABI 0.8.0) --------------------------------------------------------------------------
 * blink_eye_for_secc (inference/edit_secc.py:47-129) for F selected frames of a clip secc [T, 3, H, W] fp32 in [-1, 1], as the blink loop
 * of inference/real3d_infer.py:411-426 applies it, on the device: no host round trip and no kd-tree (DESIGN 4.15 states the rule;
 * tests/blink_ref.py is its NumPy restatement).  Per listed frame k: map frame_idx[k] with close_eye_percent percent[k] is quantised to
 * 8 bits, q = trunc(((x + 1) / 2) 255), and comes back as q / 127.5 - 1; for percent > 0 the eye holes found in the two prior regions are
 * closed from above and below by copying, to each pixel to close, the colour of the nearest face pixel that lies more than 5 pixels away
 * from every hole pixel.
 *   Differences from the reference: (1) on a distance tie the face pixel with the lowest (row, column) is taken, where the reference
 *   takes whatever its kd-tree returns (3 to 16 % of the edited pixels on the test maps; everywhere else the result is bit-identical);
 *   (2) NaN and values outside [-1, 1] quantise to 0 .. 255 by clamping; (3) maps on which the reference raises ValueError come back
 *   quantised only, with a status.
 *   frame_idx [F] int32, percent [F] double, status [F] int32: DEVICE arrays.  status[k] = 0 done; 1 no eye pixel in one of the prior
 *   regions; 2 no face pixel left around the eyes; 3 frame_idx[k] outside [0, T) or percent[k] outside [0, 1] (NaN included): that
 *   frame is neither read nor written.
 *   out [T, 3, H, W] may be secc itself (in place).  Only the listed frames are written, in place or not: with out != secc the caller
 *   copies whatever else out should hold.  Listing a frame twice is the caller's error (the result of that frame is then undefined,
 *   nothing is accessed out of bounds).
 * The result is a pure function of the input: run to run and stream to stream bit-identical.  No host synchronisation and no allocation.
 * Refused before any launch, R3D_ERR_INVALID_ARG: a NULL pointer, H or W outside 16 .. 4096, T < 1, F < 1, F > T, F > 65535;
 * R3D_ERR_WORKSPACE: a workspace that is NULL, not 8-byte aligned or smaller than r3d_secc_blink_workspace_bytes(F, H, W) (0 for sizes
 * the call refuses).  The workspace needs no initialisation and carries nothing between calls; two calls in flight on different
 * streams need a workspace each. */
size_t r3d_secc_blink_workspace_bytes(int F, int H, int W);
int r3d_secc_blink(const float* secc, int T, int H, int W, const int32_t* frame_idx, const double* percent, int F, float* out,
                   int32_t* status, void* workspace, size_t workspace_bytes, r3d_stream_t stream);

/* --- morphable face model: the vertices of the SECC meshes and the 2D landmarks, inference (added under ABI 0.8.0) ----------------------
 * r3d_face_vertex is ParametricFaceModel.compute_face_vertex (deep_3drecon/deep_3drecon_models/bfm.py:332-347), r3d_face_landmarks is
 * Face3DHelper.reconstruct_lm2d (data_util/face3d_helper.py:132-169): the same arithmetic on the L key rows plus the projection.  fp32
 * (tests/face_model_ref64.py is the fp64 restatement).  Arrays in the reference's own layouts, nothing is repacked:
 *   mean [3 N]; id_base [3 N, Ki] and exp_base [3 N, Ke] row-major (row 3 n + c is component c of vertex n); id [T, Ki], exp [T, Ke],
 *   euler [T, 3] in radians, trans [T, 3]; vertex [T, N, 3], the layout r3d_raster_forward reads; lm2d [T, L, 2].
 * Per frame t and vertex n:
 *   p = (id_base[3 n .., :] . id[t] + exp_base[3 n .., :] . exp[t]) + mean[3 n ..]: per row one chain of fused multiply-adds from +0.0f,
 *       in this order: k = 0 .. Ki - 1 of the identity, then k = 0 .. Ke - 1 of the expression; then one addition of the mean (last, as
 *       bfm.py:114 adds it: the chain rounds at the size of its own sum, not at the mean's);
 *   q = M p + trans[t] with M = Rz Ry Rx of compute_rotation (bfm.py:204-238; the reference writes p @ (Rz Ry Rx)^T);
 *   q.z = camera_distance - q.z when to_camera != 0.
 * The landmarks continue with the projection of perspective_projection(focal, center): x' = (focal q.x + center q.z) / q.z, likewise
 * y', then y' = image_size - y', and both are divided by image_size (the reference: 1015, 112, 224, camera_distance 10).
 *   exp, euler or trans may be NULL, meaning zeros: the result is bit-identical to passing arrays of +0.0f.  Ke = 0 is allowed (exp_base
 *   and exp are then ignored).
 * A frame's result depends on that frame's inputs only: not on T, not on the other frames of the call.  A frame computed alone and as
 * frame 37 of 51 is bit-identical, so a clip does not depend on how it is cut into chunks.  Run to run and stream to stream
 * bit-identical; no allocation, no workspace, no host synchronisation.  Inputs are never written.  Any 4-byte-aligned pointer and any
 * Ki, Ke are accepted; 16-byte loads are used for a base whose pointer is 16-byte aligned and whose K is a multiple of 4.
 * Refused before any launch with R3D_ERR_INVALID_ARG: NULL mean / id_base / id / output; exp_base NULL while Ke > 0; N (L) or T < 1;
 * Ki < 1, Ke < 0 or Ki + Ke > 512; 3 N T >= 2^31; camera_distance not finite; for the landmarks focal, center or image_size not
 * finite, focal <= 0 or image_size <= 0; an output that overlaps an input. */
int r3d_face_vertex(const float* mean, const float* id_base, const float* exp_base, int N, int Ki, int Ke, const float* id,
                    const float* exp, const float* euler, const float* trans, int T, float camera_distance, int to_camera,
                    float* vertex, r3d_stream_t stream);
int r3d_face_landmarks(const float* key_mean, const float* key_id_base, const float* key_exp_base, int L, int Ki, int Ke,
                       const float* id, const float* exp, const float* euler, const float* trans, int T, float camera_distance,
                       int to_camera, float focal, float center, float image_size, float* lm2d, r3d_stream_t stream);

/* --- per-clip conditions: the camera trajectory and the smoothed key points, inference (added under ABI 0.8.0) ----------------------------
 * Declared in the companion header next to this one, which this header includes: a program that includes r3d_hip.h sees them. */
#include "r3d_hip_clip.h"

/* --- the clip's output video frames, out_mode 'concat_debug', inference (added under ABI 0.8.0) -----------------------------------------------
 * Declared in the companion header next to this one, which this header includes: a program that includes r3d_hip.h sees them. */
#include "r3d_hip_video.h"

/* --- the source image's head, torso and background: the frame loop's conditions, inference (added under ABI 0.8.0) ---------------------------
 * Declared in the companion header next to this one, which this header includes: a program that includes r3d_hip.h sees them. */
#include "r3d_hip_source.h"

/* --- audio to motion: the VAE between the audio features and the expression coefficients, inference (added under ABI 0.8.0) ------------------
 * Declared in the companion header next to this one, which this header includes: a program that includes r3d_hip.h sees them. */
#include "r3d_hip_audio.h"

/* --- fit the morphable model to 2-D landmarks: the Adam loops, data generation (added under ABI 0.8.0) ---------------------------------------
 * Declared in the companion header next to this one, which this header includes: a program that includes r3d_hip.h sees them. */
#include "r3d_hip_fit.h"

#ifdef __cplusplus
}
#endif
#endif /* R3D_HIP_H */
