/*
 * r3d_hip_source.h -- companion header of r3d_hip.h (C ABI of libr3d_hip.so): the source image's head, torso and background.  r3d_hip.h
 * includes it; it can also be included on its own.  The Python binding table of this header is real3dportrait_amd/_lib.py SIGNATURES.
 */
#ifndef R3D_HIP_SOURCE_H
#define R3D_HIP_SOURCE_H

#include "r3d_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* --- the frame loop's conditions from the source image and its segmap, inference (added under ABI 0.8.0) ---------------------------------
 * What prepare_batch_from_inp builds on the host once per clip (inference/real3d_infer.py:244-260), on the device (DESIGN 4.19;
 * tests/source_conditions_ref.py is the restatement in NumPy): MediapipeSegmenter._seg_out_img_with_segmap(mode='head'),
 * inpaint_torso_job and extract_background(..., 'knn') (data_gen/utils/process_video/extract_segment_imgs.py:63-239).  Same conventions
 * as r3d_hip.h: borrowed device pointers, contiguous arrays, `stream` a hipStream_t, 0 or a negative r3d_status, the message from
 * r3d_last_error().  Images are uint8 [H, W, 3]; a segmap is uint8 [6, H, W], one plane per class (0 background, 1 hair, 2 body skin
 * = neck, 3 face skin, 4 clothes = torso, 5 others), a pixel belonging to a class where its byte is not 0.  All work is on uint8 and
 * int32: every output byte is a pure function of the inputs, with no floating-point atomics, bit-identical from run to run, from stream
 * to stream and however frames are grouped into calls.  No call synchronises with the host; inputs are never written.
 *
 * r3d_source_nearest: the exact nearest-seed transform.  mask [B, H, W], a seed where the byte is not 0.  For every pixel (r, x) of every
 *   frame: d2 [B, H, W] int32 the squared Euclidean distance to the nearest seed of its frame and index [B, H, W] int32 that seed's
 *   row * W + col; among equidistant seeds the one with the lowest (row, col), the rule of r3d_secc_blink.  d2 or index may be NULL (not
 *   wanted).  Two launches.  The column pass, a lane per (frame, column, one of 8 row segments), walks down and up and stores per pixel
 *   the row of the nearest seed of its own column, the one above on a tie (-1: a column without a seed); the segments are joined in LDS.  The row pass, a block per row and 256 pixels, stages
 *   the row's W candidates in LDS and takes per pixel the minimum over the columns c of the 64-bit key
 *       (d2 << 32) | (seed row << 11) | c,        d2 = (x - c)^2 + (seed row - r)^2,
 *   which orders by distance, then row, then column; H and W may be 1 .. R3D_SOURCE_MAX_SIDE = 2048 (11 bits each; d2 < 2^23).  A
 *   column's only candidates at its own minimum distance are its nearest seed above and below, and the one above has the lower row, so
 *   the minimum over the columns' candidates is the lexicographic minimum over all seeds.  A frame without a seed sets
 *   status word 0 and gets d2 = INT32_MAX, index = -1.
 * r3d_source_background: extract_background(img_lst, segmap_mask_lst, 'knn') (:105-146) for the B >= 1 frames the caller has selected
 *   (the sub-sampling of :91-103 is the caller's).  img [B, H, W, 3]; bg [B, H, W], segmap plane 0 of each frame.  (1) per frame the
 *   transform with the pixels that are NOT background as seeds; (2) per pixel the largest d2 over the frames and the first frame that
 *   reaches it (np.argmax); (3) a pixel is surely background where that d2 > 100, the reference's max_dist > 10 in integers; (4) it
 *   takes its colour from that frame; (5) a second transform with the sure pixels as seeds; (6) every other pixel copies the colour of
 *   its nearest sure pixel -- the lowest (row, col) among equidistant ones, where the reference takes whatever its kd-tree returns.
 *   out [H, W, 3].  Six launches and one 8-byte memset.
 * r3d_source_torso: inpaint_torso_job(img, segmap) (:148-239) in its order.  head = classes 1 | 3 | 5; the image is copied and its head
 *   pixels set to 0.  Torso paint: per column the top pixel of class 4, kept if the pixel above it is head; L = 9 rows upward from it,
 *   itself included, get uint8(colour * darken[k]), k the distance in rows, the colour that of the UNEDITED image at the top pixel, the
 *   product in fp64, truncated.  Neck paint: the class-2 mask dilated by 3 rows up and down (binary_dilation, 3 x 1, 3 iterations, zero
 *   border); per column its top pixel and its pixel COUNT ucnt; kept if the pixel above the top is head; the top pushed down by
 *   min(ucnt - 1, 4); L = 53 rows upward painted the same way, over the torso paint.  darken: R3D_SOURCE_DARKEN = 53 doubles on the HOST,
 *   NumPy's 0.98 ** arange(53) (no pow on the device).  Blur: inside the neck paint mask the pixel is replaced by the 5 x 5 blur of the
 *   painted image, border reflect-101, as separable fixed point: blur_weights, 5 ints on the HOST with 8 fractional bits (each 0 ..
 *   256, their sum at most 256), a 16-bit horizontal sum, a vertical sum rounded half up, (v + 2^15) >> 16.  The default
 *   (48, 53, 54, 53, 48) is exp(-x^2 / 32) normalised and rounded: the reference calls cv2.GaussianBlur(img, (5, 5), cv2.BORDER_DEFAULT),
 *   whose third argument is sigmaX, so sigma = 4.  This models OpenCV's 8-bit path; EQUALITY WITH cv2 HAS NOT BEEN MEASURED (cv2 is on
 *   no machine this project is built on), which is why the weights are an argument.  The four returns of :227-239 as they are:
 *   torso_img [H, W, 3] (zero outside torso_mask), torso_mask [H, W] bytes 0 / 1 = dilated neck | torso | neck paint | torso paint,
 *   with_bg_img [H, W, 3] (never masked) and with_bg_mask [H, W] = background | torso_mask.  Deviations: paint rows above row 0 are not
 *   written (NumPy's negative indices wrap them to the bottom of the image), and a column whose top pixel is in row 0 is not under
 *   head (the reference reads the bottom row).  Three launches: columns, paint, blur and masks.
 * r3d_source_select: MediapipeSegmenter._seg_out_img_with_segmap (mp_segmenter.py:230-256): out [H, W, 3] the image with every pixel outside
 *   the classes of the bit mask `classes` at 0 (bit k: class k; R3D_SOURCE_HEAD_CLASSES = 42 is mode 'head', classes 1, 3 and 5) and
 *   mask [H, W] (may be NULL) bytes 0 / 1, the selection.  One launch.
 * r3d_source_to_planes: uint8 [H, W, 3] -> fp32 [3, H, W], (float(x) - 127.5f) / 127.5f with IEEE division, torch's (t - 127.5) / 127.5.
 *   segmap NULL: every pixel; otherwise a pixel outside the classes of the bit mask `classes` (bit k: class k; 42 = head) counts as
 *   byte 0, i.e. -1.  One launch.
 *
 * Output bytes are written as dwords, a lane owning 4 consecutive pixels of the flattened image; only the last H W % 4 pixels of an image
 * are written by bytes.
 * status: R3D_SOURCE_STATUS_WORDS = 2 int32 words on the device, zeroed by the call, then word 0 != 0: a frame has no seed (in
 *   r3d_source_background: no pixel that is not background, where sklearn raises in the reference); word 1 != 0 (r3d_source_background):
 *   the clip has no surely-background pixel (the same).  The outputs are then defined but meaningless (out is 0 where word 1 is set).
 *   The library never reads the words on the host; the Python wrapper does, one 8-byte copy per call.
 * workspace: r3d_source_workspace_bytes(B, H, W) bytes (0: a size outside the limits), 16-byte aligned, N = H W, every part rounded up
 *   to 16 bytes, in this order: seed rows int32 [B N] | d2 int32 [B N] (also the column pass's scratch) | index int32 [N] | sure mask
 *   uint8 [N] | staged image uint8 [3 N] | column records int32 [2 W].  r3d_source_torso takes the size of B = 1.
 * Refused before any launch with R3D_ERR_INVALID_ARG: a NULL pointer (but d2 or index, not both; segmap in r3d_source_to_planes; mask in
 *   r3d_source_select); B, H or W
 *   below 1, B above 65535 or a side above R3D_SOURCE_MAX_SIDE (r3d_source_torso: a side below 3, the reflection's reach); 4 B H W at or above 2^31
 *   bytes; an int32 or fp32 array, the status or the workspace not 4-byte (workspace: 16-byte) aligned, an output image or mask not
 *   4-byte aligned; a workspace smaller than r3d_source_workspace_bytes; classes outside 1 .. 63 where there is a segmap; blur weights outside
 *   0 .. 256 or summing above 256; a darkening factor outside 0 .. 1; an output, the status or the workspace overlapping an input or each other. */
#define R3D_SOURCE_MAX_SIDE 2048
#define R3D_SOURCE_STATUS_WORDS 2
#define R3D_SOURCE_DARKEN 53
#define R3D_SOURCE_HEAD_CLASSES 42
size_t r3d_source_workspace_bytes(int B, int H, int W);
int r3d_source_nearest(const uint8_t* mask, int B, int H, int W, int32_t* d2, int32_t* index, int32_t* status, void* workspace,
                       size_t workspace_bytes, r3d_stream_t stream);
int r3d_source_background(const uint8_t* img, const uint8_t* bg, int B, int H, int W, uint8_t* out, int32_t* status, void* workspace,
                          size_t workspace_bytes, r3d_stream_t stream);
int r3d_source_torso(const uint8_t* img, const uint8_t* segmap, int H, int W, const double* darken, const int* blur_weights,
                     uint8_t* torso_img, uint8_t* torso_mask, uint8_t* with_bg_img, uint8_t* with_bg_mask, void* workspace,
                     size_t workspace_bytes, r3d_stream_t stream);
int r3d_source_select(const uint8_t* img, const uint8_t* segmap, int classes, int H, int W, uint8_t* out, uint8_t* mask, r3d_stream_t stream);
int r3d_source_to_planes(const uint8_t* img, const uint8_t* segmap, int classes, int H, int W, float* out, r3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* R3D_HIP_SOURCE_H */
