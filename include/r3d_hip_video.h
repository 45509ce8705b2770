/*
 * r3d_hip_video.h -- companion header of r3d_hip.h (C ABI of libr3d_hip.so): the clip's output video frames.  r3d_hip.h includes it; it can
 * also be included on its own.  The Python binding table of this header is real3dportrait_amd/_lib.py SIGNATURES.
 */
#ifndef R3D_HIP_VIDEO_H
#define R3D_HIP_VIDEO_H

#include "r3d_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* --- the clip's output video frames in out_mode 'concat_debug', inference (added under ABI 0.8.0) -----------------------------------------
 * What forward_secc2video does on the host after the frame loop (inference/real3d_infer.py:495-521), on the device (DESIGN 4.18;
 * tests/video_frames_ref.py is the restatement with the reference's operators).  Same conventions as r3d_hip.h: borrowed device pointers,
 * contiguous fp32, `stream` a hipStream_t, 0 or a negative r3d_status, the message from r3d_last_error().
 *
 * The strip of frame t, uint8 [H, 5 W, 3], holds five panels of H x W pixels, left to right (:512):
 *   0  ref [1, 3, H, W], the same for every frame;            1  secc [n, 3, hs, ws], nearest to H x W (:498), quantised twice (below);
 *   2  raw [n, 3, hr, wr], nearest to H x W;                   3  depth [n, 1, hd, wd], nearest to H x W, normalised over the CLIP, on all
 *   4  image [n, 3, H, W].                                        three channels (:504-508).
 * The five rules the bytes follow, each in the reference's order of operations:
 *   (1) the strip is quantised in fp64: the SECC panel comes back from NumPy as float64 (:502, :510), torch.cat promotes the strip, so
 *       clamp(-1, 1) and (x + 1) / 2 * 255 (:517, :521) run in fp64 on the exactly widened fp32 values; then truncation toward zero.
 *       (out_mode 'final' stays fp32: r3d_frames_to_u8.)
 *   (2) the SECC panel: q = int32(trunc((s + 1) * 127.5)) in fp32, add then multiply, no clamp (:502); v = q / 127.5 - 1 in fp64 (:510),
 *       then rule (1).  For 20 of the codes q in 0 .. 255 this gives q - 1; it is not simplified.  (A product outside int32, or NaN,
 *       converts to INT32_MIN as on x86 and ends as byte 0.)
 *   (3) depth: (d - min) / (max - min) with IEEE division, * 2 - 1, clamp(-1, 1), all fp32 (:506-508), min and max over every depth value
 *       of the clip, not of the frame; then rule (1).  A constant clip is 0 / 0 = NaN; a NaN anywhere in the depth makes min and max NaN
 *       (torch.min propagates it) and every depth pixel of every frame NaN.
 *   (4) a NaN before the truncation is byte 0, in every panel (the reference's NaN -> int32 -> uint8 on x86).
 *   (5) F.interpolate(x, (H, W)) is the legacy nearest mode: source index min(floor(dst * (float(in) / float(out))), in - 1), the scale
 *       and the product in fp32 (5 -> 12: 0 0 0 1 1 2 2 2 3 3 4 4).
 *
 * r3d_video_depth_range folds depth[0 .. count) into `state`, R3D_VIDEO_STATE_WORDS int32 words on the device:
 *   word 0 the minimum and word 1 the maximum as fp32 bit patterns, word 2 nonzero if a NaN was seen (then words 0 and 1 hold a NaN),
 *   word 3 nonzero once a call has completed; words 4 .. 7 belong to the kernel (an arrival counter and the launch's partial result).
 *   The state must be zero-filled ONCE, when it is allocated; every call leaves words 4 .. 7 zero again.  reset = 0 accumulates onto what
 *   the state holds, so a clip can be fed in chunks; reset != 0 discards words 0 .. 3 first, inside the launch (no memset, one launch per
 *   call either way).  Minimum and maximum are taken on the ordered-integer image of the fp32 values (-0.0 below +0.0), which is exact
 *   and independent of order: the state is bit-identical however the clip is chunked and from run to run.  Calls on one state are
 *   ordered by the caller (one stream, or events); two states can be reduced concurrently.
 * r3d_video_compose_debug writes the n strips of a chunk, out [n, H, 5 W, 3], from the sources of the same n frames and the state of the
 *   WHOLE clip.  `panels` selects what is written, a bit per panel (R3D_VIDEO_PANELS_ALL = 31; bit 3 is the depth panel); the bytes of
 *   the other panels are left as they are and their sources may be NULL, as may `state` without bit 3 -- a caller that holds the colours of
 *   a chunk only composes 31 - 8 per chunk and the depth panels of the clip at its end.  A lane owns 16 consecutive pixels of one panel
 *   row (sixteen-byte loads in, three sixteen-byte stores out) when W % 16 == 0 and every selected pointer is 16-byte aligned, and 4
 *   pixels (three dword stores) otherwise; there are no byte stores.  Each output byte is a pure function of the inputs: no atomics, no
 *   workspace, no allocation, no host synchronisation; run to run, stream to stream and chunk to chunk bit-identical.  Inputs are never
 *   written.  A state that no call has completed on (word 3 zero) is not detected: the depth panel is then undefined.
 * Refused before any launch with R3D_ERR_INVALID_ARG: a NULL pointer (of a selected panel, of out, of depth or state in
 * r3d_video_depth_range); count, n, H, W or a source size below 1; panels outside 1 .. 31; W % 4 != 0; out not 4-byte aligned or state not
 * 4-byte aligned; 4 count, the bytes of any selected source or the 15 n H W bytes of out at or above 2^31 per call; an output (out, or
 * the state in r3d_video_depth_range) that overlaps an input; with the depth panel selected, hd > H, wd > W or a last depth row or column
 * that rule (5) does not reach -- the reference's minimum and maximum are those of the RESIZED images (:504-506), which equal the source's,
 * what the state holds, only when the resize uses every source pixel, as nearest up-sampling does. */
#define R3D_VIDEO_STATE_WORDS 8
#define R3D_VIDEO_PANELS_ALL 31
#define R3D_VIDEO_PANEL_DEPTH 8
int r3d_video_depth_range(const float* depth, size_t count, int reset, int32_t* state, r3d_stream_t stream);
int r3d_video_compose_debug(const float* ref, const float* secc, int hs, int ws, const float* raw, int hr, int wr, const float* depth, int hd,
                            int wd, const float* image, int n, int H, int W, int panels, const int32_t* state, uint8_t* out,
                            r3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* R3D_HIP_VIDEO_H */
