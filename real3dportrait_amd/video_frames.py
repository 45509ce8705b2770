"""HIP output video frames: the tail of forward_secc2video (inference/real3d_infer.py:436-542) on the device (r3d_video_depth_range,
r3d_video_compose_debug of include/r3d_hip_video.h).

    depth_range            (depth, state=None, reset=False) -> state: the clip's depth minimum, maximum and NaN flag, accumulated
    compose_debug_frames   (ref_gt_img, drv_secc, imgs_raw, depth_imgs, imgs, depth_range=None, out=None) -> uint8 [T, H, 5 W, 3]:
                           real3d_infer.py:495-521 in out_mode 'concat_debug', byte for byte
    clip_frames            (outputs, batch, out_mode) -> uint8 [T, H, W or 5 W, 3]: 'final' or 'concat_debug'
    secc2video_frames      (infer, batch, inp, chunk_frames=None) -> the clip's frames: the frame loop of :451-492 and the above
    write_video            (frames, infer, inp) -> the file's name: :519-542, imageio and ffmpeg as there
    patch_secc2video       (infer, writer=write_video) binds forward_secc2video (the old one stays as _r3d_reference_forward_secc2video)

INFERENCE ONLY: inputs are detached, must be contiguous fp32 tensors on a GPU (anything else raises) and are never written.  No host
synchronisation before the frames are asked for on the host.  There is no fallback: without the library, importing this raises.
"""
import os
import shutil
import subprocess

import torch

from . import _lib
from .clip_conditions import _on_gpu, clip_keypoints

OUT_MODES = ("final", "concat_debug")
TORSO_SMOOTH_KERNEL = 7          # real3d_infer.py:451
MAX_CALL_BYTES = 2 ** 31 - 1     # what one call of either entry point may read from a source or write (include/r3d_hip_video.h); longer clips are cut
_lib.load()


def new_depth_state(device):
    """An empty state of r3d_video_depth_range: zero-filled once, as the header asks."""
    return torch.zeros(_lib.VIDEO_STATE_WORDS, dtype=torch.int32, device=device)


def _state(state, what):
    if not torch.is_tensor(state):
        raise TypeError("%s: the state must be a tensor, got %s" % (what, type(state).__name__))
    if state.dtype != torch.int32 or tuple(state.shape) != (_lib.VIDEO_STATE_WORDS,):
        raise TypeError("%s: the state must be int32 [%d] (new_depth_state), got %s %s" % (what, _lib.VIDEO_STATE_WORDS, state.dtype, tuple(state.shape)))
    if not state.is_contiguous():
        raise ValueError("%s: the state is not contiguous" % what)
    if not state.is_cuda:
        raise ValueError("%s: the state is on %s; the kernels run on the GPU only" % (what, state.device))
    return state


@torch.no_grad()
def depth_range(depth, state=None, reset=False):
    """depth: fp32 of any shape, a chunk of the clip's image_depth.  Folds its minimum, maximum and `a NaN was seen` into `state` (a new
    one when None) and returns the state: int32 [8], words 0 and 1 the fp32 bit patterns of min and max (state[:2].view(torch.float32)),
    word 2 the NaN flag.  reset=True discards what the state holds first, inside the launch.  One launch (one per MAX_CALL_BYTES of
    depth), no synchronisation."""
    d = _on_gpu(depth, "depth_range")
    if d.numel() < 1:
        raise ValueError("depth_range: the tensor is empty")
    state = new_depth_state(d.device) if state is None else _state(state, "depth_range")
    if state.device != d.device:
        raise ValueError("depth_range: the state is on %s, the depth on %s" % (state.device, d.device))
    flat, per_call = d.reshape(-1), max(1, MAX_CALL_BYTES // 4)
    with torch.cuda.device(d.device):
        for lo in range(0, flat.numel(), per_call):          # one launch, unless the tensor is above the entry point's limit per call
            part = flat[lo:lo + per_call]
            _lib.call("r3d_video_depth_range", part, part.numel(), 1 if reset and lo == 0 else 0, state)
    return state


_depth_range = depth_range          # (compose_debug_frames has a parameter of the function's name)


def _panels(ref_gt_img, drv_secc, imgs_raw, depth_imgs, imgs, what):
    """The five sources checked against each other; returns them detached with (T, H, W)."""
    named = list(zip(("ref_gt_img", "drv_secc", "imgs_raw", "depth_imgs", "imgs"), (ref_gt_img, drv_secc, imgs_raw, depth_imgs, imgs)))
    for name, x in named:                         # what _on_gpu asks of a tensor itself, of all five before the device of any
        if not torch.is_tensor(x):
            raise TypeError("%s %s: a tensor is needed, got %s" % (what, name, type(x).__name__))
        if x.dtype != torch.float32:
            raise TypeError("%s %s: a float32 tensor is needed, got %s" % (what, name, x.dtype))
        if not x.is_contiguous():
            raise ValueError("%s %s: the tensor is not contiguous" % (what, name))
    ref, secc, raw, dep, img = (_on_gpu(x, "%s %s" % (what, name)) for name, x in named)
    if img.dim() != 4 or img.shape[1] != 3 or img.shape[0] < 1:
        raise ValueError("%s: imgs must be [T, 3, H, W] with T >= 1, got %s" % (what, tuple(img.shape)))
    T, _, H, W = img.shape
    if tuple(ref.shape) != (1, 3, H, W):
        raise ValueError("%s: ref_gt_img must be [1, 3, %d, %d] like a frame of imgs, got %s" % (what, H, W, tuple(ref.shape)))
    for name, x, c in (("drv_secc", secc, 3), ("imgs_raw", raw, 3), ("depth_imgs", dep, 1)):
        if x.dim() != 4 or x.shape[0] != T or x.shape[1] != c or x.shape[2] < 1 or x.shape[3] < 1:
            raise ValueError("%s: %s must be [%d, %d, h, w] for the %d frames of imgs, got %s" % (what, name, T, c, T, tuple(x.shape)))
    if W % 4 != 0:
        raise ValueError("%s: W = %d must be a multiple of 4" % (what, W))
    return ref, secc, raw, dep, img, T, H, W


def _out(out, T, H, W5, device, what):
    if out is None:
        return torch.empty(T, H, W5, 3, dtype=torch.uint8, device=device)
    if not torch.is_tensor(out) or out.dtype != torch.uint8 or tuple(out.shape) != (T, H, W5, 3):
        raise TypeError("%s: out must be a uint8 tensor [%d, %d, %d, 3]" % (what, T, H, W5))
    if not out.is_contiguous():
        raise ValueError("%s: out is not contiguous" % what)
    if not out.is_cuda:
        raise ValueError("%s: out is on %s; the kernels run on the GPU only" % (what, out.device))
    return out


def _compose(ref, secc, raw, dep, img, n, H, W, panels, state, out):
    """r3d_video_compose_debug on n frames; a source may be None when its panel is not selected.  One launch, unless a source or the
    output is above the entry point's limit per call: then the frames are cut into the longest runs that stay below MAX_CALL_BYTES
    (frame slices are contiguous, ref and the state belong to every run)."""
    size = lambda x: (x.shape[2], x.shape[3]) if x is not None else (1, 1)
    (hs, ws), (hr, wr), (hd, wd) = size(secc), size(raw), size(dep)
    per_frame = max(15 * H * W, 12 * hs * ws, 12 * hr * wr, 4 * hd * wd)          # bytes a frame of the largest operand takes
    per_call = max(1, MAX_CALL_BYTES // per_frame)
    cut = lambda x, lo, hi: None if x is None else x[lo:hi]
    with torch.cuda.device(out.device):
        for lo in range(0, n, per_call):
            hi = min(lo + per_call, n)
            _lib.call("r3d_video_compose_debug", ref, cut(secc, lo, hi), hs, ws, cut(raw, lo, hi), hr, wr, cut(dep, lo, hi), hd, wd,
                      cut(img, lo, hi), hi - lo, H, W, panels, state, out[lo:hi])
    return out


@torch.no_grad()
def compose_debug_frames(ref_gt_img, drv_secc, imgs_raw, depth_imgs, imgs, depth_range=None, out=None):
    """ref_gt_img [1, 3, H, W], drv_secc [T, 3, hs, ws], imgs_raw [T, 3, hr, wr], depth_imgs [T, 1, hd, wd], imgs [T, 3, H, W] -> the
    strips ref | secc | raw | depth | image as uint8 [T, H, 5 W, 3] on the device (into `out` when given): what real3d_infer.py:495-521
    leaves in out_imgs in out_mode 'concat_debug'.  depth_range: the state of the WHOLE clip when these T frames are a chunk of it (the
    function depth_range's result); None reduces over depth_imgs first.  Any T: a clip above the entry point's 2^31 bytes per call
    (546 frames at 512 x 512) is composed in several launches."""
    what = "compose_debug_frames"
    ref, secc, raw, dep, img, T, H, W = _panels(ref_gt_img, drv_secc, imgs_raw, depth_imgs, imgs, what)
    state = _depth_range(dep) if depth_range is None else _state(depth_range, what)
    out = _out(out, T, H, 5 * W, img.device, what)
    for name, x in (("the depth_range state", state), ("out", out), ("ref_gt_img", ref), ("drv_secc", secc), ("imgs_raw", raw), ("depth_imgs", dep)):
        if x.device != img.device:
            raise ValueError("%s: %s is on %s, imgs on %s" % (what, name, x.device, img.device))
    return _compose(ref, secc, raw, dep, img, T, H, W, _lib.VIDEO_PANELS_ALL, state, out)


@torch.no_grad()
def final_frames(imgs, out=None):
    """imgs [T, 3, H, W] -> uint8 [T, H, W, 3]: clamp(-1, 1) and ((x + 1) / 2 * 255).int() in fp32, out_mode 'final' (:514-521)."""
    img = _on_gpu(imgs, "final_frames")
    if img.dim() != 4 or img.shape[1] != 3 or img.shape[0] < 1:
        raise ValueError("final_frames: imgs must be [T, 3, H, W] with T >= 1, got %s" % (tuple(img.shape),))
    T, _, H, W = img.shape
    out = _out(out, T, H, W, img.device, "final_frames")
    with torch.cuda.device(img.device):
        _lib.call("r3d_frames_to_u8", img, T, H, W, out)
    return out


def _mode(out_mode, what):
    if out_mode == "debug":
        raise NotImplementedError("to do: save separate videos")          # as the reference, :515-516
    if out_mode not in OUT_MODES:
        raise ValueError("%s: out_mode must be one of %s, got %r" % (what, OUT_MODES, out_mode))
    return out_mode


@torch.no_grad()
def clip_frames(outputs, batch, out_mode):
    """outputs: {'image' [T, 3, H, W], 'image_raw', 'image_depth'} of the whole clip; batch: 'ref_gt_img' and 'drv_secc' -> the clip's
    uint8 frames on the device, [T, H, W, 3] for 'final' and [T, H, 5 W, 3] for 'concat_debug'."""
    if _mode(out_mode, "clip_frames") == "final":
        return final_frames(outputs["image"])
    return compose_debug_frames(batch["ref_gt_img"], batch["drv_secc"], outputs["image_raw"], outputs["image_depth"], outputs["image"])


@torch.no_grad()
def secc2video_frames(infer, batch, inp, chunk_frames=None):
    """The body of forward_secc2video up to out_imgs (:437-521): smooths the driving key points, runs infer.secc2video_model.forward once per
    frame with the reference's arguments and backbone-cache flags, and returns the clip's frames, uint8 on the device: [T, H, W, 3] with
    inp['low_memory_usage'] (the image alone, clamped; the reference's branch writes it unclamped, so a value above 1 wraps there) or
    inp['out_mode'] 'final', [T, H, 5 W, 3] for 'concat_debug'.
    A frame's image, image_raw and image_depth are copied into buffers allocated once; nothing in the loop waits for the device.
    chunk_frames bounds the fp32 colour buffers to that many frames (None: the clip): each chunk is converted when it is full.  In
    'concat_debug' the depth panel needs the range of the whole clip, so the clip's depth images are kept (hd wd 4 bytes a frame), every
    chunk writes its other four panels, and the depth panels are written once the loop has ended.  The uint8 output is NOT chunked: the
    whole clip's frames stay on the device until they are returned (15 H W bytes a frame in 'concat_debug', 0.98 GB for 250 frames at
    512 x 512), because no strip is complete before the last frame's depth is known.  Clips of any length: a pass over more frames
    than one call of the entry point takes is cut into several."""
    what = "secc2video_frames"
    low = bool(inp.get("low_memory_usage", False))
    mode = "final" if low else _mode(inp["out_mode"], what)
    drv_secc = batch["drv_secc"]
    T = len(drv_secc)
    if T < 1:
        raise ValueError("%s: the clip has no frames" % what)
    chunk = T if chunk_frames is None else int(chunk_frames)
    if chunk < 1:
        raise ValueError("%s: chunk_frames = %d must be positive" % (what, chunk))
    chunk = min(chunk, T)
    camera, ref_head = batch["camera"], batch["ref_head_img"]
    if not drv_secc.is_cuda:
        drv_secc = drv_secc.to(camera.device)
    src_kp = batch["src_kp"].reshape(-1, 68, 2).contiguous()
    kp_s, kp_d = clip_keypoints(src_kp, batch["drv_kp"].reshape(-1, 68, 2).contiguous(), TORSO_SMOOTH_KERNEL)
    model = infer.secc2video_model
    ref = secc = None
    if mode == "concat_debug":
        ref, secc = _on_gpu(batch["ref_gt_img"], what), _on_gpu(drv_secc, what)
    bufs = out = depth = None
    for lo in range(0, T, chunk):
        hi = min(lo + chunk, T)
        for i in range(lo, hi):
            cond = {"cond_cano": batch["cano_secc"], "cond_src": batch["src_secc"], "cond_tgt": drv_secc[i:i + 1],
                    "ref_torso_img": batch["ref_torso_img"], "bg_img": batch["bg_img"], "segmap": batch["segmap"],
                    "kp_s": kp_s[i:i + 1], "kp_d": kp_d[i:i + 1]}
            gen = model.forward(img=ref_head, camera=camera[i:i + 1], cond=cond, ret={}, cache_backbone=i == 0, use_cached_backbone=i != 0)
            image = gen["image"]
            if bufs is None:                      # the first frame tells the sizes
                H, W = image.shape[2], image.shape[3]
                new = lambda n, like: torch.empty((n,) + tuple(like.shape[1:]), dtype=torch.float32, device=image.device)
                bufs = {"image": new(chunk, image)}
                if mode == "concat_debug":
                    bufs["image_raw"] = new(chunk, gen["image_raw"])
                    depth = new(T, gen["image_depth"])
                out = torch.empty(T, H, W if mode == "final" else 5 * W, 3, dtype=torch.uint8, device=image.device)
            bufs["image"][i - lo].copy_(image[0])
            if mode == "concat_debug":
                bufs["image_raw"][i - lo].copy_(gen["image_raw"][0])
                depth[i].copy_(gen["image_depth"][0])
        n = hi - lo
        if mode == "final":
            final_frames(bufs["image"][:n], out[lo:hi])
        else:
            r, s, raw, d, img, _, H, W = _panels(ref, secc[lo:hi], bufs["image_raw"][:n], depth[lo:hi], bufs["image"][:n], what)
            _compose(r, s, raw, None, img, n, H, W, _lib.VIDEO_PANELS_ALL - _lib.VIDEO_PANEL_DEPTH, None, out[lo:hi])
    if mode == "concat_debug":
        state = _depth_range(depth)
        _compose(None, None, None, depth, None, T, H, W, _lib.VIDEO_PANEL_DEPTH, state, out)
    return out


def write_video(frames, infer, inp, run=subprocess.call):
    """frames: uint8 [T, h, w, 3] on the host (NumPy).  The part of forward_secc2video that follows out_imgs (real3d_infer.py:519-542):
    the frames go to an h264 file at 25 frames a second through imageio, then ffmpeg adds the audio track -- infer.wav16k_name when the
    driving audio is a .wav or .mp3 (that file and the silent video are deleted afterwards), otherwise the audio stream of
    inp['drv_audio_name'], and if ffmpeg cannot take one from it the silent video becomes the output.  The output is inp['out_name'], or
    infer_out/tmp/<source image>_<driving pose>.mp4 when that is empty.  Returns the output file's name.
    ffmpeg is started with an argument list (`run`, subprocess.call by default), never through a shell, so names with blanks or shell
    characters are taken as they are.  imageio is imported here, when a video is written."""
    import imageio
    silent = "demo.mp4"
    writer = imageio.get_writer(silent, fps=25, format="FFMPEG", codec="h264")
    for frame in frames:
        writer.append_data(frame)
    writer.close()
    stem = lambda path: os.path.splitext(os.path.basename(path))[0]
    target = inp["out_name"] or os.path.join("infer_out", "tmp", "%s_%s.mp4" % (stem(inp["src_image_name"]), stem(inp["drv_pose_name"])))
    if os.path.dirname(target):
        os.makedirs(os.path.dirname(target), exist_ok=True)
    ffmpeg = lambda audio, *maps: run(["ffmpeg", "-i", silent, "-i", audio] + list(maps) + ["-y", "-v", "quiet", "-shortest", target])
    audio = inp["drv_audio_name"]
    if os.path.splitext(audio)[1] in (".wav", ".mp3"):
        ffmpeg(infer.wav16k_name)
        for leftover in (silent, infer.wav16k_name):
            if os.path.exists(leftover):
                os.remove(leftover)
    elif ffmpeg(audio, "-map", "0:v", "-map", "1:a") != 0:
        shutil.move(silent, target)
    print("Saved at %s" % target)
    return target


def patch_secc2video(infer, writer=write_video, chunk_frames=None):
    """Bind infer.forward_secc2video(batch, inp=None) to secc2video_frames followed by ONE copy of the uint8 frames to the host and
    writer(frames, infer, inp), whose result it returns (write_video: the output file's name, as the reference).  The replaced method
    stays at infer._r3d_reference_forward_secc2video.  Returns infer."""
    if not hasattr(infer, "_r3d_reference_forward_secc2video"):
        infer._r3d_reference_forward_secc2video = getattr(infer, "forward_secc2video", None)

    def forward_secc2video(batch, inp=None):
        frames = secc2video_frames(infer, batch, inp, chunk_frames)
        return writer(frames.cpu().numpy(), infer, inp)

    infer.forward_secc2video = forward_secc2video
    return infer
