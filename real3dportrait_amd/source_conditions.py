"""HIP source-image conditions: what prepare_batch_from_inp builds on the host once per clip (inference/real3d_infer.py:244-260) -- the head
image, the in-painted torso image and the background image -- on the device (include/r3d_hip_source.h).

    nearest_seed          (mask [H, W] or [B, H, W]) -> (d2, index): the exact nearest-seed transform, lowest (row, col) among ties
    head_image            (img, segmap) -> (head_img, selected_mask): MediapipeSegmenter._seg_out_img_with_segmap(img, segmap, mode='head')
    inpaint_torso_job     (gt_img, segmap) -> (torso_img, torso_img_mask, torso_with_bg_img, torso_with_bg_img_mask)
    extract_background    (img_lst, segmap_mask_lst, method='knn') -> bg_img
                          (data_gen/utils/process_video/extract_segment_imgs.py:148-239 and :63-146, their names, arguments and returns)
    source_to_planes      (img, segmap=None, classes=HEAD_CLASSES) -> fp32 [1, 3, H, W]: ((x - 127.5) / 127.5) of real3d_infer.py:249
    source_conditions     (img, segmap, bg_image=None) -> {'ref_head_img', 'ref_torso_img', 'bg_img', 'segmap'} as :247-260 builds them
    patch_segment_imgs    sets a module's names inpaint_torso_job and extract_background (real3d_infer.py binds them by `from ... import`)

img is uint8 [H, W, 3]; segmap is [6, H, W] of any dtype, a pixel belonging to a class where its value is not 0 (the reference's
.astype(bool)).  Device tensors in give device tensors out; NumPy arrays in give NumPy arrays out, with one upload and one copy back.
The results are the reference's byte for byte, with three stated exceptions: among equidistant nearest background pixels
the one with the lowest (row, col) is copied (the reference: whatever its kd-tree returns); neck and torso paint above row 0 is dropped
(the reference wraps it to the bottom rows); the blur is a fixed-point model of cv2.GaussianBlur whose equality with OpenCV has not been
measured (BLUR_WEIGHTS is an argument of the entry point for that reason).

INFERENCE ONLY.  There is no fallback: without the library, importing this raises.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._state import StreamBuffers

HEAD_CLASSES = _lib.SOURCE_HEAD_CLASSES          # classes 1 | 3 | 5: hair, face skin, others (glasses)
MAX_SIDE = _lib.SOURCE_MAX_SIDE
BLUR_WEIGHTS = (48, 53, 54, 53, 48)              # exp(-x^2 / (2 * 4^2)), x = -2 .. 2, normalised, 8 fractional bits; they sum to 256
DARKEN = 0.98 ** np.arange(_lib.SOURCE_DARKEN)   # extract_segment_imgs.py:179, :215, NumPy's own powers

_lib.load()
_DARKEN_C = (ctypes.c_double * _lib.SOURCE_DARKEN)(*DARKEN.tolist())


class _Work:
    """The workspace and the status words of one (device, stream, B, H, W)."""

    def __init__(self, dev, B, H, W):
        nbytes = _lib.call("r3d_source_workspace_bytes", B, H, W)
        if nbytes == 0:
            raise ValueError("source conditions: %d frames of %d x %d are outside what the kernels accept (sides 1 .. %d)" % (B, H, W, MAX_SIDE))
        self.ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
        self.status = torch.zeros(_lib.SOURCE_STATUS_WORDS, device=dev, dtype=torch.int32)


_WORK = StreamBuffers(_Work, cap=8)


def _device():
    if not torch.cuda.is_available():
        raise ValueError("source conditions: a NumPy array was given and there is no GPU to compute on; the kernels run on the GPU only")
    return torch.device("cuda", torch.cuda.current_device())


def _sides(H, W, what, least=1):
    if not (least <= H <= MAX_SIDE and least <= W <= MAX_SIDE):
        raise ValueError("%s: %d x %d pixels; the sides must be %d .. %d" % (what, H, W, least, MAX_SIDE))


def _image(img, what, dev=None, least=1):
    """uint8 [H, W, 3], NumPy or a device tensor, every check before the upload -> (the device tensor, was it NumPy?)."""
    host = isinstance(img, np.ndarray)
    if not host and not torch.is_tensor(img):
        raise TypeError("%s: an image is a NumPy array or a tensor, got %s" % (what, type(img).__name__))
    if img.ndim != 3 or img.shape[2] != 3 or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError("%s: an image is [H, W, 3], got %s" % (what, tuple(img.shape)))
    if img.dtype not in (np.uint8, torch.uint8):
        raise TypeError("%s: an image is uint8, got %s" % (what, img.dtype))
    _sides(img.shape[0], img.shape[1], what, least)
    if host:
        return torch.from_numpy(np.ascontiguousarray(img)).to(dev or _device()), True
    if not img.is_cuda:
        raise ValueError("%s: the image is on %s; the kernels run on the GPU only" % (what, img.device))
    return img.detach().contiguous(), False


def _planes(x, what, dev, shape):
    """Class planes or masks of any dtype, NumPy or a tensor on dev -> uint8 on dev, 1 where the value is not 0."""
    if isinstance(x, np.ndarray):
        if tuple(x.shape) != shape:
            raise ValueError("%s must be %s, got %s" % (what, list(shape), tuple(x.shape)))
        return torch.from_numpy(np.ascontiguousarray(x != 0).view(np.uint8)).to(dev)
    if not torch.is_tensor(x):
        raise TypeError("%s is a NumPy array or a tensor, got %s" % (what, type(x).__name__))
    if tuple(x.shape) != shape:
        raise ValueError("%s must be %s, got %s" % (what, list(shape), tuple(x.shape)))
    if x.device != dev:
        raise ValueError("%s is on %s, the image on %s" % (what, x.device, dev))
    x = x.detach()
    return x.contiguous() if x.dtype in (torch.uint8, torch.bool) else (x != 0).to(torch.uint8)


def _raise_status(status, what):
    """One 8-byte copy to the host (a synchronisation)."""
    s0, s1 = status.tolist()
    if s0:
        raise ValueError("%s: a frame has no seed pixel (in extract_background: no pixel that is not background; the reference fails fitting "
                         "a kd-tree on nothing)" % what)
    if s1:
        raise ValueError("%s: no pixel is more than 10 pixels away from the person in any frame (the reference fails fitting a kd-tree on "
                         "nothing)" % what)


@torch.no_grad()
def nearest_seed(mask):
    """mask [H, W] or [B, H, W] (any dtype, a seed where the value is not 0) -> (d2, index), int32 of the mask's shape: per pixel the squared
    Euclidean distance to the nearest seed of its frame and that seed's row * W + col, the lowest (row, col) among equidistant seeds.
    ValueError when a frame has no seed (the status is read: one synchronisation)."""
    what = "nearest_seed"
    host = isinstance(mask, np.ndarray)
    if not host and not torch.is_tensor(mask):
        raise TypeError("%s: the mask is a NumPy array or a tensor, got %s" % (what, type(mask).__name__))
    if mask.ndim not in (2, 3) or min(mask.shape) < 1:
        raise ValueError("%s: the mask must be [H, W] or [B, H, W], got %s" % (what, tuple(mask.shape)))
    shape = tuple(mask.shape)
    B, H, W = (1,) + shape if len(shape) == 2 else shape
    _sides(H, W, what)
    if not host and not mask.is_cuda:
        raise ValueError("%s: the mask is on %s; the kernels run on the GPU only" % (what, mask.device))
    dev = _device() if host else mask.device
    m = _planes(mask, "%s: the mask" % what, dev, shape)
    with torch.cuda.device(dev):
        work = _WORK.get(dev, B, H, W)
        d2 = torch.empty(shape, dtype=torch.int32, device=dev)
        index = torch.empty(shape, dtype=torch.int32, device=dev)
        _lib.call("r3d_source_nearest", m, B, H, W, d2, index, work.status, work.ws, work.ws.numel())
        _raise_status(work.status, what)
    return (d2.cpu().numpy(), index.cpu().numpy()) if host else (d2, index)


def _select(img, seg, classes, H, W):
    out = torch.empty(H, W, 3, dtype=torch.uint8, device=img.device)
    mask = torch.empty(H, W, dtype=torch.uint8, device=img.device)
    with torch.cuda.device(img.device):
        _lib.call("r3d_source_select", img, seg, classes, H, W, out, mask)
    return out, mask


@torch.no_grad()
def head_image(img, segmap):
    """MediapipeSegmenter._seg_out_img_with_segmap(img, segmap, mode='head') (mp_segmenter.py:230-256): (the image with every pixel outside
    hair, face skin and others at 0, selected_mask bool [1, H, W])."""
    what = "head_image"
    x, host = _image(img, what)
    H, W = x.shape[:2]
    seg = _planes(segmap, "%s: segmap" % what, x.device, (6, H, W))
    out, mask = _select(x, seg, HEAD_CLASSES, H, W)
    mask = mask.bool()[None]
    return (out.cpu().numpy(), mask.cpu().numpy()) if host else (out, mask)


def _torso(x, seg, H, W, weights):
    w = [int(v) for v in weights]
    if len(w) != 5 or min(w) < 0 or max(w) > 256 or sum(w) > 256:
        raise ValueError("inpaint_torso_job: the blur weights must be 5 integers in 0 .. 256 that sum to at most 256, got %r" % (tuple(weights),))
    dev = x.device
    imgs = [torch.empty(H, W, 3, dtype=torch.uint8, device=dev) for _ in range(2)]          # (each output is 4-byte aligned: one allocation each)
    masks = [torch.empty(H, W, dtype=torch.uint8, device=dev) for _ in range(2)]
    with torch.cuda.device(dev):
        work = _WORK.get(dev, 1, H, W)
        _lib.call("r3d_source_torso", x, seg, H, W, _DARKEN_C, (ctypes.c_int * 5)(*w), imgs[0], masks[0], imgs[1], masks[1], work.ws, work.ws.numel())
    return imgs, masks


@torch.no_grad()
def inpaint_torso_job(gt_img, segmap, blur_weights=BLUR_WEIGHTS):
    """extract_segment_imgs.py:148-239: (torso_img uint8 [H, W, 3], torso_img_mask bool [H, W], torso_with_bg_img, torso_with_bg_img_mask).
    blur_weights: the 5 x 5 blur's separable weights with 8 fractional bits (the module docstring)."""
    what = "inpaint_torso_job"
    x, host = _image(gt_img, what, least=3)
    H, W = x.shape[:2]
    seg = _planes(segmap, "%s: segmap" % what, x.device, (6, H, W))
    imgs, masks = _torso(x, seg, H, W, blur_weights)
    out = [imgs[0], masks[0].bool(), imgs[1], masks[1].bool()]
    return tuple(o.cpu().numpy() for o in out) if host else tuple(out)


def _background(imgs, bgs, B, H, W):
    dev = imgs.device
    out = torch.empty(H, W, 3, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        work = _WORK.get(dev, B, H, W)
        _lib.call("r3d_source_background", imgs, bgs, B, H, W, out, work.status, work.ws, work.ws.numel())
    return out, work.status


def frame_selection(num_frames):
    """The slice of a clip's frames extract_background looks at (:91-103): every 5th below 100 frames, every 20th below 10 000, every
    (num_frames // 500)th above; the first frame alone when the clip has no more frames than that interval."""
    interval = 5 if num_frames < 100 else 20 if num_frames < 10000 else num_frames // 500
    return slice(None, None, interval) if num_frames > interval else slice(0, 1)


@torch.no_grad()
def extract_background(img_lst, segmap_mask_lst=None, method="knn", device="cpu", mix_bg=True):
    """extract_segment_imgs.py:63-146: img_lst a list of uint8 [H, W, 3] frames, segmap_mask_lst their [6, H, W] segmaps -> the background
    image uint8 [H, W, 3].  The frames are sub-sampled as the reference does (:91-103); `device` and `mix_bg` are the reference's unused
    parameters.  The segmenter is not part of this package: segmap_mask_lst is needed, and file names are not read.  ValueError where
    sklearn raises in the reference: a selected frame without a person, or no surely-background pixel (one synchronisation)."""
    what = "extract_background"
    if method != "knn":
        raise NotImplementedError("%s: method %r (the reference has 'knn' only)" % (what, method))
    assert len(img_lst) > 0
    if segmap_mask_lst is None:
        raise ValueError("%s: segmap_mask_lst is needed (the segmenter is not part of this package)" % what)
    assert len(segmap_mask_lst) == len(img_lst)
    pick = frame_selection(len(img_lst))
    img_lst, segmap_mask_lst = list(img_lst[pick]), list(segmap_mask_lst[pick])
    if any(isinstance(v, str) for v in img_lst + segmap_mask_lst):
        raise TypeError("%s: file names are not read here; pass the frames and segmaps" % what)
    host = isinstance(img_lst[0], np.ndarray)
    for v in img_lst:
        if isinstance(v, np.ndarray) != host:
            raise TypeError("%s: the frames must be all NumPy arrays or all tensors" % what)
    if host:                                      # one upload of the frames, one of the background planes
        shapes = {tuple(v.shape) for v in img_lst}
        if len(shapes) != 1 or len(img_lst[0].shape) != 3 or img_lst[0].shape[2] != 3:
            raise ValueError("%s: the frames must all be [H, W, 3], got %s" % (what, sorted(shapes)))
        if any(v.dtype != np.uint8 for v in img_lst):
            raise TypeError("%s: an image is uint8" % what)
        B = len(img_lst)
        H, W = img_lst[0].shape[:2]
        _sides(H, W, what)
        imgs = torch.from_numpy(np.stack(img_lst)).to(_device())
    else:
        xs = [_image(v, what)[0] for v in img_lst]
        B = len(xs)
        H, W = xs[0].shape[:2]
        if any(tuple(v.shape) != (H, W, 3) or v.device != xs[0].device for v in xs):
            raise ValueError("%s: the frames differ in shape or device" % what)
        imgs = xs[0][None] if B == 1 else torch.stack(xs)
    dev = imgs.device
    for s in segmap_mask_lst:
        if not (isinstance(s, np.ndarray) or torch.is_tensor(s)) or s.ndim != 3 or s.shape[0] < 1 or tuple(s.shape[1:]) != (H, W):
            raise ValueError("%s: a segmap must be [6, %d, %d]" % (what, H, W))
    if all(isinstance(s, np.ndarray) for s in segmap_mask_lst):
        bgs = _planes(np.stack([s[0] for s in segmap_mask_lst]), "%s: the background planes" % what, dev, (B, H, W))
    else:
        bgs = torch.stack([_planes(s[0], "%s: a background plane" % what, dev, (H, W)) for s in segmap_mask_lst])
    out, status = _background(imgs, bgs, B, H, W)
    _raise_status(status, what)
    return out.cpu().numpy() if host else out


def _to_planes(x, seg, classes, H, W, out=None):
    out = torch.empty(1, 3, H, W, dtype=torch.float32, device=x.device) if out is None else out
    with torch.cuda.device(x.device):
        _lib.call("r3d_source_to_planes", x, seg, classes if seg is not None else 0, H, W, out)
    return out


@torch.no_grad()
def source_to_planes(img, segmap=None, classes=HEAD_CLASSES):
    """uint8 [H, W, 3] -> fp32 [1, 3, H, W] on the device, ((torch.tensor(img) - 127.5) / 127.5).float().unsqueeze(0).permute(0, 3, 1, 2) of
    real3d_infer.py:249.  With a segmap, a pixel outside the classes of the bit mask `classes` counts as 0 (-1)."""
    what = "source_to_planes"
    x, _ = _image(img, what)
    H, W = x.shape[:2]
    seg = None if segmap is None else _planes(segmap, "%s: segmap" % what, x.device, (6, H, W))
    if seg is not None and not 1 <= int(classes) <= 63:
        raise ValueError("%s: classes = %r must be a bit mask in 1 .. 63" % (what, classes))
    return _to_planes(x, seg, int(classes), H, W)


@torch.no_grad()
def source_conditions(img, segmap, bg_image=None):
    """real3d_infer.py:247-260: img uint8 [H, W, 3] (the 512 x 512 source image), segmap [6, H, W] (the segmenter's one-hot map) ->
    {'segmap' [1, 6, H, W], 'ref_head_img', 'ref_torso_img', 'bg_img' [1, 3, H, W]}, fp32 on the device.  bg_image: a uint8 [H, W, 3] RGB
    background already at the image's size (:257-259; reading and resizing the file stay the caller's), None: extract_background([img],
    [segmap], 'knn').  Five calls into the library (four with a bg_image): torso, background, three conversions to planes.  No image or
    map goes to the host; with bg_image None the 8 status bytes do, once (a synchronisation), so that a segmap without a person or
    without background raises ValueError as the reference does."""
    what = "source_conditions"
    x, _ = _image(img, what, least=3)
    H, W = x.shape[:2]
    dev = x.device
    seg = _planes(segmap, "%s: segmap" % what, dev, (6, H, W))
    sample = {"segmap": (torch.from_numpy(np.ascontiguousarray(segmap)).to(dev) if isinstance(segmap, np.ndarray) else segmap.detach()).float()[None]}
    sample["ref_head_img"] = _to_planes(x, seg, HEAD_CLASSES, H, W)
    imgs, _ = _torso(x, seg, H, W, BLUR_WEIGHTS)
    sample["ref_torso_img"] = _to_planes(imgs[0], None, 0, H, W)
    if bg_image is None:
        bg, status = _background(x[None], seg[:1], 1, H, W)
    else:
        bg, _ = _image(bg_image, "%s: bg_image" % what, dev)
        if tuple(bg.shape) != (H, W, 3) or bg.device != dev:
            raise ValueError("%s: bg_image must be [%d, %d, 3] on %s, got %s on %s" % (what, H, W, dev, tuple(bg.shape), bg.device))
        status = None
    sample["bg_img"] = _to_planes(bg, None, 0, H, W)
    if status is not None:
        _raise_status(status, what)
    return sample


def patch_segment_imgs(infer_module):
    """Point infer_module.inpaint_torso_job and infer_module.extract_background (inference/real3d_infer.py binds both by `from
    data_gen.utils.process_video.extract_segment_imgs import ...`) at the HIP functions above; returns the module.  prepare_batch_from_inp
    then gets NumPy arrays back as before; source_conditions replaces its lines :247-260 without the copies."""
    infer_module.inpaint_torso_job = inpaint_torso_job
    infer_module.extract_background = extract_background
    return infer_module
