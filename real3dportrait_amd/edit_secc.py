"""HIP blink edit of the driving SECC maps: blink_eye_for_secc of inference/edit_secc.py:47-129 and the loop of
inference/real3d_infer.py:411-426 that applies it, on the device (r3d_secc_blink of include/r3d_hip.h).

    blink_eye_for_secc      the reference's function: (img [3, h, w], close_eye_percent=0.5) -> [3, h, w], on img's device
    blink_frames            the batched form: F frames of a clip [T, 3, H, W] in one chain of launches, in place, no sync
    blink_schedule          the (frame, percent) pairs of the reference's loop, drawing from `rng` exactly as it does
    apply_periodic_blink    schedule + blink_frames: what replaces real3d_infer.py:411-426 (--blink_mode period)
    patch_blink             sets a module's name blink_eye_for_secc (real3d_infer.py binds it by `from inference.edit_secc import ...`)

The reference copies each map to the host, quantises it to 8 bits, fits two sklearn kd-trees and copies the map back.  Here the map stays
on the device.  The result is bit-identical to the reference's except where a pixel to close has two or more nearest face pixels at the
same distance: there the reference takes whatever its kd-tree returns, this takes the one with the lowest (row, column).  Values outside
[-1, 1] and NaN quantise by clamping (the reference's cast is undefined there; SECC_Renderer cannot produce them).

INFERENCE ONLY: no autograd graph is built.  There is no fallback: without the library, importing this raises.
"""
import random

import torch

from . import _lib
from ._state import StreamBuffers

MIN_SIZE, MAX_SIZE = 16, 4096          # r3d_secc_blink's limits on h and w

_STATUS_TEXT = {1: "no eye pixel in one of the two prior regions (the reference fails in min() of an empty array)",
                2: "no face pixel left around the eyes (the reference fails fitting a kd-tree on nothing)",
                3: "frame index or close_eye_percent out of range"}


def _new_workspace(dev, F, H, W):
    nbytes = _lib.call("r3d_secc_blink_workspace_bytes", F, H, W)
    if nbytes == 0:
        raise ValueError("blink: F = %d frames of %d x %d are outside what r3d_secc_blink accepts" % (F, H, W))
    return torch.empty(nbytes, device=dev, dtype=torch.uint8)


_WORKSPACE = StreamBuffers(_new_workspace, cap=8)          # a clip uses one or two shapes


def _check_maps(x, what, dims):
    if not torch.is_tensor(x) or x.dim() != dims or x.shape[-3] != 3:
        raise ValueError("%s must be a %s tensor" % (what, "[3, h, w]" if dims == 3 else "[T, 3, H, W]"))
    h, w = x.shape[-2:]
    if not (MIN_SIZE <= h <= MAX_SIZE and MIN_SIZE <= w <= MAX_SIZE):
        raise ValueError("%s: map size %d x %d is not in %d .. %d" % (what, h, w, MIN_SIZE, MAX_SIZE))


@torch.no_grad()
def blink_frames(drv_secc, frame_idx, percents, out=None):
    """Edit the frames frame_idx (integers, in any order) of drv_secc [T, 3, H, W] (fp32, contiguous, on the GPU) with the closing
    percentages percents (floats), IN PLACE unless `out` is given: then drv_secc is left untouched and out (same shape, fp32, contiguous)
    receives a copy of it with the listed frames edited.  Returns the int32 status tensor [F] on the device WITHOUT reading it (no sync):
    0 done, 1 / 2 the map is degenerate and came back quantised only (where the reference raises ValueError), 3 percentage outside
    [0, 1] (the frame is untouched).  Duplicate or out-of-range indices are a ValueError, raised on the host before any launch;
    frame_idx and percents are host sequences (a tensor is read with .tolist(), which synchronises when it lives on the device)."""
    _check_maps(drv_secc, "blink_frames: drv_secc", 4)
    idx = [int(i) for i in (frame_idx.tolist() if torch.is_tensor(frame_idx) else frame_idx)]
    pct = [float(p) for p in (percents.tolist() if torch.is_tensor(percents) else percents)]
    T, _, H, W = drv_secc.shape
    if len(idx) != len(pct) or not idx:
        raise ValueError("blink_frames: %d frame indices and %d percentages (need the same number, at least one)" % (len(idx), len(pct)))
    if len(set(idx)) != len(idx):
        raise ValueError("blink_frames: a frame is listed twice")
    if min(idx) < 0 or max(idx) >= T:
        raise ValueError("blink_frames: frame indices %d .. %d, the clip has %d frames" % (min(idx), max(idx), T))
    if drv_secc.dtype != torch.float32 or not drv_secc.is_contiguous():
        raise ValueError("blink_frames: drv_secc must be contiguous float32 (it is edited in place)")
    if out is not None:
        if not torch.is_tensor(out) or out.shape != drv_secc.shape or out.dtype != torch.float32 or not out.is_contiguous() \
                or out.device != drv_secc.device:
            raise ValueError("blink_frames: out must be a contiguous float32 tensor of drv_secc's shape on its device")
    if not drv_secc.is_cuda:
        raise ValueError("blink_frames: drv_secc is on %s; the edit runs on the GPU only" % (drv_secc.device,))
    dev, F = drv_secc.device, len(idx)
    target = drv_secc.detach()
    if out is not None and out.data_ptr() != drv_secc.data_ptr():
        target = out.detach()
        target.copy_(drv_secc)
    with torch.cuda.device(dev):
        ws = _WORKSPACE.get(dev, F, H, W)
        d_idx = torch.tensor(idx, dtype=torch.int32).to(dev, non_blocking=True)
        d_pct = torch.tensor(pct, dtype=torch.float64).to(dev, non_blocking=True)
        status = torch.empty(F, dtype=torch.int32, device=dev)
        _lib.call("r3d_secc_blink", target, T, H, W, d_idx, d_pct, F, target, status, ws, ws.numel())
    return status


@torch.no_grad()
def blink_eye_for_secc(img, close_eye_percent=0.5):
    """inference/edit_secc.py:47-129: img [3, h, w] in [-1, 1] -> the map with its eyes closed by close_eye_percent, quantised to 8 bits
    as the reference returns it (also at 0, which only quantises).  The result is a new fp32 tensor on img's device (the reference
    returns a host tensor that its caller moves straight back).  Reads the status, which costs one synchronisation.  AssertionError for
    a percentage outside [0, 1] and ValueError for a map without eye holes or without face around them, as the reference raises."""
    _check_maps(img, "blink_eye_for_secc: img", 3)
    assert close_eye_percent <= 1.0 and close_eye_percent >= 0.
    if not img.is_cuda:
        raise ValueError("blink_eye_for_secc: img is on %s; the edit runs on the GPU only" % (img.device,))
    clip = img.detach().to(torch.float32).clone(memory_format=torch.contiguous_format)[None]
    status = int(blink_frames(clip, [0], [float(close_eye_percent)]).item())
    if status != 0:
        raise ValueError("blink_eye_for_secc: " + _STATUS_TEXT.get(status, "status %d" % status))
    return clip[0]


def blink_schedule(T, period_frames=125, rng=random):
    """The edits of inference/real3d_infer.py:411-426 for a clip of T frames as a list of (frame, close_eye_percent): every
    period_frames frames a blink of rng.randint(8, 12) frames along the parabola -4 / dur^2 offset^2 + 4 / dur offset, cut off before the
    clip's last frame, which is never edited.  rng is consumed exactly as the reference's loop consumes `random`: one randint per
    period, also when all of the period's frames are cut off.  period_frames must exceed 12, so that no frame is edited twice."""
    if period_frames <= 12:
        raise ValueError("blink_schedule: period_frames = %d; a blink lasts up to 12 frames" % period_frames)
    edits = []
    for i in range(T):
        if i % period_frames == 0:
            blink_dur_frames = rng.randint(8, 12)
            for offset in range(blink_dur_frames):
                j = offset + i
                if j >= T - 1:
                    break
                edits.append((j, -4 / blink_dur_frames ** 2 * offset ** 2 + 4 / blink_dur_frames * offset))
    return edits


def apply_periodic_blink(drv_secc, rng=random, period_frames=125):
    """real3d_infer.py:411-426 (--blink_mode period) on drv_secc [T, 3, H, W] in place, in one batched call and without a sync: returns
    (edits, status) with edits the blink_schedule list and status blink_frames' device tensor (None for a clip too short to edit).
    Where the reference's loop raises on a degenerate map, here that frame comes back quantised with a non-zero status."""
    _check_maps(drv_secc, "apply_periodic_blink: drv_secc", 4)
    edits = blink_schedule(drv_secc.shape[0], period_frames, rng)
    if not edits:
        return edits, None
    return edits, blink_frames(drv_secc, [j for j, _ in edits], [p for _, p in edits])


def patch_blink(infer_module):
    """Point infer_module.blink_eye_for_secc (inference/real3d_infer.py binds the name by `from inference.edit_secc import
    blink_eye_for_secc`) at the HIP function above; returns the module.  Its loop then edits frame by frame, one sync each;
    apply_periodic_blink replaces the loop itself."""
    infer_module.blink_eye_for_secc = blink_eye_for_secc
    return infer_module
