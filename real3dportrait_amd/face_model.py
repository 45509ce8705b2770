"""HIP morphable face model: ParametricFaceModel.compute_face_vertex (deep_3drecon/deep_3drecon_models/bfm.py:332-347) and
Face3DHelper.reconstruct_lm2d (data_util/face3d_helper.py:132-169) in one kernel each (r3d_face_vertex / r3d_face_landmarks of
include/r3d_hip.h).

    compute_face_vertex     (face_model, id, exp, angle, trans) -> [B, N, 3], for any object with ParametricFaceModel's attributes
    reconstruct_lm2d        (helper, id_coeff, exp_coeff, euler, trans, to_camera=True) -> [T, L, 2] or [B, T, L, 2]
    patch_face_model        binds the first as face_model.compute_face_vertex (the old one stays as _r3d_reference_compute_face_vertex)
    patch_face3d_helper     binds the second as helper.reconstruct_lm2d (the old one stays as _r3d_reference_reconstruct_lm2d)

The model's arrays (numpy or tensors) are uploaded once per object and device, as the reference's .to() does: an array changed afterwards
is not seen.  A frame's result does not depend on the other frames of the call (the header states it), so a clip may be cut into chunks
of any size.

INFERENCE ONLY: inputs are detached, contiguous fp32 and never written; no autograd graph is built.  There is no fallback: without the
library, importing this raises.
"""
import numpy as np
import torch

from . import _lib

FOCAL, CENTER, IMAGE_SIZE, CAMERA_DISTANCE = 1015.0, 112.0, 224.0, 10.0          # face3d_helper.py:47, 123, 165
_CACHE = "_r3d_face_model_arrays"


def _arrays(obj, names, dev):
    """The model's arrays names = (mean, id_base, exp_base) as contiguous fp32 tensors on dev: mean flat [3 N], the bases [3 N, K].
    Made once per (object, device) and kept on the object; 'cuda' without an index is the current device, so it shares that device's entry."""
    dev = torch.device(dev)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    cache = obj.__dict__.get(_CACHE)
    if cache is None:
        cache = {}
        object.__setattr__(obj, _CACHE, cache)
    hit = cache.get((names, dev))
    if hit is None:
        out = []
        for n in names:
            a = getattr(obj, n)
            t = a.detach() if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
            out.append(t.to(device=dev, dtype=torch.float32).contiguous())
        mean, idb, expb = out[0].reshape(-1), out[1], out[2]
        if idb.dim() != 2 or expb.dim() != 2 or idb.shape[0] != mean.numel() or expb.shape[0] != mean.numel() or mean.numel() % 3:
            raise ValueError("face model: %s %s, %s %s and %s %s do not fit [3 N], [3 N, Ki], [3 N, Ke]"
                             % (names[0], tuple(out[0].shape), names[1], tuple(idb.shape), names[2], tuple(expb.shape)))
        hit = cache[(names, dev)] = (mean, idb, expb)
    return hit


def _coeff(x, what, T, C, dev):
    """A coefficient tensor as contiguous fp32 [T, C] on dev, or None."""
    if x is None:
        return None
    if not torch.is_tensor(x) or x.dim() != 2 or x.shape[0] != T or (C is not None and x.shape[1] != C):
        raise ValueError("face model: %s must be a [%d, %s] tensor, got %s" % (what, T, "C" if C is None else C,
                                                                              tuple(x.shape) if torch.is_tensor(x) else type(x).__name__))
    return x.detach().to(device=dev, dtype=torch.float32).contiguous()


def _device(first, arrays_of):
    """Where the call runs: the coefficients' device when that is a GPU, else the device the model's own tensors are on."""
    if torch.is_tensor(first) and first.is_cuda:
        return first.device
    if torch.is_tensor(arrays_of) and arrays_of.is_cuda:
        return arrays_of.device
    raise ValueError("face model: the coefficients are on %s and the model holds no GPU tensor; the kernels run on the GPU only"
                     % (first.device if torch.is_tensor(first) else "the host"))


@torch.no_grad()
def face_vertex(arrays, id, exp=None, euler=None, trans=None, camera_distance=CAMERA_DISTANCE, to_camera=True, out=None):
    """r3d_face_vertex on arrays = (mean [3 N], id_base [3 N, Ki], exp_base [3 N, Ke]), contiguous fp32 tensors on the GPU: id [T, Ki],
    exp [T, Ke], euler and trans [T, 3] (None: zeros, without reading any) -> vertex [T, N, 3], written to `out` when given (contiguous
    fp32 of that shape).  No sync."""
    mean, idb, expb = arrays
    dev, T = mean.device, id.shape[0]
    N, Ki, Ke = mean.numel() // 3, idb.shape[1], expb.shape[1]
    idc, expc = _coeff(id, "id", T, Ki, dev), _coeff(exp, "exp", T, Ke, dev)
    eu, tr = _coeff(euler, "euler", T, 3, dev), _coeff(trans, "trans", T, 3, dev)
    if out is None:
        out = torch.empty(T, N, 3, device=dev, dtype=torch.float32)
    elif out.shape != (T, N, 3) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
        raise ValueError("face_vertex: out must be a contiguous float32 [%d, %d, 3] tensor on %s" % (T, N, dev))
    with torch.cuda.device(dev):
        _lib.call("r3d_face_vertex", mean, idb, expb if Ke else None, N, Ki, Ke, idc, expc if Ke else None, eu, tr, T, float(camera_distance),
                  int(bool(to_camera)), out)
    return out


@torch.no_grad()
def face_landmarks(arrays, id, exp=None, euler=None, trans=None, camera_distance=CAMERA_DISTANCE, to_camera=True, focal=FOCAL, center=CENTER,
                   image_size=IMAGE_SIZE):
    """r3d_face_landmarks on arrays = (key_mean [3 L], key_id_base [3 L, Ki], key_exp_base [3 L, Ke]) -> lm2d [T, L, 2].  No sync."""
    mean, idb, expb = arrays
    dev, T = mean.device, id.shape[0]
    L, Ki, Ke = mean.numel() // 3, idb.shape[1], expb.shape[1]
    idc, expc = _coeff(id, "id", T, Ki, dev), _coeff(exp, "exp", T, Ke, dev)
    eu, tr = _coeff(euler, "euler", T, 3, dev), _coeff(trans, "trans", T, 3, dev)
    out = torch.empty(T, L, 2, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        _lib.call("r3d_face_landmarks", mean, idb, expb if Ke else None, L, Ki, Ke, idc, expc if Ke else None, eu, tr, T, float(camera_distance),
                  int(bool(to_camera)), float(focal), float(center), float(image_size), out)
    return out


def model_arrays(face_model, dev):
    """(mean_shape, id_base, exp_base) of a ParametricFaceModel-like object on dev, uploaded once."""
    return _arrays(face_model, ("mean_shape", "id_base", "exp_base"), dev)


def key_arrays(helper, dev):
    """(key_mean_shape, key_id_base, key_exp_base) of a Face3DHelper-like object on dev, uploaded once."""
    return _arrays(helper, ("key_mean_shape", "key_id_base", "key_exp_base"), dev)


def compute_face_vertex(face_model, id, exp, angle, trans):
    """bfm.py:332-347: id [B, Ki], exp [B, Ke], angle [B, 3] radians, trans [B, 3] -> face_vertex [B, N, 3] in camera coordinates
    (z = face_model.camera_distance - z), a new fp32 tensor on the coefficients' device."""
    dev = _device(id, getattr(face_model, "id_base", None))
    return face_vertex(model_arrays(face_model, dev), id, exp, angle, trans, camera_distance=float(face_model.camera_distance))


def reconstruct_lm2d(helper, id_coeff, exp_coeff, euler, trans, to_camera=True, focal=FOCAL, center=CENTER, image_size=IMAGE_SIZE,
                     camera_distance=CAMERA_DISTANCE):
    """face3d_helper.py:132-169: coefficients [T, C] or [B, T, C] -> lm2d [T, L, 2] or [B, T, L, 2] in [0, 1] image coordinates, y
    flipped.  focal, center, image_size and camera_distance default to the constants the reference has in its code."""
    dev = _device(id_coeff, getattr(helper, "key_id_base", None))
    btc = id_coeff.dim() == 3
    if btc:
        b, t = id_coeff.shape[:2]
        id_coeff, exp_coeff, euler, trans = (x.reshape(b * t, -1) for x in (id_coeff, exp_coeff, euler, trans))
    lm2d = face_landmarks(key_arrays(helper, dev), id_coeff, exp_coeff, euler, trans, camera_distance, to_camera, focal, center, image_size)
    return lm2d.reshape(b, t, -1, 2) if btc else lm2d


def patch_face_model(face_model):
    """Bind compute_face_vertex above as face_model's own method (a ParametricFaceModel, SECC_Renderer.face_model); the old one stays as
    face_model._r3d_reference_compute_face_vertex.  Returns face_model."""
    if not hasattr(face_model, "_r3d_reference_compute_face_vertex"):
        object.__setattr__(face_model, "_r3d_reference_compute_face_vertex", getattr(face_model, "compute_face_vertex", None))
    object.__setattr__(face_model, "compute_face_vertex", compute_face_vertex.__get__(face_model))
    return face_model


def patch_face3d_helper(helper):
    """Bind reconstruct_lm2d above as helper's own method (a Face3DHelper); the old one stays as
    helper._r3d_reference_reconstruct_lm2d.  Returns helper."""
    if not hasattr(helper, "_r3d_reference_reconstruct_lm2d"):
        object.__setattr__(helper, "_r3d_reference_reconstruct_lm2d", getattr(helper, "reconstruct_lm2d", None))
    object.__setattr__(helper, "reconstruct_lm2d", reconstruct_lm2d.__get__(helper))
    return helper
