"""HIP landmark-driven 3DMM fit: the Adam loops of fit_3dmm_for_a_image (data_gen/utils/process_image/fit_3dmm_landmark.py:85-264) and
fit_3dmm_for_a_video (data_gen/utils/process_video/fit_3dmm_landmark.py:130-459) in two kernels per iteration (r3d_fit_landmark_run of
include/r3d_hip_fit.h).

    landmark_weights        (kind, keypoint_mode) -> the [L] weights of cal_lan_loss_mp / cal_lan_loss
    fit_landmarks           (arrays, lms, weights, id_rows, lambdas) -> id, exp, euler, trans on the device and the loss record
    fit_3dmm_for_landmarks  (face_model, lms, img_size, kind, id_mode, keypoint_mode) -> the reference's coeff_dict
    patch_fit_3dmm          sets a module's fit_3dmm_for_a_image / fit_3dmm_for_a_video to wrappers over the above

The schedule is the reference's: 200 iterations of the landmark term with Adam([euler, trans], lr=.1), then 200 of the whole loss with
Adam([id, exp], lr=.1) from its step 1 beside the frame optimiser, which continues with its moments and step count.  THE FINE STAGE IS
NOT BUILT: it is dead code in the reference.  `exp_para[sel_ids].data = ...` (process_video :355-358, process_image :234-237) indexes
with a NumPy array, which makes a copy, so the assignment changes nothing, and the returned coeff_dict is the state after stage 2.  The
loss the reference would print is NaN with id_mode='global' (cal_vel_loss of one row is the mean of an empty tensor, at weight 0); the
loss record here leaves the two zero-weight velocity terms out.

INFERENCE TOOL ONLY: no autograd graph is built, inputs are never written.  There is no fallback: without the library, importing this
raises.  mediapipe and cv2 stay the caller's: they are imported only by the default landmark sources of patch_fit_3dmm.
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib
from . import face_model as _fm

UNMATCHED = (93, 127, 132, 234, 323, 356, 361, 454)
UPPER_EYE = (161, 160, 159, 158, 157) + (388, 387, 386, 385, 384)
EYE = (33, 246, 161, 160, 159, 158, 157, 173, 133, 155, 154, 153, 145, 144, 163, 7) + \
      (263, 466, 388, 387, 386, 385, 384, 398, 362, 382, 381, 380, 374, 373, 390, 249)
INNER_LIP = (78, 191, 80, 81, 82, 13, 312, 311, 310, 415, 308, 324, 318, 402, 317, 14, 87, 178, 88, 95)
OUTER_LIP = (61, 185, 40, 39, 37, 0, 267, 269, 270, 409, 291, 375, 321, 405, 314, 17, 84, 181, 91, 146)

# reg id, reg exp, lap id, lap exp, lap euler, lap trans (LAMBDA_REG_* and the factors of loss_lap in the two files)
LAMBDAS = {("image", "finegrained"): (0.3, 0.05, 0.0, 0.0, 0.0, 0.0),
           ("video", "global"): (0.2, 0.6, 1.0, 1.0, 0.3, 0.3),
           ("video", "finegrained"): (0.3, 0.05, 1.0, 1.0, 0.3, 0.3)}
ITERS, LR = (200, 200), 0.1
NAMES = ("id", "exp", "euler", "trans")
LOSS_NAMES = ("lan", "reg_id", "reg_exp", "lap_id", "lap_exp", "lap_euler", "lap_trans", "total")
RUNS_PER_FIT = 2          # library calls of one fit: stage 1 and stage 2


def landmark_weights(kind="image", keypoint_mode="mediapipe"):
    """The weights of the landmark term as an [L] float32 array: cal_lan_loss_mp of the image file (eyes 5, lips 2) or of the video file
    (eyes 3, upper eyes 20, lips 5), the eight unmatched points 0; keypoint_mode='lm68': cal_lan_loss (eyes, inner lip and nose 3)."""
    if kind not in ("image", "video"):
        raise ValueError("landmark_weights: kind is 'image' or 'video', got %r" % (kind,))
    if keypoint_mode != "mediapipe":
        w = np.ones(68, np.float32)
        w[36:48] = 3
        w[-8:] = 3
        w[28:31] = 3
        return w
    w = np.ones(468, np.float32)
    if kind == "image":
        w[list(EYE)] = 5
        w[list(INNER_LIP)] = 2
        w[list(OUTER_LIP)] = 2
    else:
        w[list(EYE)] = 3
        w[list(UPPER_EYE)] = 20
        w[list(INNER_LIP)] = 5
        w[list(OUTER_LIP)] = 5
    w[list(UNMATCHED)] = 0
    return w


def state_views(state, Ki, Ke, T, id_rows):
    """The state of r3d_fit_landmark_run as views: {'p' | 'm' | 'v': (id, exp, euler, trans)} and 'loss' [8]."""
    n = (id_rows * Ki, T * Ke, T * 3, T * 3)
    shapes = ((id_rows, Ki), (T, Ke), (T, 3), (T, 3))
    out, o = {}, 0
    for part in ("p", "m", "v"):
        views = []
        for k, s in zip(n, shapes):
            views.append(state[o:o + k].view(s))
            o += k
        out[part] = tuple(views)
    out["loss"] = state[o:o + _lib.FIT_LOSS_WORDS]
    return out


def _sizes(arrays, lms, weights, id_rows):
    mean, idb, expb = arrays
    L, Ki, Ke = mean.numel() // 3, idb.shape[1], expb.shape[1]
    if lms.dim() != 3 or lms.shape[1:] != (L, 2):
        raise ValueError("fit_3dmm: lms must be [T, %d, 2], got %s" % (L, tuple(lms.shape)))
    T = lms.shape[0]
    if weights.shape != (L,):
        raise ValueError("fit_3dmm: weights must be [%d], got %s" % (L, tuple(weights.shape)))
    if id_rows not in (1, T):
        raise ValueError("fit_3dmm: id_rows is 1 or T = %d, got %r" % (T, id_rows))
    return L, Ki, Ke, T


def _lambdas(lambdas):
    if len(lambdas) != 6:
        raise ValueError("fit_3dmm: lambdas are six numbers (reg id, reg exp, lap id, lap exp, lap euler, lap trans)")
    return (ctypes.c_float * 6)(*[float(x) for x in lambdas])


def _dev32(x, dev):
    return torch.as_tensor(x).detach().to(device=dev, dtype=torch.float32).contiguous()


@torch.no_grad()
def run(arrays, lms, weights, id_rows, lambdas, state, workspace, n_iter, groups, steps0=(0, 0), lr=(LR, LR),
        camera_distance=_fm.CAMERA_DISTANCE, focal=_fm.FOCAL, center=_fm.CENTER):
    """r3d_fit_landmark_run on tensors that are already contiguous fp32 on the device: 2 n_iter launches, no sync.  state is updated in
    place; steps0 = (steps the id / exp moments have seen, steps the euler / trans moments have seen)."""
    L, Ki, Ke, T = _sizes(arrays, lms, weights, id_rows)
    mean, idb, expb = arrays
    with torch.cuda.device(mean.device):
        _lib.call("r3d_fit_landmark_run", mean, idb, expb if Ke else None, L, Ki, Ke, lms, weights, T, id_rows, float(camera_distance), float(focal),
                  float(center), _lambdas(lambdas), float(lr[0]), float(lr[1]), int(steps0[0]), int(steps0[1]), int(n_iter), int(groups), state,
                  workspace, workspace.numel() * workspace.element_size())
    return state


@torch.no_grad()
def landmark_grad(arrays, lms, weights, id_rows, lambdas, id, exp, euler, trans, camera_distance=_fm.CAMERA_DISTANCE, focal=_fm.FOCAL,
                  center=_fm.CENTER):
    """r3d_fit_landmark_grad: one evaluation -> (loss record [8], grad_id, grad_exp, grad_euler, grad_trans), device tensors, no sync."""
    mean, idb, expb = arrays
    dev = mean.device
    lms, weights = _dev32(lms, dev), _dev32(weights, dev)
    L, Ki, Ke, T = _sizes(arrays, lms, weights, id_rows)
    p = [_dev32(x, dev) for x in (id, exp, euler, trans)]
    g = [torch.empty_like(x) for x in p]
    loss = torch.empty(_lib.FIT_LOSS_WORDS, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        ws = torch.empty(_lib.call("r3d_fit_workspace_bytes", L, Ki, Ke, T) // 4, device=dev, dtype=torch.float32)
        _lib.call("r3d_fit_landmark_grad", mean, idb, expb if Ke else None, L, Ki, Ke, lms, weights, T, id_rows, float(camera_distance), float(focal),
                  float(center), _lambdas(lambdas), p[0], p[1] if Ke else None, p[2], p[3], g[0], g[1] if Ke else None, g[2], g[3], loss, ws,
                  ws.numel() * 4)
    return (loss,) + tuple(g)


@torch.no_grad()
def fit_landmarks(arrays, lms, weights, id_rows, lambdas, iters=ITERS, lr=LR, camera_distance=_fm.CAMERA_DISTANCE, focal=_fm.FOCAL,
                  center=_fm.CENTER, stages=False):
    """The reference's schedule from zeros on arrays = (key_mean [3 L], key_id_base [3 L, Ki], key_exp_base [3 L, Ke]), contiguous fp32 on
    the GPU: lms [T, L, 2] in the 224-pixel frame with y up, weights [L], id_rows 1 (one id for the clip) or T, lambdas six numbers.
    Two library calls: iters[0] iterations of the landmark term stepping euler and trans, then iters[1] of the whole loss stepping all four,
    the frame group's step count carried on.  -> id [id_rows, Ki], exp [T, Ke], euler [T, 3], trans [T, 3] and the loss record [8]
    (LOSS_NAMES) of the last iterate consumed, device tensors; with stages=True a sixth value, the four after stage 1.  No sync."""
    mean = arrays[0]
    dev = mean.device
    lms, weights = _dev32(lms, dev), _dev32(weights, dev)
    L, Ki, Ke, T = _sizes(arrays, lms, weights, id_rows)
    with torch.cuda.device(dev):
        state = torch.zeros(_lib.call("r3d_fit_state_bytes", Ki, Ke, T, id_rows) // 4, device=dev, dtype=torch.float32)
        ws = torch.empty(_lib.call("r3d_fit_workspace_bytes", L, Ki, Ke, T) // 4, device=dev, dtype=torch.float32)
    cam = dict(camera_distance=camera_distance, focal=focal, center=center)
    run(arrays, lms, weights, id_rows, (0.0,) * 6, state, ws, iters[0], 2, (0, 0), (lr, lr), **cam)
    first = tuple(x.clone() for x in state_views(state, Ki, Ke, T, id_rows)["p"]) if stages else None
    run(arrays, lms, weights, id_rows, lambdas, state, ws, iters[1], 3, (0, iters[0]), (lr, lr), **cam)
    v = state_views(state, Ki, Ke, T, id_rows)
    out = v["p"] + (v["loss"],)
    return out + (first,) if stages else out


def prepare_landmarks(lms, img_size, L, dev):
    """The reference's preprocessing, in fp32 as it runs it: the first 468 points, y <- img_size - y, then the division by
    img_size / 224 -> [T, L, 2] on dev.  lms [T, >= L, 2], or [>= L, 2] for one image."""
    t = torch.as_tensor(np.asarray(lms) if not torch.is_tensor(lms) else lms).detach().to(dtype=torch.float32)
    if t.dim() == 2:
        t = t.unsqueeze(0)
    t = t[:, :468, :]
    if t.dim() != 3 or t.shape[1] != L or t.shape[2] != 2:
        raise ValueError("fit_3dmm: the landmarks %s do not give [T, %d, 2] after the cut to 468 points" % (tuple(t.shape), L))
    t = t.to(dev).clone()
    t[..., 1] = img_size - t[..., 1]
    t /= img_size / (2.0 * _fm.CENTER)
    return t.contiguous()


def fit_3dmm_for_landmarks(face_model, lms, img_size, kind="image", id_mode="global", keypoint_mode="mediapipe", as_numpy=True, device=None):
    """The reference's coeff_dict {'id', 'exp', 'euler', 'trans'} for landmarks in pixels of a square img_size image (y down, as mediapipe
    gives them): kind='image' is fit_3dmm_for_a_image (one frame, id [1, Ki]), kind='video' fit_3dmm_for_a_video with id_mode 'global'
    (id [1, Ki]) or 'finegrained' (id [T, Ki]); exp [T, Ke], euler and trans [T, 3].  float32 numpy arrays, or device tensors with
    as_numpy=False (then no sync).  face_model: any object with ParametricFaceModel's key_mean_shape, key_id_base, key_exp_base (uploaded
    once per object and device) and, optionally, focal, center and camera_distance."""
    if kind == "image":
        id_mode = "finegrained"
    elif kind != "video":
        raise ValueError("fit_3dmm_for_landmarks: kind is 'image' or 'video', got %r" % (kind,))
    if id_mode not in ("global", "finegrained"):
        raise NotImplementedError("id mode %s not supported! we only support global or finegrained." % id_mode)
    dev = torch.device("cuda" if device is None else device)
    arrays = _fm._arrays(face_model, ("key_mean_shape", "key_id_base", "key_exp_base"), dev)
    center = float(getattr(face_model, "center", _fm.CENTER))
    if center != _fm.CENTER:
        raise NotImplementedError("fit_3dmm_for_landmarks: the landmarks are scaled to a 224-pixel frame; center = %g is not supported" % center)
    w = landmark_weights(kind, keypoint_mode)
    t = prepare_landmarks(lms, float(img_size), len(w), arrays[0].device)
    if kind == "image" and t.shape[0] != 1:
        raise ValueError("fit_3dmm_for_landmarks: kind='image' takes the landmarks of one image, got %d frames" % t.shape[0])
    id_rows = 1 if id_mode == "global" else t.shape[0]
    out = fit_landmarks(arrays, t, torch.from_numpy(w), id_rows, LAMBDAS[(kind, id_mode)], focal=float(getattr(face_model, "focal", _fm.FOCAL)),
                        center=center, camera_distance=float(getattr(face_model, "camera_distance", _fm.CAMERA_DISTANCE)))
    return {n: (x.cpu().numpy() if as_numpy else x) for n, x in zip(NAMES, out[:4])}


def _image_source(img_name):
    """The default landmark source of the image wrapper: the reference's own lookup.  -> (lms or None, img_h)."""
    import cv2
    img_h = cv2.imread(img_name).shape[0]
    lm_name = img_name.replace("/images_512/", "/lms_2d/").replace(".png", "_lms.npy")
    if lm_name.endswith("_lms.npy") and os.path.exists(lm_name):
        return np.load(lm_name), img_h
    from data_gen.utils.mp_feature_extractors.face_landmarker import MediapipeLandmarker
    return MediapipeLandmarker().extract_lm478_from_img_name(img_name), img_h


def _video_source(video_name, nerf=False):
    """The default landmark source of the video wrapper: the reference's own lookup.  -> (lms or None, img_h)."""
    from data_gen.utils.mp_feature_extractors.face_landmarker import MediapipeLandmarker, read_video_to_frames
    frames = read_video_to_frames(video_name)
    img_h = frames.shape[1]
    lm_name = video_name.replace("/raw/", "/processed/").replace(".mp4", "/lms_2d.npy") if nerf else \
        video_name.replace("/video/", "/lms_2d/").replace(".mp4", "_lms.npy")
    if os.path.exists(lm_name):
        return np.load(lm_name), img_h
    landmarker = MediapipeLandmarker()
    img_lm478, vid_lm478 = landmarker.extract_lm478_from_frames(frames, anti_smooth_factor=20)
    return landmarker.combine_vid_img_lm478_to_lm478(img_lm478, vid_lm478), img_h


def _save(out_name, coeff_dict):
    try:
        os.makedirs(os.path.dirname(out_name), exist_ok=True)
    except OSError:
        pass
    np.save(out_name, coeff_dict, allow_pickle=True)


def patch_fit_3dmm(module, face_model, image_landmarks=None, video_landmarks=None):
    """Set module.fit_3dmm_for_a_image and module.fit_3dmm_for_a_video (inference/real3d_infer.py imports both names) to wrappers with the
    reference's arguments and returns that fit on the device; the replaced functions stay reachable as
    module._r3d_reference_fit_3dmm_for_a_image / _video.  face_model: the ParametricFaceModel whose key arrays the fit uses.
    image_landmarks(img_name) / video_landmarks(video_name) -> (landmarks in pixels or None, the square image's side); the defaults are
    the reference's lookup: the _lms.npy file it looks for, else its MediapipeLandmarker (imported then, with cv2).  debug=True (the
    reference's drawings) is not served.  Returns module."""
    image_source = image_landmarks or _image_source
    video_source = video_landmarks or (lambda name, nerf=False: _video_source(name, nerf))

    def fit_3dmm_for_a_image(img_name, debug=False, keypoint_mode="mediapipe", device="cuda:0", save=True):
        if debug:
            raise NotImplementedError("fit_3dmm_for_a_image: debug drawings are the reference's (_r3d_reference_fit_3dmm_for_a_image)")
        try:
            lms, img_h = image_source(img_name)
        except Exception as e:          # the reference prints and returns None
            print(e)
            return None
        if lms is None:
            print("get None lms_2d, please check whether each frame has one head, exiting...")
            return None
        lms = np.asarray(lms)[:468].reshape(-1, 2)
        coeff_dict = fit_3dmm_for_landmarks(face_model, lms, img_h, "image", keypoint_mode=keypoint_mode, device=device)
        if save:
            tag = "coeff_fit_mp" if keypoint_mode == "mediapipe" else "coeff_fit_lm68"
            _save(img_name.replace("/images_512/", "/%s/" % tag).replace(".png", "_%s.npy" % tag), coeff_dict)
        return coeff_dict

    def fit_3dmm_for_a_video(video_name, nerf=False, id_mode="global", debug=False, keypoint_mode="mediapipe", large_yaw_threshold=9999999.9,
                             save=True):
        assert video_name.endswith(".mp4"), "this function only support video as input"
        if debug:
            raise NotImplementedError("fit_3dmm_for_a_video: the debug video is the reference's (_r3d_reference_fit_3dmm_for_a_video)")
        if id_mode not in ("global", "finegrained"):
            raise NotImplementedError("id mode %s not supported! we only support global or finegrained." % id_mode)
        try:
            lms, img_h = video_source(video_name, nerf) if video_landmarks is None else video_source(video_name)
        except Exception as e:          # the reference prints and returns False
            print(e)
            return False
        if lms is None:
            print("get None lms_2d, please check whether each frame has one head, exiting... %s" % video_name)
            return False
        coeff_dict = fit_3dmm_for_landmarks(face_model, lms, img_h, "video", id_mode=id_mode, keypoint_mode=keypoint_mode)
        if save:
            mp = keypoint_mode == "mediapipe"
            if nerf:
                out_name = video_name.replace("/raw/", "/processed/").replace(".mp4", "/coeff_fit_mp.npy" if mp else "_coeff_fit_lm68.npy")
            else:
                tag = "coeff_fit_mp" if mp else "coeff_fit_lm68"
                out_name = video_name.replace("/video/", "/%s/" % tag).replace(".mp4", "_%s.npy" % tag)
            _save(out_name, coeff_dict)
        return coeff_dict

    for name, fn in (("fit_3dmm_for_a_image", fit_3dmm_for_a_image), ("fit_3dmm_for_a_video", fit_3dmm_for_a_video)):
        if not hasattr(module, "_r3d_reference_" + name):
            setattr(module, "_r3d_reference_" + name, getattr(module, name, None))
        setattr(module, name, fn)
    return module
