"""HIP per-clip conditions: what lies between the fitted coefficients and the frame loop, on the device (r3d_clip_camera,
r3d_camera_smooth, r3d_smooth_features of include/r3d_hip_clip.h).

    camera_pose_intrinsic   (euler, trans) -> {'c2w', 'convention_c2w', 'intrinsics'}: get_eg3d_convention_camera_pose_intrinsic
                            (data_gen/eg3d/convert_to_eg3d_convention.py:42-146)
    smooth_camera_sequence  (camera [N, 25 | 16], kernel_size=7), in place: inference/infer_utils.py:40-69
    clip_camera             (euler, trans, kernel_size=7) -> camera [T, 25]: both in one launch, inference/real3d_infer.py:312-319
    smooth_features_xd      (in_tensor, kernel_size=7), ranks 2, 4, 5: infer_utils.py:71-101
    clip_keypoints          (src_kp, drv_kp, kernel_size=7) -> (kp_s, kp_d) [T, 68, 3]: real3d_infer.py:451-452 and 481-482 for the clip
    patch_infer_utils       binds smooth_features_xd in a module's namespace (the old one stays as _r3d_reference_smooth_features_xd)

INFERENCE ONLY: inputs are detached, must be contiguous fp32 tensors on a GPU (anything else raises) and are never written, except by
smooth_camera_sequence, which changes `camera` in place as the reference does.  No host synchronisation.  There is no fallback: without
the library, importing this raises.
"""
import torch

from . import _lib

CONVENTION_RADIUS = 2.7          # _fix_pose_orig, convert_to_eg3d_convention.py:31-39
_lib.load()


def _on_gpu(x, what):
    """x detached, after the checks _lib.call makes of a device pointer, in its order and with its exceptions, so that they read alike
    whichever comes first: fp32, contiguous, on a GPU."""
    if not torch.is_tensor(x):
        raise TypeError("%s: a tensor is needed, got %s" % (what, type(x).__name__))
    if x.dtype != torch.float32:
        raise TypeError("%s: a float32 tensor is needed, got %s" % (what, x.dtype))
    if not x.is_contiguous():
        raise ValueError("%s: the tensor is not contiguous" % what)
    if not x.is_cuda:
        raise ValueError("%s: the tensor is on %s; the kernels run on the GPU only" % (what, x.device))
    return x.detach()


def _pose(euler, trans, what):
    euler, trans = _on_gpu(euler, what), _on_gpu(trans, what)
    if euler.dim() != 2 or euler.shape[1] != 3 or trans.shape != euler.shape or euler.shape[0] < 1:
        raise ValueError("%s: euler and trans must be [T, 3] with T >= 1, got %s and %s" % (what, tuple(euler.shape), tuple(trans.shape)))
    return euler, trans


def _clip_camera(euler, trans, kernel_size, radius):
    out = torch.empty(euler.shape[0], 25, device=euler.device, dtype=torch.float32)
    with torch.cuda.device(euler.device):
        _lib.call("r3d_clip_camera", euler, trans, euler.shape[0], int(kernel_size), float(radius), out)
    return out


@torch.no_grad()
def clip_camera(euler, trans, kernel_size=7):
    """euler, trans [T, 3] -> camera [T, 25] = (smoothed c2w, intrinsics), one launch; what real3d_infer.py:312-319 leaves in
    sample['camera']."""
    euler, trans = _pose(euler, trans, "clip_camera")
    return _clip_camera(euler, trans, kernel_size, 0.0)


@torch.no_grad()
def camera_pose_intrinsic(euler, trans):
    """euler, trans [T, 3], or the reference's one-frame form [3] -> {'c2w' [T, 4, 4], 'convention_c2w' [T, 4, 4], 'intrinsics'
    [T, 3, 3]} ([4, 4], [4, 4], [3, 3] for one frame): the keys the reference adds to its item, unsmoothed, new fp32 tensors on the
    inputs' device."""
    one = torch.is_tensor(euler) and euler.dim() == 1
    if one:
        euler, trans = euler.unsqueeze(0), trans.unsqueeze(0)
    euler, trans = _pose(euler, trans, "camera_pose_intrinsic")
    T = euler.shape[0]
    cam = _clip_camera(euler, trans, 1, 0.0)
    conv = _clip_camera(euler, trans, 1, CONVENTION_RADIUS)
    ret = {"c2w": cam[:, :16].reshape(T, 4, 4), "convention_c2w": conv[:, :16].reshape(T, 4, 4), "intrinsics": cam[:, 16:].reshape(T, 3, 3)}
    ret = {k: v.contiguous() for k, v in ret.items()}          # (a reshape of a column slice is a strided view)
    return {k: v[0] for k, v in ret.items()} if one else ret


@torch.no_grad()
def smooth_camera_sequence(camera, kernel_size=7):
    """camera [N, 25] or [N, 16], a device tensor whose 3 x 3 blocks are rotations: smoothed into a temporary, copied back, returned."""
    cam = _on_gpu(camera, "smooth_camera_sequence")
    if cam.dim() != 2 or cam.shape[1] not in (16, 25) or cam.shape[0] < 1:
        raise ValueError("smooth_camera_sequence: camera must be [N, 25] or [N, 16] with N >= 1, got %s" % (tuple(cam.shape),))
    tmp = torch.empty_like(cam, memory_format=torch.contiguous_format)
    with torch.cuda.device(cam.device):
        _lib.call("r3d_camera_smooth", cam, cam.shape[1], cam.shape[0], int(kernel_size), tmp)
    cam.copy_(tmp)
    return camera


def _window(x, kernel_size, what):
    """The two conditions of the reference's padding, checked before anything else is asked of x."""
    kernel_size = int(kernel_size)
    pad = (kernel_size - 1) // 2
    if kernel_size < 1 or kernel_size % 2 == 0:
        raise ValueError("%s: kernel_size = %d must be odd and positive (the reference's padding fits odd sizes only)" % (what, kernel_size))
    if x.shape[0] < 1 or x.shape[0] < pad:
        raise ValueError("%s: T = %d frames, below the padding (kernel_size - 1) / 2 = %d" % (what, x.shape[0], pad))
    return kernel_size


def _smooth(x, kernel_size, zero_columns_every):
    """x [T, ...] -> [T, prod(...)] smoothed, with the zero columns: a new tensor [T, C + C / g]."""
    T = x.shape[0]
    C = x.numel() // T
    g = int(zero_columns_every)
    y = torch.empty(T, C + C // g if g else C, device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device):
        _lib.call("r3d_smooth_features", x, T, C, kernel_size, g, y)
    return y


@torch.no_grad()
def smooth_features_xd(in_tensor, kernel_size=7):
    """in_tensor [T, c], [T, c, h, w] or [T, c1, c2, h, w] -> the mean of kernel_size neighbouring frames with the reference's mirrored
    ends, contiguous, in the input's shape.  Other ranks raise NotImplementedError, as there."""
    if in_tensor.ndim not in (2, 4, 5):
        raise NotImplementedError()
    kernel_size = _window(in_tensor, kernel_size, "smooth_features_xd")
    x = _on_gpu(in_tensor, "smooth_features_xd")
    return _smooth(x, kernel_size, 0).reshape(x.shape)


@torch.no_grad()
def clip_keypoints(src_kp, drv_kp, kernel_size=7):
    """src_kp [T, 68, 2] or [1, 68, 2], drv_kp [T, 68, 2] -> (kp_s, kp_d), both [T, 68, 3]: kp_d is drv_kp smoothed over kernel_size
    frames, kp_s is src_kp as it is (one row is broadcast, not copied), each with a zero third column; the frame loop slices
    kp_s[i:i+1] and kp_d[i:i+1]."""
    if drv_kp.ndim != 3 or drv_kp.shape[2] != 2 or src_kp.ndim != 3 or src_kp.shape[1:] != drv_kp.shape[1:] or \
            src_kp.shape[0] not in (1, drv_kp.shape[0]):
        raise ValueError("clip_keypoints: drv_kp must be [T, L, 2] and src_kp [T, L, 2] or [1, L, 2], got %s and %s"
                         % (tuple(drv_kp.shape), tuple(src_kp.shape)))
    kernel_size = _window(drv_kp, kernel_size, "clip_keypoints")
    src, drv = _on_gpu(src_kp, "clip_keypoints"), _on_gpu(drv_kp, "clip_keypoints")
    T, L = drv.shape[0], drv.shape[1]
    kp_d = _smooth(drv, kernel_size, 2).reshape(T, L, 3)
    kp_s = _smooth(src, 1, 2).reshape(src.shape[0], L, 3)
    return kp_s.expand(T, L, 3), kp_d


def patch_infer_utils(module):
    """Point module.smooth_features_xd (inference/infer_utils.py, or a module that binds the name by `from inference.infer_utils import
    smooth_features_xd`) at the HIP function above; the old one stays as module._r3d_reference_smooth_features_xd.  The module's
    smooth_camera_sequence takes a NumPy array and is left alone: clip_camera replaces its call site.  Returns the module."""
    if not hasattr(module, "_r3d_reference_smooth_features_xd"):
        module._r3d_reference_smooth_features_xd = getattr(module, "smooth_features_xd", None)
    module.smooth_features_xd = smooth_features_xd
    return module
