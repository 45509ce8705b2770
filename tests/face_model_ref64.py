"""The morphable face model's two functions in NumPy, fp64 by default: ParametricFaceModel.compute_face_vertex
(deep_3drecon/deep_3drecon_models/bfm.py:332-347) and Face3DHelper.reconstruct_lm2d (data_util/face3d_helper.py:132-169), restated line
by line.  No torch.  Inputs of any float type are promoted to `dtype` before the first operation."""
import numpy as np


def rotation(euler, dtype=np.float64):
    """compute_rotation (bfm.py:204-238): euler [T, 3] radians -> rot [T, 3, 3] = (Rz Ry Rx)^T, to be used as p @ rot."""
    e = np.asarray(euler, dtype)
    T = e.shape[0]
    x, y, z = e[:, 0], e[:, 1], e[:, 2]
    one, zero = np.ones(T, dtype), np.zeros(T, dtype)
    rx = np.stack([one, zero, zero, zero, np.cos(x), -np.sin(x), zero, np.sin(x), np.cos(x)], axis=1).reshape(T, 3, 3)
    ry = np.stack([np.cos(y), zero, np.sin(y), zero, one, zero, -np.sin(y), zero, np.cos(y)], axis=1).reshape(T, 3, 3)
    rz = np.stack([np.cos(z), -np.sin(z), zero, np.sin(z), np.cos(z), zero, zero, zero, one], axis=1).reshape(T, 3, 3)
    return np.transpose(rz @ ry @ rx, (0, 2, 1))


def face_vertex(mean, id_base, exp_base, id, exp=None, euler=None, trans=None, camera_distance=10.0, to_camera=True, dtype=np.float64):
    """mean [3 N] (any shape of 3 N numbers), id_base [3 N, Ki], exp_base [3 N, Ke], id [T, Ki], exp [T, Ke], euler, trans [T, 3] (None:
    zeros) -> vertex [T, N, 3]."""
    mean, idb, idc = np.asarray(mean, dtype).reshape(-1), np.asarray(id_base, dtype), np.asarray(id, dtype)
    T = idc.shape[0]
    shape = idc @ idb.T
    if exp is not None and np.asarray(exp_base).shape[1] > 0:
        shape = shape + np.asarray(exp, dtype) @ np.asarray(exp_base, dtype).T
    shape = (shape + mean[None]).reshape(T, -1, 3)
    rot = rotation(np.zeros((T, 3)) if euler is None else euler, dtype)
    tr = np.zeros((T, 3), dtype) if trans is None else np.asarray(trans, dtype)
    v = shape @ rot + tr[:, None, :]
    if to_camera:
        v[..., 2] = dtype(camera_distance) - v[..., 2]
    return v


def landmarks(key_mean, key_id_base, key_exp_base, id, exp=None, euler=None, trans=None, camera_distance=10.0, to_camera=True,
              focal=1015.0, center=112.0, image_size=224.0, dtype=np.float64):
    """reconstruct_lm2d: the same on the L key rows, then lm3d @ perspective_projection(focal, center), the division by the third
    component, y = image_size - y, both over image_size -> lm2d [T, L, 2]."""
    lm3d = face_vertex(key_mean, key_id_base, key_exp_base, id, exp, euler, trans, camera_distance, to_camera, dtype)
    proj = np.array([focal, 0, center, 0, focal, center, 0, 0, 1], dtype).reshape(3, 3).T
    p = lm3d @ proj
    lm2d = p[..., :2] / p[..., 2:]
    lm2d[..., 1] = dtype(image_size) - lm2d[..., 1]
    return lm2d / dtype(image_size)


def coefficients(seed, T, Ki=80, Ke=64):
    """The tests' inputs: id, exp ~ unit variance, euler ~ N(0, 0.3^2) rad, trans ~ N(0, 0.2^2), float32, from the project's hash."""
    from real3dportrait_amd import synth
    return (synth.hash_unitvar(seed, (T, Ki), stream=80), synth.hash_unitvar(seed, (T, Ke), stream=81),
            (0.3 * synth.hash_unitvar(seed, (T, 3), stream=82)).astype(np.float32),
            (0.2 * synth.hash_unitvar(seed, (T, 3), stream=83)).astype(np.float32))


def _fma32(a, b, c):
    """fmaf on float32 arrays: the product of two float32 is exact in float64, the sum is rounded there and then to float32 (a double
    rounding, which can differ from fmaf in the last place on rare ties; it does not move a largest error's printed digits)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def kernel_fp32(mean, id_base, exp_base, id, exp, euler, trans, camera_distance=10.0, to_camera=True, mean_first=False, landmarks=False,
                focal=1015.0, center=112.0, image_size=224.0):
    """The fp32 operations of csrc/r3d_face_model.hip in NumPy, one by one: the fma chain over k from 0 and then + mean (mean_first: the
    chain begun at the mean instead, as the kernel had it before), the rotation from float32 sines and cosines, q = M p + trans as two
    fmas on a product, the depth flip and, for landmarks, the projection.  For estimating what the kernel's arithmetic can reach, not
    for bit-identity with it: sin / cos are NumPy's, rounded to float32.  -> vertex [T, N, 3] or lm2d [T, N, 2], float32."""
    f32 = np.float32
    mean, idb, expb = np.asarray(mean, f32).reshape(-1), np.asarray(id_base, f32), np.asarray(exp_base, f32)
    idc, expc, euler, trans = (np.asarray(a, f32) for a in (id, exp, euler, trans))
    T, R = idc.shape[0], mean.shape[0]
    acc = np.tile(mean, (T, 1)) if mean_first else np.zeros((T, R), f32)
    for base, coef in ((idb, idc), (expb, expc)):
        for k in range(base.shape[1]):
            acc = _fma32(np.broadcast_to(base[None, :, k], (T, R)), np.broadcast_to(coef[:, k:k + 1], (T, R)), acc)
    p = (acc if mean_first else acc + mean[None]).reshape(T, -1, 3)
    sx, sy, sz = (np.sin(euler[:, i].astype(np.float64)).astype(f32) for i in range(3))
    cx, cy, cz = (np.cos(euler[:, i].astype(np.float64)).astype(f32) for i in range(3))
    a00, a01, a02, a10, a11, a12, a20, a22 = cz * cy, -sz, cz * sy, sz * cy, cz, sz * sy, -sy, cy          # Rz Ry
    M = np.stack([a00, _fma32(a02, sx, a01 * cx), _fma32(a02, cx, -(a01 * sx)), a10, _fma32(a12, sx, a11 * cx), _fma32(a12, cx, -(a11 * sx)),
                  a20, a22 * sx, a22 * cx], axis=1).reshape(T, 3, 3)
    px, py, pz = p[..., 0], p[..., 1], p[..., 2]
    col = lambda c, j: np.broadcast_to(M[:, c, j][:, None], px.shape)
    q = [_fma32(col(c, 2), pz, _fma32(col(c, 1), py, col(c, 0) * px)) + trans[:, c][:, None] for c in range(3)]
    if to_camera:
        q[2] = f32(camera_distance) - q[2]
    if not landmarks:
        return np.stack(q, axis=-1)
    u = [_fma32(np.full_like(q[c], f32(focal)), q[c], f32(center) * q[2]) / q[2] for c in range(2)]
    u[1] = f32(image_size) - u[1]
    return np.stack(u, axis=-1) / f32(image_size)
