"""The per-clip conditions in NumPy, fp64: the camera trajectory of inference/real3d_infer.py:312-319
(get_eg3d_convention_camera_pose_intrinsic, data_gen/eg3d/convert_to_eg3d_convention.py:42-146, then smooth_camera_sequence,
inference/infer_utils.py:40-69) and smooth_features_xd (infer_utils.py:71-101), restated from the rule include/r3d_hip_clip.h states.
NumPy only: no torch, no scipy (the chordal mean is np.linalg.eigh of sum q q^T).  The inputs are the fp32 arrays the kernels get; every
operation is fp64; the only fp32 roundings are the ones the rule names (the frame's own camera, the result)."""
import numpy as np

FX = 2985.29 / 700
INTRINSICS = np.array([FX, 0, 0.5, 0, FX, 0.5, 0, 0, 1], np.float64)
OFFSET = np.array([0.0, 0.006, 0.161])


def uniform(seed, shape, bound):
    """The tests' inputs: float32 uniform in (-bound, bound), from the project's hash."""
    from real3dportrait_amd import synth
    u = synth.hash_uniform(seed, int(np.prod(shape)), stream=90).reshape(shape)
    return ((2.0 * u.astype(np.float64) - 1.0) * bound).astype(np.float32)


def trajectory(T, T0=0):
    """Frames T0 .. T0 + T of a smooth head movement: (euler [T, 3], trans [T, 3]) float32, sinusoids of a few seconds' period."""
    t = np.arange(T0, T0 + T, dtype=np.float64)[:, None]
    euler = np.array([0.35, 0.5, 0.2]) * np.sin(2 * np.pi * t / np.array([97.0, 61.0, 43.0]) + np.array([0.3, 1.1, 2.0]))
    trans = np.array([0.3, 0.2, 0.25]) * np.cos(2 * np.pi * t / np.array([83.0, 131.0, 57.0]) + np.array([0.7, 0.2, 1.5]))
    return euler.astype(np.float32), trans.astype(np.float32)


def rotation(euler):
    """compute_rotation (bfm.py:204-238) of one frame: (Rz Ry Rx)^T."""
    x, y, z = (float(v) for v in euler)
    rx = np.array([[1, 0, 0], [0, np.cos(x), -np.sin(x)], [0, np.sin(x), np.cos(x)]])
    ry = np.array([[np.cos(y), 0, np.sin(y)], [0, 1, 0], [-np.sin(y), 0, np.cos(y)]])
    rz = np.array([[np.cos(z), -np.sin(z), 0], [np.sin(z), np.cos(z), 0], [0, 0, 1]])
    return (rz @ ry @ rx).T


def quaternion(m):
    """A proper rotation to its unit quaternion (x, y, z, w), from the largest component (Shepperd): 4 w^2 = 1 + trace,
    4 x^2 = 1 - trace + 2 m00, ..., and the products 4 x y = m10 + m01, 4 x w = m21 - m12, ... give the others."""
    m = np.asarray(m, np.float64)
    sq = np.array([m[0, 0], m[1, 1], m[2, 2], np.trace(m)])
    i = int(np.argmax(sq))
    q = np.empty(4)
    if i == 3:
        q[:] = m[2, 1] - m[1, 2], m[0, 2] - m[2, 0], m[1, 0] - m[0, 1], 1 + sq[3]
    else:
        j, k = (i + 1) % 3, (i + 2) % 3
        q[i], q[j], q[k], q[3] = 1 - sq[3] + 2 * m[i, i], m[j, i] + m[i, j], m[k, i] + m[i, k], m[k, j] - m[j, k]
    return q / np.linalg.norm(q)


def matrix(q):
    x, y, z, w = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def frame_cameras(euler, trans, radius=0.0):
    """F: euler, trans [T, 3] -> c2w [T, 4, 4], fp32 values held in fp64 (the rule rounds a frame's own camera to fp32)."""
    euler, trans = np.asarray(euler, np.float64).reshape(-1, 3), np.asarray(trans, np.float64).reshape(-1, 3)
    out = np.zeros((euler.shape[0], 4, 4))
    for t in range(euler.shape[0]):
        R = rotation(euler[t])
        c = -(R @ (trans[t] + np.array([0.0, 0.0, -10.0]))) * 0.27 + OFFSET
        if radius > 0:
            c = c / np.linalg.norm(c) * radius
        out[t, :3, :3] = matrix(quaternion(R @ np.diag([1.0, -1.0, -1.0])))
        out[t, :3, 3] = c
        out[t, 3, 3] = 1
    return out.astype(np.float32).astype(np.float64)


def window_gaps(rots, kernel_size):
    """(lambda1 - lambda2) / n of every window's A = sum q q^T: what the chordal mean's conditioning depends on."""
    T, K = rots.shape[0], kernel_size // 2
    gaps = []
    for i in range(T):
        q = np.stack([quaternion(m) for m in rots[max(0, i - K):min(T, i + K + 1)]])
        lam = np.linalg.eigvalsh(q.T @ q)
        gaps.append((lam[3] - lam[2]) / q.shape[0])
    return np.array(gaps)


def smooth_camera(camera, kernel_size=7):
    """smooth_camera_sequence on camera [T, 16 | 25] (fp32 values) -> a new fp64 array of that shape, before the final rounding."""
    cam = np.asarray(camera, np.float64)
    T, K = cam.shape[0], kernel_size // 2
    poses = cam[:, :16].reshape(T, 4, 4)
    out = cam.copy()
    for i in range(T):
        j0, j1 = max(0, i - K), min(T, i + K + 1)
        if j1 - j0 == 1:
            continue                                          # the mean of one frame is that frame
        q = np.stack([quaternion(m[:3, :3]) for m in poses[j0:j1]])
        lam, vec = np.linalg.eigh(q.T @ q)
        p = poses[i].copy()
        p[:3, :3] = matrix(vec[:, 3])
        p[:3, 3] = poses[j0:j1, :3, 3].sum(0) / (j1 - j0)
        out[i, :16] = p.reshape(16)
    return out


def clip_camera(euler, trans, kernel_size=7, radius=0.0):
    """r3d_clip_camera: [T, 25] in fp64, before the final rounding to fp32."""
    F = frame_cameras(euler, trans, radius)
    cam = np.concatenate([F.reshape(-1, 16), np.broadcast_to(INTRINSICS, (F.shape[0], 9))], axis=1)
    return smooth_camera(cam, kernel_size)


def smooth_features(x, kernel_size=7, zero_columns_every=0):
    """smooth_features_xd on x [T, ...] -> the same shape in fp64; with zero_columns_every = g the LAST axis gets a zero after every g
    values (the rule flattens everything behind the frames; the tests group along the last axis only)."""
    x = np.asarray(x, np.float64)
    T, pad = x.shape[0], (kernel_size - 1) // 2
    assert kernel_size % 2 == 1 and T >= pad
    padded = np.concatenate([x[:pad][::-1], x, x[T - pad:][::-1]], axis=0)
    y = sum(padded[k:k + T] for k in range(kernel_size)) / kernel_size
    g = zero_columns_every
    if g > 0:
        y = y.reshape(y.shape[:-1] + (y.shape[-1] // g, g))
        y = np.concatenate([y, np.zeros(y.shape[:-1] + (1,))], axis=-1).reshape(y.shape[:-2] + (-1,))
    return y
