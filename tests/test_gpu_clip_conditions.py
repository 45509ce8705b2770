"""GPU: the HIP per-clip conditions (r3d_clip_camera / r3d_camera_smooth / r3d_smooth_features, real3dportrait_amd/clip_conditions.py,
DESIGN 4.17) against the fp64 restatement tests/clip_conditions_ref64.py and the reference's recorded outputs, and their exact properties.

Bounds.  Cameras: |out - restatement| <= 2.4e-7, one fp32 ulp in [2, 4), the largest magnitude present (the position's z is about 2.8):
the kernels compute in fp64, so only the final rounding (half an ulp) and the libm's last bits remain; against the reference's recorded
output the fixture's ref_err_vs_fp64 is added (triangle inequality).  Features: (kernel_size + 2) 2^-24 max|x| against the restatement --
n - 1 roundings of partial sums bounded by n max|x|, the factor 1 / n, its own rounding and the product's -- and the same plus
ref_err_vs_fp64 against the reference's output.  Measured on the MI355X: cameras at most 1.2e-7 (half an ulp of z), features at most
1.4e-7 at kernel_size 7 and |x| < 1 (bound 5.4e-7)."""
import numpy as np
import pytest
import torch

from conftest import load_golden
import clip_conditions_ref64 as C64
from test_clip_conditions_host import CAMERA_CASES, FEATURE_CASES, feature_tol, split_camera

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CAM_TOL = 2.0 ** -22          # 2.4e-7
FX = np.float32(2985.29 / 700)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy().astype(np.float64)


def bits(t):
    return t.contiguous().view(torch.int32)


def two_step(euler, trans, ks):
    """camera_pose_intrinsic, the concatenation of real3d_infer.py:316, smooth_camera_sequence: (camera, the unsmoothed dict)."""
    from real3dportrait_amd import clip_conditions as CC
    ret = CC.camera_pose_intrinsic(euler, trans)
    T = euler.shape[0]
    camera = torch.cat([ret["c2w"].reshape(T, 16), ret["intrinsics"].reshape(T, 9)], dim=-1)
    assert CC.smooth_camera_sequence(camera, kernel_size=ks) is camera
    return camera, ret


def check_exact_parts(cam):
    """The bottom row, the intrinsics bit for bit, and that every block is a rotation."""
    T = cam.shape[0]
    c = cam.cpu().numpy()
    assert c.dtype == np.float32 and c.shape == (T, 25)
    want = np.array([0, 0, 0, 1, FX, 0, 0.5, 0, FX, 0.5, 0, 0, 1], np.float32)
    assert np.array_equal(c[:, 12:].view(np.int32), np.broadcast_to(want.view(np.int32), (T, 13)))
    rot = c[:, :16].reshape(T, 4, 4)[:, :3, :3].astype(np.float64)
    assert np.abs(np.transpose(rot, (0, 2, 1)) @ rot - np.eye(3)).max() <= 1e-6 and (np.linalg.det(rot) > 0).all()


@pytest.mark.parametrize("case", CAMERA_CASES)
def test_cameras_against_fp64_and_the_reference(case):
    from real3dportrait_amd import clip_conditions as CC
    g = load_golden("clip_cond_cam_" + case)
    ks, T = int(g["kernel_size"]), g["euler"].shape[0]
    euler, trans = dev(g["euler"]), dev(g["trans"])
    before = euler.clone(), trans.clone()
    one = CC.clip_camera(euler, trans, kernel_size=ks)
    two, unsmoothed = two_step(euler, trans, ks)
    assert torch.equal(euler, before[0]) and torch.equal(trans, before[1])
    assert torch.equal(bits(one), bits(two))                                       # the one launch and the two-step route
    check_exact_parts(one)
    ref = C64.clip_camera(g["euler"], g["trans"], ks)
    e_ref, e_rec = float(np.abs(host(one) - ref).max()), float(np.abs(host(one) - g["camera"].astype(np.float64)).max())
    print("%s: T %d kernel_size %d: |HIP - fp64| %.3e (bound %.3e), |HIP - reference| %.3e (bound %.3e)"
          % (case, T, ks, e_ref, CAM_TOL, e_rec, float(g["ref_err_vs_fp64"]) + CAM_TOL))
    assert e_ref <= CAM_TOL
    assert e_rec <= float(g["ref_err_vs_fp64"]) + CAM_TOL
    # the unsmoothed cameras
    assert unsmoothed["c2w"].shape == (T, 4, 4) and unsmoothed["convention_c2w"].shape == (T, 4, 4) and unsmoothed["intrinsics"].shape == (T, 3, 3)
    for key, radius in (("c2w", 0.0), ("convention_c2w", 2.7)):
        assert np.abs(host(unsmoothed[key]) - C64.frame_cameras(g["euler"], g["trans"], radius)).max() <= CAM_TOL, key
        if key in g:
            assert np.abs(host(unsmoothed[key]) - g[key].astype(np.float64)).max() <= float(g["ref_err_unsmoothed"]) + CAM_TOL, key
    first = CC.camera_pose_intrinsic(euler[0], trans[0])                              # the reference's one-frame form
    assert first["c2w"].shape == (4, 4) and first["intrinsics"].shape == (3, 3)
    assert all(torch.equal(bits(first[k]), bits(unsmoothed[k][0])) for k in first)
    if case == "c_t3_static":
        rot, _, _ = split_camera(host(one))
        assert np.abs(rot - host(unsmoothed["c2w"])[:, :3, :3]).max() <= CAM_TOL
    if "camera16" in g:                                                               # the [T, 16] form
        c16 = unsmoothed["c2w"].reshape(T, 16).clone()
        assert CC.smooth_camera_sequence(c16, ks) is c16
        assert torch.equal(bits(c16), bits(one[:, :16]))
        assert np.abs(host(c16) - g["camera16"].astype(np.float64)).max() <= float(g["ref_err_vs_fp64"]) + CAM_TOL


def test_radius_rescales_before_the_smoothing():
    """r3d_clip_camera with radius 2.7 and kernel_size 7 through the raw entry point: the restatement's bound, and bit-identical to
    smoothing the convention_c2w of camera_pose_intrinsic."""
    from real3dportrait_amd import _lib, clip_conditions as CC
    g = load_golden("clip_cond_cam_e_t41")
    euler, trans = dev(g["euler"]), dev(g["trans"])
    T = euler.shape[0]
    out = torch.empty(T, 25, device=DEV)
    _lib.call("r3d_clip_camera", euler, trans, T, 7, 2.7, out)
    check_exact_parts(out)
    assert np.abs(host(out) - C64.clip_camera(g["euler"], g["trans"], 7, 2.7)).max() <= CAM_TOL
    conv = CC.camera_pose_intrinsic(euler, trans)["convention_c2w"].reshape(T, 16)
    assert np.abs(np.linalg.norm(host(conv).reshape(T, 4, 4)[:, :3, 3], axis=1) - 2.7).max() <= 2 * CAM_TOL
    assert torch.equal(bits(CC.smooth_camera_sequence(conv, 7)), bits(out[:, :16]))


def test_a_longer_clip_changes_only_the_windows_it_reaches():
    """T = 257 (five waves, the last one ragged) against the restatement, and against T = 250 of the same trajectory: frames 0 .. 246,
    whose windows lie inside both clips, are bit-identical; so are a second run and a run on another stream."""
    from real3dportrait_amd import clip_conditions as CC
    e257, t257 = C64.trajectory(257)
    e250, t250 = C64.trajectory(250)
    assert np.array_equal(e257[:250], e250) and np.array_equal(t257[:250], t250)
    euler, trans = dev(e257), dev(t257)
    long = CC.clip_camera(euler, trans)
    short = CC.clip_camera(dev(e250), dev(t250))
    check_exact_parts(long)
    assert np.abs(host(long) - C64.clip_camera(e257, t257, 7)).max() <= CAM_TOL
    assert torch.equal(bits(long[:247]), bits(short[:247]))
    assert not torch.equal(bits(long[247:250]), bits(short[247:250]))             # the cut windows are other windows
    again = CC.clip_camera(euler, trans)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = CC.clip_camera(euler, trans)
    side.synchronize()
    assert torch.equal(bits(long), bits(again)) and torch.equal(bits(long), bits(other))
    two, _ = two_step(euler, trans, 7)
    assert torch.equal(bits(long), bits(two))


@pytest.mark.parametrize("case", FEATURE_CASES)
def test_features_against_fp64_and_the_reference(case):
    from real3dportrait_amd import clip_conditions as CC
    g = load_golden("clip_cond_feat_" + case)
    x_np, ks = g["x"], int(g["kernel_size"])
    x = dev(x_np)
    y = CC.smooth_features_xd(x, kernel_size=ks)
    assert y.shape == x.shape and y.dtype == torch.float32 and y.is_contiguous() and y.data_ptr() != x.data_ptr()
    assert torch.equal(bits(x), bits(dev(x_np)))                                    # the input is not written
    tol = feature_tol(x_np, ks)
    e_ref = float(np.abs(host(y) - C64.smooth_features(x_np, ks)).max())
    e_rec = float(np.abs(host(y) - g["y"].astype(np.float64)).max())
    print("%s: %s kernel_size %d: |HIP - fp64| %.3e (bound %.3e), |HIP - reference| %.3e (bound %.3e)"
          % (case, x_np.shape, ks, e_ref, tol, e_rec, tol + float(g["ref_err_vs_fp64"])))
    assert e_ref <= tol and e_rec <= tol + float(g["ref_err_vs_fp64"])
    if ks == 1:
        assert torch.equal(bits(y), bits(x))
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = CC.smooth_features_xd(x, kernel_size=ks)
    side.synchronize()
    assert torch.equal(bits(y), bits(CC.smooth_features_xd(x, kernel_size=ks))) and torch.equal(bits(y), bits(other))
    if x_np.ndim == 2 and x_np.shape[1] == 136:                                     # key points: [T, 68, 2]
        T = x_np.shape[0]
        drv = x.reshape(T, 68, 2)
        for src in (dev(C64.uniform(60, (T, 68, 2), 1.0)), dev(C64.uniform(61, (1, 68, 2), 1.0))):
            kept = src.clone()
            kp_s, kp_d = CC.clip_keypoints(src, drv, kernel_size=ks)
            assert kp_s.shape == kp_d.shape == (T, 68, 3) and kp_d.is_contiguous()
            assert torch.equal(bits(kp_d[..., :2]), bits(y.reshape(T, 68, 2)))          # the same sums, the zero column in between
            assert not bits(kp_d[..., 2]).any() and not bits(kp_s[..., 2]).any()        # +0.0f bit for bit
            assert torch.equal(bits(kp_s[..., :2]), bits(src.expand(T, 68, 2)))
            assert torch.equal(bits(src), bits(kept)) and torch.equal(bits(x), bits(dev(x_np)))
            assert kp_s[T - 1:T].shape == (1, 68, 3) and kp_d[T - 1:T].shape == (1, 68, 3)          # what the frame loop slices


def test_features_across_blocks_and_other_groupings():
    """[257, 9] with a zero after every 3 values: 257 x 12 outputs are more than one block and no multiple of it; T = pad at
    kernel_size 255, the largest, where every frame's window is mirrored at both ends."""
    from real3dportrait_amd import _lib
    x_np = C64.uniform(62, (257, 9), 4.0)
    x, y = dev(x_np), torch.full((257, 12), float("nan"), device=DEV)
    _lib.call("r3d_smooth_features", x, 257, 9, 5, 3, y)
    assert np.abs(host(y) - C64.smooth_features(x_np, 5, 3)).max() <= feature_tol(x_np, 5)
    assert not bits(y.reshape(257, 3, 4)[..., 3]).any()
    x_np = C64.uniform(63, (127, 3), 1.0)
    x, y = dev(x_np), torch.full((127, 3), float("nan"), device=DEV)
    _lib.call("r3d_smooth_features", x, 127, 3, 255, 0, y)
    assert np.abs(host(y) - C64.smooth_features(x_np, 255)).max() <= feature_tol(x_np, 255)


def test_c_entry_points_refuse_with_a_status_and_a_message():
    from real3dportrait_amd import _lib
    lib = _lib.load()
    st = _lib.stream_ptr()
    cam = torch.zeros(9, 25, device=DEV)
    out = torch.full((9, 25), 7.0, device=DEV)
    x, y = torch.zeros(9, 136, device=DEV), torch.full((9, 204), 7.0, device=DEV)
    e = torch.zeros(9, 3, device=DEV)
    p = lambda t: t.data_ptr()
    err = lambda: lib.r3d_last_error()
    assert lib.r3d_camera_smooth(p(cam), 25, 9, 7, p(cam), st) == -1 and b"camera_smooth:" in err() and b"overlaps" in err()
    assert lib.r3d_camera_smooth(p(cam), 25, 8, 7, p(cam) + 4 * 25, st) == -1 and b"overlaps" in err()
    assert lib.r3d_smooth_features(p(x), 9, 136, 7, 0, p(x), st) == -1 and b"smooth_features:" in err() and b"overlaps" in err()
    assert lib.r3d_clip_camera(p(e), p(e), 9, 7, 0.0, p(e), st) == -1 and b"clip_camera:" in err() and b"overlaps" in err()
    assert lib.r3d_clip_camera(p(e), p(e), 0, 7, 0.0, p(out), st) == -1 and b"must be positive" in err()
    assert lib.r3d_camera_smooth(p(cam), 25, 0, 7, p(out), st) == -1 and b"must be positive" in err()
    assert lib.r3d_smooth_features(p(x), 0, 136, 7, 2, p(y), st) == -1 and b"must be positive" in err()
    assert lib.r3d_smooth_features(p(x), 9, 136, 6, 2, p(y), st) == -1 and b"even" in err()
    assert lib.r3d_smooth_features(p(x), 2, 136, 7, 2, p(y), st) == -1 and b"below the padding" in err()
    assert lib.r3d_clip_camera(None, p(e), 9, 7, 0.0, p(out), st) == -1 and b"NULL pointer" in err()
    assert lib.r3d_camera_smooth(p(cam), 25, 9, 7, None, st) == -1 and b"NULL pointer" in err()
    assert lib.r3d_smooth_features(None, 9, 136, 7, 2, p(y), st) == -1 and b"NULL pointer" in err()
    with pytest.raises(RuntimeError, match="overlaps"):
        _lib.call("r3d_smooth_features", x, 9, 136, 7, 0, x)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((y == 7.0).all())                      # a refused call launches nothing
