"""CPU: the host side of the HIP per-clip conditions (real3dportrait_amd/clip_conditions.py, r3d_clip_camera / r3d_camera_smooth /
r3d_smooth_features of include/r3d_hip_clip.h).

The symbols; the fp64 restatement (tests/clip_conditions_ref64.py) against every output recorded from the reference
(tests/golden/clip_cond_*.npz); the argument checks of the Python functions and of the C entry points, which run before any HIP call.

Bounds of the restatement against the reference.  Cameras: 4 fp32 ulps at the entry class's largest magnitude, 9.5e-7 for the position
(|z| is about 2.8, an ulp in [2, 4) is 2.4e-7) and 4.8e-7 for the rotation (entries reach 1.0): the reference's rotation entries and
position are fp32 results a few ulps off, a window mean does not amplify that, and the eigenvector of a matrix whose gap is at least 0.25
(the maker asserts it) amplifies it by at most 1 / gap.  Features: (kernel_size + 2) 2^-24 max|x| -- n - 1 roundings of partial sums
bounded by n max|x|, the factor 1 / n, its own rounding and the product's."""
import ctypes
import glob
import os
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden
import clip_conditions_ref64 as C64

CAMERA_CASES = ("a_t1_zero", "b_t2", "c_t3_static", "d_t9_k7", "d_t9_k3", "d_t9_k1", "e_t41", "f_t70_smooth", "g_t12_k1_axes")
FEATURE_CASES = ("a_t3", "b_t4", "c_t7_k3", "d_t70", "e_rank4", "f_rank5", "g_k1")
POS_TOL, ROT_TOL = 4 * 2.0 ** -22, 4 * 2.0 ** -23          # 9.5e-7, 4.8e-7


def feature_tol(x, kernel_size):
    return (kernel_size + 2) * 2.0 ** -24 * float(np.abs(x).max())


def split_camera(cam):
    """camera [T, 16 | 25] -> (rotation [T, 3, 3], position [T, 3], the rest [T, 4 | 13])"""
    p = cam[:, :16].reshape(-1, 4, 4)
    return p[:, :3, :3], p[:, :3, 3], cam[:, 12:]


def test_every_fixture_is_listed_and_small():
    names = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "clip_cond_*.npz")))
    assert names == sorted(["clip_cond_cam_" + c for c in CAMERA_CASES] + ["clip_cond_feat_" + c for c in FEATURE_CASES])
    assert all(os.path.getsize(os.path.join(GOLDEN, n + ".npz")) <= 524288 for n in names)


def test_symbols_are_declared_exported_and_bound():
    """The three entry points live in the companion header include/r3d_hip_clip.h (tests/test_abi.py compares every declaration with the
    binding table and with what load() bound); here what is this unit's own: the parameter counts, the radius as a double, the ABI number
    and the package's names."""
    from real3dportrait_amd import _lib
    from abi import header_declarations
    import real3dportrait_amd
    lib = _lib.load()
    assert lib.r3d_version() == _lib.ABI_VERSION
    decls = header_declarations("r3d_hip_clip.h")
    assert set(decls) == {"r3d_clip_camera", "r3d_camera_smooth", "r3d_smooth_features"} <= set(_lib.SIGNATURES)
    assert [len(decls[n][1]) for n in ("r3d_clip_camera", "r3d_camera_smooth", "r3d_smooth_features")] == [7, 6, 7]
    assert decls["r3d_clip_camera"][1][4] == "double"                                  # the radius
    from real3dportrait_amd import clip_conditions
    for name in ("camera_pose_intrinsic", "smooth_camera_sequence", "clip_camera", "smooth_features_xd", "clip_keypoints", "patch_infer_utils"):
        assert getattr(real3dportrait_amd, name) is getattr(clip_conditions, name), name


@pytest.mark.parametrize("case", CAMERA_CASES)
def test_restatement_against_the_reference_cameras(case):
    g = load_golden("clip_cond_cam_" + case)
    ks = int(g["kernel_size"])
    ref = C64.clip_camera(g["euler"], g["trans"], ks)
    rec = g["camera"].astype(np.float64)
    assert rec.shape == ref.shape == (g["euler"].shape[0], 25)
    (rr, rp, rest), (gr, gp, grest) = split_camera(ref), split_camera(rec)
    er, ep = float(np.abs(rr - gr).max()), float(np.abs(rp - gp).max())
    print("%s: restatement against the reference: rotation %.3e (bound %.3e), position %.3e (bound %.3e)" % (case, er, ROT_TOL, ep, POS_TOL))
    assert er <= ROT_TOL and ep <= POS_TOL
    assert np.array_equal(rest.astype(np.float32), grest.astype(np.float32))          # the bottom row and the intrinsics
    assert abs(float(np.abs(ref - rec).max()) - float(g["ref_err_vs_fp64"])) < 1e-12          # (over all 25 columns, before the last rounding)
    # the conditions the maker asserts hold for the recorded inputs
    F = C64.frame_cameras(g["euler"], g["trans"])
    assert C64.window_gaps(F[:, :3, :3], ks).min() >= 0.25
    if case == "e_t41":
        for key, radius in (("c2w", 0.0), ("convention_c2w", 2.7)):
            f = C64.frame_cameras(g["euler"], g["trans"], radius)
            d = np.abs(f - g[key].astype(np.float64))
            assert d[:, :3, :3].max() <= ROT_TOL and d[:, :3, 3].max() <= POS_TOL and d[:, 3].max() == 0.0, key
        assert np.allclose(np.linalg.norm(g["convention_c2w"][:, :3, 3].astype(np.float64), axis=1), 2.7, atol=POS_TOL)
        assert int((1.0 + np.trace(F[:, :3, :3], axis1=1, axis2=2) < 1e-3).sum()) >= 4
    if case == "f_t70_smooth":
        assert np.array_equal(g["camera16"], g["camera"][:, :16])
        ref16 = C64.smooth_camera(C64.frame_cameras(g["euler"], g["trans"]).reshape(-1, 16), ks)
        assert np.array_equal(ref16, ref[:, :16])
    if case == "g_t12_k1_axes":
        assert {int(np.argmax(np.abs(C64.quaternion(m)))) for m in F[:, :3, :3]} == {0, 1, 2, 3}
    if case == "c_t3_static":
        # a static clip: the mean of identical blocks is the rotation next to that block; F's entries, rounded to fp32, lie within
        # 2^-24 of one, so it lies within 2^-24 of that one again
        assert np.abs(rr - F[:, :3, :3]).max() <= 2.0 ** -23


def test_restatement_is_a_rotation_at_the_trace_minus_one_point():
    """Zero pose: the block is exactly diag(1, -1, -1), the quaternion (1, 0, 0, 0); a static window's mean is the rotation itself."""
    z = np.zeros((5, 3), np.float32)
    cam = C64.clip_camera(z, z, 7)
    rot, pos, _ = split_camera(cam)
    assert np.array_equal(rot, np.broadcast_to(np.diag([1.0, -1.0, -1.0]), (5, 3, 3)))
    assert np.array_equal(C64.quaternion(np.diag([1.0, -1.0, -1.0])), [1.0, 0.0, 0.0, 0.0])
    want = np.float32(np.array([0.0, 0.006, 0.161 + 2.7]))
    assert np.abs(pos - want).max() <= 2.0 ** -23
    euler = C64.uniform(40, (30, 3), 3.0)
    for m in C64.frame_cameras(euler, np.zeros_like(euler))[:, :3, :3]:
        assert np.abs(C64.matrix(C64.quaternion(m)) - m).max() <= 2e-7          # m itself is rounded to fp32
        assert np.abs(m.T @ m - np.eye(3)).max() <= 4e-7 and np.linalg.det(m) > 0


@pytest.mark.parametrize("case", FEATURE_CASES)
def test_restatement_against_the_reference_features(case):
    g = load_golden("clip_cond_feat_" + case)
    x, ks = g["x"], int(g["kernel_size"])
    ref = C64.smooth_features(x, ks)
    e = float(np.abs(ref - g["y"].astype(np.float64)).max())
    print("%s: restatement against the reference %.3e (bound %.3e)" % (case, e, feature_tol(x, ks)))
    assert e <= feature_tol(x, ks) and abs(e - float(g["ref_err_vs_fp64"])) < 1e-12
    if ks == 1:
        assert np.array_equal(ref, x.astype(np.float64))
    if x.shape[-1] % 2 == 0:
        z = C64.smooth_features(x, ks, 2)
        assert z.shape == x.shape[:-1] + (x.shape[-1] // 2 * 3,)
        z = z.reshape(z.shape[:-1] + (-1, 3))
        assert np.array_equal(z[..., :2].reshape(ref.shape), ref) and not z[..., 2].any()


def test_python_functions_refuse_before_the_library_is_entered():
    from real3dportrait_amd import _lib, clip_conditions as CC
    x = torch.zeros(8, 136)
    with _lib.counting() as calls:
        with pytest.raises(NotImplementedError):
            CC.smooth_features_xd(torch.zeros(8, 4, 5))                              # rank 3, as the reference
        with pytest.raises(NotImplementedError):
            CC.smooth_features_xd(torch.zeros(8))
        for ks in (6, 0, -1):
            with pytest.raises(ValueError, match="odd"):
                CC.smooth_features_xd(x, ks)
        with pytest.raises(ValueError, match="below the padding"):
            CC.smooth_features_xd(torch.zeros(2, 136), 7)
        with pytest.raises(ValueError, match="below the padding"):
            CC.clip_keypoints(torch.zeros(1, 68, 2), torch.zeros(2, 68, 2), 7)
        with pytest.raises(TypeError, match="float32"):
            CC.smooth_features_xd(x.double())
        with pytest.raises(ValueError, match="not contiguous"):
            CC.smooth_features_xd(torch.zeros(136, 8).t())
        with pytest.raises(ValueError, match="GPU only"):
            CC.smooth_features_xd(x)
        with pytest.raises(ValueError, match=r"\[T, L, 2\]"):
            CC.clip_keypoints(torch.zeros(3, 68, 2), torch.zeros(8, 68, 2))          # neither T nor one source row
        with pytest.raises(ValueError, match="GPU only"):
            CC.clip_keypoints(torch.zeros(1, 68, 2), torch.zeros(8, 68, 2))
        e = torch.zeros(8, 3)
        for fn in (CC.clip_camera, CC.camera_pose_intrinsic):
            with pytest.raises(ValueError, match="GPU only"):
                fn(e, e)
            with pytest.raises(TypeError, match="float32"):
                fn(e.double(), e)
            with pytest.raises(ValueError, match="not contiguous"):
                fn(torch.zeros(3, 8).t(), e)
        with pytest.raises(ValueError, match="GPU only"):
            CC.camera_pose_intrinsic(torch.zeros(3), torch.zeros(3))                  # the one-frame form
        with pytest.raises(ValueError, match="GPU only"):
            CC.smooth_camera_sequence(torch.zeros(8, 25))
        with pytest.raises(ValueError, match="not contiguous"):
            CC.smooth_camera_sequence(torch.zeros(8, 32)[:, :25])
        with pytest.raises(TypeError, match="tensor"):
            CC.smooth_camera_sequence(np.zeros((8, 25), np.float32))                  # the reference's NumPy form is not taken
    assert calls == []


def test_patch_infer_utils_keeps_the_original():
    from real3dportrait_amd import clip_conditions as CC, patch_infer_utils
    mod = types.SimpleNamespace(smooth_features_xd=lambda t, kernel_size=7: "reference", smooth_camera_sequence="untouched")
    assert patch_infer_utils(mod) is mod and mod.smooth_features_xd is CC.smooth_features_xd
    assert mod._r3d_reference_smooth_features_xd(None) == "reference" and mod.smooth_camera_sequence == "untouched"
    assert patch_infer_utils(mod)._r3d_reference_smooth_features_xd(None) == "reference"          # patching twice keeps the first


def test_c_entry_points_reject_bad_arguments_without_a_gpu():
    from real3dportrait_amd import _lib
    lib = _lib.load()
    P = lambda k: ctypes.c_void_p(k << 32)              # never dereferenced: validation fails first
    err = lambda: lib.r3d_last_error()
    inf, nan = float("inf"), float("nan")

    def camera(euler=P(1), trans=P(2), T=9, ks=7, radius=0.0, out=P(3)):
        return lib.r3d_clip_camera(euler, trans, T, ks, radius, out, None)

    def smooth(cin=P(1), stride=25, T=9, ks=7, out=P(2)):
        return lib.r3d_camera_smooth(cin, stride, T, ks, out, None)

    def feat(x=P(1), T=9, C=136, ks=7, g=0, y=P(2)):
        return lib.r3d_smooth_features(x, T, C, ks, g, y, None)

    for call, name, ptrs in ((camera, b"clip_camera:", ("euler", "trans", "out")), (smooth, b"camera_smooth:", ("cin", "out")),
                             (feat, b"smooth_features:", ("x", "y"))):
        for k in ptrs:
            assert call(**{k: None}) == -1 and name in err() and b"NULL pointer" in err(), k
        for bad in (0, -1):
            assert call(T=bad) == -1 and name in err() and b"must be positive" in err()
        for bad in (0, -7, 256, 257):
            assert call(ks=bad) == -1 and name in err() and b"kernel_size" in err() and b"1 .. 255" in err(), bad
    assert camera(T=85899346) == -1 and b"2^31" in err()                      # 25 T = 2^31 + 2
    assert smooth(T=1 << 27, stride=16) == -1 and b"2^31" in err()
    assert feat(T=1 << 16, C=1 << 15) == -1 and b"2^31" in err()
    assert feat(T=1 << 15, C=(1 << 15) + (1 << 14), g=2) == -1 and b"2^31" in err()          # 1.5 x 2^30 values fit, with their zero columns not
    for bad in (-1.0, inf, -inf, nan):
        assert camera(radius=bad) == -1 and b"radius" in err(), bad
    for bad in (0, 12, 24, 26):
        assert smooth(stride=bad) == -1 and b"16 or 25" in err(), bad
    for bad in (0, -1):
        assert feat(C=bad) == -1 and b"C = " in err()
    for bad in (2, 6, 254):
        assert feat(ks=bad, T=200) == -1 and b"even" in err(), bad
    assert feat(T=2, ks=7) == -1 and b"below the padding" in err()
    assert feat(T=126, ks=255) == -1 and b"below the padding" in err()
    for bad in (-1, 3, 137):
        assert feat(g=bad) == -1 and b"divisor" in err(), bad
    # an output that overlaps an input, by one float at either end
    assert camera(out=P(1)) == -1 and b"overlaps" in err() and camera(out=P(2)) == -1 and b"overlaps" in err()
    assert camera(out=ctypes.c_void_p((2 << 32) + 4 * (9 * 3 - 1))) == -1 and b"overlaps" in err()
    assert camera(out=ctypes.c_void_p((1 << 32) - 4 * (9 * 25 - 1))) == -1 and b"overlaps" in err()
    assert smooth(out=P(1)) == -1 and b"overlaps" in err()
    assert smooth(out=ctypes.c_void_p((1 << 32) + 4 * (9 * 25 - 1))) == -1 and b"overlaps" in err()
    assert smooth(stride=16, out=ctypes.c_void_p((1 << 32) - 4 * (9 * 16 - 1))) == -1 and b"overlaps" in err()
    assert feat(y=P(1)) == -1 and b"overlaps" in err()
    assert feat(y=ctypes.c_void_p((1 << 32) + 4 * (9 * 136 - 1))) == -1 and b"overlaps" in err()
    assert feat(g=2, y=ctypes.c_void_p((1 << 32) - 4 * (9 * 204 - 1))) == -1 and b"overlaps" in err()
