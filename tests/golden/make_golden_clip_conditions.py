"""Regenerate the clip_cond_* golden vectors: the reference's own camera trajectory, exactly as inference/real3d_infer.py:312-319 runs it
(get_eg3d_convention_camera_pose_intrinsic of data_gen/eg3d/convert_to_eg3d_convention.py on the CPU copies of euler and trans, the
concatenation with the intrinsics, smooth_camera_sequence of inference/infer_utils.py, .float()), and its smooth_features_xd as
real3d_infer.py:452 calls it, on the CPU.

Run in the build container only (needs the reference tree and scipy):
    R3D_REFERENCE=<reference tree> python tests/golden/make_golden_clip_conditions.py
The three reference files (and utils/commons/tensor_utils.py, which the first imports) are loaded by path behind stub modules:
ref_stubs.install() plus empty librosa, deep_3drecon* and utils.commons packages.  Each file holds arrays only.
  clip_cond_cam_<case>: euler, trans [T, 3] fp32, kernel_size, camera [T, 25] (the reference's, after .float()) and ref_err_vs_fp64, the
    largest absolute distance of that output from tests/clip_conditions_ref64.py on the same inputs.  Case e also holds the unsmoothed
    c2w and convention_c2w (radius 2.7) with ref_err_unsmoothed; case f also camera16, smooth_camera_sequence on the [T, 16] form.
  clip_cond_feat_<case>: x, kernel_size, y (the reference's), ref_err_vs_fp64.
The maker asserts what keeps the reference well defined on every camera case: every window's eigen-gap (lambda1 - lambda2) / n >= 0.25
(the chordal mean is conditioned like 1 / gap), and in case g that the largest quaternion component takes all four positions."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ["R3D_REFERENCE"]          # the reference tree
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, HERE)

import clip_conditions_ref64 as C64  # noqa: E402
import ref_stubs  # noqa: E402

MAX_BYTES = 524288
MIN_GAP = 0.25


def load_reference():
    ref_stubs.install()
    for name in ("librosa", "deep_3drecon", "deep_3drecon.util", "deep_3drecon.deep_3drecon_models", "utils", "utils.commons"):
        sys.modules[name] = types.ModuleType(name)
        sys.modules[name].__path__ = []
    mats = types.ModuleType("deep_3drecon.util.load_mats")
    mats.transferBFM09 = lambda *a, **k: None
    sys.modules["deep_3drecon.util.load_mats"] = mats

    def by_path(name, rel):
        spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        return mod

    by_path("utils.commons.tensor_utils", "utils/commons/tensor_utils.py")
    by_path("deep_3drecon.deep_3drecon_models.bfm", "deep_3drecon/deep_3drecon_models/bfm.py")
    convert = by_path("r3d_reference_convert_to_eg3d_convention", "data_gen/eg3d/convert_to_eg3d_convention.py")
    infer_utils = by_path("r3d_reference_infer_utils", "inference/infer_utils.py")
    return convert.get_eg3d_convention_camera_pose_intrinsic, infer_utils.smooth_camera_sequence, infer_utils.smooth_features_xd


def camera_cases():
    """name -> (euler, trans, kernel_size)"""
    u = C64.uniform
    cases = {"a_t1_zero": (np.zeros((1, 3), np.float32), np.zeros((1, 3), np.float32), 7),
             "b_t2": (u(2, (2, 3), 1.0), u(3, (2, 3), 0.3), 7),
             "c_t3_static": (np.tile(np.float32([0.31, -0.22, 0.13]), (3, 1)), np.tile(np.float32([0.05, -0.2, 0.3]), (3, 1)), 7)}
    for ks in (7, 3, 1):
        cases["d_t9_k%d" % ks] = (u(4, (9, 3), 1.0), u(5, (9, 3), 0.3), ks)
    e = u(6, (41, 3), 1.0)
    e[[5, 17, 18, 33]] = u(8, (4, 3), 0.01)          # four frames next to the zero pose: 1 + trace < 1e-3
    cases["e_t41"] = (e, u(7, (41, 3), 0.3), 7)
    cases["f_t70_smooth"] = C64.trajectory(70) + (7,)
    base = np.float32([[0, 0, 0], [np.pi, 0, 0], [0, np.pi, 0], [0, 0, np.pi]])
    cases["g_t12_k1_axes"] = ((np.repeat(base, 3, axis=0) + u(9, (12, 3), 0.05)).astype(np.float32), u(10, (12, 3), 0.3), 1)
    return cases


def feature_cases():
    """name -> (x, kernel_size)"""
    shapes = {"a_t3": ((3, 136), 7), "b_t4": ((4, 136), 7), "c_t7_k3": ((7, 5), 3), "d_t70": ((70, 136), 7), "e_rank4": ((9, 2, 3, 5), 7),
              "f_rank5": ((8, 2, 3, 4, 5), 7), "g_k1": ((5, 136), 1)}
    return {name: (C64.uniform(20 + i, shape, 1.0), ks) for i, (name, (shape, ks)) in enumerate(shapes.items())}


def save(name, **arrays):
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **arrays)
    assert os.path.getsize(path) <= MAX_BYTES, (name, os.path.getsize(path))
    print("    %s: %d bytes" % (name, os.path.getsize(path)))


def main():
    pose_intrinsic, smooth_camera_sequence, smooth_features_xd = load_reference()
    err = lambda a, b: float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())
    for name, (euler, trans, ks) in camera_cases().items():
        T = euler.shape[0]
        ret = pose_intrinsic({"euler": torch.from_numpy(euler.copy()), "trans": torch.from_numpy(trans.copy())})
        c2w, conv, intrinsics = ret["c2w"], ret["convention_c2w"], ret["intrinsics"]
        gaps = C64.window_gaps(c2w[:, :3, :3], ks)
        assert gaps.min() >= MIN_GAP, (name, gaps.min())
        camera = np.concatenate([c2w.reshape([-1, 16]), intrinsics.reshape([-1, 9])], axis=-1)
        camera = smooth_camera_sequence(camera, kernel_size=ks)
        camera = torch.tensor(camera).float().numpy()
        ref = C64.clip_camera(euler, trans, ks)
        extra = {}
        one_plus_trace = 1.0 + np.trace(c2w[:, :3, :3], axis1=1, axis2=2)
        if name.startswith("e_"):
            assert int((one_plus_trace < 1e-3).sum()) >= 4, one_plus_trace.min()
            F = np.stack([C64.frame_cameras(euler, trans), C64.frame_cameras(euler, trans, 2.7)])
            both = np.stack([c2w, conv])
            extra = {"c2w": torch.tensor(c2w).float().numpy(), "convention_c2w": torch.tensor(conv).float().numpy(),
                     "ref_err_unsmoothed": np.float64(err(both.astype(np.float32), F))}
        if name.startswith("f_"):
            cam16 = smooth_camera_sequence(c2w.reshape([-1, 16]).copy(), kernel_size=ks)
            extra = {"camera16": torch.tensor(cam16).float().numpy()}
            assert err(extra["camera16"], camera[:, :16]) == 0.0
        if name.startswith("g_"):
            largest = {int(np.argmax(np.abs(C64.quaternion(m)))) for m in c2w[:, :3, :3]}
            assert largest == {0, 1, 2, 3}, largest
        assert camera.dtype == np.float32 and camera.shape == (T, 25) == ref.shape
        e = err(camera, ref)
        print("cam %s: T %d kernel_size %d: smallest gap %.3f, smallest 1 + trace %.2e, reference against fp64 %.3e"
              % (name, T, ks, gaps.min(), one_plus_trace.min(), e))
        save("clip_cond_cam_" + name, euler=euler, trans=trans, kernel_size=np.int64(ks), camera=camera, ref_err_vs_fp64=np.float64(e), **extra)
    for name, (x, ks) in feature_cases().items():
        with torch.no_grad():
            y = smooth_features_xd(torch.from_numpy(x.copy()), kernel_size=ks).float().contiguous().numpy()
        ref = C64.smooth_features(x, ks)
        assert y.dtype == np.float32 and y.shape == x.shape == ref.shape
        e = err(y, ref)
        print("feat %s: %s kernel_size %d: reference against fp64 %.3e, largest |x| %.3f" % (name, x.shape, ks, e, float(np.abs(x).max())))
        save("clip_cond_feat_" + name, x=x, kernel_size=np.int64(ks), y=y, ref_err_vs_fp64=np.float64(e))


if __name__ == "__main__":
    main()
