"""Regenerate the face_model_* golden vectors: the reference's own ParametricFaceModel.compute_face_vertex
(deep_3drecon/deep_3drecon_models/bfm.py:332-347) and Face3DHelper.reconstruct_lm2d (data_util/face3d_helper.py:132-169) on the CPU, in
fp32 as the reference runs them, on the synthetic model of real3dportrait_amd.synth.synth_face_model (BFM data does not exist here).

Run in the build container only (needs the reference tree):
    R3D_REFERENCE=<reference tree> python tests/golden/make_golden_face_model.py
The two reference files are loaded by path behind stub package entries (the packages' own __init__ pull in kornia and pytorch3d); the
objects are made without their constructors, which read BFM files, and given the synthetic arrays.  Each file holds arrays only:
spec (G, seed, N, T, Ki, Ke) -- the model is synth_face_model(G, seed, Ki, Ke) cut to its first N vertices, model_sum its fp64 checksum --
the coefficients id, exp, euler, trans, the reference's fp32 output (vertex [T, N, 3] or lm2d [T, 68, 2]) and ref_err_vs_fp64, the largest
absolute distance of that output from tests/face_model_ref64.py on the same inputs.  face_model_d_lm68_t51_world is the to_camera=False path,
which reconstruct_lm2d_nerf takes (face3d_helper.py:126-130): the model's own z is the depth there, so its translations are moved 6 along z,
off the projection's pole; it holds to_camera = 0, and its values reach 1.7 where the others stay below 1.3.
torch's CPU matmul sums in an order that depends on its thread count, so a regenerated output can differ from the committed one in the last
bit and ref_err_vs_fp64 by about a tenth; the inputs and the model are the hash's and do not."""
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

from real3dportrait_amd import synth  # noqa: E402
import face_model_ref64 as F64  # noqa: E402

# name -> (kind, G, seed, N, T, coefficient seed, to_camera)
CASES = {"face_model_a_n37_t5": ("vertex", 24, 0, 37, 5, 11, True),
         "face_model_b_n625_t51": ("vertex", 24, 0, 625, 51, 12, True),
         "face_model_c_lm68_t51": ("lm2d", 24, 0, 68, 51, 13, True),
         "face_model_d_lm68_t51_world": ("lm2d", 24, 0, 68, 51, 14, False)}
WORLD_DEPTH = 6.0          # added to trans z where to_camera is off
KI, KE = 80, 64
MAX_BYTES = 524288


def load_reference():
    """bfm.py and face3d_helper.py by file path; deep_3drecon and its sub-packages are empty stubs in sys.modules."""
    for name in ("deep_3drecon", "deep_3drecon.util", "deep_3drecon.deep_3drecon_models"):
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

    bfm = by_path("deep_3drecon.deep_3drecon_models.bfm", "deep_3drecon/deep_3drecon_models/bfm.py")
    helper = by_path("r3d_reference_face3d_helper", "data_util/face3d_helper.py")
    return bfm.ParametricFaceModel, helper.Face3DHelper


def model_arrays(G, seed, N, kind):
    m = synth.synth_face_model(G, seed, KI, KE)
    if kind == "lm2d":
        return m["key_mean_shape"].reshape(-1), m["key_id_base"], m["key_exp_base"]
    return m["mean_shape"].reshape(-1)[:3 * N], m["id_base"][:3 * N], m["exp_base"][:3 * N]


def main():
    FaceModel, Helper = load_reference()
    for name, (kind, G, seed, N, T, cseed, to_camera) in CASES.items():
        mean, idb, expb = model_arrays(G, seed, N, kind)
        idc, expc, euler, trans = F64.coefficients(cseed, T, KI, KE)
        if not to_camera:
            trans[:, 2] += np.float32(WORLD_DEPTH)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
        with torch.no_grad():
            if kind == "vertex":
                fm = object.__new__(FaceModel)
                fm.mean_shape, fm.id_base, fm.exp_base = mean.reshape(-1, 1).copy(), idb.copy(), expb.copy()
                fm.camera_distance, fm.device, fm.initialized = 10.0, "cpu", False
                out = fm.compute_face_vertex(t(idc), t(expc), t(euler), t(trans)).numpy()
                ref = F64.face_vertex(mean, idb, expb, idc, expc, euler, trans)
            else:
                h = object.__new__(Helper)
                torch.nn.Module.__init__(h)
                h.register_buffer("key_mean_shape", t(mean.reshape(-1, 3)))
                h.register_buffer("key_id_base", t(idb))
                h.register_buffer("key_exp_base", t(expb))
                h.register_buffer("persc_proj", torch.tensor(sys.modules["deep_3drecon.deep_3drecon_models.bfm"].perspective_projection(focal=1015, center=112)))
                out = h.reconstruct_lm2d(t(idc), t(expc), t(euler), t(trans), to_camera=to_camera).numpy()
                ref = F64.landmarks(mean, idb, expb, idc, expc, euler, trans, to_camera=to_camera)
        assert out.dtype == np.float32 and out.shape == ref.shape, (name, out.dtype, out.shape)
        err = float(np.abs(out.astype(np.float64) - ref).max())
        print("%s: reference fp32 against fp64 %.3e, largest |value| %.3f" % (name, err, float(np.abs(ref).max())))
        path = os.path.join(HERE, name + ".npz")
        model_sum = float(mean.astype(np.float64).sum() + idb.astype(np.float64).sum() + expb.astype(np.float64).sum())
        extra = {} if to_camera else {"to_camera": np.int64(0)}
        np.savez_compressed(path, spec=np.array([G, seed, N, T, KI, KE], np.int64), model_sum=np.float64(model_sum), id=idc, exp=expc,
                            euler=euler, trans=trans, ref_err_vs_fp64=np.float64(err), **{kind: out}, **extra)
        assert os.path.getsize(path) <= MAX_BYTES, (name, os.path.getsize(path))
        print(name, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
