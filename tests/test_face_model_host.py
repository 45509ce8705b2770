"""CPU: the host side of the HIP face model and of get_driving_motion (real3dportrait_amd/face_model.py, driving_motion.py,
r3d_face_vertex / r3d_face_landmarks of include/r3d_hip.h).

The symbols, the argument check of the C entry points (which runs before any HIP call), the fp64 restatement (tests/face_model_ref64.py)
against the reference's own outputs (tests/golden/face_model_*.npz), the synthetic face model, the kernels' scratch use and the blink
schedule's use of the random generator."""
import ctypes
import random

import numpy as np
import pytest

from conftest import load_golden
import blink_ref as BR
import face_model_ref64 as F64
import raster_ref64 as R64
from real3dportrait_amd import synth

FIXTURES = ("face_model_a_n37_t5", "face_model_b_n625_t51", "face_model_c_lm68_t51", "face_model_d_lm68_t51_world")
FIXTURE_SEEDS = dict(zip(FIXTURES, (11, 12, 13, 14)))


def fixture_to_camera(g):
    """Only the to_camera=False fixture (the reconstruct_lm2d_nerf path) records the flag."""
    return bool(int(g.get("to_camera", 1)))


def fixture_model(g):
    """The model arrays a fixture was made on, rebuilt from its spec and checked against its checksum."""
    G, seed, N, T, Ki, Ke = (int(x) for x in g["spec"])
    m = synth.synth_face_model(G, seed, Ki, Ke)
    if "lm2d" in g:
        arrays = m["key_mean_shape"].reshape(-1), m["key_id_base"], m["key_exp_base"]
    else:
        arrays = m["mean_shape"].reshape(-1)[:3 * N], m["id_base"][:3 * N], m["exp_base"][:3 * N]
    assert abs(sum(float(a.astype(np.float64).sum()) for a in arrays) - float(g["model_sum"])) < 1e-9
    return arrays


def test_symbols_are_declared_exported_and_bound():
    from real3dportrait_amd import _lib
    import real3dportrait_amd
    lib = _lib.load()
    assert lib.r3d_version() == _lib.ABI_VERSION
    for name in ("r3d_face_vertex", "r3d_face_landmarks"):          # (header against table: tests/test_abi.py)
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert len(_lib.SIGNATURES["r3d_face_vertex"][1]) == 15 and len(_lib.SIGNATURES["r3d_face_landmarks"][1]) == 18
    from real3dportrait_amd import driving_motion, face_model
    for name in ("compute_face_vertex", "reconstruct_lm2d", "patch_face_model", "patch_face3d_helper"):
        assert getattr(real3dportrait_amd, name) is getattr(face_model, name), name
    for name in ("get_driving_motion", "patch_driving_motion"):
        assert getattr(real3dportrait_amd, name) is getattr(driving_motion, name), name


def test_c_entry_points_reject_bad_arguments_without_a_gpu():
    from real3dportrait_amd import _lib
    lib = _lib.load()
    P = lambda k: ctypes.c_void_p(k << 32)              # never dereferenced: validation fails first
    err = lambda: lib.r3d_last_error()
    inf, nan = float("inf"), float("nan")

    def vertex(mean=P(1), idb=P(2), expb=P(3), N=37, Ki=80, Ke=64, id=P(4), exp=P(5), euler=P(6), trans=P(7), T=5, dist=10.0, out=P(8)):
        return lib.r3d_face_vertex(mean, idb, expb, N, Ki, Ke, id, exp, euler, trans, T, dist, 1, out, None)

    def lm(mean=P(1), idb=P(2), expb=P(3), L=68, Ki=80, Ke=64, id=P(4), exp=P(5), euler=P(6), trans=P(7), T=5, dist=10.0, focal=1015.0,
           center=112.0, size=224.0, out=P(8)):
        return lib.r3d_face_landmarks(mean, idb, expb, L, Ki, Ke, id, exp, euler, trans, T, dist, 1, focal, center, size, out, None)

    for call, count in ((vertex, "N"), (lm, "L")):
        for k in ("mean", "idb", "id", "out"):
            assert call(**{k: None}) == -1 and b"NULL pointer" in err(), k
        assert call(expb=None) == -1 and b"exp_base is NULL" in err()
        for bad in (0, -1):
            assert call(**{count: bad}) == -1 and b"must be positive" in err()
            assert call(T=bad) == -1 and b"must be positive" in err()
        for Ki, Ke in ((0, 64), (-1, 64), (80, -1), (449, 64), (512, 1), (1 << 30, 1 << 30)):
            assert call(Ki=Ki, Ke=Ke) == -1 and b"Ki + Ke <= 512" in err(), (Ki, Ke)
        assert call(**{count: 1 << 20}, T=1 << 10) == -1 and b"2^31" in err()          # 3 x 2^30
        assert call(**{count: 715827883}, T=1) == -1 and b"2^31" in err()              # 3 N = 2^31 + 1
        for bad in (inf, -inf, nan):
            assert call(dist=bad) == -1 and b"camera_distance" in err(), bad
        # an output that overlaps an input: mean, a base, the coefficients, the pose
        for k in ("mean", "idb", "expb", "id", "exp", "euler", "trans"):
            assert call(**{k: P(8)}) == -1 and b"overlaps" in err(), k
        assert call(out=ctypes.c_void_p((1 << 32) + 4)) == -1 and b"overlaps" in err()
    for k in ("focal", "center", "size"):
        for bad in (inf, nan):
            assert lm(**{k: bad}) == -1 and b"not finite" in err(), (k, bad)
    for k in ("focal", "size"):
        for bad in (0.0, -1.0):
            assert lm(**{k: bad}) == -1 and b"must be positive" in err(), (k, bad)


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_agrees_with_the_reference_fixtures(name):
    """fp64 restatement against the reference's recorded fp32 outputs: within ref_err_vs_fp64 (the figure the fixture was made with), and
    that figure is what fp32 can give at these magnitudes."""
    g = load_golden(name)
    mean, idb, expb = fixture_model(g)
    if "lm2d" in g:
        ref, rec = F64.landmarks(mean, idb, expb, g["id"], g["exp"], g["euler"], g["trans"], to_camera=fixture_to_camera(g)), g["lm2d"]
        assert rec.shape == (51, 68, 2)
    else:
        ref, rec = F64.face_vertex(mean, idb, expb, g["id"], g["exp"], g["euler"], g["trans"]), g["vertex"]
        assert rec.shape == (int(g["spec"][3]), int(g["spec"][2]), 3)
    e = float(np.abs(rec.astype(np.float64) - ref).max())
    print("%s: reference fp32 against the fp64 restatement %.3e (recorded %.3e), largest |value| %.2f" % (name, e, float(g["ref_err_vs_fp64"]),
                                                                                                        float(np.abs(ref).max())))
    assert rec.dtype == np.float32 and e <= float(g["ref_err_vs_fp64"]) * (1 + 1e-12)
    assert 1e-8 < float(g["ref_err_vs_fp64"]) < 2e-6          # a few ulp at |v| <= 12; a restatement of another rule would be off by far more
    # the inputs are the hash's: poses ~ N(0, 0.3^2) rad, translations ~ N(0, 0.2^2); without to_camera the model's own z (0 .. 0.9) is
    # the depth, and the translations are moved 6 along z, off the projection's pole
    idc, expc, euler, trans = F64.coefficients(FIXTURE_SEEDS[name], int(g["spec"][3]))
    if not fixture_to_camera(g):
        trans[:, 2] += np.float32(6.0)
        assert name.endswith("_world") and float(np.abs(ref).max()) > 1.5
    assert all(np.array_equal(a, b) for a, b in ((idc, g["id"]), (expc, g["exp"]), (euler, g["euler"]), (trans, g["trans"])))


def test_restatement_by_hand():
    """One vertex, identity 2 columns, a quarter turn about z: Rz maps (1, 0, 0) to (0, 1, 0); p @ (Rz)^T = Rz p."""
    mean = np.array([1.0, 0.0, 0.5])
    idb = np.array([[1.0, 0.0], [0.0, 2.0], [0.0, 0.0]])
    v = F64.face_vertex(mean, idb, np.zeros((3, 0)), np.array([[1.0, 0.5]]), None, np.array([[0.0, 0.0, np.pi / 2]]), np.array([[0.1, 0.2, 0.3]]))
    # p = (2, 1, 0.5); Rz p = (-1, 2, 0.5); + trans = (-0.9, 2.2, 0.8); z = 10 - 0.8
    assert np.allclose(v[0, 0], [-0.9, 2.2, 9.2], rtol=0, atol=1e-12)
    lm = F64.landmarks(mean, idb, np.zeros((3, 0)), np.array([[1.0, 0.5]]), None, np.array([[0.0, 0.0, np.pi / 2]]), np.array([[0.1, 0.2, 0.3]]))
    x, y = (1015 * -0.9 + 112 * 9.2) / 9.2, (1015 * 2.2 + 112 * 9.2) / 9.2
    assert np.allclose(lm[0, 0], [x / 224, (224 - y) / 224], rtol=0, atol=1e-12)
    # Rx and Ry by their action on the axes: Rx(90) y -> z, Ry(90) z -> x
    r = F64.rotation(np.array([[np.pi / 2, 0, 0], [0, np.pi / 2, 0]]))
    assert np.allclose(np.array([0.0, 1.0, 0.0]) @ r[0], [0, 0, 1], atol=1e-12) and np.allclose(np.array([0.0, 0.0, 1.0]) @ r[1], [1, 0, 0], atol=1e-12)


def test_synth_face_model():
    m = synth.synth_face_model(24, 0)
    n = 25 * 25
    assert m["mean_shape"].shape == (3 * n, 1) and m["id_base"].shape == (3 * n, 80) and m["exp_base"].shape == (3 * n, 64)
    assert m["feat"].shape == (n, 3) and m["feat"].min() >= 0.02 and m["feat"].max() <= 1.0
    assert m["keypoints"].shape == (68,) and m["keypoints"].min() >= 0 and m["keypoints"].max() < n and len(set(m["keypoints"].tolist())) == 68
    assert m["key_mean_shape"].shape == (68, 3) and m["key_id_base"].shape == (204, 80) and m["key_exp_base"].shape == (204, 64)
    assert np.array_equal(m["key_id_base"][3 * 5 + 1], m["id_base"][3 * m["keypoints"][5] + 1])
    assert all(m[k].dtype == np.float32 for k in ("mean_shape", "id_base", "exp_base", "feat", "key_mean_shape", "key_id_base", "key_exp_base"))
    assert m["tri"].dtype == np.int64 and m["tri"].min() == 0 and m["tri"].max() == n - 1 and not m["tri"][0].any()
    assert 2 * 24 * 24 - 40 < len(m["tri"]) < 2 * 24 * 24 - 4                     # the eye triangles are gone
    assert float(np.abs(m["id_base"]).max()) <= 0.004 and float(np.abs(m["exp_base"]).max()) <= 0.004
    assert synth.synth_face_model(188, 0, 4, 0)["mean_shape"].shape[0] == 3 * 35721 and synth.synth_face_model(6, 0, 7, 0)["exp_base"].shape == (147, 0)
    for k in ("mean_shape", "id_base", "tri", "keypoints"):
        assert np.array_equal(m[k], synth.synth_face_model(24, 0)[k])
    assert not np.array_equal(m["id_base"], synth.synth_face_model(24, 1)["id_base"])


@pytest.mark.parametrize("S,G", [(64, 24), (96, 40)])
def test_synth_face_model_renders_maps_the_blink_accepts_and_fp32_vertices_suffice(S, G):
    """Rendered through the fp64 rasteriser the model has two eye holes which the blink rule accepts (status 0); no triangle flips under
    unit-variance coefficients; and the reference's fp32 torch vertices rasterise to the same pix_to_face as fp64 vertices within the
    project's cap of S^2 / 1000 pixels (measured: 0 at both sizes)."""
    import torch
    m = synth.synth_face_model(G, 0)
    T = 3
    idc, expc, _, _ = F64.coefficients(5, T)
    v64 = F64.face_vertex(m["mean_shape"], m["id_base"], m["exp_base"], idc, expc)
    t = torch.from_numpy
    shape = (torch.einsum("ij,aj->ai", t(m["id_base"]), t(idc)) + torch.einsum("ij,aj->ai", t(m["exp_base"]), t(expc))
             + t(m["mean_shape"]).reshape(1, -1)).reshape(T, -1, 3)          # bfm.py:112-115 at zero pose
    shape[..., -1] = 10.0 - shape[..., -1]
    v32 = shape.numpy()
    assert float(np.abs(v32 - v64).max()) < 5e-6
    tri = m["tri"][1:]
    a, b, c = (v64[:, tri[:, k], :2] for k in range(3))
    area = (b[..., 0] - a[..., 0]) * (c[..., 1] - a[..., 1]) - (b[..., 1] - a[..., 1]) * (c[..., 0] - a[..., 0])
    assert (np.sign(area) == np.sign(area[0, 0])).all()                    # one winding: nothing flipped
    feat = np.broadcast_to(m["feat"], (T,) + m["feat"].shape)
    r64 = R64.rasterize(v64, m["tri"], feat, S, synth.BFM_FOV_DEG, 5.0)
    r32 = R64.rasterize(v32, m["tri"], feat, S, synth.BFM_FOV_DEG, 5.0)
    c = R64.compare(r32, r64)
    print("S %d G %d: fp32 vertices against fp64 vertices: %d differing pixels of %d" % (S, G, c["differing"], c["pixels"]))
    assert c["differing"] <= (S * S) // 1000
    assert (r64["pix_to_face"] != 0).all() and 0.9 < (r64["pix_to_face"] > 0).mean() < 0.97          # face 0 covers nothing
    maps = (2.0 * r64["image"] - 1.0).astype(np.float32)
    for f in range(T):
        res = BR.blink(maps[f], 0.64)
        L, R = BR.regions(S, S)
        assert res["status"] == 0 and (res["E"] & L).sum() >= 8 and (res["E"] & R).sum() >= 8 and res["B"].sum() > res["E"].sum(), f


def test_face_model_kernels_do_not_use_scratch():
    from test_render_kernel_resources import _kernel_metadata
    from real3dportrait_amd import _lib
    meta = _kernel_metadata(_lib.LIB_PATH)
    names = sorted(k for k in meta if "4face10face_model" in k)
    assert len(names) == 2, names
    # test_raster_host.py also asks for sgpr_spill_count == 0.  Not here: the coefficient pointers of 8 frames overflow the SGPR file, and the
    # compiler parks them in VGPR lanes (v_writelane, 53 / 77 of them).  That is registers, not memory: scratch use is the
    # private segment, which is zero, as is the count of VGPRs spilled to it.
    for k in names:
        print(k, "vgpr", meta[k]["vgpr_count"], "sgpr spills to VGPR lanes", meta[k]["sgpr_spill_count"])
        assert int(meta[k]["private_segment_fixed_size"]) == 0, (k, meta[k])
        assert int(meta[k]["vgpr_spill_count"]) == 0, (k, meta[k])


@pytest.mark.parametrize("T,period", [(131, 125), (10, 125), (1, 125), (300, 25), (126, 125)])
def test_blink_schedule_consumes_the_generator_as_the_reference_loop(T, period):
    """What get_driving_motion passes on: blink_schedule against the transcription of real3d_infer.py:411-426, the generator left in the
    same state."""
    from real3dportrait_amd import edit_secc
    a, b = random.Random(7), random.Random(7)
    edits = edit_secc.blink_schedule(T, period, a)
    want = []
    for i in range(T):
        if i % period == 0:
            dur = b.randint(8, 12)
            for offset in range(dur):
                j = offset + i
                if j >= T - 1:
                    break
                want.append((j, -4 / dur ** 2 * offset ** 2 + 4 / dur * offset))
    assert edits == want and a.getstate() == b.getstate()
    assert all(j < T - 1 for j, _ in edits)                    # the clip's last frame is never edited


def test_python_wrappers_refuse_malformed_input_before_the_library():
    import torch
    from real3dportrait_amd import compute_face_vertex, get_driving_motion

    class M:
        pass
    m = M()
    s = synth.synth_face_model(4, 0, 7, 5)
    m.mean_shape, m.id_base, m.exp_base, m.camera_distance = s["mean_shape"], s["id_base"], s["exp_base"], 10.0
    with pytest.raises(ValueError, match="GPU only"):
        compute_face_vertex(m, torch.zeros(2, 7), torch.zeros(2, 5), torch.zeros(2, 3), torch.zeros(2, 3))
    with pytest.raises(ValueError, match="on the GPU"):
        get_driving_motion(None, None, torch.zeros(2, 7), torch.zeros(2, 5), torch.zeros(2, 3), torch.zeros(2, 3))


# ---- the launch plan (face::plan of csrc/r3d_face_model.hip through the host-only hook r3d_debug_face_plan) ----
PLAN_NS = (1, 5, 37, 68, 468, 625, 35709)
PLAN_KS = (1, 3, 50, 51, 100, 144, 511, 512)
PLAN_TS = (1, 7, 8, 9, 16, 17, 51, 500, 2000, 70000)
FACE_PLAN = ("V", "xblocks", "chunk", "yblocks", "lds_bytes")
# the shapes tests/test_gpu_face_model.py runs for their plan: (N, Ki, Ke, T) -> (chunk, yblocks, frames of the last chunk)
GPU_PLAN_CASES = {(625, 448, 64, 100): (16, 7, 4), (625, 448, 64, 93): (16, 6, 13), (2200, 80, 64, 77): (16, 5, 13), (625, 80, 64, 300): (16, 19, 12)}


def face_plan(N, Ki, Ke, T):
    """-> (status, {V, xblocks, chunk, yblocks, lds_bytes}) of r3d_debug_face_plan; no HIP call is made."""
    from real3dportrait_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "r3d_debug_face_plan"), "%s does not export the plan hook: rebuild it" % _lib.LIB_PATH
    out = (ctypes.c_int32 * 5)(*[-1] * 5)
    rc = lib.r3d_debug_face_plan(N, Ki, Ke, T, out)
    return rc, dict(zip(FACE_PLAN, out))


def test_plan_invariants_over_the_sweep():
    """Every (N, K, T) of the sweep: what the kernel relies on (V vertices fit a block's threads and LDS, the chunks tile T with none
    empty, whole groups of 8 frames per chunk unless one block walks all of T, grid.y within HIP's limit), and the sizes the entry points
    refuse (3 N T >= 2^31) are refused by the hook with the same status and reason."""
    from real3dportrait_amd import _lib
    lib = _lib.load()
    P = lambda k: ctypes.c_void_p(k << 40)              # never dereferenced: the refusal comes first
    refused = 0
    for N in PLAN_NS:
        for K in PLAN_KS:
            Ke = K // 3
            Ki = K - Ke
            for T in PLAN_TS:
                rc, p = face_plan(N, Ki, Ke, T)
                if 3 * N * T >= 1 << 31:
                    assert rc == -1 and b"debug_face_plan" in lib.r3d_last_error() and b"2^31" in lib.r3d_last_error(), (N, K, T)
                    assert lib.r3d_face_vertex(P(1), P(2), P(3), N, Ki, Ke, P(4), P(5), P(6), P(7), T, 10.0, 1, P(8), None) == rc
                    assert b"face_vertex" in lib.r3d_last_error() and b"2^31" in lib.r3d_last_error()
                    refused += 1
                    continue
                assert rc == 0, (N, K, T, lib.r3d_last_error())
                V, xb, chunk, yb, lds = (p[k] for k in FACE_PLAN)
                assert 1 <= V <= min(N, 128 // 3) and 3 * V * K <= 15000, (N, K, T, p)
                assert V * (xb - 1) < N <= V * xb, (N, K, T, p)
                assert lds == (3 * V * K + 8 * 128 + 8 * 12) * 4 and lds <= 65536, (N, K, T, p)
                assert 1 <= chunk and chunk * (yb - 1) < T <= chunk * yb, (N, K, T, p)
                assert 1 <= yb <= 65535 and 1 <= xb <= 2 ** 31 - 1, (N, K, T, p)
                assert chunk % 8 == 0 or chunk == T, (N, K, T, p)
    assert refused == len(PLAN_KS)          # N = 35 709 at T = 70 000 alone
    out = (ctypes.c_int32 * 5)()
    for bad in ((0, 80, 64, 5), (37, 0, 64, 5), (37, 80, -1, 5), (37, 449, 64, 5), (37, 80, 64, 0)):
        assert lib.r3d_debug_face_plan(*bad, out) == -1 and b"debug_face_plan" in lib.r3d_last_error(), bad
    assert lib.r3d_debug_face_plan(37, 80, 64, 5, None) == -1 and b"NULL" in lib.r3d_last_error()


def test_plan_values_are_pinned():
    """The regimes by number.  The product's mesh (N = 35 709, K = 80 + 64, T = 250): 1051 vertex tiles fill the chip, so the frames are
    not split and ONE block walks all 250, 31 groups of 8 then 2.  The suite's older shapes: at most one group of 8 per block.  The shapes
    of test_gpu_face_model.py's long-walk cases: chunks of 16, two groups of 8 per block, and the tails named there.  A change to a plan
    constant has to come through here."""
    assert face_plan(35709, 80, 64, 250) == (0, dict(V=34, xblocks=1051, chunk=250, yblocks=1, lds_bytes=(144 * 102 + 1024 + 96) * 4))
    assert face_plan(68, 80, 64, 250)[1] == dict(V=34, xblocks=2, chunk=8, yblocks=32, lds_bytes=63232)          # landmarks: frames split
    for N in (1, 37, 625):
        for Ki, Ke in ((80, 64), (7, 5), (80, 0)):
            for T in (1, 3, 5, 50, 51):
                p = face_plan(N, Ki, Ke, T)[1]
                assert p["chunk"] == min(T, 8), (N, Ki, Ke, T, p)
    for (N, Ki, Ke, T), (chunk, yblocks, last) in GPU_PLAN_CASES.items():
        p = face_plan(N, Ki, Ke, T)[1]
        assert (p["chunk"], p["yblocks"], T - chunk * (yblocks - 1)) == (chunk, yblocks, last), (N, Ki, Ke, T, p)
    assert face_plan(625, 448, 64, 100)[1]["V"] == 9 and face_plan(2200, 80, 64, 77)[1]["xblocks"] == 65


def test_the_mean_is_added_last_because_a_chain_begun_at_it_misses_the_bound():
    """Why the kernel's rule is `chain from 0, then + mean`, without a GPU: face_model_ref64.kernel_fp32 restates the kernel's fp32
    operations in either order, on the inputs of test_gpu_face_model.py's long-walk cases.  Begun at the mean (of size 1) every one of
    the K small terms is rounded at the mean's ulp: 2.907e-06 for vertices at K = 512 and 7.996e-07 for 2200 landmarks, over the bounds
    the GPU tests hold (4 x the reference's own fp32 error on its fixture), and what the kernel measured while it summed that way.  With
    the mean last: 6.2e-07 and 2.5e-07, what NumPy's fp32 evaluation of the reference's own expression gives."""
    vert_tol = 4.0 * float(load_golden("face_model_b_n625_t51")["ref_err_vs_fp64"])
    lm_tol = 4.0 * float(load_golden("face_model_c_lm68_t51")["ref_err_vs_fp64"])
    N, Ki, Ke, T = 625, 448, 64, 100
    m = synth.synth_face_model(24, 0, Ki, Ke)
    host = m["mean_shape"].reshape(-1), m["id_base"], m["exp_base"]
    coef = F64.coefficients(300 + N + T, T, Ki, Ke)
    ref = F64.face_vertex(*host, *coef)
    err = {first: float(np.abs(F64.kernel_fp32(*host, *coef, mean_first=first) - ref).max()) for first in (True, False)}
    own = float(np.abs(F64.face_vertex(*host, *coef, dtype=np.float32) - ref).max())
    print("vertices N %d T %d K %d+%d: chain begun at the mean %.3e, mean last %.3e, the reference's expression in fp32 %.3e (bound %.3e)"
          % (N, T, Ki, Ke, err[True], err[False], own, vert_tol))
    assert err[False] <= vert_tol / 2 < vert_tol < err[True] and err[False] <= 1.1 * own
    L, T = 2200, 77
    m = synth.synth_face_model(46, 0)
    host = m["mean_shape"].reshape(-1)[:3 * L], m["id_base"][:3 * L], m["exp_base"][:3 * L]
    coef = F64.coefficients(200 + L + T, T)
    ref = F64.landmarks(*host, *coef)
    err = {first: float(np.abs(F64.kernel_fp32(*host, *coef, mean_first=first, landmarks=True) - ref).max()) for first in (True, False)}
    print("landmarks L %d T %d: chain begun at the mean %.3e, mean last %.3e (bound %.3e)" % (L, T, err[True], err[False], lm_tol))
    assert err[False] <= lm_tol / 2 < lm_tol < err[True]
