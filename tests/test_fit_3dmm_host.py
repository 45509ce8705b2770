"""CPU: the host side of the landmark-driven 3DMM fit (real3dportrait_amd/fit_3dmm.py, include/r3d_hip_fit.h): the binding
table against the header, what the two entry points refuse before any launch, the restatement tests/fit_3dmm_ref.py against the goldens
(the reference's own two functions), the landmark weights against the reference's index lists, and the dead fine stage."""
import ctypes

import numpy as np
import pytest
import torch

import abi
import fit_3dmm_ref as R
from conftest import load_golden
from real3dportrait_amd import _lib, synth
from real3dportrait_amd import fit_3dmm as f3

GOLDENS = ("fit_3dmm_image_t1", "fit_3dmm_video_global_t7", "fit_3dmm_video_global_t53", "fit_3dmm_video_fine_t7")


def test_header_mirrors_the_fit_table():
    """The four entry points live in the companion header include/r3d_hip_fit.h (tests/test_abi.py compares every declaration with the
    binding table and with what load() bound, and the header's macros with the package's constants); here what is this unit's own: the
    names, the parameter counts, the ABI number, the loss record against the module's names for it, and `lambdas`, the one host array."""
    lib = _lib.load()
    assert lib.r3d_version() == _lib.ABI_VERSION
    decls = abi.header_declarations("r3d_hip_fit.h")
    assert {name: len(types) for name, (ret, types) in decls.items()} == {"r3d_fit_workspace_bytes": 4, "r3d_fit_state_bytes": 4,
                                                                          "r3d_fit_landmark_grad": 26, "r3d_fit_landmark_run": 24}
    assert set(decls) <= set(_lib.SIGNATURES)
    assert len(f3.LOSS_NAMES) == _lib.FIT_LOSS_WORDS == 8 and _lib.FIT_LAUNCHES == 2
    for name in ("r3d_fit_landmark_grad", "r3d_fit_landmark_run"):
        assert decls[name][1][13] == "float*" and _lib.SIGNATURES[name][1][13] is ctypes.POINTER(ctypes.c_float), name          # lambdas


def test_sizes():
    lib = _lib.load()
    P = 80 + 53 * 70
    assert lib.r3d_fit_state_bytes(80, 64, 53, 1) == (3 * P + 8) * 4
    assert lib.r3d_fit_state_bytes(80, 64, 53, 53) == (3 * 53 * 150 + 8) * 4
    assert lib.r3d_fit_state_bytes(3, 0, 2, 1) == (3 * (3 + 12) + 8) * 4
    assert lib.r3d_fit_state_bytes(80, 64, 53, 2) == 0 and lib.r3d_fit_state_bytes(0, 64, 53, 1) == 0
    ws = lib.r3d_fit_workspace_bytes(468, 80, 64, 53)
    assert ws % 16 == 0 and ws >= (53 * 151 + 53 * 150) * 4          # at least one slab's partial rows and the snapshot
    assert lib.r3d_fit_workspace_bytes(468, 80, 64, 106) > ws and lib.r3d_fit_workspace_bytes(936, 80, 64, 53) > ws          # the slab count follows from L
    for bad in ((0, 80, 64, 1), (468, 0, 64, 1), (468, 80, -1, 1), (468, 400, 113, 1), (468, 80, 64, 0)):
        assert lib.r3d_fit_workspace_bytes(*bad) == 0, bad


def test_argument_errors_are_refused_before_any_launch():
    """Every refusal by name.  Every call has exactly one defect; the device pointers are fake, 1 TiB apart and never dereferenced (a
    valid call would launch: tests/test_gpu_fit_3dmm.py runs those).  lambdas is a real host array."""
    lib = _lib.load()
    MEAN, IDB, EXPB, LMS, W, ID, EXP, EU, TR, GID, GEXP, GEU, GTR, LOSS, WS, STATE = (i << 40 for i in range(1, 17))
    lam = (ctypes.c_float * 6)(0.2, 0.6, 1.0, 1.0, 0.3, 0.3)
    BIG = 1 << 39
    common = dict(mean=MEAN, idb=IDB, expb=EXPB, L=468, Ki=80, Ke=64, lms=LMS, w=W, T=7, id_rows=1, cd=10.0, focal=1015.0, center=112.0, lam=lam)
    grad = dict(common, id=ID, exp=EXP, euler=EU, trans=TR, gid=GID, gexp=GEXP, geu=GEU, gtr=GTR, loss=LOSS, ws=WS, wsb=BIG)
    run = dict(common, lr0=0.1, lr1=0.1, s0=0, s1=200, n=200, groups=3, state=STATE, ws=WS, wsb=BIG)

    refused = abi.refusals(lib, "r3d_fit_landmark_")
    for fn, base in (("grad", grad), ("run", run)):
        for p in ("mean", "idb", "lms", "w", "lam"):
            refused(fn, base, b"NULL pointer", **{p: None})
        refused(fn, base, b"key_exp_base is NULL", expb=None)
        refused(fn, base, b"must be positive", L=0)
        refused(fn, base, b"must be positive", T=0, id_rows=1)
        refused(fn, base, b"need Ki >= 1", Ki=0)
        refused(fn, base, b"need Ki >= 1", Ke=-1)
        refused(fn, base, b"Ki + Ke <= 512", Ki=449)
        refused(fn, base, b"id_rows = 2 is neither 1 nor T", id_rows=2)
        refused(fn, base, b"id_rows = 0 is neither 1 nor T", id_rows=0)
        for p in ("cd", "focal", "center"):
            refused(fn, base, b"is not finite", **{p: float("nan")})
            refused(fn, base, b"is not finite", **{p: float("inf")})
        refused(fn, base, b"focal = 0 must be positive", focal=0.0)
        refused(fn, base, b"focal = -1 must be positive", focal=-1.0)
        bad = (ctypes.c_float * 6)(0.2, 0.6, float("nan"), 1.0, 0.3, 0.3)
        refused(fn, base, b"lambdas[2] is not finite", lam=bad)
        refused(fn, base, b"2^31", L=1 << 20, T=1 << 12, id_rows=1)
        refused(fn, base, b"NULL workspace", rc=-2, ws=None)
        refused(fn, base, b"are needed (r3d_fit_workspace_bytes)", rc=-2, wsb=lib.r3d_fit_workspace_bytes(468, 80, 64, 7) - 1)
        refused(fn, base, b"not 16-byte aligned", rc=-2, ws=WS + 8)
        refused(fn, base, b"overlaps", ws=LMS)
    for p in ("id", "euler", "trans", "gid", "geu", "gtr", "loss"):
        refused("grad", grad, b"NULL pointer", **{p: None})
    refused("grad", grad, b"exp and grad_exp are required", exp=None)
    refused("grad", grad, b"exp and grad_exp are required", gexp=None)
    refused("grad", grad, b"overlaps", gid=ID)
    refused("grad", grad, b"overlaps", gexp=EXP + 4)
    refused("grad", grad, b"overlaps", geu=GTR)
    refused("grad", grad, b"overlaps", loss=IDB + 8)
    refused("run", run, b"NULL pointer (state)", state=None)
    refused("run", run, b"must be positive and finite", lr0=0.0)
    refused("run", run, b"must be positive and finite", lr1=-0.1)
    refused("run", run, b"must be positive and finite", lr0=float("nan"))
    refused("run", run, b"must be positive and finite", lr1=float("inf"))
    refused("run", run, b"must not be negative", s0=-1)
    refused("run", run, b"must not be negative", s1=-1)
    refused("run", run, b"n_iter = 0 must be positive", n=0)
    refused("run", run, b"groups = 0 is outside 1 .. 3", groups=0)
    refused("run", run, b"groups = 4 is outside 1 .. 3", groups=4)
    refused("run", run, b"overlaps", state=MEAN)
    refused("run", run, b"overlaps", state=LMS + 4 * 100)
    refused("run", run, b"overlaps", state=WS + 16)
    # the typed call path raises what the library refuses
    with pytest.raises(RuntimeError, match="fit_landmark_run: groups = 7"):
        _lib.call("r3d_fit_landmark_run", *dict(run, groups=7).values(), None)


def _golden_arrays(g):
    G, mseed, kseed, L = (int(x) for x in g["spec"][:4])
    k = synth.synth_face_keys(synth.synth_face_model(G, mseed), L, kseed)
    arrays = (k["key_mean_shape"].reshape(-1), k["key_id_base"], k["key_exp_base"])
    assert abs(float(sum(a.astype(np.float64).sum() for a in arrays)) - float(g["model_sum"])) < 1e-6
    return arrays


@pytest.mark.parametrize("name", GOLDENS)
def test_restatement_reproduces_the_goldens(name):
    """The fp32 restatement lands on the reference's own coeff_dict (own_*: fit_3dmm_for_a_image / _video themselves, run by the
    generator) and on its own recorded stages, to a few fp32 roundings of the trajectory (torch's CPU matmul sums in an order that
    depends on the thread count): 20 x the recorded fp32-against-fp64 distance.  The fp64 run is recorded, not rerun: T = 1 reruns it."""
    g = load_golden(name)
    T, id_rows, img = int(g["spec"][4]), int(g["spec"][5]), int(g["spec"][7])
    arrays = _golden_arrays(g)
    lms = R.preprocess(g["lms_px"], img)
    assert lms.shape == (T, 468, 2) and lms.dtype == np.float32
    out = R.fit(arrays, lms, g["weights"], id_rows, g["lambdas"], dtype=torch.float32)
    for i, n in enumerate(R.NAMES):
        bound = 20 * max(float(g["ref_err_vs_fp64"][i]), 1e-7)
        assert np.abs(out["stage2"][n] - g["own_" + n]).max() <= bound, n
        assert np.abs(out["stage2"][n] - g["s2_" + n]).max() <= bound and np.abs(out["stage1"][n] - g["s1_" + n]).max() <= bound, n
        assert np.abs(out["stage2"][n] - g["s2_%s_f64" % n]).max() <= 2e-4 * np.abs(g["s2_%s_f64" % n]).max(), n
        assert g["own_" + n].shape == ((id_rows if n == "id" else T), {"id": 80, "exp": 64}.get(n, 3)) and g["own_" + n].dtype == np.float32
    assert not out["stage1"]["id"].any() and not out["stage1"]["exp"].any() and out["stage1"]["euler"].any()
    assert np.abs(g["s2_id_f64"]).max() > 0.3 and np.abs(g["s2_exp_f64"]).max() > 0.3          # stage 2 moved both
    if T == 1:
        o64 = R.fit(arrays, lms, g["weights"], id_rows, g["lambdas"], dtype=torch.float64)
        for n in R.NAMES:
            assert np.abs(o64["stage2"][n] - g["s2_%s_f64" % n]).max() <= 1e-9, n
        assert abs(o64["loss"][0] - g["loss_f64"][0]) <= 1e-9 * g["loss_f64"][0]


def test_landmark_weights_match_the_index_lists():
    unmatch = [93, 127, 132, 234, 323, 356, 361, 454]
    upper_eye = [161, 160, 159, 158, 157] + [388, 387, 386, 385, 384]
    eye = [33, 246, 161, 160, 159, 158, 157, 173, 133, 155, 154, 153, 145, 144, 163, 7] + \
          [263, 466, 388, 387, 386, 385, 384, 398, 362, 382, 381, 380, 374, 373, 390, 249]
    inner_lip = [78, 191, 80, 81, 82, 13, 312, 311, 310, 415, 308, 324, 318, 402, 317, 14, 87, 178, 88, 95]
    outer_lip = [61, 185, 40, 39, 37, 0, 267, 269, 270, 409, 291, 375, 321, 405, 314, 17, 84, 181, 91, 146]
    for kind, steps in (("image", ((eye, 5), (inner_lip, 2), (outer_lip, 2), (unmatch, 0))),
                        ("video", ((eye, 3), (upper_eye, 20), (inner_lip, 5), (outer_lip, 5), (unmatch, 0)))):
        w = torch.ones(1, 468, 2)          # as cal_lan_loss_mp writes them, in its order
        for idx, v in steps:
            w[:, idx] = v
        got = f3.landmark_weights(kind)
        assert got.dtype == np.float32 and got.shape == (468,) and np.array_equal(got, w[0, :, 0].numpy()) and np.array_equal(got, w[0, :, 1].numpy())
        assert (got == 0).sum() == 8
    assert (f3.landmark_weights("video") == 20).sum() == 10 and (f3.landmark_weights("image") == 5).sum() == 32
    w68 = torch.ones(1, 68, 2)
    w68[:, 36:48, :] = 3
    w68[:, -8:, :] = 3
    w68[:, 28:31, :] = 3
    for kind in ("image", "video"):
        assert np.array_equal(f3.landmark_weights(kind, "lm68"), w68[0, :, 0].numpy())
    assert tuple(synth.MP468_UNMATCHED) == tuple(unmatch) == f3.UNMATCHED
    with pytest.raises(ValueError):
        f3.landmark_weights("clip")
    g = load_golden("fit_3dmm_video_global_t7")
    assert np.array_equal(g["weights"], f3.landmark_weights("video")) and tuple(g["lambdas"]) == f3.LAMBDAS[("video", "global")]
    assert np.array_equal(load_golden("fit_3dmm_image_t1")["weights"], f3.landmark_weights("image"))


def test_the_fine_stage_is_dead_code():
    """`exp_para[sel_ids].data = ...` (process_video/fit_3dmm_landmark.py:355-358): indexing with a NumPy array copies, so the
    assignment reaches the copy only."""
    x = torch.zeros(3, 2, requires_grad=True)
    x[np.arange(3)].data = torch.ones(3, 2)
    assert not x.any()


def test_synth_face_keys():
    m = synth.synth_face_model(24, 0)
    before = {k: np.array(v, copy=True) for k, v in m.items() if isinstance(v, np.ndarray)}
    k = synth.synth_face_keys(m, 468, 5)
    assert all(np.array_equal(m[n], v) for n, v in before.items())          # synth_face_model's outputs do not change
    key, n = k["keypoints"], 625
    assert key.shape == (468,) and key.dtype == np.int64 and key.min() == 0 and key.max() < n
    assert all(key[i] == 0 for i in synth.MP468_UNMATCHED) and len(np.unique(key)) > 250
    assert k["key_mean_shape"].shape == (468, 3) and k["key_id_base"].shape == (1404, 80) and k["key_exp_base"].shape == (1404, 64)
    assert np.array_equal(k["key_id_base"][3 * 17:3 * 18], m["id_base"][3 * key[17]:3 * key[17] + 3])
    assert np.array_equal(k["key_mean_shape"][93], m["mean_shape"].reshape(-1, 3)[0])
    small = synth.synth_face_keys(synth.synth_face_model(24, 0, 3, 0), 5, 5)
    assert small["key_id_base"].shape == (15, 3) and small["key_exp_base"].shape == (15, 0)
    assert np.array_equal(synth.synth_face_keys(m, 468, 5)["keypoints"], key) and not np.array_equal(synth.synth_face_keys(m, 468, 6)["keypoints"], key)


def test_exported_from_the_package():
    import real3dportrait_amd as pkg
    for name in ("landmark_weights", "fit_landmarks", "fit_3dmm_for_landmarks", "patch_fit_3dmm"):
        assert getattr(pkg, name) is getattr(f3, name)


# ---- the launch plan (fit::plan of csrc/r3d_fit_3dmm.hip through the host-only hook r3d_debug_fit_plan) ----
PLAN_LS = (1, 5, 37, 68, 468, 625, 35709)
PLAN_KS = (1, 3, 50, 51, 100, 144, 511, 512)
PLAN_TS = (1, 7, 8, 9, 16, 17, 51, 500, 2000, 70000)
FIT_PLAN = ("V", "slabs", "chunk", "ychunks", "nsplit", "Kc", "lds_bytes", "ws_floats")
PG = 16          # frames whose poses fit_grad computes together
# the shapes tests/test_gpu_fit_3dmm.py runs for their plan: (L, Ki, Ke, T) -> (chunk, ychunks, frames of the last chunk, nsplit)
GPU_PLAN_CASES = {(468, 80, 64, 497): (17, 30, 4, 2), (468, 448, 64, 137): (18, 8, 11, 10)}
# ... and for their K regime, at T = 3: (L, Ki, Ke) -> (V, nsplit, Kc)
GPU_K_CASES = {(468, 50, 0): (85, 1, 50), (468, 51, 0): (83, 1, 51), (468, 100, 0): (42, 2, 50), (40, 448, 64): (8, 10, 52), (468, 1, 0): (85, 1, 1)}


def fit_plan(L, Ki, Ke, T):
    """-> (status, {V, slabs, chunk, ychunks, nsplit, Kc, lds_bytes, ws_floats}) of r3d_debug_fit_plan; no HIP call is made."""
    lib = _lib.load()
    assert hasattr(lib, "r3d_debug_fit_plan"), "%s does not export the plan hook: rebuild it" % _lib.LIB_PATH
    out = (ctypes.c_int32 * 8)(*[-1] * 8)
    rc = lib.r3d_debug_fit_plan(L, Ki, Ke, T, out)
    return rc, dict(zip(FIT_PLAN, out))


def test_plan_invariants_over_the_sweep():
    """Every (L, K, T) of the sweep: what fit_grad relies on (a thread per row of the slab, nsplit parts of a row within the block's 256
    threads and pbuf's 256 floats, the parts cover K, the LDS request within 64 KiB, the chunks tile T with none empty, grid.y within
    HIP's limit), the workspace the caller is asked for is the partial rows plus the snapshot's room, and the sizes the entry points refuse
    are refused by the hook with the same status and reason."""
    lib = _lib.load()
    lam = (ctypes.c_float * 6)(0.2, 0.6, 1.0, 1.0, 0.3, 0.3)
    refused = 0
    for L in PLAN_LS:
        for K in PLAN_KS:
            Ke = K // 3
            Ki = K - Ke
            for T in PLAN_TS:
                rc, p = fit_plan(L, Ki, Ke, T)
                V = max(1, min(12800 // (3 * K), 85, L))
                slabs = -(-L // V)
                if slabs * T * (K + 7) >= 1 << 31 or 2 * L * T >= 1 << 31:
                    msg = lib.r3d_last_error()
                    assert rc == -1 and b"debug_fit_plan" in msg and b"2^31" in msg, (L, K, T)
                    ptrs = [i << 40 for i in range(1, 15)]
                    got = lib.r3d_fit_landmark_grad(ptrs[0], ptrs[1], ptrs[2], L, Ki, Ke, ptrs[3], ptrs[4], T, 1, 10.0, 1015.0, 112.0, lam,
                                                    *ptrs[5:14], ptrs[13] + (1 << 39), 1 << 38, None)
                    assert got == rc and lib.r3d_last_error() == msg.replace(b"debug_fit_plan", b"fit_landmark_grad"), (L, K, T)
                    refused += 1
                    continue
                assert rc == 0, (L, K, T, lib.r3d_last_error())
                assert (p["V"], p["slabs"]) == (V, slabs) and 1 <= V and 3 * V <= 255, (L, K, T, p)
                chunk, ychunks, nsplit, Kc = p["chunk"], p["ychunks"], p["nsplit"], p["Kc"]
                assert 1 <= chunk and chunk * (ychunks - 1) < T <= chunk * ychunks and 1 <= ychunks <= 65535, (L, K, T, p)
                assert nsplit >= 1 and nsplit * 3 * V <= 256 and Kc * nsplit >= K, (L, K, T, p)
                rows3 = 3 * V
                assert p["lds_bytes"] == (K * (rows3 | 1) + K + 2 * 256 + 7 * V + PG * 39 + rows3 + V) * 4 and p["lds_bytes"] <= 65536, (L, K, T, p)
                assert p["ws_floats"] == (slabs * T * (K + 7) + 3) // 4 * 4, (L, K, T, p)
                room = (T * (K + 6) + 3) // 4 * 4          # the snapshot: a row of id per frame at the most
                assert p["ws_floats"] + room == lib.r3d_fit_workspace_bytes(L, Ki, Ke, T) // 4, (L, K, T, p)
    assert refused > 0
    out = (ctypes.c_int32 * 8)()
    for bad in ((0, 80, 64, 5), (468, 0, 64, 5), (468, 80, -1, 5), (468, 449, 64, 5), (468, 80, 64, 0), (1 << 20, 80, 64, 1 << 12)):
        assert lib.r3d_debug_fit_plan(*bad, out) == -1 and b"debug_fit_plan" in lib.r3d_last_error(), bad
    assert lib.r3d_debug_fit_plan(468, 80, 64, 5, None) == -1 and b"NULL" in lib.r3d_last_error()


def test_plan_values_are_pinned():
    """The regimes by number.  A video of 500 / 2000 frames (L = 468, K = 80 + 64): chunks of 17 / 67 frames, longer than the PG = 16
    poses a block computes at once, so every block refreshes its poses mid-chunk.  The suite's older shapes: chunks of 1 or 2.  The K
    regimes: K = 512, the top end (8 points a slab, rows split 10 ways, 52 + ... + 44 columns); K = 50 -> 51, where V steps from 85 to
    83 and the LDS request is within 300 bytes of the largest (K = 52).  The shapes of test_gpu_fit_3dmm.py's long-chunk and K cases.  A change to a plan constant has
    to come through here."""
    p500, p2000 = fit_plan(468, 80, 64, 500)[1], fit_plan(468, 80, 64, 2000)[1]
    assert (p500["V"], p500["slabs"], p500["chunk"], p500["ychunks"], p500["nsplit"]) == (29, 17, 17, 30, 2)
    assert (p2000["chunk"], p2000["ychunks"]) == (67, 30) and p500["chunk"] > PG
    for L in (5, 37, 468):
        for Ki, Ke in ((3, 0), (80, 64)):
            for T in (1, 2, 3, 7, 51, 53):
                p = fit_plan(L, Ki, Ke, T)[1]
                assert p["chunk"] in (1, 2), (L, Ki, Ke, T, p)
    assert [(fit_plan(L, 3, 0, 3)[1]["V"], fit_plan(L, 3, 0, 3)[1]["nsplit"]) for L in (468, 5)] == [(85, 1), (5, 17)]
    top = fit_plan(468, 448, 64, 3)[1]
    assert (top["V"], top["nsplit"], top["Kc"], 512 - 9 * top["Kc"], top["lds_bytes"]) == (8, 10, 52, 44, 58144)
    assert [(fit_plan(468, K, 0, 3)[1]["V"], fit_plan(468, K, 0, 3)[1]["lds_bytes"]) for K in (50, 51)] == [(85, 59484), (83, 59196)]
    assert max(fit_plan(468, K, 0, 3)[1]["lds_bytes"] for K in range(1, 513)) == 59736          # K = 52, V = 82; every K stays under 64 KiB
    for (L, Ki, Ke, T), (chunk, ychunks, last, nsplit) in GPU_PLAN_CASES.items():
        p = fit_plan(L, Ki, Ke, T)[1]
        assert (p["chunk"], p["ychunks"], T - chunk * (ychunks - 1), p["nsplit"]) == (chunk, ychunks, last, nsplit), (L, Ki, Ke, T, p)
    for (L, Ki, Ke), want in GPU_K_CASES.items():
        p = fit_plan(L, Ki, Ke, 3)[1]
        assert (p["V"], p["nsplit"], p["Kc"]) == want, (L, Ki, Ke, p)
