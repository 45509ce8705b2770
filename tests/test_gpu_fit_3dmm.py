"""GPU: the landmark-driven 3DMM fit (real3dportrait_amd/fit_3dmm.py, include/r3d_hip_fit.h) against the restatement
tests/fit_3dmm_ref.py in fp64: one evaluation's gradients, one and three Adam iterations from a given state, whole fits on the goldens,
run-to-run and stream-to-stream identity, the package's entry points and their call counts.

Tolerance, everywhere: 2e-4 of max|ref| per array, the project's; the final landmark loss 1e-4 relative.  Every test prints
the figure it asserts (pytest -s).

Measured on one MI355X, of max|ref|: gradients 1.3e-6 at worst (the restatement's own fp32 autograd: 2.7e-6), iterations 1.5e-6, whole
fits 1.3e-5 (id of the image case; absolute 5.9e-6 / 7.8e-6 / 7.7e-8 / 6.2e-7 for id / exp / euler / trans, recorded per case as
gpu_err_vs_fp64 in the goldens beside ref_err_vs_fp64, the fp32 restatement's own distance from fp64), final landmark loss 2.8e-6.
The cases over chunks longer than a pose group and over the K regimes assert the plan they claim through the library's own answer,
r3d_debug_fit_plan (tests/test_fit_3dmm_host.py pins the numbers): gradients 2.7e-7, iterations 1.0e-5 (three steps at T = 497)."""
import types

import numpy as np
import pytest
import torch

import fit_3dmm_ref as R
from conftest import load_golden
from real3dportrait_amd import _lib, synth
from test_fit_3dmm_host import GPU_K_CASES, GPU_PLAN_CASES, PG, fit_plan

pytestmark = pytest.mark.gpu

TOL = 2e-4
LAMBDAS = (0.2, 0.6, 1.0, 1.0, 0.3, 0.3)          # every term present
GOLDENS = ("fit_3dmm_image_t1", "fit_3dmm_video_global_t7", "fit_3dmm_video_global_t53", "fit_3dmm_video_fine_t7")
_models, _inputs = {}, {}


def fit3d():
    from real3dportrait_amd import fit_3dmm
    return fit_3dmm


def key_arrays(L, Ki, Ke):
    """(key_mean [3 L], key_id_base, key_exp_base) of the synthetic model, numpy; made once per size."""
    if (Ki, Ke) not in _models:
        _models[(Ki, Ke)] = synth.synth_face_model(24, 0, Ki, Ke)
    k = synth.synth_face_keys(_models[(Ki, Ke)], L, 5)
    return k["key_mean_shape"].reshape(-1), k["key_id_base"], k["key_exp_base"]


def on_device(arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


def inputs(L, Ki, Ke, T, id_rows):
    """Arrays, landmarks, weights with zeros and with 20, and non-zero random parameters: made once per case, never changed."""
    key = (L, Ki, Ke, T, id_rows)
    if key not in _inputs:
        arrays = key_arrays(L, Ki, Ke)
        seed = 1000 + 7 * L + T
        lms = R.synthetic_landmarks(arrays, T, id_rows, seed)
        w = np.array([0.0, 1.0, 3.0, 20.0], np.float32)[(synth.hash_uniform(seed, L, stream=95) * 4).astype(np.int64)]
        w[0], w[L - 1] = 20.0, 0.0
        params = [0.5 * synth.hash_unitvar(seed, (id_rows, Ki), stream=96), 0.5 * synth.hash_unitvar(seed, (T, Ke), stream=97),
                  0.3 * synth.hash_unitvar(seed, (T, 3), stream=98), 0.2 * synth.hash_unitvar(seed, (T, 3), stream=99)]
        _inputs[key] = (arrays, lms, w, [p.astype(np.float32) for p in params])
    return _inputs[key]


def close(got, ref, what, tol=TOL):
    """|got - ref| <= tol max|ref|, printed before it is asserted.  -> the distance over max|ref| (0 when both are all zero)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if ref.size == 0:
        return 0.0
    err, top = float(np.abs(got - ref).max()), float(np.abs(ref).max())
    print("%s: |got - ref| %.3e, max|ref| %.3e, ratio %.3e" % (what, err, top, err / top if top else 0.0))
    assert np.isfinite(got).all() and err <= tol * top, (what, err, top)
    return err / top if top else 0.0


def check_gradients(L, Ki, Ke, T, id_rows):
    """r3d_fit_landmark_grad at the case's inputs(): the loss record (1e-4 relative) and each of the four gradients of the total (TOL of
    max|ref|) against fp64 autograd of the restatement; the restatement's own fp32 autograd error is printed beside."""
    arrays, lms, w, params = inputs(L, Ki, Ke, T, id_rows)
    words, grads = R.gradients(arrays, lms, w, LAMBDAS, params)
    _, grads32 = R.gradients(arrays, lms, w, LAMBDAS, params, dtype=torch.float32)
    out = fit3d().landmark_grad(on_device(arrays), lms, w, id_rows, LAMBDAS, *(torch.from_numpy(p) for p in params))
    torch.cuda.synchronize()
    assert np.abs(grads[0]).max() > 0 and np.abs(grads[2]).max() > 0 and np.abs(grads[3]).max() > 0
    for n, g, ref, r32 in zip(R.NAMES, out[1:], grads, grads32):
        top = float(np.abs(ref).max()) if ref.size else 0.0
        if top:
            print("%s: fp32 autograd of the restatement %.3e of max|ref|" % (n, float(np.abs(r32 - ref).max()) / top))
        close(g.cpu().numpy(), ref, "grad " + n)
    got = out[0].cpu().numpy()
    for i, name in enumerate(fit3d().LOSS_NAMES):
        print("loss %s: got %.6e ref %.6e" % (name, got[i], words[i]))
        assert abs(got[i] - words[i]) <= 1e-4 * abs(words[i]) + 1e-12, (name, got[i], words[i])


@pytest.mark.parametrize("id_rows_is_T", [False, True])
@pytest.mark.parametrize("T", [1, 2, 3, 51])
@pytest.mark.parametrize("Ki,Ke", [(3, 0), (80, 64)])
@pytest.mark.parametrize("L", [5, 37, 468])
def test_gradients_against_fp64_autograd(L, Ki, Ke, T, id_rows_is_T):
    """L = 5 is one partial slab, 37 and 468 end in a slab that is not full; T = 1, 2, 3 are the Laplacian's replicate edges; id_rows 1
    sums the id gradient over the frames."""
    check_gradients(L, Ki, Ke, T, T if id_rows_is_T else 1)


@pytest.mark.parametrize("L,Ki,Ke,T,id_rows", [(468, 80, 64, 497, 1), (468, 448, 64, 137, 1), (468, 448, 64, 137, 137)])
def test_gradients_over_chunks_longer_than_a_pose_group(L, Ki, Ke, T, id_rows):
    """The regime of any video over 480 frames, asserted through the library's own plan (r3d_debug_fit_plan): a block walks a chunk of 17
    or 18 frames, more than the PG = 16 poses it computes at once, so frame 16 (and 17) of every chunk follows the mid-chunk refresh
    `f == 0 && tid < min(PG, t1 - t)` with t > t0 -- one or two lanes of it; the last chunks have 4 and 11 frames."""
    chunk, ychunks, last, nsplit = GPU_PLAN_CASES[(L, Ki, Ke, T)]
    rc, p = fit_plan(L, Ki, Ke, T)
    assert rc == 0 and (p["chunk"], p["ychunks"], p["nsplit"]) == (chunk, ychunks, nsplit) and T - chunk * (ychunks - 1) == last, p
    assert PG < p["chunk"] < 2 * PG and last < PG
    print("L %d K %d+%d T %d id_rows %d: V %d slabs %d chunk %d x %d (last %d frames) nsplit %d Kc %d, %d B of LDS"
          % (L, Ki, Ke, T, id_rows, p["V"], p["slabs"], p["chunk"], p["ychunks"], last, p["nsplit"], p["Kc"], p["lds_bytes"]))
    check_gradients(L, Ki, Ke, T, id_rows)


@pytest.mark.parametrize("L,Ki,Ke", sorted(GPU_K_CASES))
def test_gradients_over_the_k_regimes(L, Ki, Ke):
    """T = 3.  K = 50 and 51: V steps from 85 to 83 points a slab, at nearly the largest LDS request; K = 100: rows split 2 ways; K = 512, the
    accepted top end: V = 8, rows split 10 ways, 52 columns a part and 44 in the last; K = 1: stage() advances 256 rows a step."""
    rc, p = fit_plan(L, Ki, Ke, 3)
    assert rc == 0 and (p["V"], p["nsplit"], p["Kc"]) == GPU_K_CASES[(L, Ki, Ke)], p
    print("L %d K %d+%d: V %d slabs %d nsplit %d Kc %d (last part %d), %d B of LDS"
          % (L, Ki, Ke, p["V"], p["slabs"], p["nsplit"], p["Kc"], Ki + Ke - (p["nsplit"] - 1) * p["Kc"], p["lds_bytes"]))
    check_gradients(L, Ki, Ke, 3, 1)


def _state(arrays, T, id_rows, params, seed):
    """A state with non-zero moments: m ~ 0.01 N, v ~ 1e-4 U + 1e-6.  -> (m, v) lists of numpy arrays."""
    m = [(0.01 * synth.hash_unitvar(seed, p.shape, stream=60 + i)).astype(np.float32) for i, p in enumerate(params)]
    v = [(1e-4 * synth.hash_uniform(seed, p.size, stream=70 + i).reshape(p.shape) + 1e-6).astype(np.float32) for i, p in enumerate(params)]
    return m, v


def _run_from(arrays_dev, lms, w, id_rows, params, m, v, steps0, groups, n_iter):
    f = fit3d()
    Ki, Ke, T = params[0].shape[1], params[1].shape[1], params[2].shape[0]
    L = lms.shape[1]
    state = torch.cat([torch.from_numpy(np.concatenate([x.reshape(-1) for x in part])) for part in (params, m, v)] +
                      [torch.zeros(_lib.FIT_LOSS_WORDS)]).cuda()
    assert state.numel() * 4 == _lib.call("r3d_fit_state_bytes", Ki, Ke, T, id_rows)
    ws = torch.empty(_lib.call("r3d_fit_workspace_bytes", L, Ki, Ke, T) // 4, device="cuda")
    f.run(arrays_dev, torch.from_numpy(lms).cuda(), torch.from_numpy(w).cuda(), id_rows, LAMBDAS, state, ws, n_iter, groups, steps0)
    torch.cuda.synchronize()
    views = f.state_views(state.cpu(), Ki, Ke, T, id_rows)
    return views


# every group mask at the small shapes; chunks longer than a pose group (the snapshot's copy_run over 17 and 18 frames, id_rows 1 and T)
# with both groups, and with one group inactive for the first of them
ITERATION_CASES = [c + (g, n) for n in (1, 3) for g in (1, 2, 3) for c in ((468, 80, 64, 7, 1), (37, 80, 64, 3, 3), (5, 3, 0, 2, 1))] + \
                  [c + (3, n) for n in (1, 3) for c in ((468, 80, 64, 497, 1), (468, 448, 64, 137, 137))] + \
                  [(468, 80, 64, 497, 1, g, 1) for g in (1, 2)]


@pytest.mark.parametrize("L,Ki,Ke,T,id_rows,groups,n_iter", ITERATION_CASES)
def test_iterations_from_a_given_state(L, Ki, Ke, T, id_rows, groups, n_iter):
    """One and three iterations per group mask: parameters and both moments against the restatement in fp64; an inactive group keeps
    its parameters and moments bit for bit."""
    if (L, Ki, Ke, T) in GPU_PLAN_CASES:
        chunk, ychunks, last, _ = GPU_PLAN_CASES[(L, Ki, Ke, T)]
        p = fit_plan(L, Ki, Ke, T)[1]
        assert (p["chunk"], p["ychunks"]) == (chunk, ychunks) and p["chunk"] > PG and T - chunk * (ychunks - 1) == last, p
    arrays, lms, w, params = inputs(L, Ki, Ke, T, id_rows)
    m, v = _state(arrays, T, id_rows, params, 3)
    steps0 = (7, 200)
    rp, rm, rv, words = R.iterate(arrays, lms, w, LAMBDAS, params, m, v, steps0, groups, n_iter)
    got = _run_from(on_device(arrays), lms, w, id_rows, params, m, v, steps0, groups, n_iter)
    for i, n in enumerate(R.NAMES):
        active = groups & (1 if i < 2 else 2)
        for part, ref, start in (("p", rp, params), ("m", rm, m), ("v", rv, v)):
            g = got[part][i].numpy()
            if active:
                close(g, ref[i], "%s %s" % (part, n))
            else:
                assert np.array_equal(g, start[i]), (part, n)
    if params[2].size:
        assert np.abs(rp[2] - params[2]).max() > 1e-3 or not groups & 2          # a step moves the parameters by about lr
    loss = got["loss"].numpy()
    print("loss total: got %.6e ref %.6e" % (loss[7], words[7]))
    assert abs(loss[7] - words[7]) <= 1e-4 * abs(words[7])


def test_frame_step_count_is_carried():
    """The frame group's Adam step number decides its bias corrections: the same state stepped as number 201 and as number 1 differs,
    and each agrees with the restatement at that number."""
    L, Ki, Ke, T, id_rows = 37, 80, 64, 3, 1
    arrays, lms, w, params = inputs(L, Ki, Ke, T, id_rows)
    m, v = _state(arrays, T, id_rows, params, 4)
    dev = on_device(arrays)
    a = _run_from(dev, lms, w, id_rows, params, m, v, (0, 200), 3, 1)
    b = _run_from(dev, lms, w, id_rows, params, m, v, (0, 0), 3, 1)
    for steps0, got in (((0, 200), a), ((0, 0), b)):
        rp = R.iterate(arrays, lms, w, LAMBDAS, params, m, v, steps0, 3, 1)[0]
        close(got["p"][2].numpy(), rp[2], "euler at step %d" % (steps0[1] + 1))
        close(got["p"][3].numpy(), rp[3], "trans at step %d" % (steps0[1] + 1))
    d = float((a["p"][2] - b["p"][2]).abs().max())
    print("euler after step 201 against step 1: %.3e" % d)
    assert d > 100 * TOL * float(a["p"][2].abs().max())
    assert torch.equal(a["p"][0], b["p"][0]) and torch.equal(a["p"][1], b["p"][1])          # id and exp: the same step 1


def _golden_fit(name, **kw):
    g = load_golden(name)
    _, _, key_seed, L, T, id_rows, _, img = (int(x) for x in g["spec"])
    arrays = key_arrays(L, 80, 64)
    assert abs(float(sum(a.astype(np.float64).sum() for a in arrays)) - float(g["model_sum"])) < 1e-6
    lms = R.preprocess(g["lms_px"], img)
    return g, fit3d().fit_landmarks(on_device(arrays), lms, g["weights"], id_rows, tuple(float(x) for x in g["lambdas"]), **kw)


@pytest.mark.parametrize("name", GOLDENS)
def test_whole_fit_against_fp64(name):
    """400 iterations from zeros: the coefficients after stage 1 and after stage 2 within 2e-4 max|ref| of the fp64 run, per array; the
    final landmark loss within 1e-4 relative of fp64's."""
    g, out = _golden_fit(name, stages=True)
    torch.cuda.synchronize()
    ratios = []
    for i, n in enumerate(R.NAMES):
        close(out[5][i].cpu().numpy(), g["s1_%s_f64" % n], "%s stage 1 %s" % (name, n))
        ratios.append(close(out[i].cpu().numpy(), g["s2_%s_f64" % n], "%s stage 2 %s" % (name, n)))
    print("%s gpu_err_vs_fp64 (absolute):" % name, [float(np.abs(out[i].cpu().numpy() - g["s2_%s_f64" % n]).max()) for i, n in enumerate(R.NAMES)],
          "ref_err_vs_fp64:", g["ref_err_vs_fp64"].tolist())
    lan, ref = float(out[4][0]), float(g["loss_f64"][0])
    print("%s final landmark loss: got %.7e fp64 %.7e, relative %.3e" % (name, lan, ref, abs(lan - ref) / ref))
    assert abs(lan - ref) <= 1e-4 * ref


def test_bit_identical_over_runs_and_streams():
    _, first = _golden_fit("fit_3dmm_video_global_t7")
    torch.cuda.synchronize()
    _, again = _golden_fit("fit_3dmm_video_global_t7")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        _, other = _golden_fit("fit_3dmm_video_global_t7")
    side.synchronize()
    for a, b, c in zip(first, again, other):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert float(first[0].abs().max()) > 0.1


class _FaceModel:
    """What fit_3dmm_for_landmarks takes from a ParametricFaceModel."""
    def __init__(self):
        arrays = key_arrays(468, 80, 64)
        self.key_mean_shape, self.key_id_base, self.key_exp_base = arrays[0].reshape(-1, 3), arrays[1], arrays[2]
        self.focal, self.center, self.camera_distance = 1015.0, 112.0, 10.0


@pytest.mark.parametrize("kind,id_mode,name", [("image", "global", "fit_3dmm_image_t1"), ("video", "global", "fit_3dmm_video_global_t7"),
                                               ("video", "finegrained", "fit_3dmm_video_fine_t7")])
def test_fit_3dmm_for_landmarks_returns_the_references_dict(kind, id_mode, name):
    """Keys, shapes and dtypes of the reference's coeff_dict, the values of the golden's fp64 run, and two `run` calls per fit."""
    g = load_golden(name)
    T = int(g["spec"][4])
    fm = _FaceModel()
    lms = g["lms_px"][0] if kind == "image" else g["lms_px"]
    with _lib.counting() as calls:
        d = fit3d().fit_3dmm_for_landmarks(fm, lms, 512, kind, id_mode=id_mode)
    runs = [c for c in calls if c[0] == "r3d_fit_landmark_run"]
    assert len(runs) == fit3d().RUNS_PER_FIT == 2 and not [c for c in calls if c[0] == "r3d_fit_landmark_grad"]
    assert [r[1][18] for r in runs] == [200, 200] and [r[1][19] for r in runs] == [2, 3] and [r[1][17] for r in runs] == [0, 200]
    assert list(d) == ["id", "exp", "euler", "trans"]
    shapes = {"id": (T if id_mode == "finegrained" else 1, 80), "exp": (T, 64), "euler": (T, 3), "trans": (T, 3)}
    for n in R.NAMES:
        assert isinstance(d[n], np.ndarray) and d[n].dtype == np.float32 and d[n].shape == shapes[n], (n, d[n].dtype, d[n].shape)
        close(d[n], g["s2_%s_f64" % n], "%s %s" % (name, n))
    t = fit3d().fit_3dmm_for_landmarks(fm, lms, 512, kind, id_mode=id_mode, as_numpy=False)
    assert all(torch.is_tensor(t[n]) and t[n].is_cuda and np.array_equal(t[n].cpu().numpy(), d[n]) for n in R.NAMES)
    assert len(fm.__dict__["_r3d_face_model_arrays"]) == 1          # uploaded once


def test_patch_fit_3dmm_on_a_stub_module(tmp_path):
    """The wrappers keep the reference's arguments and returns, take landmarks from the callable, and leave the old functions reachable."""
    g1, g7 = load_golden("fit_3dmm_image_t1"), load_golden("fit_3dmm_video_global_t7")
    old_image, old_video = (lambda *a, **k: "old image"), (lambda *a, **k: "old video")
    mod = types.SimpleNamespace(fit_3dmm_for_a_image=old_image, fit_3dmm_for_a_video=old_video)
    seen = []

    def image_landmarks(img_name):
        seen.append(img_name)
        return (None, 512) if "nobody" in img_name else (np.concatenate([g1["lms_px"][0], np.zeros((10, 2), np.float32)]), 512)          # 478 points

    def video_landmarks(video_name):
        seen.append(video_name)
        return g7["lms_px"], 512

    f = fit3d()
    assert f.patch_fit_3dmm(mod, _FaceModel(), image_landmarks, video_landmarks) is mod
    assert mod._r3d_reference_fit_3dmm_for_a_image is old_image and mod._r3d_reference_fit_3dmm_for_a_video is old_video
    d = mod.fit_3dmm_for_a_image("/data/images_512/a.png", save=False)
    for n in R.NAMES:
        close(d[n], g1["s2_%s_f64" % n], "patched image " + n)
    assert mod.fit_3dmm_for_a_image("/data/images_512/nobody.png", save=False) is None
    name = str(tmp_path / "video" / "clip.mp4")
    d = mod.fit_3dmm_for_a_video(name, False, "global", save=True)
    for n in R.NAMES:
        close(d[n], g7["s2_%s_f64" % n], "patched video " + n)
    saved = np.load(str(tmp_path / "coeff_fit_mp" / "clip_coeff_fit_mp.npy"), allow_pickle=True).item()
    assert sorted(saved) == sorted(R.NAMES) and np.array_equal(saved["exp"], d["exp"])
    assert seen == ["/data/images_512/a.png", "/data/images_512/nobody.png", name]
    with pytest.raises(AssertionError):
        mod.fit_3dmm_for_a_video("clip.avi")
    with pytest.raises(NotImplementedError):
        mod.fit_3dmm_for_a_video(name, id_mode="other")
    f.patch_fit_3dmm(mod, _FaceModel(), image_landmarks, video_landmarks)          # patched twice: the reference stays the reference
    assert mod._r3d_reference_fit_3dmm_for_a_image is old_image
