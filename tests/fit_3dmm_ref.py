"""The landmark-driven 3DMM fit restated with torch autograd and torch.optim.Adam, in any dtype: the reference for every
comparison of tests/test_gpu_fit_3dmm.py and tests/test_fit_3dmm_host.py.

fit_3dmm_for_a_image (data_gen/utils/process_image/fit_3dmm_landmark.py:85-264) and fit_3dmm_for_a_video
(data_gen/utils/process_video/fit_3dmm_landmark.py:130-459) up to the state their coeff_dict is taken from:

    project        compute_for_landmark_fit (deep_3drecon/deep_3drecon_models/bfm.py:349-366), columns 0 and 1
    lap            cal_lap_loss (process_video/fit_3dmm_landmark.py:64-74)
    terms, total   the loss record and the loss of one iteration: weighted landmark term, mean squares, Laplacians
    fit            stage 1, 200 iterations, the landmark term alone, Adam([euler, trans], lr=.1); stage 2, 200 iterations of the total,
                   Adam([id, exp], lr=.1) from step 1 beside the frame optimiser, which continues with its moments and step count
    iterate        n iterations from a given state (parameters, moments, step counts) for a group mask

The fine stage after stage 2 is not restated: its results are assigned to copies (x[numpy index].data = ...) and never reach the
coeff_dict.  The two velocity terms have weight 0 (and are NaN for a [1, 80] id): left out.
"""
import numpy as np
import torch
import torch.nn.functional as F

CAMERA_DISTANCE, FOCAL, CENTER = 10.0, 1015.0, 112.0
NAMES = ("id", "exp", "euler", "trans")


def rotation(euler):
    """compute_rotation (bfm.py:204-238): euler [T, 3] -> (Rz Ry Rx)^T per frame, to be used as p @ rot."""
    x, y, z = euler[:, :1], euler[:, 1:2], euler[:, 2:]
    one, zero = torch.ones_like(x), torch.zeros_like(x)
    T = euler.shape[0]
    rx = torch.cat([one, zero, zero, zero, torch.cos(x), -torch.sin(x), zero, torch.sin(x), torch.cos(x)], dim=1).reshape(T, 3, 3)
    ry = torch.cat([torch.cos(y), zero, torch.sin(y), zero, one, zero, -torch.sin(y), zero, torch.cos(y)], dim=1).reshape(T, 3, 3)
    rz = torch.cat([torch.cos(z), -torch.sin(z), zero, torch.sin(z), torch.cos(z), zero, zero, zero, one], dim=1).reshape(T, 3, 3)
    return (rz @ ry @ rx).permute(0, 2, 1)


def project(arrays, id, exp, euler, trans, camera_distance=CAMERA_DISTANCE, focal=FOCAL, center=CENTER):
    """arrays = (key_mean [3 L], key_id_base [3 L, Ki], key_exp_base [3 L, Ke]); id [1 or T, Ki], exp [T, Ke] -> proj [T, L, 2]."""
    mean, idb, expb = arrays
    T = euler.shape[0]
    shape = id.expand(T, -1) @ idb.t() + exp @ expb.t() + mean.reshape(1, -1)
    q = shape.reshape(T, -1, 3) @ rotation(euler) + trans.unsqueeze(1)
    z = camera_distance - q[..., 2]
    return torch.stack([(focal * q[..., 0] + center * z) / z, (focal * q[..., 1] + center * z) / z], dim=-1)


def lap(x):
    """cal_lap_loss of x [T, C]: replicate padding along T, conv1d with (-0.5, 1, -0.5), the mean of the squares."""
    t = x.shape[0]
    x = x.reshape(t, -1).permute(1, 0).unsqueeze(1)
    x = torch.cat([x[:, :, 0:1], x, x[:, :, -1:]], dim=-1)
    k = torch.tensor((-0.5, 1.0, -0.5), dtype=x.dtype, device=x.device).reshape(1, 1, 3)
    return torch.mean(F.conv1d(x, k) ** 2)


def terms(arrays, lms, weights, id, exp, euler, trans, **camera):
    """The loss record's first seven entries; mean(exp^2) and lap(exp) of an empty exp are 0."""
    proj = project(arrays, id, exp, euler, trans, **camera)
    lan = torch.mean(weights.reshape(1, -1, 1) * (proj - lms) ** 2)
    zero = lan * 0
    has_exp = exp.numel() > 0
    return [lan, torch.mean(id * id), torch.mean(exp * exp) if has_exp else zero, lap(id), lap(exp) if has_exp else zero, lap(euler), lap(trans)]


def total(tm, lambdas):
    out = tm[0]
    for lam, v in zip(lambdas, tm[1:]):
        out = out + float(lam) * v
    return out


def _t(a, dtype, device):
    return torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a).to(device=device, dtype=dtype)


def gradients(arrays, lms, weights, lambdas, params, dtype=torch.float64, device="cpu", **camera):
    """One evaluation: params = (id, exp, euler, trans) -> (the eight loss words, the four gradients of the total), numpy."""
    arrays = tuple(_t(a, dtype, device) for a in arrays)
    lms, weights = _t(lms, dtype, device), _t(weights, dtype, device)
    p = [_t(x, dtype, device).clone().requires_grad_(True) for x in params]
    tm = terms(arrays, lms, weights, *p, **camera)
    tot = total(tm, lambdas)
    tot.backward()
    grads = [x.grad if x.grad is not None else torch.zeros_like(x) for x in p]
    return np.array([float(v.detach()) for v in tm] + [float(tot.detach())]), [g.cpu().numpy() for g in grads]


def _adam(params, lr, state=None):
    opt = torch.optim.Adam(params, lr=lr)
    if state is not None:
        step0, ms, vs = state
        for p, m, v in zip(params, ms, vs):
            opt.state[p] = {"step": torch.tensor(float(step0)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
    return opt


def iterate(arrays, lms, weights, lambdas, params, m, v, steps0, groups, n_iter, lr=(0.1, 0.1), dtype=torch.float64, device="cpu", **camera):
    """n_iter iterations of the total loss from a given state: params, m, v are (id, exp, euler, trans) each, steps0 = (steps the id / exp
    moments have seen, steps the euler / trans moments have seen), groups bit 0 id + exp, bit 1 euler + trans.
    -> (params, m, v) as lists of numpy arrays and the loss words of the last iterate consumed."""
    arrays = tuple(_t(a, dtype, device) for a in arrays)
    lms, weights = _t(lms, dtype, device), _t(weights, dtype, device)
    p = [_t(x, dtype, device).clone().requires_grad_(True) for x in params]
    ms, vs = [_t(x, dtype, device) for x in m], [_t(x, dtype, device) for x in v]
    opts = []
    for bit, sl in ((1, slice(0, 2)), (2, slice(2, 4))):
        if groups & bit:
            opts.append((sl, _adam(p[sl], lr[bit - 1], (steps0[bit - 1], ms[sl], vs[sl]))))
    words = None
    for _ in range(n_iter):
        tm = terms(arrays, lms, weights, *p, **camera)
        tot = total(tm, lambdas)
        for x in p:
            x.grad = None
        tot.backward()
        for _, opt in opts:
            opt.step()
        words = np.array([float(x.detach()) for x in tm] + [float(tot.detach())])
    for sl, opt in opts:
        for i, x in zip(range(sl.start, sl.stop), p[sl]):
            if x in opt.state:          # (a parameter without a gradient, an empty exp, has no state)
                ms[i], vs[i] = opt.state[x]["exp_avg"], opt.state[x]["exp_avg_sq"]
    out = lambda xs: [x.detach().cpu().numpy() for x in xs]
    return out(p), out(ms), out(vs), words


def fit(arrays, lms, weights, id_rows, lambdas, dtype=torch.float64, device="cpu", iters=(200, 200), lr=0.1, **camera):
    """The schedule of both reference functions from zeros.  lms [T, L, 2] already in the 224-pixel frame with y up.
    -> {"stage1": {id, exp, euler, trans}, "stage2": {...}, "loss": the eight loss words of the last iterate stage 2 consumed}."""
    arrays = tuple(_t(a, dtype, device) for a in arrays)
    lms, weights = _t(lms, dtype, device), _t(weights, dtype, device)
    T, Ki, Ke = lms.shape[0], arrays[1].shape[1], arrays[2].shape[1]
    id = torch.zeros(id_rows, Ki, dtype=dtype, device=device, requires_grad=True)
    exp = torch.zeros(T, Ke, dtype=dtype, device=device, requires_grad=True)
    euler = torch.zeros(T, 3, dtype=dtype, device=device, requires_grad=True)
    trans = torch.zeros(T, 3, dtype=dtype, device=device, requires_grad=True)
    opt_idexp, opt_frame = torch.optim.Adam([id, exp], lr=lr), torch.optim.Adam([euler, trans], lr=lr)
    snap = lambda: {n: x.detach().cpu().numpy().copy() for n, x in zip(NAMES, (id, exp, euler, trans))}
    for _ in range(iters[0]):
        loss = torch.mean(weights.reshape(1, -1, 1) * (project(arrays, id, exp, euler, trans, **camera) - lms) ** 2)
        opt_frame.zero_grad()
        loss.backward()
        opt_frame.step()
    out = {"stage1": snap()}
    words = None
    for _ in range(iters[1]):
        tm = terms(arrays, lms, weights, id, exp, euler, trans, **camera)
        loss = total(tm, lambdas)
        opt_idexp.zero_grad()
        opt_frame.zero_grad()
        loss.backward()
        opt_idexp.step()
        opt_frame.step()
        words = np.array([float(x.detach()) for x in tm] + [float(loss.detach())])
    out["stage2"], out["loss"] = snap(), words
    return out


# ---- the tests' inputs -------------------------------------------------------------------------------------------------------------------
GT_SIGMA = (0.8, 0.5, 0.15, 0.1)          # ground-truth id, exp, euler, trans
NOISE_PX = 0.3


def synthetic_landmarks(arrays, T, id_rows, seed):
    """Landmarks of ground-truth coefficients of GT_SIGMA (from the project's hash) through `project` in fp64, plus NOISE_PX of noise:
    lms [T, L, 2] float32 in the 224-pixel frame, y up, as the fit takes them."""
    from real3dportrait_amd import synth
    Ki, Ke = np.asarray(arrays[1]).shape[1], np.asarray(arrays[2]).shape[1]
    gt = [GT_SIGMA[0] * synth.hash_unitvar(seed, (id_rows, Ki), stream=90), GT_SIGMA[1] * synth.hash_unitvar(seed, (T, Ke), stream=91),
          GT_SIGMA[2] * synth.hash_unitvar(seed, (T, 3), stream=92), GT_SIGMA[3] * synth.hash_unitvar(seed, (T, 3), stream=93)]
    a64 = tuple(_t(a, torch.float64, "cpu") for a in arrays)
    proj = project(a64, *(_t(g, torch.float64, "cpu") for g in gt)).numpy()
    noise = NOISE_PX * synth.hash_unitvar(seed, proj.shape, stream=94)
    return (proj + noise).astype(np.float32)


def preprocess(lms_px, img_size):
    """The reference's landmark preprocessing in fp32 as it runs it (process_video :178-206): the first 468 points, y <- img_size - y,
    then the division by img_size / 224.  lms_px [T, >= 468, 2] pixels, y down -> [T, 468, 2] float32."""
    lms = torch.FloatTensor(np.array(np.asarray(lms_px)[:, :468, :], np.float32))          # a copy: FloatTensor shares a float32 array's memory
    lms[..., 1] = img_size - lms[..., 1]
    lms /= img_size / (CENTER * 2)
    return lms.numpy()


def synthetic_pixels(arrays, T, id_rows, seed, img_size=512):
    """synthetic_landmarks as a landmarker would give them: pixels of a square img_size image, y down, float32."""
    lms = synthetic_landmarks(arrays, T, id_rows, seed).astype(np.float64) * (img_size / (CENTER * 2))
    lms[..., 1] = img_size - lms[..., 1]
    return lms.astype(np.float32)
