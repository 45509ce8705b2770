"""Time the HIP landmark-driven 3DMM fit per fit at T = 1, 53 and 250 frames and print one JSON line:

  * fit_3dmm_for_landmarks (kind 'image' at T = 1, kind 'video' with one id for the clip otherwise; 400 iterations = 800 launches in two
    library calls) on the synthetic model and landmarks, as_numpy=False, host wall clock around `calls` fits that end in one
    synchronise, `blocks` blocks after a warm-up; reported: the median of the block means and their minimum and maximum;
  * beside it, in alternating blocks of the same run: eager fp32 torch of the same math and schedule on the same GPU,
    tests/fit_3dmm_ref.py with dtype float32 on the device (autograd and torch.optim.Adam, as the reference runs them) -- the
    baseline; the reference's own two functions are not on the GPU machine;
  * the largest difference of the two results, of max|eager|, per array.

    python scripts/prof_fit_3dmm.py [--calls 3] [--blocks 5] [--frames 1 53 250] [--eager-calls 1] [--out DIR]
"""
import _prof

_prof.paths(tests=True)


def main():
    ap = _prof.parser(__doc__, calls=3)
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 53, 250])
    ap.add_argument("--eager-calls", type=int, default=1, help="fits per block of the eager route (a fit is 400 iterations)")
    a = ap.parse_args()
    import numpy as np
    import torch

    import fit_3dmm_ref as ref
    from real3dportrait_amd import _lib, fit_3dmm, synth

    assert torch.cuda.is_available(), "timings need the GPU"
    dev = "cuda:0"
    keys = synth.synth_face_keys(synth.synth_face_model(24, 0), 468, 5)
    arrays = (keys["key_mean_shape"].reshape(-1), keys["key_id_base"], keys["key_exp_base"])
    arrays_dev = tuple(torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in arrays)

    class FaceModel:
        key_mean_shape, key_id_base, key_exp_base = keys["key_mean_shape"], keys["key_id_base"], keys["key_exp_base"]
        focal, center, camera_distance = 1015.0, 112.0, 10.0

    fm = FaceModel()
    result = {"unit": "ms per fit", "calls": a.calls, "eager_calls": a.eager_calls, "blocks": a.blocks, "device": torch.cuda.get_device_name(0),
              "launches": 400 * _lib.FIT_LAUNCHES}
    for T in a.frames:
        kind = "image" if T == 1 else "video"
        lms_px = ref.synthetic_pixels(arrays, T, 1, 31 + T)
        lms = torch.from_numpy(ref.preprocess(lms_px, 512)).to(dev)
        w = torch.from_numpy(fit_3dmm.landmark_weights(kind)).to(dev)
        lam = fit_3dmm.LAMBDAS[(kind, "finegrained" if T == 1 else "global")]
        hip = lambda: fit_3dmm.fit_3dmm_for_landmarks(fm, lms_px[0] if T == 1 else lms_px, 512, kind, as_numpy=False)
        eager = lambda: ref.fit(arrays_dev, lms, w, 1, lam, dtype=torch.float32, device=dev)
        got, want = hip(), eager()["stage2"]
        diff = {n: float(np.abs(got[n].cpu().numpy() - want[n]).max() / np.abs(want[n]).max()) for n in ref.NAMES}
        samples = _prof.alternate({"hip": _prof.route(hip, _prof.by_host_clock, a.calls, warmup=2),
                                   "eager_torch_fp32": _prof.route(eager, _prof.by_host_clock, a.eager_calls, warmup=0)}, a.blocks, warmup=0)
        result["T%d" % T] = dict({k: _prof.median_min_max(v) for k, v in samples.items()}, max_diff_hip_vs_eager_of_max=diff)
    _prof.emit(result, a.out, "prof_fit_3dmm")


if __name__ == "__main__":
    main()
