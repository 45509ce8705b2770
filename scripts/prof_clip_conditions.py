"""Time the HIP per-clip conditions at T = 250 and T = 2500 frames and print one JSON line:

  * clip_camera (one launch) and clip_keypoints (two launches), host wall clock around `calls` calls that end in one synchronise,
    `blocks` blocks after a warm-up; reported: the median of the block means and their spread;
  * beside them, in alternating blocks of the same run: the host route the package can run here -- the copies of euler and trans to the
    host, tests/clip_conditions_ref64.py's per-frame NumPy loop (a STAND-IN for the reference's two functions, whose per-frame torch
    and scipy calls it does not have) and the copy back -- and the torch-on-device arithmetic of smooth_features_xd for the key points
    (flip, cat, permute, conv1d, permute back, the zero column).

    python scripts/prof_clip_conditions.py [--calls 50] [--blocks 5] [--host-calls 2] [--out DIR]
"""
import _prof

_prof.paths(tests=True)


def main():
    ap = _prof.parser(__doc__, calls=50)
    ap.add_argument("--host-calls", type=int, default=2)
    ap.add_argument("--frames", type=int, nargs="+", default=[250, 2500])
    a = ap.parse_args()
    import numpy as np
    import torch
    import torch.nn.functional as F

    import clip_conditions_ref64 as C64
    from real3dportrait_amd import clip_camera, clip_keypoints

    assert torch.cuda.is_available(), "timings need the GPU"
    dev = "cuda:0"
    D = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)

    def torch_keypoints(src, drv, ks=7):
        """smooth_features_xd's own operations (infer_utils.py:71-101) on the device, then the zero columns of real3d_infer.py:481-482."""
        t, pad = drv.shape[0], (ks - 1) // 2
        x = drv.reshape(t, -1)
        x = torch.cat([torch.flip(x[0:pad], dims=[0]), x, torch.flip(x[t - pad:t], dims=[0])], dim=0)
        x = x.permute(1, 0).reshape([-1, 1, t + 2 * pad])
        k = 1 / ks * torch.ones(1, 1, ks, device=x.device)
        y = F.conv1d(x, k).reshape([-1, t]).permute(1, 0).reshape(t, 68, 2)
        zeros = torch.zeros(t, 68, 1, device=x.device)
        return torch.cat([src.expand(t, 68, 2), zeros], dim=-1), torch.cat([y, zeros], dim=-1)

    def host_camera(euler, trans):
        cam = C64.clip_camera(euler.cpu().numpy(), trans.cpu().numpy(), 7)
        return torch.tensor(cam).to(dev).float()

    def timed(fn, calls):          # warm-up: code objects, the allocator's blocks
        return _prof.route(fn, _prof.by_host_clock, calls, warmup=min(calls, 3))

    result = {"unit": "ms per call", "calls": a.calls, "blocks": a.blocks, "host_calls": a.host_calls, "device": torch.cuda.get_device_name(0)}
    for T in a.frames:
        e_np, t_np = C64.trajectory(T)
        euler, trans = D(e_np), D(t_np)
        drv, src = D(C64.uniform(1, (T, 68, 2), 1.0)), D(C64.uniform(2, (1, 68, 2), 1.0))
        routes = {"hip_clip_camera": timed(lambda: clip_camera(euler, trans), a.calls),
                  "hip_clip_keypoints": timed(lambda: clip_keypoints(src, drv), a.calls),
                  "torch_device_keypoints": timed(lambda: torch_keypoints(src, drv), a.calls),
                  "host_numpy_camera_stand_in": timed(lambda: host_camera(euler, trans), a.host_calls)}
        got, ref = clip_keypoints(src, drv)[1], torch_keypoints(src, drv)[1]
        kp_diff = float((got - ref).abs().max())
        cam_diff = float((clip_camera(euler, trans) - host_camera(euler, trans)).abs().max())
        samples = _prof.alternate(routes, a.blocks, warmup=0)          # every route brings its own
        result["T%d" % T] = dict({k: _prof.median_min_max(v) for k, v in samples.items()},
                                 max_abs_diff_keypoints_hip_vs_torch=kp_diff, max_abs_diff_camera_hip_vs_host=cam_diff)
    _prof.emit(result, a.out, "prof_clip_conditions")


if __name__ == "__main__":
    main()
