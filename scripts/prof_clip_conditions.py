"""Time the HIP per-clip conditions at T = 250 and T = 2500 frames and print one JSON line:

  * clip_camera (one launch) and clip_keypoints (two launches), host wall clock around `calls` calls that end in one synchronise,
    `blocks` blocks after a warm-up; reported: the median of the block means and their spread;
  * beside them, in alternating blocks of the same run: the host route the package can run here -- the copies of euler and trans to the
    host, tests/clip_conditions_ref64.py's per-frame NumPy loop (a STAND-IN for the reference's two functions, whose per-frame torch
    and scipy calls it does not have) and the copy back -- and the torch-on-device arithmetic of smooth_features_xd for the key points
    (flip, cat, permute, conv1d, permute back, the zero column).

    python scripts/prof_clip_conditions.py [--calls 50] [--blocks 5] [--host-calls 2] [--out DIR]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--host-calls", type=int, default=2)
    ap.add_argument("--frames", type=int, nargs="+", default=[250, 2500])
    ap.add_argument("--out", default=None)
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

    def timed(fn, calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / calls * 1e3

    result = {"unit": "ms per call", "calls": a.calls, "blocks": a.blocks, "host_calls": a.host_calls, "device": torch.cuda.get_device_name(0)}
    for T in a.frames:
        e_np, t_np = C64.trajectory(T)
        euler, trans = D(e_np), D(t_np)
        drv, src = D(C64.uniform(1, (T, 68, 2), 1.0)), D(C64.uniform(2, (1, 68, 2), 1.0))
        routes = {"hip_clip_camera": (lambda: clip_camera(euler, trans), a.calls),
                  "hip_clip_keypoints": (lambda: clip_keypoints(src, drv), a.calls),
                  "torch_device_keypoints": (lambda: torch_keypoints(src, drv), a.calls),
                  "host_numpy_camera_stand_in": (lambda: host_camera(euler, trans), a.host_calls)}
        got, ref = clip_keypoints(src, drv)[1], torch_keypoints(src, drv)[1]
        kp_diff = float((got - ref).abs().max())
        cam_diff = float((clip_camera(euler, trans) - host_camera(euler, trans)).abs().max())
        for fn, calls in routes.values():          # warm-up: code objects, the allocator's blocks
            timed(fn, min(calls, 3))
        samples = {k: [] for k in routes}
        for _ in range(a.blocks):                  # alternating blocks
            for k, (fn, calls) in routes.items():
                samples[k].append(timed(fn, calls))
        result["T%d" % T] = dict({k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in samples.items()},
                                 max_abs_diff_keypoints_hip_vs_torch=kp_diff, max_abs_diff_camera_hip_vs_host=cam_diff)
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "prof_clip_conditions.json"), "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
