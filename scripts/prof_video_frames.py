"""Time the HIP output video frames for a clip of T = 250 frames at 512 x 512 (image_raw and image_depth 128 x 128, the
SECC maps 512 x 512), out_mode 'concat_debug', and print one JSON line:

  * hip_range, hip_compose, hip_kernels  the reduction, the composer and both, device events around `calls` calls, `blocks` blocks after
                                         a warm-up; the median of the block means and their spread;
  * hip_kernels_and_copy                 both kernels and the ONE copy of the uint8 frames to the host, host clock to the copy's end;
  * torch_device                         the reference's operator sequence (tests/video_frames_ref.py) with every tensor left on the device;
  * host_reference                       that sequence as the reference runs it: five .cpu() copies of fp32 panels and everything after
                                         them on the host's CPU, for the first `host_frames` frames (the fp64 strip of 250 frames is 7.9 GB).
  * hip_compose_panel_0 .. 4             the composer with one panel selected (ref, secc, raw, depth, image): a fifth of the output each;
  The composer's achieved bytes per second count each source once and the output once.

    python scripts/prof_video_frames.py [--frames 250] [--host-frames 50] [--calls 10] [--blocks 5] [--out DIR]
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
FLOAT4_COPY_BYTES_PER_S = 6.29e12          # the measured rate of a float4 copy on the MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=250)
    ap.add_argument("--host-frames", type=int, default=50)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import torch.nn.functional as F

    import video_frames_ref as R
    from real3dportrait_amd import video_frames as V

    assert torch.cuda.is_available(), "timings need the GPU"
    dev, T, S, s = "cuda:0", a.frames, a.size, a.size // 4
    g = torch.Generator(device=dev).manual_seed(3)
    u = lambda *shape: torch.rand(*shape, device=dev, generator=g) * 2.2 - 1.1
    ref, secc, raw, img = u(1, 3, S, S), u(T, 3, S, S), u(T, 3, s, s), u(T, 3, S, S)
    depth = torch.rand(T, 1, s, s, device=dev, generator=g) + 2
    out = torch.empty(T, S, 5 * S, 3, dtype=torch.uint8, device=dev)
    state = V.new_depth_state(dev)
    host_out = torch.empty(out.shape, dtype=torch.uint8).pin_memory()

    def torch_device(n):
        """tests/video_frames_ref.py concat_debug with no .cpu() and no NumPy: the same operators and dtypes on the device."""
        secc_img = torch.cat([F.interpolate(secc[i:i + 1], (S, S)) for i in range(n)])
        secc_img = ((secc_img + 1) * 127.5).permute(0, 2, 3, 1).int()
        d = F.interpolate(depth[:n], (S, S)).repeat([1, 3, 1, 1])
        d = (d - d.min()) / (d.max() - d.min())
        d = (d * 2 - 1).clamp(-1, 1)
        secc_img = (secc_img.double() / 127.5 - 1).permute(0, 3, 1, 2)
        strip = torch.cat([ref.repeat([n, 1, 1, 1]), secc_img, F.interpolate(raw[:n], (S, S)), d, img[:n]], dim=-1).clamp(-1, 1)
        return ((strip.permute(0, 2, 3, 1) + 1) / 2 * 255).int().to(torch.uint8)

    def host_reference(n):
        return R.concat_debug(ref.cpu(), secc[:n].cpu(), raw[:n].cpu(), depth[:n].cpu(), img[:n].cpu())

    hip_range = lambda: V.depth_range(depth, state, reset=True)
    hip_compose = lambda: V.compose_debug_frames(ref, secc, raw, depth, img, depth_range=state, out=out)

    def hip_kernels():
        hip_range()
        hip_compose()

    def hip_kernels_and_copy():
        hip_kernels()
        host_out.copy_(out)

    def by_events(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / calls

    def by_host_clock(fn, calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / calls * 1e3

    # the three routes give the same bytes
    hip_kernels()
    on_device = torch_device(T)
    same_device = bool(torch.equal(out, on_device))
    differing = [int((out[:, :, p * S:(p + 1) * S] != on_device[:, :, p * S:(p + 1) * S]).sum()) for p in range(5)]
    del on_device
    same_host = bool(np.array_equal(V.compose_debug_frames(ref, secc[:a.host_frames], raw[:a.host_frames], depth[:a.host_frames],
                                                           img[:a.host_frames]).cpu().numpy(), host_reference(a.host_frames)))
    routes = {"hip_range": (hip_range, by_events, a.calls), "hip_compose": (hip_compose, by_events, a.calls),
              "hip_kernels": (hip_kernels, by_events, a.calls), "hip_kernels_and_copy": (hip_kernels_and_copy, by_host_clock, a.calls),
              "torch_device": (lambda: torch_device(T), by_host_clock, max(1, a.calls // 5)),
              "host_reference": (lambda: host_reference(a.host_frames), by_host_clock, 1)}
    # the composer one panel at a time: which panel's arithmetic or gather costs what (each writes a fifth of the output)
    srcs = (ref, secc, raw, depth, img)
    for p in range(5):
        args = [x if i == p else None for i, x in enumerate(srcs)]
        routes["hip_compose_panel_%d" % p] = (lambda args=args, p=p: V._compose(*args, T, S, S, 1 << p, state if p == 3 else None, out), by_events, a.calls)
    for k, (fn, timer, calls) in routes.items():          # warm-up: code objects, the allocator's blocks, the pinned buffer
        if k != "host_reference":
            timer(fn, 2)
    samples = {k: [] for k in routes}
    for b in range(a.blocks):                               # alternating blocks
        for k, (fn, timer, calls) in routes.items():
            if k != "host_reference" or b < 2:
                samples[k].append(timer(fn, calls))
    read = 4 * (ref.numel() + secc.numel() + raw.numel() + depth.numel() + img.numel())
    result = {"unit": "ms per call", "frames": T, "size": S, "calls": a.calls, "blocks": a.blocks, "host_frames": a.host_frames,
              "device": torch.cuda.get_device_name(0), "bytes_equal_hip_vs_torch_device": same_device,
              "bytes_differing_hip_vs_torch_device_per_panel": differing, "bytes_equal_hip_vs_host_reference_first_frames": same_host,
              "compose_bytes_read": read, "compose_bytes_written": out.numel(), "range_bytes_read": 4 * depth.numel()}
    result.update({k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in samples.items()})
    rate = (read + out.numel()) / (result["hip_compose"]["median"] * 1e-3)
    result["compose_bytes_per_s"] = rate
    result["compose_fraction_of_float4_copy"] = rate / FLOAT4_COPY_BYTES_PER_S
    result["range_bytes_per_s"] = 4 * depth.numel() / (result["hip_range"]["median"] * 1e-3)
    result["host_reference_ms_per_frame"] = result["host_reference"]["median"] / a.host_frames
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "prof_video_frames.json"), "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
