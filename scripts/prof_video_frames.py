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
import _prof

_prof.paths(tests=True)
FLOAT4_COPY_BYTES_PER_S = 6.29e12          # the measured rate of a float4 copy on the MI355X


def main():
    ap = _prof.parser(__doc__, calls=10)
    ap.add_argument("--frames", type=int, default=250)
    ap.add_argument("--host-frames", type=int, default=50)
    ap.add_argument("--size", type=int, default=512)
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

    # the three routes give the same bytes
    hip_kernels()
    on_device = torch_device(T)
    same_device = bool(torch.equal(out, on_device))
    differing = [int((out[:, :, p * S:(p + 1) * S] != on_device[:, :, p * S:(p + 1) * S]).sum()) for p in range(5)]
    del on_device
    same_host = bool(np.array_equal(V.compose_debug_frames(ref, secc[:a.host_frames], raw[:a.host_frames], depth[:a.host_frames],
                                                           img[:a.host_frames]).cpu().numpy(), host_reference(a.host_frames)))
    route, by_events, by_host_clock = _prof.route, _prof.by_events, _prof.by_host_clock
    routes = {"hip_range": route(hip_range, by_events, a.calls), "hip_compose": route(hip_compose, by_events, a.calls),
              "hip_kernels": route(hip_kernels, by_events, a.calls), "hip_kernels_and_copy": route(hip_kernels_and_copy, by_host_clock, a.calls),
              "torch_device": route(lambda: torch_device(T), by_host_clock, max(1, a.calls // 5)),
              "host_reference": route(lambda: host_reference(a.host_frames), by_host_clock, 1, warmup=0, blocks=2)}      # seconds per call
    # the composer one panel at a time: which panel's arithmetic or gather costs what (each writes a fifth of the output)
    srcs = (ref, secc, raw, depth, img)
    for p in range(5):
        args = [x if i == p else None for i, x in enumerate(srcs)]
        routes["hip_compose_panel_%d" % p] = route(lambda args=args, p=p: V._compose(*args, T, S, S, 1 << p, state if p == 3 else None, out), by_events, a.calls)
    samples = _prof.alternate(routes, a.blocks, warmup=2)          # warm-up: code objects, the allocator's blocks, the pinned buffer
    read = 4 * (ref.numel() + secc.numel() + raw.numel() + depth.numel() + img.numel())
    result = {"unit": "ms per call", "frames": T, "size": S, "calls": a.calls, "blocks": a.blocks, "host_frames": a.host_frames,
              "device": torch.cuda.get_device_name(0), "bytes_equal_hip_vs_torch_device": same_device,
              "bytes_differing_hip_vs_torch_device_per_panel": differing, "bytes_equal_hip_vs_host_reference_first_frames": same_host,
              "compose_bytes_read": read, "compose_bytes_written": out.numel(), "range_bytes_read": 4 * depth.numel()}
    result.update({k: _prof.median_min_max(v) for k, v in samples.items()})
    rate = (read + out.numel()) / (result["hip_compose"]["median"] * 1e-3)
    result["compose_bytes_per_s"] = rate
    result["compose_fraction_of_float4_copy"] = rate / FLOAT4_COPY_BYTES_PER_S
    result["range_bytes_per_s"] = 4 * depth.numel() / (result["hip_range"]["median"] * 1e-3)
    result["host_reference_ms_per_frame"] = result["host_reference"]["median"] / a.host_frames
    _prof.emit(result, a.out, "prof_video_frames")


if __name__ == "__main__":
    main()
