"""Time the HIP Plane2GridModule (real3dportrait_amd/plane2grid.py) alone at the product shape -- N = 1, depth 3, 256 x 256,
32 channels a plane -- and print one JSON line:
  * the HIP module's forward, and the same module as eager fp32 torch on the same GPU (the mock of tests/plane2grid_common.py: GroupNorm,
    ReLU, Conv3d(padding_mode='replicate')), in alternating blocks, ms per call from device events;
  * every library launch of one forward timed on its own (the recorded calls replayed in order, two events around each), per launch, with
    its FLOPs and its share of the fp32-matrix floor (FLOPs / 157 TFLOP/s; 65.2 GFLOP for the two convs);
  * the largest difference of the branch y - x between the two routes at full size, and each one's distance from the fp64 restatement on
    the CPU (--no-fp64 skips it: a minute of CPU time), all of max|y - x|.
    python scripts/prof_plane2grid.py [--calls 5] [--blocks 3] [--out profiles/plane2grid]"""
import statistics

import _prof

_prof.paths(tests=True)

PEAK_F32_MATRIX = 157e12          # FLOP/s (MI355X, v_mfma_f32_*_f32)


def flops(name, a):
    """FLOPs (2 per multiply-add) of one recorded library call, from its marshalled arguments."""
    if name != "r3d_p2g_conv3d":
        return 0.0
    B, D, H, W, Cin, Cout = a[1], a[2], a[3], a[4], a[5], a[10]
    return 2.0 * B * D * H * W * Cout * 27 * Cin


def main():
    ap = _prof.parser(__doc__, calls=5, blocks=3)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--depth", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5, help="replays of the recorded launches for the per-launch times")
    ap.add_argument("--no-fp64", action="store_true")
    a = ap.parse_args()
    import torch

    import plane2grid_common as common
    import plane2grid_ref64 as R64
    from real3dportrait_amd import _lib

    dev, S, D = "cuda:0", a.size, a.depth
    alphas = (0.37, -0.7)[:common.layers_for(D)]
    sd = common.weights(221, D, alphas)
    m = common.hip_module(sd, D, dev)
    mock = common.mock_module(sd, D).to(dev)
    x_np = common.planes(222, 1, D, S, S)
    x = torch.from_numpy(x_np).to(dev)
    with torch.no_grad():
        hip = lambda: m(x)
        eager = lambda: mock(x)
        samples = _prof.alternate({"hip": _prof.route(hip, _prof.block_median, a.calls), "eager_fp32_torch": _prof.route(eager, _prof.block_median, a.calls)},
                                  a.blocks, warmup=2)
        result = {"metric": "plane2grid", "N": 1, "depth": D, "S": S, "channels": common.C}
        result.update({k: _prof.ms_spread(v, keep_blocks=True) for k, v in samples.items()})
        result["eager_over_hip"] = round(result["eager_fp32_torch"]["ms"] / result["hip"]["ms"], 3)

        # every launch on its own
        with _lib.counting() as calls:
            out = hip()
        lib = _lib.load()
        times = [[] for _ in calls]
        for _ in range(a.rounds):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(calls) + 1)]
            ev[0].record()
            for i, (name, args) in enumerate(calls):
                rc = getattr(lib, name)(*args)
                assert rc == 0, (name, rc)
                ev[i + 1].record()
            ev[-1].synchronize()
            for i in range(len(calls)):
                times[i].append(ev[i].elapsed_time(ev[i + 1]))
        launches, total_ms, total_gflop = [], 0.0, 0.0
        for i, ((name, args), t) in enumerate(zip(calls, times)):
            ms, gf = statistics.median(t), flops(name, args) / 1e9
            floor_ms = gf * 1e9 / PEAK_F32_MATRIX * 1e3
            launches.append({"launch": "%d %s" % (i, name[4:]), "ms": round(ms, 4), "ms_min": round(min(t), 4), "ms_max": round(max(t), 4),
                             "gflop": round(gf, 2), "floor_ms": round(floor_ms, 4), "share_of_floor": round(floor_ms / ms, 4) if gf else None})
            total_ms += ms
            total_gflop += gf
        for f in launches:
            f["share_of_total"] = round(f["ms"] / total_ms, 4)
        result["launches"] = launches
        result["sum_of_launches_ms"] = round(total_ms, 4)
        result["gflop"] = round(total_gflop, 1)
        result["floor_ms"] = round(total_gflop * 1e9 / PEAK_F32_MATRIX * 1e3, 4)
        result["share_of_floor"] = round(result["floor_ms"] / result["hip"]["ms"], 4)

        e = eager()
        bmax = float((e - x).abs().max())
        result["max_branch"] = bmax
        result["hip_vs_eager_branch_diff_of_max_branch"] = float(((out - x) - (e - x)).abs().max()) / bmax
        if not a.no_fp64:
            torch.set_num_threads(16)
            ref = R64.forward(sd, torch.from_numpy(x_np), D)[1]["branch"]
            top = float(ref.abs().max())
            result["hip_vs_fp64_branch_diff_of_max_branch"] = float(((out.cpu().double() - x.cpu().double()) - ref).abs().max()) / top
            result["eager_vs_fp64_branch_diff_of_max_branch"] = float(((e.cpu().double() - x.cpu().double()) - ref).abs().max()) / top
    _prof.emit(result, a.out, "prof_plane2grid")


if __name__ == "__main__":
    main()
