"""Time the HIP DeepLabV3 (real3dportrait_amd/deeplabv3.py) alone at the product shape -- S = 512, B = 1, in_channels 5,
resnet34 -- and print one JSON line:
  * the HIP module's forward_cl, and the same math as eager fp32 torch on the same GPU (tests/deeplabv3_ref64.py in float32, NCHW), in
    alternating blocks, ms per call from device events;
  * every library launch of one forward timed on its own (the recorded calls replayed in order, two events around each), summed per launch
    family, with the family's FLOPs and its share of the fp32-matrix floor (FLOPs / 157 TFLOP/s);
  * the largest difference between the two routes at full size, and each one's distance from the fp64 restatement (--no-fp64 skips it).
    python scripts/prof_deeplabv3.py [--calls 5] [--blocks 3] [--out profiles/deeplabv3]"""
import statistics

import _prof

_prof.paths(tests=True)

PEAK_F32_MATRIX = 157e12          # FLOP/s (MI355X, v_mfma_f32_*_f32)


def out_size(n, k, s, d, p):
    return (n + 2 * p - d * (k - 1) - 1) // s + 1


def flops(name, a):
    """FLOPs (2 per multiply-add) of one recorded library call, from its marshalled arguments."""
    if name != "r3d_dl_conv":
        return 0.0
    B, H, W, Cin, Cout, k, s, d, p = a[1], a[2], a[3], a[4], a[8], a[9], a[10], a[11], a[12]
    return 2.0 * B * out_size(H, k, s, d, p) * out_size(W, k, s, d, p) * Cout * k * k * Cin


def family(name, a):
    """The launch family of a call: r3d_dl_conv by kernel size, stride, dilation and channels."""
    if name == "r3d_dl_conv":
        return "conv k%d s%d d%d %d->%d on %dx%d" % (a[9], a[10], a[11], a[4], a[8], a[2], a[3])
    return "glue (%s)" % name[4:]


def main():
    ap = _prof.parser(__doc__, calls=5, blocks=3)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=5, help="replays of the recorded launches for the per-family times")
    ap.add_argument("--no-fp64", action="store_true")
    a = ap.parse_args()
    import torch

    import deeplabv3_common as common
    import deeplabv3_ref64 as R64
    from real3dportrait_amd import _lib

    dev, S, cin, enc = "cuda:0", a.size, 5, "resnet34"
    sd = common.weights(97, cin, enc)
    m = common.hip_model(sd, cin, dev, enc)
    x = torch.from_numpy(common.image(98, 1, S, cin)).to(dev)
    sd_dev = {k: v.to(dev) for k, v in sd.items()}
    with torch.no_grad():
        x_cl = x.permute(0, 2, 3, 1).contiguous()
        hip = lambda: m.forward_cl(x_cl)
        eager = lambda: R64.forward(sd_dev, x, torch.float32, enc)[0]
        samples = _prof.alternate({"hip": _prof.route(hip, _prof.block_median, a.calls), "eager_fp32_torch": _prof.route(eager, _prof.block_median, a.calls)},
                                  a.blocks, warmup=2)
        result = {"metric": "deeplabv3", "B": 1, "S": S, "encoder": enc, "in_channels": cin}
        result.update({k: _prof.ms_spread(v, keep_blocks=True) for k, v in samples.items()})
        result["eager_over_hip"] = round(result["eager_fp32_torch"]["ms"] / result["hip"]["ms"], 3)

        # every launch on its own
        with _lib.counting() as calls:
            out = hip().permute(0, 3, 1, 2).contiguous()
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
        fam = {}
        for (name, args), t in zip(calls, times):
            f = fam.setdefault(family(name, args), {"launches": 0, "ms": 0.0, "gflop": 0.0})
            f["launches"] += 1
            f["ms"] += statistics.median(t)
            f["gflop"] += flops(name, args) / 1e9
        total_ms, total_gflop = sum(f["ms"] for f in fam.values()), sum(f["gflop"] for f in fam.values())
        for f in fam.values():
            floor_ms = f["gflop"] * 1e9 / PEAK_F32_MATRIX * 1e3
            f.update(ms=round(f["ms"], 4), gflop=round(f["gflop"], 2), share_of_total=round(f["ms"] / total_ms, 4),
                     floor_ms=round(floor_ms, 4), share_of_floor=round(floor_ms / f["ms"], 4) if f["gflop"] else None)
        result["families"] = dict(sorted(fam.items(), key=lambda kv: -kv[1]["ms"]))
        result["launches"] = len(calls)
        result["sum_of_launches_ms"] = round(total_ms, 4)
        result["gflop"] = round(total_gflop, 1)
        result["floor_ms"] = round(total_gflop * 1e9 / PEAK_F32_MATRIX * 1e3, 4)
        result["share_of_floor"] = round(result["floor_ms"] / result["hip"]["ms"], 4)

        e = eager()
        top = float(e.abs().max())
        result["hip_vs_eager_max_diff_of_max"] = float((out - e).abs().max()) / top
        if not a.no_fp64:
            ref = R64.forward(sd_dev, x, torch.float64, enc)[0]
            top = float(ref.abs().max())
            result["hip_vs_fp64_max_diff_of_max"] = float((out.double() - ref).abs().max()) / top
            result["eager_vs_fp64_max_diff_of_max"] = float((e.double() - ref).abs().max()) / top
    _prof.emit(result, a.out, "prof_deeplabv3")


if __name__ == "__main__":
    main()
