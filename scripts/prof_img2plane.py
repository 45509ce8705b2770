"""Time the canonical image-to-plane backbone (Img2PlaneModel without DeepLabV3) at the product shape -- S = 512, B = 1,
standard scale, input mode rgb -- and print one JSON line:
  * the HIP module from feat_low and the assembled input to the planes, and the same math as eager fp32 torch on the same GPU
    (tests/img2plane_ref64.py in float32), in alternating blocks, ms per call from device events;
  * every library launch of one forward timed on its own (the recorded calls replayed in order, two events around each), summed per launch
    family, with the family's FLOPs and its share of the fp32-matrix floor (FLOPs / 157 TFLOP/s);
  * the largest difference between the two routes at full size, and each one's distance from the fp64 restatement (--no-fp64 skips it).
DeepLabV3 is not part of either side: feat_low comes from the tests' stand-in encoder, outside the timed region.
    python scripts/prof_img2plane.py [--calls 5] [--blocks 3] [--out profiles/img2plane]"""
import statistics

import _prof

_prof.paths(tests=True)

PEAK_F32_MATRIX = 157e12          # FLOP/s (MI355X, v_mfma_f32_*_f32)


def flops(name, a):
    """FLOPs (2 per multiply-add) of one recorded library call, from its marshalled arguments."""
    if name == "r3d_secc_linear":
        return 2.0 * a[1] * a[2] * a[8]
    if name == "r3d_secc_conv":
        B, Hin, Win, Cin, Cout, ks, stride, pad = a[1], a[2], a[3], a[4], a[7], a[8], a[9], a[10]
        return 2.0 * B * ((Hin + 2 * pad - ks) // stride + 1) * ((Win + 2 * pad - ks) // stride + 1) * Cout * ks * ks * Cin
    if name == "r3d_torso_conv":
        return 2.0 * a[1] * a[2] * a[3] * a[4] * a[12] * a[13] * a[13]
    if name == "r3d_i2p_attention":
        return 4.0 * a[2] * a[3] * a[4] * a[5]
    return 0.0


def family(name, a):
    """The launch family of a call: the entry point, split where one entry point serves very different shapes."""
    if name == "r3d_secc_linear":
        return "linear M=%d" % a[1]
    if name == "r3d_secc_conv":
        return "strided conv k%d s%d Cin %d" % (a[8], a[9], a[4])
    if name == "r3d_torso_conv":
        return "3x3 conv %dx%d" % (a[2], a[3])
    if name == "r3d_i2p_attention":
        return "attention N=%d L=%d" % (a[3], a[4])
    if name in ("r3d_secc_dwconv_gelu", "r3d_secc_layernorm"):
        return name[9:]
    return "glue (%s)" % name[8:]


def main():
    ap = _prof.parser(__doc__, calls=5, blocks=3)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--scale", default="standard")
    ap.add_argument("--rounds", type=int, default=5, help="replays of the recorded launches for the per-family times")
    ap.add_argument("--no-fp64", action="store_true")
    a = ap.parse_args()
    import torch

    import img2plane_common as common
    import img2plane_ref64 as R64
    from real3dportrait_amd import _lib

    dev, S = "cuda:0", a.size
    sd = common.weights(81, a.scale, 5)
    m = common.hip_model("rgb", a.scale, sd, dev)
    x = torch.from_numpy(common.image(82, 1, S)).to(dev)
    sd_dev = {k: v.to(dev) for k, v in sd.items()}
    with torch.no_grad():
        x_in = m.assemble_input(x).contiguous()
        feat_low = m.low_reso_encoder(x_in).contiguous()
        hip = lambda: m._run(x_in, feat_low)
        eager = lambda: R64.forward(sd_dev, x_in, feat_low, torch.float32)[0]
        samples = _prof.alternate({"hip": _prof.route(hip, _prof.block_median, a.calls), "eager_fp32_torch": _prof.route(eager, _prof.block_median, a.calls)},
                                  a.blocks, warmup=2)
        result = {"metric": "img2plane_without_deeplabv3", "B": 1, "S": S, "scale": a.scale, "mode": "rgb"}
        result.update({k: _prof.ms_spread(v, keep_blocks=True) for k, v in samples.items()})
        result["eager_over_hip"] = round(result["eager_fp32_torch"]["ms"] / result["hip"]["ms"], 3)

        # every launch on its own
        with _lib.counting() as calls:
            planes = hip()
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
        result["hip_vs_eager_max_diff_of_max"] = float((planes - e).abs().max()) / top
        if not a.no_fp64:
            sd64 = {k: v.double() for k, v in sd_dev.items()}
            ref = R64.forward(sd64, x_in, feat_low, torch.float64)[0]
            top = float(ref.abs().max())
            result["hip_vs_fp64_max_diff_of_max"] = float((planes.double() - ref).abs().max()) / top
            result["eager_vs_fp64_max_diff_of_max"] = float((e.double() - ref).abs().max()) / top
    _prof.emit(result, a.out, "prof_img2plane")


if __name__ == "__main__":
    main()
