"""Time the torso generator (Generator + occlusion_2_predictor) at B = 1 and the product size (64^2 feature grid, 256^2
output) and print one JSON line:

  * the HIP modules (real3dportrait_amd/torso_generator.py) against eager fp32 torch of the same math on the same GPU: F.grid_sample,
    then tests/torso_ref64.py in float32, which recomputes weight_orig / sigma per call as the reference's spectral-norm hook does in
    eval mode.  Both sides include the forward tail's F.interpolate + torch.cat in front of the predictor.  Device events around every
    call, `calls` calls per block, the two sides alternated for `blocks` blocks each after a warm-up; reported: the median of the
    block medians and the spread (max - min) of the block medians, in ms;
  * kernel launches of the HIP forward (counted at the C entry points);
  * the share of the fp32-matrix floor (92.5 GFLOP / 157.3 TFLOP/s = 0.588 ms) the HIP forward reaches.

    python scripts/prof_torso_generator.py [--calls 200] [--blocks 5] [--out DIR]     (writes DIR/prof_torso_generator.json)
    python scripts/prof_torso_generator.py --forwards 20        only runs that many HIP forwards after a warm-up, for
        rocprofv3 --kernel-trace --stats -d DIR -o torso -- python scripts/prof_torso_generator.py --forwards 20
    python scripts/prof_torso_generator.py --precision both [--calls 200] [--blocks 5] [--out DIR]
        the two precision tiers of the convolutions in alternating blocks in one run, no eager side
        (writes DIR/prof_torso_generator_precision.json); --precision bf16x3 with --forwards: that tier's forwards for a trace
"""
import collections
import statistics

import _prof

_prof.paths(tests=True)

GFLOP, PEAK_TFLOPS = 92.5, 157.3


def compare_tiers(fns, calls, blocks):
    """fns: {tier: callable}.  The tiers timed in alternating blocks in one run after 10 calls of warm-up: per tier the median of the block
    medians, the block medians and their spread (max - min), in ms; faster_by_more_than_the_spreads: f32 - bf16x3 exceeds the sum of the
    two spreads."""
    samples = _prof.alternate(_prof.routes(fns, _prof.block_median, calls), blocks, warmup=10)
    out = {t: _prof.ms_spread(v, keep_blocks=True) for t, v in samples.items()}
    gain = out["f32"]["ms"] - out["bf16x3"]["ms"]
    out["f32_minus_bf16x3_ms"] = round(gain, 4)
    out["f32_over_bf16x3"] = round(out["f32"]["ms"] / out["bf16x3"]["ms"], 3)
    out["faster_by_more_than_the_spreads"] = bool(gain > out["f32"]["spread_ms"] + out["bf16x3"]["spread_ms"])
    return out


def main():
    ap = _prof.parser(__doc__, calls=200)
    ap.add_argument("--forwards", type=int, default=0)
    ap.add_argument("--precision", default="f32", choices=("f32", "bf16x3", "both"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import torch.nn.functional as F

    import torso_ref64 as R
    from real3dportrait_amd import _lib, synth
    from real3dportrait_amd.torso_generator import Generator, Occlusion2Predictor

    def count_launches(fn):
        with _lib.counting() as calls:
            fn()
        return dict(collections.Counter(n for n, _ in calls if n.startswith("r3d_torso_")))

    dev = "cuda:0"
    T = lambda sd: {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}
    sd, psd = synth.synth_torso_generator(71), synth.synth_torso_predictor(72)
    def modules(precision):
        g, p = Generator(precision=precision), Occlusion2Predictor(precision=precision)
        g.load_state_dict(T(sd), strict=True)
        p.load_state_dict(T(psd), strict=True)
        return g.to(dev).eval(), p.to(dev).eval()

    gen, pred = modules("f32" if a.precision == "both" else a.precision)
    i = {k: torch.from_numpy(v).to(dev) for k, v in synth.synth_torso_inputs(73, 1, 64, 64).items()}
    sdd, psdd = {k: v.to(dev) for k, v in T(sd).items()}, {k: v.to(dev) for k, v in T(psd).items()}
    fs, grid, occ, occ2 = i["torso_appearance_feats"], i["deformation"], i["occlusion"], i["occlusion_2"]

    def hip(gen=gen, pred=pred):
        rgb, hid = gen(fs, grid, occ, return_hid=True)
        return rgb, hid, pred(torch.cat([hid, F.interpolate(occ2, size=(256, 256), mode="bilinear")], dim=1))

    def eager():
        d = F.grid_sample(fs, grid, align_corners=True, padding_mode="border").view(1, -1, 64, 64)
        rgb, hid = R.decoder(sdd, d, torch.float32)
        return rgb, hid, R.predictor(psdd, torch.cat([hid, F.interpolate(occ2, size=(256, 256), mode="bilinear")], dim=1), torch.float32)

    with torch.no_grad():
        if a.forwards:
            for _ in range(5 + a.forwards):
                hip()
            torch.cuda.synchronize()
            return
        if a.precision == "both":
            gb, pb = modules("bf16x3")
            fns = {"f32": hip, "bf16x3": lambda: hip(gb, pb)}
            out = {"metric": "torso_generator_b1_64_precision_tiers", "B": 1, "grid": [64, 64], "calls_per_block": a.calls, "blocks": a.blocks}
            out.update(compare_tiers(fns, a.calls, a.blocks))
            out["launches_by_entry_point"] = {t: count_launches(fn) for t, fn in fns.items()}
            out["bf16x3_vs_f32_max_rel_diff_rgb_hid_occ2"] = [float((x - y).abs().max() / y.abs().max()) for x, y in zip(fns["bf16x3"](), hip())]
            return _prof.emit(out, a.out, "prof_torso_generator_precision")
        hb, eb = _prof.alternate(_prof.routes({"hip": hip, "eager": eager}, _prof.block_median, a.calls), a.blocks, warmup=10).values()
        launches = count_launches(hip)
        diffs = [float((x - y).abs().max() / y.abs().max()) for x, y in zip(hip(), eager())]
    h, e = statistics.median(hb), statistics.median(eb)
    out = {"metric": "torso_generator_b1_64", "B": 1, "grid": [64, 64], "calls_per_block": a.calls, "blocks": a.blocks,
           "hip_ms": round(h, 4), "hip_block_medians_ms": [round(v, 4) for v in hb], "hip_spread_ms": round(max(hb) - min(hb), 4),
           "eager_fp32_torch_ms": round(e, 4), "eager_block_medians_ms": [round(v, 4) for v in eb], "eager_spread_ms": round(max(eb) - min(eb), 4),
           "speedup_vs_eager": round(e / h, 3), "faster_by_more_than_the_spread": bool(e - h > max(max(hb) - min(hb), max(eb) - min(eb))),
           "launches_per_forward": sum(launches.values()), "launches_by_entry_point": launches,
           "fp32_matrix_floor_ms": round(GFLOP / PEAK_TFLOPS, 4), "share_of_floor": round(GFLOP / PEAK_TFLOPS / h, 3),
           "hip_vs_eager_max_rel_diff_rgb_hid_occ2": diffs}
    _prof.emit(out, a.out, "prof_torso_generator")


if __name__ == "__main__":
    main()
