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
import argparse
import collections
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import torso_ref64 as R  # noqa: E402
from real3dportrait_amd import _lib, synth  # noqa: E402
from real3dportrait_amd.torso_generator import Generator, Occlusion2Predictor  # noqa: E402

GFLOP, PEAK_TFLOPS = 92.5, 157.3


def block_median(fn, calls):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(calls + 1)]
    ev[0].record()
    for i in range(calls):
        fn()
        ev[i + 1].record()
    ev[-1].synchronize()
    return statistics.median(ev[i].elapsed_time(ev[i + 1]) for i in range(calls))


def count_launches(fn):
    with _lib.counting() as calls:
        fn()
    return dict(collections.Counter(n for n, _ in calls if n.startswith("r3d_torso_")))


def compare_tiers(fns, calls, blocks, block_median):
    """fns: {tier: callable}.  The tiers timed in alternating blocks in one run: per tier the median of the block medians, the block
    medians and their spread (max - min), in ms; faster_by_more_than_the_spreads: f32 - bf16x3 exceeds the sum of the two spreads."""
    meds = {t: [] for t in fns}
    for _ in range(blocks):
        for t, fn in fns.items():
            meds[t].append(block_median(fn, calls))
    out = {}
    for t, v in meds.items():
        out[t] = {"ms": round(statistics.median(v), 4), "block_medians_ms": [round(x, 4) for x in v], "spread_ms": round(max(v) - min(v), 4)}
    gain = out["f32"]["ms"] - out["bf16x3"]["ms"]
    out["f32_minus_bf16x3_ms"] = round(gain, 4)
    out["f32_over_bf16x3"] = round(out["f32"]["ms"] / out["bf16x3"]["ms"], 3)
    out["faster_by_more_than_the_spreads"] = bool(gain > out["f32"]["spread_ms"] + out["bf16x3"]["spread_ms"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--forwards", type=int, default=0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--precision", default="f32", choices=("f32", "bf16x3", "both"))
    a = ap.parse_args()
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
            for _ in range(10):
                for fn in fns.values():
                    fn()
            out = {"metric": "torso_generator_b1_64_precision_tiers", "B": 1, "grid": [64, 64], "calls_per_block": a.calls, "blocks": a.blocks}
            out.update(compare_tiers(fns, a.calls, a.blocks, block_median))
            out["launches_by_entry_point"] = {t: count_launches(fn) for t, fn in fns.items()}
            out["bf16x3_vs_f32_max_rel_diff_rgb_hid_occ2"] = [float((x - y).abs().max() / y.abs().max()) for x, y in zip(fns["bf16x3"](), hip())]
            print(json.dumps(out))
            if a.out:
                os.makedirs(a.out, exist_ok=True)
                with open(os.path.join(a.out, "prof_torso_generator_precision.json"), "w") as f:
                    f.write(json.dumps(out, indent=1) + "\n")
            return
        for _ in range(10):
            hip()
            eager()
        hb, eb = [], []
        for _ in range(a.blocks):
            hb.append(block_median(hip, a.calls))
            eb.append(block_median(eager, a.calls))
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
    print(json.dumps(out))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "prof_torso_generator.json"), "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
