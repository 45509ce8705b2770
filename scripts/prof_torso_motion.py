"""Time the torso network's motion-field estimator at B = 1 and the product shapes (K = 4 keypoints, a 16 x 64 x 64 feature
volume, a 256^2 head image) and print one JSON line:

  * the HIP module (real3dportrait_amd/torso_motion.py) against eager fp32 torch of the same math on the same GPU in the same run:
    tests/torso_motion_ref64.py evaluated in float32 (F.conv3d, F.grid_sample's arithmetic spelt out, torch.linalg.inv).  Device events
    around every call, `calls` calls per block, the two sides alternated for `blocks` blocks each after a warm-up; reported: the median of
    the block medians and the spread (max - min) of the block medians, in ms.  When one eager call takes longer than 50 ms its blocks are
    shortened to about 10 s each (eager_calls_per_block says to what);
  * kernel launches of the HIP forward (counted at the C entry points);
  * the share of the fp32-matrix floor (208.6 GFLOP / 157.3 TFLOP/s = 1.33 ms) the HIP forward reaches.

    python scripts/prof_torso_motion.py [--calls 200] [--blocks 5] [--out DIR]     (writes DIR/prof_torso_motion.json)
    python scripts/prof_torso_motion.py --forwards 20        only runs that many HIP forwards after a warm-up, for
        rocprofv3 --kernel-trace --stats -d DIR -o motion -- python scripts/prof_torso_motion.py --forwards 20
    python scripts/prof_torso_motion.py --summarise DIR/.../motion_kernel_trace.csv --forwards 20
        the per-launch table of that trace (median over the forwards), with each layer's GFLOP and TFLOP/s
    python scripts/prof_torso_motion.py --precision both [--calls 100] [--blocks 5] [--out DIR]
        the two precision tiers of the convolutions in alternating blocks in one run, no eager side
        (writes DIR/prof_torso_motion_precision.json); --precision bf16x3 with --forwards: that tier's forwards for a trace
"""
import collections
import csv
import statistics

import _prof

_prof.paths(tests=True)

GFLOP, PEAK_TFLOPS = 208.6, 157.3
INPUT_ORDER = ("fs", "kp_s", "kp_d", "Rs", "Rd", "tgt_head_img", "tgt_head_weights")


def layers(K=4):
    """(label, GFLOP at B = 1) of the module's library launches, in launch order (real channel counts, not the padded ones)."""
    vox, cm = 16 * 64 * 64, 5 * (K + 1)
    conv = lambda pos, k3, ci, co: 2e-9 * pos * k3 * ci * co
    out = [("volume_to_cl", 0.0), ("motion input (compress + heatmaps + sample)", 2e-9 * vox * (K + 1) * 8 * 4 * 34)]
    chans = [cm, 64, 128, 256, 512, 1024]
    for i in range(5):
        out.append(("down.%d 3^3 %d->%d @%d^2 + pool" % (i, chans[i], chans[i + 1], 64 >> i), conv(16 * (64 >> i) ** 2, 27, chans[i], chans[i + 1])))
    up = [1024, 512, 256, 128, 64, 32]
    for i in range(5):
        out.append(("up.%d x2 + 3^3 %d->%d @%d^2" % (i, up[i], up[i + 1], 4 << i), conv(16 * (4 << i) ** 2, 27, up[i], up[i + 1])))
    out += [("resize 256->128 (head)", 0.0), ("encoder 7x7 4->32 @128^2", conv(128 * 128, 49, 4, 32))]
    for i in range(3):
        out += [("encoder res.%d conv 0 (prologue)" % i, conv(128 * 128, 9, 32, 32)), ("encoder res.%d conv 1 (+residual)" % i, conv(128 * 128, 9, 32, 32))]
    out += [("resize 128->64 (head features)", 0.0), ("broadcast over depth", 0.0), ("tgt_head_fuser 7^3 %d->32" % (cm + 64), conv(vox, 343, cm + 64, 32)),
            ("mask_conv 7^3 32->%d" % (K + 1), conv(vox, 343, 32, K + 1)), ("deformation (softmax + sum)", 0.0),
            ("occlusion convs 7x7 512->2 (full depth)", conv(64 * 64, 49, 512, 2))]
    return out


def summarise(path, forwards):
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    starts = [i for i, r in enumerate(rows) if "torso_volume_to_cl" in r[2]]
    segs = [rows[starts[i]:starts[i + 1]] for i in range(len(starts) - 1)][-forwards:]
    n = min(len(s) for s in segs)
    assert all(len(s) == len(segs[0]) for s in segs), sorted(set(len(s) for s in segs))
    lab = iter(layers())
    total = 0.0
    print("%-52s %-44s %9s %8s %8s" % ("launch", "kernel", "us", "GFLOP", "TFLOP/s"))
    for p in range(n):
        name = segs[0][p][2]
        us = statistics.median((s[p][1] - s[p][0]) / 1e3 for s in segs)
        total += us
        label, gf = next(lab) if "r3d::" in name else ("(torch)", 0.0)
        short = name.replace("void ", "").split("(")[0][-44:]
        print("%-52s %-44s %9.1f %8.2f %8.1f" % (label, short, us, gf, gf / us * 1e3 if us else 0.0))
    span = statistics.median((s[-1][1] - s[0][0]) / 1e3 for s in segs)
    print("\nsum of kernel durations %.1f us; first start to last end %.1f us; %.1f GFLOP at the %.1f TFLOP/s f32-matrix peak: %.0f us"
          % (total, span, GFLOP, PEAK_TFLOPS, GFLOP / PEAK_TFLOPS * 1e3))


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
    ap.add_argument("--summarise", default=None)
    ap.add_argument("--precision", default="f32", choices=("f32", "bf16x3", "both"))
    a = ap.parse_args()
    if a.summarise:
        return summarise(a.summarise, a.forwards or 20)
    import numpy as np
    import torch

    import torso_motion_ref64 as R
    from real3dportrait_amd import _lib, synth
    from real3dportrait_amd.torso_motion import MotionFieldEstimator

    def count_launches(fn):
        with _lib.counting() as calls:
            fn()
        return dict(collections.Counter(n for n, _ in calls if n.startswith("r3d_torso_") or n == "r3d_resize_bilinear"))

    dev = "cuda:0"
    sd = synth.synth_torso_motion(171, 4)
    def module(precision):
        mod = MotionFieldEstimator(precision=precision)
        mod.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}, strict=True)
        return mod.to(dev).eval()

    m = module("f32" if a.precision == "both" else a.precision)
    inp = synth.synth_torso_motion_inputs(173, 1, 4)
    args = [torch.from_numpy(inp[k]).to(dev) for k in INPUT_ORDER]
    sdd = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in sd.items()}
    hip = lambda: m(*args)
    eager = lambda: R.estimator(sdd, *args, dtype=torch.float32)

    with torch.no_grad():
        if a.forwards:
            for _ in range(5 + a.forwards):
                hip()
            torch.cuda.synchronize()
            return
        if a.precision == "both":
            mb = module("bf16x3")
            fns = {"f32": hip, "bf16x3": lambda: mb(*args)}
            out = {"metric": "torso_motion_b1_k4_precision_tiers", "B": 1, "K": 4, "calls_per_block": a.calls, "blocks": a.blocks}
            out.update(compare_tiers(fns, a.calls, a.blocks))
            out["launches_by_entry_point"] = {t: count_launches(fn) for t, fn in fns.items()}
            out["bf16x3_vs_f32_max_rel_diff_deformation_occ_occ2"] = [float((x - y).abs().max() / y.abs().max()) for x, y in zip(fns["bf16x3"](), hip())]
            return _prof.emit(out, a.out, "prof_torso_motion_precision")
        for _ in range(3):
            hip()
            eager()
        warm_ms = _prof.by_host_clock(eager, 1)
        ecalls = a.calls if warm_ms <= 50.0 else max(5, min(a.calls, int(10000.0 / warm_ms)))
        sides = {"hip": _prof.route(hip, _prof.block_median, a.calls, warmup=7), "eager": _prof.route(eager, _prof.block_median, ecalls)}
        hb, eb = _prof.alternate(sides, a.blocks, warmup=0).values()          # both sides had 3 calls above
        launches = count_launches(hip)
        diffs = [float((x - y).abs().max() / y.abs().max()) for x, y in zip(hip(), eager())]
    h, e = statistics.median(hb), statistics.median(eb)
    out = {"metric": "torso_motion_b1_k4", "B": 1, "K": 4, "calls_per_block": a.calls, "eager_calls_per_block": ecalls, "blocks": a.blocks,
           "hip_ms": round(h, 4), "hip_block_medians_ms": [round(v, 4) for v in hb], "hip_spread_ms": round(max(hb) - min(hb), 4),
           "eager_fp32_torch_ms": round(e, 4), "eager_block_medians_ms": [round(v, 4) for v in eb], "eager_spread_ms": round(max(eb) - min(eb), 4),
           "speedup_vs_eager": round(e / h, 3), "faster_by_more_than_the_spread": bool(e - h > max(max(hb) - min(hb), max(eb) - min(eb))),
           "launches_per_forward": sum(launches.values()), "launches_by_entry_point": launches,
           "fp32_matrix_floor_ms": round(GFLOP / PEAK_TFLOPS, 4), "share_of_floor": round(GFLOP / PEAK_TFLOPS / h, 3),
           "hip_vs_eager_max_rel_diff_deformation_occ_occ2": diffs}
    _prof.emit(out, a.out, "prof_torso_motion")


if __name__ == "__main__":
    main()
