"""Time the torso network's appearance feature extractor at B = 1 and the product shape (in_dim 5, a 256^2 image) and
print one JSON line:

  * the HIP module (real3dportrait_amd/torso_appearance.py), on both precision tiers, against eager fp32 torch of the same math on the
    same GPU in the same run: tests/torso_appearance_ref64.py evaluated in float32 (F.conv2d, F.conv3d, F.batch_norm).  Device events
    around every call, `calls` calls per block, the three sides alternated for `blocks` blocks each after a warm-up; reported: the median
    of the block medians and the spread (max - min) of the block medians, in ms;
  * kernel launches of the HIP forward (counted at the C entry points);
  * the share of the fp32-matrix floor (65.9 GFLOP / 157.3 TFLOP/s = 0.42 ms) each tier reaches, and the agreement of the sides.

    python scripts/prof_torso_appearance.py [--calls 100] [--blocks 5] [--out DIR]     (writes DIR/prof_torso_appearance.json)
    python scripts/prof_torso_appearance.py --forwards 20 [--precision bf16x3]   only runs that many HIP forwards after a warm-up, for
        rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o appearance -- python scripts/prof_torso_appearance.py --forwards 20
    python scripts/prof_torso_appearance.py --summarise DIR/.../appearance_kernel_trace.csv --forwards 20
        the per-launch table of that trace (median over the forwards), with each layer's GFLOP and TFLOP/s
"""
import collections
import csv
import statistics

import _prof

_prof.paths(tests=True)

PEAK_TFLOPS = 157.3


def layers(in_dim=5, S=256):
    """(label, GFLOP at B = 1) of the module's library launches, in launch order."""
    conv = lambda pos, taps, ci, co: 2e-9 * pos * taps * ci * co
    out = [("in_conv 7x7 %d->64 @%d^2" % (in_dim, S), conv(S * S, 49, in_dim, 64)),
           ("down.0 3x3 64->128 @%d^2 + pool" % S, conv(S * S, 9, 64, 128)),
           ("down.1 3x3 128->256 @%d^2 + pool" % (S // 2), conv(S * S // 4, 9, 128, 256)),
           ("mid_conv 1x1 256->512 @%d^2, depth-split store" % (S // 4), conv(S * S // 16, 1, 256, 512))]
    for i in range(6):
        out += [("res.%d conv 0 3^3 32->32 (prologue)" % i, conv(16 * S * S // 16, 27, 32, 32)),
                ("res.%d conv 1 3^3 32->32 (+residual)" % i, conv(16 * S * S // 16, 27, 32, 32))]
    return out


GFLOP = sum(g for _, g in layers())


def summarise(path, forwards):
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            if "r3d" in r["Kernel_Name"]:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    lab = layers()
    n = len(lab)
    assert len(rows) % n == 0 and len(rows) >= n * forwards, (len(rows), n)
    segs = [rows[i:i + n] for i in range(0, len(rows), n)][-forwards:]
    total = 0.0
    print("%-52s %-44s %9s %8s %8s" % ("launch", "kernel", "us", "GFLOP", "TFLOP/s"))
    for p in range(n):
        name = segs[0][p][2]
        us = statistics.median((s[p][1] - s[p][0]) / 1e3 for s in segs)
        total += us
        label, gf = lab[p]
        short = name.replace("void ", "").split("(")[0][-44:]
        print("%-52s %-44s %9.1f %8.2f %8.1f" % (label, short, us, gf, gf / us * 1e3 if us else 0.0))
    span = statistics.median((s[-1][1] - s[0][0]) / 1e3 for s in segs)
    print("\nsum of kernel durations %.1f us; first start to last end %.1f us; %.1f GFLOP at the %.1f TFLOP/s f32-matrix peak: %.0f us"
          % (total, span, GFLOP, PEAK_TFLOPS, GFLOP / PEAK_TFLOPS * 1e3))


def main():
    ap = _prof.parser(__doc__, calls=100)
    ap.add_argument("--forwards", type=int, default=0)
    ap.add_argument("--summarise", default=None)
    ap.add_argument("--precision", default="f32", choices=("f32", "bf16x3"))
    a = ap.parse_args()
    if a.summarise is not None:
        return summarise(a.summarise, a.forwards or 20)
    import numpy as np
    import torch

    import torso_appearance_ref64 as R
    from real3dportrait_amd import _lib, synth
    from real3dportrait_amd.torso_appearance import AppearanceFeatureExtractor

    def count_launches(fn):
        with _lib.counting() as calls:
            fn()
        return dict(collections.Counter(n for n, _ in calls if n.startswith("r3d_torso_")))

    dev = "cuda:0"
    sd = synth.synth_torso_appearance(181, 5)

    def module(precision):
        mod = AppearanceFeatureExtractor(in_dim=5, precision=precision)
        mod.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}, strict=True)
        return mod.to(dev).eval()

    x = torch.from_numpy(synth.synth_torso_appearance_inputs(183, 1, 5, 256, 256)["x"]).to(dev)
    sdd = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in sd.items()}
    mods = {t: module(t) for t in (("f32", "bf16x3") if not a.forwards else (a.precision,))}
    fns = {t: (lambda m=m: m(x)) for t, m in mods.items()}
    with torch.no_grad():
        if a.forwards:
            for _ in range(5 + a.forwards):
                fns[a.precision]()
            torch.cuda.synchronize()
            return
        fns["eager"] = lambda: R.extractor(sdd, x, dtype=torch.float32)
        meds = _prof.alternate(_prof.routes(fns, _prof.block_median, a.calls), a.blocks, warmup=10)
        launches = {t: count_launches(fns[t]) for t in mods}
        ref = R.extractor(sdd, x)
        rel = lambda y: float((y.double() - ref).abs().max() / ref.abs().max())
        agreement = {t + "_vs_fp64": rel(fn()) for t, fn in fns.items()}
        agreement["f32_vs_eager"] = float((fns["f32"]() - fns["eager"]()).abs().max() / ref.abs().max())
    ms = {t: statistics.median(v) for t, v in meds.items()}
    spread = {t: max(v) - min(v) for t, v in meds.items()}
    floor = GFLOP / PEAK_TFLOPS
    out = {"metric": "torso_appearance_b1_in5_256", "B": 1, "in_dim": 5, "size": 256, "calls_per_block": a.calls, "blocks": a.blocks,
           "gflop": round(GFLOP, 2), "fp32_matrix_floor_ms": round(floor, 4), "shader_clock": "not measured"}
    for t in fns:
        key = "eager_fp32_torch" if t == "eager" else "hip_" + t
        out[key + "_ms"] = round(ms[t], 4)
        out[key + "_block_medians_ms"] = [round(v, 4) for v in meds[t]]
        out[key + "_spread_ms"] = round(spread[t], 4)
    for t in mods:
        out["speedup_vs_eager_" + t] = round(ms["eager"] / ms[t], 3)
        out["faster_than_eager_by_more_than_the_spread_" + t] = bool(ms["eager"] - ms[t] > max(spread[t], spread["eager"]))
        out["share_of_floor_" + t] = round(floor / ms[t], 3)
    out["launches_per_forward"] = {t: sum(c.values()) for t, c in launches.items()}
    out["launches_by_entry_point"] = launches
    out["max_rel_diff"] = agreement
    _prof.emit(out, a.out, "prof_torso_appearance")


if __name__ == "__main__":
    main()
