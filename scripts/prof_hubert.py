"""Time the HuBERT feature extractor (real3dportrait_amd/hubert.py) at the HuBERT-large widths with all 24 layers on
synthetic weights, for a 10 s and a 20 s clip (160 080 and 320 080 samples: 500 and 1 000 frames, one chunk each), and print one JSON line:
  * hubert_features on the HIP library and the same math as eager fp32 torch on the same GPU (tests/hubert_ref64.py in float32), in
    alternating blocks of one run, ms per clip from device events;
  * every library launch of one clip timed on its own (the recorded calls replayed in order, two events around each), summed per launch
    family, with the family's FLOPs and its share of the fp32-matrix floor (FLOPs / 157 TFLOP/s);
  * the largest difference between the two routes, and each one's distance from the fp64 restatement (--no-fp64 skips it).
The weights are drawn on the device (fan-in-scaled normals as synth.synth_hubert scales them); transformers is not imported.
    python scripts/prof_hubert.py [--calls 1] [--blocks 5] [--out profiles/hubert]"""
import math
import statistics

import _prof

_prof.paths(tests=True)

PEAK_F32_MATRIX = 157e12          # FLOP/s (MI355X, v_mfma_f32_*_f32)


def flops(name, a):
    """FLOPs (2 per multiply-add) of one recorded library call, from its marshalled arguments."""
    if name == "r3d_secc_linear":
        return 2.0 * a[1] * a[2] * a[8]
    if name == "r3d_i2p_attention":
        return 4.0 * a[2] * a[3] * a[4] * a[5]
    if name == "r3d_hubert_conv0":
        B, n, C0, k, stride = a[2], a[5], a[11], a[12], a[13]
        return 2.0 * B * ((n - k) // stride + 1) * C0 * k
    if name == "r3d_hubert_conv_ln_gelu":
        B, Tin, Cin, Cout, k, stride = a[6:12]
        return 2.0 * B * ((Tin - k) // stride + 1) * Cout * k * Cin
    if name == "r3d_hubert_pos_conv":
        B, T, C, k, groups = a[3:8]
        return 2.0 * B * T * C * k * (C // groups)
    return 0.0


def family(name, a):
    """The launch family of a call: the entry point, split where one entry point serves very different shapes."""
    if name == "r3d_secc_linear":
        return "linear K=%d N=%d" % (a[2], a[8])
    if name == "r3d_hubert_conv_ln_gelu":
        return "conv_ln_gelu k%d Tin=%d" % (a[10], a[7])
    return name[4:]


def synthetic_weights(torch, dev, seed=86):
    from real3dportrait_amd import synth
    g = torch.Generator(device=dev).manual_seed(seed)
    sd = {}
    for key, shape in synth.hubert_shapes():
        n = torch.randn(shape, generator=g, device=dev, dtype=torch.float32)
        if key == "masked_spec_embed":
            v = n
        elif key.endswith("original0"):
            v = n.abs() + 0.5
        elif key.endswith(".bias"):
            v = 0.1 * n
        elif len(shape) == 1:
            v = 1.0 + 0.1 * n
        else:
            gelu_fed = "conv" in key or "intermediate_dense" in key
            v = n * math.sqrt((2.0 if gelu_fed else 1.0) / math.prod(shape[1:])) * (2.0 if "q_proj" in key or "k_proj" in key else 1.0)
        sd[key] = v
    return sd


def main():
    ap = _prof.parser(__doc__, calls=1, blocks=5)
    ap.add_argument("--rounds", type=int, default=3, help="replays of the recorded launches for the per-family times")
    ap.add_argument("--no-fp64", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch

    import hubert_common as common
    import hubert_ref64 as R64
    from real3dportrait_amd import _lib, synth
    from real3dportrait_amd.hubert import HubertFeatureModel, chunk_plan, hubert_features

    dev = "cuda:0"
    cfg = dict(synth.HUBERT_LARGE)
    with torch.no_grad():
        sd = synthetic_weights(torch, dev)
        m = HubertFeatureModel()
        m.load_state_dict(sd, strict=True)
        m = m.to(dev).eval()
        result = {"metric": "hubert_large_features", "layers": cfg["num_hidden_layers"], "hidden": cfg["hidden_size"], "clips": {}}
        lib = _lib.load()
        for tag, n in (("10s", 160080), ("20s", 320080)):
            wave = torch.from_numpy(common.waveform(87, n).astype(np.float32)).to(dev)
            plan = chunk_plan(n)
            hip = lambda: hubert_features(m, wave)
            eager = lambda: R64.features(sd, cfg, wave, plan, torch.float32)[0]
            samples = _prof.alternate({"hip": _prof.route(hip, _prof.block_median, a.calls), "eager_fp32_torch": _prof.route(eager, _prof.block_median, a.calls)},
                                      a.blocks, warmup=1)
            r = {"samples": n, "frames": (n - 80) // 320, "chunks": [list(c) for c in plan]}
            r.update({k: _prof.ms_spread(v, keep_blocks=True) for k, v in samples.items()})
            r["eager_over_hip"] = round(r["eager_fp32_torch"]["ms"] / r["hip"]["ms"], 3)

            # every launch on its own
            with _lib.counting() as calls:
                out = hip()
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
            r["families"] = dict(sorted(fam.items(), key=lambda kv: -kv[1]["ms"]))
            r["launches"] = len(calls)
            r["sum_of_launches_ms"] = round(total_ms, 4)
            r["gflop"] = round(total_gflop, 1)
            r["floor_ms"] = round(total_gflop * 1e9 / PEAK_F32_MATRIX * 1e3, 4)
            r["share_of_floor"] = round(r["floor_ms"] / r["hip"]["ms"], 4)

            e = eager()
            r["hip_vs_eager_max_diff_of_max"] = float((out - e).abs().max()) / float(e.abs().max())
            if not a.no_fp64:
                ref = R64.features(sd, cfg, wave, plan, torch.float64)[0]
                top = float(ref.abs().max())
                r["hip_vs_fp64_max_diff_of_max"] = float((out.double() - ref).abs().max()) / top
                r["eager_vs_fp64_max_diff_of_max"] = float((e.double() - ref).abs().max()) / top
                del ref
            result["clips"][tag] = r
    _prof.emit(result, a.out, "prof_hubert")


if __name__ == "__main__":
    main()
