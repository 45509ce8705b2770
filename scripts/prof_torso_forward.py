"""Time one forward of the warp-based torso model at B = 1 and the product shapes (in_dim 5, a 256^2 source image, a
512^2 six-class segmap, 4 key points) and print one JSON line:

  * the HIP forward (real3dportrait_amd/torso_forward.py: patch_model(..., torso_forward=True)) against the parent path on the same GPU
    in the same run: the reference's forward restated in torch (stand_in_torso_model of tests/test_gpu_torso_appearance.py) over the same
    three HIP modules, which is what patch_model gives without the switch.  Device events around every call, `calls` calls per block, the
    two sides alternated for `blocks` blocks each after a warm-up; reported: the median of the block medians and the spread (max - min)
    of the block medians, in ms;
  * the two glue kernels alone, the same way (r3d_torso_seg_input at 512^2 -> 256^2, r3d_torso_mask_volume at 64 x 64 x 16 x 32);
  * library launches of each side (counted at the C entry points) and the agreement of the two sides.

    python scripts/prof_torso_forward.py [--calls 100] [--blocks 5] [--out DIR]     (writes DIR/prof_torso_forward.json)
"""
import collections
import statistics

import _prof

_prof.paths(tests=True)


def main():
    a = _prof.parser(__doc__, calls=100).parse_args()
    import torch

    from test_gpu_torso_appearance import stand_in_torso_model, synth_frame
    from test_torso_generator_host import model_shell
    from real3dportrait_amd import _lib, patch_model, torso_mask_volume, torso_seg_input

    def count_launches(fn):
        with _lib.counting() as calls:
            fn()
        return dict(collections.Counter(n for n, _ in calls if n.startswith("r3d_torso_") or n == "r3d_resize_bilinear"))

    dev = "cuda:0"
    switches = dict(torso_appearance=True, torso_motion=True, torso_generator=True)
    tms = {}
    for side, on in (("hip_forward", True), ("parent_path", False)):
        tm = stand_in_torso_model(251, 252, 253, 254).to(dev)
        tms[side] = patch_model(model_shell(tm).to(dev), torso_forward=on, **switches).superresolution.torso_model
    frame = synth_frame(255)
    fns = {side: (lambda tm=tm: tm.forward(*frame)) for side, tm in tms.items()}
    seg = frame[1]
    feats_cl = torch.randn(1, 16, 64, 64, 32, device=dev)
    masked, motion, x5 = torch.empty_like(feats_cl), torch.empty(1, 16, 64, 64, 34, device=dev), torch.empty(1, 5, 256, 256, device=dev)
    fns["mask_volume_kernel"] = lambda: torso_mask_volume(feats_cl, seg, masked_cl=masked, motion_cl=motion)
    fns["seg_input_kernel"] = lambda: torso_seg_input(frame[0], seg, out=x5)
    with torch.no_grad():
        meds = _prof.alternate(_prof.routes(fns, _prof.block_median, a.calls), a.blocks, warmup=10)
        launches = {t: count_launches(fns[t]) for t in tms}
        (rgb, ret), (rgb_p, ret_p) = fns["hip_forward"](), fns["parent_path"]()
        rel = lambda y, r: float((y.double() - r.double()).abs().max() / r.double().abs().max())
        agreement = {"rgb": rel(rgb, rgb_p), "occlusion": rel(ret["occlusion"], ret_p["occlusion"]),
                     "occlusion_2": rel(ret["occlusion_2"], ret_p["occlusion_2"])}
    ms = {t: statistics.median(v) for t, v in meds.items()}
    spread = {t: max(v) - min(v) for t, v in meds.items()}
    out = {"metric": "torso_forward_b1_in5_256_seg512_kp4", "B": 1, "in_dim": 5, "size": 256, "segmap": 512, "key_points": 4,
           "calls_per_block": a.calls, "blocks": a.blocks, "shader_clock": "not measured"}
    for t in fns:
        out[t + "_ms"] = round(ms[t], 4)
        out[t + "_block_medians_ms"] = [round(v, 4) for v in meds[t]]
        out[t + "_spread_ms"] = round(spread[t], 4)
    diff, noise = ms["parent_path"] - ms["hip_forward"], max(spread["hip_forward"], spread["parent_path"])
    out["parent_minus_hip_ms"] = round(diff, 4)
    out["hip_forward_is"] = "faster by more than the spread" if diff > noise else ("slower by more than the spread" if -diff > noise
                                                                                   else "within the spread of the parent path")
    out["launches_per_forward"] = {t: sum(c.values()) for t, c in launches.items()}
    out["launches_by_entry_point"] = launches
    out["max_rel_diff_hip_vs_parent"] = agreement
    _prof.emit(out, a.out, "prof_torso_forward")


if __name__ == "__main__":
    main()
