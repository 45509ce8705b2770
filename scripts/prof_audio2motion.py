"""Time the HIP audio-to-motion VAE per clip at T = 252 and T = 2500 frames and print one JSON line:

  * PitchContourVAEModel.forward (37 library launches) on synthetic weights and inputs, the latent supplied (z_p=), host wall clock
    around `calls` forwards that end in one synchronise, `blocks` blocks after a warm-up; reported: the median of the block means and
    their minimum and maximum;
  * beside it, in alternating blocks of the same run: eager fp32 torch of the same math on the same GPU, tests/audio2motion_ref64.py
    with dtype float32 on the device (the state_dict uploaded once) -- a restatement of the reference's inference path; the reference's
    own classes are not on the GPU machine;
  * the largest difference of the two outputs, of max|eager|.

    python scripts/prof_audio2motion.py [--calls 20] [--blocks 5] [--frames 252 2500] [--out DIR]
"""
import _prof

_prof.paths(tests=True)


def main():
    ap = _prof.parser(__doc__, calls=20)
    ap.add_argument("--frames", type=int, nargs="+", default=[252, 2500])
    a = ap.parse_args()
    import numpy as np
    import torch

    import audio2motion_ref64 as ref64
    from real3dportrait_amd import audio2motion as a2m
    from real3dportrait_amd import synth

    assert torch.cuda.is_available(), "timings need the GPU"
    dev, hp = "cuda:0", synth.AUDIO2MOTION_HPARAMS
    sd = synth.synth_audio2motion(41, True)
    sd_dev = {k: torch.from_numpy(np.asarray(v)).to(dev) for k, v in sd.items()}
    model = a2m.PitchContourVAEModel(hp)
    model.load_state_dict({k: v.cpu() for k, v in sd_dev.items()}, strict=True)
    model = model.to(dev).eval()

    def timed(fn):          # warm-up: code objects, the folds, the work buffers, the allocator's blocks
        return _prof.route(fn, _prof.by_host_clock, a.calls, warmup=3)

    result = {"unit": "ms per forward", "calls": a.calls, "blocks": a.blocks, "device": torch.cuda.get_device_name(0),
              "launches": a2m.LAUNCHES_PITCH}
    for T in a.frames:
        batch = {k: torch.from_numpy(v).to(dev) for k, v in synth.synth_audio2motion_inputs(7, 1, T).items()}
        z_p = torch.from_numpy(synth.hash_unitvar(8, (1, 16, T // 4))).to(dev)
        hip = lambda: model.forward(batch, {}, z_p=z_p)
        with torch.no_grad():
            eager = lambda: ref64.forward(sd_dev, batch, z_p, True, hp, torch.float32)
            ref = eager()
            diff = float((hip() - ref).abs().max() / ref.abs().max())
            samples = _prof.alternate({"hip": timed(hip), "eager_torch_fp32": timed(eager)}, a.blocks, warmup=0)
        result["T%d" % T] = dict({k: _prof.median_min_max(v) for k, v in samples.items()}, max_diff_hip_vs_eager_of_max=diff)
    _prof.emit(result, a.out, "prof_audio2motion")


if __name__ == "__main__":
    main()
