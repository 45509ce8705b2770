"""Goldens of the audio-to-motion VAE (real3dportrait_amd/audio2motion.py): the reference's own PitchContourVAEModel and
VAEModel (modules/audio2motion/vae.py:272-454) run on the CPU in fp32 on synthetic weights and inputs.

Run where the reference tree is:   R3D_REFERENCE=<its root> python tests/golden/make_golden_audio2motion.py
Writes tests/golden/audio2motion_<case>.npz: out [B, T, 64] (the reference's x_recon), z_p [B, 16, T / 4] (the latent it drew, which the
same torch.manual_seed draws again) and the seeds; the weights and inputs are synth.synth_audio2motion(model_seed, pitch) and
synth.synth_audio2motion_inputs(input_seed, B, T).  audio2motion_keys.npz holds the reference's state_dict key names of both models.

Before it writes a case the script asserts, on the reference and the fp64 restatement alone (tests/audio2motion_ref64.py), the
conditions under which a passing comparison means something: see check_case.
"""
import os
import sys

import numpy as np
import torch

REF = os.environ.get("R3D_REFERENCE")
if not REF or not os.path.isdir(os.path.join(REF, "modules", "audio2motion")):
    sys.exit("set R3D_REFERENCE to the root of the Real3D-Portrait tree (modules/audio2motion/vae.py is imported from it)")
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REF)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
OUT = os.environ.get("R3D_GOLDEN_OUT") or HERE

import audio2motion_ref64 as ref64  # noqa: E402
from real3dportrait_amd import synth  # noqa: E402
from real3dportrait_amd.audio2motion import WN_ROWS as R  # noqa: E402

TOL = 2e-4          # the tests' tolerance, of max|ref|
MODEL_SEED = 41
# name: (pitch model, B, T, input seed, torch seed)
CASES = {
    "pitch_t4": (True, 1, 4, 101, 7),                       # Tq = 1: every tap of the flows but the centre is padding
    "pitch_b2": (True, 2, R + 4, 102, 8),                   # different samples and mouth_amp, a blink pattern, y_mask with trailing zeros
    "pitch_t2r": (True, 1, 2 * R + 4, 103, 9),
    "pitch_tr": (True, 1, R - 4, 104, 10),
    "vae_t20": (False, 1, 20, 105, 11),
}


def reference_model(pitch, sd):
    from modules.audio2motion.vae import PitchContourVAEModel, VAEModel
    m = PitchContourVAEModel(synth.AUDIO2MOTION_HPARAMS, in_out_dim=64, audio_in_dim=1024) if pitch else VAEModel(in_out_dim=64, audio_in_dim=1024)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return m.eval()


def check_model(sd, pitch):
    """The weights do not hide a missing fold."""
    for k, v in sd.items():
        if k.endswith(("post.weight", "post.bias")):
            assert np.abs(v).min() > 0 or np.abs(v).mean() > 1e-3, k          # the reference initialises them to zero
            assert np.abs(v).max() > 1e-2, k
        if k.endswith("weight_g"):
            n = np.sqrt((sd[k[:-1] + "v"].astype(np.float64) ** 2).sum(axis=(1, 2), keepdims=True))
            assert (np.abs(v / n - 1) > 0.1).all(), k
        if k.endswith("running_mean"):
            assert np.abs(v).max() > 0.1, k
        if k.endswith("running_var"):
            assert np.abs(v - 1).max() > 0.1 and v.min() > 0.1, k


def check_case(name, sd, batch, z_p, out, pitch):
    """The fp64 restatement is the reference; every piece matters; the gates are not saturated; no pitch index is at an edge."""
    hp = synth.AUDIO2MOTION_HPARAMS
    taps = {}
    run = lambda **kw: ref64.forward(sd, batch, z_p, pitch, hp, torch.float64, **kw).numpy()
    x64 = run(taps=taps)
    scale = np.abs(out).max()
    e = np.abs(x64 - out).max() / scale
    assert e <= 1e-4, (name, e)
    drops = [("flow", i) for i in range(4)] + [("cond", "vae.prior_flow.flows.%d.enc" % (2 * i), l) for i in range(4) for l in range(4)]
    drops += [("cond", "vae.decoder.wn", l) for l in range(4)] + ["gain", "flip", "bn"]
    moved = {}
    for d in drops:
        moved[d] = np.abs(run(drop={d}) - x64).max() / scale
        assert moved[d] > 100 * TOL, (name, d, moved[d])
    gates = torch.cat([v.reshape(-1) for k, v in taps.items() if ".gate" in k])
    open_ = float((gates.abs() < 4).double().mean())
    assert open_ >= 0.5, (name, open_)
    if pitch:
        m = taps["f0_mel"].numpy()
        margin = np.abs(m - np.rint(m)).min()
        f0 = batch["f0"][:, 0:2 * batch["y_mask"].shape[1]:2]
        assert margin >= 1e-3 and (f0 == 0).sum(axis=1).min() >= 3 and (f0 > 0).any(), (name, margin)
        assert len(np.unique(taps["pitch_index"].numpy())) >= 2
    print("%-10s ref32 vs fp64 %.2e | least move of a dropped piece %.2e (%s) | open gates %.2f | max|ref| %.3f"
          % (name, e, min(moved.values()), min(moved, key=moved.get), open_, scale))


def main():
    from modules.audio2motion.vae import PitchContourVAEModel, VAEModel
    keys = {}
    for pitch in (True, False):
        m = PitchContourVAEModel(synth.AUDIO2MOTION_HPARAMS, in_out_dim=64, audio_in_dim=1024) if pitch else VAEModel(in_out_dim=64, audio_in_dim=1024)
        keys["pitch" if pitch else "vae"] = np.array(list(m.state_dict().keys()))
    np.savez_compressed(os.path.join(OUT, "audio2motion_keys.npz"), **keys)
    models = {}
    for name, (pitch, B, T, in_seed, t_seed) in CASES.items():
        if pitch not in models:
            sd = synth.synth_audio2motion(MODEL_SEED, pitch)
            check_model(sd, pitch)
            models[pitch] = (sd, reference_model(pitch, sd))
        sd, model = models[pitch]
        batch = synth.synth_audio2motion_inputs(in_seed, B, T)
        if not pitch:
            batch = {k: batch[k] for k in ("audio", "y_mask")}
        torch.manual_seed(t_seed)
        z_p = torch.distributions.Normal(0, 1).sample([B, 16, T // 4])
        torch.manual_seed(t_seed)
        with torch.no_grad():
            ret = {}
            out = model.forward({k: torch.from_numpy(v) for k, v in batch.items()}, ret=ret, train=False, temperature=1.0).numpy()
        assert out.shape == (B, T, 64) and ret["pred"].shape == out.shape
        check_case(name, sd, batch, z_p, out, pitch)
        np.savez_compressed(os.path.join(OUT, "audio2motion_%s.npz" % name), out=out, z_p=z_p.numpy(),
                            seeds=np.array([MODEL_SEED, in_seed, t_seed], np.int64), shape=np.array([int(pitch), B, T], np.int64))


if __name__ == "__main__":
    main()
