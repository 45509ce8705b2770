"""Regenerate the appearance_* golden vectors: the reference's AppearanceFeatureExtractor(in_dim)
(modules/real3d/facev2v_warp/network2.py:16-45) on CPU in fp32, as WarpBasedTorsoModelMediaPipe.forward calls it (model2.py:230), with
the synthetic parameters and inputs of real3dportrait_amd.synth (synth_torso_appearance, synth_torso_appearance_inputs).

Run in the build container only (needs the reference tree):
    R3D_REFERENCE=<reference tree> python tests/golden/make_golden_torso_appearance.py
Inputs and parameters are regenerated from the seeds stored in each file, so the fixtures hold only outputs (the two-sample case on a depth
stride, to stay under the size of the largest fixture) and, in appearance_keys.npz, the reference's state_dict key names.

The conditions under which a passing test means something are asserted here, when the files are written (check_parameters, check_case)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ["R3D_REFERENCE"]          # the reference tree
sys.path.insert(0, REF)
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(REPO, "tests"))

from real3dportrait_amd import synth  # noqa: E402

# name -> (parameter seed, input seed, N, in_dim, H, W, depth stride of the stored output)
CASES = {"appearance_a_r64": (181, 183, 1, 3, 64, 64, 1),
         "appearance_b_n2_r48x80": (182, 184, 2, 5, 48, 80, 2)}       # rgb_alpha input, two different samples, not square
MAX_BYTES = 1014415
TOL = 2e-4                                 # the GPU tests' tolerance, relative to max|ref|


def reference_extractor(sd, in_dim):
    import ref_stubs
    ref_stubs.install()
    from modules.real3d.facev2v_warp.network2 import AppearanceFeatureExtractor
    m = AppearanceFeatureExtractor(in_dim=in_dim).eval()
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}, strict=True)
    return m


def check_parameters(sd):
    for k, v in sd.items():
        if k.endswith("running_mean"):
            p = k[:-12]
            s = sd[p + "weight"] / np.sqrt(sd[p + "running_var"] + 1e-5)
            t = sd[p + "bias"] - v * s
            assert np.all(t != 0.0) and min(np.std(sd[p + n]) for n in ("weight", "bias", "running_mean", "running_var")) > 0.05, k


def check_case(name, sd, x, out):
    import torso_appearance_ref64 as R64
    assert bool(torch.isfinite(out).all()), name
    xt = torch.from_numpy(x)
    parts = {}
    with torch.no_grad():
        o64 = R64.extractor(sd, xt, parts=parts)
        scale = float(o64.abs().max())
        rel = lambda a: float((a.double() - o64).abs().max()) / scale
        assert rel(out) <= 1e-4, (name, rel(out))
        zeroed = parts["relu"]
        assert len(zeroed) == 15 and all(0.2 <= z <= 0.8 for z in zeroed), (name, zeroed)
        shares = [(b / a, a / b) for a, b in parts["branches"]]
        assert len(shares) == 6 and all(min(s) >= 0.1 for s in shares), (name, shares)
        dropped = [min(rel(R64.extractor(sd, xt, drop_block=i)), rel(R64.extractor(sd, xt, drop_residual=i))) for i in range(6)]
        assert min(dropped) > 100 * TOL, (name, dropped)
        padded = [rel(R64.extractor(sd, xt, pad_before_bn=(i, j))) for i in range(6) for j in range(2)]
        assert min(padded) > 10 * TOL, (name, padded)
    if x.shape[0] > 1:
        assert not np.array_equal(x[0], x[1]) and not np.array_equal(out[0].numpy(), out[1].numpy()), name
    print("%s: max|out| %.2f; the 15 ReLUs zero %s %% of their inputs; rms(branch) / rms(x) per ResBlock3D %s; dropping a block or its "
          "residual moves the output by at least %.2e, padding before BatchNorm by at least %.2e (tolerance %.0e, all relative to max|out|); "
          "reference fp32 vs fp64 restatement %.2e"
          % (name, scale, ["%.0f" % (100 * z) for z in zeroed], ["%.2f" % s[0] for s in shares], min(dropped), min(padded), TOL, rel(out)))


def main():
    torch.set_num_threads(16)
    keys = None
    for name, (sp, sx, N, in_dim, H, W, sdz) in CASES.items():
        sd = synth.synth_torso_appearance(sp, in_dim)
        check_parameters(sd)
        m = reference_extractor(sd, in_dim)
        keys = np.array(list(m.state_dict().keys()))
        x = synth.synth_torso_appearance_inputs(sx, N, in_dim, H, W)["x"]
        with torch.no_grad():
            out = m(torch.from_numpy(x))
        assert out.shape == (N, 32, 16, H // 4, W // 4)
        check_case(name, sd, x, out)
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, spec=np.array([sp, sx, N, in_dim, H, W], np.int64), strides=np.array([sdz], np.int64),
                            out=out[:, :, ::sdz].numpy())
        assert os.path.getsize(path) <= MAX_BYTES, (name, os.path.getsize(path))
        print("   ", name, os.path.getsize(path), "bytes")
    assert keys is not None and len(keys) == 107
    np.savez_compressed(os.path.join(HERE, "appearance_keys.npz"), extractor=keys)


if __name__ == "__main__":
    main()
