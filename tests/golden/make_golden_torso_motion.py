"""Regenerate the motion_* golden vectors: the reference's MotionFieldEstimator('standard', input_channels=34, num_keypoints=K)
(modules/real3d/facev2v_warp/network2.py:162-244) on CPU in fp32, as WarpBasedTorsoModelMediaPipe.forward calls it (model2.py:250), with
the synthetic parameters and inputs of real3dportrait_amd.synth (synth_torso_motion, synth_torso_motion_inputs).

Run in the build container only (needs the reference tree):
    R3D_REFERENCE=<reference tree> python tests/golden/make_golden_torso_motion.py
The reference's func_utils.py calls .cuda() on the grids it builds; this script makes Tensor.cuda the identity for its own process.
Inputs and parameters are regenerated from the seeds stored in each file, so the fixtures hold only outputs (the deformation of the
two-sample case and the mask on strides, to stay under the size of the largest fixture) and, in motion_keys.npz, the reference's
state_dict key names.

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

# name -> (parameter seed, input seed, N, K, rotate, (deformation depth stride, mask space stride))
CASES = {"motion_a_k4": (171, 173, 1, 4, 0, (1, 4)),            # the product
         "motion_b_n2_k4": (171, 174, 2, 4, 0, (2, 4)),         # two different samples
         "motion_c_k9_rot": (172, 175, 1, 9, 1, (1, 4))}        # nine keypoints, Rs and Rd not the identity
MAX_BYTES = 1014415
INPUT_ORDER = ("fs", "kp_s", "kp_d", "Rs", "Rd", "tgt_head_img", "tgt_head_weights")


def reference_estimator(sd, K):
    import ref_stubs
    ref_stubs.install()
    torch.Tensor.cuda = lambda self, *a, **k: self              # func_utils.py:79-103,144: grids are built with .cuda()
    from modules.real3d.facev2v_warp.network2 import MotionFieldEstimator
    m = MotionFieldEstimator("standard", input_channels=34, num_keypoints=K).eval()
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}, strict=True)
    return m


def check_parameters(sd):
    for k, v in sd.items():
        if k.endswith("running_mean"):
            p = k[:-12]
            s = sd[p + "weight"] / np.sqrt(sd[p + "running_var"] + 1e-5)
            t = sd[p + "bias"] - v * s
            assert np.all(t != 0.0) and min(np.std(sd[p + n]) for n in ("weight", "bias", "running_mean", "running_var")) > 0.05, k


def check_case(name, sd, inp, K, deformation, occ, occ2, mask):
    import torso_motion_ref64 as R64
    T = {k: torch.from_numpy(v) for k, v in inp.items()}
    for k in ("kp_s", "kp_d"):
        assert float(np.abs(inp[k]).max()) < 1.0, (name, k)
    for t in (deformation, occ, occ2, mask):
        assert bool(torch.isfinite(t).all()), name
    parts = {}
    with torch.no_grad():
        d64, o64, o264 = R64.estimator(sd, *[T[k] for k in INPUT_ORDER], parts=parts)
        heat = float(parts["input"][:, ::5].abs().max())
        assert heat >= 0.5, (name, heat)
        sm = parts["sparse_motions"][:, 1:]
        out = float((sm.abs() > 1.0).any(-1).double().mean())
        assert 0.05 <= out <= 0.40, (name, out)
        for c in range(3):
            assert bool((sm[..., c] < -1.0).any()) and bool((sm[..., c] > 1.0).any()), (name, c)
        lead = [float((mask.argmax(1) == k).double().mean()) for k in range(K + 1)]
        assert min(lead) >= 0.01, (name, lead)
        top = mask.max(1).values
        decided, open_ = float((top > 0.9).double().mean()), float((top < 0.6).double().mean())
        assert decided >= 0.01 and open_ >= 0.01, (name, decided, open_)
        mid = [float(((o > 0.05) & (o < 0.95)).double().mean()) for o in (occ, occ2)]
        assert min(mid) >= 0.5 and float((occ - occ2).abs().max()) > 0.05, (name, mid)
        rms = float(parts["fused"].pow(2).mean().sqrt())
        shares = []
        for gi in range(3):
            p2 = {}
            R64.estimator(sd, *[T[k] for k in INPUT_ORDER], zero_group=gi, parts=p2)
            shares.append(float((parts["fused"] - p2["fused"]).pow(2).mean().sqrt()) / rms)
        assert min(shares) >= 0.05, (name, shares)
    if inp["fs"].shape[0] > 1:
        assert all(not np.array_equal(v[0], v[1]) for k, v in inp.items() if k not in ("Rs", "Rd")), name
        assert not np.array_equal(deformation[0].numpy(), deformation[1].numpy())
    rel = lambda a, b: float((a.double() - b).abs().max() / b.abs().max())
    print("%s: max|heatmap| %.2f, %.1f %% of the sparse-motion points outside, each mask component leads on %s %%, top weight > 0.9 on "
          "%.0f %% and < 0.6 on %.0f %%, occlusions in (0.05, 0.95) on %.0f / %.0f %%, group shares of the fuser's output %s; reference "
          "fp32 vs fp64 restatement: deformation %.2e occlusion %.2e occlusion_2 %.2e mask %.2e"
          % (name, heat, 100 * out, ["%.1f" % (100 * v) for v in lead], 100 * decided, 100 * open_, 100 * mid[0], 100 * mid[1],
             ["%.2f" % s for s in shares], rel(deformation, d64), rel(occ, o64), rel(occ2, o264), rel(mask, parts["mask"])))


def main():
    torch.set_num_threads(16)
    models, keys = {}, None
    for name, (sp, sx, N, K, rot, (sdz, sm)) in CASES.items():
        sd = synth.synth_torso_motion(sp, K)
        if (sp, K) not in models:
            check_parameters(sd)
            models[(sp, K)] = reference_estimator(sd, K)
        m = models[(sp, K)]
        if K == 4:
            keys = np.array(list(m.state_dict().keys()))
        inp = synth.synth_torso_motion_inputs(sx, N, K, rotate=bool(rot))
        captured = {}
        hook = m.mask_conv.register_forward_hook(lambda mod, i, o: captured.update(mask=torch.softmax(o, dim=1)))
        with torch.no_grad():
            deformation, occ, occ2 = m(*[torch.from_numpy(inp[k]) for k in INPUT_ORDER])
        hook.remove()
        mask = captured["mask"]
        assert deformation.shape == (N, 16, 64, 64, 3) and occ.shape == (N, 1, 64, 64) and occ2.shape == (N, 1, 64, 64)
        check_case(name, sd, inp, K, deformation, occ, occ2, mask)
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, spec=np.array([sp, sx, N, K, rot], np.int64), strides=np.array([sdz, sm], np.int64),
                            deformation=deformation[:, ::sdz].numpy(), occlusion=occ.numpy(), occlusion_2=occ2.numpy(),
                            mask=mask[:, :, ::sm, ::sm, ::sm].numpy())
        assert os.path.getsize(path) <= MAX_BYTES, (name, os.path.getsize(path))
        print("   ", name, os.path.getsize(path), "bytes")
    assert keys is not None and len(keys) == 129
    np.savez_compressed(os.path.join(HERE, "motion_keys.npz"), estimator=keys)


if __name__ == "__main__":
    main()
