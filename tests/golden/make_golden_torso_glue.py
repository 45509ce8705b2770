"""Regenerate the torso_glue_* golden vectors: the reference's own statement of what joins the torso network's modules
(modules/real3d/facev2v_warp/model2.py:226-236) -- its F.interpolate calls, its `dilate` (utils/commons/image_utils.py:10-15), the mask
multiply and the concatenation -- on CPU in fp32, on the synthetic inputs of real3dportrait_amd.synth (synth_torso_glue_inputs).

Run in the build container only (needs the reference tree):
    R3D_REFERENCE=<reference tree> python tests/golden/make_golden_torso_glue.py
Inputs are regenerated from the seed stored in each file, so the fixtures hold only results: the resized pair, the dilated mask, the
estimator's input (whose first C channels are the masked volume), in_conv's rgb_alpha input, and e32, the error of each against the same calls in float64 (the
"reference's own error" of the parity rule, tests/torso_glue_ref64.py:bound)."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ["R3D_REFERENCE"]          # the reference tree
sys.path.insert(0, REF)
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(REPO, "tests"))

from real3dportrait_amd import synth  # noqa: E402

# name -> (seed, N, Cs, Hs, Ws, C, D, h, w, ksize, image H, image W)
CASES = {"torso_glue_down_50x37": (261, 2, 6, 50, 37, 4, 2, 12, 8, 7, 8, 12),          # down-sampling at a non-integer ratio
         "torso_glue_up_3x3": (262, 2, 5, 3, 3, 4, 2, 8, 8, 7, 12, 8)}                   # up-sampling
KEYS = ("seg", "mask_d", "motion", "seg_in")          # the masked volume is motion[:, :C]
MAX_BYTES = 16384


def reference_glue(dilate, feats, segmap, ksize, img):
    """model2.py:226-236 with hparams torso_inp_mode rgb_alpha and mul_torso_mask, line by line, in the dtype of `feats` (the reference's
    segmap.float() for float32)."""
    torso_segmap = F.interpolate(segmap[:, [2, 4]].to(feats.dtype), size=(img.shape[-2], img.shape[-1]), mode="bilinear", align_corners=False, antialias=False)
    seg_in = torch.cat([img, torso_segmap], dim=1)
    torso_segmap = F.interpolate(segmap[:, [2, 4]].to(feats.dtype), size=tuple(feats.shape[-2:]), mode="bilinear", align_corners=False, antialias=False)
    torso_mask = torso_segmap.sum(dim=1).unsqueeze(1)
    torso_mask = dilate(torso_mask, ksize=ksize)
    masked = feats * torso_mask.unsqueeze(1)
    motion = torch.cat([masked, torso_segmap.unsqueeze(2).repeat([1, 1, masked.shape[2], 1, 1])], dim=1)
    return {"seg": torso_segmap, "mask_d": torso_mask[:, 0], "motion": motion, "seg_in": seg_in}


def main():
    import ref_stubs
    ref_stubs.install()
    from utils.commons.image_utils import dilate
    import torso_glue_ref64 as G
    for name, (seed, N, Cs, Hs, Ws, C, D, h, w, ksize, IH, IW) in CASES.items():
        inp = synth.synth_torso_glue_inputs(seed, N, Cs, Hs, Ws, C, D, h, w)
        img = synth.synth_torso_appearance_inputs(seed + 1, N, 3, IH, IW)["x"]
        seg, feats, img = (torch.from_numpy(v) for v in (inp["segmap"], inp["feats"], img))
        with torch.no_grad():
            out = reference_glue(dilate, feats, seg, ksize, img)
            out64 = reference_glue(dilate, feats.double(), seg, ksize, img.double())
        assert all(v.dtype == torch.float32 for v in out.values()) and all(v.dtype == torch.float64 for v in out64.values())
        e32 = np.array([G.rel(out[k].numpy(), out64[k].numpy()) for k in KEYS])
        md = out["mask_d"].numpy()
        assert not np.array_equal(md[0], md[1]) and md.std() > 0.02 and out["seg"].numpy().std() > 0.02, name
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, spec=np.array([seed, N, Cs, Hs, Ws, C, D, h, w, ksize, IH, IW], np.int64), e32=e32,
                            **{k: out[k].numpy() for k in KEYS})
        assert os.path.getsize(path) <= MAX_BYTES, (name, os.path.getsize(path))
        print(name, os.path.getsize(path), "bytes; reference fp32 against its own calls in fp64 (seg, mask_d, motion, seg_in):",
              ["%.2e" % e for e in e32])


if __name__ == "__main__":
    main()
