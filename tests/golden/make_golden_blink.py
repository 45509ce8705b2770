"""Regenerate the blink_* golden vectors: the reference's own blink_eye_for_secc (inference/edit_secc.py:47-129, with its sklearn
kd-trees) on CPU, on the synthetic maps of real3dportrait_amd.synth.synth_secc_eyes.

Run in the build container only (needs the reference tree and sklearn):
    R3D_REFERENCE=<reference tree> python tests/golden/make_golden_blink.py
Each file holds arrays only: spec (H, W, seed, crossing, zero_channel), the fp32 input img [3, H, W], the percentages p [3] and the
reference's outputs as their 8-bit q [3, H, W, 3] uint8 -- the output is exactly q / 127.5 - 1, which the tests rebuild in NumPy."""
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

# name -> (H, W, seed, crossing, zero_channel)
CASES = {"blink_a_64": (64, 64, 3, 0, 0),
         "blink_b_64x96": (64, 96, 4, 0, 0),
         "blink_c_96x64": (96, 64, 5, 0, 0),
         "blink_d_128_crossing": (128, 128, 6, 1, 0),
         "blink_e_96_zero_channel": (96, 96, 3, 0, 6)}
PERCENTS = (0.0, 0.36, 1.0)
MAX_BYTES = 262144


def main():
    import ref_stubs
    ref_stubs.install()
    from inference.edit_secc import blink_eye_for_secc
    import blink_ref as R
    for name, (H, W, seed, crossing, zero_channel) in CASES.items():
        img = synth.synth_secc_eyes(H, W, seed, crossing=bool(crossing), zero_channel=zero_channel)
        qs = []
        for p in PERCENTS:
            out = blink_eye_for_secc(torch.from_numpy(img), p).numpy()
            q = np.round((out.astype(np.float64) + 1) * 127.5).astype(np.int64).transpose(1, 2, 0)
            assert q.min() >= 0 and q.max() <= 255 and np.array_equal(R.dequantise(q), out), name          # exactly 8-bit
            qs.append(q.astype(np.uint8))
            res = R.blink(img, p)
            outside, bad = R.matches_up_to_ties(res, q)
            edited = 0 if res["B"] is None else int(res["B"].sum())
            print("%s p %.2f: %d edited pixels, %d ties; restatement differs at %d pixels outside the ties, %d tie pixels off the candidates"
                  % (name, p, edited, int(res["tie"].sum()), outside, bad))
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, spec=np.array([H, W, seed, crossing, zero_channel], np.int64), img=img, p=np.array(PERCENTS, np.float64),
                            q=np.stack(qs))
        assert os.path.getsize(path) <= MAX_BYTES, (name, os.path.getsize(path))
        print(name, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
