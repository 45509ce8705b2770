"""Records tests/golden/video_frames_*.npz: small synthetic clips (tests/video_frames_ref.py clip()) and the bytes the oracle there -- the
reference's operator sequence, inference/real3d_infer.py:495-521 -- returns for them on the CPU, in both out modes.

    python tests/golden/make_golden_video_frames.py

Inputs and expected outputs only; tests/test_video_frames_host.py checks that the oracle still reproduces every file."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import video_frames_ref as R          # noqa: E402

# name -> (seed, T, H, W, secc (h, w), raw (h, w), depth (h, w), depth kind)
CASES = {
    "a_t3_32": (11, 3, 32, 32, (32, 32), (8, 8), (8, 8), "spread"),
    "b_t2_12x20": (12, 2, 12, 20, (9, 24), (5, 7), (7, 5), "spread"),
    "c_constant_depth": (13, 2, 16, 16, (16, 16), (4, 4), (4, 4), "constant"),
    "d_nan_depth": (14, 2, 16, 16, (16, 16), (4, 4), (4, 4), "nan"),
}


def main():
    for name, (seed, T, H, W, shw, rhw, dhw, kind) in CASES.items():
        c = R.clip(seed, T, H, W, shw, rhw, dhw, kind)
        out = R.oracle_of(c)
        fin = R.final(torch.from_numpy(c["imgs"]))
        assert out.shape == (T, H, 5 * W, 3) and fin.shape == (T, H, W, 3)
        path = os.path.join(HERE, "video_frames_%s.npz" % name)
        np.savez_compressed(path, concat_debug=out, final=fin, **c)
        print("%s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
