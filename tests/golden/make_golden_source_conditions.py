"""Regenerate the source_cond_* golden vectors: the reference's own extract_background(..., 'knn') (with its sklearn kd-trees) and
inpaint_torso_job (data_gen/utils/process_video/extract_segment_imgs.py:63-239, with scipy's binary_dilation) on CPU, on the synthetic
portraits of real3dportrait_amd.synth.synth_portrait_segmap / synth_portrait_image.

Run in the build container only (needs the reference tree, sklearn and scipy):
    R3D_REFERENCE=<reference tree> python tests/golden/make_golden_source_conditions.py

cv2 is not installed here.  THE BLUR INSIDE THESE GOLDENS IS THE FIXED-POINT MODEL of tests/source_conditions_ref.py blur_fixed (separable,
weights (48, 53, 54, 53, 48) / 256, reflect-101, rounded half up), installed as cv2.GaussianBlur for the run, NOT OpenCV: whether OpenCV's
8-bit path gives the same bytes has not been measured.  Everything else in the files is the reference's own code.  mediapipe, which the
reference's module imports and never calls on this path, is a stand-in as well.

Each file holds arrays only: spec (H, W, seed, B), label [B, H, W] uint8 (the class of every pixel; the one-hot segmap is label == k), img
(the frames; for B = 3 only frames 0 and 2 are stored, frame 1 has frame 0's segmap and the image 255 - frame 0), bg_img (the reference's
background image of the B frames) and the four returns of inpaint_torso_job on frame 0.  The maker prints and asserts: the restatement
equals the reference outside the tie pixels and every tie pixel's colour is one of its candidates'; ties are at most 10 % of the filled
pixels; the portraits contain what the kernels can get wrong."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ["R3D_REFERENCE"]          # the reference tree
sys.path.insert(0, REF)
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(REPO, "tests"))

from real3dportrait_amd import synth  # noqa: E402

# name -> (H, W, seed, B)
CASES = {"source_cond_1_96": (96, 96, 1, 1),
         "source_cond_2_128x96": (128, 96, 2, 1),
         "source_cond_3_96x160": (96, 160, 3, 1),
         "source_cond_4_96x70": (96, 70, 4, 1),
         "source_cond_5_128_b3": (128, 128, 5, 3)}
SHIFT = 0.06                               # of frame 2 of the B = 3 case
INTERVAL = 5                               # the reference's FRAME_SELECT_INTERVAL below 100 frames
TIE_CAP = 0.10
MAX_BYTES = 262144


def install_stand_ins(R):
    import ref_stubs
    ref_stubs.install()
    for name in ("mediapipe", "mediapipe.tasks", "mediapipe.tasks.python", "mediapipe.tasks.python.vision"):
        if name not in sys.modules:
            m = ref_stubs._Stub(name)
            m.__path__ = []
            sys.modules[name] = m
    cv2 = sys.modules["cv2"]
    cv2.BORDER_DEFAULT = 4

    def GaussianBlur(img, ksize, sigmaX):
        assert tuple(ksize) == (5, 5) and sigmaX == 4, (ksize, sigmaX)          # the reference passes cv2.BORDER_DEFAULT as sigmaX
        return R.blur_fixed(img)
    cv2.GaussianBlur = GaussianBlur


def main():
    import source_conditions_ref as R
    install_stand_ins(R)
    from data_gen.utils.process_video.extract_segment_imgs import extract_background, inpaint_torso_job
    for name, (H, W, seed, B) in CASES.items():
        shifts = [0.0, 0.0, SHIFT][:B]
        label = np.stack([synth.synth_portrait_segmap(H, W, seed, shift=s).argmax(axis=0).astype(np.uint8) for s in shifts])
        stored = np.stack([synth.synth_portrait_image(H, W, seed + 10 * b, shift=shifts[b]) for b in range(B) if b != 1])
        g = {"spec": np.array([H, W, seed, B], np.int64), "label": label, "img": stored}
        imgs, segs = R.frames_of(g)
        if B == 1:
            bg_ref = extract_background([imgs[0]], [segs[0]], "knn")
        else:                                     # the reference keeps every fifth frame: frames 0, 5, 10 of 11 are the three
            pick = [b // INTERVAL if b % INTERVAL == 0 else 0 for b in range(INTERVAL * (B - 1) + 1)]
            bg_ref = extract_background([imgs[b] for b in pick], [segs[b] for b in pick], "knn")
            assert np.array_equal(segs[0], segs[1]) and not np.array_equal(imgs[0], imgs[1])
            moved = int((segs[0][0] != segs[2][0]).sum())
            print("%s: the person of frame 2 is shifted: %d background pixels differ" % (name, moved))
            assert moved > 0
        res = R.background(imgs, segs[:, 0])
        outside, bad = R.matches_up_to_ties(res, bg_ref)
        filled, ties = int((~res["sure"]).sum()), int(res["tie"].sum())
        print("%s: %d sure pixels, %d filled, %d ties (%.1f %%); restatement differs at %d pixels outside the ties, %d tie pixels off the candidates"
              % (name, int(res["sure"].sum()), filled, ties, 100.0 * ties / filled, outside, bad))
        assert outside == 0 and bad == 0 and ties <= TIE_CAP * filled, name
        if B > 1:
            later = int((res["frame"][res["sure"]] > 0).sum())
            print("%s: %d sure pixels take their colour from frame 2, none from frame 1" % (name, later))
            assert later > 0 and not (res["frame"] == 1).any()
        t_ref = inpaint_torso_job(imgs[0], segs[0])
        for wrap in (True, False):
            t = R.inpaint_torso(imgs[0], segs[0], wrap=wrap)
            for k, key in enumerate(("torso_img", "torso_img_mask", "torso_with_bg_img", "torso_with_bg_img_mask")):
                assert t[k].dtype == t_ref[k].dtype and np.array_equal(t[k], t_ref[k]), (name, key, wrap)
        info = t[4]
        counts = {k: info[k] for k in ("torso_cols", "neck_cols_lt5", "neck_cols_gt5", "dilated_only")}
        print("%s: %s, paint above row 0: %s, %d blurred pixels" % (name, counts, info["wraps"], int(info["neck_paint"].sum())))
        assert all(v > 0 for v in counts.values()) and not info["wraps"], name
        g.update(bg_img=bg_ref, torso_img=t_ref[0], torso_img_mask=t_ref[1], torso_with_bg_img=t_ref[2], torso_with_bg_img_mask=t_ref[3])
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **g)
        assert os.path.getsize(path) <= MAX_BYTES, (name, os.path.getsize(path))
        print(name, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
