"""CPU: the host side of the HIP source-image conditions (real3dportrait_amd/source_conditions.py, include/r3d_hip_source.h).

The goldens (tests/golden/source_cond_*.npz) are the reference's own extract_background(..., 'knn') and inpaint_torso_job on synthetic
portraits, recorded with the fixed-point blur model in the place of cv2.GaussianBlur (tests/golden/make_golden_source_conditions.py says
so: equality of that model with OpenCV has not been measured).  What is checked without a GPU: the NumPy restatement
(tests/source_conditions_ref.py) reproduces every golden, outside the tie pixels for the background; the portraits contain what the
kernels can get wrong; the companion header against the binding table and the library's exports; every argument refusal of the entry
points, which run before any HIP call; the Python functions' type, shape and dtype errors; the planes' formula on all 256 bytes."""
import ctypes
import glob
import os
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden
import source_conditions_ref as R

CASES = ("1_96", "2_128x96", "3_96x160", "4_96x70", "5_128_b3")
SIZES = {"1_96": (96, 96, 1), "2_128x96": (128, 96, 1), "3_96x160": (96, 160, 1), "4_96x70": (96, 70, 1), "5_128_b3": (128, 128, 3)}
TIE_CAP = 0.10
ENTRY_POINTS = {"r3d_source_workspace_bytes": 3, "r3d_source_nearest": 10, "r3d_source_background": 10, "r3d_source_torso": 13,
                "r3d_source_select": 8, "r3d_source_to_planes": 7}
_background = {}


def background_of(case):
    """The restatement's background of a golden, computed once for the module."""
    if case not in _background:
        g = load_golden("source_cond_" + case)
        imgs, segs = R.frames_of(g)
        _background[case] = (g, imgs, segs, R.background(imgs, segs[:, 0]))
    return _background[case]


def test_every_fixture_is_listed_and_small():
    names = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "source_cond_*.npz")))
    assert names == sorted("source_cond_" + c for c in CASES)
    assert all(os.path.getsize(os.path.join(GOLDEN, n + ".npz")) <= 262144 for n in names)
    for c in CASES:
        g = load_golden("source_cond_" + c)
        H, W, _, B = (int(v) for v in g["spec"])
        assert (H, W, B) == SIZES[c] and g["label"].shape == (B, H, W) and g["label"].max() == 5
        assert g["bg_img"].shape == (H, W, 3) and g["bg_img"].dtype == np.uint8
        assert g["torso_img_mask"].dtype == bool and g["torso_with_bg_img_mask"].dtype == bool


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_the_background_up_to_ties(case):
    g, imgs, segs, res = background_of(case)
    outside, bad = R.matches_up_to_ties(res, g["bg_img"])
    filled, ties = int((~res["sure"]).sum()), int(res["tie"].sum())
    print("%s: %d filled pixels, %d ties (%.1f %%), %d differ outside the ties, %d tie pixels off their candidates"
          % (case, filled, ties, 100.0 * ties / filled, outside, bad))
    assert outside == 0 and bad == 0
    assert 0 < ties <= TIE_CAP * filled
    if len(imgs) == 3:                            # frames 0 and 1 have one segmap: argmax takes frame 0; frame 2 is shifted and wins somewhere
        assert not (res["frame"] == 1).any() and (res["frame"][res["sure"]] == 2).any() and (res["frame"][res["sure"]] == 0).any()
        assert not np.array_equal(imgs[0], imgs[1]) and np.array_equal(segs[0], segs[1]) and (segs[0][0] != segs[2][0]).any()


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_the_torso_job_and_the_portraits_hold_every_feature(case):
    g = load_golden("source_cond_" + case)
    imgs, segs = R.frames_of(g)
    for wrap in (False, True):                    # no paint reaches above row 0 in these cases: both agree with the reference
        t = R.inpaint_torso(imgs[0], segs[0], wrap=wrap)
        for k, key in enumerate(("torso_img", "torso_img_mask", "torso_with_bg_img", "torso_with_bg_img_mask")):
            assert t[k].dtype == g[key].dtype and np.array_equal(t[k], g[key]), (key, wrap)
    info = t[4]
    assert not info["wraps"]
    assert info["torso_cols"] > 0 and info["neck_cols_lt5"] > 0 and info["neck_cols_gt5"] > 0 and info["dilated_only"] > 0
    assert info["neck_paint"].sum() > 0
    # the second masking line of the reference is a no-op and torso_with_bg_img is never masked
    assert np.array_equal(g["torso_img"][g["torso_img_mask"]], g["torso_with_bg_img"][g["torso_img_mask"]]) and not g["torso_img"][~g["torso_img_mask"]].any()
    only_bg = g["torso_with_bg_img_mask"] & ~g["torso_img_mask"]
    assert np.array_equal(g["torso_with_bg_img"][only_bg], imgs[0][only_bg]) and g["torso_with_bg_img"][only_bg].any()


def test_the_deviation_case_wraps_in_the_reference_and_not_in_the_kernels():
    from real3dportrait_amd import synth
    seg, img = synth.synth_portrait_segmap(64, 64, 6), synth.synth_portrait_image(64, 64, 6)
    dropped, wrapped = R.inpaint_torso(img, seg, wrap=False), R.inpaint_torso(img, seg, wrap=True)
    assert dropped[4]["wraps"] and wrapped[4]["wraps"]
    assert not np.array_equal(dropped[2], wrapped[2]) and wrapped[4]["neck_paint"].sum() > dropped[4]["neck_paint"].sum()


def test_the_blur_model_is_within_its_derived_bound_of_the_fp64_gaussian():
    assert sum(R.BLUR_WEIGHTS) == 256
    assert tuple(int(v) for v in np.floor(R.gaussian_weights(4.0) * 256 + 0.5)) == R.BLUR_WEIGHTS
    bound = R.blur_bound()
    assert 1 <= bound <= 3
    from real3dportrait_amd import synth
    img = synth.synth_portrait_image(40, 52, 9)
    err = np.abs(R.blur_fixed(img).astype(np.float64) - R.blur_fp64(img)).max()
    print("blur model against fp64: %g counts, bound %d" % (err, bound))
    assert err <= bound


def test_symbols_are_declared_exported_and_bound():
    """The six entry points live in the companion header include/r3d_hip_source.h (tests/test_abi.py compares every declaration with the
    binding table and with what load() bound, and the header's macros with the package's constants); here what is this unit's own: the
    parameter counts, the ABI number and the package's names."""
    from real3dportrait_amd import _lib
    from abi import header_declarations
    import real3dportrait_amd
    lib = _lib.load()
    assert lib.r3d_version() == _lib.ABI_VERSION
    decls = header_declarations("r3d_hip_source.h")
    assert set(decls) == set(ENTRY_POINTS) <= set(_lib.SIGNATURES)
    assert {name: len(types_) for name, (ret, types_) in decls.items()} == ENTRY_POINTS
    assert _lib.SOURCE_HEAD_CLASSES == (1 << 1) | (1 << 3) | (1 << 5)
    from real3dportrait_amd import source_conditions
    for name in ("nearest_seed", "head_image", "inpaint_torso_job", "extract_background", "source_to_planes", "patch_segment_imgs"):
        assert getattr(real3dportrait_amd, name) is getattr(source_conditions, name), name
    assert real3dportrait_amd.source_conditions is source_conditions and callable(source_conditions.source_conditions)          # the module's name
    assert np.array_equal(source_conditions.DARKEN, 0.98 ** np.arange(53)) and source_conditions.BLUR_WEIGHTS == R.BLUR_WEIGHTS


def test_workspace_size_follows_the_stated_layout():
    from real3dportrait_amd import _lib
    lib = _lib.load()
    pad = lambda n: (n + 15) // 16 * 16
    for B, H, W in ((1, 96, 70), (3, 128, 128), (1, 512, 512), (2, 3, 5), (1, 2048, 2048)):
        N = H * W
        assert lib.r3d_source_workspace_bytes(B, H, W) == 2 * pad(4 * B * N) + pad(4 * N) + pad(N) + pad(3 * N) + pad(8 * W), (B, H, W)
    for bad in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (1, 2049, 8), (1, 8, 2049), (65536, 8, 8), (128, 2048, 2048)):
        assert lib.r3d_source_workspace_bytes(*bad) == 0, bad


def test_c_entry_points_reject_bad_arguments_without_a_gpu():
    from real3dportrait_amd import _lib
    lib = _lib.load()
    P = lambda k: ctypes.c_void_p(k << 32)              # never dereferenced: validation fails first
    at = lambda a: ctypes.c_void_p(a)
    err = lambda: lib.r3d_last_error()
    darken = (ctypes.c_double * 53)(*(0.98 ** np.arange(53)).tolist())
    weights = lambda *w: (ctypes.c_int * 5)(*w)
    big = 1 << 26                                       # a workspace of any size asked for below

    def near(mask=P(1), B=2, H=12, W=20, d2=P(2), index=P(3), status=P(4), ws=P(5), ws_bytes=big):
        return lib.r3d_source_nearest(mask, B, H, W, d2, index, status, ws, ws_bytes, None)

    def back(img=P(1), bg=P(2), B=2, H=12, W=20, out=P(3), status=P(4), ws=P(5), ws_bytes=big):
        return lib.r3d_source_background(img, bg, B, H, W, out, status, ws, ws_bytes, None)

    def torso(img=P(1), seg=P(2), H=12, W=20, dk=darken, wts=weights(48, 53, 54, 53, 48), t_img=P(3), t_mask=P(4), b_img=P(5), b_mask=P(6), ws=P(7),
              ws_bytes=big):
        return lib.r3d_source_torso(img, seg, H, W, dk, wts, t_img, t_mask, b_img, b_mask, ws, ws_bytes, None)

    def sel(img=P(1), seg=P(2), classes=42, H=12, W=20, out=P(3), mask=P(4)):
        return lib.r3d_source_select(img, seg, classes, H, W, out, mask, None)

    def planes(img=P(1), seg=P(2), classes=42, H=12, W=20, out=P(3)):
        return lib.r3d_source_to_planes(img, seg, classes, H, W, out, None)

    need = lib.r3d_source_workspace_bytes(2, 12, 20)
    name = b"source_nearest:"
    for k in ("mask", "status", "ws"):
        assert near(**{k: None}) == -1 and name in err() and b"NULL pointer" in err(), k
    assert near(d2=None, index=None) == -1 and b"NULL pointer" in err()
    for k in ("B", "H", "W"):
        for bad in (0, -1):
            assert near(**{k: bad}) == -1 and name in err() and b"must be positive" in err(), (k, bad)
    assert near(H=2049) == -1 and b"above 2048" in err()
    assert near(W=2049) == -1 and b"above 2048" in err()
    assert near(B=65536, H=1, W=1) == -1 and b"above 65535" in err()
    assert near(B=128, H=2048, W=2048) == -1 and b"2^31" in err()          # 4 B H W = 2^31
    for k in ("d2", "index", "status"):
        assert near(**{k: at(({"d2": 2, "index": 3, "status": 4}[k] << 32) + 2)}) == -1 and b"4-byte aligned" in err(), k
    assert near(ws=at((5 << 32) + 8)) == -1 and b"16-byte aligned" in err()
    assert near(ws_bytes=need - 1) == -1 and b"are needed" in err()
    n = 2 * 12 * 20
    for k, base, nbytes in (("d2", 1, n), ("index", 1, n), ("status", 1, n), ("ws", 1, n), ("index", 2, 4 * n), ("status", 3, 4 * n), ("d2", 5, need),
                            ("status", 5, need)):
        assert near(**{k: at(base << 32)}) == -1 and b"overlaps" in err(), (k, base)
        assert near(**{k: at((base << 32) + (nbytes - 4) // 16 * 16)}) == -1 and b"overlaps" in err(), (k, base)

    name = b"source_background:"
    for k in ("img", "bg", "out", "status", "ws"):
        assert back(**{k: None}) == -1 and name in err() and b"NULL pointer" in err(), k
    for k in ("B", "H", "W"):
        for bad in (0, -1):
            assert back(**{k: bad}) == -1 and name in err() and b"must be positive" in err(), (k, bad)
    assert back(H=4096) == -1 and b"above 2048" in err()
    assert back(B=128, H=2048, W=2048) == -1 and b"2^31" in err()
    assert back(out=at((3 << 32) + 1)) == -1 and b"4-byte aligned" in err()
    assert back(status=at((4 << 32) + 2)) == -1 and b"4-byte aligned" in err()
    assert back(ws=at((5 << 32) + 4)) == -1 and b"16-byte aligned" in err()
    assert back(ws_bytes=need - 16) == -1 and b"are needed" in err()
    for k, base, nbytes in (("out", 1, 3 * n), ("out", 2, n), ("status", 1, 3 * n), ("ws", 2, n), ("status", 3, 3 * 12 * 20), ("out", 5, need)):
        assert back(**{k: at(base << 32)}) == -1 and b"overlaps" in err(), (k, base)
        assert back(**{k: at((base << 32) + (nbytes - 4) // 16 * 16)}) == -1 and b"overlaps" in err(), (k, base)

    name = b"source_torso:"
    for k in ("img", "seg", "dk", "wts", "t_img", "t_mask", "b_img", "b_mask", "ws"):
        assert torso(**{k: None}) == -1 and name in err() and b"NULL pointer" in err(), k
    for k in ("H", "W"):
        for bad in (0, -1):
            assert torso(**{k: bad}) == -1 and name in err() and b"must be positive" in err(), (k, bad)
        for bad in (1, 2):
            assert torso(**{k: bad}) == -1 and name in err() and b"below 3" in err(), (k, bad)
        assert torso(**{k: 2049}) == -1 and b"above 2048" in err()
    for bad in ((48, 53, 54, 53, 49), (-1, 53, 54, 53, 48), (257, 0, 0, 0, 0)):
        assert torso(wts=weights(*bad)) == -1 and name in err() and b"blur weight" in err(), bad
    for bad in (1.5, -0.1, float("nan")):
        dk = (ctypes.c_double * 53)(*([1.0] * 52 + [bad]))
        assert torso(dk=dk) == -1 and b"darken[52]" in err(), bad
    for k, base in (("t_img", 3), ("t_mask", 4), ("b_img", 5), ("b_mask", 6)):
        assert torso(**{k: at((base << 32) + 2)}) == -1 and b"4-byte aligned" in err(), k
    assert torso(ws=at((7 << 32) + 8)) == -1 and b"16-byte aligned" in err()
    assert torso(ws_bytes=lib.r3d_source_workspace_bytes(1, 12, 20) - 1) == -1 and b"are needed" in err()
    for k in ("t_img", "t_mask", "b_img", "b_mask", "ws"):
        for base, nbytes in ((1, 3 * 240), (2, 6 * 240)):
            assert torso(**{k: at(base << 32)}) == -1 and b"overlaps" in err(), (k, base)
            assert torso(**{k: at((base << 32) + nbytes - 16)}) == -1 and b"overlaps" in err(), (k, base)
    assert torso(t_mask=at((3 << 32) + 3 * 240 - 4)) == -1 and b"overlaps" in err()          # two outputs on each other
    assert torso(b_mask=P(7)) == -1 and b"overlaps" in err()                                 # an output in the workspace

    name = b"source_select:"
    for k in ("img", "seg", "out"):
        assert sel(**{k: None}) == -1 and name in err() and b"NULL pointer" in err(), k
    for bad in (0, -1, 64):
        assert sel(classes=bad) == -1 and name in err() and b"classes" in err(), bad
    assert sel(H=0) == -1 and b"must be positive" in err() and sel(W=2049) == -1 and b"above 2048" in err()
    assert sel(out=at((3 << 32) + 2)) == -1 and b"4-byte aligned" in err() and sel(mask=at((4 << 32) + 1)) == -1 and b"4-byte aligned" in err()
    assert sel(out=P(1)) == -1 and b"overlaps" in err() and sel(mask=at((2 << 32) + 6 * 240 - 4)) == -1 and b"overlaps" in err()
    assert sel(mask=P(3)) == -1 and b"overlaps" in err()

    name = b"source_to_planes:"
    for k in ("img", "out"):
        assert planes(**{k: None}) == -1 and name in err() and b"NULL pointer" in err(), k
    for bad in (0, -1, 64):
        assert planes(classes=bad) == -1 and name in err() and b"classes" in err(), bad
    assert planes(H=-1) == -1 and b"must be positive" in err() and planes(H=2049) == -1 and b"above 2048" in err()
    assert planes(out=at((3 << 32) + 2)) == -1 and b"4-byte aligned" in err()
    assert planes(out=P(1)) == -1 and b"overlaps" in err() and planes(out=at((2 << 32) - 12 * 240 + 4)) == -1 and b"overlaps" in err()
    # without a segmap the classes are not looked at: the one defect left is reported
    assert planes(seg=None, classes=0, out=None) == -1 and b"NULL pointer" in err()


def test_python_functions_refuse_before_the_library_is_entered():
    from real3dportrait_amd import _lib, source_conditions as S, synth
    img, seg = synth.synth_portrait_image(16, 24, 1), synth.synth_portrait_segmap(16, 24, 1)
    t_img, t_seg = torch.from_numpy(img), torch.from_numpy(seg)
    with _lib.counting() as calls:
        for fn in (S.head_image, S.inpaint_torso_job, S.source_conditions, lambda a, b: S.extract_background([a], [b])):
            with pytest.raises(ValueError, match="GPU only"):
                fn(t_img, t_seg)                                  # a host tensor is not computed on
        with pytest.raises(ValueError, match="GPU only"):
            S.nearest_seed(t_seg[0])
        with pytest.raises(ValueError, match="GPU only"):
            S.source_to_planes(t_img)
        for fn in (S.head_image, S.inpaint_torso_job, S.source_conditions, S.source_to_planes):
            with pytest.raises(TypeError, match="uint8"):
                fn(img.astype(np.float32), seg)
            with pytest.raises(TypeError, match="uint8"):
                fn(t_img.float(), t_seg)
            with pytest.raises(ValueError, match=r"\[H, W, 3\]"):
                fn(img[:, :, :2], seg)
            with pytest.raises(ValueError, match=r"\[H, W, 3\]"):
                fn(img[None], seg)
            with pytest.raises(TypeError, match="NumPy array or a tensor"):
                fn(img.tolist(), seg)
        with pytest.raises(ValueError, match="must be 3 .. 2048"):
            S.inpaint_torso_job(img[:2], seg[:, :2])
        with pytest.raises(ValueError, match="must be 1 .. 2048"):
            S.nearest_seed(np.ones((4, 2049), np.uint8))
        with pytest.raises(ValueError, match=r"\[H, W\] or \[B, H, W\]"):
            S.nearest_seed(np.ones((2, 2, 4, 4), np.uint8))
        with pytest.raises(TypeError, match="NumPy array or a tensor"):
            S.nearest_seed([[1, 0]])
        with pytest.raises(NotImplementedError):
            S.extract_background([img], [seg], "lama")
        with pytest.raises(ValueError, match="segmap_mask_lst is needed"):
            S.extract_background([img])
        with pytest.raises(AssertionError):
            S.extract_background([img, img], [seg])
        with pytest.raises(TypeError, match="file names"):
            S.extract_background(["a.png"], [seg])
        with pytest.raises(TypeError, match="uint8"):
            S.extract_background([img.astype(np.int32)], [seg])
        with pytest.raises(ValueError, match=r"\[H, W, 3\]"):
            S.extract_background([img[..., 0]], [seg])
    assert calls == []
    if not torch.cuda.is_available():             # a NumPy input needs a GPU to be uploaded to: the shapes are checked first
        with pytest.raises(ValueError, match="no GPU"):
            S.head_image(img, seg)


def test_frame_selection_is_the_references():
    """extract_background keeps every 5th frame below 100 frames, every 20th below 10 000, every (num_frames // 500)th above, and the first
    frame alone when there are no more frames than the interval (:91-103)."""
    from real3dportrait_amd import source_conditions as S
    picked = lambda n: list(range(n))[S.frame_selection(n)]
    assert picked(1) == [0] and picked(3) == [0] and picked(5) == [0] and picked(6) == [0, 5] and picked(11) == [0, 5, 10]
    assert picked(99) == list(range(0, 99, 5)) and picked(100) == [0, 20, 40, 60, 80] and picked(101) == [0, 20, 40, 60, 80, 100]
    assert picked(9999) == list(range(0, 9999, 20)) and picked(10000) == list(range(0, 10000, 20)) and picked(12000) == list(range(0, 12000, 24))


def test_planes_formula_is_torchs_on_every_byte():
    """(float(x) - 127.5f) / 127.5f with IEEE division is ((torch.tensor(img) - 127.5) / 127.5).float(): uint8 - 127.5 promotes to fp32, and
    both operations are correctly rounded; stated on all 256 bytes in NumPy fp32, the arithmetic the kernel performs."""
    b = np.arange(256, dtype=np.uint8)
    want = ((torch.tensor(b) - 127.5) / 127.5).float()
    assert want.dtype == torch.float32
    got = (b.astype(np.float32) - np.float32(127.5)) / np.float32(127.5)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.numpy().view(np.uint32))
    assert got[0] == -1.0 and got[255] == 1.0
    recip = (b.astype(np.float32) - np.float32(127.5)) * np.float32(1.0 / 127.5)          # a multiplication by the reciprocal is NOT the same
    print("multiplying by 1 / 127.5 instead differs on %d of 256 bytes" % int((recip != got).sum()))


def test_patch_segment_imgs_swaps_exactly_the_two_names():
    from real3dportrait_amd import patch_segment_imgs, source_conditions as S
    ref = lambda *a, **k: "reference"
    mod = types.SimpleNamespace(inpaint_torso_job=ref, extract_background=ref, blink_eye_for_secc=ref, MediapipeSegmenter=ref)
    before = dict(vars(mod))
    assert patch_segment_imgs(mod) is mod
    assert mod.inpaint_torso_job is S.inpaint_torso_job and mod.extract_background is S.extract_background
    assert {k for k, v in vars(mod).items() if before.get(k) is not v} == {"inpaint_torso_job", "extract_background"}
    import inspect
    assert list(inspect.signature(S.extract_background).parameters)[:3] == ["img_lst", "segmap_mask_lst", "method"]
    assert list(inspect.signature(S.inpaint_torso_job).parameters)[:2] == ["gt_img", "segmap"]
