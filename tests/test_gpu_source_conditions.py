"""GPU: the HIP source-image conditions (real3dportrait_amd/source_conditions.py, include/r3d_hip_source.h) against the
reference's recorded results (tests/golden/source_cond_*.npz: extract_background and inpaint_torso_job themselves, the blur being the
fixed-point model) and against the NumPy restatement (tests/source_conditions_ref.py).

Cases 1 to 5 are the goldens: 96 x 96; 128 x 96 (H > W); 96 x 160 (W above a wavefront, no multiple of 64); 96 x 70 (W % 4 != 0: lanes of
4 pixels straddle rows); 128 x 128 with B = 3 (frames 0 and 1 share a segmap and differ in the image, frame 2 is shifted).  Case 6,
64 x 64, has its neck less than 52 rows from the top: the reference wraps the paint to the bottom rows, the kernels drop it, so it is
compared with the restatement only.  Case 7, 45 x 39, has H W % 4 = 3: the last lane writes bytes.  The restatement of every case is
computed once for the module."""
import types

import numpy as np
import pytest
import torch

from conftest import load_golden
import source_conditions_ref as R

pytestmark = pytest.mark.gpu

GOLDEN_CASES = ("1_96", "2_128x96", "3_96x160", "4_96x70", "5_128_b3")
EXTRA_CASES = {"6_64_wraps": (64, 64, 6), "7_45x39_tail": (45, 39, 7)}
ALL_CASES = GOLDEN_CASES + tuple(EXTRA_CASES)
DEV = "cuda:0"
_cases = {}


def case_of(name):
    """(golden or None, imgs [B, H, W, 3], segs [B, 6, H, W], the restatement's background, the restatement's torso job of frame 0)."""
    if name not in _cases:
        if name in EXTRA_CASES:
            from real3dportrait_amd import synth
            H, W, seed = EXTRA_CASES[name]
            g, imgs, segs = None, synth.synth_portrait_image(H, W, seed)[None], synth.synth_portrait_segmap(H, W, seed)[None]
        else:
            g = load_golden("source_cond_" + name)
            imgs, segs = R.frames_of(g)
        _cases[name] = (g, imgs, segs, R.background(imgs, segs[:, 0]), R.inpaint_torso(imgs[0], segs[0], wrap=False))
    return _cases[name]


def on_device(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def check_nearest(mask):
    """nearest_seed of a [B, H, W] mask against the brute force at every pixel; returns the number of tie pixels."""
    from real3dportrait_amd import nearest_seed
    d2, index = nearest_seed(on_device(mask.astype(np.uint8)))
    assert d2.dtype == torch.int32 and index.dtype == torch.int32 and tuple(d2.shape) == mask.shape == tuple(index.shape)
    d2, index, ties = d2.cpu().numpy(), index.cpu().numpy(), 0
    for b in range(mask.shape[0]):
        want_d2, want_index, tie = R.nearest_brute(mask[b])
        assert np.array_equal(d2[b], want_d2) and np.array_equal(index[b], want_index), b
        ties += int(tie.sum())
    return ties


@pytest.mark.parametrize("case", ALL_CASES)
def test_nearest_seed_is_exact_at_every_pixel_ties_included(case):
    _, _, segs, res, _ = case_of(case)
    ties = check_nearest(segs[:, 0] == 0) + check_nearest(res["sure"][None])
    print("%s: %d pixels with several equidistant seeds, all at the lowest (row, col)" % (case, ties))
    assert ties > 0


def test_nearest_seed_corners_full_column_and_wide_masks():
    H, W = 37, 70
    corners = np.zeros((4, H, W), bool)
    for b, (r, c) in enumerate(((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1))):
        corners[b, r, c] = True
    check_nearest(corners)
    from real3dportrait_amd import nearest_seed
    d2, index = nearest_seed(on_device(corners.astype(np.uint8)))
    assert int(d2[0, H - 1, W - 1]) == (H - 1) ** 2 + (W - 1) ** 2 and int(index[3, 0, 0]) == (H - 1) * W + W - 1
    full = np.ones((1, H, W), bool)
    check_nearest(full)
    d2, index = nearest_seed(on_device(full.astype(np.uint8)))
    assert not d2.any() and torch.equal(index.reshape(-1).cpu(), torch.arange(H * W, dtype=torch.int32))
    column = np.zeros((1, H, W), bool)
    column[0, :, 41] = True
    assert check_nearest(column) == 0
    rows = np.zeros((1, H, W), bool)
    rows[0, 5], rows[0, 31] = True, True
    assert check_nearest(rows) > 0                # row 18 is 13 rows from both: the one above
    # more than one block along a row (W > 256), sparse seeds, and a single row and a single column of pixels
    from real3dportrait_amd import synth
    sparse = synth.hash_uniform(11, 2 * 9 * 300, stream=61).reshape(2, 9, 300) < 0.02
    assert sparse[0].any() and sparse[1].any()
    check_nearest(sparse)
    check_nearest(sparse[:, :1])
    check_nearest(np.ascontiguousarray(sparse[:, :, 7:8] | (np.arange(9) == 4)[None, :, None]))
    # NumPy in, NumPy out; a 2-D mask gives 2-D results
    d2, index = nearest_seed(rows[0])
    assert isinstance(d2, np.ndarray) and d2.shape == (H, W) and d2.dtype == np.int32 and np.array_equal(d2, R.nearest_brute(rows[0])[0])
    with pytest.raises(ValueError, match="no seed"):
        nearest_seed(np.stack([rows[0], np.zeros((H, W), bool)]))


@pytest.mark.parametrize("case", ALL_CASES)
def test_extract_background_matches_the_reference_up_to_ties_and_the_restatement_everywhere(case):
    from real3dportrait_amd import extract_background
    g, imgs, segs, res, _ = case_of(case)
    B = len(imgs)
    if B == 1:
        frames, maps = [imgs[0]], [segs[0]]
    else:                                         # frames 0, 5 and 10 of 11 are the three: the wrapper sub-samples as the reference does
        pick = [b // 5 if b % 5 == 0 else 0 for b in range(5 * (B - 1) + 1)]
        frames, maps = [imgs[b] for b in pick], [segs[b] for b in pick]
    out = extract_background(frames, maps, "knn")
    assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.shape == res["out"].shape
    assert np.array_equal(out, res["out"])
    if g is not None:
        golden = dict(res, out=out)
        outside, bad = R.matches_up_to_ties(golden, g["bg_img"])
        print("%s: %d tie pixels; %d pixels differ from the reference outside them, %d tie pixels off their candidates" % (case, int(res["tie"].sum()), outside, bad))
        assert outside == 0 and bad == 0
    dev_out = extract_background([on_device(f) for f in frames], [on_device(m) for m in maps])          # device tensors in, a device tensor out
    assert torch.is_tensor(dev_out) and dev_out.is_cuda and np.array_equal(dev_out.cpu().numpy(), out)
    as_float = extract_background([on_device(f) for f in frames], [on_device(m).float() for m in maps])  # the segmap as prepare_batch keeps it
    assert torch.equal(as_float, dev_out)


def test_extract_background_raises_where_sklearn_does():
    from real3dportrait_amd import extract_background, synth
    H, W = 48, 40
    img = synth.synth_portrait_image(H, W, 3)
    nobody = np.zeros((6, H, W), np.uint8)
    nobody[0] = 1
    with pytest.raises(ValueError, match="no seed pixel"):
        extract_background([img], [nobody])
    crowded = np.zeros((6, H, W), np.uint8)       # a person pixel every 8 rows and columns: nothing is 10 pixels away
    crowded[4, ::8, ::8] = 1
    crowded[0] = 1 - crowded[4]
    with pytest.raises(ValueError, match="more than 10 pixels away"):
        extract_background([img], [crowded])
    ok = synth.synth_portrait_segmap(H, W, 3)     # the status is zeroed by the next call
    assert extract_background([img], [ok]).shape == (H, W, 3)


def torso_on_device(img, seg):
    from real3dportrait_amd import inpaint_torso_job
    out = inpaint_torso_job(on_device(img), on_device(seg))
    assert [o.dtype for o in out] == [torch.uint8, torch.bool, torch.uint8, torch.bool] and all(o.is_cuda for o in out)
    return [o.cpu().numpy() for o in out]


@pytest.mark.parametrize("case", ALL_CASES)
def test_inpaint_torso_job_gives_the_four_returns_byte_for_byte(case):
    from real3dportrait_amd import inpaint_torso_job
    g, imgs, segs, _, want = case_of(case)
    got = torso_on_device(imgs[0], segs[0])
    keys = ("torso_img", "torso_img_mask", "torso_with_bg_img", "torso_with_bg_img_mask")
    for k, key in enumerate(keys):
        assert np.array_equal(got[k], want[k]), key
        if g is not None:
            assert got[k].dtype == g[key].dtype and np.array_equal(got[k], g[key]), key
    assert want[4]["wraps"] == (g is None)        # cases 6 and 7 are the deviation: compared with the restatement only
    host = inpaint_torso_job(imgs[0], segs[0].astype(np.int64))          # NumPy in, NumPy out; the segmenter's one-hot map is int64
    assert all(isinstance(h, np.ndarray) and np.array_equal(h, w) and h.dtype == w.dtype for h, w in zip(host, want[:4]))


def test_inpaint_torso_job_takes_the_empty_branches():
    _, imgs, segs, _, _ = case_of("1_96")
    no_neck = segs[0].copy()
    no_neck[4] |= no_neck[2]                      # the neck becomes clothes: clothes lie directly under the face, nothing is neck
    no_neck[2] = 0
    no_head = segs[0].copy()
    no_head[0] |= no_head[1] | no_head[3] | no_head[5]          # no head: no column is under head, both paints are empty
    no_head[[1, 3, 5]] = 0
    nothing = np.zeros_like(segs[0])
    nothing[0] = 1
    for name, seg, torso_cols in (("no neck", no_neck, True), ("no head", no_head, False), ("background only", nothing, False)):
        want = R.inpaint_torso(imgs[0], seg, wrap=False)
        assert (want[4]["torso_cols"] > 0) == torso_cols and want[4]["neck_paint"].sum() == 0 and not want[4]["wraps"], name
        got = torso_on_device(imgs[0], seg)
        for k in range(4):
            assert np.array_equal(got[k], want[k]), (name, k)


@pytest.mark.parametrize("case", ("1_96", "4_96x70", "7_45x39_tail"))
def test_the_blur_is_within_its_derived_bound_of_the_fp64_gaussian(case):
    """Inside the blur mask the result is the 5 x 5 Gaussian (sigma 4, reflect-101) of the painted image up to the quantisation of the five
    weights to 8 fractional bits: R.blur_bound derives the bound, 255 sum |Q - G| + 1 counts (2 for the default weights)."""
    _, imgs, segs, _, want = case_of(case)
    got = torso_on_device(imgs[0], segs[0])
    mask = want[4]["neck_paint"]
    exact = R.blur_fp64(want[4]["painted"])
    err = np.abs(got[2].astype(np.float64) - exact)[mask]
    bound = R.blur_bound()
    print("%s: %d blurred pixels, largest difference from the fp64 Gaussian %g counts, bound %d" % (case, int(mask.sum()), err.max(), bound))
    assert mask.sum() > 0 and err.max() <= bound
    assert (got[2][mask] != want[4]["painted"][mask]).any()          # the blur changes something


def reference_planes(img):
    """real3d_infer.py:249, :252, :260 on the host."""
    return ((torch.tensor(img) - 127.5) / 127.5).float().unsqueeze(0).permute(0, 3, 1, 2)


def bits_equal(a, b):
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    return a.dtype == b.dtype == torch.float32 and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("case", ("1_96", "2_128x96", "3_96x160", "4_96x70"))
def test_source_conditions_gives_the_four_tensors_of_prepare_batch_bit_for_bit(case):
    from real3dportrait_amd.source_conditions import source_conditions
    g, imgs, segs, res, _ = case_of(case)
    img, seg = imgs[0], segs[0].astype(np.int64)                       # the segmenter's map is int64
    bg_bytes = np.where(res["tie"][..., None], res["out"], g["bg_img"])          # the golden's bytes; at the tie pixels the documented choice
    assert (bg_bytes != g["bg_img"]).any(axis=-1).sum() <= res["tie"].sum()
    want = {"segmap": torch.tensor(seg).float().unsqueeze(0), "ref_head_img": reference_planes(R.head_image(img, seg)[0]),
            "ref_torso_img": reference_planes(g["torso_img"]), "bg_img": reference_planes(bg_bytes)}
    for inputs in ((on_device(img), on_device(seg)), (img, seg)):
        got = source_conditions(*inputs)
        assert set(got) == set(want)
        for k in want:
            assert got[k].is_cuda and bits_equal(got[k], want[k]), k
    H, W = img.shape[:2]
    assert tuple(got["segmap"].shape) == (1, 6, H, W) and tuple(got["bg_img"].shape) == (1, 3, H, W)
    given = imgs[0][::-1].copy()                                       # a background image of the caller's
    got = source_conditions(on_device(img), on_device(seg), bg_image=on_device(given))
    assert bits_equal(got["bg_img"], reference_planes(given)) and bits_equal(got["ref_torso_img"], want["ref_torso_img"])


def test_head_image_and_planes_on_every_byte():
    from real3dportrait_amd import head_image, source_to_planes
    _, imgs, segs, _, _ = case_of("7_45x39_tail")
    want_img, want_mask = R.head_image(imgs[0], segs[0])
    got_img, got_mask = head_image(on_device(imgs[0]), on_device(segs[0]))
    assert got_mask.dtype == torch.bool and tuple(got_mask.shape) == want_mask.shape
    assert np.array_equal(got_img.cpu().numpy(), want_img) and np.array_equal(got_mask.cpu().numpy(), want_mask)
    host_img, host_mask = head_image(imgs[0], segs[0])
    assert np.array_equal(host_img, want_img) and np.array_equal(host_mask, want_mask) and host_mask.dtype == bool
    for H, W in ((16, 16), (1, 256), (256, 1), (19, 27)):               # every byte, the vector path and the scalar one with a tail
        img = (np.arange(H * W * 3, dtype=np.int64).reshape(H, W, 3) * 7 % 256).astype(np.uint8)
        assert len(np.unique(img)) == 256 or H * W * 3 < 256
        assert bits_equal(source_to_planes(on_device(img)), reference_planes(img))
    img = np.arange(256, dtype=np.uint8).repeat(3).reshape(16, 16, 3)
    assert bits_equal(source_to_planes(on_device(img)), reference_planes(img))
    seg = np.zeros((6, 16, 16), np.uint8)
    seg[2, :8], seg[0, 8:] = 1, 1
    torso_only = img.copy()
    torso_only[8:] = 0
    assert bits_equal(source_to_planes(on_device(img), on_device(seg), classes=1 << 2 | 1 << 4), reference_planes(torso_only))


def test_chunking_and_streams_do_not_change_a_bit():
    from real3dportrait_amd import extract_background, inpaint_torso_job, nearest_seed
    _, imgs, segs, res, want = case_of("5_128_b3")
    mask = on_device((segs[:, 0] == 0).astype(np.uint8))
    d2, index = nearest_seed(mask)
    for b in range(3):                            # the three frames in one call, or the transform in three single-frame calls
        d2_b, index_b = nearest_seed(mask[b])
        assert torch.equal(d2_b, d2[b]) and torch.equal(index_b, index[b]), b
    frames, maps = [on_device(f) for f in imgs], [on_device(s) for s in segs]
    pick = [0] * 11
    pick[5], pick[10] = 1, 2
    first = extract_background([frames[b] for b in pick], [maps[b] for b in pick])
    torso = inpaint_torso_job(frames[0], maps[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        d2_s, index_s = nearest_seed(mask)
        second = extract_background([frames[b] for b in pick], [maps[b] for b in pick])
        torso_s = inpaint_torso_job(frames[0], maps[0])
    side.synchronize()
    assert torch.equal(d2_s, d2) and torch.equal(index_s, index) and torch.equal(second, first)
    assert all(torch.equal(a, b) for a, b in zip(torso_s, torso))
    assert np.array_equal(first.cpu().numpy(), res["out"]) and np.array_equal(torso[2].cpu().numpy(), want[2])
    again = extract_background([frames[b] for b in pick], [maps[b] for b in pick])                        # and from run to run
    assert torch.equal(again, first)


def test_patch_segment_imgs_swaps_exactly_the_two_names_and_they_run():
    from real3dportrait_amd import patch_segment_imgs
    _, imgs, segs, res, want = case_of("1_96")
    ref = lambda *a, **k: "reference"
    mod = types.SimpleNamespace(inpaint_torso_job=ref, extract_background=ref, blink_eye_for_secc=ref, load_img_to_512_hwc_array=ref)
    before = dict(vars(mod))
    assert patch_segment_imgs(mod) is mod
    assert {k for k, v in vars(mod).items() if before[k] is not v} == {"inpaint_torso_job", "extract_background"}
    inpaint_torso_img, _, _, _ = mod.inpaint_torso_job(imgs[0], segs[0])          # as real3d_infer.py:251 and :255 call them
    bg_img = mod.extract_background([imgs[0]], [segs[0]], 'knn')
    assert np.array_equal(inpaint_torso_img, want[0]) and np.array_equal(bg_img, res["out"])


def test_source_conditions_enters_the_library_five_times():
    """per call one torso job, one background and three conversions to planes; four with a background image given."""
    from real3dportrait_amd import _lib
    from real3dportrait_amd.source_conditions import source_conditions
    _, imgs, segs, _, _ = case_of("1_96")
    img, seg = on_device(imgs[0]), on_device(segs[0])
    source_conditions(img, seg)                   # the workspace of this size and stream exists from here on
    with _lib.counting() as calls:
        source_conditions(img, seg)
    assert sorted(name for name, _ in calls) == ["r3d_source_background", "r3d_source_to_planes", "r3d_source_to_planes", "r3d_source_to_planes",
                                                 "r3d_source_torso"]
    with _lib.counting() as calls:
        source_conditions(img, seg, bg_image=img)
    assert sorted(name for name, _ in calls) == ["r3d_source_to_planes", "r3d_source_to_planes", "r3d_source_to_planes", "r3d_source_torso"]
