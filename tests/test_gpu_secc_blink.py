"""GPU: the HIP blink edit (real3dportrait_amd/edit_secc.py, r3d_secc_blink) against the reference function's recorded
outputs (tests/golden/blink_*.npz: equal up to the documented choice among equidistant face pixels) and against the NumPy restatement
tests/blink_ref.py, which makes the kernel's choice: bit for bit at every pixel.  Everything is integer or correctly rounded
arithmetic, so there is no tolerance anywhere in this file."""
import functools
import random

import numpy as np
import pytest
import torch

from conftest import load_golden
import blink_ref as R
from real3dportrait_amd import _lib, apply_periodic_blink, blink_eye_for_secc, blink_frames, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDENS = ["blink_a_64", "blink_b_64x96", "blink_c_96x64", "blink_d_128_crossing", "blink_e_96_zero_channel"]
# name -> the map: sizes where the indexing can go wrong, and the cases worked out by hand in tests/test_secc_blink_host.py
MAPS = {"synth_16": lambda: synth.synth_secc_eyes(16, 16, 3),                       # status 2: holes of two pixels, no face pixel left
        "hand_16": lambda: R.hand_map(16, 16, [(5, 5), (5, 9)]),                    # the smallest size, edited; P reaches row 1 and column 1
        "synth_48x80": lambda: synth.synth_secc_eyes(48, 80, 3),
        "synth_80x48": lambda: synth.synth_secc_eyes(80, 48, 3),
        "synth_128_crossing": lambda: synth.synth_secc_eyes(128, 128, 6, crossing=True),
        "synth_67x53": lambda: synth.synth_secc_eyes(67, 53, 2),                    # odd sizes: h // 4, w // 4 * 3 round
        "hand_box": lambda: R.hand_map(32, 32, [(10, 10), (10, 20)]),
        "hand_erosion": lambda: R.hand_map(32, 32, [(9, 9), (12, 13), (10, 20)]),
        "hand_equality": lambda: R.hand_map(32, 32, [(10, 10), (11, 10), (10, 20)]),
        "no_right_hole": lambda: synth.synth_secc_eyes(64, 64, 3, right_hole=False),
        "a": lambda: synth.synth_secc_eyes(64, 64, 3), "b": lambda: synth.synth_secc_eyes(64, 64, 4),
        "c": lambda: synth.synth_secc_eyes(64, 64, 5, crossing=True), "d": lambda: synth.synth_secc_eyes(64, 64, 6, zero_channel=4)}


@functools.lru_cache(maxsize=None)
def image(name):
    img = load_golden(name)["img"] if name in GOLDENS else MAPS[name]()
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def reference(name, p):
    """tests/blink_ref.py on the named map: computed once, shared, never written."""
    res = R.blink(image(name), p)
    res["out"].setflags(write=False)
    return res


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)          # a copy: the cached arrays are read-only


def run_one(name, p):
    """(out [3, h, w] as NumPy, status) of one map through the batched entry point, which does not raise on degenerate maps."""
    clip = dev(image(name))[None].clone()
    status = blink_frames(clip, [0], [p])
    return clip[0].cpu().numpy(), int(status.item())


@pytest.mark.parametrize("name", GOLDENS)
def test_golden_cases(name):
    g = load_golden(name)
    for p, q in zip(g["p"], g["q"]):
        p = float(p)
        out = blink_eye_for_secc(dev(g["img"]), p)
        assert out.device == torch.device(DEV) and out.dtype == torch.float32 and tuple(out.shape) == g["img"].shape
        out = out.cpu().numpy()
        ref = reference(name, p)
        golden = R.dequantise(q.astype(np.int64))
        tie = ref["tie"]
        outside = int((out != golden).any(axis=0)[~tie].sum())
        got_q = np.round((out.astype(np.float64) + 1) * 127.5).astype(np.int64).transpose(1, 2, 0)
        off = sum(1 for (r, c), cand in ref["cands"].items() if not (cand == got_q[r, c]).all(axis=1).any())
        own = int((out != ref["out"]).any(axis=0).sum())
        print("%s p %.2f: %d ties; %d pixels differ from the reference outside them, %d tie pixels off the candidates, %d pixels differ from "
              "the restatement" % (name, p, tie.sum(), outside, off, own))
        assert outside == 0 and off == 0                         # the reference function, up to its kd-tree's choice on ties
        assert np.array_equal(R.dequantise(got_q), out)          # exactly 8-bit
        assert own == 0                                          # the restatement with the lowest (row, col): every pixel, ties included


@pytest.mark.parametrize("name", ["synth_16", "hand_16", "synth_48x80", "synth_80x48", "synth_128_crossing", "synth_67x53", "hand_box",
                                  "hand_erosion", "hand_equality", "no_right_hole"])
def test_sizes_and_hand_cases_are_bit_identical_to_the_restatement(name):
    for p in (0.0, 0.36, 0.5, 1.0):
        ref = reference(name, p)
        out, status = run_one(name, p)
        diff = int((out != ref["out"]).any(axis=0).sum())
        print("%s p %.2f: status %d (restatement %d), %d pixels differ, %d edited" % (name, p, status, ref["status"], diff,
                                                                                     0 if ref["B"] is None else ref["B"].sum()))
        assert status == ref["status"] and diff == 0
    assert reference("synth_16", 1.0)["status"] == 2 and reference("no_right_hole", 1.0)["status"] == 1
    assert reference("hand_16", 0.5)["status"] == 0 and reference("hand_16", 0.5)["B"].sum() > 0


def batched_clip():
    """[6, 3, 64, 64]: frames 0 .. 3 four different maps, 4 the map without a right hole, 5 not selected."""
    names = ["a", "b", "c", "d", "no_right_hole", "a"]
    return names, np.stack([image(n) for n in names])


def test_batched_call_equals_the_per_frame_calls():
    names, clip_np = batched_clip()
    order, pct = [2, 4, 0, 3, 1], {0: 0.0, 1: 0.36, 2: 0.75, 3: 1.0, 4: 0.5}
    clip = dev(clip_np).clone()
    status = blink_frames(clip, order, [pct[j] for j in order])
    assert status.dtype == torch.int32 and status.device == torch.device(DEV)
    assert status.cpu().tolist() == [0, 1, 0, 0, 0]
    got = clip.cpu().numpy()
    for j in range(5):
        ref = reference(names[j], pct[j])
        assert np.array_equal(got[j], ref["out"]), j
        single, st = run_one(names[j], pct[j])
        assert np.array_equal(got[j], single) and st == ref["status"], j
    assert np.array_equal(got[4], R.dequantise(R.quantise(clip_np[4])))          # degenerate: quantised only
    assert np.array_equal(got[5], clip_np[5])                                    # not selected: untouched, bit for bit
    assert reference("b", 0.36)["B"].sum() > 50 and not np.array_equal(got[1], R.dequantise(R.quantise(clip_np[1])))


def test_side_stream_and_repeated_call_are_bit_identical():
    names, clip_np = batched_clip()
    idx, pct = [0, 1, 2, 3, 4], [1.0, 0.75, 0.36, 0.5, 1.0]
    base = dev(clip_np)
    first = base.clone()
    blink_frames(first, idx, pct)
    again = base.clone()
    blink_frames(again, idx, pct)
    side = base.clone()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        st = blink_frames(side, idx, pct)
    stream.synchronize()
    assert torch.equal(first, again) and torch.equal(first, side) and st.cpu().tolist() == [0, 0, 0, 0, 1]
    assert np.array_equal(first[0].cpu().numpy(), reference("a", 1.0)["out"])


def test_out_leaves_the_callers_tensor_untouched():
    names, clip_np = batched_clip()
    clip = dev(clip_np)
    out = torch.full_like(clip, 7.0)
    status = blink_frames(clip, [3, 0], [1.0, 0.36], out=out)
    assert status.cpu().tolist() == [0, 0]
    assert np.array_equal(clip.cpu().numpy(), clip_np)
    got = out.cpu().numpy()
    assert np.array_equal(got[3], reference("d", 1.0)["out"]) and np.array_equal(got[0], reference("a", 0.36)["out"])
    for j in (1, 2, 4, 5):
        assert np.array_equal(got[j], clip_np[j]), j          # the frames not listed are copies
    src = dev(image("a"))
    keep = src.clone()
    res = blink_eye_for_secc(src, 1.0)
    assert torch.equal(src, keep) and res.data_ptr() != src.data_ptr()


def test_rejected_frames_are_left_alone():
    """Percentages outside [0, 1] reach the device through blink_frames; indices outside [0, T) only through the C entry point."""
    names, clip_np = batched_clip()
    clip = dev(clip_np).clone()
    status = blink_frames(clip, [0, 1, 2, 3], [1.5, float("nan"), -0.25, 1.0])
    assert status.cpu().tolist() == [3, 3, 3, 0]
    got = clip.cpu().numpy()
    assert np.array_equal(got[:3], clip_np[:3]) and np.array_equal(got[3], reference("d", 1.0)["out"])
    clip = dev(clip_np).clone()
    T, _, H, W = clip.shape
    idx = torch.tensor([-1, T, 2, 1 << 30], dtype=torch.int32, device=DEV)
    pct = torch.tensor([0.5, 0.5, 0.75, 0.5], dtype=torch.float64, device=DEV)
    status = torch.full((4,), -7, dtype=torch.int32, device=DEV)
    lib = _lib.load()
    ws = torch.empty(lib.r3d_secc_blink_workspace_bytes(4, H, W), dtype=torch.uint8, device=DEV)
    rc = lib.r3d_secc_blink(_lib.ptr(clip), T, H, W, _lib.ptr(idx), _lib.ptr(pct), 4, _lib.ptr(clip), _lib.ptr(status), _lib.ptr(ws),
                            ws.numel(), _lib.stream_ptr())
    assert rc == 0 and status.cpu().tolist() == [3, 3, 0, 3]
    got = clip.cpu().numpy()
    assert np.array_equal(got[2], reference("c", 0.75)["out"])
    for j in (0, 1, 3, 4, 5):
        assert np.array_equal(got[j], clip_np[j]), j


def test_blink_eye_for_secc_raises_on_degenerate_maps():
    with pytest.raises(ValueError, match="prior regions"):
        blink_eye_for_secc(dev(image("no_right_hole")), 0.5)
    with pytest.raises(ValueError, match="no face pixel left"):
        blink_eye_for_secc(dev(image("synth_16")), 1.0)
    out = blink_eye_for_secc(dev(image("no_right_hole")), 0)          # 0 only quantises, as in the reference
    assert np.array_equal(out.cpu().numpy(), R.dequantise(R.quantise(image("no_right_hole"))))
    out = blink_eye_for_secc(dev(image("a")))                         # the default is 0.5
    assert np.array_equal(out.cpu().numpy(), reference("a", 0.5)["out"])


def test_apply_periodic_blink_equals_the_transcribed_loop():
    clip_np = np.stack([synth.synth_secc_eyes(32, 32, k % 7) for k in range(130)])
    want = R.transcribed_loop(clip_np, random.Random(5))
    clip = dev(clip_np).clone()
    edits, status = apply_periodic_blink(clip, rng=random.Random(5))
    got = clip.cpu().numpy()
    frames = [j for j, _ in edits]
    assert 8 <= len(frames) <= 16 and frames[0] == 0 and 125 in frames and 129 not in frames
    assert status.cpu().tolist() == [0] * len(frames)
    assert np.array_equal(got, want)
    untouched = [j for j in range(130) if j not in frames]
    assert np.array_equal(got[untouched], clip_np[untouched])
    assert sum(1 for j in frames if not np.array_equal(got[j], R.dequantise(R.quantise(clip_np[j])))) >= len(frames) - 2
