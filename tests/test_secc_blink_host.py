"""CPU: the host side of the HIP blink edit (real3dportrait_amd/edit_secc.py, r3d_secc_blink of include/r3d_hip.h).

The NumPy restatement of the rule (tests/blink_ref.py) against the reference function's recorded outputs (tests/golden/blink_*.npz,
made by tests/golden/make_golden_blink.py) and on cases worked out by hand, the blink schedule against a transcription of the
reference's loop, the symbols, the workspace size, the argument checks (which run before any HIP call) and the kernels' registers."""
import ctypes
import os
import random

import numpy as np
import pytest

from conftest import ROOT, load_golden
import blink_ref as R
from real3dportrait_amd import synth

GOLDENS = ["blink_a_64", "blink_b_64x96", "blink_c_96x64", "blink_d_128_crossing", "blink_e_96_zero_channel"]


@pytest.mark.parametrize("name", GOLDENS)
def test_restatement_against_the_reference_function(name):
    """Bit for bit outside the tie mask; inside it the reference's colour is one of the equidistant candidates'."""
    g = load_golden(name)
    H, W, seed, crossing, zero_channel = (int(v) for v in g["spec"])
    assert np.array_equal(g["img"], synth.synth_secc_eyes(H, W, seed, crossing=bool(crossing), zero_channel=zero_channel))
    for p, q in zip(g["p"], g["q"]):
        res = R.blink(g["img"], float(p))
        outside, bad = R.matches_up_to_ties(res, q)
        edited = 0 if res["B"] is None else int(res["B"].sum())
        print("%s p %.2f: %d edited, %d ties, %d differ outside the ties, %d ties off the candidates" % (name, p, edited, res["tie"].sum(), outside, bad))
        assert res["status"] == 0 and outside == 0 and bad == 0
        assert np.array_equal(res["out"][:, ~res["tie"]], R.dequantise(q.astype(np.int64))[:, ~res["tie"]])
        if p == 0:
            assert edited == 0 and np.array_equal(res["q"], R.quantise(g["img"]))
        else:
            assert edited >= 100 and 0 < res["tie"].sum() < edited / 4


def test_synth_secc_eyes():
    img = synth.synth_secc_eyes(64, 64, 3)
    assert img.shape == (3, 64, 64) and img.dtype == np.float32 and img.min() == -1.0 and img.max() <= 1.0
    res = R.blink(img, 1.0)
    assert (int(res["E"].sum()), int(res["F"].sum()), int(res["B"].sum())) == (44, 16, 314)
    assert int(R.blink(synth.synth_secc_eyes(32, 32, 3), 1.0)["E"].sum()) >= 10
    z = R.quantise(synth.synth_secc_eyes(96, 96, 3, zero_channel=6))
    one_zero = ((z == 0).sum(-1) == 1)
    assert 1 <= one_zero.sum() <= 6                                      # a face pixel with exactly one channel at 0
    c = R.blink(synth.synth_secc_eyes(128, 128, 6, crossing=True), 0.5)["E"]
    assert c[:, 63].any() and c[:, 64].any()                             # the hole crosses the middle column
    assert R.blink(synth.synth_secc_eyes(64, 64, 3, right_hole=False), 0.5)["status"] == 1
    assert not np.array_equal(img, synth.synth_secc_eyes(64, 64, 4))


def test_hand_box_ends_are_exclusive_and_empty_columns_contribute_nothing():
    """32 x 32: L = rows 8 .. 15 x cols 8 .. 15, R = the same rows x cols 16 .. 23.  Eye pixels (10, 10) and (10, 20): min_h = max_h = 10,
    P = rows [6, 14) x (cols [6, 14) u cols [16, 24)).  Columns 14 and 15 lie between the two boxes: cnt = 0, nothing is edited there."""
    img = R.hand_map(32, 32, [(10, 10), (10, 20)])
    for p in (0.25, 1.0):
        res = R.blink(img, p)
        want = np.zeros((32, 32), bool)
        want[6:14, 6:14] = want[6:14, 16:24] = True
        assert res["status"] == 0 and np.array_equal(res["P"], want)
        assert not res["P"][14].any() and not res["P"][:, 14].any() and not res["P"][:, 24].any() and res["P"][13, 13] and res["P"][13, 23]
        assert not res["M"][:, 14:16].any() and not res["B"][:, 14:16].any()
        q0 = R.quantise(img)
        assert np.array_equal(res["q"][~res["B"]], q0[~res["B"]])          # only B is edited
        assert res["B"].sum() > 0 and (res["B"] & ~res["M"]).sum() == 0


def test_hand_erosion_boundary():
    """Eye pixels (9, 9) and (12, 13) (and (10, 20) on the right): P = rows [5, 16) x cols [5, 17) on the left.  The face pixel (5, 12) is at
    d^2 = 16 + 9 = 25 from (9, 9): removed.  (14, 8) is at d^2 = 25 + 1 = 26 from (9, 9) and 4 + 25 = 29 from (12, 13): it stays."""
    img = R.hand_map(32, 32, [(9, 9), (12, 13), (10, 20)])
    res = R.blink(img, 0.5)
    assert res["status"] == 0 and res["P"][5, 12] and res["P"][14, 8]
    assert not res["F"][5, 12] and res["M"][5, 12]
    assert res["F"][14, 8] and not res["M"][14, 8]
    eyes = np.stack(np.nonzero(res["E"]), 1)
    for r, c in zip(*np.nonzero(res["P"] & ~res["E"])):
        d2 = ((eyes - (r, c)) ** 2).sum(1).min()
        assert res["F"][r, c] == (d2 > 25), (r, c, d2)


def test_hand_row_equal_to_lo_blinks():
    """Eye pixels (10, 10), (11, 10) and (10, 20): P rows [6, 15).  Column 10 is within 5 of an eye pixel on all nine rows 6 .. 14: cnt = 9,
    mean = 10, min = 6, max = 14.  p = 0.5 (exact in binary): lo = 5 + 3 = 8 and hi = 5 + 7 = 12, integers: rows 8 and 12 blink (<=, >=)."""
    img = R.hand_map(32, 32, [(10, 10), (11, 10), (10, 20)])
    res = R.blink(img, 0.5)
    assert res["status"] == 0 and res["M"][6:15, 10].all() and res["M"][:, 10].sum() == 9
    assert np.nonzero(res["B"][:, 10])[0].tolist() == [6, 7, 8, 12, 13, 14]
    # every edited pixel carries the colour of a pixel of F, the nearest with the lowest (row, col)
    fxy = np.stack(np.nonzero(res["F"]), 1)
    q0 = R.quantise(img)
    for r, c in zip(*np.nonzero(res["B"])):
        d2 = ((fxy - (r, c)) ** 2).sum(1)
        sr, sc = min((int(y), int(x)) for (y, x), d in zip(fxy, d2) if d == d2.min())
        assert np.array_equal(res["q"][r, c], q0[sr, sc])


def test_hand_degenerate_maps():
    img = R.hand_map(32, 32, [(10, 10)])                                   # nothing in R
    res = R.blink(img, 0.5)
    assert res["status"] == 1 and np.array_equal(res["q"], R.quantise(img)) and np.array_equal(res["out"], R.dequantise(R.quantise(img)))
    assert R.blink(R.hand_map(32, 32, [(10, 20)]), 0.5)["status"] == 1     # nothing in L
    img = synth.synth_secc_eyes(16, 16, 3)                                 # holes of two pixels; every face pixel of P is within 5 of one
    res = R.blink(img, 1.0)
    assert res["status"] == 2 and res["E"].sum() == 4 and not res["F"].any() and np.array_equal(res["q"], R.quantise(img))
    ok = R.blink(R.hand_map(16, 16, [(5, 5), (5, 9)]), 0.5)                # the smallest size can still be edited: (1, 1) is at d^2 = 32
    assert ok["status"] == 0 and ok["F"][1, 1] and ok["B"].sum() > 0
    assert R.blink(img, 0.0)["status"] == 0                               # p = 0 only quantises, whatever the map
    for bad in ((15, 16), (16, 15), (4097, 16)):
        with pytest.raises(ValueError, match="map size"):
            R.blink(np.zeros((3,) + bad, np.float32), 0.5)


def reference_loop_edits(T, rng):
    """inference/real3d_infer.py:411-426, transcribed literally, recording the edits instead of performing them."""
    edits = []
    for i in range(T):
        if i % 125 == 0:
            blink_dur_frames = rng.randint(8, 12)
            for offset in range(blink_dur_frames):
                j = offset + i
                close_percent = -4 / blink_dur_frames ** 2 * offset ** 2 + 4 / blink_dur_frames * offset
                if j >= T - 1:
                    break
                edits.append((j, close_percent))
    return edits


@pytest.mark.parametrize("T", [1, 2, 9, 125, 126, 137, 251, 300])
def test_blink_schedule_is_the_reference_loop(T):
    from real3dportrait_amd import blink_schedule
    random.seed(0)
    want = reference_loop_edits(T, random)
    state = random.getstate()
    random.seed(0)
    got = blink_schedule(T)
    assert got == want and random.getstate() == state
    assert all(j < T - 1 and 0.0 <= p <= 1.0 for j, p in got) and len({j for j, _ in got}) == len(got)
    own = random.Random(7)
    assert blink_schedule(T, rng=own) == reference_loop_edits(T, random.Random(7))
    if T <= 2:
        assert got == ([] if T == 1 else [(0, 0.0)])
    with pytest.raises(ValueError, match="period_frames"):
        blink_schedule(T, period_frames=12)


def test_symbols_are_declared_exported_and_bound():
    from real3dportrait_amd import _lib
    import real3dportrait_amd
    lib = _lib.load()
    assert lib.r3d_version() == _lib.ABI_VERSION
    header = open(os.path.join(ROOT, "include", "r3d_hip.h")).read()
    for name in ("r3d_secc_blink_workspace_bytes", "r3d_secc_blink"):          # (header against table: tests/test_abi.py)
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert "r3d_debug_secc_blink" in _lib.OPTIONAL_SIGNATURES and "r3d_debug_secc_blink" not in header
    assert len(_lib.OPTIONAL_SIGNATURES["r3d_debug_secc_blink"][1]) == len(_lib.SIGNATURES["r3d_secc_blink"][1]) + 1
    from real3dportrait_amd import edit_secc
    for name in ("blink_eye_for_secc", "blink_frames", "blink_schedule", "apply_periodic_blink", "patch_blink"):
        assert getattr(real3dportrait_amd, name) is getattr(edit_secc, name), name

    class Module:
        blink_eye_for_secc = None
    assert edit_secc.patch_blink(Module) is Module and Module.blink_eye_for_secc is edit_secc.blink_eye_for_secc


def workspace_bytes(F, H, W):
    """The layout of r3d_secc_blink.hip: 256 bytes of bounds and list lengths per frame, a packed word per pixel, two coordinate lists and
    one byte of masks per pixel of the band, rows [H / 4 - 4, H / 2 + 4); each part rounded up to 256 bytes."""
    r = lambda n: (n + 255) // 256 * 256
    cap = (H // 2 - H // 4 + 8) * W
    return F * 256 + r(F * H * W * 4) + 2 * r(F * cap * 4) + r(F * cap)


def test_workspace_bytes():
    from real3dportrait_amd import _lib
    lib = _lib.load()
    for F, H, W in ((1, 16, 16), (10, 512, 512), (3, 48, 80), (7, 17, 19), (65535, 16, 16), (2, 4096, 4096)):
        assert lib.r3d_secc_blink_workspace_bytes(F, H, W) == workspace_bytes(F, H, W), (F, H, W)
    assert lib.r3d_secc_blink_workspace_bytes(10, 512, 512) < 20 << 20
    for bad in ((0, 64, 64), (-1, 64, 64), (65536, 64, 64), (1, 15, 64), (1, 64, 15), (1, 4097, 64), (1, 64, 4097), (1, 0, 0), (1, -64, 64)):
        assert lib.r3d_secc_blink_workspace_bytes(*bad) == 0, bad


def test_c_entry_point_rejects_bad_arguments_without_a_gpu():
    from real3dportrait_amd import _lib
    lib = _lib.load()
    P = lambda k: ctypes.c_void_p(k << 32)              # never dereferenced: validation fails first
    err = lambda: lib.r3d_last_error()
    need = lib.r3d_secc_blink_workspace_bytes(3, 64, 96)

    def call(secc=P(1), T=5, H=64, W=96, idx=P(2), pct=P(3), F=3, out=P(1), status=P(4), ws=P(8), ws_bytes=need, dbg=None):
        if dbg is not None:
            return lib.r3d_debug_secc_blink(secc, T, H, W, idx, pct, F, out, status, ws, ws_bytes, dbg, None)
        return lib.r3d_secc_blink(secc, T, H, W, idx, pct, F, out, status, ws, ws_bytes, None)

    for k in ("secc", "idx", "pct", "out", "status"):
        assert call(**{k: None}) == -1 and b"NULL pointer" in err(), k
    for H, W in ((15, 96), (64, 15), (4097, 96), (64, 4097), (0, 0), (-64, 96)):
        assert call(H=H, W=W, ws_bytes=1 << 62) == -1 and b"map size" in err(), (H, W)
    for T, F in ((5, 0), (5, -1), (5, 6), (0, 1), (70000, 65536)):
        assert call(T=T, F=F, ws_bytes=1 << 62) == -1 and b"selected frames" in err(), (T, F)
    assert call(ws=None) == -2 and b"NULL workspace" in err()
    assert call(ws_bytes=need - 1) == -2 and b"needed" in err()
    assert call(ws_bytes=0) == -2 and b"needed" in err()
    assert call(ws=ctypes.c_void_p((8 << 32) + 4)) == -2 and b"aligned" in err()
    assert call(dbg=-1) == -1 and b"test-hook" in err()
    assert call(dbg=32) == -1 and b"test-hook" in err()


def test_python_wrappers_refuse_malformed_input_before_the_library():
    import torch
    from real3dportrait_amd import apply_periodic_blink, blink_eye_for_secc, blink_frames
    clip = torch.zeros(4, 3, 32, 32)
    with pytest.raises(ValueError, match=r"\[3, h, w\]"):
        blink_eye_for_secc(torch.zeros(1, 3, 32, 32))
    with pytest.raises(ValueError, match=r"\[3, h, w\]"):
        blink_eye_for_secc(torch.zeros(4, 32, 32))
    for shape in ((3, 15, 32), (3, 32, 15), (3, 4097, 16)):
        with pytest.raises(ValueError, match="map size"):
            blink_eye_for_secc(torch.zeros(shape))
    for p in (-0.1, 1.5, float("nan")):
        with pytest.raises(AssertionError):
            blink_eye_for_secc(torch.zeros(3, 32, 32), p)
    with pytest.raises(ValueError, match="GPU only"):
        blink_eye_for_secc(torch.zeros(3, 32, 32), 0.5)
    with pytest.raises(ValueError, match=r"\[T, 3, H, W\]"):
        blink_frames(torch.zeros(3, 32, 32), [0], [0.5])
    with pytest.raises(ValueError, match="map size"):
        blink_frames(torch.zeros(4, 3, 8, 32), [0], [0.5])
    with pytest.raises(ValueError, match="same number"):
        blink_frames(clip, [0, 1], [0.5])
    with pytest.raises(ValueError, match="same number"):
        blink_frames(clip, [], [])
    with pytest.raises(ValueError, match="listed twice"):
        blink_frames(clip, [1, 2, 1], [0.5, 0.5, 0.5])
    for idx in ([4], [-1], [0, 7]):
        with pytest.raises(ValueError, match="frame indices"):
            blink_frames(clip, idx, [0.5] * len(idx))
    with pytest.raises(ValueError, match="contiguous float32"):
        blink_frames(clip.double(), [0], [0.5])
    with pytest.raises(ValueError, match="contiguous float32"):
        blink_frames(torch.zeros(4, 3, 32, 64)[..., ::2], [0], [0.5])
    with pytest.raises(ValueError, match="out must be"):
        blink_frames(clip, [0], [0.5], out=torch.zeros(4, 3, 32, 33))
    with pytest.raises(ValueError, match="GPU only"):
        blink_frames(clip, torch.tensor([0, 2]), torch.tensor([0.5, 1.0]))
    with pytest.raises(ValueError, match=r"\[T, 3, H, W\]"):
        apply_periodic_blink(torch.zeros(3, 32, 32))
    assert apply_periodic_blink(torch.zeros(1, 3, 32, 32), rng=random.Random(0)) == ([], None)          # one frame: the last is never edited
    assert clip.abs().sum() == 0


def test_blink_kernels_registers_and_scratch():
    """No scratch and no spills; at most 64 VGPRs, so that eight waves fit a SIMD (512 registers per lane): the fill kernel hides its
    LDS and list latency behind other waves, not behind registers."""
    from test_render_kernel_resources import _kernel_metadata
    from real3dportrait_amd import _lib
    meta = _kernel_metadata(_lib.LIB_PATH)
    names = sorted(k for k in meta if "5blink" in k)
    assert len(names) == 4 and all([n for n in names if kernel in n] for kernel in ("quantise_bounds", "erode", "columns", "fill")), names
    for k in names:
        print(k, "vgpr", meta[k]["vgpr_count"], "sgpr", meta[k]["sgpr_count"], "lds", meta[k]["group_segment_fixed_size"])
        assert int(meta[k]["private_segment_fixed_size"]) == 0, (k, meta[k])
        assert int(meta[k]["vgpr_spill_count"]) == 0 and int(meta[k]["sgpr_spill_count"]) == 0, (k, meta[k])
        assert int(meta[k]["vgpr_count"]) <= 64, (k, meta[k])
    fill = [n for n in names if "fill" in n][0]
    assert int(meta[fill]["group_segment_fixed_size"]) == 512 * 4 + 4 * 64 * 8          # the tile and the four partial minima per pixel
