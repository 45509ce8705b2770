"""CPU: the host side of the HIP output video frames (real3dportrait_amd/video_frames.py, r3d_video_depth_range / r3d_video_compose_debug
of include/r3d_hip_video.h).

The oracle (tests/video_frames_ref.py) is the reference's operator sequence, inference/real3d_infer.py:495-521, on torch-CPU and NumPy.
forward_secc2video itself cannot be called here or anywhere in the suite: it needs the generator, its checkpoints, imageio and ffmpeg.
What is checked without a GPU: the oracle reproduces every recorded fixture; the five properties of those lines that the kernel's
comments state, each from the operators themselves; the header against the binding table and the library's exports; every argument
refusal of the two entry points, which run before any HIP call; the Python functions' type, shape, dtype and contiguity errors."""
import ctypes
import glob
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, load_golden
import video_frames_ref as R

CASES = ("a_t3_32", "b_t2_12x20", "c_constant_depth", "d_nan_depth")
MINUS_ONE_CODES = [1, 2, 5, 9, 10, 13, 17, 18, 21, 25, 26, 29, 33, 34, 41, 42, 49, 50, 57, 58]


def test_every_fixture_is_listed_and_small():
    names = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "video_frames_*.npz")))
    assert names == sorted("video_frames_" + c for c in CASES)
    assert all(os.path.getsize(os.path.join(GOLDEN, n + ".npz")) <= 524288 for n in names)


@pytest.mark.parametrize("case", CASES)
def test_oracle_reproduces_the_fixture(case):
    g = load_golden("video_frames_" + case)
    out = R.oracle_of(g)
    T, _, H, W = g["imgs"].shape
    assert out.dtype == np.uint8 and out.shape == (T, H, 5 * W, 3) and np.array_equal(out, g["concat_debug"])
    assert np.array_equal(R.final(torch.from_numpy(g["imgs"])), g["final"])
    depth_panel = out[:, :, 3 * W:4 * W]
    if case in ("c_constant_depth", "d_nan_depth"):
        assert not depth_panel.any()                                    # 0 / 0, or a NaN through min(): NaN -> int -> uint8 is 0
    else:
        assert depth_panel.min() == 0 and depth_panel.max() == 255 and (depth_panel[..., 0] == depth_panel[..., 2]).all()
        # the clip's extremes lie in different frames: a per-frame normalisation would reach 0 and 255 in every frame
        assert depth_panel[0].max() < 255 and depth_panel[-1].min() > 0
    assert np.array_equal(out[:, :, :W], np.broadcast_to(out[:1, :, :W], (T, H, W, 3)))          # the ref panel is the same in every frame
    assert np.array_equal(out[:, :, 4 * W:], R.concat_debug(*(torch.from_numpy(g[k]) for k in R.ORDER))[:, :, 4 * W:])


def test_the_strip_is_quantised_in_fp64_and_the_final_mode_in_fp32():
    """Property 1: the fp64 and the fp32 quantisation of the same fp32 values differ, so the dtype of the strip is part of the result."""
    codes = R.SECC_CODES                                                 # the values next to a byte's boundary are where the two part
    x = torch.from_numpy(np.concatenate([codes, np.nextafter(codes, np.float32(2)), np.nextafter(codes, np.float32(-2))]))
    q32 = ((x + 1) / 2 * 255).int().numpy()
    q64 = ((x.double() + 1) / 2 * 255).int().numpy()
    print("fp32 and fp64 quantisation differ on %d of %d values next to the codes" % ((q32 != q64).sum(), len(x)))
    assert (q32 != q64).any() and np.abs(q32 - q64).max() == 1
    c = R.clip(21, 4, 8, 8, (8, 8), (8, 8), (8, 8))
    c["imgs"] = x.reshape(4, 3, 8, 8).numpy().copy()
    got = R.oracle_of(c)[:, :, 32:]
    assert np.array_equal(got, q64.reshape(4, 3, 8, 8).transpose(0, 2, 3, 1).astype(np.uint8))
    assert np.array_equal(R.final(torch.from_numpy(c["imgs"])), q32.reshape(4, 3, 8, 8).transpose(0, 2, 3, 1).astype(np.uint8))


def test_the_secc_panel_is_quantised_twice_and_loses_one_on_twenty_codes():
    """Property 2, from the operators: q / 127.5 - 1 in fp64, then (v + 1) / 2 * 255 truncated, maps 20 of the 256 codes to q - 1."""
    q = np.arange(256, dtype=np.int32)
    v = torch.from_numpy(q / 127.5 - 1)
    back = ((v.clamp(-1, 1) + 1) / 2 * 255).int().numpy()
    assert [int(k) for k in q[back != q]] == MINUS_ONE_CODES and np.array_equal(back[back != q], q[back != q] - 1)
    # and the first pass on the exact codes float32(k / 127.5 - 1) is fp32: add, then multiply
    first = ((torch.from_numpy(R.SECC_CODES) + 1) * 127.5).int().numpy()
    assert np.abs(first - q).max() <= 1
    c = R.clip(22, 1, 16, 16, (16, 16), (4, 4), (4, 4))
    c["drv_secc"][0, 0] = R.SECC_CODES.reshape(16, 16)
    got = R.oracle_of(c)[0, :, 16:32, 0].reshape(-1)
    assert np.array_equal(got, back[first].astype(np.uint8))


def test_nearest_is_the_legacy_rule():
    """Property 4: F.interpolate(x, (H, W)) picks min(floor(dst * (float(in) / float(out))), in - 1), the scale in fp32."""
    x = torch.arange(5, dtype=torch.float32).reshape(1, 1, 1, 5)
    assert F.interpolate(x, (1, 12)).reshape(-1).int().tolist() == [0, 0, 0, 1, 1, 2, 2, 2, 3, 3, 4, 4]
    for n_in, n_out in ((5, 12), (7, 20), (9, 12), (24, 20), (8, 32), (128, 512), (3, 7), (7, 3)):
        scale = np.float32(n_in) / np.float32(n_out)
        want = np.minimum(np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64), n_in - 1)
        x = torch.arange(n_in, dtype=torch.float32).reshape(1, 1, 1, n_in)
        assert np.array_equal(F.interpolate(x, (1, n_out)).reshape(-1).numpy().astype(np.int64), want), (n_in, n_out)


def test_depth_is_normalised_over_the_clip_and_a_nan_is_byte_zero():
    """Property 3."""
    c = R.clip(23, 3, 8, 8, (8, 8), (4, 4), (4, 4), "spread")
    whole = R.oracle_of(c)[:, :, 24:32]
    per_frame = np.concatenate([R.oracle_of({k: (v if k == "ref_gt_img" else v[t:t + 1]) for k, v in c.items()})[:, :, 24:32] for t in range(3)])
    assert not np.array_equal(whole, per_frame)
    mn, mx, nan = R.depth_min_max(torch.from_numpy(c["depth_imgs"]))
    assert (mn, mx, nan) == (np.float32(1.5), np.float32(3.75), False)
    c["depth_imgs"][2, 0, 1, 1] = np.nan
    out = R.oracle_of(c)
    assert not out[:, :, 24:32].any() and R.depth_min_max(torch.from_numpy(c["depth_imgs"]))[2]
    assert np.array_equal(out[:, :, :24], R.oracle_of(R.clip(23, 3, 8, 8, (8, 8), (4, 4), (4, 4), "spread"))[:, :, :24])          # the other panels do not see it


def test_symbols_are_declared_exported_and_bound():
    """The two entry points live in the companion header include/r3d_hip_video.h (tests/test_abi.py compares every declaration with the
    binding table and with what load() bound, and the header's macros with the package's constants); here what is this unit's own: the
    parameter counts, the ABI number and the package's names."""
    from real3dportrait_amd import _lib
    from abi import header_declarations
    import real3dportrait_amd
    lib = _lib.load()
    assert lib.r3d_version() == _lib.ABI_VERSION
    decls = header_declarations("r3d_hip_video.h")
    assert set(decls) == {"r3d_video_depth_range", "r3d_video_compose_debug"} <= set(_lib.SIGNATURES)
    assert [len(decls[n][1]) for n in ("r3d_video_depth_range", "r3d_video_compose_debug")] == [5, 18]
    from real3dportrait_amd import video_frames
    for name in ("depth_range", "compose_debug_frames", "clip_frames", "secc2video_frames", "write_video", "patch_secc2video"):
        assert getattr(real3dportrait_amd, name) is getattr(video_frames, name), name


def test_c_entry_points_reject_bad_arguments_without_a_gpu():
    from real3dportrait_amd import _lib
    lib = _lib.load()
    P = lambda k: ctypes.c_void_p(k << 32)              # never dereferenced: validation fails first
    at = lambda a: ctypes.c_void_p(a)
    err = lambda: lib.r3d_last_error()

    def rng(depth=P(1), count=1024, reset=0, state=P(2)):
        return lib.r3d_video_depth_range(depth, count, reset, state, None)

    def comp(ref=P(1), secc=P(2), hs=9, ws=24, raw=P(3), hr=5, wr=7, depth=P(4), hd=7, wd=5, image=P(5), n=2, H=12, W=20, panels=31,
             state=P(6), out=P(7)):
        return lib.r3d_video_compose_debug(ref, secc, hs, ws, raw, hr, wr, depth, hd, wd, image, n, H, W, panels, state, out, None)

    name = b"video_depth_range:"
    for k in ("depth", "state"):
        assert rng(**{k: None}) == -1 and name in err() and b"NULL pointer" in err(), k
    assert rng(count=0) == -1 and name in err() and b"must be positive" in err()
    for bad in (1 << 29, (1 << 29) + 1, 1 << 40):                       # 4 count >= 2^31
        assert rng(count=bad) == -1 and name in err() and b"2^31" in err(), bad
    assert rng(state=at((2 << 32) + 2)) == -1 and b"4-byte aligned" in err()
    assert rng(state=P(1)) == -1 and b"overlaps" in err()
    assert rng(state=at((1 << 32) + 4 * 1023)) == -1 and b"overlaps" in err()          # the last float
    assert rng(state=at((1 << 32) - 4 * 7)) == -1 and b"overlaps" in err()             # the state's last word on the first float

    name = b"video_compose_debug:"
    for k in ("ref", "secc", "raw", "depth", "image", "state", "out"):
        assert comp(**{k: None}) == -1 and name in err() and b"NULL pointer" in err(), k
    for k in ("hs", "ws", "hr", "wr", "hd", "wd", "n", "H", "W"):
        for bad in (0, -1):
            assert comp(**{k: bad}) == -1 and name in err() and b"must be positive" in err(), (k, bad)
    for bad in (0, -1, 32, 64):
        assert comp(panels=bad) == -1 and name in err() and b"panels" in err(), bad
    for bad in (1, 2, 3, 18, 22):
        assert comp(W=bad) == -1 and name in err() and b"multiple of 4" in err(), bad
    assert comp(H=(1 << 24) + 1, W=4, n=1) == -1 and b"2^24" in err()
    assert comp(n=1, H=4096, W=34956) == -1 and b"of output" in err() and b"2^31" in err()          # 15 n H W = 2^31 + 2 560
    assert comp(n=250, hs=1024, ws=1024) == -1 and b"panel 1" in err() and b"2^31" in err()
    assert comp(n=250, hr=1024, wr=1024) == -1 and b"panel 2" in err() and b"2^31" in err()
    # (ref, image and the depth, which is no larger than the frame, are at most 12 n H W bytes, below the output's 15 n H W: its rule covers them)
    for over in (dict(hd=13), dict(wd=21), dict(hd=24, wd=40)):                        # a depth image with pixels the resize drops
        assert comp(**over) == -1 and name in err() and b"every pixel used" in err(), over
    assert comp(panels=23, hd=13, wd=21, out=None) == -1 and b"NULL pointer" in err()  # (without the depth panel its size is not looked at)
    assert comp(out=at((7 << 32) + 2)) == -1 and b"4-byte aligned" in err()
    assert comp(state=at((6 << 32) + 1)) == -1 and b"4-byte aligned" in err()
    out_bytes = 15 * 2 * 12 * 20
    for k, nbytes in (("ref", 12 * 12 * 20), ("secc", 12 * 2 * 9 * 24), ("raw", 12 * 2 * 5 * 7), ("depth", 4 * 2 * 7 * 5), ("image", 12 * 2 * 12 * 20),
                      ("state", 32)):
        base = {"ref": 1, "secc": 2, "raw": 3, "depth": 4, "image": 5, "state": 6}[k] << 32
        assert comp(out=at(base)) == -1 and b"overlaps" in err(), k
        assert comp(out=at(base + nbytes - 4)) == -1 and b"overlaps" in err(), k       # the input's last dword
        assert comp(out=at(base - out_bytes + 4)) == -1 and b"overlaps" in err(), k    # the output's last dword on the input's first
    # a panel that is not selected is not looked at: its pointer may be NULL and its sizes anything
    assert comp(panels=23, depth=None, state=None, hd=0, wd=-3, out=None) == -1 and b"NULL pointer" in err()          # (out is the one defect)
    assert comp(panels=8, ref=None, secc=None, raw=None, image=None, hs=0, ws=0, hr=0, wr=0, W=6) == -1 and b"multiple of 4" in err()


def test_python_functions_refuse_before_the_library_is_entered():
    from real3dportrait_amd import _lib, video_frames as V
    c = {k: torch.from_numpy(v) for k, v in R.clip(31, 2, 8, 8, (8, 8), (4, 4), (4, 4)).items()}
    args = lambda **over: [over.get(k, c[k]) for k in R.ORDER]
    with _lib.counting() as calls:
        with pytest.raises(ValueError, match="GPU only"):
            V.compose_debug_frames(*args())
        with pytest.raises(ValueError, match="GPU only"):
            V.depth_range(c["depth_imgs"])
        with pytest.raises(ValueError, match="GPU only"):
            V.clip_frames({"image": c["imgs"], "image_raw": c["imgs_raw"], "image_depth": c["depth_imgs"]}, c, "concat_debug")
        with pytest.raises(ValueError, match="GPU only"):
            V.clip_frames({"image": c["imgs"]}, c, "final")
        for k in R.ORDER:
            with pytest.raises(TypeError, match="float32"):
                V.compose_debug_frames(*args(**{k: c[k].double()}))
            with pytest.raises(TypeError, match="a tensor is needed"):
                V.compose_debug_frames(*args(**{k: c[k].numpy()}))
            with pytest.raises(ValueError, match="not contiguous"):
                V.compose_debug_frames(*args(**{k: c[k].transpose(2, 3)}))
        with pytest.raises(TypeError, match="float32"):
            V.depth_range(c["depth_imgs"].half())
        with pytest.raises(ValueError, match="not contiguous"):
            V.depth_range(c["depth_imgs"][:, :, :, ::2])
        with pytest.raises(NotImplementedError):
            V.clip_frames({}, c, "debug")                                     # as the reference
        with pytest.raises(ValueError, match="out_mode"):
            V.clip_frames({}, c, "concat")
        with pytest.raises(NotImplementedError):
            V.secc2video_frames(None, {"drv_secc": c["drv_secc"]}, {"out_mode": "debug", "low_memory_usage": False})
        with pytest.raises(ValueError, match="chunk_frames"):
            V.secc2video_frames(None, {"drv_secc": c["drv_secc"]}, {"out_mode": "final", "low_memory_usage": False}, chunk_frames=0)
    assert calls == []


def test_patch_secc2video_keeps_the_original():
    from real3dportrait_amd import patch_secc2video
    infer = types.SimpleNamespace(forward_secc2video=lambda batch, inp=None: "reference")
    assert patch_secc2video(infer, writer=lambda frames, infer, inp: "written") is infer
    assert infer._r3d_reference_forward_secc2video(None) == "reference" and infer.forward_secc2video.__name__ == "forward_secc2video"
    assert patch_secc2video(infer)._r3d_reference_forward_secc2video(None) == "reference"          # patching twice keeps the first


def test_write_video_names_the_output_and_starts_ffmpeg_without_a_shell(tmp_path, monkeypatch):
    """write_video with a stand-in imageio and a recording runner: the frames reach the writer in order; the output's name; ffmpeg's
    argument lists (file names with blanks stay one argument each); what is deleted or moved afterwards."""
    import sys
    from real3dportrait_amd import video_frames as V
    monkeypatch.chdir(tmp_path)
    log = {"frames": [], "runs": []}

    class Writer:
        def __init__(self, name, **kw):
            log["writer"] = (name, kw)
            open(name, "wb").write(b"video")

        def append_data(self, frame):
            log["frames"].append(frame)

        def close(self):
            log["closed"] = True

    monkeypatch.setitem(sys.modules, "imageio", types.SimpleNamespace(get_writer=Writer))
    frames = np.arange(2 * 2 * 4 * 3, dtype=np.uint8).reshape(2, 2, 4, 3)
    infer = types.SimpleNamespace(wav16k_name="tmp 16k.wav")
    open(infer.wav16k_name, "wb").write(b"audio")

    def run(code):
        return lambda args: log["runs"].append(args) or code

    # a .wav: the resampled file is the audio; it and the silent video are deleted
    inp = {"out_name": "", "src_image_name": "data/my face.png", "drv_pose_name": "poses/nod.v2.npy", "drv_audio_name": "speech.wav"}
    name = V.write_video(frames, infer, inp, run=run(0))
    assert name == os.path.join("infer_out", "tmp", "my face_nod.v2.mp4") and os.path.isdir(os.path.join("infer_out", "tmp"))
    assert log["writer"] == ("demo.mp4", {"fps": 25, "format": "FFMPEG", "codec": "h264"}) and log["closed"]
    assert len(log["frames"]) == 2 and all(np.array_equal(a, b) for a, b in zip(log["frames"], frames))
    assert log["runs"] == [["ffmpeg", "-i", "demo.mp4", "-i", "tmp 16k.wav", "-y", "-v", "quiet", "-shortest", name]]
    assert not os.path.exists("demo.mp4") and not os.path.exists(infer.wav16k_name)
    # another container: its audio stream is mapped; ffmpeg succeeds, nothing is moved or deleted
    log["runs"].clear()
    inp = {"out_name": "out dir/clip.mp4", "src_image_name": "a.png", "drv_pose_name": "b.npy", "drv_audio_name": "talk; rm -rf x.mp4"}
    assert V.write_video(frames, infer, inp, run=run(0)) == "out dir/clip.mp4" and os.path.isdir("out dir")
    assert log["runs"] == [["ffmpeg", "-i", "demo.mp4", "-i", "talk; rm -rf x.mp4", "-map", "0:v", "-map", "1:a", "-y", "-v", "quiet", "-shortest",
                            "out dir/clip.mp4"]]
    assert os.path.exists("demo.mp4") and not os.path.exists("out dir/clip.mp4")
    # ... and fails: the silent video becomes the output
    assert V.write_video(frames, infer, dict(inp, out_name="plain.mp4"), run=run(1)) == "plain.mp4"
    assert open("plain.mp4", "rb").read() == b"video" and not os.path.exists("demo.mp4")
    assert V.write_video.__defaults__[0] is __import__("subprocess").call
