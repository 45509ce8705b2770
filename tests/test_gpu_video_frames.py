"""GPU: the HIP output video frames (real3dportrait_amd/video_frames.py, r3d_video_depth_range / r3d_video_compose_debug)
against the oracle tests/video_frames_ref.py, the reference's operator sequence of inference/real3d_infer.py:495-521 on torch-CPU and
NumPy.  Every comparison is byte for byte; there is no tolerance anywhere in this file.

Shapes: the two kernels' paths are the 16-pixel lane (W % 16 == 0, 16-byte aligned pointers) with its three gathers (a source as wide
as the frame, a quarter as wide, anything else) and the 4-pixel lane (W % 4 == 0, or a pointer that is only 4-byte aligned); each is
reached at the smallest clip that has more than one lane group per row, more than one block, and the nearest ratios the issue names."""
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden
import video_frames_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# name -> the arguments of R.clip: (seed, T, H, W, secc (h, w), raw (h, w), depth (h, w), depth kind)
CLIPS = {
    "w16_one_group": (41, 2, 8, 16, (8, 16), (2, 4), (5, 9), "spread"),              # one 16-pixel group per panel row; depth by the general gather
    "w48_three_groups": (42, 2, 10, 48, (20, 31), (13, 48), (7, 12), "spread"),      # SECC general, raw as wide as the frame, depth a quarter
    "t1": (43, 1, 32, 32, (32, 32), (8, 8), (8, 8), "spread"),
    "product_512": (44, 2, 512, 512, (512, 512), (128, 128), (128, 128), "spread"),
}
GOLDEN = ("a_t3_32", "b_t2_12x20", "c_constant_depth", "d_nan_depth")


@functools.lru_cache(maxsize=None)
def case(name):
    """(the clip's sources as NumPy arrays, the oracle's bytes), computed once and never written."""
    if name in GOLDEN:
        g = load_golden("video_frames_" + name)
        c, want = {k: g[k] for k in R.ORDER}, g["concat_debug"]
    else:
        c = R.clip(*CLIPS[name])
        want = R.oracle_of(c)
    for a in list(c.values()) + [want]:
        a.setflags(write=False)
    return c, want


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)          # (a copy: the cached arrays are read-only)


def on_device(c):
    return [dev(c[k]) for k in R.ORDER]


def panels(out, W):
    return [out[:, :, p * W:(p + 1) * W] for p in range(5)]


def check(got, want, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert got.dtype == np.uint8 and got.shape == want.shape, (what, got.shape, want.shape)
    W = want.shape[2] // 5
    bad = [int((g != w).sum()) for g, w in zip(panels(got, W), panels(want, W))]
    print("%s: mismatching bytes per panel (ref, secc, raw, depth, image): %s of %d" % (what, bad, want[:, :, :W].size))
    assert bad == [0, 0, 0, 0, 0], what


@pytest.mark.parametrize("name", GOLDEN[:2] + ("w16_one_group", "w48_three_groups", "t1", "product_512"))
def test_strips_equal_the_oracle(name):
    """The issue's shapes: T = 3 at 32 x 32 with integer ratios (16-pixel lanes), T = 2 at 12 x 20 with raw 5 x 7, depth 7 x 5, SECC 9 x 24
    (4-pixel lanes, a different non-integer ratio per source), W = 16 and W = 48, T = 1, and one frame pair at the product's size.  The SECC
    maps hold every exact code, uniform values, +-1 and values a few ulps and 0.25 outside [-1, 1] at panel and row ends; the depth's
    minimum lies in the first frame and its maximum in the last."""
    from real3dportrait_amd import video_frames as V
    c, want = case(name)
    check(V.compose_debug_frames(*on_device(c)), want, name)


def test_the_synthetic_clips_hold_what_the_issue_asks():
    c, want = case("a_t3_32")
    s, d = c["drv_secc"], c["depth_imgs"]
    for t in range(3):
        assert set(R.secc_edge_values().tolist()) <= set(s[t].reshape(-1).tolist())
    assert s[0, 0, 0, 0] == R.secc_edge_values()[0] and s[0, 0, -1, -1] == R.secc_edge_values()[-1]          # a panel's first and last pixel
    assert d.min() == d[0].min() < d[1:].min() and d.max() == d[-1].max() > d[:-1].max()
    W = 32
    per_frame = np.concatenate([R.oracle_of({k: (v if k == "ref_gt_img" else v[t:t + 1]) for k, v in c.items()})[:, :, 3 * W:4 * W] for t in range(3)])
    assert not np.array_equal(per_frame, want[:, :, 3 * W:4 * W])


@pytest.mark.parametrize("name", ("c_constant_depth", "d_nan_depth"))
def test_constant_and_nan_depth_give_a_zero_panel_and_leave_the_rest(name):
    from real3dportrait_amd import video_frames as V
    c, want = case(name)
    got = V.compose_debug_frames(*on_device(c)).cpu().numpy()
    check(got, want, name)
    assert not got[:, :, 48:64].any() and got[:, :, :48].any() and got[:, :, 64:].any()
    state = V.depth_range(dev(c["depth_imgs"])).cpu().numpy()
    if name == "d_nan_depth":
        assert state[2] == 1 and np.isnan(state[:2].view(np.float32)).all() and np.isnan(c["depth_imgs"][-1]).sum() == 1
    else:
        assert state[2] == 0 and state[:2].view(np.float32).tolist() == [2.5, 2.5]
    assert state[3] == 1 and not state[4:].any()


def test_chunks_with_an_accumulated_state_equal_the_single_call():
    """[0:1] then [1:3]: the state after the two reductions equals the state after one, bitwise, and the chunks composed with it equal
    the clip composed at once.  reset discards what a state holds inside the launch; the clip's extremes are the oracle's."""
    from real3dportrait_amd import video_frames as V
    c, want = case("a_t3_32")
    ref, secc, raw, depth, img = on_device(c)
    whole = V.depth_range(depth)
    parts = V.depth_range(depth[0:1])
    first = parts.clone()
    assert V.depth_range(depth[1:3], parts) is parts
    assert torch.equal(whole, parts) and not torch.equal(first, parts)
    mn, mx, nan = R.depth_min_max(torch.from_numpy(c["depth_imgs"]))
    assert whole.cpu().numpy()[:2].view(np.float32).tolist() == [mn, mx] and whole.cpu().tolist()[2:] == [0, 1, 0, 0, 0, 0] and not nan
    out = torch.empty(3, 32, 160, 3, dtype=torch.uint8, device=DEV)
    V.compose_debug_frames(ref, secc[0:1], raw[0:1], depth[0:1], img[0:1], depth_range=parts, out=out[0:1])
    V.compose_debug_frames(ref, secc[1:3], raw[1:3], depth[1:3], img[1:3], depth_range=parts, out=out[1:3])
    check(out, want, "chunks [0:1], [1:3]")
    # the other order of chunks, and many small ones: min and max do not depend on the order
    other = V.depth_range(depth[0:1], V.depth_range(depth[1:3]))
    rows = V.new_depth_state(DEV)
    for t in range(3):
        for y in range(8):
            V.depth_range(depth[t, 0, y], rows)
    assert torch.equal(other, whole) and torch.equal(rows, whole)
    # reset: the state of the last frame alone, whatever it held
    assert torch.equal(V.depth_range(depth[2:3], parts, reset=True), V.depth_range(depth[2:3])) and not torch.equal(parts, whole)
    # a NaN is sticky across chunks and gone after a reset
    nan_state = V.depth_range(dev(np.array([1.0, np.nan, 3.0], np.float32)))
    V.depth_range(depth, nan_state)
    assert nan_state.cpu().tolist()[2] == 1 and np.isnan(nan_state.cpu().numpy()[:2].view(np.float32)).all()
    assert torch.equal(V.depth_range(depth, nan_state, reset=True), whole)


def test_depth_range_of_many_blocks_and_ragged_counts():
    """More than one block (the ticket's last arriver folds the result), counts that are no multiple of 4, a pointer that is only 4-byte
    aligned (the scalar loop), negative values and signed zeros."""
    from real3dportrait_amd import video_frames as V
    rng = np.random.default_rng(7)
    x = rng.normal(0, 3, 300001).astype(np.float32)
    x[123457], x[7] = -0.0, 0.0
    d = dev(x)
    for lo, hi in ((0, 300001), (1, 300000), (3, 4098), (0, 1), (2, 5), (0, 262144)):
        st = V.depth_range(d[lo:hi]).cpu().numpy()
        assert st[:2].view(np.float32).tolist() == [x[lo:hi].min(), x[lo:hi].max()] and st[2:].tolist() == [0, 1, 0, 0, 0, 0], (lo, hi)
    z = V.depth_range(dev(np.array([0.0, -0.0, 0.0], np.float32))).cpu().numpy()
    assert z[:2].tolist() == [np.float32(-0.0).view(np.int32), 0]                   # -0.0 below +0.0, whatever the order


def test_depth_range_beyond_the_grids_cap():
    """depth_range_kernel's grid grows with the count, a block per 4096 floats, up to a cap of 1024 blocks (a 257-frame clip of 128 x 128
    depth images is past it).  Below the cap a lane takes 4 grid-stride steps of a float4, or 16 of a float in the scalar loop, and every
    other test stays there; past it the grid no longer grows and a lane takes more steps than the 16 floats a block is sized for.  With
    1024 x 4096 + 3 x 4096 + 5 floats only such further steps reach the maximum, in the first block's worth past the cap, and the
    minimum, in the last five elements (the last whole float4 and the ragged tail).  Once 16-byte aligned, once from a view one float
    in (the scalar loop), once with a NaN past the cap: min, max and the NaN word as NumPy's, the partial words and the ticket zero
    afterwards."""
    from real3dportrait_amd import video_frames as V
    cap = 1024 * 4096
    count = cap + 3 * 4096 + 5
    x = np.random.default_rng(11).normal(0, 3, count).astype(np.float32)
    x[count - 3], x[cap + 1000] = -100.0, 100.0
    assert x.argmin() == count - 3 >= count - 5 and cap <= x.argmax() < cap + 4096
    aligned = dev(x)
    buf = torch.empty(count + 1, dtype=torch.float32, device=DEV)
    shifted = buf[1:]
    shifted.copy_(aligned)
    assert aligned.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4
    for what, d in (("16-byte aligned", aligned), ("one float in", shifted)):
        st = V.depth_range(d).cpu().numpy()
        print("depth range of %d floats, %s: min %r max %r, state words 2.. %s" % (count, what, *st[:2].view(np.float32).tolist(), st[2:].tolist()))
        assert st[:2].view(np.float32).tolist() == [x.min(), x.max()] == [-100.0, 100.0] and st[2:].tolist() == [0, 1, 0, 0, 0, 0], what
    x[4200000] = np.nan
    assert np.isnan(x.min()) and np.isnan(x.max())
    for what, d in (("16-byte aligned", dev(x)), ("one float in", shifted)):
        if d is shifted:
            shifted[4200000] = float("nan")
        st = V.depth_range(d).cpu().numpy()
        print("depth range with a NaN at 4 200 000, %s: words %s" % (what, [hex(w) for w in st.view(np.uint32).tolist()]))
        assert np.isnan(st[:2].view(np.float32)).all() and st[2:].tolist() == [1, 1, 0, 0, 0, 0], what


def test_another_stream_two_runs_inputs_and_guard_bytes():
    """A run on a non-default stream; two runs bit-identical; the inputs are unchanged afterwards; 64 guard bytes in front of and behind
    `out` are untouched -- and again with `out` only 4-byte aligned, which takes the 4-pixel lanes at a W the 16-pixel lanes would take."""
    from real3dportrait_amd import video_frames as V
    c, want = case("a_t3_32")
    src = on_device(c)
    keep = [t.clone() for t in src]
    n = want.size
    first = V.compose_debug_frames(*src)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    for guard in (64, 4):
        buf = torch.full((n + 2 * guard,), 0xAB, dtype=torch.uint8, device=DEV)
        out = buf[guard:guard + n].view(want.shape)
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            assert V.compose_debug_frames(*src, out=out) is out
        torch.cuda.current_stream().wait_stream(stream)
        assert torch.equal(out, first)
        assert (buf[:guard] == 0xAB).all() and (buf[guard + n:] == 0xAB).all()
    check(first, want, "first run")
    for a, b in zip(src, keep):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_unaligned_sources_take_the_dword_lanes_to_the_same_bytes():
    from real3dportrait_amd import video_frames as V
    c, want = case("w48_three_groups")
    shifted = []
    for k in R.ORDER:
        flat = torch.empty(c[k].size + 1, dtype=torch.float32, device=DEV)
        flat[1:] = dev(c[k]).reshape(-1)
        shifted.append(flat[1:].view(c[k].shape))
        assert shifted[-1].data_ptr() % 16 == 4
    check(V.compose_debug_frames(*shifted), want, "sources 4 bytes past a 16-byte boundary")


def test_selected_panels_leave_the_others():
    """panels 31 - 8 per chunk and the depth panels at the end -- what secc2video_frames does with chunk_frames -- give the clip's bytes."""
    from real3dportrait_amd import _lib, video_frames as V
    c, want = case("a_t3_32")
    ref, secc, raw, depth, img = on_device(c)
    out = torch.full(want.shape, 0x5A, dtype=torch.uint8, device=DEV)
    V._compose(ref, secc, raw, None, img, 3, 32, 32, _lib.VIDEO_PANELS_ALL - _lib.VIDEO_PANEL_DEPTH, None, out)
    assert (out[:, :, 96:128] == 0x5A).all()
    V._compose(None, None, None, depth, None, 3, 32, 32, _lib.VIDEO_PANEL_DEPTH, V.depth_range(depth), out)
    check(out, want, "four panels, then the depth panel")


def test_long_clips_are_cut_below_the_entry_points_limit_per_call(monkeypatch):
    """The entry points take less than 2^31 bytes per call (546 frames of 512 x 512 strips); the Python layer cuts longer clips.  With
    the module's bound lowered to two frames' worth of strip, T = 5 goes out as runs of 2, 2 and 1 frames in every pass -- the single
    call, the four colour panels of a chunk and the closing depth pass of secc2video_frames -- and a depth reduction above the bound as
    several accumulating launches, to the same bytes and the same state."""
    import types
    from real3dportrait_amd import _lib, video_frames as V
    c = R.clip(51, 5, 8, 16, (8, 16), (2, 4), (4, 8), "spread")
    want = R.oracle_of(c)
    src = on_device(c)
    whole_state = V.depth_range(src[3])
    monkeypatch.setattr(V, "MAX_CALL_BYTES", 4 * 120 + 3)                    # the depth's 160 floats: launches of 120 and 40
    with _lib.counting() as calls:
        assert torch.equal(V.depth_range(src[3]), whole_state)
        assert torch.equal(V.depth_range(src[3], V.depth_range(src[0]), reset=True), whole_state)      # reset applies to the first launch only
    assert [(name, a[1], a[2]) for name, a in calls] == [("r3d_video_depth_range", n, r) for n, r in
                                                         ((120, 0), (40, 0), (120, 0), (120, 0), (120, 0), (24, 0), (120, 1), (40, 0))]
    monkeypatch.setattr(V, "MAX_CALL_BYTES", 2 * 15 * 8 * 16 + 7)
    with _lib.counting() as calls:
        got = V.compose_debug_frames(*src)
    check(got, want, "T = 5 in runs of two frames")
    assert [(name, a[1] if name == "r3d_video_depth_range" else a[11]) for name, a in calls] == \
        [("r3d_video_depth_range", 160)] + [("r3d_video_compose_debug", n) for n in (2, 2, 1)]
    # a source that is larger than the strip sets the run: SECC maps of 32 x 32 are 12 288 bytes a frame, one frame per call
    big = R.clip(52, 3, 8, 16, (32, 32), (2, 4), (4, 8), "spread")
    with _lib.counting() as calls:
        check(V.compose_debug_frames(*on_device(big)), R.oracle_of(big), "one frame per call")
    assert [a[11] for name, a in calls if name == "r3d_video_compose_debug"] == [1, 1, 1]
    # secc2video_frames: chunks of 3 and 2 frames, each colour pass and the depth pass cut again
    model = StandInModel(8, 16, 4, 8)
    g = torch.Generator().manual_seed(10)
    r = lambda *s: (torch.rand(*s, generator=g) * 2 - 1).to(DEV)
    batch = {"camera": r(5, 25), "src_kp": r(1, 68, 2), "drv_kp": r(5, 68, 2), "cano_secc": r(1, 3, 8, 16), "src_secc": r(1, 3, 8, 16),
             "drv_secc": r(5, 3, 8, 16), "ref_gt_img": r(1, 3, 8, 16), "ref_head_img": r(1, 3, 8, 16), "ref_torso_img": r(1, 3, 8, 16),
             "bg_img": r(1, 3, 8, 16), "segmap": r(1, 6, 8, 16)}
    with _lib.counting() as calls:
        frames = V.secc2video_frames(types.SimpleNamespace(secc2video_model=model), batch, {"out_mode": "concat_debug", "low_memory_usage": False}, 3)
    composed = [(a[14], a[11]) for name, a in calls if name == "r3d_video_compose_debug"]
    assert composed == [(23, 2), (23, 1), (23, 2), (8, 2), (8, 2), (8, 1)]                        # (panels, frames) per launch
    cat = lambda k: torch.cat([call["out"][k] for call in model.calls]).cpu()
    check(frames, R.concat_debug(batch["ref_gt_img"].cpu(), batch["drv_secc"].cpu(), cat("image_raw"), cat("image_depth"), cat("image")),
          "secc2video_frames in cut passes")


def test_a_state_on_another_device_is_refused():
    from real3dportrait_amd import video_frames as V
    if torch.cuda.device_count() < 2:
        return                                    # one GPU: there is no other device to put a state on
    c, _ = case("w16_one_group")
    with pytest.raises(ValueError, match="is on"):
        V.compose_debug_frames(*on_device(c), depth_range=V.new_depth_state("cuda:1"))


def test_clip_frames_dispatches_both_modes():
    from real3dportrait_amd import video_frames as V
    g = load_golden("video_frames_b_t2_12x20")
    ref, secc, raw, depth, img = (dev(g[k]) for k in R.ORDER)
    outputs, batch = {"image": img, "image_raw": raw, "image_depth": depth}, {"ref_gt_img": ref, "drv_secc": secc}
    fin = V.clip_frames(outputs, batch, "final")
    assert np.array_equal(fin.cpu().numpy(), g["final"]) and np.array_equal(g["final"], R.final(torch.from_numpy(g["imgs"])))
    check(V.clip_frames(outputs, batch, "concat_debug"), g["concat_debug"], "clip_frames concat_debug")
    with pytest.raises(NotImplementedError):
        V.clip_frames(outputs, batch, "debug")


class StandInModel:
    """In the place of infer.secc2video_model: forward returns images that are a deterministic function of `camera` and cond['kp_d'],
    computed on the device without a synchronisation, and keeps every call's arguments and outputs."""

    def __init__(self, H, W, h, w):
        g = torch.Generator().manual_seed(5)
        r = lambda *s: (torch.rand(*s, generator=g) * 2.2 - 1.1).to(DEV)
        self.base = {"image": r(1, 3, H, W), "image_raw": r(1, 3, h, w), "image_depth": r(1, 1, h, w)}
        self.calls = []

    def forward(self, img, camera, cond, ret, cache_backbone, use_cached_backbone):
        a, b = torch.tanh(camera.sum() * 0.05), cond["kp_d"].mean() * 3
        out = {"image": self.base["image"] * a + b, "image_raw": self.base["image_raw"] * (a * 0.9) - b,
               "image_depth": self.base["image_depth"] * 0.5 + 2.5 + camera[0, 3] + b}
        self.calls.append(dict(img=img, camera=camera, cond=cond, ret=ret, flags=(cache_backbone, use_cached_backbone), out=out))
        return dict(out, extra="ignored")


@pytest.mark.parametrize("mode, chunk", (("concat_debug", None), ("concat_debug", 2), ("final", 2), ("low_memory", None)))
def test_secc2video_frames_with_a_stand_in_model(mode, chunk):
    """T = 5: the arguments and flags of every forward call are the reference loop's (:481-489), the frames are the oracle's for the
    stand-in's outputs, and nothing between the first and the last launch waits for the device (sync debug mode 'error')."""
    import types
    from real3dportrait_amd import clip_keypoints, video_frames as V
    T, H, W, h, w = 5, 16, 32, 4, 8
    g = torch.Generator().manual_seed(9)
    r = lambda *s: (torch.rand(*s, generator=g) * 2 - 1).to(DEV)
    batch = {"camera": r(T, 25), "src_kp": r(1, 68, 2), "drv_kp": r(T, 68, 2), "cano_secc": r(1, 3, H, W), "src_secc": r(1, 3, H, W),
             "drv_secc": r(T, 3, H, W), "ref_gt_img": r(1, 3, H, W), "ref_head_img": r(1, 3, H, W), "ref_torso_img": r(1, 3, H, W),
             "bg_img": r(1, 3, H, W), "segmap": r(1, 6, H, W)}
    inp = {"out_mode": "concat_debug" if mode == "low_memory" else mode, "low_memory_usage": mode == "low_memory"}
    model = StandInModel(H, W, h, w)
    infer = types.SimpleNamespace(secc2video_model=model)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        frames = V.secc2video_frames(infer, batch, inp, chunk_frames=chunk)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    kp_s, kp_d = clip_keypoints(batch["src_kp"], batch["drv_kp"], 7)
    assert len(model.calls) == T
    for i, call in enumerate(model.calls):
        assert call["flags"] == ((True, False) if i == 0 else (False, True)) and call["ret"] == {} and call["img"] is batch["ref_head_img"]
        assert call["camera"].shape == (1, 25) and call["camera"].data_ptr() == batch["camera"][i:i + 1].data_ptr()
        cond = call["cond"]
        assert set(cond) == {"cond_cano", "cond_src", "cond_tgt", "ref_torso_img", "bg_img", "segmap", "kp_s", "kp_d"}
        assert cond["cond_cano"] is batch["cano_secc"] and cond["cond_src"] is batch["src_secc"] and cond["segmap"] is batch["segmap"]
        assert cond["ref_torso_img"] is batch["ref_torso_img"] and cond["bg_img"] is batch["bg_img"]
        assert cond["cond_tgt"].data_ptr() == batch["drv_secc"][i:i + 1].data_ptr() and cond["cond_tgt"].shape == (1, 3, H, W)
        assert cond["kp_s"].shape == cond["kp_d"].shape == (1, 68, 3)
        assert torch.equal(cond["kp_d"], kp_d[i:i + 1]) and torch.equal(cond["kp_s"], kp_s[i:i + 1]) and not cond["kp_d"][..., 2].any()
    cat = lambda k: torch.cat([call["out"][k] for call in model.calls]).cpu()
    if mode == "concat_debug":
        want = R.concat_debug(batch["ref_gt_img"].cpu(), batch["drv_secc"].cpu(), cat("image_raw"), cat("image_depth"), cat("image"))
        check(frames, want, "secc2video_frames %s chunk %s" % (mode, chunk))
    else:
        assert np.array_equal(frames.cpu().numpy(), R.final(cat("image")))
    # the bound method hands the host copy to the writer
    got = {}
    V.patch_secc2video(infer, writer=lambda fr, inf, p: got.update(frames=fr, infer=inf, inp=p) or "name", chunk_frames=chunk)
    assert infer.forward_secc2video(batch, inp) == "name" and got["infer"] is infer and got["inp"] is inp
    assert isinstance(got["frames"], np.ndarray) and np.array_equal(got["frames"], frames.cpu().numpy())
