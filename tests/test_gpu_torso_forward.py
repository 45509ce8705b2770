"""GPU: the HIP torso forward (real3dportrait_amd/torso_forward.py): the channel-last entry points of the three modules
against their public forwards, bit for bit; patch_model(torso_forward=True) on the stand-in torso model and frame of
tests/test_gpu_torso_appearance.py against the fp64 chain that test builds, next to the parent path (the stand-in's torch glue over the
same three HIP modules); `ret`, the losses, the launch count, determinism across batch, repeats and streams, and that nothing is cached
from one call to the next."""
import collections

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import torso_appearance_ref64 as R64
import torso_motion_ref64 as M64
import torso_ref64 as G64
from test_gpu_torso_appearance import FEATS_SCALE, KP_INDEX, glue, stand_in_torso_model, synth_frame
from test_torso_appearance_host import hip_extractor, rel
from test_torso_generator_host import hip_generator, model_shell
from test_torso_motion_host import INPUT_ORDER, hip_estimator
from real3dportrait_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2e-4
LAUNCHES = 64          # library launches per forward at B = 1, rgb_alpha
SEEDS = (251, 252, 253, 254)
FRAME = 255
ALL = dict(torso_appearance=True, torso_motion=True, torso_generator=True)
_CACHE = {}


def to_cl(v):
    """r3d_torso_volume_to_cl of [N, C, D, H, W]."""
    from real3dportrait_amd import _lib
    N, C, D, H, W = v.shape
    out = torch.empty(N, D, H, W, C, device=v.device, dtype=torch.float32)
    _lib.check(_lib.load().r3d_torso_volume_to_cl(_lib.ptr(v), N, C, D, H, W, _lib.ptr(out), _lib.stream_ptr()), "torso_volume_to_cl")
    return out


def patched(torso_forward):
    """The stand-in torso model with the three HIP modules, with or without the HIP forward (built once each)."""
    from real3dportrait_amd import patch_model
    if torso_forward not in _CACHE:
        tm = stand_in_torso_model(*SEEDS).to(DEV)
        model = patch_model(model_shell(tm).to(DEV), torso_forward=torso_forward, **ALL)
        _CACHE[torso_forward] = model.superresolution.torso_model
    return _CACHE[torso_forward]


def fp64_chain(frame):
    """extractor -> glue -> estimator -> generator -> occlusion_2_predictor in fp64 on the device, as tests/test_gpu_torso_appearance.py
    builds it (computed once per frame seed and left unchanged)."""
    if ("ref", frame) not in _CACHE:
        se, sm, sg, sp = SEEDS
        img, seg, kp_s, kp_d, head, wts = synth_frame(frame)
        esd, msd = synth.synth_torso_appearance(se, 5), synth.synth_torso_motion(sm, 4)
        msd["compress.weight"] = msd["compress.weight"] * np.float32(FEATS_SCALE)
        gsd, psd = synth.synth_torso_generator(sg), synth.synth_torso_predictor(sp)
        with torch.no_grad():
            seg_in = F.interpolate(seg[:, [2, 4]].double(), size=(256, 256), mode="bilinear", align_corners=False, antialias=False)
            feats64 = R64.extractor(esd, torch.cat([img.double(), seg_in], dim=1))
            feats64, motion_in64 = glue(feats64, seg)
            eye = torch.eye(3, device=DEV)[None]
            d64, o64, o264 = M64.estimator(msd, motion_in64, kp_s[:, KP_INDEX], kp_d[:, KP_INDEX], eye, eye.clone(), head, wts)
            _, rgb64, hid64 = G64.generator(gsd, feats64, d64)
            occ64 = G64.occlusion_2(psd, hid64, o264)
        _CACHE[("ref", frame)] = {"rgb": rgb64.cpu().numpy(), "occlusion": o64.cpu().numpy(), "occlusion_2": occ64.cpu().numpy()}
    return _CACHE[("ref", frame)]


def errors(rgb, ret, ref):
    return {"rgb": rel(rgb.cpu().numpy(), ref["rgb"]), "occlusion": rel(ret["occlusion"].cpu().numpy(), ref["occlusion"]),
            "occlusion_2": rel(ret["occlusion_2"].cpu().numpy(), ref["occlusion_2"])}


# ---- the channel-last entry points ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2])
def test_extractor_forward_cl_is_the_transposed_forward(N):
    m = hip_extractor(synth.synth_torso_appearance(261, 5), 5).to(DEV)
    x = torch.from_numpy(synth.synth_torso_appearance_inputs(262, N, 5, 24, 40)["x"]).to(DEV)
    out = m(x)
    cl = m.forward_cl(x)
    assert cl.shape == (N, 16, 6, 10, 32) and cl.is_contiguous() and cl.dtype == torch.float32
    assert torch.equal(cl, to_cl(out))
    assert torch.equal(m(x), out)                                           # the public forward is what it was after a forward_cl


@pytest.mark.parametrize("N", [1, 2])
def test_estimator_forward_cl_is_the_forward_of_the_transposed_input(N):
    from real3dportrait_amd.torso_motion import jacobian
    m = hip_estimator(synth.synth_torso_motion(263, 4), 4).to(DEV)
    inp = synth.synth_torso_motion_inputs(264, N, 4, rotate=True)
    args = [torch.from_numpy(inp[k]).to(DEV) for k in INPUT_ORDER]
    want = m(*args)
    got = m.forward_cl(to_cl(args[0]), *args[1:])
    assert all(torch.equal(a, b) for a, b in zip(want, got))
    got = m.forward_cl(to_cl(args[0]), args[1], args[2], None, None, args[5], args[6], J=jacobian(args[3], args[4]))
    assert all(torch.equal(a, b) for a, b in zip(want, got))
    with pytest.raises(ValueError, match="expected fs"):
        m.forward_cl(*args)                                                 # the NCDHW volume is not channel-last


@pytest.mark.parametrize("N", [1, 2])
def test_generator_forward_cl_is_the_forward_of_the_transposed_input(N):
    from real3dportrait_amd import torso_generator
    m = hip_generator(synth.synth_torso_generator(265)).to(DEV)
    inp = synth.synth_torso_inputs(266, N, 24, 20)
    fs, grid = (torch.from_numpy(inp[k]).to(DEV) for k in ("torso_appearance_feats", "deformation"))
    rgb, hid = m(fs, grid, None, return_hid=True)
    cached = {k: v._srcs for k, v in torso_generator._VOLUME_CL._entries.items()}
    rgb_cl, hid_cl = m.forward_cl(to_cl(fs), grid, None, return_hid=True)
    assert torch.equal(rgb, rgb_cl) and torch.equal(hid, hid_cl)
    assert torch.equal(m.forward_cl(to_cl(fs), grid), rgb)
    assert {k: v._srcs for k, v in torso_generator._VOLUME_CL._entries.items()} == cached          # _VOLUME_CL is not touched
    with pytest.raises(ValueError, match="expected fs_cl"):
        m.forward_cl(fs, grid)


# ---- the whole forward -----------------------------------------------------------------------------------------------------------------
def test_forward_against_the_fp64_chain_next_to_the_parent_path():
    """rgb, occlusion and occlusion_2 within 2e-4 of max|ref| of the fp64 chain; the parent path (the stand-in's torch glue over the
    same HIP modules) on the same frame is printed next to it.  Measured on the MI355X: see DESIGN 4.13."""
    ref = fp64_chain(FRAME)
    frame = synth_frame(FRAME)
    rgb, ret = patched(True).forward(*frame)
    rgb_p, ret_p = patched(False).forward(*frame)
    new, parent = errors(rgb, ret, ref), errors(rgb_p, ret_p, ref)
    print("HIP forward:", new)
    print("parent path:", parent)
    print("HIP forward against the parent path:", {"rgb": rel(rgb.cpu().numpy(), rgb_p.cpu().numpy()),
                                                   "occlusion_2": rel(ret["occlusion_2"].cpu().numpy(), ret_p["occlusion_2"].cpu().numpy())})
    assert all(e <= TOL for e in new.values()), (new, parent)


def test_ret_has_the_reference_s_keys_shapes_and_losses():
    from real3dportrait_amd.torso_forward import losses
    tm = patched(True)
    frame = synth_frame(FRAME)
    rgb, ret = tm.forward(*frame, cal_loss=False, target_torso_mask=None)
    assert list(ret) == ["kp_src", "kp_drv", "occlusion", "occlusion_2", "deformed_torso_hid", "losses"]          # model2.py:258-267
    assert rgb.shape == (1, 3, 256, 256) and ret["kp_src"].shape == (1, 4, 3) and ret["kp_drv"].shape == (1, 4, 3)
    assert ret["occlusion"].shape == (1, 1, 64, 64) and ret["occlusion_2"].shape == (1, 1, 256, 256)
    assert ret["deformed_torso_hid"].shape == (1, 64, 256, 256)
    assert torch.equal(ret["kp_src"], frame[2][:, KP_INDEX]) and torch.equal(ret["kp_drv"], frame[3][:, KP_INDEX])
    occ, occ2 = ret["occlusion"], ret["occlusion_2"]
    alphas = occ2.clamp(1e-5, 1 - 1e-5)
    want = {"facev2v/occlusion_reg_l1": occ.mean(), "facev2v/occlusion_2_reg_l1": occ2.mean(),
            "facev2v/occlusion_2_weights_entropy": torch.mean(- alphas * torch.log2(alphas) - (1 - alphas) * torch.log2(1 - alphas))}
    assert list(ret["losses"]) == list(want)
    for k, v in want.items():
        assert torch.equal(ret["losses"][k], v) and bool(torch.isfinite(v)), k
    # the other branch (model2.py:272-279)
    target = torch.from_numpy(synth.hash_uniform(7, 512 * 512).reshape(1, 512, 512) > 0.6).to(DEV)
    tm.hparams = {"torso_kp_num": 4, "torso_occlusion_reg_unmask_factor": 0.3}
    try:
        rgb2, ret2 = tm.forward(*frame, target_torso_mask=target)
    finally:
        del tm.hparams
    assert torch.equal(rgb2, rgb) and torch.equal(ret2["occlusion_2"], occ2)
    want2 = losses(occ, occ2, target, 0.3)
    for k in want:
        assert torch.equal(ret2["losses"][k], want2[k]), k
    assert not torch.equal(ret2["losses"]["facev2v/occlusion_reg_l1"], want["facev2v/occlusion_reg_l1"])
    assert torch.equal(ret2["losses"]["facev2v/occlusion_2_weights_entropy"], want["facev2v/occlusion_2_weights_entropy"])


def test_hparams_steer_the_glue():
    """torso_mask_dilate_ksize and mul_torso_mask are read from the torso model's hparams at call time (model2.py:233-234)."""
    tm = patched(True)
    frame = synth_frame(FRAME)
    rgb, _ = tm.forward(*frame)
    tm.hparams = {"torso_kp_num": 4, "torso_mask_dilate_ksize": 7, "mul_torso_mask": True}
    try:
        assert torch.equal(tm.forward(*frame)[0], rgb)                     # the defaults
        tm.hparams["torso_mask_dilate_ksize"] = 1
        k1 = tm.forward(*frame)[0]
        tm.hparams["torso_mask_dilate_ksize"], tm.hparams["mul_torso_mask"] = 7, False
        nomul = tm.forward(*frame)[0]
    finally:
        del tm.hparams
    assert not torch.equal(k1, rgb) and not torch.equal(nomul, rgb) and not torch.equal(nomul, k1)


def test_launches_per_forward():
    """r3d_torso_volume_to_cl is never called, the two glue kernels once each, and the total is the number DESIGN 4.13 states."""
    from real3dportrait_amd import _lib, torso_forward
    assert torso_forward.LAUNCHES == LAUNCHES
    tm = patched(True)
    frame = synth_frame(FRAME)
    rgb, _ = tm.forward(*frame)                                             # the folds and the buffers
    with _lib.counting() as calls:
        again, _ = tm.forward(*frame)
    counts = dict(collections.Counter(name for name, _ in calls))
    torch.cuda.synchronize()
    print("launches:", counts)
    assert "r3d_torso_volume_to_cl" not in counts
    assert counts["r3d_torso_seg_input"] == 1 and counts["r3d_torso_mask_volume"] == 1
    assert sum(counts.values()) == LAUNCHES, counts
    assert torch.equal(rgb, again)
    # the parent path on the same frame, for comparison: two transposes and no glue kernel
    with _lib.counting() as calls:
        patched(False).forward(*frame)
    counts = dict(collections.Counter(name for name, _ in calls))
    torch.cuda.synchronize()
    print("parent path launches:", counts)
    assert counts["r3d_torso_volume_to_cl"] == 2 and "r3d_torso_mask_volume" not in counts and sum(counts.values()) == LAUNCHES


def test_batch_repeat_and_side_stream_are_bit_identical_and_nothing_is_cached():
    tm = patched(True)
    a, b = synth_frame(FRAME), synth_frame(FRAME + 10)
    b = (b[0], torch.flip(b[1], dims=[3]).contiguous()) + b[2:]               # another segmap too
    both = tuple(torch.cat([x, y], dim=0) for x, y in zip(a, b))
    keys = ("occlusion", "occlusion_2", "deformed_torso_hid")
    rgb2, ret2 = tm.forward(*both)
    outs = []
    for n, frame in enumerate((a, b)):                                      # two consecutive calls with different segmaps
        rgb1, ret1 = tm.forward(*frame)
        outs.append(rgb1)
        assert torch.equal(rgb2[n:n + 1], rgb1), n
        for k in keys:
            assert torch.equal(ret2[k][n:n + 1], ret1[k]), (n, k)
    assert not torch.equal(outs[0], outs[1])
    # only the segmap differs: the result must follow it
    rgb_seg, _ = tm.forward(a[0], b[1], *a[2:])
    assert not torch.equal(rgb_seg, outs[0])
    assert torch.equal(tm.forward(*a)[0], outs[0])                          # and a repeated call is the first one
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s_rgb, s_ret = tm.forward(*both)
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(s_rgb, rgb2) and all(torch.equal(s_ret[k], ret2[k]) for k in keys)
    assert len(tm._r3d_torso_forward.work) == 3                             # (main, N 2), (main, N 1), (side, N 2)
    assert sorted(n for _, n in tm._r3d_torso_forward.identity_j) == [1, 2]


def test_forward_is_untouched_without_the_switch():
    from real3dportrait_amd import patch_model
    tm = patched(False)
    assert tm.forward.__name__ == "forward" and tm.forward.__module__ == "test_gpu_torso_appearance"      # the stand-in's own closure
    assert not hasattr(tm, "_r3d_torso_forward") and not hasattr(tm, "_r3d_reference_forward")
    fwd = tm.forward
    patch_model(model_shell(tm).to(DEV), torso_forward=False)
    assert tm.forward is fwd


def test_a_segmap_that_is_not_fp32_gets_the_reference_s_float():
    tm = patched(True)
    frame = synth_frame(FRAME)
    hard = (frame[1] > 0.5)
    assert torch.equal(tm.forward(frame[0], hard, *frame[2:])[0], tm.forward(frame[0], hard.float(), *frame[2:])[0])
    assert torch.equal(tm.forward(frame[0], hard.half(), *frame[2:])[0], tm.forward(frame[0], hard.float(), *frame[2:])[0])
