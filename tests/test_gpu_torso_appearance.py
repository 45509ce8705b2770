"""GPU: the HIP appearance feature extractor (real3dportrait_amd/torso_appearance.py) against the reference's goldens and,
on fresh inputs, the fp64 restatement (tests/torso_appearance_ref64.py); determinism across batch, repeats and streams; the bf16x3 tier;
the number of kernel launches per forward; the patch_model swap of all three torso modules on a stand-in torso model whose forward
restates the reference's (facev2v_warp/model2.py:226-263)."""
import collections

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import torso_appearance_ref64 as R64
import torso_motion_ref64 as M64
import torso_ref64 as G64
from test_torso_appearance_host import GOLDENS, golden_case, hip_extractor, reference_like_extractor, rel, subsample
from real3dportrait_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2e-4
LAUNCHES = 16          # library launches per forward at B = 1


def fresh(seed_p, seed_x, N, in_dim, H, W, precision="f32"):
    sd = synth.synth_torso_appearance(seed_p, in_dim)
    x = torch.from_numpy(synth.synth_torso_appearance_inputs(seed_x, N, in_dim, H, W)["x"]).to(DEV)
    return sd, hip_extractor(sd, in_dim, precision).to(DEV), x


def against_fp64(what, m, sd, x):
    out = m(x)
    with torch.no_grad():
        ref = R64.extractor(sd, x)                                     # fp64 on the device
    N, _, H, W = x.shape
    assert out.shape == (N, 32, 16, H // 4, W // 4) and out.is_contiguous() and out.dtype == torch.float32
    e = rel(out.cpu().numpy(), ref.cpu().numpy())
    print("%s: %.2e" % (what, e))
    assert e <= TOL, (what, e)
    return out


@pytest.mark.parametrize("name", GOLDENS)
def test_goldens(name):
    g, sd, x = golden_case(name)
    m = hip_extractor(sd, x.shape[1]).to(DEV)
    out = m(torch.from_numpy(x).to(DEV))
    assert out.shape == (x.shape[0], 32, 16, x.shape[2] // 4, x.shape[3] // 4) and out.is_contiguous()
    e = rel(subsample(g, out).cpu().numpy(), g["out"])
    print(name, e)
    assert e <= TOL, e


def test_fresh_inputs_against_fp64():
    sd, m, x = fresh(211, 213, 2, 5, 64, 96)
    against_fp64("N2 in_dim5 64x96", m, sd, x)


def test_smallest_input():
    sd, m, x = fresh(214, 215, 1, 3, 8, 4)
    out = against_fp64("8x4", m, sd, x)
    assert out.shape == (1, 32, 16, 2, 1)


def test_product_shape():
    sd, m, x = fresh(216, 217, 1, 5, 256, 256)
    against_fp64("product 256x256", m, sd, x)


def test_batch_repeat_and_side_stream_are_bit_identical():
    sd, m, x = fresh(221, 223, 2, 5, 24, 40)
    both = m(x)
    assert not torch.equal(both[0], both[1])
    for n in range(2):
        assert torch.equal(both[n:n + 1], m(x[n:n + 1].contiguous())), n
    assert torch.equal(both, m(x))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s_out = m(x)
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(both, s_out)
    assert len(m._work) == 3                                            # (main, N 2), (main, N 1), (side, N 2): per (device, stream, N, H, W)


def test_bf16x3_tier_meets_the_tolerance_and_is_really_taken():
    sd, m, x = fresh(231, 233, 2, 5, 64, 96)
    exact = against_fp64("f32 tier", m, sd, x)
    m3 = hip_extractor(sd, 5, "bf16x3").to(DEV)
    split = against_fp64("bf16x3 tier", m3, sd, x)
    assert not torch.equal(exact, split)
    assert torch.equal(split, m3(x))


def test_launches_per_forward():
    """Every r3d_* call of the module is one kernel launch; one forward at B = 1 makes the number DESIGN 4.12 states."""
    from real3dportrait_amd import _lib, torso_appearance
    assert torso_appearance.LAUNCHES == LAUNCHES
    for precision, first in (("f32", "r3d_torso_conv"), ("bf16x3", "r3d_torso_conv_prec")):
        sd, m, x = fresh(241, 243, 1, 5, 32, 32, precision)
        out = m(x)                                                      # the fold and the buffers
        with _lib.counting() as calls:
            again = m(x)
        counts = dict(collections.Counter(name for name, _ in calls))
        torch.cuda.synchronize()
        print("launches:", counts)
        assert sum(counts.values()) == LAUNCHES, counts
        assert counts == {first: 1, "r3d_torso_conv_pool": 2, "r3d_torso_conv_split": 1, "r3d_torso_conv3d_res": 12}
        assert torch.equal(out, again)


# ---- the whole torso model ---------------------------------------------------------------------------------------------------------------
KP_INDEX = [0, 8, 16, 27]                                               # torso_kp_num 4 (model2.py:238-240)
FEATS_SCALE = 1.0 / 8.0     # the stand-in estimator's compress reads features of rms ~ 8 here, not the unit variance its gains were chosen for


def dilate(bin_img, ksize=7):
    """utils/commons/image_utils.py:10-15."""
    pad = (ksize - 1) // 2
    return F.max_pool2d(F.pad(bin_img, pad=[pad, pad, pad, pad], mode="reflect"), kernel_size=ksize, stride=1, padding=0)


def glue(feats, segmap):
    """model2.py:231-236 on the extractor's output: (torso_appearance_feats, motion_inp_appearance_feats)."""
    torso_segmap = F.interpolate(segmap[:, [2, 4]].to(feats.dtype), size=(64, 64), mode="bilinear", align_corners=False, antialias=False)
    torso_mask = dilate(torso_segmap.sum(dim=1).unsqueeze(1), ksize=7)
    feats = feats * torso_mask.unsqueeze(1)
    return feats, torch.cat([feats, torso_segmap.unsqueeze(2).repeat([1, 1, feats.shape[2], 1, 1])], dim=1)


def stand_in_torso_model(se, sm, sg, sp):
    """The stand-in torso model of the generator's and the estimator's tests with an appearance extractor, and WarpBasedTorsoModelMediaPipe's
    forward with torso_inp_mode rgb_alpha restated in plain torch (model2.py:226-263 without the gradient scaling, which is the identity
    in value, and the losses)."""
    from test_torso_generator_host import reference_like_torso_model
    from test_torso_motion_host import reference_like_estimator
    tm = reference_like_torso_model(sg, sp)
    tm.motion_field_estimator = reference_like_estimator(sm, 4)
    with torch.no_grad():
        tm.motion_field_estimator.compress.weight.mul_(FEATS_SCALE)
    tm.appearance_extractor = reference_like_extractor(se, 5)

    @torch.no_grad()
    def forward(torso_src_img, segmap, kp_s, kp_d, tgt_head_img, tgt_head_weights):
        torso_segmap = F.interpolate(segmap[:, [2, 4]].float(), size=(torso_src_img.shape[-2], torso_src_img.shape[-1]), mode="bilinear",
                                     align_corners=False, antialias=False)
        torso_src_img = torch.cat([torso_src_img, torso_segmap], dim=1)
        torso_appearance_feats = tm.appearance_extractor(torso_src_img)
        torso_appearance_feats, motion_inp_appearance_feats = glue(torso_appearance_feats, segmap)
        kp_s, kp_d = kp_s[:, KP_INDEX, :], kp_d[:, KP_INDEX, :]
        Rs = torch.eye(3, 3).unsqueeze(0).repeat([kp_s.shape[0], 1, 1]).to(kp_s.device)
        Rd = torch.eye(3, 3).unsqueeze(0).repeat([kp_d.shape[0], 1, 1]).to(kp_d.device)
        deformation, occlusion, occlusion_2 = tm.motion_field_estimator(motion_inp_appearance_feats, kp_s, kp_d, Rs, Rd, tgt_head_img, tgt_head_weights)
        rgb, hid = tm.deform_based_generator(torso_appearance_feats, deformation, occlusion, return_hid=True)
        occlusion_2 = tm.occlusion_2_predictor(torch.cat([hid, F.interpolate(occlusion_2, size=(256, 256), mode="bilinear")], dim=1))
        return rgb, {"occlusion": occlusion, "occlusion_2": occlusion_2, "deformed_torso_hid": hid}

    tm.forward = forward
    return tm


def synth_frame(seed):
    """One frame's inputs of the torso model: the 256^2 source image, a 6-class segmap at 512^2 whose classes 2 and 4 are smooth blobs in
    [0, 1], 68 key points of which the four the model selects are those of synth_torso_motion_inputs, the head image and its weights."""
    mi = synth.synth_torso_motion_inputs(seed, 1, 4)
    img = synth.synth_torso_appearance_inputs(seed + 1, 1, 3, 256, 256)["x"]
    lin = np.linspace(-1.0, 1.0, 512, dtype=np.float32)
    yy, xx = np.meshgrid(lin, lin, indexing="ij")
    seg = np.zeros((1, 6, 512, 512), np.float32)
    seg[0, 2] = 1.0 / (1.0 + np.exp(-8.0 * (0.6 - np.hypot(xx, yy - 0.5))))
    seg[0, 4] = 1.0 / (1.0 + np.exp(-8.0 * (0.35 - np.hypot(xx + 0.1, yy + 0.3))))
    kp_s, kp_d = (np.zeros((1, 68, 3), np.float32) + 0.05 * synth.hash_unitvar(seed + 2 + i, (1, 68, 3)) for i in range(2))
    kp_s[:, KP_INDEX], kp_d[:, KP_INDEX] = mi["kp_s"], mi["kp_d"]
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return T(img), T(seg), T(kp_s), T(kp_d), T(mi["tgt_head_img"]), T(mi["tgt_head_weights"])


def test_patch_model_routes_the_whole_torso_forward_to_the_hip_modules():
    """patch_model(torso_appearance=True, torso_generator=True, torso_motion=True): the stand-in's forward returns the rgb, occlusion and
    occlusion_2 of the fp64 chain extractor -> glue -> estimator -> generator -> occlusion_2_predictor, and no torch.nn.Conv* of the torso
    model runs."""
    from real3dportrait_amd import (patch_model, Occlusion2Predictor, TorsoAppearanceFeatureExtractor, TorsoGenerator,
                                    TorsoMotionFieldEstimator)
    from test_torso_generator_host import model_shell
    se, sm, sg, sp = 251, 252, 253, 254
    tm = stand_in_torso_model(se, sm, sg, sp).to(DEV)
    model = patch_model(model_shell(tm).to(DEV), torso_appearance=True, torso_generator=True, torso_motion=True)
    tm = model.superresolution.torso_model
    assert isinstance(tm.appearance_extractor, TorsoAppearanceFeatureExtractor) and isinstance(tm.motion_field_estimator, TorsoMotionFieldEstimator)
    assert isinstance(tm.deform_based_generator, TorsoGenerator) and isinstance(tm.occlusion_2_predictor, Occlusion2Predictor)
    ran = []
    hooks = [mod.register_forward_hook(lambda mod, i, o: ran.append(type(mod).__name__)) for mod in tm.modules()
             if isinstance(mod, (nn.Conv2d, nn.Conv3d))]
    img, seg, kp_s, kp_d, head, wts = synth_frame(255)
    rgb, ret = tm.forward(img, seg, kp_s, kp_d, head, wts)
    for h in hooks:
        h.remove()
    assert len(hooks) > 40 and ran == [], ran
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
    errs = {"rgb": rel(rgb.cpu().numpy(), rgb64.cpu().numpy()), "occlusion_2": rel(ret["occlusion_2"].cpu().numpy(), occ64.cpu().numpy()),
            "occlusion": rel(ret["occlusion"].cpu().numpy(), o64.cpu().numpy())}
    print("patched forward:", errs, "rms(feats) %.2f" % float(feats64.pow(2).mean().sqrt()))
    assert rgb.shape == (1, 3, 256, 256) and ret["occlusion_2"].shape == (1, 1, 256, 256) and ret["occlusion"].shape == (1, 1, 64, 64)
    assert all(e <= TOL for e in errs.values()), errs
