"""CPU: the host side of the HIP torso forward (real3dportrait_amd/torso_forward.py, r3d_torso_seg_input / r3d_torso_mask_volume of
include/r3d_hip.h).

The fp64 restatement of the glue (tests/torso_glue_ref64.py) against the reference's goldens, the premises of the exact case, argument
validation of the two C entry points (which runs before any HIP call), the patch_model switch and its refusals, the losses against the
reference's formulas, and the kernels' scratch use."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import load_golden
import torso_glue_ref64 as G64
from real3dportrait_amd import synth

GOLDENS = ["torso_glue_down_50x37", "torso_glue_up_3x3"]
GOLDEN_KEYS = ("seg", "mask_d", "motion", "seg_in")
# the exact cases: (seed, N, Hs, Ws, h, w, ksize, centres, specks); every size ratio is 8
EXACT = {"512_to_64": (1, 2, 512, 512, 64, 64, 7, 10, 24), "32x56_to_4x7": (9, 1, 32, 56, 4, 7, 3, 5, 3)}


def golden_case(name):
    """(golden, segmap, feats, img) -- the inputs regenerated from the stored seed."""
    g = load_golden(name)
    seed, N, Cs, Hs, Ws, C, D, h, w, ksize, IH, IW = (int(v) for v in g["spec"])
    inp = synth.synth_torso_glue_inputs(seed, N, Cs, Hs, Ws, C, D, h, w)
    return g, inp["segmap"], inp["feats"], synth.synth_torso_appearance_inputs(seed + 1, N, 3, IH, IW)["x"], ksize


def exact_case(name):
    seed, N, Hs, Ws, h, w, ksize, centres, specks = EXACT[name]
    seg = synth.synth_torso_onehot_segmap(seed, N, 6, Hs, Ws, centres, specks, ratio=Hs // h)
    return seg, synth.hash_unitvar(seed + 100, (N, 32, 16, h, w)), ksize


@pytest.mark.parametrize("name", GOLDENS)
def test_fp64_restatement_matches_reference_goldens(name):
    g, seg, feats, img, ksize = golden_case(name)
    out = G64.glue(feats, seg, 2, 4, ksize)
    out["seg_in"] = G64.seg_input(img, seg)
    assert np.array_equal(g["seg_in"][:, :3], img)                    # the reference's cat copies the image
    assert not np.array_equal(g["mask_d"][0], g["mask_d"][1])
    for k, e32 in zip(GOLDEN_KEYS, g["e32"]):
        e = G64.rel(g[k], out[k].numpy())
        print(name, k, "restatement against the golden %.2e, the reference's own error %.2e" % (e, e32))
        assert e <= G64.bound(float(e32)), (name, k, e, float(e32))


def test_reflect_window_of_the_restatement_is_torch_s():
    """dilate against F.pad(mode='reflect') + max_pool2d in fp64 (a maximum: exact), up to the largest window an image takes."""
    m = torch.from_numpy(synth.hash_unitvar(3, (2, 5, 7))).double()
    for ksize in (1, 3, 5, 7, 9):
        pad = (ksize - 1) // 2
        ref = F.max_pool2d(F.pad(m[:, None], pad=[pad] * 4, mode="reflect"), kernel_size=ksize, stride=1)[:, 0]
        assert torch.equal(G64.dilate(m, ksize), ref), ksize
    with pytest.raises(AssertionError):
        G64.dilate(m, 11)                                              # pad 5 = the height: reflect padding's own limit


@pytest.mark.parametrize("name", sorted(EXACT))
def test_exact_case_premises(name):
    """One-hot labels in blobs and an integer ratio of 8: every resize weight is 1/2, so float32 torch IS the fp64 result rounded, and the
    dilated mask has zeros, ones and values between them."""
    seg, feats, ksize = exact_case(name)
    assert set(np.unique(seg)) == {0.0, 1.0} and np.array_equal(seg.sum(axis=1), np.ones_like(seg[:, 0]))
    r64, r32 = G64.glue(feats, seg, 2, 4, ksize), G64.torch_glue(feats, seg, 2, 4, ksize)
    for k in r64:
        assert torch.equal(r64[k].float(), r32[k]), k
    md = r64["mask_d"].numpy()
    cover = [float((md == 0).mean()), float(((md > 0) & (md < 1)).mean()), float((md == 1).mean())]
    print(name, "mask_d == 0 / between / == 1:", cover)
    assert min(cover) >= 0.05, cover


def test_c_entry_points_reject_bad_arguments_without_a_gpu():
    from real3dportrait_amd import _lib
    lib = _lib.load()
    assert lib.r3d_version() == _lib.ABI_VERSION
    at = lambda i: ctypes.c_void_p((1 << 30) + 4 * i)       # never dereferenced: validation fails first
    far, far2, far3 = (ctypes.c_void_p(1 << s) for s in (40, 41, 42))
    err = lambda: lib.r3d_last_error()

    def seg_in(img, seg, out, N=1, Ci=3, Cs=6, Hs=16, Ws=16, c0=2, c1=4, OH=8, OW=8):
        return lib.r3d_torso_seg_input(img, N, Ci, seg, Cs, Hs, Ws, c0, c1, out, OH, OW, None)

    assert seg_in(None, far, far2) == -1 and b"NULL" in err()
    assert seg_in(at(0), None, far2) == -1 and b"NULL" in err()
    assert seg_in(at(0), far, None) == -1 and b"NULL" in err()
    assert seg_in(at(0), far, far2, Cs=4) == -1 and b"segmap of 4 channels" in err()
    assert seg_in(at(0), far, far2, Cs=5, c1=5) == -1 and b"segmap of 5 channels" in err()
    assert seg_in(at(0), far, far2, c0=-1) == -1 and b"channels -1 and 4" in err()
    assert seg_in(at(0), far, far2, Ci=-1) == -1 and b"bad argument" in err()
    assert seg_in(at(0), far, far2, OH=0) == -1 and b"bad argument" in err()
    assert seg_in(at(0), far, far2, N=0) == -1 and b"bad argument" in err()
    # img [1, 3, 8, 8] = 192 floats, segmap [1, 6, 16, 16] = 1536, out [1, 5, 8, 8] = 320
    assert seg_in(at(0), far, at(191)) == -1 and b"overlaps" in err()
    assert seg_in(at(319), far, at(0)) == -1 and b"overlaps" in err()
    assert seg_in(far, at(0), at(1535)) == -1 and b"overlaps" in err()
    assert seg_in(None, at(0), at(127), Ci=0) == -1 and b"overlaps" in err()          # no image: out [1, 2, 8, 8] = 128 floats

    def mask(f, seg, m, mo, N=1, D=2, H=8, W=8, C=4, Cs=6, Hs=16, Ws=16, c0=2, c1=4, k=7, mul=1):
        return lib.r3d_torso_mask_volume(f, N, D, H, W, C, seg, Cs, Hs, Ws, c0, c1, k, mul, m, mo, None)

    assert mask(None, far, far2, far3) == -1 and b"NULL" in err()
    assert mask(at(0), None, far2, far3) == -1 and b"NULL" in err()
    assert mask(at(0), far, None, far3) == -1 and b"NULL" in err()
    assert mask(at(0), far, far2, None) == -1 and b"NULL" in err()
    assert mask(at(0), far, far2, far3, Cs=4) == -1 and b"segmap of 4 channels" in err()
    assert mask(at(0), far, far2, far3, Cs=2) == -1 and b"segmap of 2 channels" in err()
    assert mask(at(0), far, far2, far3, k=6) == -1 and b"ksize 6 is not odd" in err()
    assert mask(at(0), far, far2, far3, k=0) == -1 and b"ksize 0 is not odd" in err()
    assert mask(at(0), far, far2, far3, k=-3) == -1 and b"ksize -3 is not odd" in err()
    assert mask(at(0), far, far2, far3, k=17) == -1 and b"reflect padding 8" in err()                # pad 8 = min(H, W)
    assert mask(at(0), far, far2, far3, H=3, k=7) == -1 and b"reflect padding 3" in err()
    assert mask(at(0), far, far2, far3, H=256, W=256, D=1, k=119) == -1 and b"LDS" in err()
    assert mask(at(0), far, far2, far3, D=0) == -1 and b"bad argument" in err()
    assert mask(at(0), far, far2, far3, C=0) == -1 and b"bad argument" in err()
    assert mask(at(0), far, far2, far3, N=70000) == -1 and b"bad argument" in err()
    # feats and masked [1, 2, 8, 8, 4] = 512 floats, motion [1, 2, 8, 8, 6] = 768, segmap 1536
    assert mask(at(0), far, at(511), far3) == -1 and b"without being feats_cl" in err()             # a shifted overlap is not "in place"
    assert mask(at(511), far, at(0), far3) == -1 and b"without being feats_cl" in err()
    assert mask(at(0), far, far2, at(511)) == -1 and b"an output overlaps" in err()                  # motion on feats
    assert mask(at(767), far, far2, at(0)) == -1 and b"an output overlaps" in err()
    assert mask(at(0), far, at(0), at(511)) == -1 and b"an output overlaps" in err()                 # in place, motion on both
    assert mask(far, far2, at(0), at(511)) == -1 and b"an output overlaps" in err()                  # the two outputs
    assert mask(far, at(0), at(1535), far3) == -1 and b"an output overlaps" in err()                 # masked on the segmap
    assert mask(far, at(0), far2, at(1535)) == -1 and b"an output overlaps" in err()                 # motion on the segmap


def test_header_signatures_and_library_agree():
    from real3dportrait_amd import _lib
    lib = _lib.load()
    for name in ("r3d_torso_seg_input", "r3d_torso_mask_volume"):          # (header against table: tests/test_abi.py)
        assert name in _lib.SIGNATURES and hasattr(lib, name)


def test_glue_kernels_do_not_use_scratch():
    from test_render_kernel_resources import _kernel_metadata
    from real3dportrait_amd import _lib
    meta = _kernel_metadata(_lib.LIB_PATH)
    names = [k for k in meta if "tglue" in k]
    assert len(names) == 3, names          # seg_input, mask_volume x (16-byte accesses | one float)
    for k in names:
        assert int(meta[k]["private_segment_fixed_size"]) == 0, (k, meta[k])
        assert int(meta[k]["vgpr_spill_count"]) == 0, (k, meta[k])


_STAND_IN = []


def stand_in():
    """The stand-in torso model of tests/test_gpu_torso_appearance.py inside the smallest model patch_model accepts: built once, a copy
    per call (a copy's own torch `forward` still drives the first build's modules; these tests only ask which object is bound)."""
    import copy
    from test_gpu_torso_appearance import stand_in_torso_model
    from test_torso_generator_host import model_shell
    if not _STAND_IN:
        _STAND_IN.append(stand_in_torso_model(251, 252, 253, 254))
    tm = copy.deepcopy(_STAND_IN[0])
    return tm, model_shell(tm)


def test_patch_model_needs_the_three_module_switches():
    from real3dportrait_amd import patch_model
    tm, model = stand_in()
    fwd = tm.forward
    for kw in ({}, {"torso_appearance": True}, {"torso_appearance": True, "torso_motion": True}, {"torso_generator": True, "torso_motion": True},
               {"torso_appearance": True, "torso_generator": True}):
        with pytest.raises(ValueError, match="torso_forward=True needs torso_appearance=True, torso_motion=True and torso_generator=True"):
            patch_model(model, torso_forward=True, **kw)
    assert tm.forward is fwd and not hasattr(tm, "_r3d_torso_forward")
    assert type(tm.appearance_extractor).__module__ == "test_torso_appearance_host"            # a refused call swaps nothing


def test_patch_model_binds_the_forward_only_with_the_flag():
    import inspect
    from real3dportrait_amd import patch_model, torso_model_forward
    from real3dportrait_amd.torso_forward import TorsoForwardState
    tm, model = stand_in()
    fwd = tm.forward
    patch_model(model)
    assert tm.forward is fwd
    patch_model(model, torso_appearance=True, torso_motion=True, torso_generator=True)
    assert tm.forward is fwd
    patch_model(model, torso_appearance=True, torso_motion=True, torso_generator=True, torso_forward=False)
    assert tm.forward is fwd and not hasattr(tm, "_r3d_torso_forward")
    tm, model = stand_in()
    fwd = tm.forward
    patch_model(model, torso_appearance=True, torso_motion=True, torso_generator=True, torso_forward=True)
    assert tm.forward is not fwd and tm.forward.__func__ is torso_model_forward and tm.forward.__self__ is tm
    assert tm._r3d_reference_forward is fwd and isinstance(tm._r3d_torso_forward, TorsoForwardState)
    assert list(inspect.signature(tm.forward).parameters) == ["torso_src_img", "segmap", "kp_s", "kp_d", "tgt_head_img", "tgt_head_weights",
                                                               "cal_loss", "target_torso_mask"]          # model2.py:222
    assert "forward" not in tm.state_dict() and not any(k.startswith("_r3d") for k in tm.state_dict())


def test_patch_model_leaves_forward_alone_when_a_swap_is_refused():
    from real3dportrait_amd import patch_model
    from test_torso_appearance_host import reference_like_extractor
    every = dict(torso_appearance=True, torso_motion=True, torso_generator=True, torso_forward=True)
    tm, model = stand_in()
    tm.appearance_extractor = reference_like_extractor(n_res=4)          # another architecture under the class name
    fwd = tm.forward
    patch_model(model, **every)
    assert tm.forward is fwd and not hasattr(tm, "_r3d_torso_forward")
    tm, model = stand_in()
    del tm.motion_field_estimator.tgt_head_encoder                        # the v1 estimator has no target-head branch
    fwd = tm.forward
    patch_model(model, **every)
    assert tm.forward is fwd
    tm, model = stand_in()
    tm.deform_based_generator = nn.Conv2d(1, 1, 1)
    fwd = tm.forward
    patch_model(model, **every)
    assert tm.forward is fwd


def test_forward_refuses_what_the_reference_refuses():
    from real3dportrait_amd import patch_model
    tm, model = stand_in()
    patch_model(model, torso_appearance=True, torso_motion=True, torso_generator=True, torso_forward=True)
    z = torch.zeros
    args = (z(1, 3, 256, 256), z(1, 6, 512, 512), z(1, 68, 3), z(1, 68, 3), z(1, 3, 256, 256), z(1, 1, 256, 256))
    tm.hparams = {"torso_kp_num": 5}
    with pytest.raises(NotImplementedError, match="torso_kp_num 5"):
        tm.forward(*args)
    tm.hparams = {"torso_kp_num": 4}
    with pytest.raises(ValueError, match="torso_src_img"):
        tm.forward(z(1, 4, 256, 256), *args[1:])
    with pytest.raises(ValueError, match="torso_src_img"):
        tm.forward(z(1, 3, 254, 256), *args[1:])
    with pytest.raises(ValueError, match="torso_src_img"):
        tm.forward(args[0], z(2, 6, 512, 512), *args[2:])


def test_losses_are_the_reference_s():
    """model2.py:264-279 and masked_l1_reg_loss (:289-298), restated here line by line, on both target_torso_mask branches."""
    from real3dportrait_amd.torso_forward import losses
    occ = torch.from_numpy(synth.hash_uniform(5, 2 * 64 * 64).reshape(2, 1, 64, 64))
    occ2 = torch.from_numpy(synth.hash_uniform(6, 2 * 256 * 256).reshape(2, 1, 256, 256))
    occ2[0, 0, :4] = 0.0
    occ2[1, 0, :4] = 1.0                                                    # the clamp of :264 matters
    alphas = occ2.clamp(1e-5, 1 - 1e-5)
    entropy = torch.mean(- alphas * torch.log2(alphas) - (1 - alphas) * torch.log2(1 - alphas))
    got = losses(occ, occ2)
    assert list(got) == ["facev2v/occlusion_reg_l1", "facev2v/occlusion_2_reg_l1", "facev2v/occlusion_2_weights_entropy"]
    assert torch.equal(got["facev2v/occlusion_reg_l1"], occ.mean()) and torch.equal(got["facev2v/occlusion_2_reg_l1"], occ2.mean())
    assert torch.equal(got["facev2v/occlusion_2_weights_entropy"], entropy) and bool(torch.isfinite(entropy))

    def masked_l1_reg_loss(img_pred, mask, masked_weight=0.01, unmasked_weight=0.001):
        masked_weight = 1.0
        weight_mask = mask.float() * masked_weight + (~mask).float() * unmasked_weight
        return ((img_pred).abs().sum(dim=1) * weight_mask).mean()

    target = torch.from_numpy(synth.hash_uniform(7, 2 * 512 * 512).reshape(2, 512, 512) > 0.6)
    m1 = F.interpolate((~target).unsqueeze(1).float(), size=occ.shape[-2:])
    m2 = F.interpolate((~target).unsqueeze(1).float(), size=occ2.shape[-2:])
    got = losses(occ, occ2, target, 0.3)
    assert list(got) == ["facev2v/occlusion_reg_l1", "facev2v/occlusion_2_reg_l1", "facev2v/occlusion_2_weights_entropy"]
    assert torch.equal(got["facev2v/occlusion_reg_l1"], masked_l1_reg_loss(occ, m1.bool(), masked_weight=1, unmasked_weight=0.3))
    assert torch.equal(got["facev2v/occlusion_2_reg_l1"], masked_l1_reg_loss(occ2, m2.bool(), masked_weight=1, unmasked_weight=0.3))
    assert torch.equal(got["facev2v/occlusion_2_weights_entropy"], entropy)
    assert not torch.equal(got["facev2v/occlusion_reg_l1"], occ.mean())


def test_launch_count_is_the_sum_of_the_modules():
    import real3dportrait_amd
    import real3dportrait_amd.torso_forward as tf
    from real3dportrait_amd import torso_appearance
    assert tf.LAUNCHES == 64 == 2 + torso_appearance.LAUNCHES + 25 + 18 + 3
    assert real3dportrait_amd.torso_model_forward is tf.forward and real3dportrait_amd.torso_seg_input is tf.seg_input
    assert real3dportrait_amd.torso_mask_volume is tf.mask_volume
