"""CPU: the motion-field estimator's host side (real3dportrait_amd/torso_motion.py, r3d_torso_conv3d and r3d_torso_motion_* of
include/r3d_hip.h).

The fp64 restatement (tests/torso_motion_ref64.py) against the reference's goldens, the fp64 fold (BatchNorm, channel padding, the
occlusion weights' permutation) against the restatement, the state_dict layout against the reference's key list, parameter-version
tracking, the patch_model swap, argument validation of the C entry points (which runs before any HIP call) and the stale-library report."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import load_golden
import torso_motion_ref64 as R64
from real3dportrait_amd import synth

GOLDENS = ["motion_a_k4", "motion_b_n2_k4", "motion_c_k9_rot"]
INPUT_ORDER = ("fs", "kp_s", "kp_d", "Rs", "Rd", "tgt_head_img", "tgt_head_weights")


def T(sd):
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}


def rel(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return float(np.abs(a - ref).max() / np.abs(ref).max())


def golden_case(name):
    """(golden, state_dict, inputs, K) -- parameters and inputs regenerated from the stored seeds."""
    g = load_golden(name)
    sp, sx, N, K, rot = (int(v) for v in g["spec"])
    return g, synth.synth_torso_motion(sp, K), synth.synth_torso_motion_inputs(sx, N, K, rotate=bool(rot)), K


def subsample(g, deformation, occ, occ2, mask=None):
    """The golden's strides applied to full outputs (tests/golden/make_golden_torso_motion.py)."""
    sdz, sm = (int(v) for v in g["strides"])
    out = {"deformation": deformation[:, ::sdz], "occlusion": occ, "occlusion_2": occ2}
    if mask is not None:
        out["mask"] = mask[:, :, ::sm, ::sm, ::sm]
    return out


def hip_estimator(sd, K):
    from real3dportrait_amd.torso_motion import MotionFieldEstimator
    m = MotionFieldEstimator(num_keypoints=K)
    m.load_state_dict(T(sd), strict=True)
    return m.eval()


def reference_like_estimator(seed=5, K=4, v1=False):
    """A stand-in for the reference's MotionFieldEstimator in plain torch, with its class name, attributes and state_dict keys, built by
    the reference's layer recipe (layers.py; BatchNorm for SyncBatchNorm, which evaluates the same in eval mode).  Its forward is the
    restatement in float32 on its own state_dict.  v1: network.py's estimator, which has no target-head branch."""
    def block(dim, pattern, ci, co, k):
        conv, norm = (nn.Conv2d, nn.BatchNorm2d) if dim == 2 else (nn.Conv3d, nn.BatchNorm3d)
        mods = {"C": conv(ci, co, k, 1, k // 2), "N": norm(co if pattern[0] == "C" else ci), "A": nn.ReLU(inplace=True)}
        m = nn.Module()
        m.layers = nn.Sequential(*[mods[c] for c in pattern])
        return m

    def wrap(*mods):
        m = nn.Module()
        m.layers = nn.Sequential(*mods)
        return m

    class MotionFieldEstimator(nn.Module):
        def __init__(self):
            super().__init__()
            down, up = [5 * (K + 1), 64, 128, 256, 512, 1024], [1024, 512, 256, 128, 64, 32]
            self.compress = nn.Conv3d(34, 4, 1, 1, 0)
            self.down = nn.Sequential(*[wrap(block(3, "CNA", down[i], down[i + 1], 3), nn.AvgPool3d((1, 2, 2))) for i in range(5)])
            self.up = nn.Sequential(*[wrap(nn.Upsample(scale_factor=(1, 2, 2)), block(3, "CNA", up[i], up[i + 1], 3)) for i in range(5)])
            if not v1:
                self.tgt_head_encoder = nn.Sequential(block(2, "CNA", 4, 32, 7),
                                                      *[wrap(block(2, "NAC", 32, 32, 3), block(2, "NAC", 32, 32, 3)) for _ in range(3)])
                self.tgt_head_fuser = nn.Conv3d(32 + down[0] + 32, 32, 7, 1, 3)
            self.mask_conv = nn.Conv3d(32, K + 1, 7, 1, 3)
            self.predict_multiref_occ = True
            self.occlusion_conv = nn.Conv2d(32 * 16, 1, 7, 1, 3)
            self.occlusion_conv2 = nn.Conv2d(32 * 16, 1, 7, 1, 3)

        @torch.no_grad()
        def forward(self, fs, kp_s, kp_d, Rs, Rd, tgt_head_img, tgt_head_weights):
            return R64.estimator(self.state_dict(), fs, kp_s, kp_d, Rs, Rd, tgt_head_img, tgt_head_weights, dtype=torch.float32)

    m = MotionFieldEstimator().eval()
    if not v1:
        m.load_state_dict(T(synth.synth_torso_motion(seed, K)), strict=True)
    return m


def torso_model_with(estimator, seed_g=5, seed_p=6):
    """The stand-in torso model of tests/test_torso_generator_host.py with a motion-field estimator and the part of the reference's
    forward that follows the appearance extractor and the mask glue (facev2v_warp/model2.py:248-263)."""
    from test_torso_generator_host import reference_like_torso_model
    tm = reference_like_torso_model(seed_g, seed_p)
    tm.motion_field_estimator = estimator

    @torch.no_grad()
    def forward(torso_appearance_feats, motion_inp_appearance_feats, kp_s, kp_d, tgt_head_img, tgt_head_weights):
        eye = torch.eye(3, 3).unsqueeze(0).repeat([kp_s.shape[0], 1, 1]).to(kp_s.device)
        deformation, occlusion, occlusion_2 = tm.motion_field_estimator(motion_inp_appearance_feats, kp_s, kp_d, eye, eye.clone(), tgt_head_img,
                                                                        tgt_head_weights)
        rgb, hid = tm.deform_based_generator(torso_appearance_feats, deformation, occlusion, return_hid=True)
        occlusion_2 = tm.occlusion_2_predictor(torch.cat([hid, F.interpolate(occlusion_2, size=(256, 256), mode="bilinear")], dim=1))
        return rgb, {"occlusion": occlusion, "occlusion_2": occlusion_2, "deformed_torso_hid": hid}

    tm.forward = forward
    return tm


def run_folded(Fd, inp64, head_in, K):
    """fold_motion's layers as the kernels evaluate them, in fp64 torch: the motion input padded to a multiple of 4 channels, conv +
    bias + ReLU + pool / nearest x2 + conv + bias + ReLU, the encoder as r3d_torso_conv layers, the concatenation with padded groups,
    fuser, mask logits, and the occlusions as one full-depth conv over (d, c)-ordered channels.  Returns (fused, mask logits, occlusions)."""
    cw = lambda w: w.permute(0, 4, 1, 2, 3)
    N, C, D, H, W = inp64.shape
    cp = (C + 3) // 4 * 4
    x0 = torch.cat([inp64, inp64.new_zeros(N, cp - C, D, H, W)], dim=1)
    x = x0
    for L in Fd["down"]:
        x = F.avg_pool3d(F.relu(R64.conv3d(x, cw(L["w"]), L["b"], 1)), (1, 2, 2))
    for L in Fd["up"]:
        x = F.relu(R64.conv3d(x.repeat_interleave(2, dim=3).repeat_interleave(2, dim=4), cw(L["w"]), L["b"], 1))
    h, res_in = head_in, None
    for l in Fd["enc"]:
        a = h
        if l["ps"] is not None:
            a = F.relu(a * l["ps"][None, :, None, None] + l["pt"][None, :, None, None])
            res_in = h
        y = F.conv2d(a, l["w"].permute(0, 3, 1, 2), l["b"], padding=l["k"] // 2)
        if l["act"] == 1:
            y = F.relu(y)
        h = y + res_in if l["res"] else y
    h = F.interpolate(h, size=(64, 64), mode="bilinear", align_corners=False)
    fuse = torch.cat([x0, x, h[:, :, None].expand(-1, -1, D, -1, -1)], dim=1)
    assert fuse.shape[1] == Fd["fuser"]["w"].shape[-1] == cp + 64
    fused = R64.conv3d(fuse, cw(Fd["fuser"]["w"]), Fd["fuser"]["b"], 3)
    logits = R64.conv3d(fused, cw(Fd["mask"]["w"]), Fd["mask"]["b"], 3)
    ow = Fd["occ"]["w"]                                                       # [2, D, 7, 7, 32]
    occ = torch.sigmoid(F.conv2d(fused.permute(0, 2, 1, 3, 4).reshape(N, -1, H, W), ow.permute(0, 1, 4, 2, 3).reshape(2, -1, 7, 7), Fd["occ"]["b"],
                                 padding=3))
    return fused, logits, occ


def test_state_dict_keys_are_the_reference_s():
    keys = [str(k) for k in load_golden("motion_keys")["estimator"]]
    m = hip_estimator(synth.synth_torso_motion(1, 4), 4)
    assert list(m.state_dict().keys()) == keys and len(keys) == 129
    shapes = dict(synth.torso_motion_shapes(4))
    assert list(shapes) == keys
    for k, v in m.state_dict().items():
        assert tuple(v.shape) == tuple(shapes[k]), k
    assert 38.8e6 < sum(int(np.prod(s)) for k, s in shapes.items() if not k.endswith("num_batches_tracked")) < 38.9e6
    m9 = hip_estimator(synth.synth_torso_motion(1, 9), 9)
    assert list(m9.state_dict().keys()) == keys and m9.down[0].layers[0].layers[0].in_channels == 50


def test_strict_load_from_a_reference_like_module():
    from real3dportrait_amd.torso_motion import MotionFieldEstimator, is_reference_motion_estimator
    ref = reference_like_estimator(5, 4)
    assert is_reference_motion_estimator(ref) and not is_reference_motion_estimator(reference_like_estimator(v1=True))
    m = MotionFieldEstimator.from_reference(ref)
    assert not is_reference_motion_estimator(m)
    for k, v in ref.state_dict().items():
        assert torch.equal(m.state_dict()[k], v) and m.state_dict()[k].dtype == v.dtype, k
    sd = T(synth.synth_torso_motion(5, 4))
    for missing in ("down.3.layers.0.layers.1.running_var", "tgt_head_encoder.2.layers.1.layers.2.bias", "occlusion_conv2.weight",
                    "up.0.layers.1.layers.1.weight"):
        with pytest.raises(RuntimeError, match="Missing key"):
            MotionFieldEstimator().load_state_dict({k: v for k, v in sd.items() if k != missing}, strict=True)
    with pytest.raises(RuntimeError, match="Unexpected key"):
        MotionFieldEstimator().load_state_dict(dict(sd, extra=torch.zeros(1)), strict=True)


def test_unsupported_configurations_raise():
    from real3dportrait_amd.torso_motion import MotionFieldEstimator
    for kw in ({"model_scale": "small"}, {"predict_multiref_occ": False}):
        with pytest.raises(NotImplementedError, match="network2.py"):
            MotionFieldEstimator(**kw)
    m = MotionFieldEstimator()
    z = torch.zeros
    good = dict(fs=z(1, 34, 16, 64, 64), kp_s=z(1, 4, 3), kp_d=z(1, 4, 3), Rs=z(1, 3, 3), Rd=z(1, 3, 3), tgt_head_img=z(1, 3, 256, 256),
                tgt_head_weights=z(1, 1, 256, 256))
    for k, bad in (("fs", z(1, 34, 16, 32, 32)), ("fs", z(1, 32, 16, 64, 64)), ("tgt_head_img", z(1, 3, 128, 128)), ("kp_s", z(1, 9, 3)),
                   ("Rd", z(1, 3, 2)), ("tgt_head_weights", z(2, 1, 256, 256))):
        with pytest.raises(ValueError):
            m(**dict(good, **{k: bad}))


@pytest.mark.parametrize("name", GOLDENS)
def test_fp64_restatement_matches_reference_goldens(name):
    torch.set_num_threads(8)
    g, sd, inp, K = golden_case(name)
    parts = {}
    with torch.no_grad():
        d, o, o2 = R64.estimator(sd, *[torch.from_numpy(inp[k]) for k in INPUT_ORDER], parts=parts)
    errs = {k: rel(v.numpy(), g[k]) for k, v in subsample(g, d, o, o2, parts["mask"]).items()}
    print(name, errs)
    assert all(e <= 1e-4 for e in errs.values()), errs


def test_sample_restatement_equals_grid_sample():
    g = torch.Generator().manual_seed(3)
    vol = torch.randn(2, 4, 5, 7, 6, generator=g, dtype=torch.float64)
    grid = torch.rand(2, 3, 9, 4, 3, generator=g, dtype=torch.float64) * 3.0 - 1.5
    grid[0, 0, 0, :, :] = 1.0
    grid[0, 0, 1, :, :] = -1.0
    ref = F.grid_sample(vol, grid, align_corners=True, padding_mode="zeros")
    assert float((R64.sample_zeros(vol, grid) - ref).abs().max()) <= 1e-14 * float(ref.abs().max())
    x, w, b = torch.randn(2, 3, 4, 5, 6, generator=g, dtype=torch.float64), torch.randn(5, 3, 3, 3, 3, generator=g, dtype=torch.float64), torch.randn(5, dtype=torch.float64)
    assert float((R64.conv3d(x, w, b, 1) - F.conv3d(x, w, b, padding=1)).abs().max()) <= 1e-13


def test_fp64_fold_equals_the_fp64_restatement():
    """The BatchNorm of every "CNA" conv folded into weight and bias, the ResBlock2D fold, the zero columns of the padded channel groups and
    the (d, c) order of the occlusion weights."""
    from real3dportrait_amd.torso_motion import fold_motion
    torch.set_num_threads(8)
    K = 9
    sd = synth.synth_torso_motion(7, K)
    inp = {k: torch.from_numpy(v) for k, v in synth.synth_torso_motion_inputs(8, 1, K, rotate=True).items()}
    parts = {}
    with torch.no_grad():
        d, o, o2 = R64.estimator(sd, *[inp[k] for k in INPUT_ORDER], parts=parts)
        Fd = fold_motion(hip_estimator(sd, K), torch.float64)
        assert all(l["w"].dtype == torch.float64 for l in Fd["down"] + Fd["up"] + Fd["enc"] + [Fd["fuser"], Fd["mask"], Fd["occ"], Fd["compress"]])
        assert Fd["down"][0]["w"].shape == (64, 3, 3, 3, 52) and Fd["fuser"]["w"].shape == (32, 7, 7, 7, 116)
        head_in = F.interpolate(torch.cat([inp["tgt_head_img"], inp["tgt_head_weights"]], dim=1).double(), size=(128, 128), mode="bilinear",
                                align_corners=False)
        fused, logits, occ = run_folded(Fd, parts["input"], head_in, K)
    e = {"fused": rel(fused.numpy(), parts["fused"].numpy()), "mask": rel(torch.softmax(logits, 1).numpy(), parts["mask"].numpy()),
         "occlusion": rel(occ[:, :1].numpy(), o.numpy()), "occlusion_2": rel(occ[:, 1:].numpy(), o2.numpy())}
    cwt = torch.from_numpy(sd["compress.weight"]).double().reshape(4, -1)
    assert torch.equal(Fd["compress"]["w"], cwt)
    print("fold vs restatement:", e)
    assert all(v <= 1e-12 for v in e.values()), e


def test_jacobian_is_rs_times_the_inverse_of_rd():
    from real3dportrait_amd.torso_motion import jacobian
    i = synth.synth_torso_motion_inputs(3, 3, 4, rotate=True)
    Rs, Rd = torch.from_numpy(i["Rs"]).double(), torch.from_numpy(i["Rd"]).double()
    assert float((Rs - torch.eye(3)).abs().max()) > 0.1 and not torch.equal(Rs, Rd)
    J = jacobian(Rs, Rd)
    assert float((J - Rs @ torch.linalg.inv(Rd)).abs().max()) <= 1e-14
    one = jacobian(Rs[1:2].float(), Rd[1:2].float())
    assert torch.equal(jacobian(Rs.float(), Rd.float())[1:2], one)
    eye = torch.eye(3)[None]
    assert torch.equal(jacobian(eye, eye.clone()), eye)


def test_in_place_parameter_edits_are_seen_by_the_next_prepare():
    m = hip_estimator(synth.synth_torso_motion(5, 4), 4)
    a = m._prepare()
    assert m._prepare() is a
    w0 = a["down"][1]["w"].clone()
    with torch.no_grad():
        m.down[1].layers[0].layers[0].weight.add_(0.01)
    b = m._prepare()
    assert b is not a and not torch.equal(b["down"][1]["w"], w0) and torch.equal(b["down"][0]["w"], a["down"][0]["w"])
    with torch.no_grad():
        m.tgt_head_encoder[2].layers[0].layers[0].running_var.mul_(2.0)
    c = m._prepare()
    assert c is not b and not torch.equal(c["enc"][3]["ps"], b["enc"][3]["ps"])
    with torch.no_grad():
        m.occlusion_conv2.bias.add_(1.0)
    d = m._prepare()
    assert d is not c and float(d["occ"]["b"][1] - c["occ"]["b"][1]) == pytest.approx(1.0, abs=1e-6) and torch.equal(d["occ"]["b"][0], c["occ"]["b"][0])
    # a parameter replaced by another tensor at the same address and version (what the caching allocator makes of a freed one)
    from test_state_host import replaced_at_same_address
    e, f = replaced_at_same_address(m.down[1].layers[0].layers[0], "weight", m._prepare)
    assert f is not e and not torch.equal(f["down"][1]["w"], e["down"][1]["w"]) and torch.equal(f["down"][0]["w"], e["down"][0]["w"])
    assert m._prepare() is f


def test_patch_model_swaps_the_estimator_only_with_the_flag():
    from real3dportrait_amd import patch_model, TorsoMotionFieldEstimator
    from test_torso_generator_host import model_shell
    est = reference_like_estimator(5, 4)
    tm = torso_model_with(est)
    gen = tm.deform_based_generator
    patch_model(model_shell(tm))
    assert tm.motion_field_estimator is est
    patch_model(model_shell(tm), torso_generator=False, torso_motion=False)
    assert tm.motion_field_estimator is est
    before = {k: v.clone() for k, v in tm.state_dict().items()}
    patch_model(model_shell(tm), torso_motion=True)
    assert isinstance(tm.motion_field_estimator, TorsoMotionFieldEstimator) and tm.deform_based_generator is gen
    after = tm.state_dict()
    assert list(after) == list(before)
    for k, v in before.items():
        assert after[k].dtype == v.dtype and torch.equal(after[k], v), k


def test_patch_model_leaves_a_v1_estimator_alone():
    from real3dportrait_amd import patch_model
    from test_torso_generator_host import model_shell
    est = reference_like_estimator(v1=True)
    tm = torso_model_with(est)
    patch_model(model_shell(tm), torso_motion=True)
    assert tm.motion_field_estimator is est
    tm.motion_field_estimator = nn.Conv2d(1, 1, 1)
    patch_model(model_shell(tm), torso_motion=True)
    assert type(tm.motion_field_estimator) is nn.Conv2d


def test_c_entry_points_reject_bad_arguments_without_a_gpu():
    from real3dportrait_amd import _lib
    lib = _lib.load()
    assert lib.r3d_version() == _lib.ABI_VERSION
    at = lambda i: ctypes.c_void_p((1 << 30) + 4 * i)       # never dereferenced: validation fails first
    far, far2, far3 = ctypes.c_void_p(1 << 40), ctypes.c_void_p(1 << 41), ctypes.c_void_p(1 << 42)
    err = lambda: lib.r3d_last_error()

    def conv(x, w, y, yn=None, B=1, D=4, H=8, W=8, Cin=32, Cout=64, k=3, up=0, full=0, act=0, pool=0, ycs=None, yco=0):
        return lib.r3d_torso_conv3d(x, B, D, H, W, Cin, up, w, None, Cout, k, full, act, 0.0, pool, y, Cout if ycs is None else ycs, yco, yn, None)

    assert conv(None, far, far2) == -1 and b"NULL" in err()
    assert conv(at(0), None, far2) == -1 and b"NULL" in err()
    assert conv(at(0), far, None) == -1 and b"NULL" in err()                       # no output at all
    assert conv(at(0), far, far2, k=5) == -1 and b"ksize 5" in err()
    assert conv(at(0), far, far2, up=2) == -1 and b"upsample 2" in err()
    assert conv(at(0), far, far2, act=3) == -1 and b"act 3" in err()
    assert conv(at(0), far, far2, pool=2) == -1 and b"pool 2" in err()
    assert conv(at(0), far, far2, full=-1) == -1 and b"full_depth -1" in err()
    assert conv(at(0), far, far2, D=0) == -1 and b"bad argument" in err()
    assert conv(at(0), far, far2, Cin=0) == -1 and b"bad argument" in err()
    assert conv(at(0), far, far2, Cout=5000) == -1 and b"bad argument" in err()
    assert conv(at(0), far, far2, H=7, pool=1) == -1 and b"odd size" in err()
    assert conv(at(0), far, far2, W=5, pool=1) == -1 and b"odd size" in err()
    assert conv(at(0), far, far2, far3, pool=1) == -1 and b"channel-last only" in err()
    assert conv(at(0), far, far2, ycs=63) == -1 and b"does not fit" in err()
    assert conv(at(0), far, far2, ycs=92, yco=29) == -1 and b"does not fit" in err()
    assert conv(at(0), far, far2, yco=-1) == -1 and b"does not fit" in err()
    # x [1, 4, 8, 8, 32] = 8192 floats; y rows of 64: 16384 floats, of 92: 23552
    assert conv(at(0), far, at(8191)) == -1 and b"overlaps x" in err()
    assert conv(at(16383), far, at(0)) == -1 and b"overlaps x" in err()
    assert conv(at(23551), far, at(0), ycs=92, yco=28) == -1 and b"overlaps x" in err()
    assert conv(at(100000), far, None, at(99999)) == -1 and b"overlaps x" in err()
    assert conv(at(100000), far, at(0), at(16383)) == -1 and b"y and y_ncdhw" in err()
    assert conv(at(100000), at(0), at(64 * 27 * 32 - 1)) == -1 and b"overlaps x, w" in err()

    def minput(fs, cw, cb, ks, kd, J, inp, fuse, N=1, C=34, D=16, H=64, W=64, K=4, ic=28, fcs=92):
        return lib.r3d_torso_motion_input(fs, N, C, D, H, W, cw, cb, ks, kd, J, K, inp, ic, fuse, fcs, None)

    ok = (at(0), far, far, far, far, far)
    assert minput(None, far, far, far, far, far, far2, far3) == -1 and b"NULL" in err()
    assert minput(*ok[:5], None, far2, far3) == -1 and b"NULL" in err()
    assert minput(*ok, None, far3) == -1 and b"NULL" in err()
    assert minput(*ok, far2, far3, W=1) == -1 and b"bad argument" in err()
    assert minput(*ok, far2, far3, K=0) == -1 and b"bad argument" in err()
    assert minput(*ok, far2, far3, ic=24) == -1 and b"bad argument" in err()
    assert minput(*ok, far2, far3, fcs=27) == -1 and b"bad argument" in err()
    assert minput(*ok, far2, far3, C=0) == -1 and b"bad argument" in err()
    assert minput(*ok, at(65536 * 34 - 1), far3) == -1 and b"overlaps an input" in err()
    assert minput(*ok, far2, at(65536 * 34 - 1)) == -1 and b"overlaps an input" in err()
    assert minput(*ok, at(10 ** 7), at(10 ** 7 + 65536 * 28 - 1)) == -1 and b"inp and fuse" in err()
    assert minput(*ok, far2, None, W=1) == -1 and b"bad argument" in err()

    deform = lambda mask, ks, kd, J, out, N=1, D=16, H=64, W=64, K=4: lib.r3d_torso_motion_deform(mask, N, D, H, W, K, ks, kd, J, out, None)
    assert deform(None, far, far, far, far2) == -1 and b"NULL" in err()
    assert deform(at(0), far, None, far, far2) == -1 and b"NULL" in err()
    assert deform(at(0), far, far, far, None) == -1 and b"NULL" in err()
    assert deform(at(0), far, far, far, far2, D=1) == -1 and b"bad argument" in err()
    assert deform(at(0), far, far, far, far2, K=65) == -1 and b"bad argument" in err()
    assert deform(at(0), far, far, far, at(65536 * 5 - 1)) == -1 and b"overlaps an input" in err()

    bc = lambda feats, fuse, N=1, C=32, H=64, W=64, D=16, fcs=92, fco=60: lib.r3d_torso_motion_broadcast(feats, N, C, H, W, D, fuse, fcs, fco, None)
    assert bc(None, far) == -1 and b"NULL" in err()
    assert bc(at(0), None) == -1 and b"NULL" in err()
    assert bc(at(0), far, D=0) == -1 and b"bad argument" in err()
    assert bc(at(0), far, fco=61) == -1 and b"bad argument" in err()
    assert bc(at(0), far, fco=-1) == -1 and b"bad argument" in err()
    assert bc(at(0), at(32 * 4096 - 1)) == -1 and b"overlaps feats" in err()


def test_load_reports_a_library_without_a_bound_symbol_as_stale(monkeypatch):
    """New functions arrive without a new ABI number, so a stale in-tree library passes the version check: load() must name the missing
    symbol and say to rebuild, not raise AttributeError."""
    from real3dportrait_amd import _lib
    _lib.load()
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "SIGNATURES", dict(_lib.SIGNATURES, r3d_torso_not_built_yet=(ctypes.c_int, [])))
    with pytest.raises(RuntimeError, match="does not export r3d_torso_not_built_yet.*rebuild"):
        _lib.load()
    assert _lib._lib is None


def test_motion_kernels_do_not_use_scratch():
    from test_render_kernel_resources import _kernel_metadata
    from real3dportrait_amd import _lib
    meta = _kernel_metadata(_lib.LIB_PATH)
    names = [k for k in meta if "7tmotion" in k]
    assert len(names) == 13, names          # motion_input, motion_deform, motion_broadcast, conv3d x (5 tiles x 2 loaders)
    for k in names:
        assert int(meta[k]["private_segment_fixed_size"]) == 0, (k, meta[k])
        assert int(meta[k]["vgpr_spill_count"]) == 0, (k, meta[k])
