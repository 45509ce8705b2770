"""GPU: the torso modules built with precision='bf16x3' (real3dportrait_amd/torso_precision.py): the goldens of the exact
tier's tests at their tolerance; fresh inputs against the fp64 restatements, held both to that tolerance and to the exact tier's own error
on the same inputs; bit-identity across batch, repeats and streams; the launch counts of the exact tier under the _prec names; the patched
stand-in chain estimator -> generator -> predictor."""
import collections

import pytest
import torch

import test_gpu_torso_generator as TG
import test_gpu_torso_motion as TM
import torso_motion_ref64 as R64
import torso_ref64 as G64
from test_torso_generator_host import model_shell
from test_torso_motion_host import reference_like_estimator, torso_model_with
from real3dportrait_amd import _lib, synth
from real3dportrait_amd.torso_generator import Generator, Occlusion2Predictor
from real3dportrait_amd.torso_motion import MotionFieldEstimator

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2e-4
rel = TM.rel


def generator(sd, psd, precision="bf16x3"):
    from test_torso_generator_host import T
    gen, pred = Generator(precision=precision), Occlusion2Predictor(precision=precision)
    gen.load_state_dict(T(sd), strict=True)
    pred.load_state_dict(T(psd), strict=True)
    return gen.eval().to(DEV), pred.eval().to(DEV)


@pytest.fixture(autouse=True)
def bf16x3_modules(monkeypatch):
    """The builders the exact tier's tests use (hip_estimator, hip_generator, hip_predictor) build the modules of this tier, so that its
    tests can be run as they are."""
    from test_torso_generator_host import T

    def hip_generator(sd):
        m = Generator(precision="bf16x3")
        m.load_state_dict(T(sd), strict=True)
        return m.eval()

    def hip_predictor(psd):
        m = Occlusion2Predictor(precision="bf16x3")
        m.load_state_dict(T(psd), strict=True)
        return m.eval()

    def hip_estimator(sd, K):
        m = MotionFieldEstimator(num_keypoints=K, precision="bf16x3")
        m.load_state_dict(T(sd), strict=True)
        return m.eval()

    monkeypatch.setattr(TG, "hip_generator", hip_generator)
    monkeypatch.setattr(TG, "hip_predictor", hip_predictor)
    monkeypatch.setattr(TM, "hip_estimator", hip_estimator)


# ---- goldens: the exact tier's tests, with their loaders, subsampling and 2e-4, on this tier's modules --------------------------------
@pytest.mark.parametrize("name", TM.GOLDENS)
def test_motion_goldens(name):
    assert TM.TOL == TOL
    TM.test_goldens(name)


@pytest.mark.parametrize("name", TG.GOLDENS)
def test_generator_goldens(name):
    assert TG.TOL == TOL
    TG.test_goldens(name)


# ---- fresh inputs ------------------------------------------------------------------------------------------------------------------------
def _assert_fp32_class(what, e_bf, e_f32):
    print(what, "bf16x3", e_bf, "f32", e_f32)
    for k in e_bf:
        assert e_bf[k] <= TOL, (what, k, e_bf[k])
        assert e_bf[k] <= 2.0 * e_f32[k] + 1e-6, (what, k, e_bf[k], e_f32[k])


def test_motion_fresh_inputs_against_fp64_and_the_exact_tier():
    from test_torso_generator_host import T
    K = 4
    sd = synth.synth_torso_motion(281, K)
    args = TM.to_dev(synth.synth_torso_motion_inputs(283, 1, K, rotate=True))
    with torch.no_grad():
        ref = [t.cpu().numpy() for t in R64.estimator(sd, *args)]
    errs = {}
    for precision in ("bf16x3", "f32"):
        m = MotionFieldEstimator(num_keypoints=K, precision=precision)
        m.load_state_dict(T(sd), strict=True)
        out = m.eval().to(DEV)(*args)
        errs[precision] = {k: rel(o.cpu().numpy(), r) for k, o, r in zip(("deformation", "occlusion", "occlusion_2"), out, ref)}
    _assert_fp32_class("motion N1 K4:", errs["bf16x3"], errs["f32"])


def test_generator_fresh_inputs_against_fp64_and_the_exact_tier():
    sd, psd = synth.synth_torso_generator(281), synth.synth_torso_predictor(282)
    i = TG.to_dev(synth.synth_torso_inputs(283, 1, 24, 20))
    d64, rgb64, hid64 = G64.generator(sd, i["torso_appearance_feats"], i["deformation"])
    occ64 = G64.occlusion_2(psd, hid64, i["occlusion_2"])
    ref = [t.cpu().numpy() for t in (d64, hid64, rgb64, occ64)]
    errs = {}
    for precision in ("bf16x3", "f32"):
        gen, pred = generator(sd, psd, precision)
        out = TG.hip_outputs(gen, pred, i)
        errs[precision] = {k: rel(o.cpu().numpy(), r) for k, o, r in zip(("deformed", "hid", "rgb", "occlusion_2"), out, ref)}
    _assert_fp32_class("generator 1x24x20:", errs["bf16x3"], errs["f32"])


# ---- bit-identity -------------------------------------------------------------------------------------------------------------------------
def test_motion_batch_repeat_and_side_stream_are_bit_identical():
    TM.test_batch_repeat_and_side_stream_are_bit_identical()


def test_generator_batch_repeat_and_side_stream_are_bit_identical():
    TG.test_batch_repeat_and_side_stream_are_bit_identical()


# ---- launch counts -----------------------------------------------------------------------------------------------------------------------
def _count(fn):
    with _lib.counting() as calls:
        fn()
    torch.cuda.synchronize()
    return dict(collections.Counter(name for name, _ in calls))


def _renamed(counts):
    return {{"r3d_torso_conv": "r3d_torso_conv_prec", "r3d_torso_conv3d": "r3d_torso_conv3d_prec"}.get(k, k): v for k, v in counts.items()}


def test_motion_launches_per_forward():
    from test_torso_generator_host import T
    sd = synth.synth_torso_motion(191, 4)
    args = TM.to_dev(synth.synth_torso_motion_inputs(193, 1, 4))
    counts = {}
    for precision in ("f32", "bf16x3"):
        m = MotionFieldEstimator(num_keypoints=4, precision=precision)
        m.load_state_dict(T(sd), strict=True)
        m = m.eval().to(DEV)
        m(*args)                                                       # the fold and the buffers
        counts[precision] = _count(lambda: m(*args))
    print("launches:", counts)
    assert sum(counts["bf16x3"].values()) == TM.LAUNCHES == 26
    assert counts["bf16x3"] == {"r3d_torso_volume_to_cl": 1, "r3d_torso_motion_input": 1, "r3d_torso_conv3d_prec": 13, "r3d_resize_bilinear": 2,
                                "r3d_torso_conv_prec": 7, "r3d_torso_motion_broadcast": 1, "r3d_torso_motion_deform": 1}
    assert counts["bf16x3"] == _renamed(counts["f32"])


def test_generator_launches_per_forward():
    sd, psd = synth.synth_torso_generator(91), synth.synth_torso_predictor(92)
    i = TG.to_dev(synth.synth_torso_inputs(94, 1, 8, 8))
    counts = {}
    for precision in ("f32", "bf16x3"):
        gen, pred = generator(sd, psd, precision)
        TG.hip_outputs(gen, pred, i)
        counts[precision] = _count(lambda: TG.hip_outputs(gen, pred, i))
    print("launches:", counts)
    # get_deformed_feature: 1 warp; forward: 1 warp + 17 convs; the predictor: 3 convs (the channel-last volume is cached)
    assert counts["bf16x3"] == {"r3d_torso_warp": 2, "r3d_torso_conv_prec": 20}
    assert counts["bf16x3"] == _renamed(counts["f32"])


# ---- the patched chain -------------------------------------------------------------------------------------------------------------------
def test_patch_model_routes_the_torso_forward_to_the_bf16x3_modules():
    """test_gpu_torso_motion.test_patch_model_routes_the_torso_forward_to_the_hip_modules with torso_precision='bf16x3'."""
    from real3dportrait_amd import patch_model, Occlusion2Predictor as P2, TorsoGenerator, TorsoMotionFieldEstimator
    sm, sg, sp = 201, 202, 203
    tm = torso_model_with(reference_like_estimator(sm, 4), sg, sp).to(DEV)
    model = patch_model(model_shell(tm).to(DEV), torso_generator=True, torso_motion=True, torso_precision="bf16x3")
    tm = model.superresolution.torso_model
    assert isinstance(tm.motion_field_estimator, TorsoMotionFieldEstimator) and isinstance(tm.deform_based_generator, TorsoGenerator)
    assert isinstance(tm.occlusion_2_predictor, P2)
    assert [m.precision for m in (tm.motion_field_estimator, tm.deform_based_generator, tm.occlusion_2_predictor)] == ["bf16x3"] * 3
    fs, kp_s, kp_d, Rs, Rd, img, wts = TM.to_dev(synth.synth_torso_motion_inputs(204, 1, 4))
    feats = fs[:, :32].contiguous()
    rgb, ret = tm.forward(feats, fs, kp_s, kp_d, img, wts)
    msd, gsd, psd = synth.synth_torso_motion(sm, 4), synth.synth_torso_generator(sg), synth.synth_torso_predictor(sp)
    with torch.no_grad():
        d64, o64, o264 = R64.estimator(msd, fs, kp_s, kp_d, Rs, Rd, img, wts)
        _, rgb64, hid64 = G64.generator(gsd, feats, d64)
        occ64 = G64.occlusion_2(psd, hid64, o264)
    errs = {"rgb": rel(rgb.cpu().numpy(), rgb64.cpu().numpy()), "occlusion_2": rel(ret["occlusion_2"].cpu().numpy(), occ64.cpu().numpy()),
            "occlusion": rel(ret["occlusion"].cpu().numpy(), o64.cpu().numpy())}
    print("patched forward, bf16x3:", errs)
    assert rgb.shape == (1, 3, 256, 256) and ret["occlusion_2"].shape == (1, 1, 256, 256)
    assert all(e <= TOL for e in errs.values()), errs
