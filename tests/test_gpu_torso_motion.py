"""GPU: the HIP motion-field estimator (real3dportrait_amd/torso_motion.py) against the reference's goldens and, on fresh
inputs, the fp64 restatement (tests/torso_motion_ref64.py); determinism across batch, repeats and streams; the patch_model swap on a torso
model whose modules are plain-torch stand-ins with the reference's layout; the number of kernel launches per forward."""
import collections

import pytest
import torch
import torch.nn.functional as F

import torso_motion_ref64 as R64
import torso_ref64 as G64
from test_torso_motion_host import GOLDENS, INPUT_ORDER, golden_case, hip_estimator, reference_like_estimator, rel, subsample, torso_model_with
from test_torso_generator_host import model_shell
from real3dportrait_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2e-4
LAUNCHES = 26          # library launches per forward at B = 1


def to_dev(inp):
    return [torch.from_numpy(inp[k]).to(DEV) for k in INPUT_ORDER]


@pytest.mark.parametrize("name", GOLDENS)
def test_goldens(name):
    g, sd, inp, K = golden_case(name)
    m = hip_estimator(sd, K).to(DEV)
    deformation, occ, occ2 = m(*to_dev(inp))
    N = inp["fs"].shape[0]
    assert deformation.shape == (N, 16, 64, 64, 3) and occ.shape == (N, 1, 64, 64) and occ2.shape == (N, 1, 64, 64)
    assert deformation.is_contiguous() and occ.is_contiguous() and occ2.is_contiguous()
    errs = {k: rel(v.cpu().numpy(), g[k]) for k, v in subsample(g, deformation, occ, occ2).items()}
    print(name, errs)
    assert all(e <= TOL for e in errs.values()), errs


def test_fresh_inputs_against_fp64():
    """N = 3, K = 9, Rs and Rd not the identity; the restatement runs in fp64 on the device."""
    K = 9
    sd = synth.synth_torso_motion(181, K)
    m = hip_estimator(sd, K).to(DEV)
    inp = synth.synth_torso_motion_inputs(183, 3, K, rotate=True)
    assert float(abs(inp["Rs"] - inp["Rd"]).max()) > 0.1
    args = to_dev(inp)
    deformation, occ, occ2 = m(*args)
    with torch.no_grad():
        d64, o64, o264 = R64.estimator(sd, *args)
    errs = {"deformation": rel(deformation.cpu().numpy(), d64.cpu().numpy()), "occlusion": rel(occ.cpu().numpy(), o64.cpu().numpy()),
            "occlusion_2": rel(occ2.cpu().numpy(), o264.cpu().numpy())}
    print("N3 K9:", errs)
    assert all(e <= TOL for e in errs.values()), errs


def test_batch_repeat_and_side_stream_are_bit_identical():
    sd = synth.synth_torso_motion(191, 4)
    m = hip_estimator(sd, 4).to(DEV)
    args = to_dev(synth.synth_torso_motion_inputs(193, 2, 4, rotate=True))
    both = m(*args)
    for n in range(2):
        one = m(*[a[n:n + 1].contiguous() for a in args])
        for a, b in zip(both, one):
            assert torch.equal(a[n:n + 1], b), n
    again = m(*args)
    assert all(torch.equal(a, b) for a, b in zip(both, again))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s_out = m(*args)
    torch.cuda.current_stream().wait_stream(side)
    assert all(torch.equal(a, b) for a, b in zip(both, s_out))


def test_patch_model_routes_the_torso_forward_to_the_hip_modules():
    """patch_model(torso_generator=True, torso_motion=True) on the stand-in torso model: its forward (facev2v_warp/model2.py:248-263)
    returns the rgb and occlusion_2 of the fp64 restatement chain estimator -> generator -> occlusion_2_predictor."""
    from real3dportrait_amd import patch_model, TorsoGenerator, TorsoMotionFieldEstimator
    sm, sg, sp = 201, 202, 203
    tm = torso_model_with(reference_like_estimator(sm, 4), sg, sp).to(DEV)
    model = patch_model(model_shell(tm).to(DEV), torso_generator=True, torso_motion=True)
    tm = model.superresolution.torso_model
    assert isinstance(tm.motion_field_estimator, TorsoMotionFieldEstimator) and isinstance(tm.deform_based_generator, TorsoGenerator)
    inp = synth.synth_torso_motion_inputs(204, 1, 4)
    fs, kp_s, kp_d, Rs, Rd, img, wts = to_dev(inp)
    assert torch.equal(Rs[0].cpu(), torch.eye(3))
    feats = fs[:, :32].contiguous()                                   # the appearance volume the generator warps (model2.py:236,260)
    rgb, ret = tm.forward(feats, fs, kp_s, kp_d, img, wts)
    msd, gsd, psd = synth.synth_torso_motion(sm, 4), synth.synth_torso_generator(sg), synth.synth_torso_predictor(sp)
    with torch.no_grad():
        d64, o64, o264 = R64.estimator(msd, fs, kp_s, kp_d, Rs, Rd, img, wts)
        _, rgb64, hid64 = G64.generator(gsd, feats, d64)
        occ64 = G64.occlusion_2(psd, hid64, o264)
    errs = {"rgb": rel(rgb.cpu().numpy(), rgb64.cpu().numpy()), "occlusion_2": rel(ret["occlusion_2"].cpu().numpy(), occ64.cpu().numpy()),
            "occlusion": rel(ret["occlusion"].cpu().numpy(), o64.cpu().numpy())}
    print("patched forward:", errs)
    assert rgb.shape == (1, 3, 256, 256) and ret["occlusion_2"].shape == (1, 1, 256, 256)
    assert all(e <= TOL for e in errs.values()), errs


def test_launches_per_forward():
    """Every r3d_* call of the module is one kernel launch; one forward at B = 1 makes the number DESIGN 4.10 states."""
    from real3dportrait_amd import _lib
    m = hip_estimator(synth.synth_torso_motion(191, 4), 4).to(DEV)
    args = to_dev(synth.synth_torso_motion_inputs(193, 1, 4))
    m(*args)                                                           # the fold and the buffers
    with _lib.counting() as calls:
        out = m(*args)
    counts = dict(collections.Counter(name for name, _ in calls))
    torch.cuda.synchronize()
    print("launches:", counts)
    assert sum(counts.values()) == LAUNCHES, counts
    assert counts == {"r3d_torso_volume_to_cl": 1, "r3d_torso_motion_input": 1, "r3d_torso_conv3d": 13, "r3d_resize_bilinear": 2, "r3d_torso_conv": 7,
                      "r3d_torso_motion_broadcast": 1, "r3d_torso_motion_deform": 1}
    assert all(torch.equal(a, b) for a, b in zip(out, m(*args)))
