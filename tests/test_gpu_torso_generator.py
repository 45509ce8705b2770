"""GPU: the HIP torso generator (real3dportrait_amd/torso_generator.py) against the reference's goldens and, at sizes beyond
them, the fp64 restatement (tests/torso_ref64.py); determinism across batch, repeats and streams; the patch_model swap on a torso model
whose generator and predictor are plain-torch modules with the reference's layout."""
import pytest
import torch
import torch.nn.functional as F

import torso_ref64 as R64
from test_torso_generator_host import GOLDENS, golden_case, hip_generator, hip_predictor, model_shell, reference_like_torso_model, rel, subsample
from real3dportrait_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2e-4


def to_dev(inp):
    return {k: torch.from_numpy(v).to(DEV) for k, v in inp.items()}


def hip_outputs(gen, pred, i):
    """deformed_fs, hid, rgb as infer_forward_stage2 obtains them, and occlusion_2 by the forward tail (model2.py:260-263)."""
    deformed = gen.get_deformed_feature(i["torso_appearance_feats"], i["deformation"])
    rgb, hid = gen(i["torso_appearance_feats"], i["deformation"], i["occlusion"], return_hid=True)
    occ2 = pred(torch.cat([hid, F.interpolate(i["occlusion_2"], size=tuple(hid.shape[-2:]), mode="bilinear")], dim=1))
    return deformed, hid, rgb, occ2


@pytest.mark.parametrize("name", GOLDENS)
def test_goldens(name):
    g, sd, psd, inp = golden_case(name)
    gen, pred = hip_generator(sd).to(DEV), hip_predictor(psd).to(DEV)
    i = to_dev(inp)
    deformed, hid, rgb, occ2 = hip_outputs(gen, pred, i)
    N, H, W = inp["deformation"].shape[0], inp["deformation"].shape[2], inp["deformation"].shape[3]
    assert deformed.shape == (N, 512, H, W) and hid.shape == (N, 64, 4 * H, 4 * W) and rgb.shape == (N, 3, 4 * H, 4 * W)
    assert occ2.shape == (N, 1, 4 * H, 4 * W)
    errs = {k: rel(v.cpu().numpy(), g[k]) for k, v in subsample(g, deformed, hid, rgb, occ2).items()}
    # the decoder alone, from the reference's layout of the deformed features (forward_with_deformed_feature reads NCHW)
    rgb2, hid2 = gen.forward_with_deformed_feature(deformed, i["occlusion"], return_hid=True)
    s = subsample(g, deformed, hid2, rgb2, occ2)
    errs["hid_from_deformed"], errs["rgb_from_deformed"] = rel(s["hid"].cpu().numpy(), g["hid"]), rel(s["rgb"].cpu().numpy(), g["rgb"])
    assert torch.equal(gen(i["torso_appearance_feats"], i["deformation"], i["occlusion"]), rgb)          # return_hid=False: rgb alone
    print(name, errs)
    assert all(e <= TOL for e in errs.values()), errs


@pytest.mark.parametrize("N,H,W", [(1, 8, 8), (1, 64, 40), (3, 16, 12)])
def test_sizes_beyond_the_goldens_against_fp64(N, H, W):
    sd, psd = synth.synth_torso_generator(81), synth.synth_torso_predictor(82)
    gen, pred = hip_generator(sd).to(DEV), hip_predictor(psd).to(DEV)
    i = to_dev(synth.synth_torso_inputs(83, N, H, W))
    deformed, hid, rgb, occ2 = hip_outputs(gen, pred, i)
    d64, rgb64, hid64 = R64.generator(sd, i["torso_appearance_feats"], i["deformation"])
    occ64 = R64.occlusion_2(psd, hid64, i["occlusion_2"])
    errs = {"deformed": rel(deformed.cpu().numpy(), d64.cpu().numpy()), "hid": rel(hid.cpu().numpy(), hid64.cpu().numpy()),
            "rgb": rel(rgb.cpu().numpy(), rgb64.cpu().numpy()), "occlusion_2": rel(occ2.cpu().numpy(), occ64.cpu().numpy())}
    print("%dx%dx%d:" % (N, H, W), errs)
    assert all(e <= TOL for e in errs.values()), errs


def test_batch_repeat_and_side_stream_are_bit_identical():
    sd, psd = synth.synth_torso_generator(91), synth.synth_torso_predictor(92)
    gen, pred = hip_generator(sd).to(DEV), hip_predictor(psd).to(DEV)
    i = to_dev(synth.synth_torso_inputs(93, 2, 24, 20))
    both = hip_outputs(gen, pred, i)
    for n in range(2):
        one = hip_outputs(gen, pred, {k: v[n:n + 1].contiguous() for k, v in i.items()})
        for a, b in zip(both, one):
            assert torch.equal(a[n:n + 1], b), n
    again = hip_outputs(gen, pred, i)
    assert all(torch.equal(a, b) for a, b in zip(both, again))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s_out = hip_outputs(gen, pred, i)
    torch.cuda.current_stream().wait_stream(side)
    assert all(torch.equal(a, b) for a, b in zip(both, s_out))


def test_an_edited_volume_is_warped_anew():
    """The channel-last copy of the appearance volume is cached on the tensor's identity and version."""
    gen = hip_generator(synth.synth_torso_generator(91)).to(DEV)
    i = to_dev(synth.synth_torso_inputs(94, 1, 8, 8))
    fs = i["torso_appearance_feats"]
    a = gen.get_deformed_feature(fs, i["deformation"])
    fs.mul_(2.0)
    b = gen.get_deformed_feature(fs, i["deformation"])
    assert torch.equal(b, gen.get_deformed_feature(fs.clone(), i["deformation"])) and not torch.equal(a, b)
    torch.testing.assert_close(b, 2.0 * a, rtol=1e-6, atol=0)


def test_patch_model_routes_stage2_and_the_forward_tail_to_the_hip_modules():
    from real3dportrait_amd import patch_model, TorsoGenerator, Occlusion2Predictor
    g, sd, psd, inp = golden_case("torso_a_r64")
    sg, sp = (int(v) for v in g["spec"][:2])
    tm = reference_like_torso_model(sg, sp).to(DEV)
    model = patch_model(model_shell(tm).to(DEV), torso_generator=True)
    tm = model.superresolution.torso_model
    assert isinstance(tm.deform_based_generator, TorsoGenerator) and isinstance(tm.occlusion_2_predictor, Occlusion2Predictor)
    i = to_dev(inp)
    ret = {k: i[k] for k in ("torso_appearance_feats", "deformation", "occlusion")}
    rgb = tm.infer_forward_stage2(ret)                                                       # facev2v_warp/model2.py:329-336
    hid = ret["deformed_torso_hid"]
    occ2 = tm.occlusion_2_predictor(torch.cat([hid, F.interpolate(i["occlusion_2"], size=(256, 256), mode="bilinear")], dim=1))   # :262
    assert hid.is_contiguous() and hid.shape == (1, 64, 256, 256)
    deformed = tm.deform_based_generator.get_deformed_feature(i["torso_appearance_feats"], i["deformation"])
    errs = {k: rel(v.cpu().numpy(), g[k]) for k, v in subsample(g, deformed, hid, rgb, occ2).items()}
    print("patched:", errs)
    assert all(e <= TOL for e in errs.values()), errs
