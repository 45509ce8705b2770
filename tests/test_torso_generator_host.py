"""CPU: the torso generator's host side (real3dportrait_amd/torso_generator.py, r3d_torso_* of include/r3d_hip.h).

The state_dict layout against the reference's key list, the fp64 fold (spectral norm, BatchNorm) against the fp64 restatement
(tests/torso_ref64.py), the restatement against the reference's goldens, parameter-version tracking, argument validation of the C entry
points (which runs before any HIP call), the patch_model swap and the kernels' scratch use."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import load_golden
import torso_ref64 as R64
from real3dportrait_amd import synth

GOLDENS = ["torso_a_r64", "torso_b_n2_r24x20", "torso_c_r32x48"]


def T(sd):
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}


def rel(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return float(np.abs(a - ref).max() / np.abs(ref).max())


def golden_case(name):
    """(golden, generator state_dict, predictor state_dict, inputs) -- parameters and inputs regenerated from the stored seeds."""
    g = load_golden(name)
    sg, sp, sx, N, H, W = (int(v) for v in g["spec"])
    return g, synth.synth_torso_generator(sg), synth.synth_torso_predictor(sp), synth.synth_torso_inputs(sx, N, H, W)


def subsample(g, deformed, hid, rgb, occ2):
    """The golden's strides applied to full outputs (tests/golden/make_golden_torso.py)."""
    sc, sd, sh, sr, so = (int(v) for v in g["strides"])
    return {"deformed": deformed[:, ::sc, ::sd, ::sd], "hid": hid[:, :, ::sh, ::sh], "rgb": rgb[:, :, ::sr, ::sr],
            "occlusion_2": occ2[:, :, ::so, ::so]}


def hip_generator(sd):
    from real3dportrait_amd.torso_generator import Generator
    m = Generator()
    m.load_state_dict(T(sd), strict=True)
    return m.eval()


def hip_predictor(psd):
    from real3dportrait_amd.torso_generator import Occlusion2Predictor
    m = Occlusion2Predictor()
    m.load_state_dict(T(psd), strict=True)
    return m.eval()


def run_folded(L, x):
    """The folded layer list of fold_generator as r3d_torso_conv evaluates it, in torch on x [N, 512, H, W]: prologue, then the zero
    padding, nearest x2, conv, bias, activation, residual.  Returns (rgb, hid)."""
    res_in = None
    for i, l in enumerate(L):
        a = x
        if l["ps"] is not None:
            a = F.leaky_relu(a * l["ps"][None, :, None, None] + l["pt"][None, :, None, None], 0.0)
        if l["up"]:
            a = F.interpolate(a, scale_factor=2, mode="nearest")
        y = F.conv2d(a, l["w"].permute(0, 3, 1, 2), l["b"], padding=l["k"] // 2)
        if l["act"] == 1:
            y = F.leaky_relu(y, l["slope"])
        if l["ps"] is not None:
            res_in = x                    # the first conv of a residual block: its input is the block's
        if l["res"]:
            y = y + res_in
        if i == len(L) - 1:
            return y, x
        x = y


def test_state_dict_keys_are_the_reference_s():
    keys = load_golden("torso_keys")
    gen, pred = hip_generator(synth.synth_torso_generator(1)), hip_predictor(synth.synth_torso_predictor(2))
    assert list(gen.state_dict().keys()) == [str(k) for k in keys["generator"]] and len(gen.state_dict()) == 139
    assert list(pred.state_dict().keys()) == [str(k) for k in keys["predictor"]]
    shapes = dict(synth.torso_generator_shapes())
    assert sorted(shapes) == sorted(str(k) for k in keys["generator"])
    for k, v in gen.state_dict().items():
        assert tuple(v.shape) == tuple(shapes[k]), k


def test_load_state_dict_is_strict():
    from real3dportrait_amd.torso_generator import Generator, Occlusion2Predictor
    sd = T(synth.synth_torso_generator(1))
    for missing in ("res.3.layers.1.layers.2.weight_u", "up.1.layers.1.layers.1.running_var", "mid_conv.bias"):
        part = {k: v for k, v in sd.items() if k != missing}
        with pytest.raises(RuntimeError, match="Missing key"):
            Generator().load_state_dict(part, strict=True)
    with pytest.raises(RuntimeError, match="Unexpected key"):
        Generator().load_state_dict(dict(sd, extra=torch.zeros(1)), strict=True)
    psd = T(synth.synth_torso_predictor(2))
    del psd["2.bias"]
    with pytest.raises(RuntimeError, match="Missing key"):
        Occlusion2Predictor().load_state_dict(psd, strict=True)


def test_unsupported_scales_raise():
    from real3dportrait_amd.torso_generator import Generator
    for kw in ({"model_scale": "large"}, {"more_res": True}):
        with pytest.raises(NotImplementedError, match="network2.py"):
            Generator(**kw)
    assert len(Generator(model_scale="small").state_dict()) == 139


def test_fp64_fold_equals_the_fp64_restatement():
    """Spectral norm, the BatchNorm of a CNA block folded into weight and bias, the BatchNorm + ReLU of a NAC block as the prologue
    (first conv) or folded into the previous conv's rows and epilogue (second conv)."""
    from real3dportrait_amd.torso_generator import fold_generator
    torch.set_num_threads(8)
    sd = synth.synth_torso_generator(5)
    gen = hip_generator(sd)
    inp = synth.synth_torso_inputs(6, 2, 24, 20)
    d, rgb, hid = R64.generator(sd, torch.from_numpy(inp["torso_appearance_feats"]), torch.from_numpy(inp["deformation"]))
    L = fold_generator(gen, torch.float64)
    assert len(L) == 17 and all(l["w"].dtype == torch.float64 for l in L)
    frgb, fhid = run_folded(L, d)
    e_rgb, e_hid = rel(frgb.numpy(), rgb.numpy()), rel(fhid.numpy(), hid.numpy())
    print("fold vs restatement: rgb %.2e hid %.2e" % (e_rgb, e_hid))
    assert e_rgb <= 1e-12 and e_hid <= 1e-12


def test_warp_restatement_equals_grid_sample():
    inp = synth.synth_torso_inputs(7, 2, 24, 20)
    fs, grid = torch.from_numpy(inp["torso_appearance_feats"]).double(), torch.from_numpy(inp["deformation"]).double()
    ref = F.grid_sample(fs, grid, align_corners=True, padding_mode="border")
    assert float((R64.warp(fs, grid) - ref).abs().max()) <= 1e-14 * float(ref.abs().max())


@pytest.mark.parametrize("name", GOLDENS)
def test_fp64_restatement_matches_reference_goldens(name):
    torch.set_num_threads(8)
    g, sd, psd, inp = golden_case(name)
    d, rgb, hid = R64.generator(sd, torch.from_numpy(inp["torso_appearance_feats"]), torch.from_numpy(inp["deformation"]))
    occ2 = R64.occlusion_2(psd, hid, torch.from_numpy(inp["occlusion_2"]))
    errs = {k: rel(v.numpy(), g[k]) for k, v in subsample(g, d, hid, rgb, occ2).items()}
    print(name, errs)
    assert all(e <= 1e-4 for e in errs.values()), errs


def test_in_place_parameter_edits_are_seen_by_the_next_prepare():
    gen = hip_generator(synth.synth_torso_generator(5))
    a = gen._prepare()
    assert gen._prepare() is a
    w0 = a[2]["w"].clone()
    with torch.no_grad():
        gen.res[0].layers[0].layers[2].weight_orig.mul_(1.0).add_(0.01)
    b = gen._prepare()
    assert b is not a and not torch.equal(b[2]["w"], w0)
    ps0 = b[4]["ps"].clone()
    with torch.no_grad():
        gen.res[1].layers[0].layers[0].running_var.mul_(2.0)
    c = gen._prepare()
    assert c is not b and not torch.equal(c[4]["ps"], ps0) and torch.equal(c[2]["w"], b[2]["w"])
    pred = hip_predictor(synth.synth_torso_predictor(2))
    p0 = pred._prepare()
    with torch.no_grad():
        getattr(pred, "2").weight.add_(0.5)
    assert pred._prepare() is not p0
    # a parameter replaced by another tensor at the same address and version (what the caching allocator makes of a freed one)
    from test_state_host import replaced_at_same_address
    d, e = replaced_at_same_address(gen.mid_conv, "weight", gen._prepare)
    assert e is not d and torch.equal(e[1]["w"], d[1]["w"] * 3.0) and torch.equal(e[2]["w"], d[2]["w"])
    assert gen._prepare() is e


def test_c_entry_points_reject_bad_arguments_without_a_gpu():
    from real3dportrait_amd import _lib
    lib = _lib.load()
    assert lib.r3d_version() == _lib.ABI_VERSION
    at = lambda i: ctypes.c_void_p((1 << 30) + 4 * i)       # never dereferenced: validation fails first
    far = ctypes.c_void_p(1 << 40)
    err = lambda: lib.r3d_last_error()
    assert lib.r3d_torso_volume_to_cl(None, 1, 32, 16, 8, 8, far, None) == -1 and b"NULL" in err()
    assert lib.r3d_torso_volume_to_cl(at(0), 1, 32, 0, 8, 8, far, None) == -1 and b"bad argument" in err()
    assert lib.r3d_torso_volume_to_cl(at(0), 1, 32, 16, 8, 8, at(100), None) == -1 and b"overlap" in err()
    assert lib.r3d_torso_warp(at(0), 1, 32, 16, 8, 8, None, 16, 8, 8, far, 1, None) == -1 and b"NULL" in err()
    assert lib.r3d_torso_warp(at(0), 1, 32, 16, 8, 8, far, 16, -8, 8, far, 1, None) == -1 and b"bad argument" in err()
    assert lib.r3d_torso_warp(at(0), 1, 32, 16, 8, 8, far, 16, 8, 8, at(32767), 1, None) == -1 and b"overlap" in err()
    conv = lambda x, Cin, up, ps, pt, w, Cout, k, act, res, y, yn, nchw=0, B=1, H=8, W=8: lib.r3d_torso_conv(
        x, B, H, W, Cin, nchw, up, ps, pt, 0.0, w, None, Cout, k, act, 0.0, res, y, yn, None)
    assert conv(None, 32, 0, None, None, far, 64, 3, 0, None, far, None) == -1 and b"NULL" in err()
    assert conv(at(0), 32, 0, None, None, far, 64, 3, 0, None, None, None) == -1 and b"NULL" in err()        # no output at all
    assert conv(at(0), 32, 0, far, None, far, 64, 3, 0, None, far, None) == -1 and b"NULL" in err()           # scale without shift
    assert conv(at(0), 32, 0, None, None, far, 64, 5, 0, None, far, None) == -1 and b"ksize 5" in err()
    assert conv(at(0), 32, 2, None, None, far, 64, 3, 0, None, far, None) == -1 and b"upsample 2" in err()
    assert conv(at(0), 32, 0, None, None, far, 64, 3, 3, None, far, None) == -1 and b"act 3" in err()
    assert conv(at(0), 0, 0, None, None, far, 64, 3, 0, None, far, None) == -1 and b"bad argument" in err()
    assert conv(at(0), 32, 0, None, None, far, 5000, 3, 0, None, far, None) == -1 and b"bad argument" in err()
    assert conv(at(0), 32, 0, None, None, far, 64, 3, 0, None, far, None, H=0) == -1 and b"bad argument" in err()
    # x [1, 8, 8, 32] = 2048 floats; y [1, 8, 8, 64] = 4096 (16384 with upsample)
    assert conv(at(0), 32, 0, None, None, far, 64, 3, 0, None, at(2047), None) == -1 and b"overlaps x" in err()
    assert conv(at(4095), 32, 0, None, None, far, 64, 3, 0, None, None, at(0)) == -1 and b"overlaps x" in err()
    assert conv(at(16383), 32, 1, None, None, far, 64, 3, 0, None, at(0), None) == -1 and b"overlaps x" in err()
    assert conv(at(100000), 32, 0, None, None, far, 64, 3, 0, at(10), at(0), None) == -1 and b"residual" in err()   # partial overlap
    assert conv(at(100000), 32, 0, None, None, far, 64, 3, 0, None, at(0), at(4095)) == -1 and b"y and y_nchw" in err()


def reference_like_torso_model(seed=5, seed_p=6, n_res=6):
    """A stand-in for WarpBasedTorsoModelMediaPipe's second half in plain torch, with the reference's class names, attributes and
    state_dict keys, built by the reference's layer recipe (layers.py: torch.nn.utils.spectral_norm on the convs of the blocks,
    BatchNorm2d for SyncBatchNorm, which evaluates the same in eval mode)."""
    from torch.nn.utils import spectral_norm

    class ConvBlock2D(nn.Module):
        def __init__(self, pattern, ci, co, leaky=False):
            super().__init__()
            mods = {"C": spectral_norm(nn.Conv2d(ci, co, 3, 1, 1)), "N": nn.BatchNorm2d(co if pattern[0] == "C" else ci),
                    "A": nn.LeakyReLU(0.2, inplace=True) if leaky else nn.ReLU(inplace=True)}
            self.layers = nn.Sequential(*[mods[c] for c in pattern])

        def forward(self, x):
            return self.layers(x)

    class ResBlock2D(nn.Module):
        def __init__(self):
            super().__init__()
            self.layers = nn.Sequential(ConvBlock2D("NAC", 256, 256), ConvBlock2D("NAC", 256, 256))

        def forward(self, x):
            return x + self.layers(x)

    class UpBlock2D(nn.Module):
        def __init__(self, ci, co):
            super().__init__()
            self.layers = nn.Sequential(nn.Upsample(scale_factor=(2, 2)), ConvBlock2D("CNA", ci, co))

        def forward(self, x):
            return self.layers(x)

    class Generator(nn.Module):
        def __init__(self):
            super().__init__()
            self.in_conv = ConvBlock2D("CNA", 512, 256, leaky=True)
            self.mid_conv = nn.Conv2d(256, 256, 1, 1, 0)
            self.res = nn.Sequential(*[ResBlock2D() for _ in range(n_res)])
            self.up = nn.Sequential(UpBlock2D(256, 128), UpBlock2D(128, 64))
            self.out_conv = nn.Conv2d(64, 3, 7, 1, 3)

        def forward(self, fs, deformation, occlusion, return_hid=False):
            N, _, D, H, W = fs.shape
            x = F.grid_sample(fs, deformation, align_corners=True, padding_mode="border").view(N, -1, H, W)
            x = self.up(self.res(self.mid_conv(self.in_conv(x))))
            rgb = self.out_conv(x)
            return (rgb, x) if return_hid else rgb

    class TorsoModel(nn.Module):
        def __init__(self):
            super().__init__()
            self.deform_based_generator = Generator()
            self.occlusion_2_predictor = nn.Sequential(nn.Conv2d(65, 32, 3, 1, 1), nn.ReLU(), nn.Conv2d(32, 32, 3, 1, 1), nn.ReLU(),
                                                       nn.Conv2d(32, 1, 3, 1, 1), nn.Sigmoid())

        @torch.no_grad()
        def infer_forward_stage2(self, ret):            # the reference's call (facev2v_warp/model2.py:329-336)
            img, hid = self.deform_based_generator(ret["torso_appearance_feats"], ret["deformation"], ret["occlusion"], return_hid=True)
            ret["deformed_torso_hid"] = hid
            return img

    tm = TorsoModel().eval()
    if n_res == 6:
        tm.deform_based_generator.load_state_dict(T(synth.synth_torso_generator(seed)), strict=True)
    tm.occlusion_2_predictor.load_state_dict(T(synth.synth_torso_predictor(seed_p)), strict=True)
    return tm


def model_shell(torso_model):
    """The smallest model patch_model accepts whose superresolution carries a torso model."""
    class SR(nn.Module):
        def __init__(self):
            super().__init__()
            self.block0 = nn.Linear(1, 1)
            self.torso_model = torso_model

    class Model(nn.Module):
        def __init__(self):
            super().__init__()
            self.renderer = nn.Module()
            self.superresolution = SR()

    return Model()


def test_the_plain_torch_stand_in_meets_the_golden():
    """The torso model the patch_model tests swap (here and on the GPU) computes what the reference computed."""
    torch.set_num_threads(8)
    g, sd, psd, inp = golden_case("torso_b_n2_r24x20")
    sg, sp = (int(v) for v in g["spec"][:2])
    tm = reference_like_torso_model(sg, sp)
    ret = {k: torch.from_numpy(inp[k]) for k in ("torso_appearance_feats", "deformation", "occlusion")}
    rgb = tm.infer_forward_stage2(ret)
    hid = ret["deformed_torso_hid"]
    with torch.no_grad():
        occ2 = tm.occlusion_2_predictor(torch.cat([hid, F.interpolate(torch.from_numpy(inp["occlusion_2"]), size=tuple(hid.shape[-2:]),
                                                                        mode="bilinear")], dim=1))
    s = subsample(g, hid, hid, rgb, occ2)
    errs = {k: rel(s[k].numpy(), g[k]) for k in ("hid", "rgb", "occlusion_2")}
    assert all(e <= 1e-4 for e in errs.values()), errs


def test_patch_model_leaves_the_torso_model_alone_without_the_flag():
    from real3dportrait_amd import patch_model
    tm = reference_like_torso_model()
    gen, pred = tm.deform_based_generator, tm.occlusion_2_predictor
    patch_model(model_shell(tm))
    assert tm.deform_based_generator is gen and tm.occlusion_2_predictor is pred
    patch_model(model_shell(tm), torso_generator=False)
    assert tm.deform_based_generator is gen and tm.occlusion_2_predictor is pred


def test_patch_model_swaps_generator_and_predictor_with_identical_keys():
    from real3dportrait_amd import patch_model, TorsoGenerator, Occlusion2Predictor
    tm = reference_like_torso_model()
    before = {k: v.clone() for k, v in tm.state_dict().items()}
    patch_model(model_shell(tm), torso_generator=True)
    assert isinstance(tm.deform_based_generator, TorsoGenerator) and isinstance(tm.occlusion_2_predictor, Occlusion2Predictor)
    after = tm.state_dict()
    assert list(after) == list(before)
    for k, v in before.items():
        assert after[k].dtype == v.dtype and torch.equal(after[k], v), k


def test_patch_model_leaves_other_generators():
    from real3dportrait_amd import patch_model
    tm = reference_like_torso_model(n_res=12)          # the 'large' scale's residual depth
    gen, pred = tm.deform_based_generator, tm.occlusion_2_predictor
    patch_model(model_shell(tm), torso_generator=True)
    assert tm.deform_based_generator is gen and tm.occlusion_2_predictor is pred


def test_torso_kernels_do_not_use_scratch():
    from test_render_kernel_resources import _kernel_metadata
    from real3dportrait_amd import _lib
    meta = _kernel_metadata(_lib.LIB_PATH)
    names = [k for k in meta if "5torso" in k]
    assert len(names) == 10, names          # torso_volume_to_cl, torso_warp, torso_conv x (4 tiles x 2 loaders)
    for k in names:
        assert int(meta[k]["private_segment_fixed_size"]) == 0, (k, meta[k])
        assert int(meta[k]["vgpr_spill_count"]) == 0, (k, meta[k])
