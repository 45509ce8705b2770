"""CPU: DeepLabV3's host side (real3dportrait_amd/deeplabv3.py, include/r3d_hip_deeplab.h): the fp64 restatement against the
reference's goldens and the conditions their maker stored, state_dict keys, the BatchNorm fold, the pooled branch as a bias, the header
against its binding table, the argument checks of every r3d_dl_* entry point, and patch_model(cano_low_reso_encoder=True) on mocks."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import deeplabv3_common as common
import deeplabv3_ref64 as R64
from abi import C_RETURNS, entry_matches, header_declarations, refusals
from conftest import ROOT, load_golden
from real3dportrait_amd import synth

HEADER = "r3d_hip_deeplab.h"
LLVM = "/opt/rocm/lib/llvm/bin"


@pytest.mark.parametrize("name", list(common.CASES))
def test_fp64_restatement_meets_the_reference(name):
    torch.set_num_threads(8)
    g = load_golden(name)
    S, B, cin, enc, seed_w, seed_x = common.CASES[name]
    enc, cin, sd, x = common.case_inputs(name)
    assert [int(v) for v in g["spec"]] == [seed_w, seed_x, B, cin, S, S] and str(g["encoder"]) == enc
    stats = []
    out, taps = R64.forward(sd, torch.from_numpy(x), torch.float64, enc, stats)
    assert tuple(out.shape) == (B, 256, S // 8, S // 8)
    errs = {"out": common.rel(common.sub(out.numpy(), common.OUT_BUDGET), g["out"])}
    errs.update({k: common.rel(common.sub(taps[k].numpy()), g[k]) for k in common.TAPS})
    print(name, errs)
    assert all(e <= common.TOL for e in errs.values()), errs
    # the conditions on the inputs the maker stored: no ReLU is dead or the identity, no stage's magnitude ran away
    assert [n for n, _ in stats] == [str(n) for n in g["relu_names"]] and len(stats) == 1 + 2 * 16 + 6
    for (n, share), stored in zip(stats, g["relu"]):
        assert abs(share - stored) < 1e-3 and 0.10 < stored < 0.95, (n, share, stored)
    tap_max = [float(taps[k].abs().max()) for k in common.TAPS] + [float(out.abs().max())]
    for k, v, stored in zip(common.TAPS + ("out",), tap_max, g["tap_max"]):
        assert abs(v - stored) <= 1e-5 * stored and 1.0 < stored < 100.0, (k, v, stored)


def test_state_dict_keys_are_the_references():
    from real3dportrait_amd.deeplabv3 import DeepLabV3
    stored = load_golden("deeplabv3_keys")
    assert set(stored) == {p + s for p in ("resnet34.c5", "resnet34.c6", "resnet18.c5") for s in ("", ".shapes")}
    for tag in ("resnet34.c5", "resnet34.c6", "resnet18.c5"):
        enc, cin = tag.split(".c")[0], int(tag.split(".c")[1])
        m = DeepLabV3(enc, in_channels=cin)
        sd = m.state_dict()
        assert list(sd) == [str(k) for k in stored[tag]], tag          # the reference's order too
        shapes = {str(k): tuple(int(v) for v in row[:np.count_nonzero(row)]) for k, row in zip(stored[tag], stored[tag + ".shapes"])}
        assert {k: tuple(v.shape) for k, v in sd.items()} == shapes == dict(synth.deeplabv3_shapes(cin, enc)), tag
        assert sum(k.endswith("num_batches_tracked") for k in sd) == (36 if enc == "resnet34" else 20)
        w = {k: torch.from_numpy(v) for k, v in synth.synth_deeplabv3(3, cin, enc).items()}
        m.load_state_dict(w, strict=True)
        assert all(torch.equal(m.state_dict()[k], v) for k, v in w.items())
        with pytest.raises(RuntimeError):
            m.load_state_dict({k: v for k, v in w.items() if k != "encoder.layer3.0.downsample.1.running_var"}, strict=True)


def test_constructor_rules():
    from real3dportrait_amd import DeepLabV3
    for name in ("resnet50", "resnext50_32x4d", "mobilenet_v2"):
        with pytest.raises(NotImplementedError, match=name):
            DeepLabV3(name)
    with pytest.raises(ValueError, match="fetches no weights"):
        DeepLabV3("resnet34", encoder_weights="imagenet")
    m = DeepLabV3()
    assert m.encoder_name == "resnet34" and m.in_channels == 5 and m.out_channels == 256
    with pytest.raises(ValueError, match="not on a GPU"):
        m(torch.zeros(1, 5, 64, 64))
    with pytest.raises(RuntimeError, match=r"Wrong input shape height=60, width=64.*\(64, 64\)"):
        m(torch.zeros(1, 5, 60, 64))
    with pytest.raises(ValueError, match="5 channels"):
        m(torch.zeros(1, 3, 64, 64))


def test_geometry_is_the_references():
    """Every conv of layer3 / layer4 -- each stage's first conv and its 1 x 1 downsample included -- is stride 1 with dilation 2 / 4 and
    padding (k // 2) dilation (encoders/_utils.py:40-47); the mock is strided at construction and patched the same way."""
    from real3dportrait_amd.deeplabv3 import DeepLabV3, conv_geometry
    m, mock = DeepLabV3(), common.DeepLabV3(5)
    geo = lambda mod: {k: conv_geometry(v) for k, v in mod.named_modules() if isinstance(v, nn.Conv2d)}
    assert geo(m) == geo(mock) and len(geo(m)) == 1 + 2 * 16 + 3 + 7 and None not in geo(m).values()
    g = geo(m)
    assert g["encoder.conv1"] == (5, 64, 7, 2, 3, 1) and g["encoder.layer2.0.conv1"] == (64, 128, 3, 2, 1, 1)
    assert g["encoder.layer2.0.downsample.0"] == (64, 128, 1, 2, 0, 1)
    assert g["encoder.layer3.0.conv1"] == (128, 256, 3, 1, 2, 2) and g["encoder.layer3.0.downsample.0"] == (128, 256, 1, 1, 0, 2)
    assert g["encoder.layer3.5.conv2"] == (256, 256, 3, 1, 2, 2)
    assert g["encoder.layer4.0.conv1"] == (256, 512, 3, 1, 4, 4) and g["encoder.layer4.0.downsample.0"] == (256, 512, 1, 1, 0, 4)
    assert g["decoder.0.convs.3.0"] == (512, 256, 3, 1, 36, 36) and g["decoder.1"] == (256, 256, 3, 1, 1, 1)


def test_batchnorm_fold_is_eval_batchnorm():
    from real3dportrait_amd.deeplabv3 import fold_batchnorm
    torch.manual_seed(0)
    conv, bn = nn.Conv2d(6, 10, 3, 1, 2, 2, bias=False), nn.BatchNorm2d(10)
    with torch.no_grad():
        bn.weight.copy_(1 + 0.1 * torch.randn(10)); bn.bias.copy_(0.1 * torch.randn(10))
        bn.running_mean.copy_(0.1 * torch.randn(10)); bn.running_var.copy_(1 + 0.2 * torch.rand(10))
    w, b = fold_batchnorm(conv.weight, bn)
    assert w.dtype == b.dtype == torch.float32 and w.shape == conv.weight.shape and b.shape == (10,)
    x = torch.randn(2, 6, 9, 7, dtype=torch.float64)
    with torch.no_grad():
        want = bn.double().eval()(conv.double()(x))
        got = F.conv2d(x, w.double(), b.double(), 1, 2, 2)
        # the folded pair is the fp64 fold rounded to fp32 once: each weight and bias is off by at most 2^-24 of itself, so an output by at
        # most 2^-24 (sum |w| |x| + |b|)
        bound = 2.0 ** -24 * F.conv2d(x.abs(), w.double().abs(), b.double().abs(), 1, 2, 2)
    assert bool(((got - want).abs() <= bound * (1 + 1e-9)).all()) and float((got - want).abs().max()) > 0


def test_pooled_branch_is_a_per_sample_bias():
    """ASPPPooling's bilinear up-sampling of a 1 x 1 map (align_corners=False) is a constant, so its 256 channels enter `project` as
    W_proj[:, 1024:1280] . pooled, a bias per sample: against the literal cat + project in fp64."""
    torch.manual_seed(1)
    B, C, h, w = 2, 256, 5, 7
    x = torch.randn(B, 512, h, w, dtype=torch.float64)
    four = torch.randn(B, 4 * C, h, w, dtype=torch.float64)
    w4, wp = torch.randn(C, 512, 1, 1, dtype=torch.float64) / 512 ** 0.5, torch.randn(C, 5 * C, 1, 1, dtype=torch.float64) / (5 * C) ** 0.5
    pooled = F.relu(F.conv2d(F.adaptive_avg_pool2d(x, 1), w4))
    up = F.interpolate(pooled, size=(h, w), mode="bilinear", align_corners=False)
    # torch forms each output as w0 v + w1 v with w0 + w1 == 1 from one source pixel: the constant to within an ulp
    assert float((up - pooled).abs().max()) <= 2.0 ** -52 * float(pooled.max()) and float(pooled.max()) > 0
    want = F.relu(F.conv2d(torch.cat([four, up], dim=1), wp))
    bias = F.conv2d(pooled, wp[:, 4 * C:])          # [B, C, 1, 1]
    got = F.relu(F.conv2d(four, wp[:, :4 * C]) + bias)
    assert float((got - want).abs().max()) <= 1e-13 * float(want.abs().max())


def test_header_mirrors_its_table():
    from real3dportrait_amd import _lib
    lib = _lib.load()
    decls = header_declarations(HEADER)
    table = _lib.FEATURE_SIGNATURES[HEADER]
    assert set(decls) == set(table) == {"r3d_dl_conv", "r3d_dl_maxpool", "r3d_dl_global_mean", "r3d_dl_assemble_input"}
    assert set(_lib.FEATURE_SIGNATURES) == {"r3d_hip_hubert.h", HEADER} and len(_lib.EXTENSION_SIGNATURES) == 1
    others = set(_lib.SIGNATURES) | set(_lib.OPTIONAL_SIGNATURES) | {n for t in _lib.EXTENSION_SIGNATURES.values() for n in t} \
        | set(_lib.FEATURE_SIGNATURES["r3d_hip_hubert.h"])
    assert not set(table) & others
    src = open(os.path.join(ROOT, "include", HEADER)).read()
    assert '#include "r3d_hip.h"' in src
    for h in ("r3d_hip.h", "r3d_hip_img2plane.h", "r3d_hip_hubert.h"):
        assert HEADER not in open(os.path.join(ROOT, "include", h)).read() and "r3d_dl_" not in open(os.path.join(ROOT, "include", h)).read()
    for name, (ret, types) in decls.items():
        res, entries = table[name]
        assert res is C_RETURNS[ret] and res is ctypes.c_int, name
        assert len(entries) == len(types), (name, len(entries), len(types))
        for i, (e, t) in enumerate(zip(entries, types)):
            assert entry_matches(e, t, _lib), "%s: parameter %d is %s in the header, %r in the table" % (name, i, t, e)
        assert [isinstance(e, _lib.Stream) for e in entries] == [False] * (len(entries) - 1) + [True], name
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == [getattr(e, "ctype", e) for e in entries], name
        assert name in _lib._plans
    assert lib.r3d_version() == _lib.ABI_VERSION == 80


@pytest.mark.parametrize("lang", ["c99", "c++17"])
def test_header_stands_alone(lang, tmp_path):
    clang = os.path.join(LLVM, "clang")
    if not os.path.exists(clang):
        pytest.skip("no %s: the header is not compiled here" % clang)
    flags = ["-x", "c", "-std=c99"] if lang == "c99" else ["-x", "c++", "-std=c++17"]
    for i, unit in enumerate(([HEADER], [HEADER, "r3d_hip.h"], ["r3d_hip.h", HEADER], ["r3d_hip_img2plane.h", "r3d_hip_hubert.h", HEADER])):
        src = tmp_path / ("unit%d.%s" % (i, "c" if lang == "c99" else "cpp"))
        src.write_text("".join('#include "%s"\n' % h for h in unit))
        r = subprocess.run([clang] + flags + ["-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                           capture_output=True, text=True)
        assert r.returncode == 0, "%s as %s:\n%s" % (" + ".join(unit), lang, r.stderr)


def test_entry_points_refuse_bad_arguments():
    """Every refusal of the four r3d_dl_* entry points: R3D_ERR_INVALID_ARG and a tagged message before any launch (the checks run before
    any HIP call and the addresses are never dereferenced, so they run without a GPU)."""
    from real3dportrait_amd import _lib
    refused = refusals(_lib.load(), "r3d_dl_")
    X, Y, W, Bi, R = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000
    cv = dict(x=X, B=2, Hin=13, Win=10, Cin=16, w=W, bias=Bi, bias_bstride=0, Cout=40, ksize=3, stride=1, dilation=2, pad=2, residual=R, act=1,
              y=Y, ycs=40, yco=0)
    for p in ("x", "w", "y"):
        refused("conv", cv, b"NULL pointer", **{p: None})
    for p in ("B", "Hin", "Win", "Cin", "Cout"):
        refused("conv", cv, b"bad argument", **{p: 0})
    for p in ("Cin", "Cout"):
        refused("conv", cv, b"bad argument", **{p: 4097})
    for k in (0, 2, 5, 9):
        refused("conv", cv, b"ksize %d is not 1, 3 or 7" % k, ksize=k)
    for s in (0, 3, -1):
        refused("conv", cv, b"stride %d is not 1 or 2" % s, stride=s)
    for d in (0, 65, -2):
        refused("conv", cv, b"dilation %d is not in 1 .. 64" % d, dilation=d)
    refused("conv", cv, b"pad -1 is not in", pad=-1)
    refused("conv", cv, b"pad 65537 is not in", pad=65537)
    refused("conv", cv, b"above 2^24", Hin=(1 << 24) + 1)
    for a in (-1, 2, 3):
        refused("conv", cv, b"act %d is not 0" % a, act=a)
    # Ho <= 0: the window (dilation (k - 1) + 1) does not fit the padded image
    refused("conv", cv, b"no output: 4 x 10 with ksize 3, dilation 4, pad 1", Hin=4, dilation=4, pad=1)
    refused("conv", cv, b"no output: 13 x 2 with ksize 3, dilation 2, pad 1", Win=2, pad=1)
    refused("conv", cv, b"no output", Hin=6, Win=6, ksize=7, dilation=1, pad=0)
    # the slice and the per-sample bias
    refused("conv", cv, b"channel slice [0, 0 + 40) does not fit rows of 39", ycs=39)
    refused("conv", cv, b"channel slice [61, 61 + 40) does not fit rows of 100", ycs=100, yco=61, residual=None)
    refused("conv", cv, b"channel slice [-1, -1 + 40)", yco=-1, ycs=100, residual=None)
    for bs in (1, 39, -40):
        refused("conv", cv, b"bias_bstride %d is not 0 or at least Cout = 40" % bs, bias_bstride=bs)
    # overlaps: the output with an input, the residual without being y, the residual as y of a slice
    M = 2 * 13 * 10
    refused("conv", cv, b"an output overlaps x, w, bias", y=X + 4 * (2 * 13 * 10 * 16 - 1))
    refused("conv", cv, b"an output overlaps x, w, bias", y=W + 4 * (40 * 9 * 16 - 1))
    refused("conv", cv, b"an output overlaps x, w, bias", bias=Y + 4 * (M * 40 - 1))
    refused("conv", cv, b"an output overlaps x, w, bias", bias=Y - 4 * (40 + 39), bias_bstride=40)          # sample 1's bias row reaches y
    refused("conv", cv, b"overlaps the residual without y being the residual", residual=Y + 4)
    refused("conv", cv, b"overlaps the residual without y being the residual", residual=Y - 4 * (M * 40 - 1))
    refused("conv", cv, b"cannot be y with rows of 100 floats at channel 0", residual=Y, ycs=100)
    refused("conv", cv, b"cannot be y with rows of 80 floats at channel 40", residual=Y, ycs=80, yco=40)
    refused("conv", cv, b"more than 2^31 - 1 output positions", B=1 << 11, Hin=1 << 10, Win=1 << 10, ksize=1, dilation=1, pad=0, Cin=1, Cout=1,
            ycs=1, residual=None)

    mp = dict(x=X, B=2, H=7, W=5, C=24, y=Y)
    for p in ("x", "y"):
        refused("maxpool", mp, b"NULL pointer", **{p: None})
    for p in ("B", "H", "W", "C"):
        refused("maxpool", mp, b"bad argument", **{p: 0})
    refused("maxpool", mp, b"limit per call is 2^31", H=1 << 14, W=1 << 14)
    refused("maxpool", mp, b"x and y overlap", y=X + 4 * (2 * 7 * 5 * 24 - 1))
    refused("maxpool", mp, b"x and y overlap", x=Y + 4 * (2 * 4 * 3 * 24 - 1))

    gm = dict(x=X, B=2, HW=35, C=24, y=Y)
    for p in ("x", "y"):
        refused("global_mean", gm, b"NULL pointer", **{p: None})
    for p in ("B", "HW", "C"):
        refused("global_mean", gm, b"bad argument", **{p: 0})
    refused("global_mean", gm, b"bad argument", B=65536)
    refused("global_mean", gm, b"limit per call is 2^31", HW=1 << 20, C=1 << 10)
    refused("global_mean", gm, b"x and y overlap", y=X + 4 * (2 * 35 * 24 - 1))

    ai = dict(img=X, alpha=W, camera_feat=Bi, B=2, H=8, W=6, y=Y)
    for p in ("img", "y"):
        refused("assemble_input", ai, b"NULL pointer", **{p: None})
    for p in ("B", "H", "W"):
        refused("assemble_input", ai, b"bad argument", **{p: 0})
    refused("assemble_input", ai, b"above 2^24", H=(1 << 24) + 1, W=1, B=1)
    refused("assemble_input", ai, b"limit per call is 2^31", H=1 << 14, W=1 << 14)
    refused("assemble_input", ai, b"y overlaps an input", y=X + 4 * (2 * 3 * 48 - 1))
    refused("assemble_input", ai, b"y overlaps an input", alpha=Y + 4 * (2 * 48 * 9 - 1))
    refused("assemble_input", ai, b"y overlaps an input", camera_feat=Y + 4 * (2 * 48 * 9 - 1))
    refused("assemble_input", ai, b"y overlaps an input", img=Y + 4 * (2 * 48 * 5 - 1), alpha=None, camera_feat=None)


def mock_model(backbone, name="cano_img2plane_backbone"):
    """The smallest model patch_model accepts, holding `backbone` under `name`."""
    class SR(nn.Module):
        def __init__(self):
            super().__init__()
            self.block0 = nn.Linear(1, 1)

    class Model(nn.Module):
        def __init__(self):
            super().__init__()
            self.renderer = nn.Module()
            self.superresolution = SR()
            self.secc_img2plane_backbone = nn.Identity()
            setattr(self, name, backbone)

    return Model()


def reference_like_backbone(encoder):
    import img2plane_common as i2p
    ref = i2p.Img2PlaneModel("rgb", "small")
    ref.low_reso_encoder = encoder
    return ref


def test_from_reference_reads_each_convs_geometry():
    from real3dportrait_amd.deeplabv3 import DeepLabV3, is_reference_deeplabv3
    mock = common.DeepLabV3(5)
    mock.load_state_dict(common.weights(91, 5), strict=True)
    assert is_reference_deeplabv3(mock) and not is_reference_deeplabv3(mock.encoder) and not is_reference_deeplabv3(nn.Identity())
    hip = DeepLabV3.from_reference(mock)
    assert type(hip) is DeepLabV3 and not hip.training and not is_reference_deeplabv3(hip)
    assert list(hip.state_dict()) == list(mock.state_dict()) and all(torch.equal(hip.state_dict()[k], v) for k, v in mock.state_dict().items())
    assert type(DeepLabV3.from_reference(common.DeepLabV3(6, "resnet18"))) is DeepLabV3
    # other geometries are refused: output stride 16 and 32, and one conv patched by hand
    assert DeepLabV3.from_reference(common.DeepLabV3(5, output_stride=16)) is None
    assert DeepLabV3.from_reference(common.DeepLabV3(5, output_stride=32)) is None
    for key, field, value in (("encoder.layer3.2.conv2", "dilation", (1, 1)), ("encoder.layer4.0.downsample.0", "stride", (2, 2)),
                              ("decoder.0.convs.2.0", "padding", (12, 12)), ("encoder.layer3.0.conv1", "padding", (1, 1))):
        odd = common.DeepLabV3(5)
        setattr(odd.get_submodule(key), field, value)
        assert DeepLabV3.from_reference(odd) is None, key
    odd = common.DeepLabV3(5)
    odd.encoder.maxpool = nn.MaxPool2d(2, 2)
    assert DeepLabV3.from_reference(odd) is None
    assert DeepLabV3.from_reference(nn.Identity()) is None


def test_patch_model_swaps_the_low_reso_encoder_on_request_only():
    from real3dportrait_amd import DeepLabV3, Img2PlaneModel, patch_model
    enc = common.DeepLabV3(5)
    with pytest.raises(ValueError, match="cano_low_reso_encoder=True needs cano_backbone=True"):
        patch_model(mock_model(reference_like_backbone(enc)), cano_low_reso_encoder=True)
    # without the switch the backbone keeps the reference's encoder object
    model = patch_model(mock_model(reference_like_backbone(enc)), cano_backbone=True)
    assert model.cano_img2plane_backbone.low_reso_encoder is enc and not hasattr(model.cano_img2plane_backbone, "_r3d_reference_low_reso_encoder")
    assert model.cano_img2plane_backbone._fast_encoder() is None
    model = patch_model(mock_model(reference_like_backbone(enc)), cano_backbone=True, cano_low_reso_encoder=True)
    bb = model.cano_img2plane_backbone
    assert type(bb) is Img2PlaneModel and type(bb.low_reso_encoder) is DeepLabV3 and bb._r3d_reference_low_reso_encoder is enc
    assert bb._fast_encoder() is bb.low_reso_encoder and "_r3d_reference_low_reso_encoder" not in dict(bb.named_modules())
    assert all(torch.equal(bb.low_reso_encoder.state_dict()[k], v) for k, v in enc.state_dict().items())
    # a foreign encoder, a geometry other than output stride 8 and an encoder of another input width are left alone
    import img2plane_common as i2p
    for other in (i2p.StandInEncoder(5), common.DeepLabV3(5, output_stride=16), common.DeepLabV3(6)):
        model = patch_model(mock_model(reference_like_backbone(other)), cano_backbone=True, cano_low_reso_encoder=True)
        bb = model.cano_img2plane_backbone
        assert bb.low_reso_encoder is other and not hasattr(bb, "_r3d_reference_low_reso_encoder") and bb._fast_encoder() is None
