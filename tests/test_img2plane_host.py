"""CPU: the image-to-plane backbone's host side (real3dportrait_amd/img2plane.py, include/r3d_hip_img2plane.h): state_dict
keys, the fp64 restatement against the reference's goldens, the weight and pixel-shuffle index maps, forward's refusals, the argument
checks of every r3d_i2p_* entry point, the header against its binding table, and patch_model(cano_backbone=True) on a mock model."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn as nn

import img2plane_common as common
import img2plane_ref64 as R64
from abi import C_RETURNS, entry_matches, header_declarations, refusals
from conftest import ROOT, load_golden
from real3dportrait_amd import synth

HEADER = "r3d_hip_img2plane.h"
LLVM = "/opt/rocm/lib/llvm/bin"


def package_model(mode="rgb", scale="small", encoder=True):
    from real3dportrait_amd.img2plane import Img2PlaneModel
    return Img2PlaneModel(96, hp={"img2plane_input_mode": mode, "img2plane_backbone_scale": scale},
                          low_reso_encoder=common.StandInEncoder(common.MODE_CHANNELS[mode] + 2) if encoder else None)


def own_keys(m):
    return sorted(k for k in m.state_dict() if not k.startswith("low_reso_encoder."))


def test_state_dict_keys_are_the_references():
    stored = load_golden("img2plane_keys")
    assert set(stored) == {"rgb.standard", "rgb.small", "rgb_alpha.small", "rgb_camera.small", "rgb_alpha_camera.small"}
    for tag, keys in stored.items():
        mode, scale = tag.split(".")
        assert own_keys(package_model(mode, scale)) == list(keys), tag
        assert sorted(k for k, _ in synth.img2plane_shapes(scale, common.MODE_CHANNELS[mode] + 2)) == list(keys), tag
    for scale, counts in synth.IMG2PLANE_BLOCKS.items():
        m = package_model("rgb", scale)
        assert (m.low_reso_vit.num_blocks, m.triplane_predictor_vit.num_blocks) == counts
        assert {k: tuple(v.shape) for k, v in m.state_dict().items() if not k.startswith("low_reso_encoder.")} == dict(synth.img2plane_shapes(scale, 5))


def test_load_state_dict_strict_round_trip():
    sd = common.weights(73, "small", 5)
    m = common.hip_model("rgb", "small", sd, "cpu")
    back = m.state_dict()
    assert all(torch.equal(back[k], v) for k, v in sd.items())
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in back.items() if k != "low_reso_vit.block2.attn.kv.bias"}, strict=True)
    with pytest.raises(RuntimeError):
        m.load_state_dict(dict(back, **{"low_reso_vit.block3.norm1.weight": torch.zeros(1024)}), strict=True)


@pytest.mark.parametrize("name", list(common.CASES))
def test_fp64_restatement_meets_the_reference(name):
    torch.set_num_threads(8)
    g, mode, scale, cin, sd, x = common.golden_case(name)
    m = common.hip_model(mode, scale, sd, "cpu")
    x_in = m.assemble_input(torch.from_numpy(x))
    assert x_in.shape[1] == cin and [int(v) for v in g["spec"][2:]] == [x.shape[0], cin, x.shape[2], x.shape[3]]
    if "alpha" in mode:
        assert set(np.unique(x_in[:, 3].numpy()).tolist()) == {0.0, 1.0}
    with torch.no_grad():
        feat_low = m.low_reso_encoder(x_in)
    stats = []
    planes, taps = R64.forward(sd, x_in, feat_low, torch.float64, stats)
    errs = {"planes": common.rel(planes.numpy(), g["planes"])}
    errs.update({k: common.rel(taps[k].numpy()[common.TAP_SLICES[k]], g[k]) for k in common.TAPS})
    print(name, errs)
    assert all(e <= common.TOL for e in errs.values()), errs
    # the condition on the inputs the maker stored: no attention is uniform or one-hot
    assert len(stats) == len(g["attention"]) == sum(synth.IMG2PLANE_BLOCKS[scale])
    for (blk, L, med), (gl, gmed) in zip(stats, g["attention"]):
        assert L == gl and abs(med - gmed) < 1e-3 and 2.0 / L < gmed < 0.9, (blk, L, med, gmed)


def test_index_maps_against_torch():
    from real3dportrait_amd.img2plane import conv_weight_cl, pixel_shuffle_source
    w = torch.arange(4 * 3 * 2 * 2, dtype=torch.float32).reshape(4, 3, 2, 2)
    cl = conv_weight_cl(w)
    assert cl.shape == (4, 2, 2, 3) and cl.is_contiguous()
    assert all(cl[o, ky, kx, c] == w[o, c, ky, kx] for o in range(4) for c in range(3) for ky in range(2) for kx in range(2))
    x = torch.arange(2 * 12 * 5 * 7, dtype=torch.float64).reshape(2, 12, 5, 7)
    ps = nn.PixelShuffle(2)(x)
    assert torch.equal(R64.pixel_shuffle2(x), ps)
    for c in range(3):
        for i in range(2):
            for j in range(2):
                assert torch.equal(ps[:, c, i::2, j::2], x[:, pixel_shuffle_source(c, i, j)])
    g = torch.Generator().manual_seed(3)
    y = torch.randn(2, 3, 5, 7, dtype=torch.float64, generator=g)
    assert float((R64.upsample2x_align(y) - nn.UpsamplingBilinear2d(scale_factor=2.0)(y)).abs().max()) < 1e-13
    one = torch.randn(1, 2, 1, 1, dtype=torch.float64, generator=g)
    assert torch.equal(R64.upsample2x_align(one), one.expand(1, 2, 2, 2))
    p = torch.randn(2, 6, 5, 7, dtype=torch.float64, generator=g)
    v = p.view(2, 3, 2, 5, 7)
    want = torch.stack([torch.flip(v[:, 0], [2]), torch.flip(v[:, 1], [2]), torch.flip(v[:, 2], [2, 3])], dim=1)
    assert torch.equal(R64.flip_planes(p), want)


def test_forward_refuses_before_the_library_is_entered():
    from real3dportrait_amd import _lib
    from real3dportrait_amd.img2plane import Img2PlaneModel
    with pytest.raises(ValueError, match="img2plane_input_mode"):
        Img2PlaneModel(96, hp={"img2plane_input_mode": "rgbd"})
    with pytest.raises(ValueError, match="img2plane_backbone_scale"):
        Img2PlaneModel(96, hp={"img2plane_backbone_scale": "huge"})
    with pytest.raises(ValueError, match="multiple of 3"):
        Img2PlaneModel(95)
    m = package_model()
    cam = package_model("rgb_alpha_camera")
    with _lib.counting() as calls:
        for bad, what in ((torch.zeros(1, 3, 64, 48), "square"), (torch.zeros(1, 3, 72, 72), "multiple of 16"), (torch.zeros(1, 4, 64, 64), r"\[B, 3, S, S\]"),
                          (torch.zeros(3, 64, 64), r"\[B, 3, S, S\]"), (torch.zeros(0, 3, 64, 64), "empty"), (torch.zeros(1, 3, 64, 64), "not on a GPU")):
            with pytest.raises(ValueError, match=what):
                m(bad)
        with pytest.raises(ValueError, match="ref_cameras"):
            cam(torch.zeros(1, 3, 64, 64))
        with pytest.raises(ValueError, match="ref_cameras"):
            cam(torch.zeros(2, 3, 64, 64), {"ref_cameras": torch.zeros(1, 25)})
        with pytest.raises(ValueError, match="ref_alphas"):
            cam(torch.zeros(1, 3, 64, 64), {"ref_cameras": torch.zeros(1, 25), "ref_alphas": torch.zeros(1, 1, 32, 32)})
        assert calls == []


def test_input_assembly_is_the_references():
    """img2plane_model.py:45-64 on the CPU for the four modes: channel counts, the alpha rule, grid_y / H (not W)."""
    x = torch.from_numpy(common.image(5, 2, 16, black_rows=4))
    cams = torch.arange(50, dtype=torch.float32).reshape(2, 25) / 50
    for mode, cin in common.MODE_CHANNELS.items():
        m = package_model(mode)
        got = m.assemble_input(x, {"ref_cameras": cams})
        assert got.shape == (2, cin + 2, 16, 16)
        assert torch.equal(got[:, :3], x)
        gx, gy = torch.meshgrid(torch.arange(16), torch.arange(16), indexing="ij")
        assert torch.equal(got[:, -2], (gx / 16).expand(2, 16, 16)) and torch.equal(got[:, -1], (gy / 16).expand(2, 16, 16))
        if "alpha" in mode:
            assert torch.equal(got[:, 3, :4], torch.zeros(2, 4, 16)) and torch.equal(got[:, 3, 4:], torch.ones(2, 12, 16))
        if "camera" in mode:
            feat = m.camera_to_channel(cams).detach()
            assert torch.equal(got[:, -5:-2], feat.reshape(2, 3, 1, 1).expand(2, 3, 16, 16))


def test_header_mirrors_its_table():
    from real3dportrait_amd import _lib
    lib = _lib.load()
    decls = header_declarations(HEADER)
    table = _lib.EXTENSION_SIGNATURES[HEADER]
    assert set(_lib.EXTENSION_SIGNATURES) == {HEADER}
    assert set(decls) == set(table) and len(decls) == 6 and all(n.startswith("r3d_i2p_") for n in decls)
    assert not set(table) & (set(_lib.SIGNATURES) | set(_lib.OPTIONAL_SIGNATURES))
    src = open(os.path.join(ROOT, "include", HEADER)).read()
    assert '#include "r3d_hip.h"' in src and HEADER not in open(os.path.join(ROOT, "include", "r3d_hip.h")).read()
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
    assert lib.r3d_version() == _lib.ABI_VERSION


@pytest.mark.parametrize("lang", ["c99", "c++17"])
def test_header_stands_alone(lang, tmp_path):
    clang = os.path.join(LLVM, "clang")
    if not os.path.exists(clang):
        pytest.skip("no %s: the header is not compiled here" % clang)
    flags = ["-x", "c", "-std=c99"] if lang == "c99" else ["-x", "c++", "-std=c++17"]
    for i, unit in enumerate(([HEADER], [HEADER, "r3d_hip.h"], ["r3d_hip.h", HEADER])):
        src = tmp_path / ("unit%d.%s" % (i, "c" if lang == "c99" else "cpp"))
        src.write_text("".join('#include "%s"\n' % h for h in unit))
        r = subprocess.run([clang] + flags + ["-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                           capture_output=True, text=True)
        assert r.returncode == 0, "%s as %s:\n%s" % (" + ".join(unit), lang, r.stderr)


def test_entry_points_refuse_bad_arguments():
    """NULL, ranges, overlap and alignment of every r3d_i2p_* entry point: R3D_ERR_INVALID_ARG and a tagged message, before any launch
    (the addresses are never dereferenced)."""
    from real3dportrait_amd import _lib
    refused = refusals(_lib.load(), "r3d_i2p_")
    X, Y, Z = 0x10000000, 0x20000000, 0x30000000
    att = dict(q=X, kv=Y, B=1, N=70, L=100, C=1024, heads=4, scale=0.0625, out=Z)
    for p in ("q", "kv", "out"):
        refused("attention", att, b"NULL pointer", **{p: None})
        refused("attention", att, b"16-byte aligned", **{p: att[p] + 4})
    for p in ("B", "N", "L", "C", "heads"):
        refused("attention", att, b"bad argument", **{p: 0})
    refused("attention", att, b"bad argument", B=65536)
    refused("attention", att, b"multiple of 16", C=1024, heads=3)          # C % heads
    refused("attention", att, b"multiple of 16", C=96, heads=4)            # D = 24
    refused("attention", att, b"multiple of 16", C=1088, heads=4)          # D = 272
    for bad in (float("nan"), float("inf"), float("-inf")):
        refused("attention", att, b"scale is not finite", scale=bad)
    refused("attention", att, b"limit per call is 2^31", N=1 << 21)
    refused("attention", att, b"limit per call is 2^31", L=1 << 20)
    refused("attention", att, b"out overlaps q or kv", out=X)               # the in-place form is refused
    refused("attention", att, b"out overlaps q or kv", out=X + 4 * 70 * 1024 - 16)
    refused("attention", att, b"out overlaps q or kv", out=Y + 16)
    up = dict(x=X, B=1, H=5, W=7, C=3, y=Y)
    for p in ("x", "y"):
        refused("upsample2x", up, b"NULL pointer", **{p: None})
    for p in ("B", "H", "W", "C"):
        refused("upsample2x", up, b"bad argument", **{p: 0})
    refused("upsample2x", up, b"limit per call is 2^31", H=1 << 14, W=1 << 14)
    refused("upsample2x", up, b"x and y overlap", y=X + 4 * 104)
    refused("upsample2x", up, b"x and y overlap", x=Y + 4 * 419)
    ps = dict(x=X, B=1, h=5, w=7, Co=3, y=Y, y_cstride=8, y_coffset=2)
    for p in ("x", "y"):
        refused("pixel_shuffle", ps, b"NULL pointer", **{p: None})
    for p in ("B", "h", "w", "Co"):
        refused("pixel_shuffle", ps, b"bad argument", **{p: 0})
    refused("pixel_shuffle", ps, b"outside a row of 8", y_coffset=6)
    refused("pixel_shuffle", ps, b"outside a row of 8", y_coffset=-1)
    refused("pixel_shuffle", ps, b"outside a row of 0", y_cstride=0, y_coffset=0)
    refused("pixel_shuffle", ps, b"limit per call is 2^31", h=1 << 13, w=1 << 13)
    refused("pixel_shuffle", ps, b"x and y overlap", y=X)
    cp = dict(x=X, M=35, C=3, y=Y, y_cstride=8, y_coffset=5)
    for p in ("x", "y"):
        refused("copy_channels", cp, b"NULL pointer", **{p: None})
    refused("copy_channels", cp, b"bad argument", M=0)
    refused("copy_channels", cp, b"bad argument", C=0)
    refused("copy_channels", cp, b"outside a row of 8", y_coffset=6)
    refused("copy_channels", cp, b"outside a row of 8", y_coffset=-3)
    refused("copy_channels", cp, b"limit per call is 2^31", M=1 << 28)
    refused("copy_channels", cp, b"x and y overlap", y=X + 4 * 104)
    tr = dict(x=X, B=2, C=5, H=5, W=7, y=Y)
    for p in ("x", "y"):
        refused("nchw_to_cl", tr, b"NULL pointer", **{p: None})
    for p in ("B", "C", "H", "W"):
        refused("nchw_to_cl", tr, b"bad argument", **{p: 0})
    refused("nchw_to_cl", tr, b"limit per call is 2^31", H=1 << 14, W=1 << 14)
    refused("nchw_to_cl", tr, b"x and y overlap", y=X)
    po = dict(x=X, B=2, H=5, W=7, Cp=4, planes=Y)
    for p in ("x", "planes"):
        refused("planes_out", po, b"NULL pointer", **{p: None})
    for p in ("B", "H", "W", "Cp"):
        refused("planes_out", po, b"bad argument", **{p: 0})
    refused("planes_out", po, b"limit per call is 2^31", H=1 << 14, W=1 << 14)
    refused("planes_out", po, b"x and planes overlap", planes=X + 4 * 839)


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


def test_patch_model_swaps_the_canonical_backbone_only():
    from real3dportrait_amd import Img2PlaneModel, patch_model
    children = lambda m: {n: type(c).__name__ for n, c in m.named_children()}
    ref = common.Img2PlaneModel("rgb", "small")
    sd = common.weights(73, "small", 5)
    ref.load_state_dict(dict(sd, **{"low_reso_encoder." + k: v for k, v in ref.low_reso_encoder.state_dict().items()}), strict=True)
    # without the switch, and with it off: the backbone stays
    for kw in ({}, {"cano_backbone": False}):
        plain = patch_model(mock_model(ref), **kw)
        assert plain.cano_img2plane_backbone is ref and not hasattr(plain, "_r3d_reference_cano_backbone")
    model = patch_model(mock_model(ref), cano_backbone=True)
    new = model.cano_img2plane_backbone
    assert type(new) is Img2PlaneModel and model._r3d_reference_cano_backbone is ref
    assert new.low_reso_encoder is ref.low_reso_encoder and new.input_mode == "rgb" and not new.training
    assert (new.low_reso_vit.num_blocks, new.triplane_predictor_vit.num_blocks) == (2, 1)
    got = new.state_dict()
    assert sorted(got) == sorted(ref.state_dict()) and all(torch.equal(got[k], v) for k, v in ref.state_dict().items())
    want = dict(children(plain), cano_img2plane_backbone="Img2PlaneModel")          # (the stand-in carries the same class name)
    assert children(model) == want and "_r3d_reference_cano_backbone" not in dict(model.named_modules())
    # OSAvatar_Img2plane holds it as img2plane_backbone
    model = patch_model(mock_model(ref, "img2plane_backbone"), cano_backbone=True)
    assert type(model.img2plane_backbone) is Img2PlaneModel and model._r3d_reference_cano_backbone is ref
    # anything else is left alone: another class, and this package's own module
    for other in (nn.Identity(), new):
        model = patch_model(mock_model(other), cano_backbone=True)
        assert model.cano_img2plane_backbone is other and not hasattr(model, "_r3d_reference_cano_backbone")
