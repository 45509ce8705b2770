"""CPU: the HuBERT feature extractor's host side (real3dportrait_amd/hubert.py, include/r3d_hip_hubert.h): state_dict keys,
the legacy weight-norm keys, the effective positional weight, the chunk plan, the configs it refuses, the fp64 restatement against the
reference's goldens, the header against its binding table, and the argument checks of every r3d_hubert_* entry point."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import hubert_common as common
import hubert_ref64 as R64
from abi import C_RETURNS, entry_matches, header_declarations, refusals
from conftest import ROOT, load_golden
from real3dportrait_amd import synth

HEADER = "r3d_hip_hubert.h"
LLVM = "/opt/rocm/lib/llvm/bin"


def test_state_dict_keys_are_the_references():
    from real3dportrait_amd.hubert import HubertFeatureModel
    stored = load_golden("hubert_keys")
    assert set(stored) == {"small", "small.shapes", "wide", "wide.shapes"}
    for name, over in common.CONFIGS.items():
        sd = HubertFeatureModel(over).state_dict()
        assert sorted(sd) == list(stored[name]), name
        shapes = {k: tuple(int(v) for v in row[:np.count_nonzero(row)]) for k, row in zip(stored[name], stored[name + ".shapes"])}
        assert {k: tuple(v.shape) for k, v in sd.items()} == shapes == dict(synth.hubert_shapes(over)), name
    # the default is HuBERT-large; a config without masking has no masked_spec_embed, as the reference has none
    assert {k: tuple(v.shape) for k, v in HubertFeatureModel().state_dict().items()} == dict(synth.hubert_shapes())
    plain = HubertFeatureModel(dict(common.SMALL, mask_time_prob=0.0))
    assert "masked_spec_embed" not in plain.state_dict() and sorted(plain.state_dict()) == sorted(k for k, _ in synth.hubert_shapes(common.SMALL, False))


def test_load_state_dict_strict_and_the_legacy_weight_norm_keys():
    sd = common.weights(81, "small")
    m = common.hip_model("small", sd, "cpu")
    back = m.state_dict()
    assert all(torch.equal(back[k], v) for k, v in sd.items())
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in back.items() if k != "encoder.layers.1.attention.k_proj.bias"}, strict=True)
    p = "encoder.pos_conv_embed.conv."
    legacy = {k: v for k, v in sd.items() if "parametrizations" not in k}
    legacy[p + "weight_g"] = sd[p + "parametrizations.weight.original0"] * 2
    legacy[p + "weight_v"] = sd[p + "parametrizations.weight.original1"] * 3
    m.load_state_dict(legacy, strict=True)
    got = m.state_dict()
    assert torch.equal(got[p + "parametrizations.weight.original0"], legacy[p + "weight_g"])
    assert torch.equal(got[p + "parametrizations.weight.original1"], legacy[p + "weight_v"])
    assert p + "weight_g" not in got and p + "weight_g" in legacy          # the caller's dict is not modified


def test_effective_positional_weight_and_layouts():
    from real3dportrait_amd.hubert import conv1d_weight_cl, effective_pos_weight
    sd = common.weights(81, "small")
    g, v = (sd["encoder.pos_conv_embed.conv.parametrizations.weight.original%d" % i] for i in (0, 1))
    want = torch._weight_norm(v, g, 2)
    got = effective_pos_weight(g, v)
    assert got.dtype == torch.float32 and got.shape == v.shape
    assert float((got - want).abs().max()) <= 4e-7 * float(want.abs().max())          # a few fp32 ulps: torch forms the norm in fp32
    w64 = R64.pos_weight(g.double(), v.double())
    assert float((got.double() - w64).abs().max()) <= 6e-8 * float(w64.abs().max())   # one rounding of the fp64 value
    # the norm of every tap's [C, C / groups] slice is that tap's g
    assert torch.allclose(got.double().pow(2).sum(dim=(0, 1)).sqrt(), g.double().view(-1), rtol=1e-6)
    w = torch.arange(4 * 3 * 2, dtype=torch.float32).reshape(4, 3, 2)
    cl = conv1d_weight_cl(w)
    assert cl.shape == (4, 2, 3) and cl.is_contiguous() and all(cl[o, j, c] == w[o, c, j] for o in range(4) for c in range(3) for j in range(2))


def reference_plan(n, clip_frames=1000):
    """extract_hubert.py:48-71, the slices it takes, written as it writes them."""
    kernel, stride = 400, 320
    clip_length = stride * clip_frames
    num_iter = n // clip_length
    plan = []
    for i in range(num_iter):
        start_idx = clip_length * i
        plan.append((start_idx, min(start_idx + (clip_length - stride + kernel), n)))
    if n - clip_length * num_iter >= kernel:
        plan.append((clip_length * num_iter, n))
    return plan


def test_chunk_plan_is_the_references():
    from real3dportrait_amd.hubert import chunk_plan
    for name, (_, n, _, _, _) in common.CASES.items():
        assert chunk_plan(n) == [tuple(int(v) for v in c) for c in load_golden(name)["chunks"]], name
    assert chunk_plan(399) == [] and chunk_plan(400) == [(0, 400)]
    assert chunk_plan(320079) == [(0, 320079)] and chunk_plan(320080) == [(0, 320080)] and chunk_plan(320081) == [(0, 320080)]
    assert chunk_plan(640000) == [(0, 320080), (320000, 640000)]
    assert chunk_plan(320400) == [(0, 320080), (320000, 320400)]
    for n in (399, 400, 719, 720, 320079, 320080, 320081, 320399, 320400, 640000, 640079, 960085):
        assert chunk_plan(n) == reference_plan(n), n
    assert chunk_plan(9000, 10) == reference_plan(9000, 10) == [(0, 3280), (3200, 6480), (6400, 9000)]
    # the frames never fall short of expected_T (the reference's repeat branch is unreachable), whatever the remainder
    frames = lambda L: (L - 400) // 320 + 1
    for n in list(range(400, 3000)) + list(range(319990, 320500)) + [640000, 640079, 640080]:
        for cf in (2, 1000):
            assert sum(frames(e - s) for s, e in chunk_plan(n, cf)) == (n - 80) // 320, (n, cf)


def test_unsupported_configs_raise():
    from real3dportrait_amd.hubert import HubertFeatureModel
    for field, bad in (("feat_extract_norm", "group"), ("do_stable_layer_norm", False), ("feat_proj_layer_norm", False), ("conv_bias", False),
                       ("hidden_act", "relu"), ("feat_extract_activation", "relu"), ("conv_pos_batch_norm", True)):
        with pytest.raises(NotImplementedError, match=field):
            HubertFeatureModel(dict(common.SMALL, **{field: bad}))

    class Cfg:          # an object with attributes, as a transformers config is
        hidden_size, num_hidden_layers, num_attention_heads, intermediate_size = 64, 1, 2, 128
        conv_dim, conv_kernel, conv_stride = [16, 16], [10, 3], [5, 2]
        num_conv_pos_embeddings, num_conv_pos_embedding_groups, layer_norm_eps = 8, 2, 1e-5
        feat_extract_norm, do_stable_layer_norm = "layer", True
    m = HubertFeatureModel(Cfg)
    assert m.config["conv_dim"] == (16, 16) and m.frames(33) == (2, [5, 2]) and m.frames(9) == (None, [])
    Cfg.do_stable_layer_norm = False
    with pytest.raises(NotImplementedError, match="do_stable_layer_norm"):
        HubertFeatureModel(Cfg)
    with pytest.raises(ValueError, match="differ in length"):
        HubertFeatureModel(dict(common.SMALL, conv_kernel=(10, 3)))


def test_refuses_before_the_library_is_entered():
    from real3dportrait_amd import _lib
    from real3dportrait_amd.hubert import hubert_features, patch_hubert
    m = common.hip_model("small", common.weights(81, "small"), "cpu")
    with _lib.counting() as calls:
        with pytest.raises(ValueError, match="fewer than"):
            hubert_features(m, np.zeros(399))
        with pytest.raises(ValueError, match=r"\[B, n\]"):
            m(torch.zeros(400))
        with pytest.raises(ValueError, match="fewer than one frame"):
            m(torch.zeros(1, 399))
        with pytest.raises(ValueError, match="not on a GPU"):
            m(torch.zeros(1, 400))
        with pytest.raises(TypeError, match="HubertFeatureModel"):
            patch_hubert(object(), object())
        assert calls == []


@pytest.mark.parametrize("name", list(common.CASES))
def test_fp64_restatement_meets_the_reference(name):
    torch.set_num_threads(8)
    g, cfg_name, cfg, sd, speech = common.golden_case(name)
    assert [int(v) for v in g["spec"]] == list(common.CASES[name][2:4]) + [len(speech)] and str(g["config"]) == cfg_name
    assert np.array_equal(speech, np.round(speech * 32768) / 32768) and speech.dtype == np.float64          # PCM-16: exact in fp32
    stats = []
    chunks = [tuple(int(v) for v in c) for c in g["chunks"]]
    out, taps = R64.features(sd, cfg, torch.from_numpy(speech.astype(np.float32)), chunks, torch.float64, stats)
    errs = {"hubert": common.rel(out.numpy(), g["hubert"])}
    errs.update({k: common.rel(common.tap_rows(name, taps[k][0].numpy()), g[k]) for k in common.TAPS})
    print(name, errs)
    assert out.shape == g["hubert"].shape == ((len(speech) - 80) // 320, cfg["hidden_size"])
    assert all(e <= common.TOL for e in errs.values()), errs
    # the condition on the inputs the maker stored: no attention is uniform or one-hot
    assert len(stats) == len(g["attention"]) == cfg["num_hidden_layers"] * len(chunks)
    for (L, med), (gl, gmed) in zip(stats, g["attention"]):
        assert L == gl and abs(med - gmed) < 1e-3 and 2.0 / L < gmed < 0.9, (L, med, gmed)


def test_header_mirrors_its_table():
    from real3dportrait_amd import _lib
    lib = _lib.load()
    decls = header_declarations(HEADER)
    table = _lib.FEATURE_SIGNATURES[HEADER]
    assert set(decls) == set(table) and len(decls) == 4 and all(n.startswith("r3d_hubert_") for n in decls)
    assert not set(table) & (set(_lib.SIGNATURES) | set(_lib.OPTIONAL_SIGNATURES) | {n for t in _lib.EXTENSION_SIGNATURES.values() for n in t})
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
    assert lib.r3d_version() == _lib.ABI_VERSION == 80


@pytest.mark.parametrize("lang", ["c99", "c++17"])
def test_header_stands_alone(lang, tmp_path):
    clang = os.path.join(LLVM, "clang")
    if not os.path.exists(clang):
        pytest.skip("no %s: the header is not compiled here" % clang)
    flags = ["-x", "c", "-std=c99"] if lang == "c99" else ["-x", "c++", "-std=c++17"]
    for i, unit in enumerate(([HEADER], [HEADER, "r3d_hip.h"], ["r3d_hip.h", HEADER], ["r3d_hip_img2plane.h", HEADER])):
        src = tmp_path / ("unit%d.%s" % (i, "c" if lang == "c99" else "cpp"))
        src.write_text("".join('#include "%s"\n' % h for h in unit))
        r = subprocess.run([clang] + flags + ["-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                           capture_output=True, text=True)
        assert r.returncode == 0, "%s as %s:\n%s" % (" + ".join(unit), lang, r.stderr)


def test_entry_points_refuse_bad_arguments():
    """NULL, ranges, the 2^31 limit, alignment and overlap of every r3d_hubert_* entry point: R3D_ERR_INVALID_ARG and a tagged message,
    before any launch (the addresses are never dereferenced)."""
    from real3dportrait_amd import _lib
    refused = refusals(_lib.load(), "r3d_hubert_")
    X, Y, Z, W, P = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000
    ws = dict(wave=X, n=4077, stats=Y)
    for p in ("wave", "stats"):
        refused("wave_stats", ws, b"NULL pointer", **{p: None})
    refused("wave_stats", ws, b"bad argument", n=0)
    refused("wave_stats", ws, b"limit per call is 2^31", n=1 << 31)
    refused("wave_stats", ws, b"8-byte aligned", stats=Y + 4)
    refused("wave_stats", ws, b"stats overlaps wave", stats=X + 4 * 4076)
    refused("wave_stats", ws, b"stats overlaps wave", stats=X)

    c0 = dict(wave=X, stats=Y, B=2, sample_offset=0, sample_stride=3200, n_chunk=3280, w=W, bias=W + 4096, ln_g=W + 8192, ln_b=W + 12288,
              eps=1e-5, C0=32, k=10, stride=5, y=Z)
    for p in ("wave", "stats", "w", "bias", "ln_g", "ln_b", "y"):
        refused("conv0", c0, b"NULL pointer", **{p: None})
    for p in ("B", "n_chunk", "C0", "k", "stride"):
        refused("conv0", c0, b"bad argument", **{p: 0})
    refused("conv0", c0, b"bad argument", B=65536)
    refused("conv0", c0, b"outside the range", k=17)
    refused("conv0", c0, b"outside the range", stride=17)
    refused("conv0", c0, b"outside the range", C0=24)
    refused("conv0", c0, b"outside the range", C0=528)
    refused("conv0", c0, b"shorter than the kernel", n_chunk=9)
    for bad in (-1e-5, float("nan"), float("inf")):
        refused("conv0", c0, b"eps is negative or not finite", eps=bad)
    refused("conv0", c0, b"limit per call is 2^31", sample_offset=(1 << 31) - 3280 - 3200)
    refused("conv0", c0, b"limit per call is 2^31", sample_stride=1 << 31)
    refused("conv0", c0, b"limit per call is 2^31", B=16, sample_stride=0, n_chunk=(1 << 31) - 1, C0=512, stride=1)
    refused("conv0", c0, b"8-byte aligned", stats=Y + 4)
    refused("conv0", c0, b"y overlaps an input", y=X + 4 * (3200 + 3279))          # the last sample sequence 1 reads
    refused("conv0", c0, b"y overlaps an input", y=Y + 8)
    refused("conv0", c0, b"y overlaps an input", y=W + 4 * 319)
    refused("conv0", c0, b"y overlaps an input", ln_b=Z + 4 * (2 * 655 * 32 - 32))

    cl = dict(x=X, w=W, bias=P, ln_g=P + 4096, ln_b=P + 8192, eps=1e-5, B=2, Tin=99, Cin=32, Cout=48, k=3, stride=2, y=Z)
    for p in ("x", "w", "bias", "ln_g", "ln_b", "y"):
        refused("conv_ln_gelu", cl, b"NULL pointer", **{p: None})
    for p in ("B", "Tin", "Cin", "Cout", "k", "stride"):
        refused("conv_ln_gelu", cl, b"bad argument", **{p: 0})
    refused("conv_ln_gelu", cl, b"outside the range", k=5)
    for p in ("Cin", "Cout"):
        refused("conv_ln_gelu", cl, b"outside the range", **{p: 40})
        refused("conv_ln_gelu", cl, b"outside the range", **{p: 528})
    refused("conv_ln_gelu", cl, b"shorter than the kernel", Tin=2)
    for bad in (-1.0, float("nan"), float("inf")):
        refused("conv_ln_gelu", cl, b"eps is negative or not finite", eps=bad)
    refused("conv_ln_gelu", cl, b"limit per call is 2^31", B=1 << 10, Tin=1 << 16)
    refused("conv_ln_gelu", cl, b"limit per call is 2^31", Tin=1 << 23, Cin=16, Cout=512, k=1, stride=1)
    for p in ("x", "w"):
        refused("conv_ln_gelu", cl, b"16-byte aligned", **{p: cl[p] + 4})
    refused("conv_ln_gelu", cl, b"y overlaps an input", y=X + 4 * (2 * 99 * 32 - 1))
    refused("conv_ln_gelu", cl, b"y overlaps an input", y=W + 4 * (48 * 3 * 32 - 1))
    refused("conv_ln_gelu", cl, b"y overlaps an input", bias=Z + 4 * (2 * 49 * 48 - 1))

    pc = dict(x=X, w=W, bias=P, B=2, T=37, C=128, k=16, groups=4, y=Z)
    for p in ("x", "w", "bias", "y"):
        refused("pos_conv", pc, b"NULL pointer", **{p: None})
    for p in ("B", "T", "C", "k", "groups"):
        refused("pos_conv", pc, b"bad argument", **{p: 0})
    refused("pos_conv", pc, b"bad argument", B=65536)
    refused("pos_conv", pc, b"outside the range", k=129)
    refused("pos_conv", pc, b"outside the range", groups=3)            # C % groups
    refused("pos_conv", pc, b"outside the range", groups=16)           # C / groups = 8
    refused("pos_conv", pc, b"outside the range", groups=1)            # C / groups = 128
    refused("pos_conv", pc, b"outside the range", C=96, groups=4)      # C / groups = 24
    refused("pos_conv", pc, b"limit per call is 2^31", B=1 << 10, T=1 << 14)
    for p in ("x", "w"):
        refused("pos_conv", pc, b"16-byte aligned", **{p: pc[p] + 4})
    refused("pos_conv", pc, b"y overlaps an input", y=X)              # the in-place form
    refused("pos_conv", pc, b"y overlaps an input", y=X + 4 * (2 * 37 * 128 - 4))
    refused("pos_conv", pc, b"y overlaps an input", y=W + 16)
    refused("pos_conv", pc, b"y overlaps an input", bias=Z + 4 * (2 * 37 * 128 - 1))
