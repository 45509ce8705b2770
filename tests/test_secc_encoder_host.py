"""CPU: the SECC encoder's host side (real3dportrait_amd/segformer.py, r3d_secc_* of include/r3d_hip.h).

The fp64 restatement (tests/segformer_ref64.py) against the reference's goldens, the head fold, argument validation of the C entry points
(which runs before any HIP call), the patch_model swap and the kernels' scratch use."""
import ctypes
import sys
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden
import segformer_ref64 as R64
from real3dportrait_amd import synth


def secc_input(seed, B, in_dim, H, W):
    """tests/golden/make_golden_secc.py's input (hash uniform in [-1, 1])."""
    return synth.hash_uniform(seed, B * in_dim * H * W, stream=5).reshape(B, in_dim, H, W) * np.float32(2.0) - np.float32(1.0)


def golden_case(name):
    g = load_golden(name)
    sw, sx, B, in_dim, H, W = (int(v) for v in g["spec"])
    sd = synth.synth_secc_backbone(sw, str(g["mode"]))
    return g, sd, secc_input(sx, B, in_dim, H, W)


def rel(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(a - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("name", ["secc_a_r64", "secc_b_r64"])
def test_fp64_restatement_matches_reference_goldens(name):
    g, sd, x = golden_case(name)
    feats, head, planes = R64.backbone(sd, torch.from_numpy(x))
    for i in range(4):
        assert rel(feats[i].numpy(), g["c%d" % (i + 1)]) <= 1e-5, i
    assert rel(head.numpy(), g["head"]) <= 1e-5
    assert rel(planes.numpy(), g["planes"]) <= 1e-5


def test_fp64_restatement_matches_512_golden():
    torch.set_num_threads(8)
    g, sd, x = golden_case("secc_c_r512")
    feats = R64.encoder(sd, torch.from_numpy(x))
    head = R64.head(sd, feats)
    # at 512^2 the golden's own fp32 rounding (the reference runs in fp32) reaches 3.6e-5 of max|c4| against this fp64 evaluation
    assert rel(feats[3].numpy(), g["c4"]) <= 1e-4
    assert rel(head[:, :, ::8, ::8].numpy(), g["head_s8"]) <= 1e-4


def test_fp64_restatement_matches_non_square_golden():
    """288 x 256 (H != W): an H / W swap in the token reshape, the SR-conv grid or the head's resize would show here."""
    torch.set_num_threads(8)
    g, sd, x = golden_case("secc_d_r288x256")
    feats, head, planes = R64.backbone(sd, torch.from_numpy(x))
    errs = {"c1_s2": rel(feats[0][..., ::2, ::2].numpy(), g["c1_s2"]), "head_s8": rel(head[..., ::8, ::8].numpy(), g["head_s8"]),
            "planes_s8": rel(planes[..., ::8, ::8].numpy(), g["planes_s8"])}
    for i in (2, 3, 4):
        errs["c%d" % i] = rel(feats[i - 1].numpy(), g["c%d" % i])
    assert all(e <= 1e-4 for e in errs.values()), errs         # the golden's own fp32 rounding, as at 512^2


def test_head_fold_equals_unfolded_head():
    g, sd, x = golden_case("secc_a_r64")
    feats = [torch.from_numpy(g["c%d" % i]).double() for i in range(1, 5)]
    a, b = R64.head(sd, feats), R64.head_folded(sd, feats)
    assert float((a - b).abs().max()) <= 1e-12 * float(a.abs().max())


def test_synth_weights_give_a_peaked_softmax():
    """The q / k gains of synth_secc_backbone put the stage-1 attention logits around +-20 (the issue's 'peaked, not uniform')."""
    g, sd, x = golden_case("secc_a_r64")
    import torch.nn.functional as F
    t = lambda k: torch.from_numpy(sd[k]).double()
    xx = torch.from_numpy(x).double()
    y = F.conv2d(xx, t("prenet.weight") / 3.0, t("prenet.bias"))
    y = F.conv2d(y, t("mix_vit.patch_embed1.proj.weight"), t("mix_vit.patch_embed1.proj.bias"), stride=4, padding=3)
    tok = F.layer_norm(y.flatten(2).transpose(1, 2), (32,), t("mix_vit.patch_embed1.norm.weight"), t("mix_vit.patch_embed1.norm.bias"), 1e-5)
    n = F.layer_norm(tok, (32,), t("mix_vit.block1.0.norm1.weight"), t("mix_vit.block1.0.norm1.bias"), 1e-6)
    q = n @ t("mix_vit.block1.0.attn.q.weight").T + t("mix_vit.block1.0.attn.q.bias")
    r = F.conv2d(n.transpose(1, 2).reshape(1, 32, 16, 16), t("mix_vit.block1.0.attn.sr.weight"), t("mix_vit.block1.0.attn.sr.bias"), stride=8)
    r = F.layer_norm(r.flatten(2).transpose(1, 2), (32,), t("mix_vit.block1.0.attn.norm.weight"), t("mix_vit.block1.0.attn.norm.bias"), 1e-5)
    k = (r @ t("mix_vit.block1.0.attn.kv.weight").T + t("mix_vit.block1.0.attn.kv.bias"))[..., :32]
    s = (q @ k.transpose(1, 2)) * 32 ** -0.5
    assert 8.0 <= float(s.abs().max()) <= 60.0


def test_state_dict_keys_match_the_reference_layout():
    from real3dportrait_amd.segformer import SegFormerSECC2PlaneBackbone
    for mode in ("cano_src_tgt", "cano_tgt"):
        m = SegFormerSECC2PlaneBackbone(pncc_cond_mode=mode)
        ref = synth.secc_backbone_shapes(mode)
        sd = m.state_dict()
        assert sorted(sd) == sorted(k for k, _ in ref)
        for k, shape in ref:
            assert tuple(sd[k].shape) == tuple(shape), k
        m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_secc_backbone(3, mode).items()}, strict=True)


def test_parameter_edits_and_replacements_are_seen_by_the_next_prepare():
    from real3dportrait_amd import SegFormerSECC2PlaneBackbone
    from test_state_host import replaced_at_same_address
    m = SegFormerSECC2PlaneBackbone().eval()
    a = m._prepare()
    assert m._prepare() is a
    with torch.no_grad():
        m.mix_vit.patch_embed2.proj.weight.add_(0.01)
    b = m._prepare()
    assert b is not a and not torch.equal(b["conv"]["pe2"], a["conv"]["pe2"]) and torch.equal(b["wfold1"], a["wfold1"])
    with torch.no_grad():
        m.fuse_head.linear_fuse.bn.running_var.mul_(2.0)
    c = m._prepare()
    assert c is not b and not torch.equal(c["bn_scale"], b["bn_scale"]) and torch.equal(c["conv"]["pe2"], b["conv"]["pe2"])
    # a parameter replaced by another tensor at the same address and version (what the caching allocator makes of a freed one)
    d, e = replaced_at_same_address(m.fuse_head.linear_c1.proj, "weight", m._prepare)
    # (3 w rounds to fp32 and so does the folded row, a dot product of 32 terms in fp64: <= 34 x 2^-24 of max|3 wfold1| = 2e-6)
    assert e is not d and float((e["wfold1"] - d["wfold1"] * 3.0).abs().max()) <= 1e-5 * float(d["wfold1"].abs().max())
    assert not torch.equal(e["wfold1"], d["wfold1"]) and torch.equal(e["wfold2"], d["wfold2"])
    assert m._prepare() is e


def test_unsupported_configurations_raise():
    from real3dportrait_amd.segformer import SegFormerSECC2PlaneBackbone
    with pytest.raises(NotImplementedError):
        SegFormerSECC2PlaneBackbone(mode="b3")
    m = SegFormerSECC2PlaneBackbone()
    with pytest.raises(NotImplementedError):
        m._check_input(torch.zeros(1, 9, 80, 64))
    with pytest.raises(NotImplementedError):
        m._check_input(torch.zeros(1, 9, 32 * 33, 32 * 32))      # 1056 keys


def test_c_entry_points_reject_bad_arguments_without_a_gpu():
    from real3dportrait_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(64)      # never dereferenced: validation fails first
    rc = lib.r3d_secc_embed1(None, 1, 9, 64, 64, one, one, one, one, one, one, one, None)
    assert rc == -1 and b"NULL" in lib.r3d_last_error()
    rc = lib.r3d_secc_embed1(one, 1, 9, 80, 64, one, one, one, one, one, one, one, None)
    assert rc == -1 and b"multiples of 32" in lib.r3d_last_error()
    rc = lib.r3d_secc_embed1(one, 1, 9, 32 * 33, 32 * 32, one, one, one, one, one, one, one, None)
    assert rc == -1 and b"1024" in lib.r3d_last_error()
    rc = lib.r3d_secc_embed1(one, 1, 7, 64, 64, one, one, one, one, one, one, one, None)
    assert rc == -1 and b"in_dim" in lib.r3d_last_error()
    rc = lib.r3d_secc_attention(one, one, 1, 256, 1025, 64, 2, 0.17, one, None)
    assert rc == -1 and b"1025" in lib.r3d_last_error()
    rc = lib.r3d_secc_attention(one, one, 1, 256, 256, 64, 1, 0.17, one, None)
    assert rc == -1 and b"C = 32 heads" in lib.r3d_last_error()
    rc = lib.r3d_secc_attention(None, one, 1, 256, 256, 64, 2, 0.17, one, None)
    assert rc == -1 and b"NULL" in lib.r3d_last_error()
    rc = lib.r3d_secc_head(one, 1, 20, 16, one, one, one, one, one, one, one, one, None)
    assert rc == -1 and b"multiples of 8" in lib.r3d_last_error()
    rc = lib.r3d_secc_head(one, 1, 16, 16, None, one, one, one, one, one, one, one, None)
    assert rc == -1 and b"NULL" in lib.r3d_last_error()
    rc = lib.r3d_secc_linear(None, 64, 32, None, None, 0.0, one, None, 32, 0, None, one, None)
    assert rc == -1 and b"NULL" in lib.r3d_last_error()
    rc = lib.r3d_secc_linear(one, 64, 32, one, None, 1e-6, one, None, 32, 0, None, ctypes.c_void_p(1 << 30), None)
    assert rc == -1 and b"NULL" in lib.r3d_last_error()      # LayerNorm weight without its bias
    rc = lib.r3d_secc_linear(one, 64, 32, None, None, 0.0, one, None, 32, 0, None, one, None)
    assert rc == -1 and b"overlap" in lib.r3d_last_error()
    rc = lib.r3d_secc_conv(one, 1, 16, 16, 32, one, one, 64, 3, 2, 3, None, None, 0.0, one, None)
    assert rc == -1 and b"bad argument" in lib.r3d_last_error()
    rc = lib.r3d_secc_dwconv_gelu(one, 1, 16, 16, 128, one, one, one, None)
    assert rc == -1 and b"bad argument" in lib.r3d_last_error()      # in place is not supported
    rc = lib.r3d_secc_layernorm(one, 16, 32, one, one, 0.0, one, None)
    assert rc == -1 and b"bad argument" in lib.r3d_last_error()
    rc = lib.r3d_secc_conv(one, 1, 1, 1, 3, one, one, 17, 4, 2, 1, None, None, 0.0, ctypes.c_void_p(1 << 30), None)
    assert rc == -1 and b"empty output" in lib.r3d_last_error()      # 1 + 2 - 4 < 0: nn.Conv2d has no output either
    # a "bad argument" names the values it is about
    far = ctypes.c_void_p(1 << 30)
    rc = lib.r3d_secc_embed1(one, 1, 7, 64, 64, one, one, one, one, one, one, one, None)
    assert rc == -1 and b"bad argument" in lib.r3d_last_error() and b"in_dim = 7" in lib.r3d_last_error()
    rc = lib.r3d_secc_conv(one, 1, 16, 16, 32, one, one, 64, 3, 0, 1, None, None, 0.0, far, None)
    assert rc == -1 and b"bad argument" in lib.r3d_last_error() and b"stride = 0" in lib.r3d_last_error()
    rc = lib.r3d_secc_conv(one, 1, 16, 16, 1025, one, one, 64, 3, 2, 1, None, None, 0.0, far, None)
    assert rc == -1 and b"bad argument" in lib.r3d_last_error() and b"Cin = 1025" in lib.r3d_last_error()
    rc = lib.r3d_secc_conv(one, 1, 16, 16, 32, one, one, 64, 3, 2, 3, None, None, 0.0, far, None)
    assert rc == -1 and b"bad argument" in lib.r3d_last_error() and b"pad = 3" in lib.r3d_last_error()
    rc = lib.r3d_secc_conv(one, 1, 16, 16, 32, one, one, 64, 9, 2, 1, None, None, 0.0, far, None)
    assert rc == -1 and b"bad argument" in lib.r3d_last_error() and b"ksize = 9" in lib.r3d_last_error()
    rc = lib.r3d_secc_linear(one, 64, 4097, None, None, 0.0, one, None, 32, 0, None, far, None)
    assert rc == -1 and b"bad argument" in lib.r3d_last_error() and b"K = 4097" in lib.r3d_last_error()
    rc = lib.r3d_secc_layernorm(one, 16, 32, one, one, 0.0, far, None)
    assert rc == -1 and b"bad argument" in lib.r3d_last_error() and b"eps = 0" in lib.r3d_last_error()
    rc = lib.r3d_secc_attention(one, far, 1, 256, 256, 64, 1, 0.17, ctypes.c_void_p(1 << 31), None)
    assert rc == -1 and b"bad argument" in lib.r3d_last_error() and b"C = 64, heads = 1" in lib.r3d_last_error()
    rc = lib.r3d_secc_dwconv_gelu(one, 1, 16, 0, 128, one, one, far, None)
    assert rc == -1 and b"bad argument" in lib.r3d_last_error() and b"W = 0" in lib.r3d_last_error()
    # products of sizes that the entry point or its kernel forms in int or unsigned are refused at 2^31, before any is formed
    rc = lib.r3d_secc_conv(one, 65536, 512, 512, 32, one, one, 64, 3, 1, 1, None, None, 0.0, one, None)          # B Ho Wo = 2^34
    assert rc == -1 and b"2^31" in lib.r3d_last_error() and b"B Ho Wo" in lib.r3d_last_error()
    rc = lib.r3d_secc_conv(one, 1 << 15, 256, 256, 32, one, one, 64, 3, 1, 1, None, None, 0.0, one, None)        # = 2^31 exactly
    assert rc == -1 and b"2^31" in lib.r3d_last_error()
    rc = lib.r3d_secc_embed1(one, 1 << 21, 9, 128, 128, one, one, one, one, one, one, one, None)                  # B (H/4)(W/4) = 2^31
    assert rc == -1 and b"2^31" in lib.r3d_last_error() and b"B (H/4)(W/4)" in lib.r3d_last_error()
    rc = lib.r3d_secc_dwconv_gelu(one, 65536, 2048, 2048, 128, one, one, one, None)                               # 2^45 elements, 2^37 blocks
    assert rc == -1 and b"2^31" in lib.r3d_last_error() and b"blocks" in lib.r3d_last_error()
    rc = lib.r3d_secc_linear(one, (1 << 31) - 63, 32, None, None, 0.0, one, None, 32, 0, None, one, None)         # the last 64-row tile ends at 2^31
    assert rc == -1 and b"2^31" in lib.r3d_last_error()
    rc = lib.r3d_secc_head(one, 1 << 17, 128, 128, one, one, one, one, one, one, one, one, None)                  # B H1 W1 = 2^31
    assert rc == -1 and b"2^31" in lib.r3d_last_error()


def test_c_entry_points_reject_racing_overlaps_without_a_gpu():
    """Outputs that overlap an input the same launch still reads (include/r3d_hip.h states each rule); addresses in floats."""
    from real3dportrait_amd import _lib
    lib = _lib.load()
    at = lambda i: ctypes.c_void_p(4 * (1 << 20) + 4 * i)       # never dereferenced: validation fails first
    w = ctypes.c_void_p(1 << 40)
    # conv: x [1, 16, 16, 32] = 8192 floats, y [1, 8, 8, 64] = 4096
    rc = lib.r3d_secc_conv(at(0), 1, 16, 16, 32, w, w, 64, 3, 2, 1, None, None, 0.0, at(8191), None)
    assert rc == -1 and b"overlap" in lib.r3d_last_error()
    rc = lib.r3d_secc_conv(at(4096), 1, 16, 16, 32, w, w, 64, 3, 2, 1, None, None, 0.0, at(1), None)
    assert rc == -1 and b"overlap" in lib.r3d_last_error()
    # embed1: x [1, 9, 64, 64] = 36864 floats, y [1, 16, 16, 32] = 8192
    rc = lib.r3d_secc_embed1(at(0), 1, 9, 64, 64, w, w, w, w, w, w, at(36863), None)
    assert rc == -1 and b"overlap" in lib.r3d_last_error()
    rc = lib.r3d_secc_embed1(at(8191), 1, 9, 64, 64, w, w, w, w, w, w, at(0), None)
    assert rc == -1 and b"overlap" in lib.r3d_last_error()
    # attention: q / out [1, 64, 64] = 4096 floats, kv [1, 16, 128] = 2048
    rc = lib.r3d_secc_attention(at(0), at(10000), 1, 64, 16, 64, 2, 0.17, at(12047), None)
    assert rc == -1 and b"overlap" in lib.r3d_last_error()
    rc = lib.r3d_secc_attention(at(0), at(10000), 1, 64, 16, 64, 2, 0.17, at(5905), None)
    assert rc == -1 and b"overlap" in lib.r3d_last_error()
    rc = lib.r3d_secc_attention(at(0), at(10000), 1, 64, 16, 64, 2, 0.17, at(32), None)
    assert rc == -1 and b"overlap" in lib.r3d_last_error()      # out overlaps q without being q
    # dwconv: [1, 4, 4, 128] = 2048 floats, any overlap
    rc = lib.r3d_secc_dwconv_gelu(at(0), 1, 4, 4, 128, w, w, at(2047), None)
    assert rc == -1 and b"overlap" in lib.r3d_last_error()
    rc = lib.r3d_secc_dwconv_gelu(at(128), 1, 4, 4, 128, w, w, at(0), None)
    assert rc == -1 and b"overlap" in lib.r3d_last_error()
    # layernorm: partial overlap (y == x is in place and allowed)
    rc = lib.r3d_secc_layernorm(at(0), 16, 32, w, w, 1e-5, at(32), None)
    assert rc == -1 and b"overlap" in lib.r3d_last_error()
    # linear: x [64, 32] = 2048 floats, y and the residual [64, 64] = 4096; a residual that is not y itself may not share a float with it
    rc = lib.r3d_secc_linear(at(0), 64, 32, None, None, 0.0, w, None, 64, 0, at(10000 + 4095), at(10000), None)
    assert rc == -1 and b"overlap" in lib.r3d_last_error() and b"residual" in lib.r3d_last_error()
    rc = lib.r3d_secc_linear(at(0), 64, 32, None, None, 0.0, w, None, 64, 0, at(10000), at(2047), None)
    assert rc == -1 and b"overlap" in lib.r3d_last_error()
    # head: out [1, 256, 8, 8] = 16384 floats; c1 2048, f2 4096, f3 1024, f4 256
    ins = [at(100000), at(200000), at(300000), at(400000), at(500000)]      # c1, f2, f3, f4, w1f
    for j in range(5):
        args = list(ins)
        args[j] = at(16383) if j % 2 else at(-100)
        c1, f2, f3, f4, w1f = args
        rc = lib.r3d_secc_head(c1, 1, 8, 8, w1f, f2, f3, f4, w, w, w, at(0), None)
        assert rc == -1 and b"overlap" in lib.r3d_last_error(), j


def _reference_like_backbone(mode="b0", pncc_cond_mode="cano_src_tgt"):
    """A CPU stand-in with the reference's class name, attributes and state_dict (the reference module needs timm / mmcv)."""
    from real3dportrait_amd.segformer import SegFormerSECC2PlaneBackbone as Hip
    import torch.nn as nn

    class SegFormerSECC2PlaneBackbone(nn.Module):
        pass

    m = SegFormerSECC2PlaneBackbone()
    h = Hip(pncc_cond_mode=pncc_cond_mode)
    for name in ("prenet", "mix_vit", "fuse_head"):
        setattr(m, name, getattr(h, name))
    m.to_plane_cnn = nn.Sequential(nn.Conv2d(256, 256, 3, 1, 1), nn.LeakyReLU(0.01, inplace=True), nn.Conv2d(256, 256, 3, 1, 1),
                                   nn.LeakyReLU(0.01, inplace=True), nn.Conv2d(256, 256, 3, 1, 1), nn.LeakyReLU(0.01, inplace=True),
                                   nn.UpsamplingBilinear2d(scale_factor=2.0), nn.Conv2d(256, 96, 3, 1, 1))
    m.mode, m.pncc_cond_mode = mode, pncc_cond_mode
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_secc_backbone(5, pncc_cond_mode).items()}, strict=True)
    return m


def _model_shell(backbone):
    """The smallest model patch_model accepts (renderer, superresolution, the SECC backbone)."""
    import torch.nn as nn

    class SR(nn.Module):
        def __init__(self):
            super().__init__()
            self.block0 = nn.Linear(1, 1)

    class Model(nn.Module):
        def __init__(self):
            super().__init__()
            self.renderer = nn.Module()
            self.superresolution = SR()
            self.secc_img2plane_backbone = backbone

    return Model()


@pytest.mark.parametrize("pncc", ["cano_src_tgt", "cano_tgt"])
def test_patch_model_swaps_the_reference_backbone_with_identical_keys(pncc):
    from real3dportrait_amd import patch_model
    from real3dportrait_amd.segformer import SegFormerSECC2PlaneBackbone as Hip
    ref = _reference_like_backbone(pncc_cond_mode=pncc)
    before = {k: v.clone() for k, v in ref.state_dict().items()}
    model = patch_model(_model_shell(ref), secc_encoder=True)
    new = model.secc_img2plane_backbone
    assert isinstance(new, Hip) and new.pncc_cond_mode == pncc
    sd = new.state_dict()
    assert sorted(sd) == sorted(before)
    for k, v in before.items():
        assert sd[k].dtype == v.dtype and torch.equal(sd[k], v), k


def test_patch_model_leaves_the_backbone_without_the_flag_or_outside_b0():
    from real3dportrait_amd import patch_model
    from real3dportrait_amd.superresolution import ConvStack
    ref = _reference_like_backbone()
    model = patch_model(_model_shell(ref))
    assert model.secc_img2plane_backbone is ref and isinstance(ref.to_plane_cnn, ConvStack)       # only the existing tail swap
    ref = _reference_like_backbone(mode="b1")
    model = patch_model(_model_shell(ref), secc_encoder=True)
    assert model.secc_img2plane_backbone is ref


def test_secc_kernels_do_not_use_scratch():
    from test_render_kernel_resources import _kernel_metadata
    from real3dportrait_amd import _lib
    meta = _kernel_metadata(_lib.LIB_PATH)
    names = [k for k in meta if "3seg" in k]
    assert len(names) >= 7, names          # seg_gemm x 4 variants, seg_layernorm, seg_attention, seg_dwconv_gelu
    for k in names:
        assert int(meta[k]["private_segment_fixed_size"]) == 0, (k, meta[k])
        assert int(meta[k]["vgpr_spill_count"]) == 0, (k, meta[k])
