"""GPU: the HIP SECC encoder (real3dportrait_amd/segformer.py) against the reference's goldens (64^2, the 512^2 subset) and
the fp64 restatement (tests/segformer_ref64.py) at full size; determinism across batch, repeats and streams; the raw/flipped plane
hand-off to ImportanceRenderer.prepare_planes."""
import numpy as np
import pytest
import torch

import segformer_ref64 as R64
from test_secc_encoder_host import golden_case, rel, secc_input
from real3dportrait_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2e-4


def hip_backbone(sd, pncc="cano_src_tgt"):
    from real3dportrait_amd.segformer import SegFormerSECC2PlaneBackbone
    m = SegFormerSECC2PlaneBackbone(pncc_cond_mode=pncc)
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}, strict=True)
    return m.to(DEV).eval()


@pytest.mark.parametrize("name", ["secc_a_r64", "secc_b_r64"])
def test_goldens_64(name):
    g, sd, x = golden_case(name)
    m = hip_backbone(sd, str(g["mode"]))
    xt = torch.from_numpy(x).to(DEV)
    feats = m.forward_stages(xt)
    errs = {}
    for i in range(4):
        errs["c%d" % (i + 1)] = rel(feats[i].cpu().numpy(), g["c%d" % (i + 1)])
    errs["head"] = rel(m.forward_features(xt).cpu().numpy(), g["head"])
    errs["planes"] = rel(m(xt).cpu().numpy(), g["planes"])
    print(name, errs)
    assert all(e <= TOL for e in errs.values()), errs


def test_512_against_fp64_and_golden_subset():
    g, sd, x = golden_case("secc_c_r512")
    m = hip_backbone(sd)
    xt = torch.from_numpy(x).to(DEV)
    feats = m.forward_stages(xt)
    head = m.forward_features(xt)
    ref = R64.encoder(sd, xt.double())
    href = R64.head(sd, ref)
    errs = {"c%d" % (i + 1): rel(feats[i].cpu().numpy(), ref[i].cpu().numpy()) for i in range(4)}
    errs["head"] = rel(head.cpu().numpy(), href.cpu().numpy())
    errs["golden_c4"] = rel(feats[3].cpu().numpy(), g["c4"])
    errs["golden_head_s8"] = rel(head[:, :, ::8, ::8].cpu().numpy(), g["head_s8"])
    print("512:", errs)
    assert all(e <= TOL for e in errs.values()), errs


@pytest.mark.parametrize("B,H,W", [(2, 32, 32), (1, 32, 1024), (1, 1024, 32), (1, 1024, 1024)])
def test_sizes_at_the_edges_against_fp64(B, H, W):
    """32^2 (every L = 1, stage 4 is 1 x 1), a 1 x 32 and a 32 x 1 grid of keys, and 1024^2 (L = 1024, the key limit); the planes
    except at 1024^2 (the fp64 to_plane_cnn costs too much there)."""
    sd = synth.synth_secc_backbone(51)
    m = hip_backbone(sd)
    x = torch.from_numpy(secc_input(52, B, 9, H, W)).to(DEV)
    feats = m.forward_stages(x)
    head = m.forward_features(x)
    ref = R64.encoder(sd, x.double())
    href = R64.head(sd, ref)
    errs = {"c%d" % (i + 1): rel(feats[i].cpu().numpy(), ref[i].cpu().numpy()) for i in range(4)}
    errs["head"] = rel(head.cpu().numpy(), href.cpu().numpy())
    if H * W < 1024 * 1024:
        errs["planes"] = rel(m(x).cpu().numpy(), R64.flip_planes(R64.to_plane_cnn(sd, href)).cpu().numpy())
    print("%dx%dx%d:" % (B, H, W), errs)
    assert all(e <= TOL for e in errs.values()), errs


def test_non_square_golden():
    g, sd, x = golden_case("secc_d_r288x256")
    m = hip_backbone(sd, str(g["mode"]))
    xt = torch.from_numpy(x).to(DEV)
    feats = m.forward_stages(xt)
    errs = {"c1_s2": rel(feats[0][..., ::2, ::2].cpu().numpy(), g["c1_s2"])}
    for i in (2, 3, 4):
        errs["c%d" % i] = rel(feats[i - 1].cpu().numpy(), g["c%d" % i])
    errs["head_s8"] = rel(m.forward_features(xt)[..., ::8, ::8].cpu().numpy(), g["head_s8"])
    errs["planes_s8"] = rel(m(xt)[..., ::8, ::8].cpu().numpy(), g["planes_s8"])
    print("288x256:", errs)
    assert all(e <= TOL for e in errs.values()), errs


def test_batch_of_three_at_a_ragged_non_square_size_equals_single_calls():
    """160 x 96: 15 keys at stage 1, 240 stage-2 tokens per sample (its 64-row tiles straddle samples)."""
    sd = synth.synth_secc_backbone(61)
    m = hip_backbone(sd)
    x = torch.from_numpy(secc_input(62, 3, 9, 160, 96)).to(DEV)
    feats, head = m.forward_stages(x), m.forward_features(x)
    for i in range(3):
        xi = x[i:i + 1].contiguous()
        fi, hi = m.forward_stages(xi), m.forward_features(xi)
        assert all(torch.equal(a[i:i + 1], b) for a, b in zip(feats, fi)), i
        assert torch.equal(head[i:i + 1], hi), i


def test_batch_repeat_and_side_stream_are_bit_identical():
    sd = synth.synth_secc_backbone(21)
    m = hip_backbone(sd)
    x = torch.from_numpy(secc_input(22, 2, 9, 128, 96)).to(DEV)
    both = m.forward_features(x)
    one = torch.cat([m.forward_features(x[:1].contiguous()), m.forward_features(x[1:].contiguous())])
    assert torch.equal(both, one)
    again = m.forward_features(x)
    assert torch.equal(both, again)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s_out = m.forward_features(x)
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(both, s_out)


def test_on_a_device_that_is_not_the_current_one():
    """Module and input on the last visible GPU while the process's current device stays 0 (with one GPU they are the same device): the
    launches go to the input's device and its current stream.  An input on another device than the parameters, or on none, is refused
    before the library is entered."""
    from real3dportrait_amd import _lib
    g, sd, x = golden_case("secc_a_r64")
    last = "cuda:%d" % (torch.cuda.device_count() - 1)
    m = hip_backbone(sd, str(g["mode"])).to(last)
    assert torch.cuda.current_device() == 0
    head = m.forward_features(torch.from_numpy(x).to(last))
    assert str(head.device) == last and torch.cuda.current_device() == 0
    assert rel(head.cpu().numpy(), g["head"]) <= TOL
    with _lib.counting() as calls:
        if last != DEV:
            with pytest.raises(ValueError, match="the module's parameters on"):
                m.forward_features(torch.from_numpy(x).to(DEV))
        for fn in (m.forward_features, m.forward_stages, m):
            with pytest.raises(ValueError, match="not on a GPU"):
                fn(torch.from_numpy(x))
    assert calls == []


def test_launch_list_of_forward_features():
    """embed1; per stage the embedding conv (stages 2-4), two blocks and the stage's LayerNorm, a block being nine launches with
    spatial reduction (stages 1-3) and seven without (stage 4); then the three folded linears and the head: 80."""
    from real3dportrait_amd import _lib
    g, sd, x = golden_case("secc_a_r64")
    m = hip_backbone(sd, str(g["mode"]))
    with _lib.counting() as calls:
        m.forward_features(torch.from_numpy(x).to(DEV))
    tail = ["r3d_secc_attention", "r3d_secc_linear", "r3d_secc_linear", "r3d_secc_dwconv_gelu", "r3d_secc_linear"]
    reduced = ["r3d_secc_layernorm", "r3d_secc_linear", "r3d_secc_conv", "r3d_secc_linear"] + tail
    plain = ["r3d_secc_linear", "r3d_secc_linear"] + tail
    stage = lambda block: block * 2 + ["r3d_secc_layernorm"]
    want = ["r3d_secc_embed1"] + stage(reduced) + (["r3d_secc_conv"] + stage(reduced)) * 2 + ["r3d_secc_conv"] + stage(plain) \
        + ["r3d_secc_linear"] * 3 + ["r3d_secc_head"]
    names = [n for n, _ in calls]
    assert names == want
    assert len(names) == 80 and names.count("r3d_secc_attention") == 8 and "r3d_i2p_attention" not in names


def test_peaked_softmax_has_no_overflow():
    """q weights x 4 on top of synth's gain: the attention logits reach about +-80.  The max-subtracted softmax stays finite; c1 matches
    fp64 within the tolerance, and every later output as closely as an eager fp32 evaluation of the same math does (the cascade of
    peaked softmaxes amplifies fp32 rounding: eager fp32 torch itself is 4e-3 of max|c4| from fp64 here)."""
    sd = synth.synth_secc_backbone(31)
    for k in list(sd):
        if k.endswith("attn.q.weight"):
            sd[k] = sd[k] * np.float32(4.0)
    m = hip_backbone(sd)
    x = torch.from_numpy(secc_input(32, 1, 9, 128, 128)).to(DEV)
    feats = m.forward_stages(x)
    head = m.forward_features(x)
    assert all(bool(torch.isfinite(f).all()) for f in feats) and bool(torch.isfinite(head).all())
    ref = R64.encoder(sd, x.double())
    href = R64.head(sd, ref)
    e32 = R64.encoder(sd, x, torch.float32)
    h32 = R64.head(sd, e32, torch.float32)
    errs = [rel(feats[i].cpu().numpy(), ref[i].cpu().numpy()) for i in range(4)] + [rel(head.cpu().numpy(), href.cpu().numpy())]
    eager = [rel(e32[i].cpu().numpy(), ref[i].cpu().numpy()) for i in range(4)] + [rel(h32.cpu().numpy(), href.cpu().numpy())]
    print("peaked: hip", errs, "eager fp32", eager)
    assert errs[0] <= TOL, errs
    assert all(e <= max(TOL, 3.0 * g) for e, g in zip(errs, eager)), (errs, eager)


def test_forward_raw_with_prepare_planes_equals_flipped_add():
    from real3dportrait_amd import ImportanceRenderer
    sd = synth.synth_secc_backbone(41)
    m = hip_backbone(sd)
    x = torch.from_numpy(secc_input(42, 1, 9, 64, 64)).to(DEV)
    raw = m.forward_raw(x)
    planes = m(x)
    assert planes.shape == (1, 3, 32, 32, 32)
    cano = torch.from_numpy(synth.synth_planes(43, 1, 32, 32, 32)).to(DEV)
    ren = ImportanceRenderer(hp={})
    a = ren.prepare_planes(cano, add=raw, add_flip=53)
    b = ren.prepare_planes(cano + planes)
    assert torch.equal(a, b)
