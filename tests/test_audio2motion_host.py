"""CPU: the host side of the audio-to-motion VAE (real3dportrait_amd/audio2motion.py, include/r3d_hip_audio.h): the
reference's state_dict keys, the parameter folds against torch's own weight_norm / BatchNorm1d in fp64, the latent draw, the binding
table against the header, and what the three entry points refuse before any launch."""
import warnings

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import abi
import audio2motion_ref64 as ref64
from conftest import load_golden
from real3dportrait_amd import _lib, synth
from real3dportrait_amd import audio2motion as a2m

HP = synth.AUDIO2MOTION_HPARAMS


def _model(pitch, sd=None):
    m = a2m.PitchContourVAEModel(HP) if pitch else a2m.VAEModel()
    if sd is not None:
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return m.eval()


@pytest.mark.parametrize("pitch", [True, False])
def test_state_dict_keys_are_the_references_and_load_strictly(pitch):
    recorded = [str(k) for k in load_golden("audio2motion_keys")["pitch" if pitch else "vae"]]
    sd = synth.synth_audio2motion(3, pitch)
    assert sorted(sd) == sorted(recorded) and len(recorded) == (231 if pitch else 220)
    m = _model(pitch, sd)
    back = m.state_dict()
    assert sorted(back) == sorted(recorded)
    for k, v in sd.items():
        assert back[k].shape == np.asarray(v).shape and np.array_equal(back[k].numpy(), v), k
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in back.items() if k != "vae.encoder.out_proj.bias"}, strict=True)
    assert all(k.split(".")[0] != "mouth_amp_embed" for k in recorded) is (not pitch)


def test_unsupported_modes_raise():
    with pytest.raises(NotImplementedError, match="sqz_prior"):
        a2m.VAEModel(sqz_prior=True)
    with pytest.raises(NotImplementedError, match="cond_drop"):
        a2m.PitchContourVAEModel(HP, cond_drop=True)
    with pytest.raises(NotImplementedError, match="use_adapters"):
        a2m.PitchContourVAEModel(dict(HP, use_adapters=True))
    with pytest.raises(NotImplementedError, match="train=True"):
        a2m.VAEModel().forward({}, {}, train=True)


def test_weight_norm_fold_is_torchs_in_fp64():
    sd = synth.synth_audio2motion(5, False)
    m = _model(False, sd)
    for layer in (m.vae.decoder.wn.in_layers[1], m.vae.decoder.wn.cond_layer, m.vae.prior_flow.flows[2].enc.res_skip_layers[3]):
        cout, cin, k = layer.weight_v.shape
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ref = torch.nn.utils.weight_norm(nn.Conv1d(cin, cout, k).double(), name="weight")
        with torch.no_grad():
            ref.weight_g.copy_(layer.weight_g)
            ref.weight_v.copy_(layer.weight_v)
        x = torch.from_numpy(synth.hash_unitvar(6, (1, cin, 9))).double()
        ref(x)                                                        # the hook recomputes .weight
        w = a2m.wn_weight(layer)
        assert w.dtype == torch.float64 and (w - ref.weight).abs().max() <= 1e-14 * ref.weight.abs().max()
        # the gain is not ||v||: a fold without it would be seen
        assert ((layer.weight_g / layer.weight_v.norm(dim=(1, 2), keepdim=True) - 1).abs() > 0.1).all()


def test_batchnorm_fold_is_torchs_in_fp64():
    sd = synth.synth_audio2motion(5, True)
    m = _model(True, sd).double()
    for seq, cin in ((m.mel_encoder, 1024), (m.pitch_encoder, 128)):
        x = torch.from_numpy(synth.hash_unitvar(7, (2, cin, 11))).double()
        with torch.no_grad():
            ref = seq[1](seq[0](x))
        w, b = a2m.fold_conv_bn(seq[0], seq[1])
        got = F.conv1d(x, w, b, padding=1)
        assert (got - ref).abs().max() <= 1e-12 * ref.abs().max()
        assert (ref - seq[0](x)).abs().max() > 0.1                    # the BatchNorm does something
        f = a2m.fold_encoder(seq, torch.float64)
        assert f["w0"].shape == (seq[0].out_channels, 3, cin) and torch.equal(f["w0"], w.permute(0, 2, 1))


def test_wn_layer_and_flow_folds_state_the_reference_in_fp64():
    """fold_wn's [k H + Cg, 2 H] rows and the summed bias give the reference's gate pre-activations; fold_flow's column-reversed pre is
    pre on the flipped state; the transposed conv's k = 1 view and the cond_proj table and vector are the reference's terms."""
    sd = synth.synth_audio2motion(5, True)
    m = _model(True, sd)
    sd64 = {k: torch.from_numpy(np.asarray(v)).double() for k, v in sd.items() if np.asarray(v).dtype != np.int64}
    B, T, H, Cg, k = 2, 7, 256, 128, 5
    x = torch.from_numpy(synth.hash_unitvar(8, (B, T, H))).double()
    g = torch.from_numpy(synth.hash_unitvar(9, (B, T, Cg))).double()
    taps = {}
    ref64._wn(sd64, "vae.decoder.wn", x.transpose(1, 2), g.transpose(1, 2), set(), taps, "dec")
    layer = a2m.fold_wn(m.vae.decoder.wn, torch.float64)[0]
    xp = F.pad(x, (0, 0, k // 2, k // 2))
    a = torch.cat([xp[:, j:j + T] for j in range(k)] + [g], -1) @ layer["w_in"] + layer["b_in"]
    ref = taps["vae.decoder.wn.gate0"].transpose(1, 2)
    assert (a - ref).abs().max() <= 1e-12 * ref.abs().max()
    rs = (torch.tanh(a[..., :H]) * torch.sigmoid(a[..., H:])) @ layer["w_rs"] + layer["b_rs"]
    assert ((x + rs[..., :H]) - taps["dec_x0"]).abs().max() <= 1e-12 and (rs[..., H:] - taps["dec_out0"]).abs().max() <= 1e-12
    assert a2m.fold_wn(m.vae.decoder.wn)[3]["w_rs"].shape == (H, H)

    z = torch.from_numpy(synth.hash_unitvar(10, (B, T, 16))).double()
    fl = m.vae.prior_flow.flows[6]
    want = F.conv1d(z.flip(2)[..., :8].transpose(1, 2), fl.pre.weight.double(), fl.pre.bias.double()).transpose(1, 2)
    f = a2m.fold_flow(fl, True, torch.float64)
    assert ((z[..., 8:] @ f["pre_w"][:, 0].t() + f["pre_b"]) - want).abs().max() <= 1e-12
    assert [d["flipped"] for d in a2m.fold_vae(m.vae)["flows"]] == [True, False, True, False]

    F_ = a2m.fold_vae(m.vae, torch.float64)
    zq = z.transpose(1, 2)
    up = m.vae.decoder.pre_net[0]
    want = F.conv_transpose1d(zq, up.weight.double(), up.bias.double(), stride=4).transpose(1, 2)
    got = (z @ F_["up_w"][:, 0].t() + F_["up_b"]).reshape(B, 4 * T, 256)
    assert (got - want).abs().max() <= 1e-12

    P = a2m.fold_cond_proj(m, torch.float64)
    f_ = 128
    cat = torch.from_numpy(synth.hash_unitvar(11, (B, T, 2 * f_))).double()
    blink = torch.tensor([[0, 1, 1, 0, 0, 1, 0], [1, 0, 0, 0, 1, 1, 1]])
    amp = torch.tensor([[0.3], [0.7]]).double()
    full = torch.cat([cat, m.blink_embed.weight.double()[blink], (amp.unsqueeze(1) * m.mouth_amp_embed.double()).repeat(1, T, 1)], -1)
    want = F.linear(full, m.cond_proj.weight.double(), m.cond_proj.bias.double())
    got = cat @ P["w"][:, 0].t() + P["b"] + P["table"][blink] + amp.unsqueeze(1) * P["mouth"]
    assert (got - want).abs().max() <= 1e-12 and P["eye"] is None


def test_folds_follow_the_staleness_rule():
    m = _model(False, synth.synth_audio2motion(5, False))
    F1 = m._prepare()
    assert m._prepare() is F1
    with torch.no_grad():
        m.vae.decoder.out_proj.bias.add_(1.0)
    F2 = m._prepare()
    assert F2 is not F1 and torch.equal(F2["vae"]["out_b"], F1["vae"]["out_b"] + 1.0)


def test_latent_draw_is_the_references_call():
    for name in ("audio2motion_pitch_b2", "audio2motion_vae_t20"):
        g = load_golden(name)
        _, B, T = (int(v) for v in g["shape"])
        torch.manual_seed(int(g["seeds"][2]))
        z = a2m.draw_latent(B, T // 4)
        torch.manual_seed(int(g["seeds"][2]))
        ref = torch.distributions.Normal(0, 1).sample([B, 16, T // 4])          # FVAE.forward, vae.py:191,243-244
        assert z.dtype == torch.float32 and torch.equal(z, ref) and np.array_equal(z.numpy(), g["z_p"])


def test_patch_leaves_other_models_alone():
    class Infer:
        pass
    infer = Infer()
    infer.audio2secc_model = nn.Linear(2, 2)          # stands for the ICL model
    assert a2m.patch_audio2secc(infer) is False and isinstance(infer.audio2secc_model, nn.Linear) and not hasattr(infer, "_r3d_reference_audio2secc_model")
    infer.audio2secc_model = _model(False)            # a module of this package: already replaced
    assert a2m.patch_audio2secc(infer) is False


def test_header_mirrors_the_audio_table():
    """The three entry points live in the companion header include/r3d_hip_audio.h (tests/test_abi.py compares every declaration with the
    binding table and with what load() bound, and the header's macro with the package's constant); here what is this unit's own: the
    names, the parameter counts, the ABI number and the rows of a block against the module that sizes its launches by them."""
    lib = _lib.load()
    assert lib.r3d_version() == _lib.ABI_VERSION
    decls = abi.header_declarations("r3d_hip_audio.h")
    assert {name: len(types) for name, (ret, types) in decls.items()} == {"r3d_a2m_conv1d": 29, "r3d_a2m_wn_layer": 17, "r3d_a2m_pitch_embed": 9}
    assert set(decls) <= set(_lib.SIGNATURES)
    assert a2m.WN_ROWS == _lib.A2M_WN_ROWS == 16


def test_argument_errors_are_refused_before_any_launch():
    """Every call has exactly one defect; the pointers are fake, 1 TiB apart and never dereferenced (a valid call would launch:
    tests/test_gpu_audio2motion_ops.py runs those)."""
    lib = _lib.load()
    X, W, BIAS, Y, MASK, TAB, IDX, AMP, U, G, XN, OUT = (i << 40 for i in range(1, 13))
    conv = dict(x=X, B=1, Tin=8, Cin=16, xs=16, xo=0, mode=0, w=W, bias=BIAS, Cout=8, k=3, stride=1, pad=1, gelu=0, mask=None, table=None, idx=None,
                rows=0, step=1, amp0=None, u0=None, amp1=None, u1=None, sub=None, y=Y, ys=8, yo=0, flip=0)
    wn = dict(x=X, g=G, B=1, T=8, H=64, Cg=128, k=3, w_in=W, b_in=BIAS, w_rs=TAB, b_rs=U, mask=None, first=1, last=0, xn=XN, out=OUT)
    pitch = dict(f0=X, B=1, T=8, table=TAB, rows=300, C=128, index=IDX, y=Y)
    refused = abi.refusals(lib, "r3d_a2m_")

    for p in ("x", "w", "y"):
        refused("conv1d", conv, b"NULL pointer", **{p: None})
    refused("conv1d", conv, b"table and idx go together", table=TAB, rows=2)
    refused("conv1d", conv, b"amp and u go together", amp0=AMP)
    refused("conv1d", conv, b"amp and u go together", u1=U)
    for p in ("B", "Tin", "Cin", "Cout"):
        refused("conv1d", conv, b"must be positive", **{p: 0})
    refused("conv1d", conv, b"exceeds 65535", B=65536)
    refused("conv1d", conv, b"k = 9", k=9, pad=0)
    refused("conv1d", conv, b"k = 0", k=0, pad=0)
    refused("conv1d", conv, b"stride = 0", stride=0)
    refused("conv1d", conv, b"pad = 3", pad=3)
    refused("conv1d", conv, b"pad = -1", pad=-1)
    refused("conv1d", conv, b"row_mode = 3", mode=3)
    refused("conv1d", conv, b"shorter than k", Tin=1, k=8, pad=2)
    refused("conv1d", conv, b"outside a row of x_stride", xo=1)
    refused("conv1d", conv, b"outside a row of y_stride", ys=15, yo=8)
    refused("conv1d", conv, b"table_rows = 0", table=TAB, idx=IDX)
    refused("conv1d", conv, b"idx_step = 3", table=TAB, idx=IDX, rows=2, step=3)
    refused("conv1d", conv, b"2^31", B=4096, Tin=1 << 15, xs=16)
    refused("conv1d", conv, b"2^31", Tin=1 << 20, ys=4096, yo=0)
    refused("conv1d", conv, b"overlaps", y=X)
    refused("conv1d", conv, b"overlaps", y=X + 4 * 100)                # inside x [1, 8, 16]
    refused("conv1d", conv, b"overlaps", sub=Y + 4)                    # subtract_from: y itself or disjoint
    refused("conv1d", conv, b"overlaps", mask=Y)

    for p in ("x", "g", "w_in", "b_in", "w_rs", "b_rs", "out"):
        refused("wn_layer", wn, b"NULL pointer", **{p: None})
    refused("wn_layer", wn, b"x_next is written by every layer but the last", xn=None)
    refused("wn_layer", wn, b"the last layer writes no x_next", last=1)
    refused("wn_layer", wn, b"must be positive", T=0)
    refused("wn_layer", wn, b"must be positive", B=0)
    refused("wn_layer", wn, b"H = 128 is not supported", H=128)
    for k in (0, 2, 4, 7):
        refused("wn_layer", wn, b"is not supported (1, 3 or 5)", k=k)
    for cg in (0, 6, 260):
        refused("wn_layer", wn, b"Cg = %d must be" % cg, Cg=cg)
    refused("wn_layer", wn, b"2^31", B=4096, T=1 << 14, H=256)
    refused("wn_layer", wn, b"overlaps", xn=X)
    refused("wn_layer", wn, b"overlaps", out=X + 4)
    refused("wn_layer", wn, b"overlaps", out=XN)
    refused("wn_layer", wn, b"overlaps", out=G)

    for p in ("f0", "table", "index", "y"):
        refused("pitch_embed", pitch, b"NULL pointer", **{p: None})
    for p in ("B", "T", "rows", "C"):
        refused("pitch_embed", pitch, b"must be positive", **{p: 0})
    refused("pitch_embed", pitch, b"2^31", B=1 << 12, T=1 << 12, C=128)
    refused("pitch_embed", pitch, b"overlaps", y=X)
    refused("pitch_embed", pitch, b"overlaps", index=Y)
    # the typed call path raises what the library refuses
    with pytest.raises(RuntimeError, match="a2m_wn_layer: H = 32 is not supported"):
        _lib.call("r3d_a2m_wn_layer", X, G, 1, 8, 32, 128, 3, W, BIAS, TAB, U, None, 1, 0, XN, OUT, None)
