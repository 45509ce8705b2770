"""A plain-torch restatement of the audio-to-motion VAE's inference path (modules/audio2motion/vae.py:272-454 with FVAE.forward(infer=True),
:243-269, ResidualCouplingBlock reverse, flow_base.py:696-703, and WN.forward, :70-96) from a state_dict, for both models.

    forward(sd, batch, z_p, pitch, hparams, dtype)  ->  x_recon [B, T, C]

dtype float64 is the truth the tests compare with; float32 on a GPU is the eager baseline scripts/prof_audio2motion.py times.  `taps`, a
dict, receives the intermediates: cond_feat [B, T, F], g_sqz [B, T / 4, F], z_flow<i> [B, T / 4, 16] (the state after coupling layer i,
before the Flip that follows it in reversed(flows)), dec_in [B, T, 256], every WN layer's x and out (dec_x<l> / dec_out<l> [B, T, 256] of
the decoder's WN, flow<i>_x<l> / flow<i>_out<l> [B, T / 4, 64] of coupling layer i's), every WN's gate pre-activations
'<prefix>.gate<l>' and, for the pitch model, pitch_index [B, T] and f0_mel [B, T] (the value that is truncated).
`drop`, a set, switches pieces OFF so that the golden script can show that each one matters:
    ('flow', i)              coupling layer i is skipped (its Flip stays)
    ('cond', prefix, l)      layer l of the WN at `prefix` gets no condition term
    'gain'                   weight norm without its gain: w = v
    'bn'                     the BatchNorms are skipped
    'flip'                   no Flip
"""
import math

import torch
import torch.nn.functional as F

LATENT, N_FLOWS = 16, 4
F0_MEL_MIN = 1127 * math.log(1 + 50.0 / 700)
F0_MEL_MAX = 1127 * math.log(1 + 1100.0 / 700)


def _wn_weight(sd, name, drop):
    v = sd[name + ".weight_v"]
    if "gain" in drop:
        return v
    return sd[name + ".weight_g"] * v / v.norm(dim=(1, 2), keepdim=True)


def _wn(sd, prefix, x, g, drop, taps, tap_name=None):
    """WN.forward with x_mask = 1; x [B, H, T], g [B, Cg, T]."""
    H = x.shape[1]
    n = sum(1 for k in sd if k.startswith(prefix + ".in_layers.") and k.endswith(".weight_v"))
    gc = F.conv1d(g, _wn_weight(sd, prefix + ".cond_layer", drop), sd[prefix + ".cond_layer.bias"])
    out = torch.zeros_like(x)
    for i in range(n):
        w = _wn_weight(sd, "%s.in_layers.%d" % (prefix, i), drop)
        a = F.conv1d(x, w, sd["%s.in_layers.%d.bias" % (prefix, i)], padding=w.shape[2] // 2)
        if ("cond", prefix, i) not in drop:
            a = a + gc[:, 2 * H * i:2 * H * (i + 1)]
        if taps is not None:
            taps["%s.gate%d" % (prefix, i)] = a
        acts = torch.tanh(a[:, :H]) * torch.sigmoid(a[:, H:])
        rs = F.conv1d(acts, _wn_weight(sd, "%s.res_skip_layers.%d" % (prefix, i), drop), sd["%s.res_skip_layers.%d.bias" % (prefix, i)])
        if i < n - 1:
            x = x + rs[:, :H]
            out = out + rs[:, H:]
        else:
            out = out + rs
        if taps is not None and tap_name:
            taps["%s_out%d" % (tap_name, i)] = out.transpose(1, 2)
            if i < n - 1:
                taps["%s_x%d" % (tap_name, i)] = x.transpose(1, 2)
    return out


def _encoder(sd, prefix, x, drop):
    """Conv1d(k 3, no bias), BatchNorm1d (eval), GELU (erf), Conv1d(k 3, no bias); x [B, C, T]."""
    h = F.conv1d(x, sd[prefix + ".0.weight"], None, padding=1)
    if "bn" not in drop:
        h = F.batch_norm(h, sd[prefix + ".1.running_mean"], sd[prefix + ".1.running_var"], sd[prefix + ".1.weight"], sd[prefix + ".1.bias"], False, 0.0,
                         1e-5)
    return F.conv1d(F.gelu(h), sd[prefix + ".3.weight"], None, padding=1)


def f0_to_coarse(f0):
    """utils/commons/pitch_utils.py:17-26 in f0's dtype (torch rounds the fp64 scalars to it); also returns the value that is truncated."""
    m = 1127 * (1 + f0 / 700).log()
    pos = m > 0
    m = torch.where(pos, (m - F0_MEL_MIN) * 254 / (F0_MEL_MAX - F0_MEL_MIN) + 1, m)
    m = torch.where(m <= 1, torch.ones_like(m), m)
    m = torch.where(m > 255, torch.full_like(m, 255), m)
    return (m + 0.5).long(), m + 0.5


def _vae(sd, g, z_p, temperature, drop, taps):
    """FVAE.forward(infer=True): g [B, Cg, T] -> [B, C, T]."""
    g_sqz = F.conv1d(g, sd["vae.g_pre_net.0.weight"], sd["vae.g_pre_net.0.bias"], stride=4, padding=2)
    z = z_p.to(g) * temperature
    if "vae.prior_flow.flows.0.pre.weight" in sd:
        for i in reversed(range(N_FLOWS)):
            if "flip" not in drop:
                z = z.flip(1)
            if ("flow", i) not in drop:
                p = "vae.prior_flow.flows.%d" % (2 * i)
                x0, x1 = z[:, :LATENT // 2], z[:, LATENT // 2:]
                h = F.conv1d(x0, sd[p + ".pre.weight"], sd[p + ".pre.bias"])
                h = _wn(sd, p + ".enc", h, g_sqz, drop, taps, "flow%d" % i)
                z = torch.cat([x0, x1 - F.conv1d(h, sd[p + ".post.weight"], sd[p + ".post.bias"])], 1)
            if taps is not None:
                taps["z_flow%d" % i] = z.transpose(1, 2)
    x = F.conv_transpose1d(z, sd["vae.decoder.pre_net.0.weight"], sd["vae.decoder.pre_net.0.bias"], stride=4)
    if taps is not None:
        taps.update(g_sqz=g_sqz.transpose(1, 2), dec_in=x.transpose(1, 2))
    x = _wn(sd, "vae.decoder.wn", x, g, drop, taps, "dec")
    return F.conv1d(x, sd["vae.decoder.out_proj.weight"], sd["vae.decoder.out_proj.bias"])


def forward(sd, batch, z_p, pitch=True, hparams=None, dtype=torch.float64, temperature=1.0, drop=(), taps=None):
    """sd: the reference's state_dict (tensors or arrays); batch: y_mask [B, T], audio [B, 2 T, Cin], and for the pitch model f0 [B, 2 T],
    optional blink [B, 2 T, 1], mouth_amp / eye_amp [B, 1]; z_p [B, 16, T / 4], the draw before the temperature.  Runs on y_mask's device."""
    hparams, drop = hparams or {}, set(drop)
    mask = torch.as_tensor(batch["y_mask"])
    dev = mask.device
    t = lambda v: torch.as_tensor(v).to(device=dev)
    sd = {k: t(v).to(dtype) if torch.as_tensor(v).is_floating_point() else t(v) for k, v in sd.items()}
    mask, mel = mask.to(dtype), t(batch["audio"]).to(dtype)
    if not pitch:
        mel = F.interpolate(mel.transpose(1, 2), scale_factor=0.5, mode="linear")
        g = _encoder(sd, "mel_encoder", mel, drop)
    else:
        f0 = t(batch["f0"]).to(dtype)
        B = f0.shape[0]
        blink = t(batch["blink"]).long() if "blink" in batch else torch.zeros(B, f0.shape[1], 1, dtype=torch.long, device=dev)
        down = lambda x: F.interpolate(x.transpose(1, 2), scale_factor=0.5, mode="nearest").transpose(1, 2)
        blink_feat = down(sd["blink_embed.weight"][blink.squeeze(2)])
        mel = down(mel)
        index, f0_mel = f0_to_coarse(down(f0.unsqueeze(-1)).squeeze(-1))
        cond = _encoder(sd, "mel_encoder", mel.transpose(1, 2), drop).transpose(1, 2)
        pit = _encoder(sd, "pitch_encoder", sd["pitch_embed.weight"][index].transpose(1, 2), drop).transpose(1, 2)
        feats = [cond, pit, blink_feat]
        for key in ("mouth", "eye"):
            if hparams.get("use_%s_amp_embed" % key, False):
                amp = t(batch[key + "_amp"]).to(dtype) if key + "_amp" in batch else torch.full([B, 1], 0.4, dtype=dtype, device=dev)
                feats.append((amp.unsqueeze(1) * sd[key + "_amp_embed"].unsqueeze(0)).repeat([1, cond.shape[1], 1]))
        g = F.linear(torch.cat(feats, -1), sd["cond_proj.weight"], sd["cond_proj.bias"]).transpose(1, 2)
        if taps is not None:
            taps.update(pitch_index=index, f0_mel=f0_mel)
    if taps is not None:
        taps["cond_feat"] = g.transpose(1, 2)
    x = _vae(sd, g, t(z_p), temperature, drop, taps).transpose(1, 2)
    return x * mask.unsqueeze(-1)
