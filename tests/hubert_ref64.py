"""transformers.HubertModel with the large model's structure (layer-norm feature extractor, stable layer norm), restated in plain torch ops
from the model's definition, in any dtype: the fp64 reference of the HuBERT tests, the float32 eager side of scripts/prof_hubert.py, and
get_hubert_from_16k_speech (data_gen/utils/process_audio/extract_hubert.py:18-80) around it.  Each op of include/r3d_hip_hubert.h has its
own function here.  Imported by tests; it holds none and imports neither transformers nor the package's hubert module."""
import math

import torch
import torch.nn.functional as F


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def layer_norm(x, w, b, eps):
    mu = x.mean(dim=-1, keepdim=True)
    var = (x - mu).pow(2).mean(dim=-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


def wave_stats(wave):
    """(mean, 1 / sqrt(population variance + 1e-7)) of a 1-D waveform, in its dtype."""
    mean = wave.mean()
    return mean, 1.0 / torch.sqrt((wave - mean).pow(2).mean() + 1e-7)


def conv_ln_gelu(x, w, bias, g, b, eps, stride):
    """x [B, Tin, Cin], w [Cout, Cin, k] (the parameter as stored) -> [B, Tout, Cout]: Conv1d, LayerNorm over channels, GELU."""
    y = F.conv1d(x.transpose(1, 2), w, bias, stride=stride).transpose(1, 2)
    return gelu(layer_norm(y, g, b, eps))


def pos_weight(g, v):
    """weight_norm(dim=2): v g / ||v||, the norm over dims 0 and 1."""
    return v * (g / v.pow(2).sum(dim=(0, 1), keepdim=True).sqrt())


def pos_conv(x, w, bias, groups):
    """x [B, T, C], w [C, C / groups, k] the effective weight -> x + gelu(conv(x)), the last output dropped for an even k."""
    k = w.shape[2]
    y = F.conv1d(x.transpose(1, 2), w, bias, padding=k // 2, groups=groups)
    if k % 2 == 0:
        y = y[:, :, :-1]
    return x + gelu(y.transpose(1, 2))


def attention(q, k, v, heads, stats=None):
    B, T, C = q.shape
    D = C // heads
    split = lambda t: t.view(B, T, heads, D).transpose(1, 2)
    p = torch.softmax(split(q) @ split(k).transpose(2, 3) * D ** -0.5, dim=-1)
    if stats is not None:
        stats.append((T, float(p.max(dim=-1).values.median())))
    return (p @ split(v)).transpose(1, 2).reshape(B, T, C)


def forward(sd, cfg, x, dtype=torch.float64, stats=None):
    """sd: a state_dict of HubertModel (tensors), cfg: the widths (synth.HUBERT_LARGE's fields), x [B, n] normalised input ->
    (last_hidden_state [B, T, hidden], taps).  stats collects (keys, median over rows of the largest softmax probability) per attention."""
    p = {k: v.to(dtype) for k, v in sd.items()}
    x = x.to(dtype)
    eps = cfg["layer_norm_eps"]
    h = x[:, :, None]
    for i, s in enumerate(cfg["conv_stride"]):
        q = "feature_extractor.conv_layers.%d." % i
        h = conv_ln_gelu(h, p[q + "conv.weight"], p[q + "conv.bias"], p[q + "layer_norm.weight"], p[q + "layer_norm.bias"], 1e-5, s)
    taps = {"extract_features": h}
    h = layer_norm(h, p["feature_projection.layer_norm.weight"], p["feature_projection.layer_norm.bias"], eps)
    h = h @ p["feature_projection.projection.weight"].t() + p["feature_projection.projection.bias"]
    taps["projected"] = h
    q = "encoder.pos_conv_embed.conv."
    h = pos_conv(h, pos_weight(p[q + "parametrizations.weight.original0"], p[q + "parametrizations.weight.original1"]), p[q + "bias"],
                 cfg["num_conv_pos_embedding_groups"])
    taps["pos_conv"] = h
    lin = lambda t, name: t @ p[name + ".weight"].t() + p[name + ".bias"]
    for i in range(cfg["num_hidden_layers"]):
        q = "encoder.layers.%d." % i
        n = layer_norm(h, p[q + "layer_norm.weight"], p[q + "layer_norm.bias"], eps)
        a = attention(lin(n, q + "attention.q_proj"), lin(n, q + "attention.k_proj"), lin(n, q + "attention.v_proj"), cfg["num_attention_heads"], stats)
        h = h + lin(a, q + "attention.out_proj")
        n = layer_norm(h, p[q + "final_layer_norm.weight"], p[q + "final_layer_norm.bias"], eps)
        h = h + lin(gelu(lin(n, q + "feed_forward.intermediate_dense")), q + "feed_forward.output_dense")
        if i == 0:
            taps["layer0"] = h
    return layer_norm(h, p["encoder.layer_norm.weight"], p["encoder.layer_norm.bias"], eps), taps


def features(sd, cfg, wave, plan, dtype=torch.float64, stats=None):
    """get_hubert_from_16k_speech: wave [n] (fp32 samples) normalised by its own statistics in `dtype`, the model on every (start, end) of
    `plan`, concatenated and cut to (n - 80) // 320 frames.  -> ([T, hidden], the taps of the first chunk)."""
    w = wave.to(dtype)
    mean, rstd = wave_stats(w)
    xn = (w - mean) * rstd
    outs, taps = [], None
    for s, e in plan:
        y, t = forward(sd, cfg, xn[None, s:e], dtype, stats)
        outs.append(y[0])
        taps = taps or t
    return torch.cat(outs, dim=0)[:(wave.numel() - 80) // 320], taps
