"""The HuBERT audio features of GeneFace2Infer.get_hubert (inference/real3d_infer.py:323-334 -> get_hubert_from_16k_speech,
data_gen/utils/process_audio/extract_hubert.py:18-80 -> transformers.HubertModel of facebook/hubert-large-ls960-ft) on the HIP library, in
exact fp32 (include/r3d_hip_hubert.h).  This module does not import transformers.

    HubertFeatureModel(config)     the model: state_dict keys of transformers.HubertModel, forward(input_values [B, n]) -> [B, T, hidden]
    chunk_plan(n, clip_frames)     the reference's (start, end) sample ranges of a clip of n samples
    hubert_features(model, speech) get_hubert_from_16k_speech: [expected_T, hidden] on the device
    get_hubert(model, wav)         GeneFace2Infer.get_hubert: the [T8, hidden] NumPy array, rows zero-padded to a multiple of 8
    patch_hubert(infer, model)     binds infer.get_hubert

Only the large model's structure is built (layer-norm feature extractor, stable layer norm, GELU); INFERENCE ONLY.
"""
import numpy as np
import torch
import torch.nn as nn

from . import _lib
from ._state import _FoldedModule
from .synth import HUBERT_LARGE
from .token_blocks import attention_half

KERNEL, STRIDE = 400, 320          # the conv stack as one Conv1d (extract_hubert.py:48-49): 400 samples a frame, a frame every 320
# the structure this module builds: field -> the value it must have (a config that lacks the field is taken to have it)
STRUCTURE = {"feat_extract_norm": "layer", "do_stable_layer_norm": True, "feat_proj_layer_norm": True, "conv_bias": True,
             "hidden_act": "gelu", "feat_extract_activation": "gelu", "conv_pos_batch_norm": False}


def _read_config(config):
    get = (lambda k, d: config.get(k, d)) if isinstance(config, dict) else (lambda k, d: getattr(config, k, d))
    if config is None:
        get = lambda k, d: d
    for field, want in STRUCTURE.items():
        if get(field, want) != want:
            raise NotImplementedError("HubertFeatureModel: %s = %r is not built (only %r, the structure of hubert-large-ls960-ft)"
                                      % (field, get(field, want), want))
    c = {k: get(k, v) for k, v in HUBERT_LARGE.items()}
    for k in ("conv_dim", "conv_kernel", "conv_stride"):
        c[k] = tuple(int(v) for v in c[k])
    if not (len(c["conv_dim"]) == len(c["conv_kernel"]) == len(c["conv_stride"]) >= 1):
        raise ValueError("HubertFeatureModel: conv_dim, conv_kernel and conv_stride differ in length")
    if c["hidden_size"] % c["num_attention_heads"] or c["hidden_size"] % c["num_conv_pos_embedding_groups"]:
        raise ValueError("HubertFeatureModel: hidden_size is not a multiple of num_attention_heads and num_conv_pos_embedding_groups")
    c["masked_spec_embed"] = get("mask_time_prob", 0.05) > 0.0 or get("mask_feature_prob", 0.0) > 0.0          # HubertModel.__init__
    return c


class _Holder(nn.Module):
    pass


class _ConvLayer(nn.Module):
    def __init__(self, cin, cout, k, stride):
        super().__init__()
        self.conv = nn.Conv1d(cin, cout, k, stride)
        self.layer_norm = nn.LayerNorm(cout)          # (HubertLayerNormConvLayer: the default eps, not the config's)


class _PosConv(nn.Module):
    """conv.bias and conv.parametrizations.weight.original0 (g [1, 1, k]) / original1 (v [C, C / groups, k]): weight_norm(dim=2)."""

    def __init__(self, C, k, groups):
        super().__init__()
        self.conv = _Holder()
        self.conv.bias = nn.Parameter(torch.zeros(C))
        self.conv.parametrizations = _Holder()
        self.conv.parametrizations.weight = _Holder()
        self.conv.parametrizations.weight.original0 = nn.Parameter(torch.ones(1, 1, k))
        self.conv.parametrizations.weight.original1 = nn.Parameter(torch.zeros(C, C // groups, k))


class _EncoderLayer(nn.Module):
    def __init__(self, H, I, eps):
        super().__init__()
        self.attention = _Holder()
        for n in ("k_proj", "v_proj", "q_proj", "out_proj"):
            setattr(self.attention, n, nn.Linear(H, H))
        self.layer_norm = nn.LayerNorm(H, eps=eps)
        self.feed_forward = _Holder()
        self.feed_forward.intermediate_dense, self.feed_forward.output_dense = nn.Linear(H, I), nn.Linear(I, H)
        self.final_layer_norm = nn.LayerNorm(H, eps=eps)


def effective_pos_weight(g, v):
    """The weight of weight_norm(conv, dim=2): v g / ||v|| with the norm over dims 0 and 1 (torch._weight_norm(v, g, 2)), formed in fp64 and
    rounded once."""
    v64 = v.detach().double()
    return (v64 * (g.detach().double() / v64.pow(2).sum(dim=(0, 1), keepdim=True).sqrt())).float()


def conv1d_weight_cl(w):
    """[Cout, Cin, k] -> [Cout, k, Cin], what r3d_hubert_conv_ln_gelu and r3d_hubert_pos_conv read."""
    return w.detach().permute(0, 2, 1).contiguous().float()


def chunk_plan(n, clip_frames=1000):
    """The (start, end) sample ranges get_hubert_from_16k_speech runs the model on (extract_hubert.py:50-71): n // (320 clip_frames) full
    chunks at 320 clip_frames i of 320 clip_frames + 80 samples (end clipped to n, as the reference's slice is), then the tail from
    320 clip_frames num_iter where it has at least 400 samples."""
    clip = STRIDE * clip_frames
    num = n // clip
    plan = [(clip * i, min(clip * i + clip - STRIDE + KERNEL, n)) for i in range(num)]
    if n - clip * num >= KERNEL:
        plan.append((clip * num, n))
    return plan


class HubertFeatureModel(_FoldedModule):
    def __init__(self, config=None):
        super().__init__()
        c = self.config = _read_config(config)
        H, I, eps = c["hidden_size"], c["intermediate_size"], c["layer_norm_eps"]
        if c["masked_spec_embed"]:
            self.masked_spec_embed = nn.Parameter(torch.zeros(H))          # never read: masking is a training-time step
        self.feature_extractor = _Holder()
        dims = (1,) + c["conv_dim"]
        self.feature_extractor.conv_layers = nn.ModuleList(
            _ConvLayer(dims[i], dims[i + 1], c["conv_kernel"][i], c["conv_stride"][i]) for i in range(len(c["conv_dim"])))
        self.feature_projection = _Holder()
        self.feature_projection.layer_norm = nn.LayerNorm(dims[-1], eps=eps)
        self.feature_projection.projection = nn.Linear(dims[-1], H)
        self.encoder = _Holder()
        self.encoder.pos_conv_embed = _PosConv(H, c["num_conv_pos_embeddings"], c["num_conv_pos_embedding_groups"])
        self.encoder.layer_norm = nn.LayerNorm(H, eps=eps)
        self.encoder.layers = nn.ModuleList(_EncoderLayer(H, I, eps) for _ in range(c["num_hidden_layers"]))
        self.eval()

    def load_state_dict(self, state_dict, strict=True, **kw):
        """Also accepts the legacy pair encoder.pos_conv_embed.conv.weight_g / weight_v of the published checkpoint file."""
        p = "encoder.pos_conv_embed.conv."
        if p + "weight_g" in state_dict or p + "weight_v" in state_dict:
            state_dict = dict(state_dict)
            for old, new in (("weight_g", "parametrizations.weight.original0"), ("weight_v", "parametrizations.weight.original1")):
                if p + old in state_dict:
                    state_dict[p + new] = state_dict.pop(p + old)
        return super().load_state_dict(state_dict, strict=strict, **kw)

    @classmethod
    def from_reference(cls, ref):
        """A HIP copy of a constructed transformers.HubertModel: its config, its parameters (strict), its device."""
        m = cls(ref.config)
        m.load_state_dict(ref.state_dict(), strict=True)
        return m.to(next(ref.parameters()).device).eval()

    # ---- parameters in the kernels' layouts (_prepare: once per parameter version) -------------------------------------------------
    def _fold(self):
        d = {}
        layers = self.feature_extractor.conv_layers
        d["conv0"] = layers[0].conv.weight.detach().reshape(layers[0].conv.out_channels, -1).contiguous().float()
        for i in range(1, len(layers)):
            d["conv%d" % i] = conv1d_weight_cl(layers[i].conv.weight)
        pw = self.encoder.pos_conv_embed.conv.parametrizations.weight
        d["pos"] = conv1d_weight_cl(effective_pos_weight(pw.original0, pw.original1))
        for i, layer in enumerate(self.encoder.layers):
            a = layer.attention
            d["kv_w%d" % i] = torch.cat([a.k_proj.weight.detach(), a.v_proj.weight.detach()], dim=0).contiguous().float()
            d["kv_b%d" % i] = torch.cat([a.k_proj.bias.detach(), a.v_proj.bias.detach()], dim=0).contiguous().float()
        d["unit_stats"] = torch.tensor([0.0, 1.0], dtype=torch.float64, device=d["conv0"].device)          # forward(): input already normalised
        return d

    def frames(self, n):
        """Frames of a sequence of n samples (None when a layer has fewer inputs than its kernel), and every layer's length."""
        lens = []
        for k, s in zip(self.config["conv_kernel"], self.config["conv_stride"]):
            if n < k:
                return None, lens
            n = (n - k) // s + 1
            lens.append(n)
        return n, lens

    def _new_buffers(self, dev, B, n):
        c = self.config
        T, lens = self.frames(n)
        e = lambda m: torch.empty(m, device=dev, dtype=torch.float32)
        conv = max(B * t * cd for t, cd in zip(lens, c["conv_dim"]))
        tok = B * T
        return {"a": e(conv), "b": e(conv), "x": e(tok * c["hidden_size"]), "p": e(tok * c["hidden_size"]), "q": e(tok * c["hidden_size"]),
                "o": e(tok * c["hidden_size"]), "kv": e(tok * 2 * c["hidden_size"]), "h": e(tok * c["intermediate_size"])}

    # ---- the launches: B sequences of n samples at wave + offset + b stride ------------------------------------------------------------
    def _run(self, wave, stats, B, offset, stride, n, taps=None):
        with self._device_of(wave):
            return self._launches(wave, stats, B, offset, stride, n, taps)

    def _launches(self, wave, stats, B, offset, stride, n, taps):
        c = self.config
        T, lens = self.frames(n)
        if T is None:
            raise ValueError("HubertFeatureModel: %d samples are fewer than one frame needs" % n)
        H, I, heads = c["hidden_size"], c["intermediate_size"], c["num_attention_heads"]
        st = torch.cuda.current_stream().cuda_stream
        d = self._prepare()
        w = self._buffers_for(wave.device, B, n)
        stats = d["unit_stats"] if stats is None else stats
        tap = (lambda name, t, shape: taps.__setitem__(name, t[:shape[0] * shape[1] * shape[2]].view(shape).clone())) if taps is not None \
            else (lambda *a: None)
        layers = self.feature_extractor.conv_layers
        l0 = layers[0]
        cur, nxt = w["a"], w["b"]
        _lib.call("r3d_hubert_conv0", wave, stats, B, offset, stride, n, d["conv0"], l0.conv.bias, l0.layer_norm.weight, l0.layer_norm.bias,
                  l0.layer_norm.eps, c["conv_dim"][0], c["conv_kernel"][0], c["conv_stride"][0], cur, st)
        for i in range(1, len(layers)):
            li = layers[i]
            _lib.call("r3d_hubert_conv_ln_gelu", cur, d["conv%d" % i], li.conv.bias, li.layer_norm.weight, li.layer_norm.bias, li.layer_norm.eps, B,
                      lens[i - 1], c["conv_dim"][i - 1], c["conv_dim"][i], c["conv_kernel"][i], c["conv_stride"][i], nxt, st)
            cur, nxt = nxt, cur
        tap("extract_features", cur, (B, T, c["conv_dim"][-1]))
        M = B * T
        X, P, Hb = w["x"], w["p"], w["h"]
        fp = self.feature_projection
        _lib.call("r3d_secc_linear", cur, M, c["conv_dim"][-1], fp.layer_norm.weight, fp.layer_norm.bias, fp.layer_norm.eps, fp.projection.weight,
                  fp.projection.bias, H, 0, None, P, st)
        tap("projected", P, (B, T, H))
        pc = self.encoder.pos_conv_embed.conv
        _lib.call("r3d_hubert_pos_conv", P, d["pos"], pc.bias, B, T, H, c["num_conv_pos_embeddings"], c["num_conv_pos_embedding_groups"], X, st)
        tap("pos_conv", X, (B, T, H))
        for i, layer in enumerate(self.encoder.layers):
            a, ln, ff, fl = layer.attention, layer.layer_norm, layer.feed_forward, layer.final_layer_norm
            attention_half("r3d_i2p_attention", w, st, B, T, 1, H, heads, ln, a.q_proj, d["kv_w%d" % i], d["kv_b%d" % i], a.out_proj)
            _lib.call("r3d_secc_linear", X, M, H, fl.weight, fl.bias, fl.eps, ff.intermediate_dense.weight, ff.intermediate_dense.bias, I, 1, None, Hb,
                      st)
            _lib.call("r3d_secc_linear", Hb, M, I, None, None, 0.0, ff.output_dense.weight, ff.output_dense.bias, H, 0, X, X, st)
            if i == 0:
                tap("layer0", X, (B, T, H))
        out = torch.empty(B, T, H, device=wave.device, dtype=torch.float32)
        en = self.encoder.layer_norm
        _lib.call("r3d_secc_layernorm", X, M, H, en.weight, en.bias, en.eps, out, st)
        return out

    @torch.no_grad()
    def forward(self, input_values, taps=None):
        """input_values [B, n], already normalised -> last_hidden_state [B, T, hidden]."""
        if not torch.is_tensor(input_values) or input_values.dim() != 2 or input_values.shape[0] < 1:
            raise ValueError("HubertFeatureModel: expected input_values [B, n], got %s"
                             % (tuple(input_values.shape) if torch.is_tensor(input_values) else type(input_values),))
        B, n = input_values.shape
        if self.frames(n)[0] is None:
            raise ValueError("HubertFeatureModel: %d samples are fewer than one frame needs" % n)
        self._check_device(input_values, "waveform")
        x = input_values.detach().float().contiguous()
        return self._run(x, None, B, 0, n, n, taps)


def _as_wave(speech):
    """speech (NumPy or tensor; [n] or [n, channels]) as a 1-D fp32 tensor: the first channel, float64 rounded to fp32 first."""
    t = speech if torch.is_tensor(speech) else torch.from_numpy(np.ascontiguousarray(speech))
    if t.dim() == 2:
        t = t[:, 0]
    if t.dim() != 1:
        raise ValueError("hubert_features: expected speech [n] or [n, channels], got %s" % (tuple(t.shape),))
    return t.detach().float().contiguous()


@torch.no_grad()
def hubert_features(model, speech, clip_frames=1000, chunk_batch=4, taps=None):
    """get_hubert_from_16k_speech (extract_hubert.py:18-80): speech [n] (or [n, channels]: the first channel) -> [expected_T, hidden] on the
    model's device, expected_T = (n - 80) // 320.  The clip is normalised by its own mean and variance (r3d_hubert_wave_stats, once), cut by
    chunk_plan, and full chunks run chunk_batch at a time as one batch, which is bit-identical to one at a time.

    Float64 input is rounded to fp32 before the statistics, as Wav2Vec2FeatureExtractor does: exact for PCM-16 data (what sf.read returns).
    The statistics themselves are fp64 here and fp32 NumPy in the reference, a stated deviation.

    The reference's `ret[:, -1:, :]` repeat branch (taken when fewer than expected_T frames came out) is unreachable for n >= 400 and is not
    reproduced.  With c = 320 F (F = clip_frames), N = n // c and r = n - c N: a chunk of L samples gives (L - 400) // 320 + 1 frames, so
    every full chunk of c + 80 samples gives F; the last one is clipped to c + r samples when r < 80 and gives F - 1; the tail gives
    (r - 80) // 320 frames when r >= 400.  For r >= 80 that is F N + (r - 80) // 320 (the quotient is 0 below 400), for r < 80 it is
    F N - 1 = F N + floor((r - 80) / 320): both are expected_T = (c N + r - 80) // 320 exactly, never fewer.  n < 400 is a ValueError."""
    wave = _as_wave(speech)
    n = wave.numel()
    if n < KERNEL:
        raise ValueError("hubert_features: %d samples are fewer than the %d one frame needs" % (n, KERNEL))
    if clip_frames < 1 or chunk_batch < 1:
        raise ValueError("hubert_features: clip_frames and chunk_batch must be at least 1")
    dev = model.encoder.layer_norm.weight.device
    wave = wave.to(dev)
    model._check_device(wave, "waveform")
    expected_T = (n - (KERNEL - STRIDE)) // STRIDE
    with model._device_of(wave):
        stats = torch.empty(2, device=dev, dtype=torch.float64)
        _lib.call("r3d_hubert_wave_stats", wave, n, stats)
        plan = chunk_plan(n, clip_frames)
        clip = STRIDE * clip_frames
        out, i = [], 0
        while i < len(plan):
            s0, e0 = plan[i]
            nb = 1          # chunks of the full length that follow one another run as one batch: sequence b starts at s0 + b clip
            while e0 - s0 == clip + KERNEL - STRIDE and nb < chunk_batch and i + nb < len(plan) and plan[i + nb][1] - plan[i + nb][0] == e0 - s0:
                nb += 1
            y = model._run(wave, stats, nb, s0, clip, e0 - s0, taps if i == 0 else None)
            out.extend(y[b] for b in range(nb))
            i += nb
        ret = torch.cat(out, dim=0)
    if ret.shape[0] < expected_T:
        raise RuntimeError("hubert_features: %d frames for %d samples, %d expected" % (ret.shape[0], n, expected_T))
    return ret[:expected_T].contiguous()


def read_wav16k(name):
    """(samples as float64 in [-1, 1), rate): soundfile where it is importable, else the stdlib wave module for 16-bit PCM (int / 32768)."""
    try:
        import soundfile as sf
    except ImportError:
        sf = None
    if sf is not None:
        return sf.read(name)
    import wave
    with wave.open(name, "rb") as f:
        if f.getsampwidth() != 2 or f.getcomptype() != "NONE":
            raise ValueError("get_hubert: %s is not 16-bit PCM (install soundfile for other formats)" % name)
        rate, ch = f.getframerate(), f.getnchannels()
        data = np.frombuffer(f.readframes(f.getnframes()), dtype="<i2").astype(np.float64) / 32768.0
    return (data.reshape(-1, ch) if ch > 1 else data), rate


def get_hubert(model, wav16k_name):
    """GeneFace2Infer.get_hubert (real3d_infer.py:323-334): the [T8, hidden] float32 NumPy array, rows zero-padded to a multiple of 8."""
    speech, _ = read_wav16k(wav16k_name)
    feats = hubert_features(model, speech)
    T = feats.shape[0]
    out = torch.zeros((T + 7) // 8 * 8, feats.shape[1], device=feats.device, dtype=torch.float32)
    out[:T] = feats
    return out.cpu().numpy()


def patch_hubert(infer, model):
    """Bind infer.get_hubert (a GeneFace2Infer) to get_hubert(model, .); the old method stays at infer._r3d_reference_get_hubert."""
    if not isinstance(model, HubertFeatureModel):
        raise TypeError("patch_hubert: model is a %s, not a HubertFeatureModel" % type(model).__name__)
    if not hasattr(infer, "_r3d_reference_get_hubert"):
        infer._r3d_reference_get_hubert = getattr(infer, "get_hubert", None)
    infer.get_hubert = lambda wav16k_name: get_hubert(model, wav16k_name)
    return True
