"""The audio-to-motion VAE on the HIP kernels r3d_a2m_conv1d, r3d_a2m_wn_layer and r3d_a2m_pitch_embed (include/r3d_hip_audio.h,
DESIGN 4.20):

    PitchContourVAEModel   modules/audio2motion/vae.py:340-454  (use_pitch: true, the shipped egs/os_avatar/audio2motion_vae.yaml)
    VAEModel               modules/audio2motion/vae.py:272-337
    patch_audio2secc       installs one of them as infer.audio2secc_model (inference/real3d_infer.py:365-388 calls its forward)

Both keep the reference's constructor arguments and its state_dict keys (the training-only encoder, weight_g / weight_v and the BatchNorm
buffers included), so a reference checkpoint loads with strict=True.  INFERENCE ONLY: forward(batch, ret, train=False, temperature=1.)
returns x_recon [B, T, in_out_dim] and sets ret['pred'] and ret['mask']; train=True, sqz_prior, cond_drop and hparams['use_adapters']
raise NotImplementedError.  Inputs are detached and no autograd graph is built.

The forward is LAUNCHES_PITCH = 37 (LAUNCHES_VAE = 33) library launches and no torch convolution or linear:
    pitch_embed                     f0 [B, 2 T] -> indices -> pitch_embed rows                                   (pitch model only)
    mel_encoder  x 2                Conv1d(k 3) + folded BatchNorm1d + GELU, then Conv1d(k 3); the 0.5 x down-sampling of the audio
                                    (nearest, or linear for VAEModel) is the first conv's row mode; the second writes columns 0 .. F of
                                    the [B, T, 2 F] buffer cond_proj reads
    pitch_encoder x 2               the same on the pitch rows, into columns F .. 2 F                             (pitch model only)
    cond_proj                       k = 1 over [cond_feat | pitch_feat]; blink_embed and the amplitude vectors are folded through
                                    cond_proj's columns into a [2, F] table and one vector each                   (pitch model only)
    g_pre_net                       Conv1d(k 8, stride 4, pad 2): g_sqz [B, T / 4, F]
    4 x (pre, 4 x wn_layer, post)   the reverse ResidualCouplingLayers.  No Flip moves data: with the state kept in place, a flipped
                                    layer reads columns 8 .. 16 through pre's column-reversed weights and post subtracts its mean,
                                    flip_out, from columns 0 .. 8 (subtract_from = the state itself)
    decoder pre_net                 ConvTranspose1d(16, 256, 4, 4) as k = 1 to [T / 4, 4 x 256] = [T, 256]
    4 x wn_layer, out_proj          WN(256, k 5) conditioned on cond_feat at full rate, then out_proj with the final * mask
Weight norm, the BatchNorm folds, the cond_proj folds and the kernel layouts are computed in fp64 once per parameter version (_prepare of
_state.py); work buffers live per (device, stream, B, T) and are not reallocated by a second call.  The latent is drawn exactly as the
reference draws it, torch.distributions.Normal(0, 1).sample([B, 16, T / 4]) on the CPU generator, so one torch.manual_seed gives one clip;
z_p= supplies the draw instead.  T must be a multiple of 4 (the reference pads the audio to a multiple of 8, real3d_infer.py:328-333).
"""
import copy

import torch
import torch.nn as nn

from . import _lib
from ._state import _FoldedModule

WN_ROWS = _lib.A2M_WN_ROWS          # the time tile of r3d_a2m_wn_layer (R3D_A2M_WN_ROWS): tests put their edges around it
LATENT, HIDDEN, DEC_LAYERS, DEC_K, ENC_LAYERS, FLOW_HIDDEN, FLOW_K, FLOW_LAYERS, N_FLOWS, SQZ = 16, 256, 4, 5, 8, 64, 3, 4, 4, 4   # vae.py:292-294
LAUNCHES_FLOW = N_FLOWS * (FLOW_LAYERS + 2)
LAUNCHES_VAE = 2 + 1 + LAUNCHES_FLOW + 1 + DEC_LAYERS + 1            # mel_encoder, g_pre_net, the flows, pre_net, the decoder's WN, out_proj
LAUNCHES_PITCH = LAUNCHES_VAE + 1 + 2 + 1                            # + pitch_embed, pitch_encoder, cond_proj
DEFAULT_AMP = 0.4                                                    # vae.py:419,425


# ---- parameter holders with the reference's names (never called: the kernels read the folded weights) ----------------------------------
class _WNConv(nn.Module):
    """torch.nn.utils.weight_norm(nn.Conv1d(cin, cout, k)): weight_g [cout, 1, 1], weight_v [cout, cin, k], bias."""

    def __init__(self, cin, cout, k):
        super().__init__()
        conv = nn.Conv1d(cin, cout, k)
        self.bias = nn.Parameter(conv.bias.detach().clone())
        self.weight_g = nn.Parameter(conv.weight.detach().norm(dim=(1, 2), keepdim=True))
        self.weight_v = nn.Parameter(conv.weight.detach().clone())


class _WN(nn.Module):
    """flow_base.py:21-68 (dilation_rate 1, p_dropout 0)."""

    def __init__(self, hidden, k, n_layers, gin):
        super().__init__()
        self.hidden_channels, self.kernel_size, self.n_layers, self.gin_channels = hidden, k, n_layers, gin
        self.cond_layer = _WNConv(gin, 2 * hidden * n_layers, 1)
        self.in_layers = nn.ModuleList(_WNConv(hidden, 2 * hidden, k) for _ in range(n_layers))
        self.res_skip_layers = nn.ModuleList(_WNConv(hidden, 2 * hidden if i < n_layers - 1 else hidden, 1) for i in range(n_layers))


class _Flip(nn.Module):
    pass


class _CouplingLayer(nn.Module):
    """ResidualCouplingLayer(mean_only=True), flow_base.py:614-667."""

    def __init__(self, channels, hidden, k, n_layers, gin):
        super().__init__()
        self.pre = nn.Conv1d(channels // 2, hidden, 1)
        self.enc = _WN(hidden, k, n_layers, gin)
        self.post = nn.Conv1d(hidden, channels // 2, 1)
        nn.init.zeros_(self.post.weight)
        nn.init.zeros_(self.post.bias)


class _CouplingBlock(nn.Module):
    def __init__(self, channels, hidden, k, n_layers, n_flows, gin):
        super().__init__()
        self.flows = nn.ModuleList()
        for _ in range(n_flows):
            self.flows.append(_CouplingLayer(channels, hidden, k, n_layers, gin))
            self.flows.append(_Flip())


class _Encoder(nn.Module):
    """FVAEEncoder, vae.py:99-124: training only; its parameters are held so that a checkpoint loads with strict=True."""

    def __init__(self, cin, hidden, latent, k, n_layers, gin):
        super().__init__()
        self.pre_net = nn.Sequential(nn.Conv1d(cin, hidden, 2 * SQZ, SQZ, SQZ // 2))
        self.wn = _WN(hidden, k, n_layers, gin)
        self.out_proj = nn.Conv1d(hidden, 2 * latent, 1)


class _Decoder(nn.Module):
    """FVAEDecoder, vae.py:127-148."""

    def __init__(self, latent, hidden, cout, k, n_layers, gin):
        super().__init__()
        self.pre_net = nn.Sequential(nn.ConvTranspose1d(latent, hidden, SQZ, SQZ))
        self.wn = _WN(hidden, k, n_layers, gin)
        self.out_proj = nn.Conv1d(hidden, cout, 1)


class _FVAE(nn.Module):
    """FVAE, vae.py:150-191, as the two models build it: strides [4], sqz_prior False."""

    def __init__(self, in_out, gin, use_prior_glow):
        super().__init__()
        self.g_pre_net = nn.Sequential(nn.Conv1d(gin, gin, 2 * SQZ, SQZ, SQZ // 2))
        self.encoder = _Encoder(in_out, HIDDEN, LATENT, DEC_K, ENC_LAYERS, gin)
        if use_prior_glow:
            self.prior_flow = _CouplingBlock(LATENT, FLOW_HIDDEN, FLOW_K, FLOW_LAYERS, N_FLOWS, gin)
        self.decoder = _Decoder(LATENT, HIDDEN, in_out, DEC_K, DEC_LAYERS, gin)


def _mel_encoder(cin, feat):
    return nn.Sequential(nn.Conv1d(cin, feat, 3, 1, 1, bias=False), nn.BatchNorm1d(feat), nn.GELU(), nn.Conv1d(feat, feat, 3, 1, 1, bias=False))


# ---- the folds, in fp64 (tests compare them with torch's weight_norm / BatchNorm1d); `dtype` is what they are rounded to --------------
def _d(p):
    return p.detach().double()


def wn_weight(layer):
    """g v / ||v||, the norm over dims 1, 2 (torch.nn.utils.weight_norm, dim 0) -> [cout, cin, k] fp64."""
    v = _d(layer.weight_v)
    return _d(layer.weight_g) * v / v.norm(dim=(1, 2), keepdim=True)


def kernel_weight(w):
    """torch's Conv1d weight [cout, cin, k] -> r3d_a2m_conv1d's [cout, k, cin]."""
    return w.permute(0, 2, 1).contiguous()


def fold_conv_bn(conv, bn):
    """A bias-free Conv1d followed by BatchNorm1d in eval mode -> (w [cout, cin, k], b [cout]) fp64."""
    s = _d(bn.weight) / torch.sqrt(_d(bn.running_var) + bn.eps)
    return _d(conv.weight) * s[:, None, None], _d(bn.bias) - _d(bn.running_mean) * s


def fold_encoder(seq, dtype=torch.float32):
    """mel_encoder / pitch_encoder -> the two conv launches' (w, b) in kernel layout."""
    w0, b0 = fold_conv_bn(seq[0], seq[1])
    return {"w0": kernel_weight(w0).to(dtype), "b0": b0.to(dtype).contiguous(), "w1": kernel_weight(_d(seq[3].weight)).to(dtype)}


def fold_wn(wn, dtype=torch.float32):
    """One dict per layer of r3d_a2m_wn_layer: w_in [k H + Cg, 2 H] (row j H + ci: tap j, channel ci of the in_layer; row k H + cg: the
    layer's slice of cond_layer), b_in the two biases' sum, w_rs [H, 2 H or H], b_rs."""
    H, k, L = wn.hidden_channels, wn.kernel_size, wn.n_layers
    wc, bc = wn_weight(wn.cond_layer)[:, :, 0], _d(wn.cond_layer.bias)          # [2 H L, Cg]
    out = []
    for i in range(L):
        w = wn_weight(wn.in_layers[i])                                          # [2 H, H, k]
        sl = slice(2 * H * i, 2 * H * (i + 1))
        w_in = torch.cat([w.permute(2, 1, 0).reshape(k * H, 2 * H), wc[sl].t()], 0)
        rs = wn.res_skip_layers[i]
        out.append({"w_in": w_in.to(dtype).contiguous(), "b_in": (_d(wn.in_layers[i].bias) + bc[sl]).to(dtype).contiguous(),
                    "w_rs": wn_weight(rs)[:, :, 0].t().to(dtype).contiguous(), "b_rs": _d(rs.bias).to(dtype).contiguous()})
    return out


def fold_flow(layer, flipped, dtype=torch.float32):
    """One reverse ResidualCouplingLayer on the in-place state: `flipped` layers see flip(state), so pre reads columns 8 .. 16 with its
    input columns reversed and post's mean is stored flip_out."""
    w = _d(layer.pre.weight)
    if flipped:
        w = w.flip(1)
    return {"pre_w": kernel_weight(w).to(dtype), "pre_b": _d(layer.pre.bias).to(dtype).contiguous(), "wn": fold_wn(layer.enc, dtype),
            "post_w": kernel_weight(_d(layer.post.weight)).to(dtype), "post_b": _d(layer.post.bias).to(dtype).contiguous(), "flipped": flipped}


def fold_vae(vae, dtype=torch.float32):
    F = {"g_pre_w": kernel_weight(_d(vae.g_pre_net[0].weight)).to(dtype), "g_pre_b": _d(vae.g_pre_net[0].bias).to(dtype).contiguous(), "flows": []}
    if hasattr(vae, "prior_flow"):
        # reversed(flows) = Flip, layer 3, Flip, layer 2, ...: layer i runs on a state flipped (i odd) or not (i even), and the state ends unflipped
        F["flows"] = [fold_flow(vae.prior_flow.flows[2 * i], i % 2 == 1, dtype) for i in reversed(range(N_FLOWS))]
    up = vae.decoder.pre_net[0]                                                  # weight [16, 256, 4]: y[co, 4 t + j] = sum_ci x[ci, t] w[ci, co, j]
    F["up_w"] = _d(up.weight).permute(2, 1, 0).reshape(SQZ * HIDDEN, 1, LATENT).to(dtype).contiguous()
    F["up_b"] = _d(up.bias).repeat(SQZ).to(dtype).contiguous()
    F["dec"] = fold_wn(vae.decoder.wn, dtype)
    F["out_w"] = kernel_weight(_d(vae.decoder.out_proj.weight)).to(dtype)
    F["out_b"] = _d(vae.decoder.out_proj.bias).to(dtype).contiguous()
    return F


def fold_cond_proj(m, dtype=torch.float32):
    """cond_proj over [cond_feat | pitch_feat | blink_feat | mouth | eye] -> the k = 1 weight over the first two, the blink table
    blink_embed cond_proj[:, 2 F : 3 F]^T [2, F] and one vector cond_proj[:, ...] amp_embed per amplitude."""
    W, f = _d(m.cond_proj.weight), m.feat_dim
    F = {"w": W[:, :2 * f].reshape(f, 1, 2 * f).to(dtype).contiguous(), "b": _d(m.cond_proj.bias).to(dtype).contiguous(),
         "table": (_d(m.blink_embed.weight) @ W[:, 2 * f:3 * f].t()).to(dtype).contiguous(), "mouth": None, "eye": None}
    c = 3 * f
    for name in ("mouth", "eye"):
        if hasattr(m, name + "_amp_embed"):
            F[name] = (W[:, c:c + f] @ _d(getattr(m, name + "_amp_embed"))).to(dtype).contiguous()
            c += f
    return F


def draw_latent(B, Tq):
    """The reference's own draw (FVAE.forward, vae.py:243-244): prior_dist.sample([B, 16, Tq]) on the CPU generator."""
    return torch.distributions.Normal(0, 1).sample([B, LATENT, Tq])


# ---- launch wrappers -------------------------------------------------------------------------------------------------------------------
def conv1d(x, B, Tin, Cin, w, y, k=1, stride=1, pad=0, bias=None, x_stride=None, x_offset=0, row_mode=0, gelu=False, mask=None, table=None,
           idx=None, idx_step=1, amp0=None, u0=None, amp1=None, u1=None, subtract_from=None, y_stride=None, y_offset=0, flip_out=False):
    """r3d_a2m_conv1d; w [Cout, k, Cin]."""
    Cout = w.shape[0]
    _lib.call("r3d_a2m_conv1d", x, B, Tin, Cin, x_stride or Cin, x_offset, row_mode, w, bias, Cout, k, stride, pad, int(gelu), mask, table, idx,
              0 if table is None else table.shape[0], idx_step, amp0, u0, amp1, u1, subtract_from, y, y_stride or Cout, y_offset, int(flip_out))
    return y


def wn_layer(x, g, B, T, H, Cg, k, layer, mask, first, last, x_next, out):
    """r3d_a2m_wn_layer with one entry of fold_wn."""
    _lib.call("r3d_a2m_wn_layer", x, g, B, T, H, Cg, k, layer["w_in"], layer["b_in"], layer["w_rs"], layer["b_rs"], mask, int(first), int(last),
              x_next, out)


def pitch_embed(f0, B, T, table, index, y):
    _lib.call("r3d_a2m_pitch_embed", f0, B, T, table, table.shape[0], table.shape[1], index, y)


def _wn(layers, x, spare, g, B, T, H, Cg, k, out, taps=None, name=None):
    """WN.forward with mask 1: x and spare ping-pong; returns out."""
    n = len(layers)
    for i, layer in enumerate(layers):
        wn_layer(x, g, B, T, H, Cg, k, layer, None, i == 0, i == n - 1, None if i == n - 1 else spare, out)
        if taps is not None:
            taps["%s_out%d" % (name, i)] = out.clone()
            if i < n - 1:
                taps["%s_x%d" % (name, i)] = spare.clone()
        x, spare = spare, x
    return out


class _Audio2Motion(_FoldedModule):
    """What the two models share: the FVAE's inference path, the input checks, the latent and the work buffers."""

    def _init_common(self, in_out_dim, audio_in_dim, feat_dim, sqz_prior, cond_drop, use_prior_flow):
        for flag, value in (("sqz_prior", sqz_prior), ("cond_drop", cond_drop)):
            if value:
                raise NotImplementedError("%s: %s=True has no HIP implementation" % (type(self).__name__, flag))
        self.audio_in_dim, self.feat_dim, self.in_dim, self.out_dim = audio_in_dim, feat_dim, in_out_dim, in_out_dim
        self.sqz_prior, self.cond_drop, self.use_prior_flow = sqz_prior, cond_drop, use_prior_flow

    @property
    def device(self):
        return next(self.vae.parameters()).device

    def _new_buffers(self, dev, B, T):
        e = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)
        Tq, f = T // SQZ, self.feat_dim
        return {"h": e(B, T, f), "cat": e(B, T, 2 * f), "pe": e(B, T, f), "index": torch.empty(B, T, device=dev, dtype=torch.int32),
                "cond": e(B, T, f), "gq": e(B, Tq, f), "z": e(B, Tq, LATENT), "fa": e(B, Tq, FLOW_HIDDEN), "fb": e(B, Tq, FLOW_HIDDEN),
                "fo": e(B, Tq, FLOW_HIDDEN), "da": e(B, T, HIDDEN), "db": e(B, T, HIDDEN), "do": e(B, T, HIDDEN)}

    def _inputs(self, batch, train):
        if train:
            raise NotImplementedError("%s: train=True has no HIP implementation (inference only)" % type(self).__name__)
        dev = self.device
        if dev.type != "cuda":
            raise ValueError("%s: the module is on %s; the kernels run on the GPU only" % (type(self).__name__, dev))
        f = lambda t: t.detach().to(device=dev, dtype=torch.float32).contiguous()
        mask, mel = f(batch["y_mask"]), f(batch["audio"])
        B, T = mask.shape
        if mel.dim() != 3 or mel.shape[0] != B or mel.shape[1] // 2 != T or mel.shape[2] != self.audio_in_dim:
            raise ValueError("%s: audio %s does not go with y_mask %s (expected [B, 2 T, %d])"
                             % (type(self).__name__, tuple(mel.shape), tuple(mask.shape), self.audio_in_dim))
        if T < SQZ or T % SQZ:
            raise ValueError("%s: T = %d must be a positive multiple of %d (the reference pads the audio to a multiple of 8)"
                             % (type(self).__name__, T, SQZ))
        return dev, mask, mel[:, :2 * T].contiguous(), B, T

    def _latent(self, z_p, B, Tq, temperature, dev, z):
        if z_p is None:
            z_p = draw_latent(B, Tq)
        if tuple(z_p.shape) != (B, LATENT, Tq):
            raise ValueError("%s: z_p %s, expected %s" % (type(self).__name__, tuple(z_p.shape), (B, LATENT, Tq)))
        z.copy_((z_p.detach().to(device=dev, dtype=torch.float32) * temperature).transpose(1, 2))
        return z

    def _vae(self, F, w, g, mask, B, T, temperature, z_p, taps):
        """FVAE.forward(infer=True), vae.py:243-269, on cond_feat g [B, T, F]; returns x_recon * mask, a new tensor."""
        dev, Tq, f = g.device, T // SQZ, self.feat_dim
        conv1d(g, B, T, f, F["g_pre_w"], w["gq"], k=2 * SQZ, stride=SQZ, pad=SQZ // 2, bias=F["g_pre_b"])
        z = self._latent(z_p, B, Tq, temperature, dev, w["z"])
        half = LATENT // 2
        for n, fl in enumerate(F["flows"]):
            conv1d(z, B, Tq, half, fl["pre_w"], w["fa"], bias=fl["pre_b"], x_stride=LATENT, x_offset=half if fl["flipped"] else 0)
            _wn(fl["wn"], w["fa"], w["fb"], w["gq"], B, Tq, FLOW_HIDDEN, f, FLOW_K, w["fo"])
            conv1d(w["fo"], B, Tq, FLOW_HIDDEN, fl["post_w"], z, bias=fl["post_b"], subtract_from=z, y_stride=LATENT, y_offset=half,
                   flip_out=fl["flipped"])
            if taps is not None:          # the reference's state after this layer, before the Flip that follows it in reversed(flows)
                taps["z_flow%d" % (N_FLOWS - 1 - n)] = z.flip(2) if fl["flipped"] else z.clone()
        conv1d(z, B, Tq, LATENT, F["up_w"], w["da"], bias=F["up_b"])              # [B, Tq, 4 x 256] = [B, T, 256]
        if taps is not None:
            taps.update(g_sqz=w["gq"].clone(), dec_in=w["da"].clone())
        _wn(F["dec"], w["da"], w["db"], g, B, T, HIDDEN, f, DEC_K, w["do"], taps, "dec")
        out = torch.empty(B, T, self.out_dim, device=dev, dtype=torch.float32)
        return conv1d(w["do"], B, T, HIDDEN, F["out_w"], out, bias=F["out_b"], mask=mask)

    @classmethod
    def from_reference(cls, ref):
        """A HIP copy of a constructed reference model: same arguments, parameters and buffers, device and eval mode."""
        for m in ref.modules():
            if getattr(m, "use_adapters", False):
                raise NotImplementedError("%s: hparams['use_adapters'] has no HIP implementation" % cls.__name__)
        new = cls(**cls._reference_args(ref))
        new.load_state_dict(ref.state_dict(), strict=True)
        return new.to(next(ref.parameters()).device).eval()


class VAEModel(_Audio2Motion):
    """vae.py:272-337.  batch: 'y_mask' [B, T], 'audio' [B, 2 T, audio_in_dim] (down-sampled with mode='linear')."""

    def __init__(self, in_out_dim=64, audio_in_dim=1024, sqz_prior=False, cond_drop=False, use_prior_flow=True):
        super().__init__()
        self._init_common(in_out_dim, audio_in_dim, 64, sqz_prior, cond_drop, use_prior_flow)
        self.blink_embed = nn.Embedding(2, self.feat_dim)
        self.mel_encoder = _mel_encoder(audio_in_dim, self.feat_dim)
        self.vae = _FVAE(in_out_dim, self.feat_dim, use_prior_flow)

    def _fold(self):
        return {"mel": fold_encoder(self.mel_encoder), "vae": fold_vae(self.vae)}

    @torch.no_grad()
    def forward(self, batch, ret, train=False, return_latent=False, temperature=1., z_p=None, _taps=None):
        dev, mask, mel, B, T = self._inputs(batch, train)
        F, w, f = self._prepare(), self._buffers_for(dev, B, T), self.feat_dim
        conv1d(mel, B, T, self.audio_in_dim, F["mel"]["w0"], w["h"], k=3, pad=1, bias=F["mel"]["b0"], row_mode=2, gelu=True)
        conv1d(w["h"], B, T, f, F["mel"]["w1"], w["cond"], k=3, pad=1)
        if _taps is not None:
            _taps["cond_feat"] = w["cond"].clone()
        x = self._vae(F["vae"], w, w["cond"], mask, B, T, temperature, z_p, _taps)
        ret["pred"], ret["mask"] = x, mask
        return x

    @staticmethod
    def _reference_args(ref):
        return {"in_out_dim": ref.in_dim, "audio_in_dim": ref.audio_in_dim, "sqz_prior": ref.sqz_prior, "cond_drop": ref.cond_drop,
                "use_prior_flow": ref.use_prior_flow}


class PitchContourVAEModel(_Audio2Motion):
    """vae.py:340-454.  batch: 'y_mask' [B, T], 'audio' [B, 2 T, audio_in_dim], 'f0' [B, 2 T]; optional 'blink' [B, 2 T, 1] int64 (zeros),
    'mouth_amp' / 'eye_amp' [B, 1] (0.4) when hparams switch their embeddings on."""

    def __init__(self, hparams, in_out_dim=64, audio_in_dim=1024, sqz_prior=False, cond_drop=False, use_prior_flow=True):
        super().__init__()
        self.hparams = copy.deepcopy(hparams)
        if hparams.get("use_adapters", False):
            raise NotImplementedError("PitchContourVAEModel: hparams['use_adapters'] has no HIP implementation")
        self._init_common(in_out_dim, audio_in_dim, 128, sqz_prior, cond_drop, use_prior_flow)
        f = self.feat_dim
        self.blink_embed = nn.Embedding(2, f)
        self.mel_encoder = _mel_encoder(audio_in_dim, f)
        self.pitch_embed = nn.Embedding(300, f, None)
        nn.init.normal_(self.pitch_embed.weight, mean=0, std=f ** -0.5)
        self.pitch_encoder = _mel_encoder(f, f)
        cond_dim = 3 * f
        if hparams.get("use_mouth_amp_embed", False):
            self.mouth_amp_embed = nn.Parameter(torch.randn(f))
            cond_dim += f
        if hparams.get("use_eye_amp_embed", False):
            self.eye_amp_embed = nn.Parameter(torch.randn(f))
            cond_dim += f
        self.cond_proj = nn.Linear(cond_dim, f, bias=True)
        self.vae = _FVAE(in_out_dim, f, use_prior_flow)

    def _fold(self):
        return {"mel": fold_encoder(self.mel_encoder), "pitch": fold_encoder(self.pitch_encoder), "proj": fold_cond_proj(self),
                "table": self.pitch_embed.weight.detach().float().contiguous(), "vae": fold_vae(self.vae)}

    @torch.no_grad()
    def forward(self, batch, ret, train=False, return_latent=False, temperature=1., z_p=None, _taps=None):
        dev, mask, mel, B, T = self._inputs(batch, train)
        name, f = type(self).__name__, self.feat_dim
        f0 = batch["f0"].detach().to(device=dev, dtype=torch.float32)
        if f0.dim() != 2 or f0.shape[0] != B or f0.shape[1] // 2 != T:
            raise ValueError("%s: f0 %s, expected [B, 2 T] = %s" % (name, tuple(f0.shape), (B, 2 * T)))
        f0 = f0[:, :2 * T].contiguous()
        if "blink" not in batch:          # as the reference does (vae.py:404-405)
            batch["blink"] = torch.zeros([B, f0.shape[1], 1], dtype=torch.long, device=dev)
        blink = batch["blink"].detach().to(device=dev, dtype=torch.long)
        if blink.dim() != 3 or blink.shape[0] != B or blink.shape[1] // 2 != T or blink.shape[2] != 1:
            raise ValueError("%s: blink %s, expected [B, 2 T, 1] = %s" % (name, tuple(blink.shape), (B, 2 * T, 1)))
        blink = blink[:, :2 * T, 0].contiguous()
        amps = {}
        for key in ("mouth", "eye"):
            if self.hparams.get("use_%s_amp_embed" % key, False):
                a = batch.get(key + "_amp")
                a = torch.full([B], DEFAULT_AMP, device=dev, dtype=torch.float32) if a is None else a.detach().to(device=dev, dtype=torch.float32)
                if a.numel() != B:
                    raise ValueError("%s: %s_amp %s, expected [B, 1] = %s" % (name, key, tuple(a.shape), (B, 1)))
                amps[key] = a.reshape(B).contiguous()
        F, w = self._prepare(), self._buffers_for(dev, B, T)
        pitch_embed(f0, B, T, F["table"], w["index"], w["pe"])
        conv1d(mel, B, T, self.audio_in_dim, F["mel"]["w0"], w["h"], k=3, pad=1, bias=F["mel"]["b0"], row_mode=1, gelu=True)
        conv1d(w["h"], B, T, f, F["mel"]["w1"], w["cat"], k=3, pad=1, y_stride=2 * f)
        conv1d(w["pe"], B, T, f, F["pitch"]["w0"], w["h"], k=3, pad=1, bias=F["pitch"]["b0"], gelu=True)
        conv1d(w["h"], B, T, f, F["pitch"]["w1"], w["cat"], k=3, pad=1, y_stride=2 * f, y_offset=f)
        P = F["proj"]
        conv1d(w["cat"], B, T, 2 * f, P["w"], w["cond"], bias=P["b"], table=P["table"], idx=blink, idx_step=2,
               amp0=amps.get("mouth"), u0=P["mouth"] if "mouth" in amps else None, amp1=amps.get("eye"), u1=P["eye"] if "eye" in amps else None)
        if _taps is not None:
            _taps.update(cond_feat=w["cond"].clone(), pitch_index=w["index"].clone())
        x = self._vae(F["vae"], w, w["cond"], mask, B, T, temperature, z_p, _taps)
        ret["pred"], ret["mask"] = x, mask
        return x

    @staticmethod
    def _reference_args(ref):
        return {"hparams": ref.hparams, "in_out_dim": ref.in_dim, "audio_in_dim": ref.audio_in_dim, "sqz_prior": ref.sqz_prior,
                "cond_drop": ref.cond_drop, "use_prior_flow": ref.use_prior_flow}


def is_reference_audio2secc(m):
    """One of the reference's two VAE models (not the ICL model, not a module of this package)."""
    return type(m).__name__ in ("PitchContourVAEModel", "VAEModel") and not type(m).__module__.startswith("real3dportrait_amd")


def patch_audio2secc(infer):
    """Replace infer.audio2secc_model (a GeneFace2Infer, inference/real3d_infer.py) by its HIP copy when it is one of the reference's two
    VAE models: same device, eval mode; the original stays at infer._r3d_reference_audio2secc_model.  forward_audio2secc itself is not
    replaced.  Anything else (the ICL model, a module already replaced) is left alone.  Returns whether the model was replaced."""
    ref = getattr(infer, "audio2secc_model", None)
    if not is_reference_audio2secc(ref):
        return False
    cls = PitchContourVAEModel if type(ref).__name__ == "PitchContourVAEModel" else VAEModel
    new = cls.from_reference(ref)
    infer._r3d_reference_audio2secc_model = ref
    infer.audio2secc_model = new
    return True
