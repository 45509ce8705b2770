"""Img2PlaneModel (modules/img2plane/img2plane_model.py:12-82), the canonical image-to-plane backbone, on the HIP library: HighResoEncoder
(simple_encoders/high_resolution_encoder.py), LowResolutionViT and TriplanePredictorViT (segformer/models.py, base.py) in exact fp32
(include/r3d_hip_img2plane.h).  DeepLabV3 (low_reso_encoder) is whatever module the caller hands over.  When it is this package's
DeepLabV3 (deeplabv3.py) the forward takes a fast path: r3d_dl_assemble_input writes the channel-last input, the encoder's
forward_cl writes feat_low channel-last, and no layout conversion runs.  Any other encoder runs as it is, in torch, on the input that
assemble_input (img2plane_model.py:45-64, verbatim) builds; nothing in this module constructs a DeepLabV3.

The module keeps the reference's attribute names and state_dict keys, so a reference checkpoint loads with strict=True.  INFERENCE ONLY
(Dropout / DropPath are identity); inputs are detached and no autograd graph is built.

    forward(x, cond=None)   [B, 3, S, S] -> the reference's flipped planes [B, 3, out_channels / 3, S/2, S/2]
    from_reference(m)       a HIP copy of a constructed reference Img2PlaneModel, around m's own low_reso_encoder
"""
import torch
import torch.nn as nn

from . import _lib
from ._state import _FoldedModule
from .token_blocks import Block, PatchEmbed, conv_weight_cl, mit_block          # conv_weight_cl: also this module's name for it

DIM, HEADS, HIDDEN = 1024, 4, 2048          # Block(dim=1024, num_heads=4, mlp_ratio=2) of segformer/models.py:28,114
INPUT_CHANNELS = {"rgb": 3, "rgb_alpha": 4, "rgb_camera": 6, "rgb_alpha_camera": 7}          # img2plane_model.py:19-29, before the 2 grid channels
BLOCKS = {"small": (2, 1), "standard": (5, 1), "large": (10, 3)}          # (LowResolutionViT, TriplanePredictorViT), models.py:21-26,105-110
LN_EPS = 1e-5


class _HighResoEncoder(nn.Module):
    """The parameters of HighResoEncoder; its `activation` is never applied by the reference's forward (high_resolution_encoder.py:33-36)."""

    def __init__(self, in_dim):
        super().__init__()
        self.first = nn.Conv2d(in_dim, 64, 7, 2, 3)
        self.conv_layers = nn.Sequential(nn.Conv2d(64, 96, 3, 1, 1), nn.LeakyReLU(0.01), nn.Conv2d(96, 96, 3, 1, 1), nn.LeakyReLU(0.01),
                                         nn.Conv2d(96, 96, 3, 1, 1), nn.LeakyReLU(0.01), nn.Conv2d(96, 96, 3, 1, 1), nn.LeakyReLU(0.01))
        self.final = nn.Conv2d(96, 96, 3, 1, 1)


class _LowResolutionViT(nn.Module):
    def __init__(self, num_blocks):
        super().__init__()
        self.patch_embed = PatchEmbed(256, DIM, 3, 2)
        self.num_blocks = num_blocks
        for i in range(1, num_blocks + 1):
            setattr(self, "block%d" % i, Block(DIM, HIDDEN, 1))
        self.conv_after_upsample1 = nn.Conv2d(256, 128, 3, 1, 1)
        self.conv_after_upsample2 = nn.Conv2d(128, 128, 3, 1, 1)
        self.final_conv = nn.Conv2d(128, 96, 3, 1, 1)


class _TriplanePredictorViT(nn.Module):
    def __init__(self, out_channels, num_blocks):
        super().__init__()
        self.first_conv = nn.Conv2d(192, 256, 3, 1, 1)
        self.second_conv = nn.Conv2d(256, 128, 3, 1, 1)
        self.patch_embed = PatchEmbed(128, DIM, 3, 2)
        self.num_blocks = num_blocks
        for i in range(1, num_blocks + 1):
            setattr(self, "block%d" % i, Block(DIM, HIDDEN, 2))
        self.first_conv_after_cat = nn.Conv2d(352, 256, 3, 1, 1)
        self.second_conv_after_cat = nn.Conv2d(256, 128, 3, 1, 1)
        self.third_conv_after_cat = nn.Conv2d(128, 128, 3, 1, 1)
        self.final_conv = nn.Conv2d(128, out_channels, 3, 1, 1)


def pixel_shuffle_source(c, i, j):
    """nn.PixelShuffle(2): out[b, c, 2y + i, 2x + j] = in[b, 4c + 2i + j, y, x] -- the input channel r3d_i2p_pixel_shuffle reads."""
    return 4 * c + 2 * i + j


def is_reference_img2plane(m):
    """Is m the reference's Img2PlaneModel (by class name and parts), and not this package's?"""
    return (type(m).__name__ == "Img2PlaneModel" and not type(m).__module__.startswith("real3dportrait_amd")
            and all(hasattr(m, n) for n in ("low_reso_encoder", "high_reso_encoder", "low_reso_vit", "triplane_predictor_vit")))


class Img2PlaneModel(_FoldedModule):
    def __init__(self, out_channels=96, hp=None, low_reso_encoder=None, _blocks=None):
        super().__init__()
        self.hparams = dict(hp) if hp is not None else {}
        self.input_mode = self.hparams.get("img2plane_input_mode", "rgb")
        if self.input_mode not in INPUT_CHANNELS:
            raise ValueError("Img2PlaneModel: unknown img2plane_input_mode %r" % (self.input_mode,))
        scale = self.hparams.get("img2plane_backbone_scale", "standard")
        if _blocks is None and scale not in BLOCKS:
            raise ValueError("Img2PlaneModel: unknown img2plane_backbone_scale %r" % (scale,))
        if out_channels <= 0 or out_channels % 3:
            raise ValueError("Img2PlaneModel: out_channels = %r is not a positive multiple of 3" % (out_channels,))
        n_low, n_pred = _blocks if _blocks is not None else BLOCKS[scale]
        if "camera" in self.input_mode:
            self.camera_to_channel = nn.Linear(25, 3)
        self.in_channels = INPUT_CHANNELS[self.input_mode] + 2
        self.out_channels = out_channels
        self.low_reso_encoder = low_reso_encoder
        self.high_reso_encoder = _HighResoEncoder(self.in_channels)
        self.low_reso_vit = _LowResolutionViT(n_low)
        self.triplane_predictor_vit = _TriplanePredictorViT(out_channels, n_pred)

    # ---- parameters in the kernels' layouts (_prepare: once per parameter version) -------------------------------------------------
    def _fold(self):
        d = {}
        for part in ("high_reso_encoder", "low_reso_vit", "triplane_predictor_vit"):
            for name, m in getattr(self, part).named_modules():
                if isinstance(m, nn.Conv2d) and m.groups == 1:
                    d[part + "." + name] = conv_weight_cl(m.weight)
        return d

    def _new_buffers(self, dev, B, S, cin):
        s2, s4, s8 = S // 2, S // 4, S // 8
        e = lambda n: torch.empty(n, device=dev, dtype=torch.float32)
        tok, img = B * s4 * s4, B * s2 * s2
        return {"xcl": e(B * S * S * cin), "fl": e(B * s8 * s8 * 256),
                "x": e(tok * DIM), "t": e(tok * DIM), "q": e(tok * DIM), "o": e(tok * DIM), "h1": e(tok * HIDDEN), "h2": e(tok * HIDDEN),
                "sr": e(B * s8 * s8 * DIM), "kv": e(B * s8 * s8 * 2 * DIM),
                "a": e(img * 256), "b": e(img * 256), "lv": e(img * 96), "cat192": e(img * 192), "cat352": e(img * 352),
                "out": e(img * self.out_channels)}

    # ---- torch: the input assembly, shared with DeepLabV3 (img2plane_model.py:45-64, verbatim) --------------------------------------
    def _check(self, x, cond):
        if not torch.is_tensor(x) or x.dim() != 4 or x.shape[1] != 3:
            raise ValueError("Img2PlaneModel: expected an image [B, 3, S, S], got %s" % (tuple(x.shape) if torch.is_tensor(x) else type(x),))
        B, _, H, W = x.shape
        if B < 1:
            raise ValueError("Img2PlaneModel: empty batch")
        if H != W:
            raise ValueError("Img2PlaneModel: the image must be square (the reference calls block(h, H, H)), got %d x %d" % (H, W))
        if H < 16 or H % 16:
            raise ValueError("Img2PlaneModel: the side S = %d must be a positive multiple of 16" % H)
        if "camera" in self.input_mode:
            cams = cond.get("ref_cameras") if isinstance(cond, dict) else None
            if not torch.is_tensor(cams) or tuple(cams.shape) != (B, 25):
                raise ValueError("Img2PlaneModel: input mode %r needs cond['ref_cameras'] [B, 25]" % (self.input_mode,))
        if "alpha" in self.input_mode and isinstance(cond, dict) and cond.get("ref_alphas") is not None:
            if tuple(cond["ref_alphas"].shape) != (B, 1, H, W):
                raise ValueError("Img2PlaneModel: cond['ref_alphas'] must be [B, 1, S, S], got %s" % (tuple(cond["ref_alphas"].shape),))
        self._check_device(x, "image", next(self.high_reso_encoder.parameters()))
        if self.low_reso_encoder is None:
            raise ValueError("Img2PlaneModel: no low_reso_encoder was given (this package constructs no DeepLabV3)")
        return B, H

    def assemble_input(self, x, cond=None):
        """img2plane_model.py:45-64: [x | ref_alphas | camera_feat | grid_x | grid_y], NCHW."""
        bs, _, H, W = x.shape
        if self.input_mode in ("rgb_alpha", "rgb_alpha_camera"):
            if cond is None or cond.get("ref_alphas") is None:
                ref_alphas = (x.mean(dim=1, keepdim=True) >= -0.999).float()
            else:
                ref_alphas = cond["ref_alphas"].detach().float()
            x = torch.cat([x, ref_alphas], dim=1)
        if self.input_mode in ("rgb_camera", "rgb_alpha_camera"):
            camera_feat = self.camera_to_channel(cond["ref_cameras"].detach().float()).reshape(bs, 3, 1, 1).repeat([1, 1, H, W])
            x = torch.cat([x, camera_feat], dim=1)
        grid_x, grid_y = torch.meshgrid(torch.arange(H, device=x.device), torch.arange(W, device=x.device), indexing="ij")
        grid_x = grid_x / H
        grid_y = grid_y / H
        expanded_x = grid_x[None, None, :, :].repeat(bs, 1, 1, 1)
        expanded_y = grid_y[None, None, :, :].repeat(bs, 1, 1, 1)
        return torch.cat([x, expanded_x, expanded_y], dim=1)

    # ---- HIP: everything from feat_low and the assembled input to the planes ------------------------------------------------------------
    def _conv3(self, d, key, x, B, h, cin, act, slope, y, st):
        m = self.get_submodule(key)
        _lib.call("r3d_torso_conv", x, B, h, h, cin, 0, 0, None, None, 0.0, d[key], m.bias, m.out_channels, 3, act, slope, None, y, None, st)

    def _block(self, d, key, w, B, h, st):
        mit_block("r3d_i2p_attention", self.get_submodule(key), d.get(key + ".attn.sr"), w, st, B, h, h, DIM, HIDDEN, HEADS)

    def _run(self, x_in, feat_low, taps=None):
        """The library launches, on x_in's device and that device's current stream (which need not be the process's current device)."""
        with self._device_of(x_in):
            B, cin, S, _ = x_in.shape
            return self._launches(x_in.device, B, cin, S, x_in, feat_low, taps)

    def _launches(self, dev, B, cin, S, x_in, feat_low, taps):
        """x_in / feat_low None: the stream's "xcl" / "fl" buffers hold them channel-last already (the fast path)."""
        s2, s4, s8, s16 = S // 2, S // 4, S // 8, S // 16
        st = torch.cuda.current_stream().cuda_stream
        d = self._prepare()
        w = self._buffers_for(dev, B, S, cin)
        A, Bf, X, LV, C192, C352, OUT = w["a"], w["b"], w["x"], w["lv"], w["cat192"], w["cat352"], w["out"]
        img = B * s2 * s2
        lv, hv, pv = self.low_reso_vit, self.high_reso_encoder, self.triplane_predictor_vit
        tap = (lambda name, t, shape: taps.__setitem__(name, t[:shape[0] * shape[1] * shape[2] * shape[3]].view(shape).permute(0, 3, 1, 2).contiguous())) \
            if taps is not None else (lambda *a: None)

        # LowResolutionViT (models.py:65-88)
        if feat_low is not None:
            _lib.call("r3d_i2p_nchw_to_cl", feat_low, B, 256, s8, s8, w["fl"], st)
        pe = lv.patch_embed
        _lib.call("r3d_secc_conv", w["fl"], B, s8, s8, 256, d["low_reso_vit.patch_embed.proj"], pe.proj.bias, DIM, 3, 2, 1, pe.norm.weight, pe.norm.bias,
                  pe.norm.eps, X, st)
        for i in range(1, lv.num_blocks + 1):
            self._block(d, "low_reso_vit.block%d" % i, w, B, s16, st)
        _lib.call("r3d_i2p_pixel_shuffle", X, B, s16, s16, 256, A, 256, 0, st)
        _lib.call("r3d_i2p_upsample2x", A, B, s8, s8, 256, Bf, st)
        self._conv3(d, "low_reso_vit.conv_after_upsample1", Bf, B, s4, 256, 1, 0.0, A, st)
        _lib.call("r3d_i2p_upsample2x", A, B, s4, s4, 128, Bf, st)
        self._conv3(d, "low_reso_vit.conv_after_upsample2", Bf, B, s2, 128, 1, 0.0, A, st)
        self._conv3(d, "low_reso_vit.final_conv", A, B, s2, 128, 0, 0.0, LV, st)
        tap("feat_low_after_vit", LV, (B, s2, s2, 96))
        _lib.call("r3d_i2p_copy_channels", LV, img, 96, C192, 192, 0, st)
        _lib.call("r3d_i2p_copy_channels", LV, img, 96, C352, 352, 256, st)

        # HighResoEncoder (high_resolution_encoder.py:28-36)
        if x_in is not None:
            _lib.call("r3d_i2p_nchw_to_cl", x_in, B, cin, S, S, w["xcl"], st)
        _lib.call("r3d_secc_conv", w["xcl"], B, S, S, cin, d["high_reso_encoder.first"], hv.first.bias, 64, 7, 2, 3, None, None, 0.0, A, st)
        self._conv3(d, "high_reso_encoder.conv_layers.0", A, B, s2, 64, 1, 0.01, Bf, st)
        self._conv3(d, "high_reso_encoder.conv_layers.2", Bf, B, s2, 96, 1, 0.01, A, st)
        self._conv3(d, "high_reso_encoder.conv_layers.4", A, B, s2, 96, 1, 0.01, Bf, st)
        self._conv3(d, "high_reso_encoder.conv_layers.6", Bf, B, s2, 96, 1, 0.01, A, st)
        self._conv3(d, "high_reso_encoder.final", A, B, s2, 96, 0, 0.0, Bf, st)
        tap("feat_high", Bf, (B, s2, s2, 96))
        _lib.call("r3d_i2p_copy_channels", Bf, img, 96, C192, 192, 96, st)

        # TriplanePredictorViT (models.py:151-183)
        self._conv3(d, "triplane_predictor_vit.first_conv", C192, B, s2, 192, 1, 0.01, A, st)
        self._conv3(d, "triplane_predictor_vit.second_conv", A, B, s2, 256, 1, 0.01, Bf, st)
        pe = pv.patch_embed
        _lib.call("r3d_secc_conv", Bf, B, s2, s2, 128, d["triplane_predictor_vit.patch_embed.proj"], pe.proj.bias, DIM, 3, 2, 1, pe.norm.weight,
                  pe.norm.bias, pe.norm.eps, X, st)
        for i in range(1, pv.num_blocks + 1):
            self._block(d, "triplane_predictor_vit.block%d" % i, w, B, s4, st)
        tap("predictor_tokens", X, (B, s4, s4, DIM))
        _lib.call("r3d_i2p_pixel_shuffle", X, B, s4, s4, 256, C352, 352, 0, st)
        self._conv3(d, "triplane_predictor_vit.first_conv_after_cat", C352, B, s2, 352, 1, 0.01, A, st)
        self._conv3(d, "triplane_predictor_vit.second_conv_after_cat", A, B, s2, 256, 1, 0.01, Bf, st)
        self._conv3(d, "triplane_predictor_vit.third_conv_after_cat", Bf, B, s2, 128, 1, 0.01, A, st)
        self._conv3(d, "triplane_predictor_vit.final_conv", A, B, s2, 128, 0, 0.0, OUT, st)
        planes = torch.empty(B, 3, self.out_channels // 3, s2, s2, device=dev, dtype=torch.float32)
        _lib.call("r3d_i2p_planes_out", OUT, B, s2, s2, self.out_channels // 3, planes, st)
        return planes

    def _fast_encoder(self):
        """This package's DeepLabV3 as low_reso_encoder, of this model's input width and 256 output channels (and _r3d_fast_path not
        switched off, which tests do to compare the two routes): the encoder the fast path drives channel-last."""
        from .deeplabv3 import DeepLabV3
        enc = self.low_reso_encoder
        if (isinstance(enc, DeepLabV3) and enc.in_channels == self.in_channels and enc.out_channels == 256
                and getattr(self, "_r3d_fast_path", True)):
            return enc
        return None

    def _forward_fast(self, enc, x, cond, B, S, taps):
        """r3d_dl_assemble_input -> "xcl", enc.forward_cl -> "fl", then the launches without their two layout conversions.  The alpha
        threshold and the camera Linear stay torch (a re-ordered mean could flip a borderline pixel; the Linear is 75 products)."""
        x = x.detach().float().contiguous()
        alpha = cam = None
        if "alpha" in self.input_mode:
            if cond is None or cond.get("ref_alphas") is None:
                alpha = (x.mean(dim=1, keepdim=True) >= -0.999).float()
            else:
                alpha = cond["ref_alphas"].detach().float().contiguous()
        if "camera" in self.input_mode:
            cam = self.camera_to_channel(cond["ref_cameras"].detach().float()).reshape(B, 3).contiguous()
        cin = self.in_channels
        with self._device_of(x):
            w = self._buffers_for(x.device, B, S, cin)
            _lib.call("r3d_dl_assemble_input", x, alpha, cam, B, S, S, w["xcl"], torch.cuda.current_stream().cuda_stream)
            fl = enc.forward_cl(w["xcl"][:B * S * S * cin].view(B, S, S, cin), out=w["fl"])
            if taps is not None:
                taps["feat_low"] = fl.permute(0, 3, 1, 2).contiguous()
            return self._launches(x.device, B, cin, S, None, None, taps)

    def _forward(self, x, cond, taps):
        B, S = self._check(x, cond)
        enc = self._fast_encoder()
        if enc is not None:
            return self._forward_fast(enc, x, cond, B, S, taps)
        x_in = self.assemble_input(x.detach().float(), cond).contiguous()
        feat_low = self.low_reso_encoder(x_in)
        if not torch.is_tensor(feat_low) or tuple(feat_low.shape) != (B, 256, S // 8, S // 8):
            raise ValueError("Img2PlaneModel: low_reso_encoder must return [B, 256, S/8, S/8] = %s, got %s"
                             % ((B, 256, S // 8, S // 8), tuple(feat_low.shape) if torch.is_tensor(feat_low) else type(feat_low)))
        feat_low = feat_low.detach().float().contiguous()
        if taps is not None:
            taps["feat_low"] = feat_low.clone()
        return self._run(x_in, feat_low, taps)

    @torch.no_grad()
    def forward(self, x, cond=None, **synthesis_kwargs):
        return self._forward(x, cond, None)

    @torch.no_grad()
    def _forward_taps(self, x, cond=None):
        """Not part of the interface: (planes, taps), the intermediate tensors in the reference's NCHW layouts (predictor_tokens as [B, 1024, S/4, S/4]), as new
        tensors; for tests and the timing script."""
        taps = {}
        return self._forward(x, cond, taps), taps

    @classmethod
    def from_reference(cls, ref):
        """A HIP copy of a constructed reference Img2PlaneModel: ref's own low_reso_encoder object, the other parameters copied (strict),
        the block counts read from what ref holds."""
        hp = dict(getattr(ref, "hparams", None) or {})
        hp["img2plane_input_mode"] = getattr(ref, "input_mode", hp.get("img2plane_input_mode", "rgb"))
        blocks = (ref.low_reso_vit.num_blocks, ref.triplane_predictor_vit.num_blocks)
        m = cls(out_channels=ref.triplane_predictor_vit.final_conv.out_channels, hp=hp, low_reso_encoder=ref.low_reso_encoder, _blocks=blocks)
        m.load_state_dict(ref.state_dict(), strict=True)
        dev = next(ref.parameters()).device
        return m.to(dev).eval()
