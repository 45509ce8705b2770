"""SegFormerSECC2PlaneBackbone (modules/real3d/segformer.py:672-731) in mode b0 on the HIP SECC encoder (r3d_secc_* of
include/r3d_hip.h): prenet, the MiT-b0 encoder and the SegFormerHead in exact fp32, then to_plane_cnn as a ConvStack.

The module keeps the reference's parameter names, so a reference checkpoint loads with strict=True.  INFERENCE ONLY (eval semantics:
DropPath / Dropout are identity, BatchNorm uses its running statistics); inputs are detached and no autograd graph is built.

    forward(x)          [B, in_dim, H, W] -> the reference's flipped planes [B, 3, 32, H/2, W/2]
    forward_features(x) -> the head output [B, 256, H/4, W/4]
    forward_raw(x)      -> the unflipped to_plane_cnn output [B, 96, H/2, W/2], for
                           ImportanceRenderer.prepare_planes(cano, add=raw, add_flip=SECC_PLANE_FLIPS)
"""
import torch
import torch.nn as nn

from . import _lib
from ._state import _FoldedModule
from .superresolution import Conv2d, ConvStack
from .synth import SECC_DIMS, SECC_HEADS, SECC_SR
from .token_blocks import Block, PatchEmbed, conv_weight_cl, mit_block

MAX_KEYS = 1024          # r3d_secc_attention's limit on L = (H/32)(W/32): inputs up to 1024^2


class _Prenet(nn.Module):
    """Conv2dLayer(in_dim, 3, 1) (modules/eg3ds/models/networks_stylegan2.py:139-190): parameters and the resample_filter buffer."""

    def __init__(self, in_dim):
        super().__init__()
        self.weight = nn.Parameter(torch.randn(3, in_dim, 1, 1))
        self.bias = nn.Parameter(torch.zeros(3))
        f = torch.tensor([1.0, 3.0, 3.0, 1.0])
        self.register_buffer("resample_filter", torch.outer(f, f) / 64.0)


class _MixVisionTransformer(nn.Module):
    """mit_b0's parameters (segformer.py:244-310, 407-413)."""

    def __init__(self):
        super().__init__()
        cin = 3
        for s, (C, sr) in enumerate(zip(SECC_DIMS, SECC_SR), 1):
            setattr(self, "patch_embed%d" % s, PatchEmbed(cin, C, 7 if s == 1 else 3, 4 if s == 1 else 2))
            setattr(self, "block%d" % s, nn.ModuleList([Block(C, 4 * C, sr) for _ in range(2)]))
            setattr(self, "norm%d" % s, nn.LayerNorm(C))
            cin = C


class _HeadMLP(nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.proj = nn.Linear(cin, 256)


class _ConvModule(nn.Module):
    """mmcv ConvModule(1024, 256, 1, norm_cfg=BN): conv without bias, BatchNorm2d, ReLU."""

    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(1024, 256, 1, bias=False)
        self.bn = nn.BatchNorm2d(256)


class _SegFormerHead(nn.Module):
    def __init__(self):
        super().__init__()
        for s, C in enumerate(SECC_DIMS, 1):
            setattr(self, "linear_c%d" % s, _HeadMLP(C))
        self.linear_fuse = _ConvModule()


class SegFormerSECC2PlaneBackbone(_FoldedModule):
    def __init__(self, mode="b0", out_channels=96, pncc_cond_mode="cano_src_tgt"):
        super().__init__()
        if mode != "b0":
            raise NotImplementedError("SegFormerSECC2PlaneBackbone: only mode 'b0' has a HIP encoder (got %r)" % (mode,))
        self.mode, self.pncc_cond_mode = mode, pncc_cond_mode
        self.in_dim = 9 if pncc_cond_mode == "cano_src_tgt" else 6
        self.prenet = _Prenet(self.in_dim)
        self.mix_vit = _MixVisionTransformer()
        self.fuse_head = _SegFormerHead()
        self.to_plane_cnn = ConvStack(Conv2d(256, 256, 3, 1, 1), nn.LeakyReLU(0.01), Conv2d(256, 256, 3, 1, 1), nn.LeakyReLU(0.01),
                                      Conv2d(256, 256, 3, 1, 1), nn.LeakyReLU(0.01), nn.UpsamplingBilinear2d(scale_factor=2.0),
                                      Conv2d(256, out_channels, 3, 1, 1))

    # ---- parameters in the kernels' layouts (_prepare: once per parameter version) -------------------------------------------------
    def _fold(self):
        mv, fh = self.mix_vit, self.fuse_head
        d = {"conv": {}}
        for s in range(1, 5):
            pe = getattr(mv, "patch_embed%d" % s)
            d["conv"]["pe%d" % s] = conv_weight_cl(pe.proj.weight)
            for j, blk in enumerate(getattr(mv, "block%d" % s)):
                if hasattr(blk.attn, "sr"):
                    d["conv"]["sr%d.%d" % (s, j)] = conv_weight_cl(blk.attn.sr.weight)
        # the head fold, in fp64: W'_i = W_fuse[:, block(i)] W_ci, const = sum_i W_fuse[:, block(i)] b_ci, BN -> scale, shift
        wf = fh.linear_fuse.conv.weight.detach().double()[:, :, 0, 0]
        const = torch.zeros(256, dtype=torch.float64, device=wf.device)
        for blk, s in enumerate((4, 3, 2, 1)):
            part = wf[:, 256 * blk:256 * (blk + 1)]
            lin = getattr(fh, "linear_c%d" % s).proj
            d["wfold%d" % s] = (part @ lin.weight.detach().double()).float().contiguous()
            const = const + part @ lin.bias.detach().double()
        bn = fh.linear_fuse.bn
        scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
        d["hconst"] = const.float().contiguous()
        d["bn_scale"] = scale.float().contiguous()
        d["bn_shift"] = (bn.bias.detach().double() - bn.running_mean.detach().double() * scale).float().contiguous()
        return d

    def _new_buffers(self, dev, B, H, W):
        n1 = B * (H // 4) * (W // 4)
        L = B * (H // 32) * (W // 32) * 64       # spatial-reduction output rows x C, the largest stage (C sr^2 = 2048 ... 256)
        e = lambda n: torch.empty(n, device=dev, dtype=torch.float32)
        return {"x": e(n1 * 32), "t": e(n1 * 32), "q": e(n1 * 32), "o": e(n1 * 32), "h1": e(n1 * 128), "h2": e(n1 * 128),
                "sr": e(L * 4), "kv": e(L * 8),
                "c": [e(n1 * 32), e(n1 // 4 * 64), e(n1 // 16 * 160), e(n1 // 64 * 256)],
                "f": [None, e(n1 // 4 * 256), e(n1 // 16 * 256), e(n1 // 64 * 256)]}

    # ---- the encoder ---------------------------------------------------------------------------------------------------------------
    def _check_input(self, x):
        if x.dim() != 4 or x.shape[1] != self.in_dim:
            raise ValueError("SegFormerSECC2PlaneBackbone: expected [B, %d, H, W], got %s" % (self.in_dim, tuple(x.shape)))
        B, _, H, W = x.shape
        if H % 32 or W % 32:
            raise NotImplementedError("SegFormerSECC2PlaneBackbone: H and W must be multiples of 32 (got %d x %d)" % (H, W))
        if (H // 32) * (W // 32) > MAX_KEYS:
            raise NotImplementedError("SegFormerSECC2PlaneBackbone: (H/32)(W/32) = %d keys > %d" % ((H // 32) * (W // 32), MAX_KEYS))
        return B, H, W

    def _encode(self, x, head=False):
        """Runs prenet + mix_vit on x's device and that device's current stream (the device rule of _FoldedModule); returns the stream's
        buffers, where the stage outputs c1..c4 stay as [B, h, w, C], or with `head` the fuse_head output."""
        B, H, W = self._check_input(x)
        self._check_device(x, "input")
        x = x.detach().float().contiguous()
        with self._device_of(x):
            st = torch.cuda.current_stream().cuda_stream
            d = self._prepare()
            w = self._buffers_for(x.device, B, H, W)
            self._stages(x, w, d, B, H, W, st)
            return self._head(w, d, B, H, W, st) if head else w

    def _stages(self, x, w, d, B, H, W, st):
        mv, X = self.mix_vit, w["x"]
        h, wd = H // 4, W // 4
        pe = mv.patch_embed1
        _lib.call("r3d_secc_embed1", x, B, self.in_dim, H, W, self.prenet.weight, self.prenet.bias, d["conv"]["pe1"], pe.proj.bias, pe.norm.weight,
                  pe.norm.bias, X, st)
        for s, (C, heads) in enumerate(zip(SECC_DIMS, SECC_HEADS), 1):
            if s > 1:
                pe, prev = getattr(mv, "patch_embed%d" % s), w["c"][s - 2]
                _lib.call("r3d_secc_conv", prev, B, h, wd, SECC_DIMS[s - 2], d["conv"]["pe%d" % s], pe.proj.bias, C, 3, 2, 1, pe.norm.weight,
                          pe.norm.bias, pe.norm.eps, X, st)
                h, wd = h // 2, wd // 2
            for j, blk in enumerate(getattr(mv, "block%d" % s)):
                mit_block("r3d_secc_attention", blk, d["conv"].get("sr%d.%d" % (s, j)), w, st, B, h, wd, C, 4 * C, heads)
            nrm = getattr(mv, "norm%d" % s)
            _lib.call("r3d_secc_layernorm", X, B * h * wd, C, nrm.weight, nrm.bias, nrm.eps, w["c"][s - 1], st)

    def _head(self, w, d, B, H, W, st):
        for s in (2, 3, 4):
            n = B * (H // 2 ** (s + 1)) * (W // 2 ** (s + 1))
            _lib.call("r3d_secc_linear", w["c"][s - 1], n, SECC_DIMS[s - 1], None, None, 0.0, d["wfold%d" % s], None, 256, 0, None, w["f"][s - 1], st)
        out = torch.empty(B, 256, H // 4, W // 4, device=w["x"].device, dtype=torch.float32)
        _lib.call("r3d_secc_head", w["c"][0], B, H // 4, W // 4, d["wfold1"], w["f"][1], w["f"][2], w["f"][3], d["hconst"], d["bn_scale"],
                  d["bn_shift"], out, st)
        return out

    @torch.no_grad()
    def forward_stages(self, x):
        """[c1, c2, c3, c4] NCHW (MixVisionTransformer.forward_features, segformer.py:377-410), as new tensors."""
        w = self._encode(x)
        (B, _, H, W), out = x.shape, []
        for s, C in enumerate(SECC_DIMS, 1):
            h, wd = H // (2 ** (s + 1)), W // (2 ** (s + 1))
            out.append(w["c"][s - 1][:B * h * wd * C].view(B, h, wd, C).permute(0, 3, 1, 2).contiguous())
        return out

    @torch.no_grad()
    def forward_features(self, x):
        """fuse_head(mix_vit(prenet(x))): [B, 256, H/4, W/4] NCHW fp32."""
        return self._encode(x, head=True)

    @torch.no_grad()
    def forward_raw(self, x):
        """to_plane_cnn(forward_features(x)): [B, out_channels, H/2, W/2], before the flips of segformer.py:721-729."""
        return self.to_plane_cnn(self.forward_features(x))

    @torch.no_grad()
    def forward(self, x):
        planes = self.forward_raw(x)
        planes = planes.view(len(planes), 3, -1, planes.shape[-2], planes.shape[-1])
        return torch.stack([torch.flip(planes[:, 0], [2]), torch.flip(planes[:, 1], [2]), torch.flip(planes[:, 2], [2, 3])], dim=1)

    @classmethod
    def from_reference(cls, ref):
        """A HIP copy of a constructed reference SegFormerSECC2PlaneBackbone in mode b0 (strict key copy)."""
        out_channels = ref.to_plane_cnn[-1].out_channels
        m = cls(mode=ref.mode, out_channels=out_channels, pncc_cond_mode=ref.pncc_cond_mode)
        m.load_state_dict(ref.state_dict(), strict=True)
        dev = next(ref.parameters()).device
        return m.to(dev).eval()
