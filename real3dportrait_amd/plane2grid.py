"""Plane2GridModule (modules/real3d/img2plane_baseline.py:32-77), the SameBlock3d residual blocks that turn the canonical backbone's planes
into tri-grids (triplane_feature_type trigrid_v2), on the HIP library in exact fp32 (include/r3d_hip_plane2grid.h).

The module keeps the reference's attribute names and state_dict keys (res_blocks_3d.{i}.conv1|conv2.weight|bias,
res_blocks_3d.{i}.norm1|norm2.weight|bias, res_blocks_3d.{i}.alpha), so the reference's state_dict loads with strict=True.  INFERENCE ONLY:
inputs are detached.  One SameBlock3d is five launches and a statistics finalize per GroupNorm:

    r3d_torso_volume_to_cl      [3N, C, D, H, W] (the input as stored: channel (k c d)) -> channel-last [3N, D, H, W, C]   (first layer only)
    r3d_p2g_groupnorm_stats     norm1 as a per-sample (scale, shift)
    r3d_p2g_conv3d              conv1 over relu(scale x + shift), replicate padding
    r3d_p2g_groupnorm_stats     norm2
    r3d_p2g_conv3d              alpha conv2 (alpha folded into its weights and bias) + x

    forward(x)        [N, 3 C D, H, W] -> [N, 3 C D, H, W], a new contiguous tensor in the reference's channel order (k c d)
    forward_cl(x)     the same values as [N, 3, D, H, W, C], the layout r3d_planes_to_nhwc(depth=D) produces: a view of the stream's work
                      buffer, valid until the next call on this stream
    from_reference(m) a HIP copy of a constructed reference Plane2GridModule, or None when its width is not the renderer's 32
"""
import torch
import torch.nn as nn

from . import _lib
from ._state import _FoldedModule

CHANNELS = 32          # the renderer's feature width (OSGDecoder's input): the only C the reference's configurations use
GROUPS = 4             # SameBlock3d's nn.GroupNorm(4, C)


class SameBlock3d(nn.Module):
    """The parameters of the reference's SameBlock3d (img2plane_baseline.py:32-55); Plane2GridModule computes with them."""

    def __init__(self, in_features):
        super().__init__()
        self.conv1 = nn.Conv3d(in_features, in_features, 3, padding=1, padding_mode="replicate")
        self.conv2 = nn.Conv3d(in_features, in_features, 3, padding=1, padding_mode="replicate")
        self.norm1 = nn.GroupNorm(GROUPS, in_features, affine=True)
        self.norm2 = nn.GroupNorm(GROUPS, in_features, affine=True)
        self.alpha = nn.Parameter(torch.tensor([0.01]))


def conv3d_weight_cl(w):
    """[Cout, Cin, kd, kh, kw] -> the kernels' [Cout, kd, kh, kw, Cin] (depth-major taps, channel fastest), contiguous."""
    return w.detach().permute(0, 2, 3, 4, 1).contiguous()


def fold_alpha(conv_weight, conv_bias, alpha):
    """x + alpha conv2(h) as x + conv2'(h): (alpha weight, alpha bias), formed in fp64 and rounded to fp32 once."""
    a = alpha.detach().double().reshape(())
    return (conv_weight.detach().double() * a).float(), (conv_bias.detach().double() * a).float()


def groupnorm_scale_shift(x, groups, gamma, beta, eps):
    """nn.GroupNorm(groups, C, eps)(x) = scale x + shift, x [B, C, ...]: (scale, shift) [B, C] in x's dtype, the statistics r3d_p2g_groupnorm_stats
    computes (mean and biased variance per (sample, group), the variance clamped at 0).  Plain torch; for tests and the fp64 restatement."""
    B, C = x.shape[:2]
    g = x.reshape(B, groups, -1)
    mean, var = g.mean(dim=2), (g * g).mean(dim=2) - g.mean(dim=2) ** 2
    rstd = 1.0 / torch.sqrt(var.clamp_min(0) + eps)
    scale = gamma.view(1, C) * rstd.repeat_interleave(C // groups, dim=1)
    return scale, beta.view(1, C) - mean.repeat_interleave(C // groups, dim=1) * scale


def is_reference_plane2grid(m):
    """Is m the reference's Plane2GridModule (by class name and parts), and not this package's?"""
    return (type(m).__name__ == "Plane2GridModule" and not type(m).__module__.startswith("real3dportrait_amd")
            and all(hasattr(m, n) for n in ("res_blocks_3d", "triplane_depth", "in_out_dim")))


class Plane2GridModule(_FoldedModule):
    def __init__(self, triplane_depth=3, in_out_dim=96):
        super().__init__()
        if int(triplane_depth) != triplane_depth or triplane_depth < 1:
            raise ValueError("Plane2GridModule: triplane_depth = %r is not a positive integer" % (triplane_depth,))
        if in_out_dim != 3 * CHANNELS:
            raise NotImplementedError("Plane2GridModule: in_out_dim = %r: the HIP module is built for the renderer's width, 3 x %d channels"
                                      % (in_out_dim, CHANNELS))
        self.triplane_depth, self.in_out_dim = int(triplane_depth), in_out_dim
        self.num_layers_per_block = 1 if self.triplane_depth <= 3 else 2
        self.res_blocks_3d = nn.Sequential(*[SameBlock3d(in_out_dim // 3) for _ in range(self.num_layers_per_block)])

    # ---- parameters in the kernels' layouts (_prepare: once per parameter version) -------------------------------------------------
    def _fold(self):
        layers = []
        for blk in self.res_blocks_3d:
            w2, b2 = fold_alpha(blk.conv2.weight, blk.conv2.bias, blk.alpha)
            layers.append({"w1": conv3d_weight_cl(blk.conv1.weight.float()), "b1": blk.conv1.bias.detach().float().contiguous(),
                           "w2": conv3d_weight_cl(w2), "b2": b2.contiguous(),
                           "g1": blk.norm1.weight.detach().float().contiguous(), "be1": blk.norm1.bias.detach().float().contiguous(),
                           "g2": blk.norm2.weight.detach().float().contiguous(), "be2": blk.norm2.bias.detach().float().contiguous(),
                           "eps1": float(blk.norm1.eps), "eps2": float(blk.norm2.eps)})
        return layers

    def _new_buffers(self, dev, B, D, H, W):
        C = CHANNELS
        e = lambda n: torch.empty(n, device=dev, dtype=torch.float32)
        nws = _lib.call("r3d_p2g_groupnorm_stats_workspace_bytes", B, D, H, W, C, GROUPS)
        return {"x": e(B * D * H * W * C), "h": e(B * D * H * W * C), "scale": e(B * C), "shift": e(B * C),
                "ws": torch.empty(max(nws, 16), device=dev, dtype=torch.uint8), "nws": nws}

    # ---- checks ---------------------------------------------------------------------------------------------------------------------
    def _check(self, x):
        D, C = self.triplane_depth, CHANNELS
        if not torch.is_tensor(x) or x.dim() != 4 or x.shape[1] != 3 * C * D or x.shape[0] < 1 or x.shape[2] < 1 or x.shape[3] < 1:
            raise ValueError("Plane2GridModule: expected [N, %d, H, W] (3 planes x %d channels x depth %d), got %s"
                             % (3 * C * D, C, D, tuple(x.shape) if torch.is_tensor(x) else type(x)))
        if x.dtype != torch.float32:
            raise ValueError("Plane2GridModule: the input is %s, not float32" % (x.dtype,))
        if not x.is_contiguous():
            raise ValueError("Plane2GridModule: the input is not contiguous")
        self._check_device(x, "input")
        return x.shape[0], x.shape[2], x.shape[3]

    # ---- HIP ------------------------------------------------------------------------------------------------------------------------
    def _launches(self, x, N, H, W, y_ncdhw, taps):
        """The layers on x [N, 3 C D, H, W] = [3N, C, D, H, W]; the last conv writes y_ncdhw [3N, C, D, H, W] when given, the channel-last
        work buffer (returned) otherwise."""
        st = torch.cuda.current_stream().cuda_stream
        B, D, C = 3 * N, self.triplane_depth, CHANNELS
        layers = self._prepare()
        w = self._buffers_for(x.device, B, D, H, W)
        X, Hb = w["x"], w["h"]
        _lib.call("r3d_torso_volume_to_cl", x, B, C, D, H, W, X, st)
        stats = lambda t, gamma, beta, eps: _lib.call("r3d_p2g_groupnorm_stats", t, B, D, H, W, C, GROUPS, gamma, beta, eps, w["scale"], w["shift"],
                                                      w["ws"], w["nws"], st)
        for i, L in enumerate(layers):
            last = i == len(layers) - 1
            stats(X, L["g1"], L["be1"], L["eps1"])
            _lib.call("r3d_p2g_conv3d", X, B, D, H, W, C, w["scale"], w["shift"], L["w1"], L["b1"], C, None, Hb, None, st)
            if taps is not None:
                taps["conv1.%d" % i] = Hb[:B * D * H * W * C].view(B, D, H, W, C).permute(0, 4, 1, 2, 3).contiguous()
            stats(Hb, L["g2"], L["be2"], L["eps2"])
            if last and y_ncdhw is not None:
                _lib.call("r3d_p2g_conv3d", Hb, B, D, H, W, C, w["scale"], w["shift"], L["w2"], L["b2"], C, X, None, y_ncdhw, st)
            else:
                _lib.call("r3d_p2g_conv3d", Hb, B, D, H, W, C, w["scale"], w["shift"], L["w2"], L["b2"], C, X, X, None, st)      # in place on x
        return X

    def _forward(self, x, taps):
        N, H, W = self._check(x)
        x = x.detach()
        with self._device_of(x):
            y = torch.empty_like(x)
            self._launches(x, N, H, W, y, taps)
        return y

    @torch.no_grad()
    def forward(self, x):
        return self._forward(x, None)

    @torch.no_grad()
    def forward_cl(self, x):
        """[N, 3 C D, H, W] -> [N, 3, D, H, W, C]: a view of the stream's work buffer (valid until the next call on this stream)."""
        N, H, W = self._check(x)
        x = x.detach()
        with self._device_of(x):
            X = self._launches(x, N, H, W, None, None)
        return X[:3 * N * self.triplane_depth * H * W * CHANNELS].view(N, 3, self.triplane_depth, H, W, CHANNELS)

    @torch.no_grad()
    def _forward_taps(self, x):
        """Not part of the interface: (output, taps) with every layer's first conv output `conv1.<i>` [3N, C, D, H, W] as a new tensor;
        for tests and the timing script."""
        taps = {}
        return self._forward(x, taps), taps

    @classmethod
    def from_reference(cls, ref):
        """A HIP copy of a constructed reference Plane2GridModule, or None: its width must be the renderer's (in_out_dim 96) and every
        SameBlock3d what the reference builds (3 x 3 x 3 replicate-padded convs, GroupNorm(4) with affine parameters)."""
        try:
            if ref.in_out_dim != 3 * CHANNELS:
                return None
            m = cls(ref.triplane_depth, ref.in_out_dim)
            if len(ref.res_blocks_3d) != m.num_layers_per_block:
                return None
            for blk in ref.res_blocks_3d:
                for conv in (blk.conv1, blk.conv2):
                    if (not isinstance(conv, nn.Conv3d) or conv.padding_mode != "replicate" or tuple(conv.kernel_size) != (3, 3, 3)
                            or tuple(conv.stride) != (1, 1, 1) or tuple(conv.padding) != (1, 1, 1) or tuple(conv.dilation) != (1, 1, 1)
                            or conv.groups != 1 or conv.bias is None or conv.in_channels != CHANNELS or conv.out_channels != CHANNELS):
                        return None
                for norm in (blk.norm1, blk.norm2):
                    if not isinstance(norm, nn.GroupNorm) or norm.num_groups != GROUPS or norm.num_channels != CHANNELS or not norm.affine:
                        return None
            m.load_state_dict(ref.state_dict(), strict=True)
            for new, old in zip(m.res_blocks_3d, ref.res_blocks_3d):
                new.norm1.eps, new.norm2.eps = old.norm1.eps, old.norm2.eps
        except (AttributeError, TypeError, IndexError, RuntimeError, ValueError, NotImplementedError):
            return None
        return m.to(next(ref.parameters()).device).eval()
