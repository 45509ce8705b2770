"""The third module of the face-vid2vid torso network on the HIP torso kernels (r3d_torso_conv, r3d_torso_conv_pool, r3d_torso_conv_split
and r3d_torso_conv3d_res of include/r3d_hip.h):

    AppearanceFeatureExtractor  modules/real3d/facev2v_warp/network2.py:16-45: in_conv (7 x 7), two DownBlock2D, mid_conv (1 x 1) viewed
                                as a [N, 32, 16, H / 4, W / 4] volume, six ResBlock3D

in exact fp32 by default (precision='f32'), or with precision='bf16x3' with every convolution on the split-precision tier of
torso_precision.py.  It keeps the reference's attribute names and its 107 state_dict keys, so a reference checkpoint loads with strict=True.
WarpBasedTorsoModelMediaPipe.forward calls the module on every frame (model2.py:230) with a freshly concatenated input (:226-228), and so
does this one: every call computes, nothing is cached across calls.
INFERENCE ONLY (eval semantics: BatchNorm on its running statistics, no spectral norm: use_weight_norm=False); inputs are detached and no
autograd graph is built.  The BatchNorms are folded into the conv weights, biases and prologue vectors in fp64 once per parameter version
(_prepare), where mid_conv's rows are also put in the depth-major order of r3d_torso_conv_split.  The building blocks, the two BatchNorm
folds, the module base (_prepare, work buffers, from_reference) and the launch wrappers are torso_layers.py's.
"""
import torch
import torch.nn as nn

from .torso_layers import (LEAKY, NONE, _check_f32, _conv, _conv3d_res, _conv_pool, _conv_split, _ConvBlock, _kernel_weight, _kernel_weight3d,
                           _ResBlock, _TorsoModule, conv_layer, conv_weight64, fold_cna, fold_res_pair)
from .torso_precision import F32

C, DEPTH, DOWN, N_RES = 32, 16, (64, 128, 256), 6          # network2.py:27-30
LAUNCHES = 16          # library launches per forward: in_conv, two pooled convs, mid_conv, twelve Conv3d


class _DownBlock2D(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.layers = nn.Sequential(_ConvBlock(2, "CNA", cin, cout, 3), nn.AvgPool2d((2, 2)))


def fold_appearance(m, dtype=torch.float32):
    """The extractor's convolutions as kernel calls, folded in fp64 and rounded once to `dtype` (float64: the fold itself, for the tests).
    A dict:  in_conv: one r3d_torso_conv layer in fold_generator's format;  down: two r3d_torso_conv_pool layers (w [Cout, 3, 3, Cin], b;
    the BatchNorm is in the rows and the bias, ReLU and the pool are the kernel's);  mid: w [512, 1, 1, 256] and b with row d 32 + c = the
    reference's channel c 16 + d;  res: twelve r3d_torso_conv3d_res layers (w [32, 3, 3, 3, 32], b, ps / pt or None, act, res)."""
    f = lambda v: None if v is None else v.to(dtype).contiguous()
    d64 = lambda p: p.detach().double()
    F = {"in_conv": conv_layer(*fold_cna(m.in_conv, conv_weight64), 7, dtype, act=LEAKY), "down": [], "res": []}
    for blk in m.down:
        w, b = fold_cna(blk.layers[0], conv_weight64)
        F["down"].append({"w": _kernel_weight(w, dtype), "b": f(b)})
    cin = m.mid_conv.in_channels
    F["mid"] = {"w": _kernel_weight(d64(m.mid_conv.weight).view(m.C, m.D, cin, 1, 1).transpose(0, 1).reshape(m.C * m.D, cin, 1, 1), dtype),
                "b": f(d64(m.mid_conv.bias).view(m.C, m.D).t().reshape(-1))}
    for blk in m.res:
        (w1, b1, ps, pt), (w2, b2) = fold_res_pair(blk.layers[0], blk.layers[1], conv_weight64)
        F["res"] += [{"w": _kernel_weight3d(w1, dtype), "b": f(b1), "ps": f(ps), "pt": f(pt), "act": LEAKY, "res": False},
                     {"w": _kernel_weight3d(w2, dtype), "b": f(b2), "ps": None, "pt": None, "act": NONE, "res": True}]
    return F


class AppearanceFeatureExtractor(_TorsoModule):
    """network2.py:16-45.  forward(x [N, in_dim, H, W]) -> [N, 32, 16, H / 4, W / 4] (fp32, contiguous NCDHW: what the glue of
    model2.py:231-236 consumes).  The module is fully convolutional; H and W are multiples of 4 (two 2 x 2 pools)."""

    def __init__(self, in_dim=3, model_scale="standard", lora_args=None, precision=F32):
        super().__init__(precision)
        if lora_args is not None:
            raise NotImplementedError("AppearanceFeatureExtractor: lora_args has no HIP implementation (got %r)" % (lora_args,))
        self.in_dim = in_dim
        self.in_conv = _ConvBlock(2, "CNA", in_dim, DOWN[0], 7)
        self.down = nn.Sequential(*[_DownBlock2D(DOWN[i], DOWN[i + 1]) for i in range(len(DOWN) - 1)])
        self.mid_conv = nn.Conv2d(DOWN[-1], C * DEPTH, 1, 1, 0)
        self.res = nn.Sequential(*[_ResBlock(3, C) for _ in range(N_RES)])
        self.C, self.D = C, DEPTH

    def _fold(self):
        return fold_appearance(self)

    def _new_buffers(self, dev, N, H, W):
        e = lambda n: torch.empty(n, device=dev, dtype=torch.float32)
        px = N * H * W
        return {"a0": e(px * DOWN[0]), "a1": e(px // 4 * DOWN[1]), "a2": e(px // 16 * DOWN[2]), "x": e(px // 16 * C * DEPTH),
                "h": e(px // 16 * C * DEPTH)}

    def _run(self, x, channel_last):
        x = _check_f32(x, "AppearanceFeatureExtractor input", 4)
        N, cin, H, W = x.shape
        if cin != self.in_dim or N < 1 or H < 4 or W < 4 or H % 4 or W % 4:
            raise ValueError("AppearanceFeatureExtractor: expected [N, %d, H, W] with H and W positive multiples of 4, got %s"
                             % (self.in_dim, tuple(x.shape)))
        dev = x.device
        F, w, pr = self._prepare(), self._buffers_for(dev, N, H, W), self.precision
        h4, w4 = H // 4, W // 4
        _conv(x, N, H, W, cin, F["in_conv"], y=w["a0"], in_nchw=True, precision=pr)
        _conv_pool(w["a0"], N, H, W, DOWN[0], F["down"][0], w["a1"], pr)
        _conv_pool(w["a1"], N, H // 2, W // 2, DOWN[1], F["down"][1], w["a2"], pr)
        _conv_split(w["a2"], N, h4, w4, DOWN[2], F["mid"], DEPTH, w["x"], pr)
        out = None if channel_last else torch.empty(N, C, DEPTH, h4, w4, device=dev, dtype=torch.float32)
        X, Hb = w["x"], w["h"]
        for i in range(N_RES):
            _conv3d_res(X, N, DEPTH, h4, w4, C, F["res"][2 * i], None, Hb, None, pr)
            if i < N_RES - 1 or channel_last:
                _conv3d_res(Hb, N, DEPTH, h4, w4, C, F["res"][2 * i + 1], X, X, None, pr)
            else:
                _conv3d_res(Hb, N, DEPTH, h4, w4, C, F["res"][2 * i + 1], X, None, out, pr)
        return X.view(N, DEPTH, h4, w4, C) if channel_last else out

    @torch.no_grad()
    def forward(self, x):
        return self._run(x, False)

    @torch.no_grad()
    def forward_cl(self, x):
        """forward(x) as the channel-last volume [N, 16, H / 4, W / 4, 32] (bit for bit r3d_torso_volume_to_cl of forward's result): the
        same 16 launches, the last of which writes only its channel-last y, and no NCDHW store.  x [N, in_dim, H, W] as for forward, for
        instance the tensor r3d_torso_seg_input assembled.  The result is the module's work buffer of this (device, stream, N, H, W): the
        next call with that key overwrites it, so consume it on the same stream before calling again (torso_forward.py does)."""
        return self._run(x, True)

    @staticmethod
    def _reference_args(ref):
        return {"in_dim": ref.in_conv.layers[0].in_channels}


def is_reference_appearance_extractor(m):
    """The reference's AppearanceFeatureExtractor (network2.py:16-45; network.py's is the same module): in_conv 7 x 7 to 64 channels, two
    DownBlock2D, mid_conv to 32 x 16 channels, six ResBlock3D."""
    try:
        return (type(m).__name__ == "AppearanceFeatureExtractor" and not type(m).__module__.startswith("real3dportrait_amd")
                and m.in_conv.layers[0].out_channels == DOWN[0] and m.in_conv.layers[0].kernel_size == (7, 7) and len(m.down) == 2
                and type(m.down[0].layers[1]).__name__ == "AvgPool2d" and m.mid_conv.out_channels == C * DEPTH
                and m.mid_conv.kernel_size == (1, 1) and len(m.res) == N_RES and type(m.res[0].layers[0].layers[2]).__name__ == "Conv3d"
                and m.C == C and m.D == DEPTH)
    except (AttributeError, IndexError, TypeError):
        return False
