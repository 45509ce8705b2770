"""The second half of the face-vid2vid torso network on the HIP torso kernels (r3d_torso_* of include/r3d_hip.h):

    Generator            modules/real3d/facev2v_warp/network2.py:248-301 (network.py:240-298 is the same module): the trilinear warp of
                         the appearance volume, in_conv, mid_conv, six ResBlock2D, two UpBlock2D, out_conv
    Occlusion2Predictor  the nn.Sequential occlusion_2_predictor of WarpBasedTorsoModelMediaPipe (model2.py:212-219)

in exact fp32 by default (precision='f32'), or with precision='bf16x3' with every convolution on the split-precision tier of
torso_precision.py (the warp stays as it is).  Both keep the reference's attribute names and state_dict keys, so a reference checkpoint loads with strict=True.
INFERENCE ONLY (eval semantics: spectral norm without power iteration, BatchNorm on its running statistics); inputs are detached and
no autograd graph is built.  Spectral norm and the BatchNorms are folded into the conv weights, biases and prologue vectors in fp64
once per parameter version (_prepare).  The building blocks, the two BatchNorm folds, the module base (_prepare, work buffers,
from_reference) and the launch wrapper are torso_layers.py's, shared with the other torso modules.
"""
import torch
import torch.nn as nn

from . import _lib
from ._state import Derived, StreamBuffers
from .torso_layers import (LEAKY, SIGMOID, _check_f32, _conv, _ConvBlock, _ResBlock, _TorsoModule, conv_layer, conv_weight64, fold_cna,
                           fold_res_pair, sn_weight64)
from .torso_precision import F32


class _UpBlock2D(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.layers = nn.Sequential(nn.Upsample(scale_factor=(2, 2)), _ConvBlock(2, "CNA", cin, cout, 3, spectral=True))


def fold_generator(gen, dtype=torch.float32):
    """The Generator's convolutions as r3d_torso_conv calls, folded in fp64 and rounded once to `dtype` (float64: the fold itself, for
    the tests): a list of dicts with w [Cout, k, k, Cin], bias, ps / pt (the prologue of a "NAC" conv, or None), k, up, act, slope,
    res (the conv adds its block's input)."""
    L = [conv_layer(*fold_cna(gen.in_conv, sn_weight64), 3, dtype, act=LEAKY, slope=0.2),
         conv_layer(conv_weight64(gen.mid_conv), gen.mid_conv.bias.detach().double(), 1, dtype)]
    for blk in gen.res:
        (w1, b1, ps, pt), (w2, b2) = fold_res_pair(blk.layers[0], blk.layers[1], sn_weight64)
        L += [conv_layer(w1, b1, 3, dtype, ps=ps, pt=pt, act=LEAKY), conv_layer(w2, b2, 3, dtype, res=True)]
    L += [conv_layer(*fold_cna(up.layers[1], sn_weight64), 3, dtype, up=1, act=LEAKY) for up in gen.up]
    L.append(conv_layer(conv_weight64(gen.out_conv), gen.out_conv.bias.detach().double(), 7, dtype))
    return L


_VOLUME_CL = StreamBuffers(lambda dev: Derived())          # per stream: the channel-last copy of the appearance volume (constant over a clip)


class Generator(_TorsoModule):
    """network2.py:248-301.  forward(fs [N, 32, 16, H, W], deformation [N, 16, H, W, 3], occlusion) -> rgb [N, 3, 4H, 4W]
    (and hid [N, 64, 4H, 4W] with return_hid=True); `occlusion` is accepted and unused, as in the reference."""

    def __init__(self, input_channels=32, model_scale="standard", more_res=False, precision=F32):
        super().__init__(precision)
        if model_scale not in ("standard", "small") or more_res:
            raise NotImplementedError("Generator: only model_scale 'standard' / 'small' without more_res has a HIP implementation "
                                      "(network2.py:261-270; got %r, more_res=%r)" % (model_scale, more_res))
        C, D, up_seq = input_channels, 16, [256, 128, 64]
        self.input_channels, self.depth = C, D
        self.in_conv = _ConvBlock(2, "CNA", C * D, up_seq[0], 3, spectral=True, leaky=True)
        self.mid_conv = nn.Conv2d(up_seq[0], up_seq[0], 1, 1, 0)
        self.res = nn.Sequential(*[_ResBlock(2, up_seq[0], spectral=True) for _ in range(6)])
        self.up = nn.Sequential(*[_UpBlock2D(up_seq[i], up_seq[i + 1]) for i in range(2)])
        self.out_conv = nn.Conv2d(up_seq[-1], 3, 7, 1, 3)

    def _fold(self):
        return fold_generator(self)

    def _new_buffers(self, dev, N, H, W):
        e = lambda n: torch.empty(n, device=dev, dtype=torch.float32)
        px = N * H * W
        return {"warp": e(px * self.input_channels * self.depth), "x": e(px * 256), "h": e(px * 256), "u0": e(px * 4 * 128), "u1": e(px * 16 * 64)}

    @staticmethod
    def _warp_inputs(fs, deformation):
        key = fs          # the caller's tensor: detach() below returns a new object per call
        fs, grid = _check_f32(fs, "fs", 5), _check_f32(deformation, "deformation", 5)
        N, C, D, H, W = fs.shape
        if grid.shape[0] != N or grid.shape[4] != 3:
            raise ValueError("deformation: expected [%d, Do, Ho, Wo, 3], got %s" % (N, tuple(grid.shape)))
        Do, Ho, Wo = grid.shape[1:4]
        st = torch.cuda.current_stream().cuda_stream

        def to_cl():
            cl = torch.empty(N, D, H, W, C, device=fs.device, dtype=torch.float32)
            _lib.call("r3d_torso_volume_to_cl", fs, N, C, D, H, W, cl, st)
            return cl

        cl = _VOLUME_CL.get(fs.device).get([key], to_cl)
        return fs, grid, cl, (N, C, D, H, W, Do, Ho, Wo)

    @staticmethod
    @torch.no_grad()
    def get_deformed_feature(fs, deformation):
        """network2.py:297-301: grid_sample(fs, deformation, align_corners=True, padding_mode='border').view(N, -1, H, W)."""
        fs, grid, cl, (N, C, D, H, W, Do, Ho, Wo) = Generator._warp_inputs(fs, deformation)
        out = torch.empty(N, C, Do, Ho, Wo, device=fs.device, dtype=torch.float32)
        _lib.call("r3d_torso_warp", cl, N, C, D, H, W, grid, Do, Ho, Wo, out, 0)
        return out.view(N, -1, H, W)

    def _decode(self, x, in_nchw, N, H, W, return_hid):
        """in_conv .. out_conv on x = the deformed features [N, H, W, 512] (or NCHW)."""
        dev = x.device
        L = self._prepare()
        w = self._buffers_for(dev, N, H, W)
        X, Hb, pr = w["x"], w["h"], self.precision
        _conv(x, N, H, W, self.input_channels * self.depth, L[0], y=Hb, in_nchw=in_nchw, precision=pr)
        _conv(Hb, N, H, W, 256, L[1], y=X, precision=pr)
        for i in range(6):
            _conv(X, N, H, W, 256, L[2 + 2 * i], y=Hb, precision=pr)
            _conv(Hb, N, H, W, 256, L[3 + 2 * i], y=X, res=X, precision=pr)
        _conv(X, N, H, W, 256, L[14], y=w["u0"], precision=pr)
        hid = torch.empty(N, 64, 4 * H, 4 * W, device=dev, dtype=torch.float32) if return_hid else None
        _conv(w["u0"], N, 2 * H, 2 * W, 128, L[15], y=w["u1"], y_nchw=hid, precision=pr)
        rgb = torch.empty(N, 3, 4 * H, 4 * W, device=dev, dtype=torch.float32)
        _conv(w["u1"], N, 4 * H, 4 * W, 64, L[16], y_nchw=rgb, precision=pr)
        return (rgb, hid) if return_hid else rgb

    @torch.no_grad()
    def forward(self, fs, deformation, occlusion=None, return_hid=False):
        fs, grid, cl, (N, C, D, H, W, Do, Ho, Wo) = self._warp_inputs(fs, deformation)
        if C != self.input_channels or D != self.depth or (Do, Ho, Wo) != (D, H, W):
            raise ValueError("Generator: expected fs [N, %d, %d, H, W] and deformation [N, %d, H, W, 3], got %s and %s"
                             % (self.input_channels, self.depth, self.depth, tuple(fs.shape), tuple(grid.shape)))
        warped = self._buffers_for(fs.device, N, H, W)["warp"]
        _lib.call("r3d_torso_warp", cl, N, C, D, H, W, grid, Do, Ho, Wo, warped, 1)
        return self._decode(warped, False, N, H, W, return_hid)

    @torch.no_grad()
    def forward_cl(self, fs_cl, deformation, occlusion=None, return_hid=False):
        """forward with the appearance volume already channel-last, fs_cl [N, 16, H, W, 32] (what r3d_torso_volume_to_cl makes of forward's
        fs, for instance r3d_torso_mask_volume's masked_cl): straight to r3d_torso_warp, without the transpose and without _VOLUME_CL."""
        cl, grid = _check_f32(fs_cl, "fs_cl", 5), _check_f32(deformation, "deformation", 5)
        N, D, H, W, C = cl.shape
        if C != self.input_channels or D != self.depth or tuple(grid.shape) != (N, D, H, W, 3):
            raise ValueError("Generator: expected fs_cl [N, %d, H, W, %d] and deformation [N, %d, H, W, 3], got %s and %s"
                             % (self.depth, self.input_channels, self.depth, tuple(cl.shape), tuple(grid.shape)))
        warped = self._buffers_for(cl.device, N, H, W)["warp"]
        _lib.call("r3d_torso_warp", cl, N, C, D, H, W, grid, D, H, W, warped, 1)
        return self._decode(warped, False, N, H, W, return_hid)

    @torch.no_grad()
    def forward_with_deformed_feature(self, deformed_fs, occlusion=None, return_hid=False):
        x = _check_f32(deformed_fs, "deformed_fs", 4)
        N, C, H, W = x.shape
        if C != self.input_channels * self.depth:
            raise ValueError("Generator: expected deformed_fs [N, %d, H, W], got %s" % (self.input_channels * self.depth, tuple(x.shape)))
        return self._decode(x, True, N, H, W, return_hid)

    @staticmethod
    def _reference_args(ref):          # a constructed reference Generator at standard / small scale
        return {"input_channels": ref.in_conv.layers[0].in_channels // 16}


def is_reference_generator(g):
    """The reference Generator at standard / small scale: six residual blocks and two up blocks without the large scale's extra ones."""
    return (type(g).__name__ == "Generator" and not type(g).__module__.startswith("real3dportrait_amd") and hasattr(g, "in_conv")
            and len(getattr(g, "res", ())) == 6 and len(getattr(g, "up", ())) == 2 and type(g.up[0]).__name__ == "UpBlock2D"
            and type(g.up[1]).__name__ == "UpBlock2D")


class Occlusion2Predictor(_TorsoModule):
    """occlusion_2_predictor (model2.py:212-219): Conv2d(65, 32, 3, 1, 1), ReLU, Conv2d(32, 32, 3, 1, 1), ReLU, Conv2d(32, 1, 3, 1, 1),
    Sigmoid, with the nn.Sequential's keys ('0.weight', ..., '4.bias').  Called with cat([hid, occlusion_2 at 256^2]) [N, 65, H, W]."""

    def __init__(self, in_channels=65, hidden=32, precision=F32):
        super().__init__(precision)
        for i, (ci, co) in zip((0, 2, 4), ((in_channels, hidden), (hidden, hidden), (hidden, 1))):
            self.add_module(str(i), nn.Conv2d(ci, co, 3, 1, 1))

    def _fold(self):
        convs = [getattr(self, str(i)) for i in (0, 2, 4)]
        return [conv_layer(conv_weight64(c), c.bias.detach(), 3, act=SIGMOID if c is convs[2] else LEAKY) for c in convs]

    def _new_buffers(self, dev, N, H, W):
        return [torch.empty(N * H * W * getattr(self, "0").out_channels, device=dev, dtype=torch.float32) for _ in range(2)]

    @torch.no_grad()
    def forward(self, x):
        x = _check_f32(x, "occlusion_2_predictor input", 4)
        N, C, H, W = x.shape
        L = self._prepare()
        if C != L[0]["w"].shape[3]:
            raise ValueError("occlusion_2_predictor: expected [N, %d, H, W], got %s" % (L[0]["w"].shape[3], tuple(x.shape)))
        w = self._buffers_for(x.device, N, H, W)
        out = torch.empty(N, 1, H, W, device=x.device, dtype=torch.float32)
        _conv(x, N, H, W, C, L[0], y=w[0], in_nchw=True, precision=self.precision)
        _conv(w[0], N, H, W, L[1]["w"].shape[3], L[1], y=w[1], precision=self.precision)
        _conv(w[1], N, H, W, L[2]["w"].shape[3], L[2], y_nchw=out, precision=self.precision)
        return out

    @staticmethod
    def _reference_args(seq):
        return {"in_channels": seq[0].in_channels, "hidden": seq[0].out_channels}


def is_reference_predictor(seq):
    kinds = [type(m).__name__ for m in seq] if type(seq).__name__ == "Sequential" else []
    return kinds == ["Conv2d", "ReLU", "Conv2d", "ReLU", "Conv2d", "Sigmoid"] and all(
        seq[i].kernel_size == (3, 3) and seq[i].stride == (1, 1) and seq[i].padding == (1, 1) for i in (0, 2, 4)) and seq[4].out_channels == 1
