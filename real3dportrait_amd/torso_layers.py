"""What the four HIP torso modules (torso_generator.py, torso_motion.py, torso_appearance.py, torso_forward.py) share: the reference's
building blocks with its state_dict keys, the fp64 folds of spectral norm and BatchNorm into kernel weights, the module base (folded
weights and work buffers kept by the rules of _state.py), and one launch wrapper per conv entry point
of include/r3d_hip.h (r3d_torso_conv, r3d_torso_conv3d, r3d_torso_conv_pool, r3d_torso_conv_split, r3d_torso_conv3d_res).
"""
import torch
import torch.nn as nn

from . import _lib
from ._state import _FoldedModule
from .torso_precision import F32, PRECISIONS, check_precision

NONE, LEAKY, SIGMOID = 0, 1, 2          # the conv entry points' `act`
BN_EPS = 1e-5


def _check_f32(t, what, dims):
    if not torch.is_tensor(t) or t.dim() != dims:
        raise ValueError("%s: expected a %d-D tensor" % (what, dims))
    return t.detach().float().contiguous()


def _pad4(c):
    return (c + 3) // 4 * 4


class _SNConv(nn.Module):
    """The parameters torch.nn.utils.spectral_norm leaves on a Conv2d (layers.py:4,12,30): bias, weight_orig, and the buffers weight_u,
    weight_v of the power iteration."""

    def __init__(self, cin, cout, k):
        super().__init__()
        self.in_channels, self.out_channels, self.kernel_size = cin, cout, (k, k)
        self.bias = nn.Parameter(torch.zeros(cout))
        self.weight_orig = nn.Parameter(torch.randn(cout, cin, k, k) * (cin * k * k) ** -0.5)
        self.register_buffer("weight_u", nn.functional.normalize(torch.randn(cout), dim=0))
        self.register_buffer("weight_v", nn.functional.normalize(torch.randn(cin * k * k), dim=0))


class _ConvBlock(nn.Module):
    """ConvBlock2D / ConvBlock3D (layers.py:6-55) with SyncBatchNorm: `layers` holds the modules in the pattern's order.  spectral: the
    conv carries spectral norm (2-D only, the Generator's blocks); the others have no weight norm."""

    def __init__(self, dim, pattern, cin, cout, k, spectral=False, leaky=False):
        super().__init__()
        self.pattern = pattern
        conv, norm = (nn.Conv2d, nn.BatchNorm2d) if dim == 2 else (nn.Conv3d, nn.BatchNorm3d)
        mods = {"C": _SNConv(cin, cout, k) if spectral else conv(cin, cout, k, 1, k // 2),
                "N": norm(cout if pattern.find("C") < pattern.find("N") else cin, eps=BN_EPS), "A": nn.LeakyReLU(0.2) if leaky else nn.ReLU()}
        self.layers = nn.Sequential(*[mods[c] for c in pattern])

    conv = property(lambda self: self.layers[self.pattern.index("C")])
    bn = property(lambda self: self.layers[self.pattern.index("N")])


class _ResBlock(nn.Module):
    """ResBlock2D / ResBlock3D: x + two "NAC" blocks."""

    def __init__(self, dim, c, spectral=False):
        super().__init__()
        self.layers = nn.Sequential(_ConvBlock(dim, "NAC", c, c, 3, spectral), _ConvBlock(dim, "NAC", c, c, 3, spectral))


def conv_weight64(conv):
    return conv.weight.detach().double()


def sn_weight64(conv):
    """Eval-mode spectral norm in fp64: weight_orig / sigma, sigma = u . (W_mat v) (no power iteration in eval)."""
    w = conv.weight_orig.detach().double()
    sigma = torch.dot(conv.weight_u.detach().double(), w.reshape(w.shape[0], -1) @ conv.weight_v.detach().double())
    return w / sigma


def bn_affine64(bn):
    """Eval BatchNorm as y = s x + t, fp64."""
    s = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    return s, bn.bias.detach().double() - bn.running_mean.detach().double() * s


def _rows(s, w):
    return s.reshape(-1, *[1] * (w.dim() - 1))


def fold_cna(block, weight64):
    """A "CNA" block (conv, BatchNorm, activation) as (w, b) in fp64: the BatchNorm goes into the weight rows and the bias.  weight64: the
    conv's fp64 weight (conv_weight64, or sn_weight64 under spectral norm)."""
    s, t = bn_affine64(block.bn)
    w = weight64(block.conv)
    return w * _rows(s, w), block.conv.bias.detach().double() * s + t


def fold_res_pair(a, b, weight64):
    """The two "NAC" blocks of a ResBlock as ((w, b, ps, pt), (w, b)) in fp64.  The first conv's only reader is the second block's
    BatchNorm + ReLU: they go into its rows, bias and epilogue; its own BatchNorm + ReLU are its prologue (ps, pt)."""
    s1, t1 = bn_affine64(a.bn)
    s2, t2 = bn_affine64(b.bn)
    w = weight64(a.conv)
    return (w * _rows(s2, w), a.conv.bias.detach().double() * s2 + t2, s1, t1), (weight64(b.conv), b.conv.bias.detach().double())


def _kernel_weight(w64, dtype=torch.float32):
    """[Cout, Cin, k, k] fp64 -> the kernels' [Cout, k, k, Cin] fp32."""
    return w64.permute(0, 2, 3, 1).contiguous().to(dtype)


def _kernel_weight3d(w64, dtype, groups=None):
    """[Cout, Cin, kd, kh, kw] fp64 -> the kernel's [Cout, kd, kh, kw, Cin'] in `dtype`; groups: the sizes of the input's channel groups,
    each padded with zero columns to a multiple of 4 (default: the whole input as one group)."""
    w = w64.permute(0, 2, 3, 4, 1)
    parts, c0 = [], 0
    for c in groups or [w.shape[-1]]:
        parts.append(w[..., c0:c0 + c])
        if _pad4(c) != c:
            parts.append(w.new_zeros(w.shape[:-1] + (_pad4(c) - c,)))
        c0 += c
    assert c0 == w.shape[-1]
    return torch.cat(parts, dim=-1).contiguous().to(dtype)


def conv_layer(w, b, k, dtype=torch.float32, ps=None, pt=None, up=0, act=NONE, slope=0.0, res=False):
    """One r3d_torso_conv call as the dict _conv reads: w [Cout, k, k, Cin], bias, ps / pt (the prologue of a "NAC" conv, or None), k, up,
    act, slope, res (the conv adds its block's input); the tensors rounded once to `dtype`."""
    f = lambda v: None if v is None else v.to(dtype).contiguous()
    return {"w": _kernel_weight(w, dtype), "b": f(b), "ps": f(ps), "pt": f(pt), "k": k, "up": up, "act": act, "slope": slope, "res": res}


class _TorsoModule(_FoldedModule):
    """The host side every HIP torso module has: the derived (folded) weights and the work buffers per (device, stream, *shape), both by
    the rules of _state.py; from_reference.  A subclass supplies _fold() -> the derived weights, _new_buffers(dev, *shape) -> the buffers,
    and _reference_args(ref) -> the constructor arguments of a HIP copy of the reference module `ref`."""

    def __init__(self, precision):
        super().__init__()
        self.precision = check_precision(precision, "%s: precision" % type(self).__name__)

    @classmethod
    def from_reference(cls, ref, precision=F32):
        """A HIP copy of a constructed reference module (strict key copy)."""
        m = cls(precision=precision, **cls._reference_args(ref))
        m.load_state_dict(ref.state_dict(), strict=True)
        return m.to(next(ref.parameters()).device).eval()


# ---- one wrapper per conv entry point.  f32 goes through r3d_torso_conv / r3d_torso_conv3d, another tier through their _prec forms.

def _conv(x, B, Hs, Ws, cin, L, y=None, y_nchw=None, in_nchw=False, res=None, precision=F32):
    args = (x, B, Hs, Ws, cin, int(in_nchw), L["up"], L["ps"], L["pt"], 0.0, L["w"], L["b"], L["w"].shape[0], L["k"], L["act"], L["slope"], res, y, y_nchw)
    if precision == F32:
        _lib.call("r3d_torso_conv", *args)
    else:
        _lib.call("r3d_torso_conv_prec", *args, PRECISIONS[precision])


def _conv3d(x, B, D, Hs, Ws, cin, L, k, y, ycs=None, yco=0, up=0, act=NONE, pool=0, full_depth=0, y_ncdhw=None, precision=F32):
    cout = L["w"].shape[0]
    args = (x, B, D, Hs, Ws, cin, up, L["w"], L["b"], cout, k, full_depth, act, 0.0, pool, y, cout if ycs is None else ycs, yco, y_ncdhw)
    if precision == F32:
        _lib.call("r3d_torso_conv3d", *args)
    else:
        _lib.call("r3d_torso_conv3d_prec", *args, PRECISIONS[precision])


def _conv_pool(x, B, Hs, Ws, cin, L, y, precision):
    _lib.call("r3d_torso_conv_pool", x, B, Hs, Ws, cin, 0, L["w"], L["b"], L["w"].shape[0], 3, LEAKY, 0.0, 1, y, PRECISIONS[precision])


def _conv_split(x, B, Hs, Ws, cin, L, depth, y, precision):
    _lib.call("r3d_torso_conv_split", x, B, Hs, Ws, cin, 0, L["w"], L["b"], L["w"].shape[0], 1, NONE, 0.0, depth, y, PRECISIONS[precision])


def _conv3d_res(x, B, D, Hs, Ws, cin, L, res, y, y_ncdhw, precision):
    _lib.call("r3d_torso_conv3d_res", x, B, D, Hs, Ws, cin, L["ps"], L["pt"], 0.0, L["w"], L["b"], L["w"].shape[0], 3, L["act"], 0.0, res, y, y_ncdhw,
              PRECISIONS[precision])
