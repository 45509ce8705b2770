"""The second half of the face-vid2vid torso network on the HIP torso kernels (r3d_torso_* of include/r3d_hip.h):

    Generator            modules/real3d/facev2v_warp/network2.py:248-301 (network.py:240-298 is the same module): the trilinear warp of
                         the appearance volume, in_conv, mid_conv, six ResBlock2D, two UpBlock2D, out_conv
    Occlusion2Predictor  the nn.Sequential occlusion_2_predictor of WarpBasedTorsoModelMediaPipe (model2.py:212-219)

in exact fp32 by default (precision='f32'), or with precision='bf16x3' with every convolution on the split-precision tier of
torso_precision.py (the warp stays as it is).  Both keep the reference's attribute names and state_dict keys, so a reference checkpoint loads with strict=True.
INFERENCE ONLY (eval semantics: spectral norm without power iteration, BatchNorm on its running statistics); inputs are detached and
no autograd graph is built.  Spectral norm and the BatchNorms are folded into the conv weights, biases and prologue vectors in fp64
once per parameter version (_prepare).
"""
import torch
import torch.nn as nn

from . import _lib
from .torso_precision import F32, PRECISIONS, check_precision

NONE, LEAKY, SIGMOID = 0, 1, 2          # r3d_torso_conv's `act`
BN_EPS = 1e-5


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


class _ConvBlock2D(nn.Module):
    """ConvBlock2D (layers.py:6-48) with spectral norm and SyncBatchNorm: `layers` holds the modules in the pattern's order."""

    def __init__(self, pattern, cin, cout, k, leaky=False):
        super().__init__()
        self.pattern = pattern
        norm = cout if pattern.find("C") < pattern.find("N") else cin
        mods = {"C": _SNConv(cin, cout, k), "N": nn.BatchNorm2d(norm, eps=BN_EPS), "A": nn.LeakyReLU(0.2) if leaky else nn.ReLU()}
        self.layers = nn.Sequential(*[mods[c] for c in pattern])

    conv = property(lambda self: self.layers[self.pattern.index("C")])
    bn = property(lambda self: self.layers[self.pattern.index("N")])


class _ResBlock2D(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.layers = nn.Sequential(_ConvBlock2D("NAC", c, c, 3), _ConvBlock2D("NAC", c, c, 3))


class _UpBlock2D(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.layers = nn.Sequential(nn.Upsample(scale_factor=(2, 2)), _ConvBlock2D("CNA", cin, cout, 3))


def _params_key(m):
    return tuple((p.data_ptr(), p._version) for p in m.parameters()) + tuple((b.data_ptr(), b._version) for b in m.buffers())


def sn_weight64(conv):
    """Eval-mode spectral norm in fp64: weight_orig / sigma, sigma = u . (W_mat v) (no power iteration in eval)."""
    w = conv.weight_orig.detach().double()
    sigma = torch.dot(conv.weight_u.detach().double(), w.reshape(w.shape[0], -1) @ conv.weight_v.detach().double())
    return w / sigma


def bn_affine64(bn):
    """Eval BatchNorm as y = s x + t, fp64."""
    s = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    return s, bn.bias.detach().double() - bn.running_mean.detach().double() * s


def _kernel_weight(w64, dtype=torch.float32):
    """[Cout, Cin, k, k] fp64 -> the kernels' [Cout, k, k, Cin] fp32."""
    return w64.permute(0, 2, 3, 1).contiguous().to(dtype)


def fold_generator(gen, dtype=torch.float32):
    """The Generator's convolutions as r3d_torso_conv calls, folded in fp64 and rounded once to `dtype` (float64: the fold itself, for
    the tests): a list of dicts with w [Cout, k, k, Cin], bias, ps / pt (the prologue of a "NAC" conv, or None), k, up, act, slope,
    res (the conv adds its block's input)."""
    L = []

    def layer(w, b, k, ps=None, pt=None, up=0, act=NONE, slope=0.0, res=False):
        f = lambda v: None if v is None else v.to(dtype).contiguous()
        L.append({"w": _kernel_weight(w, dtype), "b": f(b), "ps": f(ps), "pt": f(pt), "k": k, "up": up, "act": act, "slope": slope, "res": res})

    def cna(block, up, slope):          # conv, BatchNorm, activation: the BatchNorm goes into the weight rows and the bias
        s, t = bn_affine64(block.bn)
        layer(sn_weight64(block.conv) * s[:, None, None, None], block.conv.bias.detach().double() * s + t, 3, up=up, act=LEAKY, slope=slope)

    cna(gen.in_conv, 0, 0.2)
    layer(gen.mid_conv.weight.detach().double(), gen.mid_conv.bias.detach().double(), 1)
    for blk in gen.res:
        a, b = blk.layers[0], blk.layers[1]
        s1, t1 = bn_affine64(a.bn)
        s2, t2 = bn_affine64(b.bn)
        # the first conv's only reader is the second block's BatchNorm + ReLU: they go into its rows, bias and epilogue
        layer(sn_weight64(a.conv) * s2[:, None, None, None], a.conv.bias.detach().double() * s2 + t2, 3, ps=s1, pt=t1, act=LEAKY)
        layer(sn_weight64(b.conv), b.conv.bias.detach().double(), 3, res=True)
    for up in gen.up:
        cna(up.layers[1], 1, 0.0)
    layer(gen.out_conv.weight.detach().double(), gen.out_conv.bias.detach().double(), 7)
    return L


class _Cached:
    """value = fn(tensor), recomputed only when `tensor` is another object or was modified in place (the entry holds the tensor)."""

    def __init__(self):
        self._src, self._ver, self._val = None, None, None

    def get(self, t, fn):
        if self._src is not t or self._ver != t._version:
            self._val = fn(t)
            self._src, self._ver = t, t._version
        return self._val


_VOLUME_CL = {}          # stream -> _Cached: the channel-last copy of the appearance volume (constant over a clip)


def _conv(x, B, Hs, Ws, cin, L, y=None, y_nchw=None, in_nchw=False, res=None, precision=F32):
    """One r3d_torso_conv launch; a tier other than 'f32' goes through r3d_torso_conv_prec."""
    P = _lib.ptr
    args = (P(x), B, Hs, Ws, cin, int(in_nchw), L["up"], P(L["ps"]), P(L["pt"]), 0.0, P(L["w"]), P(L["b"]), L["w"].shape[0], L["k"], L["act"],
            L["slope"], P(res), P(y), P(y_nchw))
    if precision == F32:
        _lib.check(_lib.load().r3d_torso_conv(*args, _lib.stream_ptr()), "torso_conv")
    else:
        _lib.check(_lib.load().r3d_torso_conv_prec(*args, PRECISIONS[precision], _lib.stream_ptr()), "torso_conv_prec")


def _check_f32(t, what, dims):
    if not torch.is_tensor(t) or t.dim() != dims:
        raise ValueError("%s: expected a %d-D tensor" % (what, dims))
    return t.detach().float().contiguous()


class Generator(nn.Module):
    """network2.py:248-301.  forward(fs [N, 32, 16, H, W], deformation [N, 16, H, W, 3], occlusion) -> rgb [N, 3, 4H, 4W]
    (and hid [N, 64, 4H, 4W] with return_hid=True); `occlusion` is accepted and unused, as in the reference."""

    def __init__(self, input_channels=32, model_scale="standard", more_res=False, precision=F32):
        super().__init__()
        self.precision = check_precision(precision, "Generator: precision")
        if model_scale not in ("standard", "small") or more_res:
            raise NotImplementedError("Generator: only model_scale 'standard' / 'small' without more_res has a HIP implementation "
                                      "(network2.py:261-270; got %r, more_res=%r)" % (model_scale, more_res))
        C, D, up_seq = input_channels, 16, [256, 128, 64]
        self.input_channels, self.depth = C, D
        self.in_conv = _ConvBlock2D("CNA", C * D, up_seq[0], 3, leaky=True)
        self.mid_conv = nn.Conv2d(up_seq[0], up_seq[0], 1, 1, 0)
        self.res = nn.Sequential(*[_ResBlock2D(up_seq[0]) for _ in range(6)])
        self.up = nn.Sequential(*[_UpBlock2D(up_seq[i], up_seq[i + 1]) for i in range(2)])
        self.out_conv = nn.Conv2d(up_seq[-1], 3, 7, 1, 3)
        self._derived_key, self._derived = None, None
        self._work = {}          # (device, stream, N, H, W) -> activation buffers: two streams in flight never share one

    def _prepare(self):
        key = _params_key(self)
        if key != self._derived_key:
            with torch.no_grad():
                self._derived_key, self._derived = key, fold_generator(self)
        return self._derived

    def _buffers_for(self, N, H, W, dev):
        key = (dev, _lib.stream_ptr(), N, H, W)
        w = self._work.get(key)
        if w is None:
            e = lambda n: torch.empty(n, device=dev, dtype=torch.float32)
            px = N * H * W
            w = self._work[key] = {"warp": e(px * self.input_channels * self.depth), "x": e(px * 256), "h": e(px * 256), "u0": e(px * 4 * 128),
                                   "u1": e(px * 16 * 64)}
        return w

    @staticmethod
    def _warp_inputs(fs, deformation):
        key = fs          # the caller's tensor: detach() below returns a new object per call
        fs, grid = _check_f32(fs, "fs", 5), _check_f32(deformation, "deformation", 5)
        N, C, D, H, W = fs.shape
        if grid.shape[0] != N or grid.shape[4] != 3:
            raise ValueError("deformation: expected [%d, Do, Ho, Wo, 3], got %s" % (N, tuple(grid.shape)))
        Do, Ho, Wo = grid.shape[1:4]
        lib, P, st = _lib.load(), _lib.ptr, _lib.stream_ptr()

        def to_cl(_):
            cl = torch.empty(N, D, H, W, C, device=fs.device, dtype=torch.float32)
            _lib.check(lib.r3d_torso_volume_to_cl(P(fs), N, C, D, H, W, P(cl), st), "torso_volume_to_cl")
            return cl

        cl = _VOLUME_CL.setdefault(st, _Cached()).get(key, to_cl)
        return fs, grid, cl, (N, C, D, H, W, Do, Ho, Wo)

    @staticmethod
    @torch.no_grad()
    def get_deformed_feature(fs, deformation):
        """network2.py:297-301: grid_sample(fs, deformation, align_corners=True, padding_mode='border').view(N, -1, H, W)."""
        fs, grid, cl, (N, C, D, H, W, Do, Ho, Wo) = Generator._warp_inputs(fs, deformation)
        out = torch.empty(N, C, Do, Ho, Wo, device=fs.device, dtype=torch.float32)
        _lib.check(_lib.load().r3d_torso_warp(_lib.ptr(cl), N, C, D, H, W, _lib.ptr(grid), Do, Ho, Wo, _lib.ptr(out), 0, _lib.stream_ptr()),
                   "torso_warp")
        return out.view(N, -1, H, W)

    def _decode(self, x, in_nchw, N, H, W, return_hid):
        """in_conv .. out_conv on x = the deformed features [N, H, W, 512] (or NCHW)."""
        dev = x.device
        L = self._prepare()
        w = self._buffers_for(N, H, W, dev)
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
        warped = self._buffers_for(N, H, W, fs.device)["warp"]
        _lib.check(_lib.load().r3d_torso_warp(_lib.ptr(cl), N, C, D, H, W, _lib.ptr(grid), Do, Ho, Wo, _lib.ptr(warped), 1, _lib.stream_ptr()),
                   "torso_warp")
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
        warped = self._buffers_for(N, H, W, cl.device)["warp"]
        _lib.check(_lib.load().r3d_torso_warp(_lib.ptr(cl), N, C, D, H, W, _lib.ptr(grid), D, H, W, _lib.ptr(warped), 1, _lib.stream_ptr()),
                   "torso_warp")
        return self._decode(warped, False, N, H, W, return_hid)

    @torch.no_grad()
    def forward_with_deformed_feature(self, deformed_fs, occlusion=None, return_hid=False):
        x = _check_f32(deformed_fs, "deformed_fs", 4)
        N, C, H, W = x.shape
        if C != self.input_channels * self.depth:
            raise ValueError("Generator: expected deformed_fs [N, %d, H, W], got %s" % (self.input_channels * self.depth, tuple(x.shape)))
        return self._decode(x, True, N, H, W, return_hid)

    @classmethod
    def from_reference(cls, ref, precision=F32):
        """A HIP copy of a constructed reference Generator at standard / small scale (strict key copy)."""
        m = cls(input_channels=ref.in_conv.layers[0].in_channels // 16, precision=precision)
        m.load_state_dict(ref.state_dict(), strict=True)
        return m.to(next(ref.parameters()).device).eval()


def is_reference_generator(g):
    """The reference Generator at standard / small scale: six residual blocks and two up blocks without the large scale's extra ones."""
    return (type(g).__name__ == "Generator" and not type(g).__module__.startswith("real3dportrait_amd") and hasattr(g, "in_conv")
            and len(getattr(g, "res", ())) == 6 and len(getattr(g, "up", ())) == 2 and type(g.up[0]).__name__ == "UpBlock2D"
            and type(g.up[1]).__name__ == "UpBlock2D")


class Occlusion2Predictor(nn.Module):
    """occlusion_2_predictor (model2.py:212-219): Conv2d(65, 32, 3, 1, 1), ReLU, Conv2d(32, 32, 3, 1, 1), ReLU, Conv2d(32, 1, 3, 1, 1),
    Sigmoid, with the nn.Sequential's keys ('0.weight', ..., '4.bias').  Called with cat([hid, occlusion_2 at 256^2]) [N, 65, H, W]."""

    def __init__(self, in_channels=65, hidden=32, precision=F32):
        super().__init__()
        self.precision = check_precision(precision, "Occlusion2Predictor: precision")
        for i, (ci, co) in zip((0, 2, 4), ((in_channels, hidden), (hidden, hidden), (hidden, 1))):
            self.add_module(str(i), nn.Conv2d(ci, co, 3, 1, 1))
        self._derived_key, self._derived = None, None
        self._work = {}

    def _prepare(self):
        key = _params_key(self)
        if key != self._derived_key:
            with torch.no_grad():
                d = []
                for i in (0, 2, 4):
                    c = getattr(self, str(i))
                    d.append({"w": _kernel_weight(c.weight.detach().double()), "b": c.bias.detach().float().contiguous(), "ps": None, "pt": None,
                              "k": 3, "up": 0, "act": SIGMOID if i == 4 else LEAKY, "slope": 0.0, "res": False})
            self._derived_key, self._derived = key, d
        return self._derived

    @torch.no_grad()
    def forward(self, x):
        x = _check_f32(x, "occlusion_2_predictor input", 4)
        N, C, H, W = x.shape
        L = self._prepare()
        if C != L[0]["w"].shape[3]:
            raise ValueError("occlusion_2_predictor: expected [N, %d, H, W], got %s" % (L[0]["w"].shape[3], tuple(x.shape)))
        key = (x.device, _lib.stream_ptr(), N, H, W)
        w = self._work.get(key)
        if w is None:
            hid = L[0]["w"].shape[0]
            w = self._work[key] = [torch.empty(N * H * W * hid, device=x.device, dtype=torch.float32) for _ in range(2)]
        out = torch.empty(N, 1, H, W, device=x.device, dtype=torch.float32)
        _conv(x, N, H, W, C, L[0], y=w[0], in_nchw=True, precision=self.precision)
        _conv(w[0], N, H, W, L[1]["w"].shape[3], L[1], y=w[1], precision=self.precision)
        _conv(w[1], N, H, W, L[2]["w"].shape[3], L[2], y_nchw=out, precision=self.precision)
        return out

    @classmethod
    def from_reference(cls, seq, precision=F32):
        m = cls(seq[0].in_channels, seq[0].out_channels, precision=precision)
        m.load_state_dict(seq.state_dict(), strict=True)
        return m.to(seq[0].weight.device).eval()


def is_reference_predictor(seq):
    kinds = [type(m).__name__ for m in seq] if type(seq).__name__ == "Sequential" else []
    return kinds == ["Conv2d", "ReLU", "Conv2d", "ReLU", "Conv2d", "Sigmoid"] and all(
        seq[i].kernel_size == (3, 3) and seq[i].stride == (1, 1) and seq[i].padding == (1, 1) for i in (0, 2, 4)) and seq[4].out_channels == 1
