"""DeepLabV3 (modules/img2plane/deeplabv3/decoders/my_model.py), the low-resolution encoder of Img2PlaneModel, on the HIP library: a
BasicBlock ResNet dilated to output stride 8 (encoders/resnet.py, encoders/_utils.py:40-47), ASPP with rates 12 / 24 / 36 and one 3 x 3
conv (decoders/my_decoder.py) in exact fp32 (include/r3d_hip_deeplab.h).

The module keeps the reference's attribute names and state_dict keys (num_batches_tracked included), so the reference's state_dict loads
with strict=True.  Nothing here fetches weights: encoder_weights other than None is refused.  INFERENCE ONLY: BatchNorm uses its running
statistics (folded into the conv's weight and bias once per parameter version), Dropout is the identity, inputs are detached.

    forward(x)                  [B, Cin, H, W] -> [B, 256, H/8, W/8]
    forward_cl(x_cl, out=None)  the same on channel-last [B, H, W, Cin] -> [B, H/8, W/8, 256] (written into `out` when given)
    from_reference(m)           a HIP copy of a constructed reference DeepLabV3, or None when m's geometry is not the one built here
"""
import torch
import torch.nn as nn

from . import _lib
from ._state import _FoldedModule
from .token_blocks import conv_weight_cl

LAYERS = {"resnet18": (2, 2, 2, 2), "resnet34": (3, 4, 6, 3)}          # BasicBlock encoders (encoders/resnet.py:126-144)
PLANES = (64, 128, 256, 512)
ATROUS_RATES = (12, 24, 36)
OUTPUT_STRIDE = 8
# make_dilated(8) (encoders/_base.py:41-65): EVERY conv of layer3 gets stride 1, dilation 2, padding (k // 2) 2; of layer4, dilation 4
STAGE_DILATION = (1, 1, 2, 4)


class _BasicBlock(nn.Module):
    """torchvision's BasicBlock (its parameters and geometry; relu(bn2(conv2(relu(bn1(conv1(x))))) + downsample(x)))."""

    def __init__(self, inplanes, planes, stride, dilation):
        super().__init__()
        s, d = (1, dilation) if dilation > 1 else (stride, 1)
        self.conv1 = nn.Conv2d(inplanes, planes, 3, s, d, d, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, 1, d, d, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = None
        if stride != 1 or inplanes != planes:
            self.downsample = nn.Sequential(nn.Conv2d(inplanes, planes, 1, s, 0, d, bias=False), nn.BatchNorm2d(planes))


class _Encoder(nn.Module):
    def __init__(self, name, in_channels):
        super().__init__()
        self.conv1 = nn.Conv2d(in_channels, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        inplanes = 64
        for i, (planes, n, dil) in enumerate(zip(PLANES, LAYERS[name], STAGE_DILATION)):
            blocks = [_BasicBlock(inplanes if j == 0 else planes, planes, (1 if i == 0 else 2) if j == 0 else 1, dil) for j in range(n)]
            setattr(self, "layer%d" % (i + 1), nn.Sequential(*blocks))
            inplanes = planes
        self.output_stride = OUTPUT_STRIDE


class _ASPP(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        convs = [nn.Sequential(nn.Conv2d(cin, cout, 1, bias=False), nn.ReLU())]
        convs += [nn.Sequential(nn.Conv2d(cin, cout, 3, padding=r, dilation=r, bias=False), nn.ReLU()) for r in ATROUS_RATES]
        convs.append(nn.Sequential(nn.AdaptiveAvgPool2d(1), nn.Conv2d(cin, cout, 1, bias=False), nn.ReLU()))
        self.convs = nn.ModuleList(convs)
        self.project = nn.Sequential(nn.Conv2d(5 * cout, cout, 1, bias=False), nn.ReLU(), nn.Dropout(0.5))


def conv_geometry(m):
    """What r3d_dl_conv needs to know of an nn.Conv2d, or None when it is not a square, ungrouped, zero-padded, bias-free one."""
    if not isinstance(m, nn.Conv2d) or m.groups != 1 or m.bias is not None or getattr(m, "padding_mode", "zeros") != "zeros":
        return None
    pair = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v, v)
    k, s, p, d = pair(m.kernel_size), pair(m.stride), pair(m.padding), pair(m.dilation)
    if any(a != b or not isinstance(a, int) for a, b in (k, s, p, d)):
        return None
    return (m.in_channels, m.out_channels, k[0], s[0], p[0], d[0])


def fold_batchnorm(conv_weight, bn):
    """eval BatchNorm2d after a bias-free conv as (weight [Cout, Cin, k, k], bias [Cout]), formed in fp64 and rounded to fp32 once:
    scale = gamma / sqrt(running_var + eps), weight' = weight scale, bias' = beta - running_mean scale."""
    scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    w = conv_weight.detach().double() * scale.view(-1, 1, 1, 1)
    b = bn.bias.detach().double() - bn.running_mean.detach().double() * scale
    return w.float(), b.float()


def is_reference_deeplabv3(m):
    """Is m the reference's DeepLabV3 (by class name and parts), and not this package's?"""
    return (type(m).__name__ == "DeepLabV3" and not type(m).__module__.startswith("real3dportrait_amd")
            and all(hasattr(m, n) for n in ("encoder", "decoder")) and hasattr(getattr(m, "encoder", None), "layer4"))


class DeepLabV3(_FoldedModule):
    def __init__(self, encoder_name="resnet34", encoder_depth=5, encoder_weights=None, decoder_channels=256, in_channels=5):
        super().__init__()
        if encoder_name not in LAYERS:
            raise NotImplementedError("DeepLabV3: encoder %r is not a BasicBlock ResNet (%s)" % (encoder_name, ", ".join(sorted(LAYERS))))
        if encoder_weights is not None:
            raise ValueError("DeepLabV3: encoder_weights=%r: this package fetches no weights; construct with None and load a state_dict"
                             % (encoder_weights,))
        if encoder_depth != 5:
            raise NotImplementedError("DeepLabV3: encoder_depth %r is not 5" % (encoder_depth,))
        if in_channels < 1 or decoder_channels < 1:
            raise ValueError("DeepLabV3: in_channels = %r and decoder_channels = %r must be positive" % (in_channels, decoder_channels))
        self.encoder_name, self.in_channels, self.out_channels = encoder_name, in_channels, decoder_channels
        self.encoder = _Encoder(encoder_name, in_channels)
        self.decoder = nn.Sequential(_ASPP(PLANES[-1], decoder_channels), nn.Conv2d(decoder_channels, decoder_channels, 3, padding=1, bias=False))

    # ---- parameters in the kernels' layouts (_prepare: once per parameter version) -------------------------------------------------
    def _blocks(self):
        for i in range(1, 5):
            for j, blk in enumerate(getattr(self.encoder, "layer%d" % i)):
                yield "encoder.layer%d.%d" % (i, j), blk

    def _fold(self):
        d = {}

        def put(key, conv, bn):
            w, b = fold_batchnorm(conv.weight, bn)
            d[key] = (conv_weight_cl(w), b.contiguous())
        put("encoder.conv1", self.encoder.conv1, self.encoder.bn1)
        for key, blk in self._blocks():
            put(key + ".conv1", blk.conv1, blk.bn1)
            put(key + ".conv2", blk.conv2, blk.bn2)
            if blk.downsample is not None:
                put(key + ".downsample", blk.downsample[0], blk.downsample[1])
        aspp, C = self.decoder[0], self.out_channels
        for i in range(4):
            d["aspp.%d" % i] = conv_weight_cl(aspp.convs[i][0].weight.detach())
        d["aspp.4"] = conv_weight_cl(aspp.convs[4][1].weight.detach())
        wp = aspp.project[0].weight.detach()          # [C, 5 C, 1, 1]: the four conv branches, then the pooled branch
        d["project"] = wp[:, :4 * C, 0, 0].contiguous()
        d["project.pooled"] = wp[:, 4 * C:, 0, 0].contiguous()
        d["final"] = conv_weight_cl(self.decoder[1].weight.detach())
        return d

    def _new_buffers(self, dev, B, H, W, cin):
        e = lambda n: torch.empty(n, device=dev, dtype=torch.float32)
        h2, w2, h8, w8, C = H // 2, W // 2, H // 8, W // 8, self.out_channels
        stage = B * max((H // 4) * (W // 4) * PLANES[0], h8 * w8 * PLANES[-1])
        return {"xcl": e(B * H * W * cin), "stem": e(B * h2 * w2 * 64), "x": e(stage), "t": e(stage), "y": e(stage),
                "cat": e(B * h8 * w8 * 4 * C), "pooled": e(B * PLANES[-1]), "pf": e(B * C), "pbias": e(B * C), "aspp": e(B * h8 * w8 * C),
                "out": e(B * h8 * w8 * C)}

    # ---- checks ---------------------------------------------------------------------------------------------------------------------
    def check_input_shape(self, h, w):
        """my_model.py:76-86."""
        s = OUTPUT_STRIDE
        if h % s != 0 or w % s != 0:
            new_h = (h // s + 1) * s if h % s != 0 else h
            new_w = (w // s + 1) * s if w % s != 0 else w
            raise RuntimeError("Wrong input shape height=%d, width=%d. Expected image height and width divisible by %d. Consider pad your "
                               "images to shape (%d, %d)." % (h, w, s, new_h, new_w))

    def _check(self, x, layout):
        ci = 1 if layout == "NCHW" else 3
        if not torch.is_tensor(x) or x.dim() != 4 or x.shape[ci] != self.in_channels or x.shape[0] < 1:
            raise ValueError("DeepLabV3: expected %s with %d channels, got %s" % (layout, self.in_channels, tuple(x.shape) if torch.is_tensor(x) else type(x)))
        H, W = (x.shape[2], x.shape[3]) if layout == "NCHW" else (x.shape[1], x.shape[2])
        if H < 1 or W < 1:
            raise ValueError("DeepLabV3: empty image %d x %d" % (H, W))
        self.check_input_shape(H, W)
        self._check_device(x, "input", self.encoder.conv1.weight)
        return x.shape[0], H, W

    # ---- HIP ------------------------------------------------------------------------------------------------------------------------
    def _launches(self, x_cl, B, H, W, out, taps):
        st = torch.cuda.current_stream().cuda_stream
        d = self._prepare()
        w = self._buffers_for(x_cl.device, B, H, W, self.in_channels)
        C = self.out_channels
        conv = lambda x, h, wd, cin, wt, bias, bs, cout, k, s, dil, pad, res, act, y, ycs, yco: \
            _lib.call("r3d_dl_conv", x, B, h, wd, cin, wt, bias, bs, cout, k, s, dil, pad, res, act, y, ycs, yco, st)
        tap = (lambda name, t, shape: taps.__setitem__(name, t[:shape[0] * shape[1] * shape[2] * shape[3]].view(shape).permute(0, 3, 1, 2).contiguous())) \
            if taps is not None else (lambda *a: None)
        size = lambda n, k, s, dil, pad: (n + 2 * pad - dil * (k - 1) - 1) // s + 1

        # encoder stages 1 and 2: conv1 + bn1 + relu; maxpool + layer1
        wt, bias = d["encoder.conv1"]
        h, wd = size(H, 7, 2, 1, 3), size(W, 7, 2, 1, 3)
        conv(x_cl, H, W, self.in_channels, wt, bias, 0, 64, 7, 2, 1, 3, None, 1, w["stem"], 64, 0)
        tap("f1", w["stem"], (B, h, wd, 64))
        _lib.call("r3d_dl_maxpool", w["stem"], B, h, wd, 64, w["x"], st)
        h, wd = (h - 1) // 2 + 1, (wd - 1) // 2 + 1
        X, T, Y, cin = w["x"], w["t"], w["y"], 64
        for key, blk in self._blocks():
            _, cout, _, s1, p1, d1 = conv_geometry(blk.conv1)
            _, _, _, _, p2, d2 = conv_geometry(blk.conv2)
            ho, wo = size(h, 3, s1, d1, p1), size(wd, 3, s1, d1, p1)
            wt, bias = d[key + ".conv1"]
            conv(X, h, wd, cin, wt, bias, 0, cout, 3, s1, d1, p1, None, 1, T, cout, 0)
            if blk.downsample is not None:
                _, _, _, sd, pd, dd = conv_geometry(blk.downsample[0])
                wt, bias = d[key + ".downsample"]
                conv(X, h, wd, cin, wt, bias, 0, cout, 1, sd, dd, pd, None, 0, Y, cout, 0)
                X, Y = Y, X
            wt, bias = d[key + ".conv2"]
            conv(T, ho, wo, cout, wt, bias, 0, cout, 3, 1, d2, p2, X, 1, X, cout, 0)          # relu(conv2 + identity), in place on the identity
            h, wd, cin = ho, wo, cout
            if key.endswith(".%d" % (len(getattr(self.encoder, key.split(".")[1])) - 1)):
                tap("f%d" % (int(key.split(".")[1][5:]) + 1), X, (B, h, wd, cout))

        # ASPP: four branches into their slices of one [M, 4 C] tensor; the pooled branch enters `project` as a per-sample bias
        aspp = self.decoder[0]
        conv(X, h, wd, cin, d["aspp.0"], None, 0, C, 1, 1, 1, 0, None, 1, w["cat"], 4 * C, 0)
        for i, r in enumerate(ATROUS_RATES):
            conv(X, h, wd, cin, d["aspp.%d" % (i + 1)], None, 0, C, 3, 1, r, r, None, 1, w["cat"], 4 * C, (i + 1) * C)
        _lib.call("r3d_dl_global_mean", X, B, h * wd, cin, w["pooled"], st)
        conv(w["pooled"], 1, 1, cin, d["aspp.4"], None, 0, C, 1, 1, 1, 0, None, 1, w["pf"], C, 0)
        conv(w["pf"], 1, 1, C, d["project.pooled"], None, 0, C, 1, 1, 1, 0, None, 0, w["pbias"], C, 0)
        conv(w["cat"], h, wd, 4 * C, d["project"], w["pbias"], C, C, 1, 1, 1, 0, None, 1, w["aspp"], C, 0)
        tap("aspp", w["aspp"], (B, h, wd, C))
        y = w["out"] if out is None else out
        conv(w["aspp"], h, wd, C, d["final"], None, 0, C, 3, 1, 1, 1, None, 0, y, C, 0)
        return y[:B * h * wd * C].view(B, h, wd, C)

    def _forward_cl(self, x_cl, out, taps):
        B, H, W = self._check(x_cl, "NHWC")
        x_cl = x_cl.detach()
        if x_cl.dtype != torch.float32 or not x_cl.is_contiguous():
            x_cl = x_cl.float().contiguous()
        if out is not None:
            need = B * (H // 8) * (W // 8) * self.out_channels
            if not torch.is_tensor(out) or out.dtype != torch.float32 or not out.is_contiguous() or out.numel() < need or out.device != x_cl.device:
                raise ValueError("DeepLabV3: `out` must be a contiguous float32 tensor of at least %d elements on %s" % (need, x_cl.device))
        with self._device_of(x_cl):
            return self._launches(x_cl, B, H, W, out, taps)

    @torch.no_grad()
    def forward_cl(self, x_cl, out=None):
        """[B, H, W, Cin] -> [B, H/8, W/8, 256] channel-last: a view of `out` when given, of the stream's buffer otherwise (valid until
        the next call on this stream)."""
        return self._forward_cl(x_cl, out, None)

    def _forward(self, x, taps):
        B, H, W = self._check(x, "NCHW")
        x = x.detach().float().contiguous()
        with self._device_of(x):
            w = self._buffers_for(x.device, B, H, W, self.in_channels)
            _lib.call("r3d_i2p_nchw_to_cl", x, B, self.in_channels, H, W, w["xcl"], torch.cuda.current_stream().cuda_stream)
            y = self._launches(w["xcl"].view(B, H, W, self.in_channels), B, H, W, None, taps)
        return y.permute(0, 3, 1, 2).contiguous()

    @torch.no_grad()
    def forward(self, x):
        return self._forward(x, None)

    @torch.no_grad()
    def _forward_taps(self, x):
        """Not part of the interface: (output, taps) with the five encoder features f1 .. f5 and the ASPP output `aspp`, NCHW, as new
        tensors; for tests and the timing script."""
        taps = {}
        return self._forward(x, taps), taps

    @classmethod
    def from_reference(cls, ref):
        """A HIP copy of a constructed reference DeepLabV3, or None: stride, dilation and padding are read from each of ref's Conv2d
        objects (the reference patches them after construction, encoders/_utils.py:40-47) and must be what this class builds."""
        try:
            name = {v: k for k, v in LAYERS.items()}.get(tuple(len(getattr(ref.encoder, "layer%d" % i)) for i in range(1, 5)))
            if name is None or getattr(ref.encoder, "output_stride", OUTPUT_STRIDE) != OUTPUT_STRIDE:
                return None
            m = cls(name, 5, None, ref.decoder[1].out_channels, ref.encoder.conv1.in_channels)
            want = {k: v for k, v in m.named_modules() if isinstance(v, (nn.Conv2d, nn.BatchNorm2d))}
            got = {k: v for k, v in ref.named_modules() if isinstance(v, (nn.Conv2d, nn.BatchNorm2d))}
            if set(want) != set(got):
                return None
            for k, v in want.items():
                r = got[k]
                if isinstance(v, nn.Conv2d):
                    if conv_geometry(r) is None or conv_geometry(r) != conv_geometry(v):
                        return None
                elif not isinstance(r, nn.BatchNorm2d) or r.eps != v.eps or not r.track_running_stats or not r.affine:
                    return None
            mp = getattr(ref.encoder, "maxpool", None)
            if mp is not None and (mp.kernel_size, mp.stride, mp.padding, mp.dilation, mp.ceil_mode) != (3, 2, 1, 1, False):
                return None
            m.load_state_dict(ref.state_dict(), strict=True)
        except (AttributeError, TypeError, IndexError, RuntimeError):
            return None
        return m.to(next(ref.parameters()).device).eval()
