"""What the DeepLabV3 tests and tests/golden/make_golden_deeplabv3.py share: the golden cases with their inputs and synthetic weights, how
the taps are sub-sampled in the fixtures, and a plain-torch mock with the reference's attribute layout.  Imported by tests; it holds none."""
import functools

import numpy as np
import torch
import torch.nn as nn

from real3dportrait_amd import synth

TOL = 2e-4          # of max|ref|
# name -> (S, B, in_channels, encoder, weight seed, input seed); tests/golden/<name>.npz
CASES = {"deeplabv3_a_s64_b2": (64, 2, 5, "resnet34", 91, 92),          # 8 x 8 features: every ASPP tap but the centre falls in padding
         "deeplabv3_b_s128_c6": (128, 1, 6, "resnet34", 93, 94),       # rate 12 reaches real pixels
         "deeplabv3_c_s320": (320, 1, 5, "resnet34", 95, 96)}          # 40 x 40 features: all three rates do
TAPS = ("f1", "f2", "f3", "f4", "f5", "aspp")
TAP_BUDGET, OUT_BUDGET = 16384, 65536          # floats a stored tap / the stored output may hold (a committed file stays under 1 MiB)


def sub_slice(shape, budget):
    """How a [B, C, H, W] tensor is sub-sampled in the golden files: every second row and column above 16 x 16, then every cs-th channel
    with cs the smallest power of two that brings the count under `budget`.  A function of the shape alone."""
    B, C, H, W = shape
    ss = 2 if H * W > 256 else 1
    n = lambda cs: B * len(range(0, C, cs)) * len(range(0, H, ss)) * len(range(0, W, ss))
    cs = 1
    while n(cs) > budget:
        cs *= 2
    return np.s_[:, ::cs, ::ss, ::ss]


def sub(t, budget=TAP_BUDGET):
    t = np.asarray(t)
    return np.ascontiguousarray(t[sub_slice(t.shape, budget)])


def image(seed, B, S, cin):
    """[B, cin, S, S] float32 as Img2PlaneModel assembles it: rgb in [-1, 1] (8 x 8 blocks plus pixel noise), for cin 6 an alpha plane
    (0 on the first quarter of the rows), then row / S and col / S."""
    coarse = synth.hash_uniform(seed, B * 3 * (S // 8) ** 2, stream=5).reshape(B, 3, S // 8, S // 8) * np.float32(2.0) - np.float32(1.0)
    fine = synth.hash_uniform(seed, B * 3 * S * S, stream=6).reshape(B, 3, S, S) * np.float32(2.0) - np.float32(1.0)
    x = np.zeros((B, cin, S, S), np.float32)
    x[:, :3] = np.float32(0.7) * np.repeat(np.repeat(coarse, 8, axis=2), 8, axis=3) + np.float32(0.3) * fine
    if cin == 6:
        x[:, 3, S // 4:] = 1.0
    grid = (np.arange(S, dtype=np.float32) / np.float32(S)).astype(np.float32)
    x[:, cin - 2] = grid[:, None]
    x[:, cin - 1] = grid[None, :]
    return x


@functools.lru_cache(maxsize=4)
def weights(seed, cin, encoder="resnet34"):
    return {k: torch.from_numpy(v) for k, v in synth.synth_deeplabv3(seed, cin, encoder).items()}


def case_inputs(name):
    """(encoder name, in_channels, state_dict, input [B, cin, S, S] float32 numpy)."""
    S, B, cin, enc, seed_w, seed_x = CASES[name]
    return enc, cin, weights(seed_w, cin, enc), image(seed_x, B, S, cin)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def hip_model(sd, cin, dev, encoder="resnet34"):
    from real3dportrait_amd.deeplabv3 import DeepLabV3
    m = DeepLabV3(encoder, in_channels=cin)
    m.load_state_dict(sd, strict=True)
    return m.to(dev).eval()


def _patch_dilation(stage, rate):
    """replace_strides_with_dilation (encoders/_utils.py:40-47), as the reference applies it after construction."""
    for mod in stage.modules():
        if isinstance(mod, nn.Conv2d):
            mod.stride, mod.dilation = (1, 1), (rate, rate)
            mod.padding = ((mod.kernel_size[0] // 2) * rate,) * 2


class _Block(nn.Module):
    def __init__(self, cin, planes, stride):
        super().__init__()
        self.conv1, self.bn1 = nn.Conv2d(cin, planes, 3, stride, 1, bias=False), nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2, self.bn2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False), nn.BatchNorm2d(planes)
        self.downsample = None
        if stride != 1 or cin != planes:
            self.downsample = nn.Sequential(nn.Conv2d(cin, planes, 1, stride, bias=False), nn.BatchNorm2d(planes))


class _MockEncoder(nn.Module):
    def __init__(self, cin, layers, output_stride):
        super().__init__()
        self.conv1, self.bn1, self.relu = nn.Conv2d(cin, 64, 7, 2, 3, bias=False), nn.BatchNorm2d(64), nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        inplanes = 64
        for i, (planes, n) in enumerate(zip((64, 128, 256, 512), layers)):
            blocks = [_Block(inplanes if j == 0 else planes, planes, (1 if i == 0 else 2) if j == 0 else 1) for j in range(n)]
            setattr(self, "layer%d" % (i + 1), nn.Sequential(*blocks))
            inplanes = planes
        self._output_stride = 32
        if output_stride == 8:
            _patch_dilation(self.layer3, 2)
            _patch_dilation(self.layer4, 4)
            self._output_stride = 8
        elif output_stride == 16:
            _patch_dilation(self.layer4, 2)
            self._output_stride = 16

    @property
    def output_stride(self):
        return min(self._output_stride, 32)


class DeepLabV3(nn.Module):
    """A plain-torch mock with the reference's class name, attribute layout (torchvision's ResNet under `encoder`, the Sequential decoder)
    and state_dict keys: strided at construction, then patched to dilation the way the reference patches its encoder.  Parameters only;
    it computes through tests/deeplabv3_ref64.py in float32."""

    def __init__(self, in_channels=5, encoder_name="resnet34", output_stride=8):
        super().__init__()
        self.encoder_name = encoder_name
        self.encoder = _MockEncoder(in_channels, synth.DEEPLAB_LAYERS[encoder_name], output_stride)
        convs = [nn.Sequential(nn.Conv2d(512, 256, 1, bias=False), nn.ReLU())]
        convs += [nn.Sequential(nn.Conv2d(512, 256, 3, padding=r, dilation=r, bias=False), nn.ReLU()) for r in (12, 24, 36)]
        convs.append(nn.Sequential(nn.AdaptiveAvgPool2d(1), nn.Conv2d(512, 256, 1, bias=False), nn.ReLU()))
        aspp = nn.Module()
        aspp.convs = nn.ModuleList(convs)
        aspp.project = nn.Sequential(nn.Conv2d(1280, 256, 1, bias=False), nn.ReLU(), nn.Dropout(0.5))
        self.decoder = nn.Sequential(aspp, nn.Conv2d(256, 256, 3, padding=1, bias=False))

    @torch.no_grad()
    def forward(self, x):
        import deeplabv3_ref64 as R64
        return R64.forward(self.state_dict(), x, torch.float32, self.encoder_name)[0]
