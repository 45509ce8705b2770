"""Regenerate the deeplabv3_* golden vectors: the reference's DeepLabV3 (modules/img2plane/deeplabv3/decoders/my_model.py) on CPU in fp32,
its own __init__ (get_encoder, set_in_channels, make_dilated, DeepLabV3Decoder) and forward, with the synthetic weights of
real3dportrait_amd.synth.synth_deeplabv3 and the inputs of tests/deeplabv3_common.py.

Run in the build container only (needs the reference tree, R3D_REFERENCE):
    python tests/golden/make_golden_deeplabv3.py
Inputs and weights are regenerated from the seeds of deeplabv3_common.CASES, so the fixtures hold only outputs.

The reference's package imports torchvision, pretrainedmodels and timm, which are not installed.  Three small stand-ins go into
sys.modules before it is imported:
    torchvision.models.resnet                                         ResNet, BasicBlock, Bottleneck restated below from torchvision's
                                                                      published definition (parameters, attribute names, forward)
    pretrainedmodels.models.torchvision_models.pretrained_settings    a dict with the resnet names (URLs never read)
    timm                                                              an empty module
THE ONLY RESTATED PART ON THE REFERENCE SIDE IS torchvision's ResNet CLASS: equality with a torchvision-built module has not been measured.
The model is always constructed with encoder_weights=None -- "imagenet" would call model_zoo.load_url -- and the reference's Img2PlaneModel
is never constructed around the real package (its constructor asks for the ImageNet weights).

Stored per case: the output and six taps (f1 .. f5, aspp), sub-sampled by deeplabv3_common.sub; `relu`: the share of elements every ReLU
passes (names in `relu_names`), required to lie in (0.10, 0.95); `tap_max`: max|x| of every whole tap and of the output, required to lie in
(1, 100); measured by the fp64 restatement (tests/deeplabv3_ref64.py), which the maker also requires to meet the reference within 2e-4 of
max|ref|.  On every reference model it constructs, the maker also runs the package's DeepLabV3.from_reference."""
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("R3D_REFERENCE", "/root/reference")
sys.path.insert(0, REF)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, HERE)

import deeplabv3_common as common  # noqa: E402
import deeplabv3_ref64 as R64  # noqa: E402


# ---- torchvision.models.resnet, restated: the classes the reference's ResNetEncoder derives from ---------------------------------------
def conv3x3(cin, cout, stride=1, groups=1, dilation=1):
    return nn.Conv2d(cin, cout, 3, stride, dilation, dilation, groups, bias=False)


def conv1x1(cin, cout, stride=1):
    return nn.Conv2d(cin, cout, 1, stride, bias=False)


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None, groups=1, base_width=64, dilation=1, norm_layer=None):
        super().__init__()
        norm_layer = norm_layer or nn.BatchNorm2d
        self.conv1 = conv3x3(inplanes, planes, stride)
        self.bn1 = norm_layer(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = conv3x3(planes, planes)
        self.bn2 = norm_layer(planes)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        identity = x
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        if self.downsample is not None:
            identity = self.downsample(x)
        return self.relu(out + identity)


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, *a, **k):
        raise NotImplementedError("Bottleneck encoders are not constructed here")


class ResNet(nn.Module):
    def __init__(self, block, layers, num_classes=1000, zero_init_residual=False, groups=1, width_per_group=64,
                 replace_stride_with_dilation=None, norm_layer=None):
        super().__init__()
        self._norm_layer = norm_layer or nn.BatchNorm2d
        self.inplanes, self.dilation, self.groups, self.base_width = 64, 1, groups, width_per_group
        self.conv1 = nn.Conv2d(3, self.inplanes, 7, 2, 3, bias=False)
        self.bn1 = self._norm_layer(self.inplanes)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        self.layer1 = self._make_layer(block, 64, layers[0])
        self.layer2 = self._make_layer(block, 128, layers[1], stride=2)
        self.layer3 = self._make_layer(block, 256, layers[2], stride=2)
        self.layer4 = self._make_layer(block, 512, layers[3], stride=2)
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(512 * block.expansion, num_classes)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, (nn.BatchNorm2d, nn.GroupNorm)):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)

    def _make_layer(self, block, planes, blocks, stride=1, dilate=False):
        downsample = None
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(conv1x1(self.inplanes, planes * block.expansion, stride), self._norm_layer(planes * block.expansion))
        layers = [block(self.inplanes, planes, stride, downsample, self.groups, self.base_width, self.dilation, self._norm_layer)]
        self.inplanes = planes * block.expansion
        for _ in range(1, blocks):
            layers.append(block(self.inplanes, planes, groups=self.groups, base_width=self.base_width, dilation=self.dilation,
                                norm_layer=self._norm_layer))
        return nn.Sequential(*layers)


def _install_stand_ins():
    def module(name, **attrs):
        m = types.ModuleType(name)
        m.__path__ = []
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m
    names = ("resnet18", "resnet34", "resnet50", "resnet101", "resnet152")
    module("torchvision")
    module("torchvision.models")
    module("torchvision.models.resnet", ResNet=ResNet, BasicBlock=BasicBlock, Bottleneck=Bottleneck)
    module("pretrainedmodels")
    module("pretrainedmodels.models")
    module("pretrainedmodels.models.torchvision_models", pretrained_settings={n: {} for n in names})
    module("timm")


def reference_model(cin, encoder, sd):
    _install_stand_ins()
    from modules.img2plane.deeplabv3.decoders.my_model import DeepLabV3
    m = DeepLabV3(encoder_name=encoder, encoder_weights=None, in_channels=cin)          # never "imagenet": that would fetch
    m.load_state_dict(sd, strict=True)
    return m.eval()


def check_from_reference(m, cin, encoder):
    from real3dportrait_amd.deeplabv3 import DeepLabV3 as Hip, is_reference_deeplabv3
    assert is_reference_deeplabv3(m) and not is_reference_deeplabv3(m.encoder)
    hip = Hip.from_reference(m)
    assert hip is not None and hip.encoder_name == encoder and hip.in_channels == cin and not hip.training
    want, got = m.state_dict(), hip.state_dict()
    assert list(want) == list(got) and all(torch.equal(got[k], v) for k, v in want.items())
    assert not is_reference_deeplabv3(hip)


@torch.no_grad()
def run(m, x):
    got = {}
    h = m.decoder[0].register_forward_hook(lambda mod, inp, out: got.__setitem__("aspp", out))
    feats = m.encoder(x)
    out = m(x)
    h.remove()
    assert len(feats) == 6 and torch.equal(feats[0], x)
    got.update({"f%d" % i: feats[i] for i in range(1, 6)})
    return out, got


def main():
    torch.set_num_threads(16)
    keys = {}
    for name, (S, B, cin, enc, seed_w, seed_x) in common.CASES.items():
        enc, cin, sd, x = common.case_inputs(name)
        m = reference_model(cin, enc, sd)
        check_from_reference(m, cin, enc)
        out, taps = run(m, torch.from_numpy(x))
        assert tuple(out.shape) == (B, 256, S // 8, S // 8)
        keys["%s.c%d" % (enc, cin)] = np.array(list(m.state_dict()))
        keys["%s.c%d.shapes" % (enc, cin)] = np.array([list(v.shape) + [0] * (4 - v.dim()) for v in m.state_dict().values()], np.int64)
        stats = []
        o64, t64 = R64.forward(sd, torch.from_numpy(x), torch.float64, enc, stats)
        errs = {"out": common.rel(o64.numpy(), out.numpy())}
        errs.update({k: common.rel(t64[k].numpy(), taps[k].numpy()) for k in common.TAPS})
        assert all(e <= common.TOL for e in errs.values()), (name, errs)
        assert all(0.10 < share < 0.95 for _, share in stats), (name, [s for s in stats if not 0.10 < s[1] < 0.95])
        tap_max = {k: float(t64[k].abs().max()) for k in common.TAPS}
        tap_max["out"] = float(o64.abs().max())
        assert all(1.0 < v < 100.0 for v in tap_max.values()), (name, tap_max)
        res = {"spec": np.array([seed_w, seed_x, B, cin, S, S], np.int64), "encoder": np.array(enc),
               "relu_names": np.array([n for n, _ in stats]), "relu": np.array([s for _, s in stats], np.float64),
               "tap_max": np.array([tap_max[k] for k in common.TAPS + ("out",)], np.float64),
               "out": common.sub(out.numpy(), common.OUT_BUDGET)}
        for k in common.TAPS:
            res[k] = common.sub(taps[k].numpy())
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **res)
        print("%s: %d bytes, fp64 restatement vs reference %s, ReLU shares %.2f .. %.2f, max|x| %s"
              % (name, os.path.getsize(path), {k: "%.2g" % v for k, v in errs.items()}, min(s for _, s in stats), max(s for _, s in stats),
                 {k: "%.3g" % v for k, v in tap_max.items()}))
    # resnet18's keys: constructed only (no forward)
    m = reference_model(5, "resnet18", {k: torch.from_numpy(v) for k, v in common.synth.synth_deeplabv3(1, 5, "resnet18").items()})
    check_from_reference(m, 5, "resnet18")
    keys["resnet18.c5"] = np.array(list(m.state_dict()))
    keys["resnet18.c5.shapes"] = np.array([list(v.shape) + [0] * (4 - v.dim()) for v in m.state_dict().values()], np.int64)
    np.savez_compressed(os.path.join(HERE, "deeplabv3_keys.npz"), **keys)


if __name__ == "__main__":
    main()
