"""DeepLabV3 (modules/img2plane/deeplabv3: decoders/my_model.py, decoders/my_decoder.py, encoders/resnet.py, encoders/_base.py,
encoders/_utils.py of the reference; torchvision's ResNet / BasicBlock forward) restated functionally, for any dtype: F.conv2d, F.max_pool2d,
eval F.batch_norm from a state_dict.  Written from those sources; the tests run it in float64 as the yardstick and in float32 as the
"same math in torch".  It holds no tests.

    forward(sd, x, dtype, encoder_name="resnet34", stats=None) -> (out [B, 256, H/8, W/8], taps)
taps: f1 .. f5 (the encoder's five features after the input itself) and aspp (ASPP's output, before the last conv).  stats, when a list,
receives (name, share of elements > 0) for every ReLU.
"""
import torch
import torch.nn.functional as F

LAYERS = {"resnet18": (2, 2, 2, 2), "resnet34": (3, 4, 6, 3)}
BN_EPS = 1e-5
RATES = (12, 24, 36)


def stage_geometry(stage, block):
    """(stride, dilation) of a block's first conv and of its downsample conv: torchvision strides the first block of layer2 .. layer4 by
    2, and make_dilated(output_stride=8) then sets EVERY conv of layer3 / layer4 to stride 1, dilation 2 / 4, padding (k // 2) dilation
    (replace_strides_with_dilation, encoders/_utils.py:40-47)."""
    dilation = {3: 2, 4: 4}.get(stage, 1)
    stride = 2 if (stage == 2 and block == 0) else 1
    return stride, dilation


def forward(sd, x, dtype=torch.float64, encoder_name="resnet34", stats=None):
    p = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    x = x.to(dtype)

    def relu(name, t):
        t = F.relu(t)
        if stats is not None:
            stats.append((name, float((t > 0).double().mean())))
        return t

    bn = lambda t, k: F.batch_norm(t, p[k + ".running_mean"], p[k + ".running_var"], p[k + ".weight"], p[k + ".bias"], False, 0.0, BN_EPS)
    taps = {}
    # stage 1: conv1, bn1, relu; stage 2: maxpool, layer1
    x = relu("relu", bn(F.conv2d(x, p["encoder.conv1.weight"], None, 2, 3), "encoder.bn1"))
    taps["f1"] = x
    x = F.max_pool2d(x, 3, 2, 1)
    for stage, n in enumerate(LAYERS[encoder_name], start=1):
        for j in range(n):
            k = "encoder.layer%d.%d." % (stage, j)
            stride, d = stage_geometry(stage, j)
            out = relu(k + "relu1", bn(F.conv2d(x, p[k + "conv1.weight"], None, stride, d, d), k + "bn1"))
            out = bn(F.conv2d(out, p[k + "conv2.weight"], None, 1, d, d), k + "bn2")
            if k + "downsample.0.weight" in p:
                x = bn(F.conv2d(x, p[k + "downsample.0.weight"], None, stride, 0, d), k + "downsample.1")
            x = relu(k + "relu2", out + x)
        taps["f%d" % (stage + 1)] = x
    # ASPP (my_decoder.py:155-189): 1 x 1, three dilated 3 x 3, the pooled branch; cat; project (Dropout is the identity in eval)
    res = [relu("aspp.0", F.conv2d(x, p["decoder.0.convs.0.0.weight"]))]
    for i, r in enumerate(RATES, start=1):
        res.append(relu("aspp.%d" % i, F.conv2d(x, p["decoder.0.convs.%d.0.weight" % i], None, 1, r, r)))
    pooled = relu("aspp.4", F.conv2d(F.adaptive_avg_pool2d(x, 1), p["decoder.0.convs.4.1.weight"]))
    res.append(F.interpolate(pooled, size=x.shape[-2:], mode="bilinear", align_corners=False))
    x = relu("project", F.conv2d(torch.cat(res, dim=1), p["decoder.0.project.0.weight"]))
    taps["aspp"] = x
    return F.conv2d(x, p["decoder.1.weight"], None, 1, 1), taps
