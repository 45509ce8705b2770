"""The appearance feature extractor of the face-vid2vid torso network (modules/real3d/facev2v_warp/network2.py:16-45) restated from a
state dict in plain torch ops, fp64 by default: no fold, BatchNorm as F.batch_norm on the running statistics, the padding of every
convolution applied to the activated tensor as the reference's modules do.  dtype=torch.float32 is the eager opponent of the profile
script."""
import torch
import torch.nn.functional as F

from torso_ref64 import _t, _bn
from torso_motion_ref64 import conv3d


def extractor(sd, x, dtype=torch.float64, parts=None, pad_before_bn=None, drop_block=None, drop_residual=None):
    """x [N, in_dim, H, W] -> [N, 32, 16, H / 4, W / 4].  parts: a dict that receives 'relu' (the share of its inputs each ReLU zeroes, in
    the order of evaluation) and 'branches' ((rms of the block's input, rms of its branch) per ResBlock3D).  The three switches are for
    the golden script's conditions only: pad_before_bn = (block, conv): that "NAC" conv zero-pads its input BEFORE BatchNorm + ReLU (the
    wrong order); drop_block = i: ResBlock3D i is the identity; drop_residual = i: block i returns its branch alone."""
    dev = x.device
    x = x.to(dtype)
    zeroed = []

    def relu(v):
        if parts is not None:                      # (a host synchronisation: not in the timed eager forward)
            zeroed.append(float((v <= 0).double().mean()))
        return F.relu(v)

    x = relu(_bn(F.conv2d(x, _t(sd, "in_conv.layers.0.weight", dev, dtype), _t(sd, "in_conv.layers.0.bias", dev, dtype), padding=3),
                 sd, "in_conv.layers.1.", dev, dtype))
    for i in range(2):
        p = "down.%d.layers.0.layers." % i
        x = relu(_bn(F.conv2d(x, _t(sd, p + "0.weight", dev, dtype), _t(sd, p + "0.bias", dev, dtype), padding=1), sd, p + "1.", dev, dtype))
        x = F.avg_pool2d(x, (2, 2))
    x = F.conv2d(x, _t(sd, "mid_conv.weight", dev, dtype), _t(sd, "mid_conv.bias", dev, dtype))
    N, _, H, W = x.shape
    x = x.view(N, 32, 16, H, W)
    branches = []
    for i in range(6):
        if drop_block == i:
            continue
        h = x
        for j in range(2):
            p = "res.%d.layers.%d.layers." % (i, j)
            w, b = _t(sd, p + "2.weight", dev, dtype), _t(sd, p + "2.bias", dev, dtype)
            if pad_before_bn == (i, j):
                # the padding voxels then hold relu(bn(0)) = a constant per channel: by linearity, the zero-padded conv of (a - const)
                # plus the conv of the constant volume
                const = F.relu(_bn(torch.zeros(1, 32, 1, 1, 1, dtype=dtype, device=dev), sd, p + "0.", dev, dtype))
                h = conv3d(relu(_bn(h, sd, p + "0.", dev, dtype)) - const, w, b, 1, dtype) + (w.sum((2, 3, 4)) @ const.view(32)).view(1, 32, 1, 1, 1)
            else:
                h = conv3d(relu(_bn(h, sd, p + "0.", dev, dtype)), w, b, 1, dtype)
        if parts is not None:
            branches.append((float(x.pow(2).mean().sqrt()), float(h.pow(2).mean().sqrt())))
        x = h if drop_residual == i else x + h
    if parts is not None:
        parts["relu"], parts["branches"] = zeroed, branches
    return x
