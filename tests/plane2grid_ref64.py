"""Plane2GridModule (modules/real3d/img2plane_baseline.py:32-77) restated in plain torch on the CPU, in the dtype asked for (float64 for the
tests): GroupNorm as its definition (mean and biased variance per (sample, group)), ReLU, F.conv3d over F.pad(mode='replicate'), and
x + alpha out.  It shares no code with real3dportrait_amd/plane2grid.py: no scale / shift form, no alpha fold, no permuted weights."""
import torch
import torch.nn.functional as F

GROUPS = 4


def group_norm(x, gamma, beta, eps=1e-5, groups=GROUPS):
    B, C = x.shape[:2]
    g = x.reshape(B, groups, -1)
    mean = g.mean(dim=2, keepdim=True)
    var = ((g - mean) ** 2).mean(dim=2, keepdim=True)
    y = ((g - mean) / torch.sqrt(var + eps)).reshape(x.shape)
    shape = (1, C) + (1,) * (x.dim() - 2)
    return y * gamma.view(shape) + beta.view(shape)


def conv3d_replicate(x, w, b):
    return F.conv3d(F.pad(x, (1, 1, 1, 1, 1, 1), mode="replicate"), w, b)


def forward(sd, x, depth, dtype=torch.float64):
    """x [N, 3 C D, H, W] -> (y [N, 3 C D, H, W], taps {"conv1.<i>": [3N, C, D, H, W], "branch": y - x formed in `dtype`})."""
    p = {k: v.to(dtype) for k, v in sd.items()}
    N, KCD, H, W = x.shape
    C = KCD // 3 // depth
    v = x.to(dtype).reshape(N * 3, C, depth, H, W)
    x0, taps, i = v, {}, 0
    while "res_blocks_3d.%d.alpha" % i in p:
        k = "res_blocks_3d.%d." % i
        h = conv3d_replicate(F.relu(group_norm(v, p[k + "norm1.weight"], p[k + "norm1.bias"])), p[k + "conv1.weight"], p[k + "conv1.bias"])
        taps["conv1.%d" % i] = h
        out = conv3d_replicate(F.relu(group_norm(h, p[k + "norm2.weight"], p[k + "norm2.bias"])), p[k + "conv2.weight"], p[k + "conv2.bias"])
        v = v + p[k + "alpha"] * out
        i += 1
    taps["branch"] = (v - x0).reshape(N, KCD, H, W)
    return v.reshape(N, KCD, H, W), taps
