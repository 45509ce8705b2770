"""fp64 restatement of the torso Generator (modules/real3d/facev2v_warp/network2.py:248-301) and of occlusion_2_predictor
(model2.py:212-219, called at :262), written from the semantics alone (not from the reference's code): the CPU tests check it against the
reference's goldens, the GPU tests use it as the reference at sizes beyond them (the reference tree is not available there), and its
float32 evaluation on the GPU is the eager side of scripts/prof_torso_generator.py.  Functional, on state_dicts of tensors or arrays."""
import torch
import torch.nn.functional as F


def _t(sd, k, dev, dtype):
    v = sd[k]
    if not torch.is_tensor(v):
        v = torch.from_numpy(v)
    return v.to(dev, dtype)


def warp(fs, grid, dtype=torch.float64):
    """grid_sample(fs [N, C, D, H, W], grid [N, Do, Ho, Wo, 3], align_corners=True, padding_mode='border') -> [N, C, Do, Ho, Wo], spelt
    out: i = (g + 1) / 2 (size - 1), clipped, trilinear over floor(i) and floor(i) + 1 (an index equal to `size` has weight 0)."""
    fs, grid = fs.to(dtype), grid.to(dtype)
    N, C, D, H, W = fs.shape
    out = torch.zeros((N, C) + tuple(grid.shape[1:4]), dtype=dtype, device=fs.device)
    idx, frac = [], []
    for comp, size in ((0, W), (1, H), (2, D)):
        i = ((grid[..., comp] + 1) / 2 * (size - 1)).clamp(0, size - 1)
        i0 = i.floor()
        idx.append(i0.long())
        frac.append(i - i0)
    flat = fs.reshape(N, C, -1)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                x, y, z = idx[0] + dx, idx[1] + dy, idx[2] + dz
                wgt = (frac[0] if dx else 1 - frac[0]) * (frac[1] if dy else 1 - frac[1]) * (frac[2] if dz else 1 - frac[2])
                ok = (x < W) & (y < H) & (z < D)
                lin = ((z.clamp(max=D - 1) * H + y.clamp(max=H - 1)) * W + x.clamp(max=W - 1)).reshape(N, 1, -1).expand(N, C, -1)
                out += (flat.gather(2, lin).reshape(out.shape)) * (wgt * ok)[:, None]
    return out


def _sn(sd, p, dev, dtype):
    w = _t(sd, p + "weight_orig", dev, dtype)
    sigma = torch.dot(_t(sd, p + "weight_u", dev, dtype), w.reshape(w.shape[0], -1) @ _t(sd, p + "weight_v", dev, dtype))
    return w / sigma, _t(sd, p + "bias", dev, dtype)


def _bn(x, sd, p, dev, dtype):
    return F.batch_norm(x, _t(sd, p + "running_mean", dev, dtype), _t(sd, p + "running_var", dev, dtype), _t(sd, p + "weight", dev, dtype),
                        _t(sd, p + "bias", dev, dtype), False, 0.0, 1e-5)


def decoder(sd, x, dtype=torch.float64, branches=None):
    """in_conv .. out_conv on the deformed features [N, 512, H, W] -> (rgb [N, 3, 4H, 4W], hid [N, 64, 4H, 4W]).  Spectral norm is
    evaluated per call (weight_orig / sigma), as the reference's hook does in eval mode.  branches: a list that receives
    (rms of the block's input, rms of its residual branch) per ResBlock2D."""
    dev = x.device
    x = x.to(dtype)
    w, b = _sn(sd, "in_conv.layers.0.", dev, dtype)
    x = F.leaky_relu(_bn(F.conv2d(x, w, b, padding=1), sd, "in_conv.layers.1.", dev, dtype), 0.2)
    x = F.conv2d(x, _t(sd, "mid_conv.weight", dev, dtype), _t(sd, "mid_conv.bias", dev, dtype))
    for i in range(6):
        y = x
        for j in range(2):
            p = "res.%d.layers.%d.layers." % (i, j)
            w, b = _sn(sd, p + "2.", dev, dtype)
            y = F.conv2d(F.relu(_bn(y, sd, p + "0.", dev, dtype)), w, b, padding=1)
        if branches is not None:
            branches.append((float(x.pow(2).mean().sqrt()), float(y.pow(2).mean().sqrt())))
        x = x + y
    for i in range(2):
        p = "up.%d.layers.1.layers." % i
        w, b = _sn(sd, p + "0.", dev, dtype)
        x = F.interpolate(x, scale_factor=2, mode="nearest")
        x = F.relu(_bn(F.conv2d(x, w, b, padding=1), sd, p + "1.", dev, dtype))
    rgb = F.conv2d(x, _t(sd, "out_conv.weight", dev, dtype), _t(sd, "out_conv.bias", dev, dtype), padding=3)
    return rgb, x


def generator(sd, fs, grid, dtype=torch.float64, branches=None):
    """Generator.forward(fs, deformation, occlusion, return_hid=True) -> (deformed_fs [N, 512, H, W], rgb, hid)."""
    N, _, _, H, W = fs.shape
    d = warp(fs, grid, dtype).reshape(N, -1, H, W)
    rgb, hid = decoder(sd, d, dtype, branches)
    return d, rgb, hid


def predictor(psd, x, dtype=torch.float64):
    """occlusion_2_predictor on the concatenated [N, 65, H, W]."""
    dev = x.device
    x = x.to(dtype)
    for i in (0, 2, 4):
        x = F.conv2d(x, _t(psd, "%d.weight" % i, dev, dtype), _t(psd, "%d.bias" % i, dev, dtype), padding=1)
        x = torch.sigmoid(x) if i == 4 else F.relu(x)
    return x


def occlusion_2(psd, hid, occ2_low, dtype=torch.float64):
    """The forward tail (model2.py:262): predictor(cat([hid, bilinear(occlusion_2 -> hid's size)])), align_corners=False."""
    up = F.interpolate(occ2_low.to(dtype), size=tuple(hid.shape[-2:]), mode="bilinear", align_corners=False)
    return predictor(psd, torch.cat([hid.to(dtype), up], dim=1), dtype)
