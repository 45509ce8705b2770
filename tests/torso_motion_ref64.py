"""fp64 restatement of the torso network's MotionFieldEstimator (modules/real3d/facev2v_warp/network2.py:162-244 with the helpers of
func_utils.py:91-191), written from the semantics alone (not from the reference's code): the CPU tests check it against the reference's
goldens, the GPU tests use it as the reference beyond them (the reference tree is not available there), and its float32 evaluation on
the GPU is the eager side of scripts/prof_torso_motion.py.  Functional, on state_dicts of tensors or arrays.

Grid convention: component 0 of a point indexes W, 1 H, 2 D, each in [-1, 1] with align_corners=True (node i of n sits at 2 i / (n - 1) - 1)."""
import torch
import torch.nn.functional as F

from torso_ref64 import _t, _bn


def conv3d(x, w, b, pad, dtype=torch.float64):
    """Stride-1 Conv3d with zero padding `pad` on all three axes.  float32: F.conv3d (the eager opponent of the profile script).  Otherwise
    a sum over the depth taps of 2-D convolutions on the depth slices: torch's fp64 Conv3d unfolds a whole volume at once (16 GB for the
    fuser), and the GPU has no fp64 Conv3d kernel."""
    if dtype == torch.float32:
        return F.conv3d(x, w, b, padding=pad)
    N, C, D, H, W = x.shape
    Co, kd = w.shape[0], w.shape[2]
    xs = x.permute(0, 2, 1, 3, 4)
    out = torch.zeros(N, D, Co, H, W, dtype=x.dtype, device=x.device)
    for kz in range(kd):
        lo, hi = max(0, pad - kz), min(D, D + pad - kz)          # the output depths d whose tap d + kz - pad exists
        if lo < hi:
            src = xs[:, lo + kz - pad:hi + kz - pad].reshape(-1, C, H, W)
            out[:, lo:hi] += F.conv2d(src, w[:, :, kz], None, padding=w.shape[-1] // 2).reshape(N, hi - lo, Co, H, W)
    if b is not None:
        out += b[None, None, :, None, None]
    return out.permute(0, 2, 1, 3, 4)


def identity_grid(D, H, W, dtype, dev):
    lin = lambda n: 2.0 * (torch.arange(n, dtype=dtype, device=dev) / (n - 1)) - 1.0
    z, y, x = torch.meshgrid(lin(D), lin(H), lin(W), indexing="ij")
    return torch.stack([x, y, z], dim=-1)                          # [D, H, W, 3]


def sparse_motions(kp_s, kp_d, Rs, Rd, D, H, W, dtype=torch.float64):
    """[N, K + 1, D, H, W, 3]: the identity grid, then J (grid - kp_d[k]) + kp_s[k] with J = Rs Rd^-1."""
    kp_s, kp_d = kp_s.to(dtype), kp_d.to(dtype)
    N = kp_s.shape[0]
    g = identity_grid(D, H, W, dtype, kp_s.device)
    if dtype == torch.float32:
        J = Rs.to(dtype) @ torch.linalg.inv(Rd.to(dtype))                      # as the eager module does it, on the device
    else:
        J = Rs.to(dtype) @ torch.linalg.inv(Rd.to(dtype).cpu()).to(Rd.device)  # fp64: the 3 x 3 inverses on the host (no device LAPACK needed)
    v = g[None, None] - kp_d[:, :, None, None, None, :]
    m = torch.einsum("nij,nkdhwj->nkdhwi", J, v) + kp_s[:, :, None, None, None, :]
    return torch.cat([g[None, None].expand(N, 1, D, H, W, 3), m], dim=1)


def heatmaps(kp_s, kp_d, D, H, W, dtype=torch.float64):
    """[N, K + 1, D, H, W]: 0, then exp(-|grid - kp_d[k]|^2 / 0.02) - exp(-|grid - kp_s[k]|^2 / 0.02)."""
    g = identity_grid(D, H, W, dtype, kp_s.device)
    gauss = lambda kp: torch.exp(-0.5 * (g[None, None] - kp.to(dtype)[:, :, None, None, None, :]).pow(2).sum(-1) / 0.01)
    h = gauss(kp_d) - gauss(kp_s)
    return torch.cat([torch.zeros_like(h[:, :1]), h], dim=1)


def sample_zeros(vol, grid):
    """grid_sample(vol [N, C, D, H, W], grid [N, Do, Ho, Wo, 3], align_corners=True, padding_mode='zeros') -> [N, C, Do, Ho, Wo], spelt out:
    i = (g + 1) / 2 (size - 1), trilinear over floor(i) and floor(i) + 1; a corner outside the volume contributes 0."""
    N, C, D, H, W = vol.shape
    out = torch.zeros((N, C) + tuple(grid.shape[1:4]), dtype=vol.dtype, device=vol.device)
    idx, frac = [], []
    for comp, size in ((0, W), (1, H), (2, D)):
        i = ((grid[..., comp] + 1) / 2 * (size - 1)).clamp(-2, size + 1)          # (beyond these both corners are outside anyway)
        i0 = i.floor()
        idx.append(i0.long())
        frac.append(i - i0)
    flat = vol.reshape(N, C, -1)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                x, y, z = idx[0] + dx, idx[1] + dy, idx[2] + dz
                wgt = (frac[0] if dx else 1 - frac[0]) * (frac[1] if dy else 1 - frac[1]) * (frac[2] if dz else 1 - frac[2])
                ok = (x >= 0) & (x < W) & (y >= 0) & (y < H) & (z >= 0) & (z < D)
                lin = ((z.clamp(0, D - 1) * H + y.clamp(0, H - 1)) * W + x.clamp(0, W - 1)).reshape(N, 1, -1).expand(N, C, -1)
                out += flat.gather(2, lin).reshape(out.shape) * (wgt * ok)[:, None]
    return out


def motion_input(sd, fs, kp_s, kp_d, Rs, Rd, dtype=torch.float64):
    """The hourglass input [N, 5 (K + 1), D, H, W] (channel 5 k: the heatmap, 5 k + 1 .. 5 k + 4: the compressed source sampled along sparse
    motion k) and the sparse motions."""
    dev = fs.device
    fs = fs.to(dtype)
    N, _, D, H, W = fs.shape
    K = kp_s.shape[1]
    comp = conv3d(fs, _t(sd, "compress.weight", dev, dtype), _t(sd, "compress.bias", dev, dtype), 0, dtype)
    sm = sparse_motions(kp_s, kp_d, Rs, Rd, D, H, W, dtype)
    heat = heatmaps(kp_s, kp_d, D, H, W, dtype)
    deformed = torch.stack([sample_zeros(comp, sm[:, k]) for k in range(K + 1)], dim=1)           # [N, K + 1, 4, D, H, W]
    return torch.cat([heat[:, :, None], deformed], dim=2).reshape(N, 5 * (K + 1), D, H, W), sm


def hourglass(sd, x, dtype=torch.float64):
    dev = x.device
    for i in range(5):
        p = "down.%d.layers.0.layers." % i
        x = conv3d(x, _t(sd, p + "0.weight", dev, dtype), _t(sd, p + "0.bias", dev, dtype), 1, dtype)
        x = F.avg_pool3d(F.relu(_bn(x, sd, p + "1.", dev, dtype)), (1, 2, 2))
    for i in range(5):
        p = "up.%d.layers.1.layers." % i
        x = x.repeat_interleave(2, dim=3).repeat_interleave(2, dim=4)                              # nearest x2 of H and W
        x = F.relu(_bn(conv3d(x, _t(sd, p + "0.weight", dev, dtype), _t(sd, p + "0.bias", dev, dtype), 1, dtype), sd, p + "1.", dev, dtype))
    return x


def head_encoder(sd, img, weights, dtype=torch.float64):
    """tgt_head_encoder on cat([img, weights]) at 128^2, resized to 64^2 (bilinear, align_corners=False, no antialias)."""
    dev = img.device
    x = F.interpolate(torch.cat([img.to(dtype), weights.to(dtype)], dim=1), size=(128, 128), mode="bilinear", align_corners=False)
    p = "tgt_head_encoder.0.layers."
    x = F.relu(_bn(F.conv2d(x, _t(sd, p + "0.weight", dev, dtype), _t(sd, p + "0.bias", dev, dtype), padding=3), sd, p + "1.", dev, dtype))
    for i in range(1, 4):
        y = x
        for j in range(2):
            p = "tgt_head_encoder.%d.layers.%d.layers." % (i, j)
            y = F.conv2d(F.relu(_bn(y, sd, p + "0.", dev, dtype)), _t(sd, p + "2.weight", dev, dtype), _t(sd, p + "2.bias", dev, dtype), padding=1)
        x = x + y
    return F.interpolate(x, size=(64, 64), mode="bilinear", align_corners=False)


def estimator(sd, fs, kp_s, kp_d, Rs, Rd, img, weights, dtype=torch.float64, zero_group=None, parts=None):
    """MotionFieldEstimator.forward -> (deformation [N, D, H, W, 3], occlusion [N, 1, H, W], occlusion_2 [N, 1, H, W]).
    zero_group: 0, 1 or 2 zeroes that channel group of the fuser's input (motion input, hourglass output, head features), for measuring
    each group's share of the fuser's output.  parts: a dict that receives 'mask' (softmax), 'fused' (the fuser's output) and 'input'."""
    dev = fs.device
    N, _, D, H, W = fs.shape
    inp, sm = motion_input(sd, fs, kp_s, kp_d, Rs, Rd, dtype)
    groups = [inp, hourglass(sd, inp, dtype), head_encoder(sd, img, weights, dtype)[:, :, None].expand(-1, -1, D, -1, -1)]
    if zero_group is not None:
        groups[zero_group] = torch.zeros_like(groups[zero_group])
    x = conv3d(torch.cat(groups, dim=1), _t(sd, "tgt_head_fuser.weight", dev, dtype), _t(sd, "tgt_head_fuser.bias", dev, dtype), 3, dtype)
    mask = torch.softmax(conv3d(x, _t(sd, "mask_conv.weight", dev, dtype), _t(sd, "mask_conv.bias", dev, dtype), 3, dtype), dim=1)
    deformation = (sm * mask[..., None]).sum(dim=1)
    flat = x.reshape(N, -1, H, W)                                                                  # channel c D + d
    occ = [torch.sigmoid(F.conv2d(flat, _t(sd, k + ".weight", dev, dtype), _t(sd, k + ".bias", dev, dtype), padding=3))
           for k in ("occlusion_conv", "occlusion_conv2")]
    if parts is not None:
        parts.update(mask=mask, fused=x, input=inp, sparse_motions=sm)
    return deformation, occ[0], occ[1]
