"""fp64 restatement of SegFormerSECC2PlaneBackbone in mode b0 (modules/real3d/segformer.py:672-731), written from the semantics alone
(not from the reference's code): the CPU tests check it against the reference's goldens, the GPU tests use it as the full-size reference
(the reference tree is not available there).  Functional, on a state_dict of tensors; runs on any device in float64."""
import torch
import torch.nn.functional as F

from real3dportrait_amd.synth import SECC_DIMS, SECC_HEADS, SECC_SR


def _t(sd, k, dev, dtype=torch.float64):
    v = sd[k]
    if not torch.is_tensor(v):
        v = torch.from_numpy(v)
    return v.to(dev, dtype)


def _ln(x, sd, p, eps, dev, dtype=None):      # evaluated in x.dtype
    return F.layer_norm(x, x.shape[-1:], _t(sd, p + ".weight", dev, x.dtype), _t(sd, p + ".bias", dev, x.dtype), eps)


def _lin(x, sd, p, dev, dtype=None):
    return x @ _t(sd, p + ".weight", dev, x.dtype).T + _t(sd, p + ".bias", dev, x.dtype)


def encoder(sd, x, dtype=torch.float64):
    """x [B, in_dim, H, W] -> [c1, c2, c3, c4] NCHW (prenet + mix_vit.forward_features), evaluated in `dtype` (float64: the
    restatement; float32 on the GPU: the eager evaluation scripts/prof_secc_encoder.py times)."""
    dev = x.device
    x = x.to(dtype)
    in_dim = x.shape[1]
    w = _t(sd, "prenet.weight", dev, dtype) * (1.0 / in_dim ** 0.5)
    x = F.conv2d(x, w, _t(sd, "prenet.bias", dev, dtype))
    outs = []
    B = x.shape[0]
    for s, (C, heads, sr) in enumerate(zip(SECC_DIMS, SECC_HEADS, SECC_SR), 1):
        p = "mix_vit.patch_embed%d." % s
        k, st = (7, 4) if s == 1 else (3, 2)
        x = F.conv2d(x, _t(sd, p + "proj.weight", dev, dtype), _t(sd, p + "proj.bias", dev, dtype), stride=st, padding=k // 2)
        H, W = x.shape[2:]
        x = _ln(x.flatten(2).transpose(1, 2), sd, p + "norm", 1e-5, dev, dtype)          # [B, HW, C]
        for j in range(2):
            p = "mix_vit.block%d.%d." % (s, j)
            y = _ln(x, sd, p + "norm1", 1e-6, dev, dtype)
            q = _lin(y, sd, p + "attn.q", dev, dtype)
            if sr > 1:
                r = F.conv2d(y.transpose(1, 2).reshape(B, C, H, W), _t(sd, p + "attn.sr.weight", dev, dtype), _t(sd, p + "attn.sr.bias", dev, dtype), stride=sr)
                r = _ln(r.flatten(2).transpose(1, 2), sd, p + "attn.norm", 1e-5, dev, dtype)
            else:
                r = y
            kv = _lin(r, sd, p + "attn.kv", dev, dtype)
            d = C // heads
            qh = q.reshape(B, -1, heads, d).transpose(1, 2)
            kh = kv[..., :C].reshape(B, -1, heads, d).transpose(1, 2)
            vh = kv[..., C:].reshape(B, -1, heads, d).transpose(1, 2)
            a = torch.softmax((qh @ kh.transpose(-2, -1)) * d ** -0.5, dim=-1)
            o = (a @ vh).transpose(1, 2).reshape(B, -1, C)
            x = x + _lin(o, sd, p + "attn.proj", dev, dtype)
            y = _lin(_ln(x, sd, p + "norm2", 1e-6, dev, dtype), sd, p + "mlp.fc1", dev, dtype)
            y = F.conv2d(y.transpose(1, 2).reshape(B, 4 * C, H, W), _t(sd, p + "mlp.dwconv.dwconv.weight", dev, dtype),
                         _t(sd, p + "mlp.dwconv.dwconv.bias", dev, dtype), padding=1, groups=4 * C)
            y = F.gelu(y.flatten(2).transpose(1, 2))
            x = x + _lin(y, sd, p + "mlp.fc2", dev, dtype)
        x = _ln(x, sd, "mix_vit.norm%d" % s, 1e-6, dev, dtype)
        x = x.reshape(B, H, W, C).permute(0, 3, 1, 2).contiguous()
        outs.append(x)
    return outs


def head(sd, feats, dtype=torch.float64):
    """SegFormerHead.forward in eval: [B, 256, H/4, W/4] float64 (unfolded: the four linears, the resizes, the 1024 -> 256 fuse)."""
    dev = feats[0].device
    size = feats[0].shape[2:]
    ups = []
    for s in (4, 3, 2, 1):
        c = feats[s - 1]
        y = _lin(c.flatten(2).transpose(1, 2), sd, "fuse_head.linear_c%d.proj" % s, dev, dtype)
        y = y.transpose(1, 2).reshape(c.shape[0], 256, c.shape[2], c.shape[3])
        if s != 1:
            y = F.interpolate(y, size=size, mode="bilinear", align_corners=False)
        ups.append(y)
    z = F.conv2d(torch.cat(ups, 1), _t(sd, "fuse_head.linear_fuse.conv.weight", dev, dtype))
    p = "fuse_head.linear_fuse.bn."
    z = F.batch_norm(z, _t(sd, p + "running_mean", dev, dtype), _t(sd, p + "running_var", dev, dtype), _t(sd, p + "weight", dev, dtype), _t(sd, p + "bias", dev, dtype),
                     False, 0.0, 1e-5)
    return torch.relu(z)


def head_fold(sd, dev="cpu"):
    """The fp64 fold of the head that the HIP module applies: {1..4: W'_i [256, C_i]}, const [256], BN scale, shift."""
    wf = _t(sd, "fuse_head.linear_fuse.conv.weight", dev)[:, :, 0, 0]
    wfold, const = {}, torch.zeros(256, dtype=torch.float64, device=dev)
    for blk, s in enumerate((4, 3, 2, 1)):
        part = wf[:, 256 * blk:256 * (blk + 1)]
        wfold[s] = part @ _t(sd, "fuse_head.linear_c%d.proj.weight" % s, dev)
        const = const + part @ _t(sd, "fuse_head.linear_c%d.proj.bias" % s, dev)
    p = "fuse_head.linear_fuse.bn."
    scale = _t(sd, p + "weight", dev) / torch.sqrt(_t(sd, p + "running_var", dev) + 1e-5)
    shift = _t(sd, p + "bias", dev) - _t(sd, p + "running_mean", dev) * scale
    return wfold, const, scale, shift


def head_folded(sd, feats):
    """The head evaluated through head_fold (fp64): equals head() up to rounding."""
    dev = feats[0].device
    wfold, const, scale, shift = head_fold(sd, dev)
    size = feats[0].shape[2:]
    z = 0
    for s in (1, 2, 3, 4):
        c = feats[s - 1]
        y = torch.einsum("bchw,oc->bohw", c, wfold[s])
        if s != 1:
            y = F.interpolate(y, size=size, mode="bilinear", align_corners=False)
        z = z + y
    z = z + const[None, :, None, None]
    return torch.relu(z * scale[None, :, None, None] + shift[None, :, None, None])


def to_plane_cnn(sd, feat):
    x = feat
    for i in (0, 2, 4):
        x = F.leaky_relu(F.conv2d(x, _t(sd, "to_plane_cnn.%d.weight" % i, x.device), _t(sd, "to_plane_cnn.%d.bias" % i, x.device), padding=1), 0.01)
    x = F.interpolate(x, scale_factor=2.0, mode="bilinear", align_corners=True)
    return F.conv2d(x, _t(sd, "to_plane_cnn.7.weight", x.device), _t(sd, "to_plane_cnn.7.bias", x.device), padding=1)


def flip_planes(raw):
    """segformer.py:721-729: [B, 96, H, W] -> [B, 3, 32, H, W]; planes 0, 1 flipped along H, plane 2 along H and W."""
    p = raw.view(raw.shape[0], 3, -1, raw.shape[-2], raw.shape[-1])
    return torch.stack([torch.flip(p[:, 0], [2]), torch.flip(p[:, 1], [2]), torch.flip(p[:, 2], [2, 3])], dim=1)


def backbone(sd, x):
    """(feats, head output, flipped planes) of the whole backbone in fp64."""
    feats = encoder(sd, x)
    h = head(sd, feats)
    return feats, h, flip_planes(to_plane_cnn(sd, h))
