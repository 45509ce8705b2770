"""Img2PlaneModel without its DeepLabV3 (modules/img2plane/img2plane_model.py:66-82; segformer/models.py, base.py;
simple_encoders/high_resolution_encoder.py) restated in plain torch, parametrised by dtype: in float64 it is the reference the HIP module
and its kernels are tested against (tests/test_img2plane_host.py validates it on the reference's own outputs), in float32 on a GPU it is
the "eager torch of the same math" scripts/prof_img2plane.py times.  Pixel shuffle, the align_corners=True up-sampling and the flips are
written out as index arithmetic, not through the nn modules the kernels' tests compare against.  Imported by tests; it holds none."""
import torch
import torch.nn.functional as F


def pixel_shuffle2(x):
    """nn.PixelShuffle(2): out[b, c, 2y + i, 2x + j] = in[b, 4c + 2i + j, y, x]."""
    B, C4, h, w = x.shape
    return x.reshape(B, C4 // 4, 2, 2, h, w).permute(0, 1, 4, 2, 5, 3).reshape(B, C4 // 4, 2 * h, 2 * w)


def _up_axis(n, dtype, device):
    o = torch.arange(2 * n, device=device)
    num, den = o * (n - 1), 2 * n - 1
    i0 = torch.div(num, den, rounding_mode="floor")
    lam = (num - i0 * den).to(dtype) / den
    return i0, torch.clamp(i0 + 1, max=n - 1), lam


def upsample2x_align(x):
    """nn.UpsamplingBilinear2d(scale_factor=2): output index o reads source position o (n - 1) / (2n - 1)."""
    B, C, H, W = x.shape
    y0, y1, ly = _up_axis(H, x.dtype, x.device)
    x0, x1, lx = _up_axis(W, x.dtype, x.device)
    rows = x[:, :, y0, :] * (1 - ly)[None, None, :, None] + x[:, :, y1, :] * ly[None, None, :, None]
    return rows[:, :, :, x0] * (1 - lx) + rows[:, :, :, x1] * lx


def flip_planes(planes96):
    """img2plane_model.py:72-81: [B, 3 Cp, H, W] -> [B, 3, Cp, H, W], planes 0 and 1 flipped along H, plane 2 along H and W."""
    B, C, H, W = planes96.shape
    p = planes96.reshape(B, 3, C // 3, H, W)
    hr, wr = torch.arange(H - 1, -1, -1, device=p.device), torch.arange(W - 1, -1, -1, device=p.device)
    return torch.stack([p[:, 0][:, :, hr], p[:, 1][:, :, hr], p[:, 2][:, :, hr][:, :, :, wr]], dim=1)


def attention(q, kv, heads, scale):
    """q [B, N, C], kv [B, L, 2C] -> [B, N, C] (base.py:103-118)."""
    B, N, C = q.shape
    L = kv.shape[1]
    qh = q.reshape(B, N, heads, C // heads).permute(0, 2, 1, 3)
    kvh = kv.reshape(B, L, 2, heads, C // heads).permute(2, 0, 3, 1, 4)
    attn = ((qh @ kvh[0].transpose(-2, -1)) * scale).softmax(dim=-1)
    return (attn @ kvh[1]).transpose(1, 2).reshape(B, N, C), attn


def _ln(sd, p, x):
    return F.layer_norm(x, (x.shape[-1],), sd[p + ".weight"], sd[p + ".bias"], 1e-5)


def _lin(sd, p, x):
    return F.linear(x, sd[p + ".weight"], sd[p + ".bias"])


def _conv(sd, p, x, stride=1, pad=1):
    return F.conv2d(x, sd[p + ".weight"], sd[p + ".bias"], stride=stride, padding=pad)


def block(sd, p, x, H, sr, stats=None):
    """Block.forward (base.py:160-164) on tokens [B, H H, 1024], heads 4."""
    B, N, C = x.shape
    t = _ln(sd, p + "norm1", x)
    q = _lin(sd, p + "attn.q", t)
    if sr > 1:
        t = F.conv2d(t.permute(0, 2, 1).reshape(B, C, H, H), sd[p + "attn.sr.weight"], sd[p + "attn.sr.bias"], stride=sr).reshape(B, C, -1).permute(0, 2, 1)
        t = _ln(sd, p + "attn.norm", t)
    o, attn = attention(q, _lin(sd, p + "attn.kv", t), 4, (C // 4) ** -0.5)
    if stats is not None:
        stats.append((p, attn.shape[-1], float(attn.max(dim=-1).values.median())))
    x = x + _lin(sd, p + "attn.proj", o)
    t = _lin(sd, p + "mlp.fc1", _ln(sd, p + "norm2", x))
    t = F.conv2d(t.transpose(1, 2).reshape(B, -1, H, H), sd[p + "mlp.dwconv.dwconv.weight"], sd[p + "mlp.dwconv.dwconv.bias"], padding=1, groups=t.shape[-1])
    t = F.gelu(t.flatten(2).transpose(1, 2))
    return x + _lin(sd, p + "mlp.fc2", t)


def _embed(sd, p, x):
    x = _conv(sd, p + "proj", x, 2, 1)
    H = x.shape[-1]
    return _ln(sd, p + "norm", x.flatten(2).transpose(1, 2)), H


def _blocks(sd, p):
    n = 0
    while p + "block%d.norm1.weight" % (n + 1) in sd:
        n += 1
    return n


def high_reso_encoder(sd, x, p="high_reso_encoder."):
    h = _conv(sd, p + "first", x, 2, 3)          # no activation after `first` (high_resolution_encoder.py:33-34)
    for i in (0, 2, 4, 6):
        h = F.leaky_relu(_conv(sd, p + "conv_layers.%d" % i, h), 0.01)
    return _conv(sd, p + "final", h)


def low_reso_vit(sd, feat_low, p="low_reso_vit.", stats=None):
    h, H = _embed(sd, p + "patch_embed.", feat_low)
    for i in range(1, _blocks(sd, p) + 1):
        h = block(sd, p + "block%d." % i, h, H, 1, stats)
    h = pixel_shuffle2(h.permute(0, 2, 1).reshape(h.shape[0], h.shape[2], H, H))
    h = F.relu(_conv(sd, p + "conv_after_upsample1", upsample2x_align(h)))
    h = F.relu(_conv(sd, p + "conv_after_upsample2", upsample2x_align(h)))
    return _conv(sd, p + "final_conv", h)


def triplane_predictor_vit(sd, x_low, x_high, p="triplane_predictor_vit.", stats=None):
    h = F.leaky_relu(_conv(sd, p + "first_conv", torch.cat([x_low, x_high], dim=1)), 0.01)
    h = F.leaky_relu(_conv(sd, p + "second_conv", h), 0.01)
    h, H = _embed(sd, p + "patch_embed.", h)
    for i in range(1, _blocks(sd, p) + 1):
        h = block(sd, p + "block%d." % i, h, H, 2, stats)
    tokens = h.permute(0, 2, 1).reshape(h.shape[0], h.shape[2], H, H)
    h = torch.cat([pixel_shuffle2(tokens), x_low], dim=1)
    for name in ("first", "second", "third"):
        h = F.leaky_relu(_conv(sd, p + name + "_conv_after_cat", h), 0.01)
    return _conv(sd, p + "final_conv", h), tokens


@torch.no_grad()
def forward(sd, x_in, feat_low, dtype=torch.float64, stats=None):
    """(planes [B, 3, Cp, S/2, S/2], taps) from the assembled input x_in [B, Cin, S, S] and DeepLabV3's feat_low [B, 256, S/8, S/8];
    sd: the state_dict (tensors, any float dtype; low_reso_encoder.* is not read).  stats (a list): one (block, L, median over query rows
    of the largest softmax probability) per attention."""
    sd = {k: v.to(dtype) for k, v in sd.items() if not k.startswith("low_reso_encoder.")}
    x_in, feat_low = x_in.to(dtype), feat_low.to(dtype)
    low = low_reso_vit(sd, feat_low, stats=stats)
    high = high_reso_encoder(sd, x_in)
    out, tokens = triplane_predictor_vit(sd, low, high, stats=stats)
    return flip_planes(out), {"feat_low": feat_low, "feat_low_after_vit": low, "feat_high": high, "predictor_tokens": tokens}
