"""What joins the three modules in WarpBasedTorsoModelMediaPipe.forward (modules/real3d/facev2v_warp/model2.py:226-236), restated in
fp64 without F.interpolate, F.pad or max_pool2d: the bilinear resize of two segmap channels by explicit neighbour indices
and weights, the mask sum, the dilation as a maximum over shifted views with `reflect` indices, the multiply and the concatenation.
torch_glue is the reference's own statement (its torch calls, any dtype): in float32 it gives the reference's error e32 of the parity
rule  e <= max(4 e32, 2^-22) of max|ref|."""
import numpy as np
import torch
import torch.nn.functional as F

FLOOR = 2.0 ** -22


def _axis(out_size, in_size):
    """F.interpolate(mode='bilinear', align_corners=False, antialias=False) along one axis: src = max((dst + 0.5) in / out - 0.5, 0),
    the upper neighbour clamped at the edge.  (i0, i1, l0, l1), fp64."""
    src = np.maximum((np.arange(out_size, dtype=np.float64) + 0.5) * (float(in_size) / float(out_size)) - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), in_size - 1)
    i1 = np.minimum(i0 + 1, in_size - 1)
    l1 = src - i0
    return i0, i1, 1.0 - l1, l1


def resize(x, size):
    """x [..., Hs, Ws] -> [..., h, w], fp64."""
    x = torch.as_tensor(x).double()
    (y0, y1, ly0, ly1), (x0, x1, lx0, lx1) = _axis(size[0], x.shape[-2]), _axis(size[1], x.shape[-1])
    T = torch.from_numpy
    rows = x[..., T(y0), :] * T(ly0)[:, None] + x[..., T(y1), :] * T(ly1)[:, None]
    return rows[..., T(x0)] * T(lx0) + rows[..., T(x1)] * T(lx1)


def _reflect(i, n):
    i = np.abs(i)
    return np.where(i >= n, 2 * (n - 1) - i, i)


def dilate(mask, ksize):
    """utils/commons/image_utils.py:10-15 on mask [N, h, w]: the maximum over the ksize x ksize window, indices outside reflected."""
    pad = (ksize - 1) // 2
    h, w = mask.shape[-2:]
    assert ksize % 2 == 1 and pad < min(h, w)
    out = None
    for dy in range(-pad, pad + 1):
        iy = torch.from_numpy(_reflect(np.arange(h) + dy, h))
        for dx in range(-pad, pad + 1):
            ix = torch.from_numpy(_reflect(np.arange(w) + dx, w))
            v = mask[..., iy, :][..., ix]
            out = v if out is None else torch.maximum(out, v)
    return out


def glue(feats, segmap, c0=2, c1=4, ksize=7, mul_mask=True):
    """model2.py:231-236 in fp64 on feats [N, C, D, h, w]: {seg [N, 2, h, w], mask_d [N, h, w], masked [N, C, D, h, w], motion
    [N, C + 2, D, h, w]}."""
    feats = torch.as_tensor(feats).double()
    N, C, D, h, w = feats.shape
    seg = resize(torch.as_tensor(segmap)[:, [c0, c1]], (h, w))
    mask_d = dilate(seg[:, 0] + seg[:, 1], ksize)
    masked = feats * mask_d[:, None, None] if mul_mask else feats
    motion = torch.cat([masked, seg[:, :, None].expand(N, 2, D, h, w)], dim=1)
    return {"seg": seg, "mask_d": mask_d, "masked": masked, "motion": motion}


def seg_input(img, segmap, c0=2, c1=4, size=None):
    """model2.py:226-228 in fp64: cat(img, resize(segmap[:, [c0, c1]])) (img None: the pair alone at `size`)."""
    seg = resize(torch.as_tensor(segmap)[:, [c0, c1]], size if img is None else tuple(img.shape[-2:]))
    return seg if img is None else torch.cat([torch.as_tensor(img).double(), seg], dim=1)


def torch_glue(feats, segmap, c0=2, c1=4, ksize=7, mul_mask=True, dtype=torch.float32):
    """The reference's statement of the same lines, with its torch calls, in `dtype`."""
    feats, segmap = torch.as_tensor(feats).to(dtype), torch.as_tensor(segmap)
    seg = F.interpolate(segmap[:, [c0, c1]].to(dtype), size=tuple(feats.shape[-2:]), mode="bilinear", align_corners=False, antialias=False)
    pad = (ksize - 1) // 2
    mask_d = F.max_pool2d(F.pad(seg.sum(dim=1).unsqueeze(1), pad=[pad, pad, pad, pad], mode="reflect"), kernel_size=ksize, stride=1, padding=0)
    masked = feats * mask_d.unsqueeze(1) if mul_mask else feats
    motion = torch.cat([masked, seg.unsqueeze(2).repeat([1, 1, feats.shape[2], 1, 1])], dim=1)
    return {"seg": seg, "mask_d": mask_d[:, 0], "masked": masked, "motion": motion}


def torch_seg_input(img, segmap, c0=2, c1=4, size=None, dtype=torch.float32):
    seg = F.interpolate(torch.as_tensor(segmap)[:, [c0, c1]].to(dtype), size=size if img is None else tuple(img.shape[-2:]), mode="bilinear",
                        align_corners=False, antialias=False)
    return seg if img is None else torch.cat([torch.as_tensor(img).to(dtype), seg], dim=1)


def rel(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return float(np.abs(a - ref).max() / np.abs(ref).max())


def bound(e32):
    """The parity rule: 4 x the fp32 reference's own error against fp64, with a floor of 2^-22, of max|ref|."""
    return max(4.0 * e32, FLOOR)


def to_cl(v):
    """[N, C, D, h, w] -> [N, D, h, w, C], what r3d_torso_volume_to_cl gives."""
    return v.permute(0, 2, 3, 4, 1).contiguous()
