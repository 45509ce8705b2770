"""GPU: each kernel of include/r3d_hip_img2plane.h at its edges.  r3d_i2p_attention against an fp64 evaluation, with the
same op in fp32 torch on the CPU as the yardstick: the kernel may be at most four times as far from fp64 as that evaluation is (it sums in
k-chunks of 4 and rescales in the streaming softmax, so it need not match torch's order; more than that is a bug, not rounding), and never
more than 2e-4 of max|ref|.  The copies against their torch operators bit for bit, the up-sampling within two fp32 ulps of max|x|."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import img2plane_ref64 as R64
from real3dportrait_amd import _lib, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2e-4


def unit(seed, shape, stream=0):
    return torch.from_numpy(synth.hash_unitvar(seed, shape, stream))


def attention_inputs(B, N, L, C, seed, gain=1.5):
    """q and kv as the blocks produce them: unit-variance entries, the logits' spread about gain^2."""
    q = unit(seed, (B, N, C), 1) * gain
    kv = unit(seed, (B, L, 2 * C), 2)
    kv[..., :C] *= gain
    return q.contiguous(), kv.contiguous()


def hip_attention(q, kv, heads, scale):
    B, N, C = q.shape
    out = torch.full((B, N, C), float("nan"), device=DEV)
    _lib.call("r3d_i2p_attention", q.to(DEV), kv.to(DEV), B, N, kv.shape[1], C, heads, scale, out)
    return out


def check_attention(q, kv, heads, tag):
    scale = (q.shape[-1] // heads) ** -0.5
    ref = R64.attention(q.double(), kv.double(), heads, scale)[0]
    cpu32 = R64.attention(q, kv, heads, scale)[0]
    out = hip_attention(q, kv, heads, scale).cpu()
    assert bool(torch.isfinite(out).all())
    top = float(ref.abs().max())
    e_hip, e_cpu = float((out.double() - ref).abs().max()) / top, float((cpu32.double() - ref).abs().max()) / top
    print("attention %s: hip %.3g, fp32 torch on the CPU %.3g of max|ref|" % (tag, e_hip, e_cpu))
    assert e_hip <= TOL and e_hip <= 4.0 * e_cpu, (tag, e_hip, e_cpu)
    return out


@pytest.mark.parametrize("B,N,L,C,heads", [(1, 1, 1, 1024, 4), (2, 70, 64, 1024, 4), (1, 37, 1100, 1024, 4), (1, 64, 130, 512, 2),
                                             (1, 33, 40, 192, 4), (2, 20, 33, 32, 2), (1, 17, 70, 288, 2)])
def test_attention_against_fp64(B, N, L, C, heads):
    """Single query and key; a ragged last query tile with exactly one 64-key pair of chunks; L past r3d_secc_attention's 1024 and no chunk
    multiple; a second channel count; head dimensions 48 (padded to 64), 16 (the smallest) and 144 (padded to 256)."""
    q, kv = attention_inputs(B, N, L, C, 100 + N)
    check_attention(q, kv, heads, "%dx%dx%dx%d/%d" % (B, N, L, C, heads))


def test_attention_max_subtraction_holds():
    """One logit row shifted by +80: the first channel of every head is 1 in every key and 0 in every query, except 80 / scale in query
    row 5, which adds exactly 80 to each of that row's logits.  exp() of an unshifted logit near 90 overflows fp32; the softmax does not
    change under the shift, so the row stays what it was, and the other rows are untouched bit for bit.  Then one key shifted by +80 for
    every query, in the last-but-one chunk: it takes all the weight, and the running maximum jumps in mid-stream."""
    B, N, L, C, heads = 1, 37, 130, 1024, 4
    q, kv = attention_inputs(B, N, L, C, 7)
    D = C // heads
    for h in range(heads):
        q[:, :, h * D] = 0.0
        kv[:, :, h * D] = 1.0
    base = check_attention(q, kv, heads, "unshifted")
    for h in range(heads):
        q[:, 5, h * D] = 80.0 * 16.0                # scale = 1/16: +80 on every logit of row 5
    out = check_attention(q, kv, heads, "row +80")
    rows = [r for r in range(N) if r != 5]
    assert torch.equal(out[:, rows], base[:, rows])
    assert float((out[:, 5] - base[:, 5]).abs().max()) <= TOL * float(base.abs().max())
    for h in range(heads):
        q[:, :, h * D] = 16.0                       # now this channel adds k[key, h D] to every logit of head h
        kv[:, :, h * D] = 0.0
        kv[:, 97, h * D] = 80.0
    out = check_attention(q, kv, heads, "key +80")
    assert float((out[0] - kv[0, 97, C:]).abs().max()) < 1e-6


def test_attention_is_bit_identical_across_runs_batch_and_tile_position():
    B, N, L, C, heads = 2, 70, 130, 1024, 4
    q, kv = attention_inputs(B, N, L, C, 9)
    scale = (C // heads) ** -0.5
    both = hip_attention(q, kv, heads, scale)
    assert torch.equal(both, hip_attention(q, kv, heads, scale))
    for b in range(B):
        assert torch.equal(both[b:b + 1], hip_attention(q[b:b + 1].contiguous(), kv[b:b + 1].contiguous(), heads, scale)), b
    # queries 13 .. 69 as a problem of their own: they land in other rows of other blocks
    assert torch.equal(both[:, 13:], hip_attention(q[:, 13:].contiguous(), kv, heads, scale))


@pytest.mark.parametrize("B,H,W,C", [(2, 5, 7, 3), (1, 1, 1, 5), (1, 8, 8, 256), (1, 1, 9, 2), (1, 40000, 1, 1), (1, 2, 33000, 1)])
def test_upsample2x_against_the_fp64_rule(B, H, W, C):
    """Odd sizes, a single pixel, the model's width, and sides past 32 768, where o (n - 1) no longer fits 32 bits."""
    x = unit(21, (B, C, H, W))
    ref = R64.upsample2x_align(x.double())
    # torch's own fp64 evaluation rounds the scale first: its position o * scale is off by up to 2n ulps of 1
    assert float((ref - nn.UpsamplingBilinear2d(scale_factor=2.0)(x.double())).abs().max()) < 1e-13 * max(1, max(H, W) // 8)
    y = torch.full((B, 2 * H, 2 * W, C), float("nan"), device=DEV)
    _lib.call("r3d_i2p_upsample2x", x.permute(0, 2, 3, 1).contiguous().to(DEV), B, H, W, C, y)
    got = y.cpu().permute(0, 3, 1, 2).double()
    cpu32 = nn.UpsamplingBilinear2d(scale_factor=2.0)(x).double()
    ulp = float(x.abs().max()) * 2.0 ** -23
    e_hip, e_cpu = float((got - ref).abs().max()) / ulp, float((cpu32 - ref).abs().max()) / ulp
    print("upsample2x %dx%dx%dx%d: hip %.2f, fp32 torch on the CPU %.2f ulp of max|x|" % (B, H, W, C, e_hip, e_cpu))
    assert e_hip <= 2.0, (e_hip, e_cpu)
    # the corners are copies
    assert torch.equal(got[:, :, 0, 0], x[:, :, 0, 0].double()) and torch.equal(got[:, :, -1, -1], x[:, :, -1, -1].double())


@pytest.mark.parametrize("B,h,w,Co,cstride,coffset", [(2, 5, 7, 3, 3, 0), (1, 5, 7, 5, 11, 4), (1, 4, 4, 256, 352, 0)])
def test_pixel_shuffle_into_a_channel_slice(B, h, w, Co, cstride, coffset):
    x = unit(22, (B, 4 * Co, h, w))
    y = torch.full((B, 2 * h, 2 * w, cstride), -7.0, device=DEV)
    tokens = x.permute(0, 2, 3, 1).reshape(B, h * w, 4 * Co).contiguous()
    _lib.call("r3d_i2p_pixel_shuffle", tokens.to(DEV), B, h, w, Co, y, cstride, coffset)
    got = y.cpu()
    assert torch.equal(got[..., coffset:coffset + Co].permute(0, 3, 1, 2), nn.PixelShuffle(2)(x))
    rest = torch.cat([got[..., :coffset], got[..., coffset + Co:]], dim=-1)
    assert bool((rest == -7.0).all())


@pytest.mark.parametrize("M,C,cstride,coffset", [(35, 3, 3, 0), (35, 5, 11, 6), (70, 96, 352, 256)])
def test_copy_channels_is_one_side_of_cat(M, C, cstride, coffset):
    x = unit(23, (M, C))
    y = torch.full((M, cstride), -7.0, device=DEV)
    _lib.call("r3d_i2p_copy_channels", x.to(DEV), M, C, y, cstride, coffset)
    want = torch.cat([torch.full((M, coffset), -7.0), x, torch.full((M, cstride - coffset - C), -7.0)], dim=1)
    assert torch.equal(y.cpu(), want)


@pytest.mark.parametrize("B,C,H,W", [(2, 5, 5, 7), (1, 9, 16, 16), (1, 1, 1, 1)])
def test_nchw_to_channel_last(B, C, H, W):
    x = unit(24, (B, C, H, W))
    y = torch.full((B, H, W, C), float("nan"), device=DEV)
    _lib.call("r3d_i2p_nchw_to_cl", x.to(DEV), B, C, H, W, y)
    assert torch.equal(y.cpu(), x.permute(0, 2, 3, 1).contiguous())


@pytest.mark.parametrize("B,H,W,Cp", [(2, 5, 7, 2), (1, 8, 8, 32), (1, 1, 1, 1)])
def test_planes_out_flips_as_the_reference(B, H, W, Cp):
    x = unit(25, (B, 3 * Cp, H, W))
    planes = torch.full((B, 3, Cp, H, W), float("nan"), device=DEV)
    _lib.call("r3d_i2p_planes_out", x.permute(0, 2, 3, 1).contiguous().to(DEV), B, H, W, Cp, planes)
    v = x.view(B, 3, Cp, H, W)
    want = torch.stack([torch.flip(v[:, 0], [2]), torch.flip(v[:, 1], [2]), torch.flip(v[:, 2], [2, 3])], dim=1)      # img2plane_model.py:72-81
    assert torch.equal(planes.cpu(), want)
