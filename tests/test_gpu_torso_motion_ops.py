"""GPU: r3d_torso_conv3d and r3d_torso_motion_* (include/r3d_hip.h, csrc/r3d_torso_motion.hip) called directly, as
torso_motion.py calls them, and compared with a float64 torch statement of the same operation on the CPU at the shapes and values where
tiling, padding and addressing go wrong: ragged tiles, 1-pixel images, channel counts off the vector width, one and two depth slices,
pooling and up-sampling from the smallest sizes, channel slices of a wider buffer, sample points outside the volume and exactly on its faces.

One error rule for every case, that of tests/test_gpu_torso_ops.py (check): e = max|y - y64| / max|y64| must stay within
max(2^-22 sqrt(K_eff), 4 e32), where e32 is the same statement evaluated in fp32 torch on the CPU and K_eff the reduction length:
kd ksize^2 Cin for the conv, 8 C for the motion input (8 corners of C channels), K + 1 for the deformation."""
import pytest
import torch
import torch.nn.functional as F

import torso_motion_ref64 as R64
from test_gpu_torso_ops import DEV, call, check, dev, randn

pytestmark = pytest.mark.gpu


# ---- conv3d -----------------------------------------------------------------------------------------------------------------------------
def _conv3d(seed, B, D, Hs, Ws, Cin, Cout, k, up=0, pool=0, act=0, slope=0.0, full=0, bias=True, out="cl", ycs=None, yco=0, bias_scale=0.1):
    """out: 'cl' (y), 'ncdhw' or 'both'.  Returns (outputs as [B, Cout, Do, Ho, Wo], ref, K_eff, (y buffer, its fill before the call))."""
    g = torch.Generator().manual_seed(seed)
    H, W, kd, Do = Hs << up, Ws << up, (D if full else k), (1 if full else D)
    x = randn(g, B, Cin, D, Hs, Ws)
    w = randn(g, Cout, Cin, kd, k, k, scale=(Cin * kd * k * k) ** -0.5)
    b = randn(g, Cout, scale=bias_scale) if bias else None

    def ref(dt):
        a = x.to(dt)
        if up:
            a = a.repeat_interleave(2, dim=3).repeat_interleave(2, dim=4)
        bb = b.to(dt) if bias else None
        if full:          # nn.Conv2d on the viewed tensor: channel c D + d
            y = F.conv2d(a.reshape(B, Cin * D, H, W), w.to(dt).reshape(Cout, Cin * D, k, k), bb, padding=k // 2)[:, :, None]
        else:
            y = R64.conv3d(a, w.to(dt), bb, k // 2, dt)
        if act == 1:
            y = F.leaky_relu(y, slope)
        elif act == 2:
            y = torch.sigmoid(y)
        return F.avg_pool3d(y, (1, 2, 2)) if pool else y

    Ho, Wo = H >> pool, W >> pool
    ycs = Cout if ycs is None else ycs
    y = fill = None
    if out in ("cl", "both"):
        fill = randn(g, B * Do * Ho * Wo, ycs)
        y = dev(fill)
    yn = torch.empty(B, Cout, Do, Ho, Wo, device=DEV) if out in ("ncdhw", "both") else None
    call("conv3d", dev(x.permute(0, 2, 3, 4, 1)), B, D, Hs, Ws, Cin, up, dev(w.permute(0, 2, 3, 4, 1)), dev(b) if bias else None, Cout, k, full, act,
         float(slope), pool, y, ycs, yco, yn)
    outs = []
    if y is not None:
        outs.append(y.view(B, Do, Ho, Wo, ycs)[..., yco:yco + Cout].permute(0, 4, 1, 2, 3))
    if yn is not None:
        outs.append(yn)
    return outs, ref, kd * k * k * Cin, (y, fill)


def _check(what, outs, ref, keff):
    for o in outs:
        check(what, o, ref, keff)
    if len(outs) == 2:
        assert torch.equal(outs[0], outs[1]), what


CINS, COUTS = (1, 4, 25, 28, 89, 92, 512), (1, 2, 5, 32, 64, 1024)
SIZES = [(1, 1), (2, 2), (6, 6), (62, 62), (66, 66), (6, 62), (66, 2), (1, 6)]
PAIRS = []
for i, cin in enumerate(CINS):
    for j, cout in enumerate(COUTS):
        k = (1, 3, 7)[(i + j) % 3]
        D = (1, 2, 16)[(i + 2 * j) % 3]
        Hs, Ws = SIZES[(3 * i + j) % 8]
        if cin * cout * k ** 3 > 1 << 24:                 # (the weights alone would be 0.7 GB at 512 x 1024 x 7^3; that pair runs at the product's ksize)
            k = 3
        while D * Hs * Ws * cin * cout * k ** 3 > 6e10:   # (keeps the fp64 reference on the CPU short)
            if D > 2:
                D = 2
            else:
                Hs, Ws = 6, 6
        PAIRS.append((1 + (i + j) % 2, D, Hs, Ws, cin, cout, k))


@pytest.mark.parametrize("B,D,Hs,Ws,Cin,Cout,k", PAIRS)
def test_conv3d_channel_pairs(B, D, Hs, Ws, Cin, Cout, k):
    """Every Cin x Cout, with ksize, depth and image size rotating (Cin 4, 28, 92 and 512 take the 16-byte loader, the others the element loader)."""
    outs, ref, keff, _ = _conv3d(2000 + D + Hs + Ws + Cin + Cout + k, B, D, Hs, Ws, Cin, Cout, k, bias=(Cin + Cout) % 2 == 0, out="both")
    _check("conv3d B%d D%d %dx%d Cin%d Cout%d k%d" % (B, D, Hs, Ws, Cin, Cout, k), outs, ref, keff)


@pytest.mark.parametrize("k", [1, 3, 7])
@pytest.mark.parametrize("D", [1, 2, 16])
@pytest.mark.parametrize("Hs,Ws,Cin,Cout", [(1, 1, 28, 5), (2, 2, 25, 64), (6, 6, 4, 2), (62, 62, 4, 32), (66, 66, 1, 5), (6, 62, 92, 32), (66, 2, 89, 1)])
def test_conv3d_ksize_depth_size(k, D, Hs, Ws, Cin, Cout):
    B = 2 if Hs * Ws < 100 else 1
    outs, ref, keff, _ = _conv3d(2100 + k + D + Hs + Cin, B, D, Hs, Ws, Cin, Cout, k, act=1, slope=0.2, out="both")
    _check("conv3d k%d D%d %dx%d Cin%d Cout%d B%d" % (k, D, Hs, Ws, Cin, Cout, B), outs, ref, keff)


def test_conv3d_depth_one_is_the_2d_conv():
    """D = 1: the depth taps outside the single slice are padding, so ksize^3 weights act as their middle ksize^2 -- and the result is
    r3d_torso_conv's on those, bit for bit (one template, the same order of the sum over the taps that exist)."""
    g = torch.Generator().manual_seed(7)
    B, H, W, Cin, Cout = 2, 9, 13, 32, 64
    x, w = randn(g, B, H, W, Cin), randn(g, Cout, 3, 3, 3, Cin, scale=0.05)
    w[:, 0] = 0.0
    w[:, 2] = 0.0
    y3, y2 = torch.empty(B, H, W, Cout, device=DEV), torch.empty(B, H, W, Cout, device=DEV)
    call("conv3d", dev(x), B, 1, H, W, Cin, 0, dev(w), None, Cout, 3, 0, 0, 0.0, 0, y3, Cout, 0, None)
    call("conv", dev(x), B, H, W, Cin, 0, 0, None, None, 0.0, dev(w[:, 1]), None, Cout, 3, 0, 0.0, None, y2, None)
    torch.cuda.synchronize()
    assert torch.equal(y3, y2)


@pytest.mark.parametrize("pool,up", [(1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("B,D,Hs,Ws,Cin,Cout,k", [(1, 1, 2, 2, 4, 5, 3), (2, 2, 2, 2, 25, 64, 3), (1, 16, 2, 6, 28, 32, 3), (1, 2, 6, 2, 92, 2, 7),
                                                (2, 2, 62, 66, 4, 64, 3), (1, 16, 6, 6, 512, 1024, 3), (1, 1, 2, 2, 1, 1, 1)])
def test_conv3d_pool_and_upsample_from_the_smallest_even_sizes(B, D, Hs, Ws, Cin, Cout, k, pool, up):
    # (LeakyReLU 0.2, not ReLU: a single output channel behind a single weight can be negative everywhere)
    outs, ref, keff, _ = _conv3d(2200 + D + Hs + Ws + Cin + Cout + pool + 2 * up, B, D, Hs, Ws, Cin, Cout, k, up=up, pool=pool, act=1, slope=0.2,
                                 out="cl" if pool else "both")
    _check("conv3d pool%d up%d B%d D%d %dx%d Cin%d Cout%d k%d" % (pool, up, B, D, Hs, Ws, Cin, Cout, k), outs, ref, keff)


def test_conv3d_upsample_from_one_pixel_then_pool():
    outs, ref, keff, _ = _conv3d(2250, 2, 2, 1, 1, 28, 64, 3, up=1, pool=1, act=1)          # ReLU, as DownBlock3D
    _check("conv3d 1x1 up pool", outs, ref, keff)
    outs, ref, keff, _ = _conv3d(2251, 1, 16, 1, 3, 25, 5, 7, up=1, act=1, slope=0.2, out="both")
    _check("conv3d 1x3 up", outs, ref, keff)


@pytest.mark.parametrize("pool", [0, 1])
@pytest.mark.parametrize("B,D,Hs,Ws,Cin,Cout,k,ycs,yco", [(1, 16, 6, 6, 64, 32, 3, 92, 28), (2, 2, 62, 2, 4, 5, 7, 7, 2), (1, 1, 2, 2, 25, 64, 1, 65, 0),
                                                          (1, 2, 6, 6, 28, 1, 3, 3, 2)])
def test_conv3d_channel_slice_leaves_the_rest_of_the_buffer_bit_unchanged(B, D, Hs, Ws, Cin, Cout, k, ycs, yco, pool):
    outs, ref, keff, (y, fill) = _conv3d(2300 + D + Hs + Cin + Cout + pool, B, D, Hs, Ws, Cin, Cout, k, pool=pool, act=1, slope=0.2, ycs=ycs, yco=yco)
    _check("conv3d slice [%d, %d) of %d pool%d B%d D%d %dx%d Cin%d k%d" % (yco, yco + Cout, ycs, pool, B, D, Hs, Ws, Cin, k), outs, ref, keff)
    got = y.cpu()
    keep = torch.ones(ycs, dtype=torch.bool)
    keep[yco:yco + Cout] = False
    assert torch.equal(got[:, keep], fill[:, keep]) and not torch.equal(got[:, ~keep], fill[:, ~keep])


@pytest.mark.parametrize("B,D,Hs,Ws,Cin,Cout,k", [(1, 16, 64, 64, 32, 2, 7), (2, 2, 6, 62, 4, 5, 3), (1, 1, 1, 1, 25, 1, 7), (2, 16, 2, 2, 28, 64, 1)])
def test_conv3d_full_depth_is_conv2d_on_the_viewed_tensor(B, D, Hs, Ws, Cin, Cout, k):
    outs, ref, keff, _ = _conv3d(2400 + D + Hs + Cin + Cout, B, D, Hs, Ws, Cin, Cout, k, full=1, act=2, out="both")
    _check("conv3d full-depth B%d D%d %dx%d Cin%d Cout%d k%d" % (B, D, Hs, Ws, Cin, Cout, k), outs, ref, keff)


@pytest.mark.parametrize("B,D,Hs,Ws,Cin,Cout,k,full", [(1, 2, 62, 66, 28, 1, 3, 0), (2, 16, 6, 6, 89, 5, 3, 0), (1, 16, 6, 6, 32, 2, 7, 1)])
def test_conv3d_sigmoid_to_plus_minus_30(B, D, Hs, Ws, Cin, Cout, k, full):
    """Pre-activations spread over about [-35, 35] (bias ~ 12 n): the sigmoid saturates on both sides without a NaN or an Inf."""
    outs, ref, keff, _ = _conv3d(2500 + Hs + Cin + Cout, B, D, Hs, Ws, Cin, Cout, k, full=full, act=2, bias_scale=12.0, out="both")
    _check("conv3d sigmoid B%d D%d %dx%d Cin%d Cout%d k%d" % (B, D, Hs, Ws, Cin, Cout, k), outs, ref, keff)
    assert float(outs[0].min()) >= 0.0 and float(outs[0].max()) <= 1.0


def test_conv3d_sigmoid_extremes():
    """Pre-activations of exactly +-30 and +-100 (zero weights, the bias alone)."""
    x, w = torch.zeros(1, 2, 2, 2, 4, device=DEV), torch.zeros(4, 1, 1, 1, 4, device=DEV)
    b = torch.tensor([-100.0, -30.0, 30.0, 100.0], device=DEV)
    y = torch.empty(1, 2, 2, 2, 4, device=DEV)
    call("conv3d", x, 1, 2, 2, 2, 4, 0, w, b, 4, 1, 0, 2, 0.0, 0, y, 4, 0, None)
    torch.cuda.synchronize()
    ref, got = torch.sigmoid(b.double().cpu()), y[0, 1, 1, 1].double().cpu()
    assert bool(torch.isfinite(got).all()) and float((got - ref).abs().max()) <= 2e-7, (got, ref)
    assert float(got[0]) == 0.0 or float(got[0]) < 1e-40


# the estimator's own layers at B = 1 (K = 4): (D, Hs, Ws, Cin, Cout, k, up, pool)
PRODUCT = [(16, 64 >> i, 64 >> i, c[0], c[1], 3, 0, 1) for i, c in enumerate(((28, 64), (64, 128), (128, 256), (256, 512), (512, 1024)))]
PRODUCT += [(16, 2 << i, 2 << i, c[0], c[1], 3, 1, 0) for i, c in enumerate(((1024, 512), (512, 256), (256, 128), (128, 64), (64, 32)))]
PRODUCT += [(16, 64, 64, 92, 32, 7, 0, 0), (16, 64, 64, 32, 5, 7, 0, 0)]


@pytest.mark.parametrize("D,Hs,Ws,Cin,Cout,k,up,pool", PRODUCT)
def test_conv3d_product_shapes(D, Hs, Ws, Cin, Cout, k, up, pool):
    """One case per hourglass layer (down.0 .. down.4 pooled, up.0 .. up.4 up-sampled; down.4 and up.0 take the m-fast tile order), the
    fuser and mask_conv."""
    outs, ref, keff, _ = _conv3d(2600 + Hs + Cin + Cout, 1, D, Hs, Ws, Cin, Cout, k, up=up, pool=pool, act=1 if k == 3 else 0)
    _check("conv3d product D%d %dx%d Cin%d Cout%d k%d up%d pool%d" % (D, Hs, Ws, Cin, Cout, k, up, pool), outs, ref, keff)


# ---- motion input -----------------------------------------------------------------------------------------------------------------------
def _motion_points(g, kind, N, K):
    """kp_s, kp_d and J (any 3 x 3, not only rotations) that put the sample points J (grid - kp_d) + kp_s where `kind` says."""
    eye = torch.eye(3).expand(N, 3, 3).contiguous()
    kp_d = torch.rand(N, K, 3, generator=g) * 1.2 - 0.6
    if kind == "nodes":                     # the identity for every k: exactly on the volume's nodes
        return kp_d.clone(), kp_d, eye
    if kind == "faces":                     # J = 0: every point of motion k is kp_s[k], each component exactly -1 or 1
        return torch.where(torch.rand(N, K, 3, generator=g) < 0.5, -1.0, 1.0), kp_d, torch.zeros(N, 3, 3)
    if kind == "far":                       # shifted out of the volume by 3 .. 9 on every axis, either side
        shift = (torch.rand(N, K, 3, generator=g) * 6.0 + 3.0) * torch.where(torch.rand(N, K, 3, generator=g) < 0.5, -1.0, 1.0)
        return kp_d + shift, kp_d, eye
    kp_s = torch.rand(N, K, 3, generator=g) * 1.2 - 0.6          # "mixed": a general J, a third or so of the points outside
    return kp_s, kp_d, eye + randn(g, N, 3, 3, scale=0.3)


@pytest.mark.parametrize("with_fuse", [False, True])
@pytest.mark.parametrize("kind,N,K,C,D,H,W", [("mixed", 1, 4, 34, 16, 64, 64), ("mixed", 2, 9, 34, 16, 20, 12), ("nodes", 1, 4, 34, 16, 12, 9),
                                              ("faces", 2, 4, 34, 4, 5, 7), ("far", 1, 9, 34, 16, 8, 8), ("mixed", 3, 1, 5, 2, 2, 2),
                                              ("mixed", 1, 4, 1, 3, 7, 5), ("faces", 1, 9, 33, 2, 9, 2)])
def test_motion_input(kind, N, K, C, D, H, W, with_fuse):
    g = torch.Generator().manual_seed(600 + N + K + C + D + H + W)
    fs = randn(g, N, C, D, H, W)
    sd = {"compress.weight": randn(g, 4, C, 1, 1, 1, scale=C ** -0.5), "compress.bias": randn(g, 4, scale=0.3)}
    kp_s, kp_d, J = _motion_points(g, kind, N, K)
    eye = torch.eye(3).expand(N, 3, 3).contiguous()
    cm = 5 * (K + 1)
    cp, fcs = (cm + 3) // 4 * 4, (cm + 3) // 4 * 4 + 9
    cl = torch.empty(N, D, H, W, C, device=DEV)
    call("volume_to_cl", dev(fs), N, C, D, H, W, cl)
    inp_fill, fuse_fill = randn(g, N * D * H * W, cp), randn(g, N * D * H * W, fcs)
    inp, fuse = dev(inp_fill), dev(fuse_fill) if with_fuse else None
    call("motion_input", cl, N, C, D, H, W, dev(sd["compress.weight"].reshape(4, C)), dev(sd["compress.bias"]), dev(kp_s), dev(kp_d), dev(J), K,
         inp, cp, fuse, fcs)
    ref = lambda dt: R64.motion_input(sd, fs, kp_s, kp_d, J, eye, dt)[0]
    sm = R64.sparse_motions(kp_s, kp_d, J, eye, D, H, W)[:, 1:]
    outside = float((sm.abs() > 1.0).any(-1).double().mean())
    what = "motion_input %s N%d K%d C%d %dx%dx%d (%.0f %% outside)" % (kind, N, K, C, D, H, W, 100 * outside)
    check(what, inp.view(N, D, H, W, cp)[..., :cm].permute(0, 4, 1, 2, 3), ref, 8 * C)
    if kind == "far":
        assert outside == 1.0 and float(inp.view(N, D, H, W, cp)[..., :cm].view(N, D, H, W, K + 1, 5)[..., 1:, 1:].abs().max()) == 0.0
    if kind == "faces":
        assert bool((sm.abs() == 1.0).all())
    if kind == "nodes":                     # every motion is the identity: each k samples the compressed volume at its own nodes
        comp = R64.conv3d(fs.double(), sd["compress.weight"].double(), sd["compress.bias"].double(), 0)
        got = inp.view(N, D, H, W, cp)[..., :cm].view(N, D, H, W, K + 1, 5)[..., 1:].cpu().double()
        assert float((got - comp.permute(0, 2, 3, 4, 1)[..., None, :]).abs().max()) <= 4e-6 * float(comp.abs().max())
    assert float(inp.view(-1, cp)[:, cm:].abs().max()) == 0.0 if cp > cm else True
    if with_fuse:
        got = fuse.cpu()
        assert torch.equal(got[:, :cp], inp.cpu().view(-1, cp)) and torch.equal(got[:, cp:], fuse_fill[:, cp:])


# ---- deformation ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,N,K,D,H,W", [("random", 1, 4, 16, 64, 64), ("random", 2, 9, 16, 12, 20), ("saturated", 2, 4, 4, 6, 5),
                                            ("saturated", 1, 9, 2, 2, 2), ("equal", 1, 4, 3, 5, 7), ("equal", 2, 1, 2, 9, 2)])
def test_motion_deform(kind, N, K, D, H, W):
    g = torch.Generator().manual_seed(700 + N + K + D + H + W)
    kp_s, kp_d, J = _motion_points(g, "mixed", N, K)
    eye = torch.eye(3).expand(N, 3, 3).contiguous()
    if kind == "random":
        logits = randn(g, N, D, H, W, K + 1, scale=3.0)
    elif kind == "saturated":               # +-80: one component takes everything, exp(-160) underflows to 0
        logits = torch.where(torch.rand(N, D, H, W, K + 1, generator=g) < 0.3, 80.0, -80.0)
    else:                                   # equal logits, large and small: the plain mean of the motions
        logits = torch.where(torch.rand(N, D, H, W, 1, generator=g) < 0.5, 80.0, -3.0).expand(N, D, H, W, K + 1).contiguous()
    out = torch.empty(N, D, H, W, 3, device=DEV)
    call("motion_deform", dev(logits), N, D, H, W, K, dev(kp_s), dev(kp_d), dev(J), out)

    def ref(dt):
        sm = R64.sparse_motions(kp_s, kp_d, J, eye, D, H, W, dt)                           # [N, K + 1, D, H, W, 3]
        return (sm * torch.softmax(logits.to(dt), dim=-1).permute(0, 4, 1, 2, 3)[..., None]).sum(dim=1)

    check("motion_deform %s N%d K%d %dx%dx%d" % (kind, N, K, D, H, W), out, ref, K + 1)
    if kind == "equal":
        torch.testing.assert_close(out.cpu().double(), R64.sparse_motions(kp_s, kp_d, J, eye, D, H, W).mean(dim=1), rtol=0, atol=2e-6)


def test_motion_broadcast_writes_its_slice_only():
    g = torch.Generator().manual_seed(800)
    N, C, H, W, D, fcs, fco = 2, 32, 6, 10, 16, 92, 60
    feats, fill = randn(g, N, C, H, W), randn(g, N * D * H * W, fcs)
    fuse = dev(fill)
    call("motion_broadcast", dev(feats), N, C, H, W, D, fuse, fcs, fco)
    torch.cuda.synchronize()
    got = fuse.cpu().view(N, D, H, W, fcs)
    assert torch.equal(got[..., fco:fco + C], feats.permute(0, 2, 3, 1)[:, None].expand(N, D, H, W, C))
    assert torch.equal(got[..., :fco], fill.view(N, D, H, W, fcs)[..., :fco])
