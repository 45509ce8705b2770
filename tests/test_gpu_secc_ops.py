"""GPU: every r3d_secc_* entry point (include/r3d_hip.h, csrc/r3d_segformer.hip) called directly, as segformer.py calls it,
and compared with a float64 torch statement of the same operation at the shapes and values where tiling, masking and reductions go wrong:
ragged tiles and key chunks, non-square grids, batches whose 64-row tiles straddle samples, constant rows, large means, peaked softmaxes.

One error rule for every case (check): e = max|y - y64| / max|y64| must stay within max(2^-22 sqrt(K_eff), 4 e32), where e32 is the
same statement evaluated in fp32 torch on the CPU (no TF32, no device library choices) and K_eff the reduction length: K for linear,
conv and embed1, C for layernorm, max(L, 32) for attention, 9 for dwconv, 32 for head.  Inputs come from seeded CPU generators."""
import math

import pytest
import torch
import torch.nn.functional as F

from real3dportrait_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR = 2.0 ** -22


def call(name, *args):
    """Tensor arguments go in as device pointers; holding them here keeps temporaries alive until the launch is queued."""
    args = [_lib.ptr(a) if torch.is_tensor(a) else a for a in args]
    _lib.check(getattr(_lib.load(), "r3d_secc_" + name)(*args, _lib.stream_ptr()), "secc_" + name)


def randn(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


def uniform(g, lo, hi, *shape):
    return torch.rand(*shape, generator=g) * (hi - lo) + lo


def dev(t):
    return t.float().contiguous().to(DEV)


def check(what, y, ref, keff):
    """y: the kernel's output on the device; ref(dtype): the operation on the CPU in that dtype (float64: the reference)."""
    torch.cuda.synchronize()
    y = y.cpu().double()
    y64, y32 = ref(torch.float64), ref(torch.float32).double()
    assert y.shape == y64.shape and bool(torch.isfinite(y).all()), what
    m = float(y64.abs().max())
    assert m > 0.0, what
    e, e32 = float((y - y64).abs().max()) / m, float((y32 - y64).abs().max()) / m
    floor = FLOOR * math.sqrt(keff)
    bound = max(floor, 4.0 * e32)
    print("%s: e %.2e e32 %.2e bound %.2e%s" % (what, e, e32, bound, "  [within the floor only]" if e > 4.0 * e32 else ""))
    assert e <= bound, (what, e, e32, bound)
    return y64


# ---- linear: y = act(LN?(x) w^T + bias) (+ residual) ------------------------------------------------------------------------------------
def _rows(g, kind, M, K, eps):
    """normal rows; rows whose variance is comparable to eps; constant rows; rows of mean 1e3 and std 1."""
    if kind == "normal":
        return randn(g, M, K) * uniform(g, 0.5, 2.0, M, 1) + randn(g, M, 1)
    if kind == "tiny_var":
        return randn(g, M, K) * (math.sqrt(eps) * uniform(g, 0.3, 3.0, M, 1)) + uniform(g, -1.0, 1.0, M, 1)
    if kind == "constant":
        return randn(g, M, 1, scale=3.0).expand(M, K).contiguous()
    return randn(g, M, K) + 1e3 * uniform(g, 1.0, 2.0, M, 1)


def _linear(seed, M, K, N, bias=True, ln=None, rows="normal", gelu=False, res=None):
    g = torch.Generator().manual_seed(seed)
    x = _rows(g, rows, M, K, ln or 1e-6) if ln else randn(g, M, K)
    w = randn(g, N, K, scale=K ** -0.5)
    b = (uniform(g, -4.0, 4.0, N) if gelu else randn(g, N, scale=0.1)) if bias else None
    lg, lb = (uniform(g, 0.5, 1.5, K), randn(g, K, scale=0.1)) if ln else (None, None)
    r = randn(g, M, N) if res else None

    def ref(dt):
        v = x.to(dt)
        if ln:
            v = F.layer_norm(v, (K,), lg.to(dt), lb.to(dt), ln)
        v = v @ w.to(dt).T
        if b is not None:
            v = v + b.to(dt)
        if gelu:
            v = F.gelu(v)
        return v + r.to(dt) if r is not None else v

    y = dev(r) if res == "in_place" else torch.empty(M, N, device=DEV)
    rd = y if res == "in_place" else (dev(r) if res else None)
    xd, wd, bd = dev(x), dev(w), dev(b) if b is not None else None
    lgd, lbd = (dev(lg), dev(lb)) if ln else (None, None)
    call("linear", xd, M, K, lgd, lbd, float(ln or 0.0), wd, bd, N, int(gelu), rd, y)
    return y, ref


LIN_M, LIN_K, LIN_N = (1, 63, 64, 65, 1000), (1, 3, 17, 32, 160, 1024, 4096), (1, 15, 64, 65, 256)
LIN_SHAPES = [(M, K, LIN_N[(i + j) % 5], (i + j) % 2 == 0) for i, M in enumerate(LIN_M) for j, K in enumerate(LIN_K)]


@pytest.mark.parametrize("M,K,N,bias", LIN_SHAPES)
def test_linear_shapes(M, K, N, bias):
    y, ref = _linear(100 + M + K + N, M, K, N, bias)
    check("linear M%d K%d N%d bias%d" % (M, K, N, bias), y, ref, K)


@pytest.mark.parametrize("rows", ["normal", "tiny_var", "constant", "large_mean"])
@pytest.mark.parametrize("M,K,N,eps", [(65, 32, 64, 1e-6), (63, 160, 65, 1e-5), (1000, 256, 15, 1e-6), (64, 1024, 256, 1e-5),
                                       (5, 1, 15, 1e-6), (130, 17, 1, 1e-5)])
def test_linear_layernorm_prologue(rows, M, K, N, eps):
    y, ref = _linear(200 + M + K, M, K, N, True, ln=eps, rows=rows)
    check("linear LN %s M%d K%d N%d eps%g" % (rows, M, K, N, eps), y, ref, K)


@pytest.mark.parametrize("M,K,N", [(1000, 32, 64), (65, 160, 256), (63, 3, 15), (1, 1024, 65)])
def test_linear_gelu(M, K, N):
    y, ref = _linear(300 + M + K, M, K, N, True, gelu=True)
    check("linear gelu M%d K%d N%d" % (M, K, N), y, ref, K)


def test_linear_gelu_spans_the_curve():
    """The pre-activations of the gelu cases cover [-5, 5] (bias uniform in [-4, 4] plus a unit-variance product)."""
    g = torch.Generator().manual_seed(301)
    x, w, b = randn(g, 1000, 32), randn(g, 64, 32, scale=32 ** -0.5), uniform(g, -4.0, 4.0, 64)
    pre = x.double() @ w.double().T + b.double()
    assert float(pre.min()) < -4.5 and float(pre.max()) > 4.5


@pytest.mark.parametrize("res", ["separate", "in_place"])
@pytest.mark.parametrize("M,K,N,ln,gelu", [(1000, 160, 64, None, False), (65, 32, 65, 1e-6, False), (63, 1024, 256, None, True),
                                           (1, 17, 15, 1e-5, True)])
def test_linear_residual(res, M, K, N, ln, gelu):
    y, ref = _linear(400 + M + K, M, K, N, True, ln=ln, gelu=gelu, res=res)
    check("linear residual %s M%d K%d N%d ln%s gelu%d" % (res, M, K, N, ln, gelu), y, ref, K)


# ---- conv: strided conv over NHWC, optional LayerNorm epilogue ----------------------------------------------------------------------------
CONV = [  # B, Hin, Win, Cin, Cout, ksize, stride, pad, LayerNorm eps (None: no epilogue)
    (1, 1, 1, 3, 17, 1, 1, 0, None),
    (3, 1, 1, 32, 64, 3, 1, 1, None),          # 1 x 1 input: only the centre tap is inside
    (1, 1, 1, 3, 17, 5, 5, 4, 1e-5),
    (1, 5, 7, 1, 1, 2, 1, 0, None),
    (3, 5, 7, 3, 17, 3, 2, 1, 1e-5),           # 12 rows per sample: the 64-row tiles straddle samples
    (1, 33, 17, 32, 64, 3, 2, 1, 1e-5),        # patch_embed2..4
    (3, 33, 17, 160, 256, 4, 3, 2, None),
    (3, 12, 18, 32, 64, 6, 6, 0, None),
    (1, 33, 17, 3, 17, 7, 4, 3, 1e-6),
    (3, 16, 24, 32, 64, 8, 8, 0, None),        # the stage-1 spatial reduction, K = 2048
    (1, 5, 7, 1, 1, 8, 7, 7, None),            # windows mostly in the padding
    (3, 33, 17, 160, 17, 2, 8, 1, None),
    (1, 5, 7, 32, 256, 4, 1, 3, 1e-5),
    (3, 5, 7, 160, 1, 1, 2, 0, None),
    (1, 5, 7, 3, 1, 3, 1, 1, 1e-5),            # LayerNorm over one channel: the LN bias
    (3, 33, 17, 1, 64, 5, 3, 2, None),
    (1, 2, 3, 3, 17, 6, 4, 5, 1e-6),
    (1, 64, 64, 32, 32, 8, 8, 0, None),
    (2, 3, 5, 1024, 1024, 2, 1, 1, 1e-5),      # Cin = Cout = 1024, K = 4096
    (3, 17, 33, 64, 160, 3, 2, 1, 1e-5),
]


@pytest.mark.parametrize("B,Hin,Win,Cin,Cout,ks,stride,pad,eps", CONV)
def test_conv(B, Hin, Win, Cin, Cout, ks, stride, pad, eps):
    g = torch.Generator().manual_seed(500 + Hin * Win + Cin + Cout + ks)
    x = randn(g, B, Hin, Win, Cin)
    w = randn(g, Cout, ks, ks, Cin, scale=(ks * ks * Cin) ** -0.5)
    b = randn(g, Cout, scale=0.1)
    lg, lb = uniform(g, 0.5, 1.5, Cout), randn(g, Cout, scale=0.1)

    def ref(dt):
        v = F.conv2d(x.to(dt).permute(0, 3, 1, 2), w.to(dt).permute(0, 3, 1, 2), b.to(dt), stride=stride, padding=pad).permute(0, 2, 3, 1)
        return F.layer_norm(v, (Cout,), lg.to(dt), lb.to(dt), eps) if eps else v

    Ho, Wo = (Hin + 2 * pad - ks) // stride + 1, (Win + 2 * pad - ks) // stride + 1
    y = torch.empty(B, Ho, Wo, Cout, device=DEV)
    lgd, lbd = (dev(lg), dev(lb)) if eps else (None, None)
    call("conv", dev(x), B, Hin, Win, Cin, dev(w), dev(b), Cout, ks, stride, pad, lgd, lbd, float(eps or 0.0), y)
    check("conv B%d %dx%d Cin%d Cout%d k%d s%d p%d ln%s" % (B, Hin, Win, Cin, Cout, ks, stride, pad, eps), y, ref, ks * ks * Cin)


# ---- embed1: prenet 1x1 conv folded into the 7x7 / s4 patch conv, then LayerNorm 1e-5 -------------------------------------------------
@pytest.mark.parametrize("in_dim", [6, 9])
@pytest.mark.parametrize("H,W", [(32, 32), (32, 96), (96, 32)])
def test_embed1(in_dim, H, W):
    g = torch.Generator().manual_seed(600 + in_dim + H + 2 * W)
    B = 2
    x = uniform(g, -1.0, 1.0, B, in_dim, H, W)
    pw, pb = randn(g, 3, in_dim), randn(g, 3, scale=0.1)
    w, b = randn(g, 32, 7, 7, 3, scale=147 ** -0.5), randn(g, 32, scale=0.1)
    lg, lb = uniform(g, 0.5, 1.5, 32), randn(g, 32, scale=0.1)

    def ref(dt):
        v = F.conv2d(x.to(dt), pw.to(dt)[:, :, None, None] / math.sqrt(in_dim), pb.to(dt))
        v = F.conv2d(v, w.to(dt).permute(0, 3, 1, 2), b.to(dt), stride=4, padding=3).permute(0, 2, 3, 1)
        return F.layer_norm(v, (32,), lg.to(dt), lb.to(dt), 1e-5)

    y = torch.empty(B, H // 4, W // 4, 32, device=DEV)
    call("embed1", dev(x), B, in_dim, H, W, dev(pw), dev(pb), dev(w), dev(b), dev(lg), dev(lb), y)
    check("embed1 in_dim%d %dx%d" % (in_dim, H, W), y, ref, 147)


# ---- layernorm ---------------------------------------------------------------------------------------------------------------------------
def _ln_rows(g, kind, M, C):
    if kind == "normal":
        return randn(g, M, C) * uniform(g, 0.5, 2.0, M, 1) + randn(g, M, 1)
    if kind == "constant":
        return randn(g, M, 1, scale=3.0).expand(M, C).contiguous()
    return randn(g, M, C) + float(kind.split("_")[1]) * uniform(g, 1.0, 2.0, M, 1)        # mean_1e2 ... mean_1e4, std 1


@pytest.mark.parametrize("kind", ["normal", "constant", "mean_1e2", "mean_1e3", "mean_1e4"])
@pytest.mark.parametrize("C", [1, 2, 63, 64, 65, 160, 1024])
def test_layernorm(kind, C):
    M = 1001 if kind == "normal" else 13
    g = torch.Generator().manual_seed(700 + C)
    x = _ln_rows(g, kind, M, C)
    lg, lb = uniform(g, 0.5, 1.5, C), randn(g, C)
    eps = 1e-6 if C % 2 else 1e-5
    in_place = C in (2, 65, 1024)
    xd = dev(x)
    y = xd if in_place else torch.empty_like(xd)
    call("layernorm", xd, M, C, dev(lg), dev(lb), eps, y)
    check("layernorm %s C%d M%d%s" % (kind, C, M, " in place" if in_place else ""), y, lambda dt: F.layer_norm(
        x.to(dt), (C,), lg.to(dt), lb.to(dt), eps), C)


# ---- attention ---------------------------------------------------------------------------------------------------------------------------
def _attention(seed, B, N, L, heads, scale, kind="random", amp=20.0):
    """kind: random | equal (every key the same: equal logits) | peak_first / peak_last / peak_end (one key per (batch, head) with logit
    about +amp for every query: in the first chunk, in the last (ragged) chunk, on key L - 1; with amp = 80 a second key sits at -80)."""
    g = torch.Generator().manual_seed(seed)
    C = 32 * heads
    q, k, v = randn(g, B, N, C), randn(g, B, L, C), randn(g, B, L, C)
    if kind == "equal":
        k = k[:, :1].expand(B, L, C).contiguous()
    elif kind != "random":
        u = randn(g, heads, 32)
        u = u / u.norm(dim=1, keepdim=True)
        a = math.sqrt(amp / scale)
        q = (a * u).reshape(1, 1, C) + 0.3 * q
        k = 0.3 * k
        last0 = (L - 1) // 64 * 64
        j = {"peak_first": min(3, L - 1), "peak_last": last0 + (L - 1 - last0) // 2, "peak_end": L - 1}[kind]
        k[:, j] = (a * u).reshape(1, C)
        if amp >= 80.0 and L > 1:
            k[:, (j + 1) % L] = -(a * u).reshape(1, C)
    kv = torch.cat([k, v], dim=2)

    def ref(dt):
        qh = q.to(dt).reshape(B, N, heads, 32).transpose(1, 2)
        kh = k.to(dt).reshape(B, L, heads, 32).transpose(1, 2)
        vh = v.to(dt).reshape(B, L, heads, 32).transpose(1, 2)
        return (torch.softmax((qh @ kh.transpose(-2, -1)) * scale, dim=-1) @ vh).transpose(1, 2).reshape(B, N, C)

    out = torch.empty(B, N, C, device=DEV)
    call("attention", dev(q), dev(kv), B, N, L, C, heads, scale, out)
    return out, ref


ATT_L = (1, 15, 16, 17, 63, 64, 65, 127, 129, 255, 257, 1000, 1024)
ATT_N, ATT_HEADS = (1, 15, 17, 64, 65, 200), (1, 2, 5, 8)


@pytest.mark.parametrize("i,L", list(enumerate(ATT_L)))
@pytest.mark.parametrize("scale", [32 ** -0.5, 1.0])
def test_attention_random(i, L, scale):
    B, N, heads = (1, 3)[i % 2], ATT_N[i % 6], ATT_HEADS[i % 4]
    out, ref = _attention(800 + L, B, N, L, heads, scale)
    check("attention random B%d N%d L%d heads%d scale%.3g" % (B, N, L, heads, scale), out, ref, max(L, 32))


@pytest.mark.parametrize("L", [1, 17, 64, 65, 257, 1024])
def test_attention_equal_logits(L):
    out, ref = _attention(900 + L, 3, 65, L, 2, 32 ** -0.5, "equal")
    check("attention equal L%d" % L, out, ref, max(L, 32))


@pytest.mark.parametrize("kind", ["peak_first", "peak_last", "peak_end"])
@pytest.mark.parametrize("L,N,heads,B", [(17, 15, 1, 3), (65, 64, 2, 1), (129, 17, 5, 3), (257, 200, 8, 1), (1000, 65, 5, 3),
                                         (1024, 1, 8, 3)])
@pytest.mark.parametrize("amp,scale", [(20.0, 32 ** -0.5), (80.0, 1.0)])
def test_attention_peaked(kind, L, N, heads, B, amp, scale):
    out, ref = _attention(1000 + L + N, B, N, L, heads, scale, kind, amp)
    check("attention %s amp%g L%d N%d heads%d B%d" % (kind, amp, L, N, heads, B), out, ref, max(L, 32))


# ---- depthwise 3x3 + GELU ------------------------------------------------------------------------------------------------------------------
DW_HW = (1, 2, 3, 17)


@pytest.mark.parametrize("C", [1, 3, 128, 1024])
@pytest.mark.parametrize("j,H", list(enumerate(DW_HW)))
def test_dwconv_gelu(C, j, H):
    W = DW_HW[(j + C) % 4]
    B = 2
    g = torch.Generator().manual_seed(1100 + C + H + W)
    x, w, b = uniform(g, -10.0, 10.0, B, H, W, C), randn(g, C, 1, 3, 3, scale=1.0 / 3.0), uniform(g, -1.0, 1.0, C)

    def ref(dt):
        v = F.conv2d(x.to(dt).permute(0, 3, 1, 2), w.to(dt), b.to(dt), padding=1, groups=C)
        return F.gelu(v).permute(0, 2, 3, 1)

    y = torch.empty(B, H, W, C, device=DEV)
    call("dwconv_gelu", dev(x), B, H, W, C, dev(w), dev(b), y)
    check("dwconv_gelu C%d %dx%d" % (C, H, W), y, ref, 9)


# ---- head: c1 GEMM + bilinear samples of the folded maps + constant, BatchNorm, ReLU ----------------------------------------------------
@pytest.mark.parametrize("H1,W1", [(8, 8), (8, 256), (256, 8), (72, 64)])
def test_head(H1, W1):
    B = 2
    g = torch.Generator().manual_seed(1200 + H1 + 3 * W1)
    c1, w1f = randn(g, B, H1, W1, 32), randn(g, 256, 32, scale=32 ** -0.5)
    fs = [randn(g, B, H1 >> s, W1 >> s, 256) for s in (1, 2, 3)]
    hconst = randn(g, 256, scale=0.1)
    sign = torch.where(torch.rand(256, generator=g) < 0.2, -1.0, 1.0)
    bn_s, bn_t = sign * uniform(g, 0.5, 1.5, 256), uniform(g, 1.5, 2.5, 256)

    def ref(dt):
        z = torch.einsum("bhwc,oc->bohw", c1.to(dt), w1f.to(dt)) + hconst.to(dt)[None, :, None, None]
        for f in fs:
            z = z + F.interpolate(f.to(dt).permute(0, 3, 1, 2), size=(H1, W1), mode="bilinear", align_corners=False)
        return torch.relu(z * bn_s.to(dt)[None, :, None, None] + bn_t.to(dt)[None, :, None, None])

    out = torch.empty(B, 256, H1, W1, device=DEV)
    call("head", dev(c1), B, H1, W1, dev(w1f), dev(fs[0]), dev(fs[1]), dev(fs[2]), dev(hconst), dev(bn_s),
         dev(bn_t), out)
    y64 = check("head %dx%d" % (H1, W1), out, ref, 32)
    clipped = float((y64 == 0).double().mean())
    assert 0.05 < clipped < 0.5, clipped          # ReLU clips some outputs, not most


# ---- the call path (_lib.call) against the raw idiom of `call` above ------------------------------------------------------
def _layernorm_case():
    """M = 5 rows of C = 32: the last block of four rows is ragged."""
    g = torch.Generator().manual_seed(811)
    return dev(randn(g, 5, 32)), dev(uniform(g, 0.5, 1.5, 32)), dev(randn(g, 32, scale=0.1))


def test_call_path_and_raw_idiom_are_bit_identical():
    x, lg, lb = _layernorm_case()
    raw, via = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
    call("layernorm", x, 5, 32, lg, lb, 1e-5, raw)
    _lib.call("r3d_secc_layernorm", x, 5, 32, lg, lb, 1e-5, via)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(raw).all()) and torch.equal(raw, via)          # the same kernel with the same arguments: no tolerance


def test_call_path_passes_the_current_stream_or_the_one_given():
    x, lg, lb = _layernorm_case()
    y, side, other = torch.empty_like(x), torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    other.wait_stream(torch.cuda.current_stream(DEV))
    with _lib.counting() as calls:
        with torch.cuda.stream(side):
            _lib.call("r3d_secc_layernorm", x, 5, 32, lg, lb, 1e-5, y)
            side.synchronize()
            _lib.call("r3d_secc_layernorm", x, 5, 32, lg, lb, 1e-5, y, other.cuda_stream)          # explicit: used as given
            other.synchronize()
    assert [n for n, _ in calls] == ["r3d_secc_layernorm"] * 2
    assert calls[0][1] == (x.data_ptr(), 5, 32, lg.data_ptr(), lb.data_ptr(), 1e-5, y.data_ptr(), side.cuda_stream)
    assert calls[1][1][-1] == other.cuda_stream != side.cuda_stream


def test_call_path_refuses_device_tensors_before_any_launch():
    x, lg, lb = _layernorm_case()
    y = torch.empty_like(x)
    with _lib.counting() as calls:
        with pytest.raises(ValueError, match="r3d_secc_layernorm: argument 0 .* not contiguous"):
            _lib.call("r3d_secc_layernorm", dev(torch.zeros(5, 64))[:, ::2], 5, 32, lg, lb, 1e-5, y)
        with pytest.raises(TypeError, match=r"r3d_secc_layernorm: argument 6 is a float\*, got a torch.int32"):
            _lib.call("r3d_secc_layernorm", x, 5, 32, lg, lb, 1e-5, torch.zeros(5, 32, dtype=torch.int32, device=DEV))
    assert calls == []
