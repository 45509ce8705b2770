"""The SPLIT / SPLIT_MX activation formats of the SR path (include/r3d_hip.h r3d_act_format) restated in plain torch on the
CPU: what a producer must write, how to read it back, and the contract a written tensor is held to (check_split).  Imported by
tests/test_gpu_sr_ops.py and tests/test_sr_formats_host.py the way tests/torso_ref64.py is; it never imports the library.

  SPLIT      fp16 [N][hi|lo][C/8][H][W][8]: hi = fp16(clamp(t, +-65504)), lo = fp16(t - hi), t the fp32 activation ALREADY multiplied by the
             consumer's in-multiplier.
  SPLIT_MX   the same hi plane; the lo plane holds, in its place, 8-bit OCP e5m2 records: "lo" chunk 2G = xh8 = e5m2(hi) of channels
             16G .. 16G+15, "lo" chunk 2G+1 = xl8 = e5m2((t - hi) 2^11).  Per pixel a record is 16 bytes = 4 dwords; dwords (cb & 1) and
             2 + (cb & 1) carry channels 0-3 and 4-7 of the 8-channel chunk cb (blend_cat_to_split_kernel, csrc/r3d_sr_f16x3.hip).

Also here, because the GPU tests and the host test share them: the case lists of the resampling tests and their float64 references."""
import math

import torch
import torch.nn.functional as F

F16_MAX = 65504.0
E5M2_MAX = 57344.0
XL8_SCALE = 2048.0          # xl8 = e5m2(lo * 2^11)

# byte of a 16-byte record that holds channel ch (0..15) of its group: chunk p = ch / 8, half h = (ch % 8) / 4 -> dword 2 h + p
REC_BYTE = [4 * (2 * ((ch % 8) // 4) + ch // 8) + ch % 4 for ch in range(16)]


def split_ref(t32):
    """(hi, lo) fp16 as every producer computes them from the scaled fp32 value."""
    t32 = t32.float()
    hi = t32.clamp(-F16_MAX, F16_MAX).half()
    lo = (t32 - hi.float()).half()
    return hi, lo


def _plane_to_nchw(p, C):
    """[N, C/8, H, W, 8] -> [N, C, H, W]"""
    N, C8, H, W, _ = p.shape
    assert C8 * 8 == C
    return p.permute(0, 1, 4, 2, 3).reshape(N, C, H, W)


def _nchw_to_plane(t):
    N, C, H, W = t.shape
    return t.reshape(N, C // 8, 8, H, W).permute(0, 1, 3, 4, 2).contiguous()


def decode_split(y, C):
    """y: fp16 [N, 2, C/8, H, W, 8] -> (hi, lo) float32 [N, C, H, W]."""
    assert y.dtype == torch.float16 and y.dim() == 6 and y.shape[1] == 2 and y.shape[2] * 8 == C and y.shape[5] == 8, y.shape
    y = y.cpu()
    return _plane_to_nchw(y[:, 0], C).float(), _plane_to_nchw(y[:, 1], C).float()


def decode_split_mx(y, C):
    """y: fp16 [N, 2, C/8, H, W, 8] written as SPLIT_MX -> (hi, xh8, xl8) float32 [N, C, H, W]; xl8 is the record's value, lo * 2^11."""
    assert C % 16 == 0
    hi, _ = decode_split(y, C)
    N, _, C8, H, W, _ = y.shape
    rec = y.cpu()[:, 1].contiguous().view(torch.uint8).reshape(N, C // 16, 2, H, W, 16)      # [group][xh8 | xl8][pixel][16 bytes]
    rec = rec[..., REC_BYTE]                                                                    # bytes in channel order
    val = rec.contiguous().view(torch.float8_e5m2).float()
    val = val.permute(0, 1, 2, 5, 3, 4)                                                         # [N, G, kind, 16, H, W]
    return hi, val[:, :, 0].reshape(N, C, H, W), val[:, :, 1].reshape(N, C, H, W)


def encode_split_ref(t32):
    """SPLIT written from Python: fp16 [N, 2, C/8, H, W, 8]."""
    hi, lo = split_ref(t32)
    return torch.stack([_nchw_to_plane(hi), _nchw_to_plane(lo)], dim=1).contiguous()


def encode_split_mx_ref(t32):
    """SPLIT_MX written from Python (the layout of the kernels, stated independently of decode_split_mx: byte by byte)."""
    t32 = t32.float()
    N, C, H, W = t32.shape
    assert C % 16 == 0 and float(t32.abs().max()) < E5M2_MAX
    hi, _ = split_ref(t32)
    lo32 = t32 - hi.float()
    xh8 = hi.float().to(torch.float8_e5m2).view(torch.uint8)
    xl8 = (lo32 * XL8_SCALE).to(torch.float8_e5m2).view(torch.uint8)
    rec = torch.zeros(N, C // 16, 2, H, W, 16, dtype=torch.uint8)
    for ch in range(16):
        chunk, half, k = ch // 8, (ch % 8) // 4, ch % 4
        dword = half * 2 + chunk
        rec[:, :, 0, :, :, 4 * dword + k] = xh8[:, ch::16]
        rec[:, :, 1, :, :, 4 * dword + k] = xl8[:, ch::16]
    lo_plane = rec.reshape(N, C // 8, H, W, 16).view(torch.float16)                             # [N, C/8, H, W, 8]
    return torch.stack([_nchw_to_plane(hi), lo_plane], dim=1).contiguous()


def _bits(h):
    return h.contiguous().view(torch.int16)


def _e5m2_close(what, got, want):
    """|got - want| <= half an e5m2 ulp of want: 2^-3 |want| in the normal range (2 mantissa bits), 2^-17 below 2^-14 (subnormal step 2^-16)."""
    want = want.double()
    tol = torch.where(want.abs() >= 2.0 ** -14, want.abs() * 2.0 ** -3, torch.full_like(want, 2.0 ** -17))
    bad = (got.double() - want).abs() > tol
    assert not bool(bad.any()), "%s: %d records off by more than half an e5m2 ulp, first at %s" % (what, int(bad.sum()), bad.nonzero()[0].tolist())


def check_split(y, t64, mx, exact_lo=False, what="split"):
    """y: a written SPLIT (mx False) / SPLIT_MX (mx True) tensor, fp16 [N, 2, C/8, H, W, 8]; t64: the exact scaled value it stands for,
    float64 [N, C, H, W].  Every bound follows from the formats:
      hi            == fp16 round-to-nearest-even of fp32(t), bit for bit, wherever |t| < 65504;
      SPLIT         |hi + lo - t| <= 2^-22 |t| + 2^-25: fp32 rounding of t (2^-24 |t|), the residual t32 - hi (at most half an fp16 ulp of hi,
                    i.e. 11 bits below it) rounded to fp16's 11 bits (2^-23 |t|), and half the fp16 subnormal step;
                    exact_lo (t is exact in fp32: a power-of-two multiplier): lo == split_ref(t).lo bit for bit;
      SPLIT_MX      xh8 within half an e5m2 ulp of hi, xl8 within half an e5m2 ulp of (fp32(t) - hi) 2^11 (either tie rule passes).
    Raises AssertionError."""
    t64 = t64.double().cpu()
    N, C, H, W = t64.shape
    assert tuple(y.shape) == (N, 2, C // 8, H, W, 8), (what, tuple(y.shape), tuple(t64.shape))
    assert bool(torch.isfinite(t64).all()), what
    t32 = t64.float()
    hi_ref, lo_ref = split_ref(t32)
    inside = t64.abs() < F16_MAX
    if mx:
        assert float(t64.abs().max()) < E5M2_MAX, "%s: keep SPLIT_MX test values below the e5m2 maximum" % what
        hi, xh8, xl8 = decode_split_mx(y, C)
    else:
        hi, lo = decode_split(y, C)
    bad = (_bits(hi.half()) != _bits(hi_ref)) & inside
    assert not bool(bad.any()), "%s: hi differs from fp16(fp32(t)) at %d of %d values, first at %s" % (what, int(bad.sum()), bad.numel(), bad.nonzero()[0].tolist())
    if mx:
        _e5m2_close(what + " xh8", xh8, hi)
        _e5m2_close(what + " xl8", xl8, (t32 - hi) * XL8_SCALE)
        return
    err = (hi.double() + lo.double() - t64).abs()
    bad = (err > t64.abs() * 2.0 ** -22 + 2.0 ** -25) & inside
    assert not bool(bad.any()), "%s: hi + lo misses t at %d values, first at %s (err %.3e)" % (what, int(bad.sum()), bad.nonzero()[0].tolist(), float(err[bad].max()))
    if exact_lo:
        assert bool((t32.double() == t64).all()), "%s: exact_lo needs a t that is exact in fp32" % what
        bad = (_bits(lo.half()) != _bits(lo_ref)) & inside
        assert not bool(bad.any()), "%s: lo differs from fp16(t - hi) at %d values, first at %s" % (what, int(bad.sum()), bad.nonzero()[0].tolist())


# ---- the one error rule of the *_ops tests (tests/test_gpu_torso_ops.py check), for a result that is already on the CPU ------------------
FLOOR = 2.0 ** -22


def error_bound(ref, keff):
    """(y64, bound): bound = max(2^-22 sqrt(K_eff), 4 e32) on max|y - y64| / max|y64|, e32 the same statement in fp32 on the CPU."""
    y64, y32 = ref(torch.float64), ref(torch.float32).double()
    m = float(y64.abs().max())
    assert m > 0.0
    e32 = float((y32 - y64).abs().max()) / m
    return y64, e32, max(FLOOR * math.sqrt(keff), 4.0 * e32)


# ---- r3d_upsample2x_bilinear (test 2a) ------------------------------------------------------------------------------------------------------
UPSAMPLE_SHAPES = [(1, 8, 1, 1), (2, 16, 1, 5), (1, 16, 7, 1), (1, 24, 5, 9), (2, 32, 33, 17)]      # N, C, H, W; the last: 2244 output pixels


def upsample_ref(x, align_corners=True):
    return lambda dt: F.interpolate(x.to(dt), scale_factor=2, mode="bilinear", align_corners=align_corners)


# ---- r3d_blend_cat_to_split (test 2b) -------------------------------------------------------------------------------------------------------
BLEND_CAT_CASES = [(1, 8, 8, 1, 1, "nchw", "nchw"), (2, 24, 40, 7, 9, "cb8", "nchw"), (1, 16, 48, 17, 16, "nchw", "cb8"), (2, 32, 32, 5, 3, "cb8", "cb8")]


# ---- r3d_resize_bilinear (test 2c) ----------------------------------------------------------------------------------------------------------
RESIZE_SHAPES = [(1, 1, 1, 3, 4), (3, 7, 5, 1, 1), (1, 37, 53, 5, 3), (2, 3, 4, 17, 23), (1, 16, 16, 17, 15), (1, 300, 1, 128, 1), (2, 5, 9, 5, 9)]


def resize_ref(x, OH, OW, antialias):
    """F.interpolate(size=(OH, OW), mode='bilinear', align_corners=False, antialias=A) on the CPU.  A one-column image ([.., H, 1] -> [.., OH, 1]) is
    evaluated as its transpose ([.., 1, H] -> [.., 1, OH]), the same operation with the axes renamed: a dense [N, C, H, 1] tensor is also a valid
    channels-last one, and torch's antialiased CPU kernel then reads it with the wrong strides (torch 2.10: every output row equals the first;
    resize_spelled_out and tests/test_sr_formats_host.py pin this reference to the formula)."""
    def ref(dt):
        t = x.to(dt)
        if t.shape[-1] == 1 and OW == 1 and t.shape[-2] > 1:
            return F.interpolate(t.transpose(-1, -2).contiguous(), size=(1, OH), mode="bilinear", align_corners=False, antialias=bool(antialias)).transpose(-1, -2)
        return F.interpolate(t, size=(OH, OW), mode="bilinear", align_corners=False, antialias=bool(antialias))
    return ref


def _resize_matrix(n_in, n_out, antialias):
    """[n_out, n_in] float64: ATen's separable weights (UpSampleKernel.cpp _compute_indices_weights_aa): scale = in / out, support = max(scale, 1) when
    antialiased and 1 otherwise, centre = scale (i + 0.5), taps [int(centre - support + 0.5), int(centre + support + 0.5)) clipped to the image,
    triangle weights normalised to sum 1."""
    scale = n_in / n_out
    sup = max(scale, 1.0) if antialias else 1.0
    M = torch.zeros(n_out, n_in, dtype=torch.float64)
    for i in range(n_out):
        c = scale * (i + 0.5)
        lo, hi = max(int(c - sup + 0.5), 0), min(int(c + sup + 0.5), n_in)
        w = torch.tensor([max(0.0, 1.0 - abs((j - c + 0.5) / sup)) for j in range(lo, hi)], dtype=torch.float64)
        M[i, lo:hi] = w / w.sum()
    return M


def resize_spelled_out(x, OH, OW, antialias):
    """The same resize as two matrix products in float64."""
    My, Mx = _resize_matrix(x.shape[-2], OH, antialias), _resize_matrix(x.shape[-1], OW, antialias)
    return My @ x.double() @ Mx.t()


def resize_keff(H, W, OH, OW):
    """taps_y taps_x with taps = 2 max(scale, 1) + 1, rounded up: the widest antialiased window."""
    taps = lambda i, o: int(math.ceil(2.0 * max(i / o, 1.0) + 1.0))
    return taps(H, OH) * taps(W, OW)
