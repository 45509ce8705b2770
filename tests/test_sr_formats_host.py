"""CPU: tests/sr_formats.py against itself -- the decoder reads what the independently written encoder wrote, check_split accepts a correct
tensor and rejects every layout / rounding slip the GPU tests rely on it to see, and the resampling references of tests/test_gpu_sr_ops.py are
sensitive to the conventions they state (align_corners, antialias) far beyond the bound they are compared under."""
import pytest
import torch

import sr_formats as SF


def _values(seed, N, C, H, W):
    """Scaled activations over the whole fp16 window: most around 2^0 .. 2^13, some tiny (fp16-subnormal hi and lo), exact zeros, both signs."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(N, C, H, W, generator=g) * torch.exp2(torch.randint(-3, 13, (N, C, H, W), generator=g).float())
    tiny = torch.rand(N, C, H, W, generator=g) < 0.1
    t = torch.where(tiny, t * 2.0 ** -24, t)
    t = torch.where(torch.rand(N, C, H, W, generator=g) < 0.05, torch.zeros_like(t), t)
    return t.clamp(-50000.0, 50000.0)


SHAPES = [(N, Ca + Cb, H, W) for N, Ca, Cb, H, W, _, _ in SF.BLEND_CAT_CASES]


@pytest.mark.parametrize("N,C,H,W", SHAPES)
def test_encode_decode_round_trip_and_check_accepts(N, C, H, W):
    t = _values(10 + C + H, N, C, H, W)
    hi_ref, lo_ref = SF.split_ref(t)
    y = SF.encode_split_ref(t)
    hi, lo = SF.decode_split(y, C)
    assert torch.equal(hi, hi_ref.float()) and torch.equal(lo, lo_ref.float())
    SF.check_split(y, t.double(), mx=False, exact_lo=True)
    ymx = SF.encode_split_mx_ref(t)
    hi, xh8, xl8 = SF.decode_split_mx(ymx, C)
    assert torch.equal(hi, hi_ref.float())
    assert torch.equal(xh8, hi_ref.float().to(torch.float8_e5m2).float())
    assert torch.equal(xl8, ((t - hi_ref.float()) * SF.XL8_SCALE).to(torch.float8_e5m2).float())
    SF.check_split(ymx, t.double(), mx=True)


def test_record_layout_is_the_documented_one():
    """One pixel, one group, channel c holding 2^c (exact in e5m2): dword d = 2 h + p of the record holds channels 8 p + 4 h .. + 3."""
    t = torch.exp2(torch.arange(16).float()).view(1, 16, 1, 1)
    y = SF.encode_split_mx_ref(t)
    rec = y[0, 1, 0, 0, 0].view(torch.uint8).view(torch.float8_e5m2).float().log2().tolist()        # xh8: "lo" chunk 0
    assert rec == [0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15]
    assert y[0, 0, :, 0, 0].float().log2().flatten().tolist() == list(range(16))                     # hi: chunk-major, channel-minor
    hi, xh8, xl8 = SF.decode_split_mx(y, 16)
    assert torch.equal(hi, t) and torch.equal(xh8, t) and not bool(xl8.any())


def _swap_chunks(plane, i, j):
    p = plane.clone()
    p[:, i], p[:, j] = plane[:, j], plane[:, i]
    return p


def _mutations(t):
    """{name: (tensor, mx)}: each a correct encoding of t with one slip a kernel could make."""
    N, C, H, W = t.shape
    y, ymx = SF.encode_split_ref(t), SF.encode_split_mx_ref(t)
    out = {}
    m = ymx.clone(); m[:, 1] = _swap_chunks(ymx[:, 1], 0, 1); out["xh8 and xl8 chunks exchanged"] = (m, True)
    m = ymx.clone(); m[:, 0] = _swap_chunks(ymx[:, 0], 0, 1); out["hi chunks of a group exchanged (mx)"] = (m, True)
    m = y.clone(); m[:, 0] = _swap_chunks(y[:, 0], C // 8 - 2, C // 8 - 1); m[:, 1] = _swap_chunks(y[:, 1], C // 8 - 2, C // 8 - 1)
    out["both chunks of a group exchanged (split)"] = (m, False)
    m = y.clone(); m[:, 1] = _swap_chunks(y[:, 1], 0, 1); out["lo chunks of a group exchanged (split)"] = (m, False)
    rec = ymx[:, 1].contiguous().view(torch.uint8).reshape(N, C // 8, H, W, 4, 4).clone()
    rec[..., [1, 2], :] = rec[..., [2, 1], :]
    m = ymx.clone(); m[:, 1] = rec.reshape(N, C // 8, H, W, 16).view(torch.float16); out["dwords 1 and 2 of a record exchanged"] = (m, True)
    m = y.clone(); m[:, 1] = 0.0; out["lo = fp16(t) - hi"] = (m, False)
    hi = SF.split_ref(t)[0]
    away = hi.float().abs() > t.abs()                                   # rounded away from zero: step one fp16 back toward zero
    hz = torch.where(away, (SF._bits(hi) - 1).view(torch.float16), hi)  # (sign-magnitude: bits - 1 is the next value toward zero for either sign)
    lz = (t - hz.float()).half()
    m = torch.stack([SF._nchw_to_plane(hz), SF._nchw_to_plane(lz)], dim=1); out["hi rounded toward zero"] = (m, False)
    return out


@pytest.mark.parametrize("N,C,H,W", SHAPES)
def test_check_split_rejects_layout_and_rounding_slips(N, C, H, W):
    t = _values(20 + C + W, N, C, H, W)
    muts = _mutations(t)
    assert len(muts) == 7
    for name, (y, mx) in muts.items():
        with pytest.raises(AssertionError):
            SF.check_split(y, t.double(), mx=mx, exact_lo=False, what=name)
    # the truncated hi is a consistent split otherwise: it is the bit-exactness of hi that sees it, not the sum
    y, _ = muts["hi rounded toward zero"]
    hi, lo = SF.decode_split(y, C)
    assert float(((hi.double() + lo.double() - t.double()).abs() - (t.double().abs() * 2.0 ** -21 + 2.0 ** -24)).max()) <= 0.0


def test_check_split_accepts_either_tie_rule_of_the_records():
    """A record rounded to the other neighbour on an exact e5m2 tie (hi = 1.125: between 1.0 and 1.25) passes: the bound is half an ulp."""
    t = torch.full((1, 16, 1, 1), 1.125)
    y = SF.encode_split_mx_ref(t)
    b = y[:, 1].contiguous().view(torch.uint8).clone()
    xh = b[0, 0, 0, 0]
    assert set(xh.tolist()) == {0x3C}                                    # ties-to-even: 1.0
    b[0, 0, 0, 0] = 0x3D                                                 # 1.25
    y2 = y.clone(); y2[:, 1] = b.view(torch.float16)
    SF.check_split(y, t.double(), mx=True)
    SF.check_split(y2, t.double(), mx=True)
    b[0, 0, 0, 0] = 0x3E                                                 # 1.5: a whole ulp off
    y3 = y.clone(); y3[:, 1] = b.view(torch.float16)
    with pytest.raises(AssertionError):
        SF.check_split(y3, t.double(), mx=True)


# ---- the references are visibly shape-sensitive (as test_conv_prologue_padding_rule_is_visible_to_the_check) ---------------------------------
@pytest.mark.parametrize("N,C,H,W", SF.UPSAMPLE_SHAPES)
def test_upsample_reference_sees_align_corners(N, C, H, W):
    g = torch.Generator().manual_seed(30 + H + W)
    x = torch.randn(N, C, H, W, generator=g)
    y64, e32, bound = SF.error_bound(SF.upsample_ref(x), 4)
    wrong = SF.upsample_ref(x, align_corners=False)(torch.float64)
    d = float((wrong - y64).abs().max() / y64.abs().max())
    if H * W == 1:
        assert d == 0.0             # one input pixel: every output pixel is that pixel under either convention
    else:
        assert d > 100.0 * bound, (d, bound)


@pytest.mark.parametrize("planes,H,W,OH,OW", SF.RESIZE_SHAPES)
def test_resize_reference_sees_antialias(planes, H, W, OH, OW):
    g = torch.Generator().manual_seed(40 + H + OW)
    x = torch.randn(1, planes, H, W, generator=g)
    keff = SF.resize_keff(H, W, OH, OW)
    y64, e32, bound = SF.error_bound(SF.resize_ref(x, OH, OW, True), keff)
    wrong = SF.resize_ref(x, OH, OW, False)(torch.float64)
    d = float((wrong - y64).abs().max() / y64.abs().max())
    if H > OH or W > OW:
        assert d > 100.0 * bound, (d, bound)
    else:
        assert d <= 1e-12           # no axis shrinks: the antialiased window is the plain bilinear one
    assert keff >= 9


def test_resize_identity_reference_is_the_input():
    x = torch.randn(1, 2, 5, 9, generator=torch.Generator().manual_seed(3))
    for aa in (0, 1):
        assert torch.equal(SF.resize_ref(x, 5, 9, aa)(torch.float32), x)


@pytest.mark.parametrize("antialias", [0, 1])
@pytest.mark.parametrize("planes,H,W,OH,OW", SF.RESIZE_SHAPES)
def test_resize_reference_is_the_stated_formula(planes, H, W, OH, OW, antialias):
    """The reference of tests/test_gpu_sr_ops.py::test_resize_bilinear against the separable weights written out (float64, a few ulps): torch's
    antialiased CPU kernel misreads a one-column image, which resize_ref evaluates as its transpose."""
    x = torch.randn(1, planes, H, W, generator=torch.Generator().manual_seed(50 + H + OH))
    want = SF.resize_spelled_out(x, OH, OW, antialias)
    got = SF.resize_ref(x, OH, OW, antialias)(torch.float64)
    assert got.shape == want.shape
    assert float((got - want).abs().max()) <= 1e-13 * float(want.abs().max())
