"""CPU: the bf16x3 tier of the torso convolutions (real3dportrait_amd/torso_precision.py) as far as it can be held without a
GPU: the host mirror of the split is exact and its pieces are bf16, a CPU model of the kernels' arithmetic (three pieces, six products in
the kernels' order, fp32 accumulation in 32-wide steps) is fp32-class, the option is validated everywhere it is accepted, and the new
kernels use no scratch."""
import ctypes
import math

import pytest
import torch

from real3dportrait_amd.torso_precision import BF16_MAX, PRECISIONS, split_bf16x3
from test_torso_generator_host import model_shell, reference_like_torso_model

FP32_MAX = float.fromhex("0x1.fffffep127")
ORDER = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))          # (activation piece, weight piece): l.h, h.l, m.m, m.h, h.m, h.h


def edge_values():
    """Every power of two from 2^-100 to 2^127 times (1, 1 + 2^-23, 2 - 2^-23), both signs, +-0 and fp32 max (= 2^127 (2 - 2^-23))."""
    p = torch.tensor([2.0 ** e for e in range(-100, 128)], dtype=torch.float64)
    f = torch.tensor([1.0, 1.0 + 2.0 ** -23, 2.0 - 2.0 ** -23], dtype=torch.float64)
    v = (p[:, None] * f[None, :]).reshape(-1)
    v = torch.cat([v, -v, torch.tensor([0.0, -0.0, FP32_MAX, -FP32_MAX], dtype=torch.float64)])
    v32 = v.float()
    assert torch.equal(v32.double(), v) and bool(torch.isfinite(v32).all())          # every value is an fp32 number
    return v32


def split_values():
    """The value set of the split tests, here and on the GPU: 1 M Gaussian values and the edge values."""
    g = torch.Generator().manual_seed(11)
    return torch.cat([torch.randn(1 << 20, generator=g), edge_values()])


def test_split_is_exact():
    x = split_values()
    h, m, l = split_bf16x3(x)
    assert h.dtype == m.dtype == l.dtype == torch.bfloat16
    assert torch.equal(h.double() + m.double() + l.double(), x.double())
    assert torch.equal((l.float() + m.float()) + h.float(), x)                       # ... and in fp32, smallest first (h + m of fp32 max is 2^128)
    assert bool(torch.isfinite(h.float()).all())
    xm = torch.tensor([FP32_MAX, -FP32_MAX])
    hm = split_bf16x3(xm)[0]
    assert torch.equal(hm.float(), torch.tensor([BF16_MAX, -BF16_MAX]))              # the clamp, not an infinity
    # the pieces shrink by 2^-8 each (round to nearest: |m| <= ulp_bf16(h) / 2 = 2^-8 |h| at most)
    nz = (x != 0) & (x.abs() <= BF16_MAX)          # (above BF16_MAX the clamp leaves m up to 2^-7 of h)
    assert bool((m.float().abs()[nz] <= h.float().abs()[nz] * 2.0 ** -8).all()) and bool((l.float().abs()[nz] <= h.float().abs()[nz] * 2.0 ** -16).all())


def test_pieces_are_bf16():
    """A piece widened to fp32 has its lower 16 bits clear (and is what the bfloat16 tensor holds)."""
    for p in split_bf16x3(split_values()):
        bits = p.float().view(torch.int32)
        assert int((bits & 0xFFFF).abs().max()) == 0
        assert torch.equal(p.float().to(torch.bfloat16), p)
    with pytest.raises(ValueError):
        split_bf16x3(torch.zeros(4, dtype=torch.float64))


def model_gemm(a, b, step=32):
    """a [M, K] @ b [K, N] as the kernels evaluate it: both operands split, per 32 k entries the six products in ORDER, each added to the
    fp32 accumulator.  Returns (fp32 model, the six products summed in fp64)."""
    pa, pb = [p.float() for p in split_bf16x3(a)], [p.float() for p in split_bf16x3(b)]
    acc = torch.zeros(a.shape[0], b.shape[1])
    for k0 in range(0, a.shape[1], step):
        for i, j in ORDER:
            acc = acc + pa[i][:, k0:k0 + step] @ pb[j][k0:k0 + step]
    six = sum(pa[i].double() @ pb[j].double() for i, j in ORDER)
    return acc, six


@pytest.mark.parametrize("K", [32, 252, 4361, 31556])
@pytest.mark.parametrize("spread", [0, 12])
def test_cpu_model_is_fp32_class(K, spread):
    """spread: per-element scales 2^+-spread on both operands (the split has no range to fall out of)."""
    torch.set_num_threads(8)
    g = torch.Generator().manual_seed(100 + K + spread)
    a, b = torch.randn(48, K, generator=g), torch.randn(K, 40, generator=g)
    if spread:
        a = a * 2.0 ** torch.randint(-spread, spread + 1, a.shape, generator=g).float()
        b = b * 2.0 ** torch.randint(-spread, spread + 1, b.shape, generator=g).float()
    ref = a.double() @ b.double()
    m = float(ref.abs().max())
    acc, six = model_gemm(a, b)
    e = float((acc.double() - ref).abs().max()) / m
    e32 = float(((a @ b).double() - ref).abs().max()) / m
    e6 = float((six - ref).abs().max()) / m
    bound = max(2.0 ** -22 * math.sqrt(K), 4.0 * e32)
    print("K %d spread %d: model %.2e  fp32 %.2e  bound %.2e  six products in fp64 %.2e" % (K, spread, e, e32, bound, e6))
    assert e <= bound, (e, e32, bound)
    assert e6 <= 2e-8, e6          # about 2 x 2^-24: the three products left out


def test_precision_names_are_validated():
    from real3dportrait_amd import Occlusion2Predictor, TorsoGenerator, TorsoMotionFieldEstimator, patch_model
    assert PRECISIONS == {"f32": 0, "bf16x3": 1}
    for cls in (TorsoGenerator, Occlusion2Predictor, TorsoMotionFieldEstimator):
        assert cls().precision == "f32" and cls(precision="bf16x3").precision == "bf16x3"
        for bad in ("bf16", "F32", None, 1):
            with pytest.raises(ValueError):
                cls(precision=bad)
    with pytest.raises(ValueError):
        patch_model(model_shell(reference_like_torso_model()), torso_precision="bf16x3")             # without either switch
    with pytest.raises(ValueError):
        patch_model(model_shell(reference_like_torso_model()), torso_generator=True, torso_precision="fp16")
    for given, want in ((None, "f32"), ("f32", "f32"), ("bf16x3", "bf16x3")):
        tm = reference_like_torso_model()
        patch_model(model_shell(tm), torso_generator=True, torso_precision=given)
        assert isinstance(tm.deform_based_generator, TorsoGenerator) and tm.deform_based_generator.precision == want
        assert isinstance(tm.occlusion_2_predictor, Occlusion2Predictor) and tm.occlusion_2_predictor.precision == want


def test_patch_model_passes_the_precision_to_the_motion_estimator():
    from real3dportrait_amd import TorsoMotionFieldEstimator, patch_model
    from test_torso_motion_host import reference_like_estimator, torso_model_with
    tm = torso_model_with(reference_like_estimator(5, 4))
    patch_model(model_shell(tm), torso_motion=True, torso_precision="bf16x3")
    assert isinstance(tm.motion_field_estimator, TorsoMotionFieldEstimator) and tm.motion_field_estimator.precision == "bf16x3"
    assert type(tm.deform_based_generator).__name__ == "Generator" and not hasattr(tm.deform_based_generator, "precision")     # not switched on


def test_prec_entry_points_reject_bad_arguments_without_a_gpu():
    """The checks of r3d_torso_conv / r3d_torso_conv3d, plus the precision's (validation runs before any HIP call)."""
    from real3dportrait_amd import _lib
    lib = _lib.load()
    at = lambda i: ctypes.c_void_p((1 << 30) + 4 * i)       # never dereferenced: validation fails first
    far = ctypes.c_void_p(1 << 40)
    err = lambda: lib.r3d_last_error()
    conv = lambda prec, x=at(0), k=3, y=far: lib.r3d_torso_conv_prec(x, 1, 8, 8, 32, 0, 0, None, None, 0.0, far, None, 64, k, 0, 0.0, None, y, None, prec, None)
    conv3 = lambda prec, x=at(0), k=3, y=far: lib.r3d_torso_conv3d_prec(x, 1, 2, 8, 8, 32, 0, far, None, 64, k, 0, 0, 0.0, 0, y, 64, 0, None, prec, None)
    for f, name in ((conv, b"torso_conv:"), (conv3, b"torso_conv3d:")):
        for bad in (2, -1, 7):
            assert f(bad) == -1 and name in err() and b"precision %d" % bad in err()
        for prec in (0, 1):
            assert f(prec, x=None) == -1 and b"NULL" in err()
            assert f(prec, k=5) == -1 and b"ksize 5" in err()
            assert f(prec, y=at(100)) == -1 and b"overlaps x" in err()
    h = ctypes.c_void_p(1 << 41)
    assert lib.r3d_torso_split_bf16x3(None, 4, far, h, at(0), None) == -1 and b"NULL" in err()
    assert lib.r3d_torso_split_bf16x3(at(0), 0, far, h, ctypes.c_void_p(1 << 42), None) == -1 and b"n is not" in err()
    assert lib.r3d_torso_split_bf16x3(at(0), 64, at(8), h, far, None) == -1 and b"overlaps x" in err()
    assert lib.r3d_torso_split_bf16x3(at(0), 64, far, far, h, None) == -1 and b"outputs overlap" in err()


def test_bf16x3_kernels_do_not_use_scratch_and_keep_two_blocks_per_cu():
    from test_render_kernel_resources import _kernel_metadata
    from real3dportrait_amd import _lib
    meta = _kernel_metadata(_lib.LIB_PATH)
    names = [k for k in meta if "9torso_bf3" in k or "11tmotion_bf3" in k]
    assert len(names) == 19, names          # torso_conv x (4 tiles x 2 loaders), torso_split, conv3d x (5 tiles x 2 loaders)
    for k in names:
        assert int(meta[k]["private_segment_fixed_size"]) == 0, (k, meta[k])
        assert int(meta[k]["vgpr_spill_count"]) == 0, (k, meta[k])
        assert 2 * int(meta[k]["group_segment_fixed_size"]) <= 160 * 1024, (k, meta[k])
        assert int(meta[k]["vgpr_count"]) + int(meta[k].get("agpr_count", 0)) <= 256, (k, meta[k])      # 256 threads: two blocks per CU
