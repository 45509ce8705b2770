"""GPU: each kernel of include/r3d_hip_hubert.h at its edges, against the fp64 restatement of that op (tests/hubert_ref64.py).
The tolerance rule of DESIGN 4.22: the kernel may be at most four times as far from fp64 as the same op in fp32 torch on the CPU is (it
sums in another order; more than that is a bug, not rounding), need never beat one fp32 ulp of max|ref| (1.2e-7), and is never more than
2e-4 of max|ref|.  Batches against single sequences, sub-problems against the larger one and repeats are compared bit for bit."""
import numpy as np
import pytest
import torch

import hubert_common as common
import hubert_ref64 as R64
from real3dportrait_amd import _lib, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL, ULP = 2e-4, 1.2e-7


def unit(seed, shape, stream=0):
    return torch.from_numpy(synth.hash_unitvar(seed, shape, stream))


def check(tag, out, ref, cpu32):
    out = out.cpu()
    assert bool(torch.isfinite(out).all()), tag
    top = float(ref.abs().max())
    e_hip, e_cpu = float((out.double() - ref).abs().max()) / top, float((cpu32.double() - ref).abs().max()) / top
    print("%s: hip %.3g, fp32 torch on the CPU %.3g of max|ref|" % (tag, e_hip, e_cpu))
    assert e_hip <= TOL and e_hip <= max(4.0 * e_cpu, ULP), (tag, e_hip, e_cpu)
    return out


def ln_params(seed, C):
    return unit(seed, (C,), 11) * 0.1, 1.0 + unit(seed, (C,), 12) * 0.1, unit(seed, (C,), 13) * 0.1          # bias, ln weight, ln bias


# ---- r3d_hubert_wave_stats ------------------------------------------------------------------------------------------------------------
def hip_stats(wave):
    stats = torch.full((2,), float("nan"), device=DEV, dtype=torch.float64)
    _lib.call("r3d_hubert_wave_stats", wave, wave.numel(), stats)
    return stats


@pytest.mark.parametrize("n", [1, 400, 1023, 1025, 330123])
def test_wave_stats_against_numpy(n):
    x = common.waveform(90 + n % 7, n).astype(np.float32)
    got = hip_stats(torch.from_numpy(x).to(DEV)).cpu().numpy()
    x64 = x.astype(np.float64)
    want = np.array([x64.mean(), 1.0 / np.sqrt(x64.var() + 1e-7)])
    print("wave_stats n=%d: %s against %s" % (n, got, want))
    assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want))
    assert torch.equal(hip_stats(torch.from_numpy(x).to(DEV)).cpu(), torch.from_numpy(got))


def test_wave_stats_of_a_constant_waveform_are_finite():
    got = hip_stats(torch.full((5000,), 0.25, device=DEV)).cpu().numpy()
    assert np.all(np.isfinite(got)) and got[0] == 0.25 and abs(got[1] - 1.0 / np.sqrt(1e-7)) <= 1e-12 * got[1]


# ---- r3d_hubert_conv0 -------------------------------------------------------------------------------------------------------------------
def conv0_weights(C0, k, seed=5):
    return (unit(seed, (C0, 1, k), 10) * float(np.sqrt(2.0 / k)),) + ln_params(seed, C0)


def hip_conv0(wave_dev, stats, B, offset, sstride, n_chunk, params, stride):
    w, bias, g, b = (t.to(DEV) for t in params)
    C0, _, k = w.shape
    T0 = (n_chunk - k) // stride + 1
    y = torch.full((B, T0, C0), float("nan"), device=DEV)
    _lib.call("r3d_hubert_conv0", wave_dev, stats, B, offset, sstride, n_chunk, w.reshape(C0, k).contiguous(), bias, g, b, 1e-5, C0, k, stride, y)
    return y


@pytest.mark.parametrize("C0", [32, 512])
@pytest.mark.parametrize("n_chunk", [10, 330, 757])
def test_conv0_against_fp64(C0, n_chunk):
    """T0 = 1, one 64-row tile + 1, and a ragged last tile (150 rows, two samples left over); the chunk starts 37 samples into the clip."""
    k, stride, off = 10, 5, 37
    x = torch.from_numpy(common.waveform(91, off + n_chunk + 11).astype(np.float32))
    params = conv0_weights(C0, k)
    dev = x.to(DEV)
    stats = hip_stats(dev)
    out = hip_conv0(dev, stats, 1, off, 0, n_chunk, params, stride)
    mean, rstd = R64.wave_stats(x.double())
    ref = R64.conv_ln_gelu(((x.double() - mean) * rstd)[None, off:off + n_chunk, None], *(p.double() for p in params), 1e-5, stride)
    m32, r32 = R64.wave_stats(x)
    cpu32 = R64.conv_ln_gelu(((x - m32) * r32)[None, off:off + n_chunk, None], *params, 1e-5, stride)
    assert out.shape == ref.shape == (1, (n_chunk - k) // stride + 1, C0)
    check("conv0 C0=%d n=%d" % (C0, n_chunk), out, ref, cpu32)


def test_conv0_batch_of_overlapping_chunks_equals_the_chunks_alone():
    k, stride, n_chunk, step = 10, 5, 3280, 3200
    dev = torch.from_numpy(common.waveform(92, step + n_chunk).astype(np.float32)).to(DEV)
    stats = hip_stats(dev)
    params = conv0_weights(32, k)
    both = hip_conv0(dev, stats, 2, 0, step, n_chunk, params, stride)
    for b in range(2):
        assert torch.equal(both[b], hip_conv0(dev, stats, 1, b * step, 0, n_chunk, params, stride)[0])
    # reading the second chunk from a copy gives what reading it in place gives
    alone = hip_conv0(dev[step:].clone(), stats, 1, 0, 0, n_chunk, params, stride)
    assert torch.equal(both[1], alone[0])
    assert torch.equal(both, hip_conv0(dev, stats, 2, 0, step, n_chunk, params, stride))


# ---- r3d_hubert_conv_ln_gelu --------------------------------------------------------------------------------------------------------------
def conv_weights(Cin, Cout, k, seed=6):
    return (unit(seed, (Cout, Cin, k), 10) * float(np.sqrt(2.0 / (Cin * k))),) + ln_params(seed, Cout)


def hip_conv(x_dev, params, stride):
    w, bias, g, b = (t.to(DEV) for t in params)
    Cout, Cin, k = w.shape
    B, Tin, _ = x_dev.shape
    y = torch.full((B, (Tin - k) // stride + 1, Cout), float("nan"), device=DEV)
    _lib.call("r3d_hubert_conv_ln_gelu", x_dev, w.permute(0, 2, 1).contiguous(), bias, g, b, 1e-5, B, Tin, Cin, Cout, k, stride, y)
    return y


@pytest.mark.parametrize("k,stride,Cin,Cout,Tin", [(3, 2, 32, 32, 3), (3, 2, 32, 32, 67), (3, 2, 512, 512, 68), (2, 2, 32, 32, 2), (2, 2, 512, 512, 67),
                                                    (2, 2, 512, 512, 66), (3, 2, 48, 80, 150), (4, 3, 16, 144, 40), (1, 1, 64, 16, 35)])
def test_conv_ln_gelu_against_fp64(k, stride, Cin, Cout, Tin):
    """(k 3, s 2) and (k 2, s 2) at widths 32 and 512, Tin odd and even, Tout = 1 and one 32-row tile + 1; then unequal widths with five
    column tiles over four waves and a ragged last row tile, and the ends of the accepted kernel range."""
    x = unit(20 + Tin, (1, Tin, Cin), 3)
    params = conv_weights(Cin, Cout, k)
    out = hip_conv(x.to(DEV), params, stride)
    ref = R64.conv_ln_gelu(x.double(), *(p.double() for p in params), 1e-5, stride)
    assert out.shape == ref.shape
    check("conv_ln_gelu k=%d s=%d %d->%d Tin=%d" % (k, stride, Cin, Cout, Tin), out, ref, R64.conv_ln_gelu(x, *params, 1e-5, stride))


@pytest.mark.parametrize("C", [32, 512])
def test_conv_ln_gelu_rows_do_not_depend_on_the_problem(C):
    """B = 2 equals the two alone; output rows 13 .. 69 as a problem of their own (input rows 26 .. 140) equal the same rows of the
    larger one; a repeat is bit-identical."""
    x = unit(31, (2, 150, C), 3).to(DEV)
    params = conv_weights(C, C, 3)
    both = hip_conv(x, params, 2)
    assert both.shape == (2, 74, C)
    for b in range(2):
        assert torch.equal(both[b], hip_conv(x[b:b + 1].contiguous(), params, 2)[0])
    part = hip_conv(x[:1, 26:141].contiguous(), params, 2)
    assert part.shape == (1, 57, C) and torch.equal(part[0], both[0, 13:70])
    assert torch.equal(both, hip_conv(x, params, 2))


# ---- r3d_hubert_pos_conv ------------------------------------------------------------------------------------------------------------------
def pos_weights(C, k, groups, seed=8):
    Ng = C // groups
    return unit(seed, (C, Ng, k), 10) * float(np.sqrt(2.0 / (Ng * k))), unit(seed, (C,), 11) * 0.1


def hip_pos_conv(x_dev, w, bias, groups):
    B, T, C = x_dev.shape
    y = torch.full((B, T, C), float("nan"), device=DEV)
    _lib.call("r3d_hubert_pos_conv", x_dev, w.permute(0, 2, 1).contiguous().to(DEV), bias.to(DEV), B, T, C, w.shape[2], groups, y)
    return y


@pytest.mark.parametrize("C,k,groups", [(128, 16, 4), (1024, 128, 16), (96, 15, 2)])
@pytest.mark.parametrize("T", [1, 37, 130])
def test_pos_conv_against_fp64(C, k, groups, T):
    """The small and the product shape and an odd k at C / groups = 48; T = 1 and 37 (every window clipped at both ends when k = 128) and
    130 (three 64-row tiles, the last with two rows)."""
    x = unit(40 + T, (1, T, C), 3)
    w, bias = pos_weights(C, k, groups)
    out = hip_pos_conv(x.to(DEV), w, bias, groups)
    ref = R64.pos_conv(x.double(), w.double(), bias.double(), groups)
    assert out.shape == ref.shape == (1, T, C)
    check("pos_conv C=%d k=%d g=%d T=%d" % (C, k, groups, T), out, ref, R64.pos_conv(x, w, bias, groups))


@pytest.mark.parametrize("C,k,groups", [(128, 16, 4), (1024, 128, 16)])
def test_pos_conv_batch_equals_the_singles_and_repeats(C, k, groups):
    x = unit(50, (2, 70, C), 3).to(DEV)
    w, bias = pos_weights(C, k, groups)
    both = hip_pos_conv(x, w, bias, groups)
    for b in range(2):
        assert torch.equal(both[b], hip_pos_conv(x[b:b + 1].contiguous(), w, bias, groups)[0])
    assert torch.equal(both, hip_pos_conv(x, w, bias, groups))
