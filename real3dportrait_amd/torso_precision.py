"""The precision tiers of the torso network's convolutions (r3d_torso_conv_prec / r3d_torso_conv3d_prec of include/r3d_hip.h):

    'f32'     every product on the fp32 matrix instruction: the exact tier, the default.
    'bf16x3'  every staged activation and weight split into three bf16 pieces, x == h + m + l, and six of the nine piece products summed
              in fp32 on the bf16 matrix instruction: fp32-class results (the same test bound as the exact tier), no range fold and no
              per-tensor state, bit-identical across batch sizes, runs and streams.

split_bf16x3 is the host mirror of the kernels' split (tconv::split_bf16x3 in csrc/r3d_torso_conv.h), bit for bit.
"""
import torch

F32, BF16X3 = "f32", "bf16x3"
PRECISIONS = {F32: 0, BF16X3: 1}          # name -> R3D_TORSO_F32 / R3D_TORSO_BF16X3

BF16_MAX = float.fromhex("0x1.fep127")    # 0x7f7f0000, the largest finite bf16


def check_precision(precision, who="precision"):
    """The tier's name, or ValueError."""
    if precision not in PRECISIONS:
        raise ValueError("%s: expected one of %s, got %r" % (who, sorted(PRECISIONS), precision))
    return precision


def split_bf16x3(t):
    """fp32 tensor -> (h, m, l), three bfloat16 tensors with h + m + l == t exactly (summed in fp32 in that order of magnitude):
    h = bf16(clamp(t, -BF16_MAX, BF16_MAX)), m = bf16(t - h), l = bf16(t - h - m), round to nearest even.  The clamp keeps the values
    that would round to infinity finite (fp32 max splits exactly); both subtractions are exact in fp32.  Exact down to |t| ~ 2^-110,
    where l leaves bf16's normal range."""
    if t.dtype != torch.float32:
        raise ValueError("split_bf16x3: expected a float32 tensor, got %s" % t.dtype)
    h = t.clamp(-BF16_MAX, BF16_MAX).to(torch.bfloat16)
    r1 = t - h.float()
    m = r1.to(torch.bfloat16)
    l = (r1 - m.float()).to(torch.bfloat16)
    return h, m, l
